// Sizes, the gradient buffer's layout, the level rule and HOST argument validation of the pyramid RoIAlign (pyramid_roi_align.hip).
// Plain C++ so that a host program can walk the layout, the level rule's rounding and clamp and the validators without the HIP
// runtime (tools/pyramid_roi_align_check.cpp).
#pragma once

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"

namespace sdn {

constexpr int PRA_LEVELS = 4;         // P2 .. P5
constexpr int PRA_THREADS = 256;
constexpr int PRA_CHANNELS = 64;      // channels of one workgroup: a workgroup owns (box, channel chunk)
constexpr int PRA_MAX_POOL = 32;      // the sample table of pool x pool entries must fit the LDS: 32 * 32 * 28 bytes = 28 KiB
constexpr int PRA_SAMPLE_BYTES = 28;  // four tap offsets (int), two lerp weights (float), an inside flag (int)
constexpr int PRA_ALIGN_FLOATS = 4;   // every level's gradient range starts on 16 bytes: the zero fill stores 16 bytes at a time

// the ordered backward (k_pra_box_records, k_pra_bwd_ordered): a workgroup owns (level, tile of PRA_TILE x PRA_TILE pixels, channel chunk)
constexpr int PRA_TILE = 8;           // 64 pixels, one per lane of a wave; the four waves share the chunk's channels: 16 fp64 sums per lane
constexpr int PRA_RECORD_BYTES = 32;  // workspace per box: level (or -1: no sample inside), window r0, r1, q0, q1, three unused ints
constexpr int PRA_ORD_BATCH = 8;      // boxes whose per-axis tables stand in the LDS at once

SDN_HD int pra_chunks(int C) { return (C + PRA_CHANNELS - 1) / PRA_CHANNELS; }
SDN_HD int pra_tiles(int extent) { return (extent - 1) / PRA_TILE + 1; }   // extent >= 1; no overflow at INT_MAX
SDN_HD size_t pra_table_bytes(int pool) { return (size_t)pool * (size_t)pool * PRA_SAMPLE_BYTES; }

// model.py:456-457 on the value of :455: round half to even (torch.round, rintf in the default rounding mode), then clamp to [2, 5].
// A non-finite value -- a box of area <= 0 gives log(0) = -inf or sqrt(< 0) = NaN -- gives level 2: the reference's .int() of such a
// float is INT_MIN on x86 (cvttss2si's "integer indefinite"), which the clamp lifts to 2, for +inf and NaN as for -inf.
SDN_HD int pra_level_of(float v)
{
    if (!(v - v == 0.0f)) return 2;   // NaN, +inf, -inf
    const float r = rintf(v);
    return r < 2.0f ? 2 : r > 5.0f ? 5 : (int)r;
}

// model.py:445-455 with log2 of :95-100, operation for operation in fp32; image_area = float(image_shape[0] * image_shape[1])
SDN_HD float pra_level_value(float y1, float x1, float y2, float x2, float image_area)
{
    const float h = y2 - y1, w = x2 - x1;
    return 4.0f + logf(sqrtf(h * w) / (224.0f / sqrtf(image_area))) / logf(2.0f);
}

// 0 when the sizes of sdn_pyramid_roi_align_fwd / _bwd / _grad_floats are valid; otherwise 1 with the reason in msg
inline int pra_validate_maps(int C, const int* H, const int* W, char* msg, size_t cap)
{
    if (!H || !W) SDN_FAIL("H or W is NULL");
    if (C <= 0) SDN_FAIL("bad sizes: C %d", C);
    for (int l = 0; l < PRA_LEVELS; l++) {
        if (H[l] <= 0 || W[l] <= 0) SDN_FAIL("bad sizes: level P%d is %d x %d", l + 2, H[l], W[l]);
        // no product overflows: every factor is below 2^31 and the running product is checked before the next factor
        const long long hw = (long long)H[l] * (long long)W[l];
        if (hw > INT_MAX || hw * C > INT_MAX) SDN_FAIL("C * H * W = %d * %d * %d of level P%d must stay below 2^31", C, H[l], W[l], l + 2);
    }
    return 0;
}

// the gradients of the four maps in one allocation: level l is [C, H_l, W_l] at float offsets[l], every range starting on 16 bytes
inline int pra_grad_layout(int C, const int* H, const int* W, size_t offsets[PRA_LEVELS], size_t* total, char* msg, size_t cap)
{
    if (pra_validate_maps(C, H, W, msg, cap)) return 1;
    if (!offsets || !total) SDN_FAIL("offsets or total is NULL");
    size_t at = 0;
    for (int l = 0; l < PRA_LEVELS; l++) {
        offsets[l] = at;
        const size_t n = (size_t)C * (size_t)H[l] * (size_t)W[l];   // < 2^31 each: four of them cannot overflow
        at += (n + PRA_ALIGN_FLOATS - 1) / PRA_ALIGN_FLOATS * PRA_ALIGN_FLOATS;
    }
    *total = at;
    return 0;
}

inline int pra_validate_sizes(int R, int C, const int* H, const int* W, int pool, float image_area, char* msg, size_t cap)
{
    if (R < 0) SDN_FAIL("bad sizes: R %d", R);
    if (pra_validate_maps(C, H, W, msg, cap)) return 1;
    if (pool <= 0 || pool > PRA_MAX_POOL) SDN_FAIL("pool %d; 1 to %d are supported (the sample table lives in the LDS)", pool, PRA_MAX_POOL);
    if (!(image_area - image_area == 0.0f) || image_area <= 0.0f) SDN_FAIL("image_area %g must be finite and positive", (double)image_area);
    const long long per_box = (long long)C * pool * pool;   // C < 2^31, pool <= 32
    if (per_box > INT_MAX) SDN_FAIL("C * pool * pool = %d * %d * %d must stay below 2^31", C, pool, pool);
    if ((long long)R * pra_chunks(C) > INT_MAX) SDN_FAIL("R * ceil(C / %d) = %d * %d workgroups must stay below 2^31", PRA_CHANNELS, R, pra_chunks(C));
    return 0;
}

inline int pra_validate_fwd(const void* boxes, const void* const* maps, const int* H, const int* W, int R, int C, int pool, float image_area,
                            const void* pooled, const void* levels, char* msg, size_t cap)
{
    if (pra_validate_sizes(R, C, H, W, pool, image_area, msg, cap)) return 1;
    if (R == 0) return 0;   // nothing is read or written
    if (!boxes || !pooled || !levels) SDN_FAIL("boxes, pooled or levels is NULL with R > 0");
    if (!maps) SDN_FAIL("maps is NULL with R > 0");
    for (int l = 0; l < PRA_LEVELS; l++) {
        if (!maps[l]) SDN_FAIL("the map of level P%d is NULL with R > 0", l + 2);
        if (misaligned(maps[l], 4)) SDN_FAIL("the maps must be aligned to 4 bytes");
    }
    if (misaligned(boxes, 4) || misaligned(pooled, 4) || misaligned(levels, 4)) SDN_FAIL("boxes, pooled and levels must be aligned to 4 bytes");
    return 0;
}

inline int pra_validate_bwd(const void* grads, const void* boxes, const int* H, const int* W, int R, int C, int pool, float image_area,
                            const void* grad_maps, char* msg, size_t cap)
{
    if (pra_validate_sizes(R, C, H, W, pool, image_area, msg, cap)) return 1;
    if (!grad_maps) SDN_FAIL("grad_maps is NULL");   // zero-filled for R = 0 too
    if (misaligned(grad_maps, 16)) SDN_FAIL("grad_maps must be aligned to 16 bytes");
    if (R == 0) return 0;
    if (!grads || !boxes) SDN_FAIL("grads or boxes is NULL with R > 0");
    if (misaligned(grads, 4) || misaligned(boxes, 4)) SDN_FAIL("grads and boxes must be aligned to 4 bytes");
    return 0;
}

// ---- the ordered backward -----------------------------------------------------------------------------------------------------------
// bytes of the workspace of sdn_pyramid_roi_align_bwd_ordered: one record per box
inline int pra_ordered_workspace_bytes(int R, size_t* bytes, char* msg, size_t cap)
{
    if (R < 0) SDN_FAIL("bad sizes: R %d", R);
    if (!bytes) SDN_FAIL("bytes is NULL");
    *bytes = (size_t)R * PRA_RECORD_BYTES;
    return 0;
}

// workgroups of k_pra_bwd_ordered: every tile of every level, once per channel chunk.  Valid sizes only (pra_validate_maps): a level has
// at most 2^31 / 8 tiles (H * W < 2^31), so four levels times the chunks fit a long long with room to spare.
inline long long pra_ordered_blocks(int C, const int* H, const int* W)
{
    long long tiles = 0;
    for (int l = 0; l < PRA_LEVELS; l++) tiles += (long long)pra_tiles(H[l]) * pra_tiles(W[l]);
    return tiles * pra_chunks(C);
}

inline int pra_validate_bwd_ordered(const void* grads, const void* boxes, const int* H, const int* W, int R, int C, int pool, float image_area,
                                    const void* grad_maps, const void* workspace, size_t workspace_bytes, char* msg, size_t cap)
{
    if (pra_validate_bwd(grads, boxes, H, W, R, C, pool, image_area, grad_maps, msg, cap)) return 1;
    // sizes that passed above give at most 2^30 (four levels of 1 x (2^31 - 1)); the test stands so that another PRA_TILE or
    // PRA_CHANNELS cannot overflow the grid unnoticed
    const long long blocks = pra_ordered_blocks(C, H, W);
    if (blocks > INT_MAX) SDN_FAIL("%lld tiles of %d x %d pixels times channel chunks must stay below 2^31 workgroups", blocks, PRA_TILE, PRA_TILE);
    if (R == 0) return 0;   // no record is written or read
    if (!workspace) SDN_FAIL("workspace is NULL with R > 0");
    if (misaligned(workspace, 16)) SDN_FAIL("workspace must be aligned to 16 bytes");
    const size_t need = (size_t)R * PRA_RECORD_BYTES;
    if (workspace_bytes < need) SDN_FAIL("workspace of %zu bytes; %zu are needed for %d boxes", workspace_bytes, need, R);
    return 0;
}

}  // namespace sdn
