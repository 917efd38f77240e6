// Constants, the level prefix table and HOST argument validation of the fused RPN output kernels (rpn_outputs.hip).  Plain C++ so that
// a host program can walk the table, the index map and the validators without the HIP runtime (tools/rpn_outputs_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"

namespace sdn {

constexpr int RPO_MAX_LEVELS = 8;      // L: the pointers and the prefix table travel by value in the kernel's arguments
constexpr int RPO_MAX_K = 16;          // k: anchors per location; a tile of 6k channels lies in the LDS
constexpr int RPO_TILE = 64;           // pixels of one level a workgroup owns: one wave reads one channel of the tile at once
constexpr int RPO_THREADS = 256;
constexpr int RPO_MAX_BATCH = 65535;   // B: the second axis of the launch grid
constexpr long long RPO_LIMIT = 1ll << 31;   // every element count stays below it: the kernels index with 32-bit integers

// The levels as the kernels see them.  pix[l]: pixels of the levels before l (pix[L] = all); tile[l]: workgroups of the levels before l.
struct RpoTable {
    int L, k, B;
    int anchors;                       // A = k * pix[L]
    int hw[RPO_MAX_LEVELS];
    int pix[RPO_MAX_LEVELS + 1];
    int tile[RPO_MAX_LEVELS + 1];
};

SDN_HD int rpo_tiles(int hw) { return (hw + RPO_TILE - 1) / RPO_TILE; }

// the level that owns workgroup `t` (0 <= t < tile[L])
SDN_HD int rpo_level_of(const RpoTable& T, int t)
{
    int l = 0;
    while (l + 1 < T.L && t >= T.tile[l + 1]) l++;
    return l;
}

// Place of element i of a run of rows of `ch` floats in a tile whose rows are padded to ch + 1 floats
SDN_HD int rpo_padded(int i, int ch) { return i + i / ch; }

// Floats of the LDS tile: logits and probabilities [RPO_TILE][2k + 1] each, boxes [RPO_TILE][4k + 1]
SDN_HD int rpo_lds_floats(int k) { return RPO_TILE * (2 * (2 * k + 1) + (4 * k + 1)); }

// Anchor (y * W + x) * k + a of level l, component j of `comps` (2: classes, 4: boxes), image b: where it lies in the output
// [B, A, comps] and where its source lies in the level's map [B, comps * k, H, W] (pixel = y * W + x)
SDN_HD long long rpo_out_index(const RpoTable& T, int l, int b, int pixel, int a, int j, int comps)
{
    return ((long long)b * T.anchors + (long long)T.k * (T.pix[l] + pixel) + a) * comps + j;
}
SDN_HD long long rpo_map_index(const RpoTable& T, int l, int b, int pixel, int a, int j, int comps)
{
    return ((long long)b * (comps * T.k) + (a * comps + j)) * T.hw[l] + pixel;
}

// 0 with the table filled when (H, W, L, k, B) is a valid problem; otherwise 1 with the reason in msg
inline int rpo_table(const int* H, const int* W, int L, int k, int B, RpoTable* T, char* msg, size_t cap)
{
    if (!T) SDN_FAIL("the table is NULL");
    if (L < 1 || L > RPO_MAX_LEVELS) SDN_FAIL("L %d; 1 to %d levels are supported", L, RPO_MAX_LEVELS);
    if (k < 1 || k > RPO_MAX_K) SDN_FAIL("k %d; 1 to %d anchors per location are supported", k, RPO_MAX_K);
    if (B < 1 || B > RPO_MAX_BATCH) SDN_FAIL("bad sizes: B %d; 1 to %d images are supported", B, RPO_MAX_BATCH);
    if (!H || !W) SDN_FAIL("H or W is NULL (L ints each in host memory)");
    long long pixels = 0, tiles = 0;
    T->L = L;
    T->k = k;
    T->B = B;
    for (int l = 0; l < RPO_MAX_LEVELS; l++) T->hw[l] = 0;
    for (int l = 0; l <= RPO_MAX_LEVELS; l++) T->pix[l] = T->tile[l] = 0;
    for (int l = 0; l < L; l++) {
        if (H[l] < 1 || W[l] < 1) SDN_FAIL("bad sizes: level %d is %d x %d", l, H[l], W[l]);
        const long long hw = (long long)H[l] * W[l];
        if (hw >= RPO_LIMIT) SDN_FAIL("level %d: H * W = %lld must stay below 2^31", l, hw);
        T->hw[l] = (int)hw;
        T->pix[l] = (int)pixels;
        T->tile[l] = (int)tiles;
        pixels += hw;
        tiles += (hw + RPO_TILE - 1) / RPO_TILE;
        // the largest tensor is rpn_bbox, B * A * 4 floats; the box maps together hold as many
        if ((long long)B * 4 * k * pixels >= RPO_LIMIT) SDN_FAIL("B * A * 4 = %lld must stay below 2^31", (long long)B * 4 * k * pixels);
    }
    T->pix[L] = (int)pixels;
    T->tile[L] = (int)tiles;
    for (int l = L + 1; l <= RPO_MAX_LEVELS; l++) {
        T->pix[l] = (int)pixels;
        T->tile[l] = (int)tiles;
    }
    T->anchors = (int)(k * pixels);
    return 0;
}

// L pointers in host memory, each to a map on the device: none NULL, all on 4 bytes
inline int rpo_validate_maps(const void* const* maps, int L, const char* name, char* msg, size_t cap)
{
    if (!maps) SDN_FAIL("%s is NULL (L pointers in host memory)", name);
    for (int l = 0; l < L; l++) {
        if (!maps[l]) SDN_FAIL("%s[%d] is NULL", name, l);
        if (misaligned(maps[l], 4)) SDN_FAIL("%s[%d] must be aligned to 4 bytes", name, l);
    }
    return 0;
}

inline int rpo_validate_fwd(const void* const* class_maps, const void* const* bbox_maps, const int* H, const int* W, int L, int k, int B,
                            const void* logits, const void* probs, const void* bbox, RpoTable* T, char* msg, size_t cap)
{
    if (rpo_table(H, W, L, k, B, T, msg, cap)) return 1;
    if (rpo_validate_maps(class_maps, L, "class_maps", msg, cap) || rpo_validate_maps(bbox_maps, L, "bbox_maps", msg, cap)) return 1;
    if (!logits || !probs || !bbox) SDN_FAIL("rpn_class_logits, rpn_probs or rpn_bbox is NULL");
    if (misaligned(logits, 16) || misaligned(probs, 16) || misaligned(bbox, 16))
        SDN_FAIL("rpn_class_logits, rpn_probs and rpn_bbox must be aligned to 16 bytes");
    return 0;
}

// any of the three gradients may be NULL (it counts as zero); the saved probabilities are read only beside grad_probs
inline int rpo_validate_bwd(const void* grad_logits, const void* grad_probs, const void* grad_bbox, const void* probs, const int* H,
                            const int* W, int L, int k, int B, const void* const* grad_class_maps, const void* const* grad_bbox_maps,
                            RpoTable* T, char* msg, size_t cap)
{
    if (rpo_table(H, W, L, k, B, T, msg, cap)) return 1;
    if (rpo_validate_maps(grad_class_maps, L, "grad_class_maps", msg, cap) || rpo_validate_maps(grad_bbox_maps, L, "grad_bbox_maps", msg, cap))
        return 1;
    if (grad_probs && !probs) SDN_FAIL("rpn_probs is NULL although grad_probs is given");
    if (misaligned(grad_logits, 4) || misaligned(grad_probs, 4) || misaligned(grad_bbox, 4) || misaligned(probs, 4))
        SDN_FAIL("grad_logits, grad_probs, grad_bbox and rpn_probs must be aligned to 4 bytes");
    return 0;
}

}  // namespace sdn
