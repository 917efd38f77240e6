// Sizes, scratch layout and HOST argument validation of the semantic training loss (segm_loss.hip).  Plain C++ so that a host
// program can walk the block arithmetic and the validator without the HIP runtime (tools/segm_loss_check.cpp).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"
#include "segm_tail_check.h"   // SEG_MAX_CLASSES

namespace sdn {

constexpr int SGL_THREADS = 64;    // a workgroup is one wave: its sums need shuffles only, no LDS and no barrier
constexpr int SGL_PIXELS = 256;    // pixels of one item's plane per workgroup: four per lane.  Fixes the scratch size (ops.py mirrors it)
constexpr int SGL_PART_BYTES = 32; // scratch per workgroup: two doubles (sum of -log p[label], main and deepsup head), then four
                                   // ints (acc_sum, pixel_sum, bad, one pad)
static_assert(SGL_PIXELS == 4 * SGL_THREADS, "a lane takes one float4 of pixels, or four strided pixels on the scalar path");

SDN_HD int sgl_chunks(long HW) { return (int)((HW + SGL_PIXELS - 1) / SGL_PIXELS); }   // workgroups per item
SDN_HD long sgl_blocks(int B, long HW) { return (long)B * sgl_chunks(HW); }
SDN_HD size_t sgl_scratch_bytes(int B, long HW) { return (size_t)sgl_blocks(B, HW) * SGL_PART_BYTES; }
// byte offsets of workgroup g's partials in a scratch of n workgroups: the doubles first, so that both parts stay aligned
SDN_HD size_t sgl_sum_at(long g) { return (size_t)g * 16; }
SDN_HD size_t sgl_cnt_at(long n, long g) { return (size_t)n * 16 + (size_t)g * 16; }

// the pixels [first, first + count) of chunk k of a plane of HW pixels; count is 0 beyond the plane
SDN_HD void sgl_chunk_range(long HW, int k, long* first, int* count)
{
    const long p0 = (long)k * SGL_PIXELS;
    long n = HW - p0;
    if (n > SGL_PIXELS) n = SGL_PIXELS;
    if (n < 0) n = 0;
    *first = p0;
    *count = (int)n;
}

// 0 when the sizes of sdn_segm_loss_fwd / _bwd are valid; otherwise 1 with the reason in msg
inline int sgl_validate_sizes(int B, int C, int h, int w, char* msg, size_t cap)
{
    if (C < 1 || C > SEG_MAX_CLASSES) SDN_FAIL("%d classes; 1 to %d are supported", C, SEG_MAX_CLASSES);
    if (B < 1 || h < 1 || w < 1) SDN_FAIL("bad sizes: B %d, h %d, w %d", B, h, w);
    // no product overflows: every factor is below 2^31 and the running product is checked before the next factor
    const long hw = (long)h * (long)w;
    if (hw > INT_MAX || hw * C > INT_MAX || hw * C * B > INT_MAX)
        SDN_FAIL("B * C * h * w = %d * %d * %d * %d must stay below 2^31", B, C, h, w);
    return 0;
}

// the forward call: pointers, sizes and the caller's scratch
inline int sgl_validate_fwd(const void* scores, const void* seg_label, const void* scratch, size_t scratch_bytes, const void* lse,
                            const void* out, const void* counts, int B, int C, int h, int w, char* msg, size_t cap)
{
    if (!scores) SDN_FAIL("scores is NULL");
    if (!seg_label) SDN_FAIL("seg_label is NULL");
    if (!scratch || !lse || !out || !counts) SDN_FAIL("scratch, lse, out or counts is NULL");
    if (sgl_validate_sizes(B, C, h, w, msg, cap)) return 1;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(counts) & 7) || (reinterpret_cast<uintptr_t>(seg_label) & 7))
        SDN_FAIL("scratch, counts and seg_label must be aligned to 8 bytes");
    const size_t need = sgl_scratch_bytes(B, (long)h * w);
    if (scratch_bytes < need) SDN_FAIL("scratch of %zu bytes; %zu are needed (32 per %d pixels of an item)", scratch_bytes, need, SGL_PIXELS);
    return 0;
}

// the backward call
inline int sgl_validate_bwd(const void* scores, const void* scores_deepsup, const void* seg_label, const void* lse, const void* counts,
                            const void* grad_out, const void* grad_scores, const void* grad_deepsup, int B, int C, int h, int w, char* msg,
                            size_t cap)
{
    if (!seg_label) SDN_FAIL("seg_label is NULL");
    if (!lse || !counts || !grad_out) SDN_FAIL("lse, counts or grad_out is NULL");
    if (!grad_scores && !grad_deepsup) SDN_FAIL("no gradient asked for");
    if (grad_scores && !scores) SDN_FAIL("grad_scores without scores");
    if (grad_deepsup && !scores_deepsup) SDN_FAIL("grad_scores_deepsup without scores_deepsup");
    if (sgl_validate_sizes(B, C, h, w, msg, cap)) return 1;
    if ((reinterpret_cast<uintptr_t>(counts) & 7) || (reinterpret_cast<uintptr_t>(seg_label) & 7))
        SDN_FAIL("counts and seg_label must be aligned to 8 bytes");
    return 0;
}

}  // namespace sdn
