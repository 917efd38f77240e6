// The pair test and the pair-mask block of the greedy NMS, shared by raster_boxes.hip (sdn_nms) and proposal_layer.hip
// (sdn_proposal_layer); detection_layer.hip adds the class test to the pair test.  All are built without FMA contraction, so all
// produce the same bits.  nms_scan_words is the one-wave greedy scan over such a mask that stops at a limit, shared by
// proposal_layer.hip (k_prop_scan) and detection_layer.hip (k_det_scan).
#pragma once

#include <hip/hip_runtime.h>

#include "prop_device.h"

namespace sdn {

// nms.c:51-58 with box i's corners first.  IoU is symmetric in (x, y), so the caller's column order does not matter.
__device__ __forceinline__ bool suppresses(const float4 bi, const float ai, const float4 bj, const float aj, const float thresh,
                                           const int strict)
{
    const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y);
    const float xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
    const float w = fmaxf(0.0f, xx2 - xx1 + 1.0f), h = fmaxf(0.0f, yy2 - yy1 + 1.0f);
    const float inter = w * h;
    const float ovr = inter / (ai + aj - inter);
    return strict ? ovr > thresh : ovr >= thresh;  // nms_kernel.cu:66 compares with `>`, cpu_nms (nms.c:59) with `>=`
}

// One wave's 64 x 64 block of the pair mask (the body of k_nms_mask): block (blockIdx.y, blockIdx.x) of the (row box i, column box j)
// pairs of the score-sorted boxes, lane = row box.  cb / ca: 64 entries of LDS each.  boxes [n,4], areas [n]: already in descending
// score order.  mask [n, nb] u64, nb = ceil(n / 64).
__device__ __forceinline__ void nms_mask_block(const float4* __restrict__ boxes, const float* __restrict__ areas, int n, float thresh,
                                               unsigned long long* __restrict__ mask, int nb, int strict, float4* cb, float* ca)
{
    const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64, lane = threadIdx.x;
    if (col0 + 63 <= row0 && blockIdx.x != blockIdx.y) {  // every column precedes every row: nothing to suppress
        if (row0 + lane < n) mask[(size_t)(row0 + lane) * nb + blockIdx.x] = 0ull;
        return;
    }
    if (col0 + lane < n) {
        cb[lane] = boxes[col0 + lane];
        ca[lane] = areas[col0 + lane];
    }
    __syncthreads();
    const int i = row0 + lane;
    if (i >= n) return;
    const float4 bi = boxes[i];
    const float ai = areas[i];
    const int cols = min(64, n - col0);
    unsigned long long t = 0ull;
    for (int c = 0; c < cols; c++) {
        const int j = col0 + c;
        if (j <= i) continue;
        const bool s = suppresses(bi, ai, cb[c], ca[c], thresh, strict);
        if (s) t |= 1ull << c;
    }
    mask[(size_t)i * nb + blockIdx.x] = t;
}

constexpr int NMS_SCAN_ROWS = 16;   // mask rows one batch of the scan fetches before it waits: a word of object-like boxes keeps about ten
// One batch of row words as one register value.  Plain arrays here would be turned into such values by the compiler, but inside a
// device function it does that before inlining and within a register budget that knows nothing of the kernel's 64 lanes: one of the
// scan's two arrays fits, the other is split into scalars whose zeroes cost a taken branch per row (profiles/mrcnn_shared_helpers.md).
typedef unsigned long long nms_scan_rows_t __attribute__((ext_vector_type(NMS_SCAN_ROWS)));

// ONE wave walks the first M rows of mask [., nb] word by word (64 rows; prop_words(M) <= min(nb, 128) words): the decisions inside a
// word come from the word's diagonal mask block held in registers, the rows of the word's kept places are then ORed into the running
// "removed" bitmap with independent loads.  It stops once `limit` rows are kept.  remv: at least prop_words(M) words of LDS; s_keep:
// at least `limit` ints of LDS, the kept places in order on return (behind a barrier).  Returns how many are kept, the same in
// every lane.
__device__ __forceinline__ int nms_scan_words(const unsigned long long* mask, int nb, int M, int limit, unsigned long long* remv, int* s_keep)
{
    const int lane = threadIdx.x;
    const int nbm = prop_words(M);   // <= nb
    __builtin_assume(nb > 0);        // both callers pass prop_words(n >= 1): the row offsets need no sign extension of nb
    for (int w = lane; w < nbm; w += 64) remv[w] = 0ull;
    __syncthreads();
    int kept = 0;
    unsigned long long diag = lane < M ? mask[(size_t)lane * nb] : 0ull;   // word 0 of the first 64 rows
    for (int blk = 0; blk < nbm && kept < limit; blk++) {
        const int base = blk * 64, cnt = min(64, M - base);
        unsigned long long alive = ~prop_uniform64(remv[blk]);
        if (cnt < 64) alive &= (1ull << cnt) - 1ull;
        unsigned long long kept_bits = 0ull;
        const int kept_before = kept;
        while (alive) {   // uniform: the lowest place still alive is kept and removes what it suppresses inside the word
            const int b = __ffsll((long long)alive) - 1;
            kept_bits |= 1ull << b;
            alive &= ~(prop_lane64(diag, b) | (1ull << b));
            if (++kept == limit) break;
        }
        if ((kept_bits >> lane) & 1ull) s_keep[kept_before + __popcll(kept_bits & ((1ull << lane) - 1ull))] = base + lane;
        // the next word's diagonal block does not depend on this word's decisions: it is fetched with the rows below, one wait for all
        unsigned long long diag_next = 0ull;
        if (blk + 1 < nbm && base + 64 + lane < M) diag_next = mask[(size_t)(base + 64 + lane) * nb + blk + 1];
        if (kept < limit) {
            // OR the rows of this word's kept places into the words behind it: lane = word, NMS_SCAN_ROWS rows' loads in flight at a time
            const int j0 = blk + 1 + lane, j1 = j0 + 64;   // nbm <= 128: two words per lane reach the end
            unsigned long long acc0 = 0ull, acc1 = 0ull, kb = kept_bits;
            while (kb) {
                nms_scan_rows_t t0, t1;
#pragma unroll
                for (int u = 0; u < NMS_SCAN_ROWS; u++) {
                    t0[u] = t1[u] = 0ull;
                    if (kb) {
                        const unsigned long long* row = mask + (size_t)(base + __ffsll((long long)kb) - 1) * nb;
                        kb &= kb - 1ull;
                        if (j0 < nbm) t0[u] = row[j0];
                        if (j1 < nbm) t1[u] = row[j1];
                    }
                }
#pragma unroll
                for (int u = 0; u < NMS_SCAN_ROWS; u++) {
                    acc0 |= t0[u];
                    acc1 |= t1[u];
                }
            }
            if (j0 < nbm) remv[j0] |= acc0;
            if (j1 < nbm) remv[j1] |= acc1;
        }
        __syncthreads();
        diag = diag_next;
    }
    __syncthreads();
    return kept;
}

}  // namespace sdn
