// The pair test and the pair-mask block of the greedy NMS, shared by raster_boxes.hip (sdn_nms) and proposal_layer.hip
// (sdn_proposal_layer).  Both files are built without FMA contraction, so both produce the same bits.
#pragma once

#include <hip/hip_runtime.h>

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

}  // namespace sdn
