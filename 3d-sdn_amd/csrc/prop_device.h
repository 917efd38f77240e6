// Device helpers shared by proposal_layer.hip, detection_layer.hip and detection_targets.hip: torch.clamp's form of a clamp, the
// bitonic sort of 64-bit keys in LDS (prop_sort_keys, the one device caller of prop_bitonic_pair), apply_box_deltas in fp32
// (prop_apply_deltas) and the wave-uniform 64-bit reads of the NMS scan (nms_mask.h: nms_scan_words).  Every file that includes this
// is built without FMA contraction.
#pragma once

#include <hip/hip_runtime.h>

#include "proposal_layer_check.h"

namespace sdn {

// torch.clamp: NaN stays NaN (the float min / max intrinsics would drop it)
__device__ __forceinline__ float prop_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup of `threads` lanes sorts the n = 2^m keys of s (LDS), best first: torch.sort(descending=True, stable=True) where the
// keys are unique.  The caller fills s and passes a barrier before the call; every (k, j) step ends in a barrier, so s is sorted for
// every lane on return.  n == 1 has no step and passes no barrier.
__device__ __forceinline__ void prop_sort_keys(uint64_t* s, int n, int tid, int threads)
{
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n / 2; t += threads) {
                int i, l;
                bool descending;
                prop_bitonic_pair(t, j, k, &i, &l, &descending);
                const uint64_t a = s[i], b = s[l];
                if (descending ? a < b : a > b) {
                    s[i] = b;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// apply_box_deltas of the reference's geometric/maskrcnn/model.py:313-326, operation by operation in fp32: box (ay1, ax1, ay2, ax2),
// deltas (d0 .. d3) already multiplied by std_dev.  Returns (y1, x1, y2, x2).  expf is the only operation that can differ from the
// reference's CPU run.
__device__ __forceinline__ float4 prop_apply_deltas(float ay1, float ax1, float ay2, float ax2, float d0, float d1, float d2, float d3)
{
    float h = ay2 - ay1, w = ax2 - ax1;
    float cy = ay1 + 0.5f * h, cx = ax1 + 0.5f * w;
    cy = cy + d0 * h;
    cx = cx + d1 * w;
    h = h * expf(d2);
    w = w * expf(d3);
    const float y1 = cy - 0.5f * h, x1 = cx - 0.5f * w;
    const float y2 = y1 + h, x2 = x1 + w;
    return make_float4(y1, x1, y2, x2);
}

__device__ __forceinline__ unsigned long long prop_uniform64(unsigned long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long prop_lane64(unsigned long long v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

}  // namespace sdn
