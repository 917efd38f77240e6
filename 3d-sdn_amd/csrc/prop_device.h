// Device helpers shared by proposal_layer.hip and detection_layer.hip: torch.clamp's form of a clamp and the wave-uniform 64-bit
// reads of the NMS scans.  Moved here unchanged from proposal_layer.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace sdn {

// torch.clamp: NaN stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float prop_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

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
