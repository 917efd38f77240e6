// Device helpers shared by the kernels of libsdn_hip.so: the 64-lane wave reductions, the 8-bit clip, the packed colour of a scene pixel, the partial quad store and
// the NaN-first min / max.  HIP only: the *_check.h headers are plain C++ and never include this file (check_common.h is theirs).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sdn {

// ---- wave reductions -------------------------------------------------------------------------------------------------------
// Every lane gets the result.  One xor butterfly over the offsets 32, 16, .., 1: a floating-point sum adds in that order and
// gives the same bits in every lane and on every run.
// (Still written out in place, on purpose: the sums of transform.hip, fast_ffd.hip and fast_loss.hip and the loops of segm_loss.hip
// that reduce several values at once.  Calling the helpers there gave the same arithmetic but other register names and another
// instruction order in those kernels' listings; the change that introduced this header left every listing as it was.)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_imin(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_imax(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// The floating-point min / max differ in what a NaN does, so each rule has its own name.
// fminf / fmaxf: a NaN loses against a number.
__device__ __forceinline__ float wave_fminf(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_fmaxf(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// t > v ? t : v: a lane keeps what it holds unless the other lane's value compares greater, so a NaN neither spreads nor yields.
__device__ __forceinline__ double wave_max_greater(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// the lanes below this one: the sum of their v; total: the wave's
__device__ __forceinline__ int wave_exclusive_sum(int v, int lane, int& total)
{
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        incl += lane >= o ? t : 0;
    }
    total = __shfl(incl, 63, 64);
    return incl - v;
}

// ---- scalars ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the packed colour r | g << 8 | b << 16 of the three bytes at s (a pixel of a scene image, a row of a code table)
__device__ __forceinline__ int code24(const uint8_t* s) { return (int)s[0] | ((int)s[1] << 8) | ((int)s[2] << 16); }

// torch.max / torch.min of two tensors, np.maximum / np.minimum / np.amax: a NaN on either side is the result
template <typename T>
__device__ __forceinline__ T nan_first_max(T a, T b) { return (a > b || a != a) ? a : b; }
template <typename T>
__device__ __forceinline__ T nan_first_min(T a, T b) { return (a < b || a != a) ? a : b; }

// ---- partial quad store ----------------------------------------------------------------------------------------------------
template <typename T> struct Quad;
template <> struct Quad<float> { using type = float4; };
template <> struct Quad<uint32_t> { using type = uint4; };

// `vals` of the elements [e0, e0 + 4) of an array whose element 0 is 16-byte aligned; only [lo, hi) is written.
template <typename T>
__device__ __forceinline__ void store_quad(T* base, long e0, long lo, long hi, const T vals[4])
{
    if (e0 >= lo && e0 + 4 <= hi) {
        *reinterpret_cast<typename Quad<T>::type*>(base + e0) = typename Quad<T>::type{vals[0], vals[1], vals[2], vals[3]};
    } else {
        for (int j = 0; j < 4; j++)
            if (e0 + j >= lo && e0 + j < hi) base[e0 + j] = vals[j];
    }
}

}  // namespace sdn
