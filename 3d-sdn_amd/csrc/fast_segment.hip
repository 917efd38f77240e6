// Instance-wise average pooling of the textural Encoder (textural/models/networks.py:310-325): every pixel of an
// instance is replaced by the instance's mean feature.  The reference walks np.unique(inst) on the host and masks per
// (instance, channel); torch's index_add_ does it on the device but serialises on the ~10 instance rows (0.7 ms per
// call at 384 x 1248).  Here the sums are REPEATABLE: the same input gives the same bits on every launch (the appearance
// code of an instance is such a mean; an edit session and a second encoding of the frame must agree, textural/edit.py).
//   k_segment_partial  one wave per (pixel chunk, channel, image): per step the wave takes each distinct id among its
//                      lanes in turn, sums that id's lanes with a fixed butterfly and lane 0 adds the sum to the id's row
//                      of an LDS table -- one writer, program order, no atomics (segments are spatially coherent: one to
//                      three ids per step).  The chunk's table goes to scratch: the head of the (image, channel) plane of
//                      `out`, which nobody reads before k_segment_bcast overwrites it.
//   k_segment_combine  sums[c, k] = the chunk tables added in a fixed order.
//   k_segment_bcast    divides and broadcasts.
// Pixel counts are sums of exact integers in fp32 (order-free below 2^24 pixels) and keep their atomics.  Tables that do
// not fit (K > 4096 or K > HW) take k_segment_sum, the float-atomic kernel of r01-r06, whose sums depend on arrival order.
// The backward pass is the same operator applied to the incoming gradient (d/dx of mean-broadcast = mean-broadcast of the
// gradient).  HBM-bound: 2 reads + 1 write of the [N, C, H, W] map.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "sdn_common.h"

namespace sdn {

constexpr int SEG_LDS = 4096;  // table rows kept in LDS; larger id counts go straight to global atomics

// x [N, C, HW] (NCHW), seg [N, HW] dense ids in [0, K): sums [C, K] += x, counts [K] += 1 (from channel 0's blocks)
__global__ __launch_bounds__(256) void k_segment_sum(const float* __restrict__ x, const int* __restrict__ seg,
                                                     float* __restrict__ sums, float* __restrict__ counts, int C, int HW,
                                                     int K, int chunk)
{
    __shared__ float tab[SEG_LDS];
    __shared__ float cnt[SEG_LDS];
    const int n = blockIdx.z, c = blockIdx.y;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    const bool use_lds = K <= SEG_LDS;
    const bool count = c == 0;
    if (use_lds) {
        for (int k = threadIdx.x; k < K; k += 256) {
            tab[k] = 0.f;
            cnt[k] = 0.f;
        }
        __syncthreads();
    }
    const float* xp = x + ((size_t)n * C + c) * HW;
    const int* sp = seg + (size_t)n * HW;
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        const int k = sp[p];
        const float v = xp[p];
        if (use_lds) {
            atomicAdd(&tab[k], v);
            if (count) atomicAdd(&cnt[k], 1.f);
        } else {
            unsafeAtomicAdd(sums + (size_t)c * K + k, v);
            if (count) unsafeAtomicAdd(counts + k, 1.f);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += 256) {
            if (count && cnt[k] != 0.f) unsafeAtomicAdd(counts + k, cnt[k]);
            if (tab[k] != 0.f) unsafeAtomicAdd(sums + (size_t)c * K + k, tab[k]);
        }
    }
}

constexpr int SEG_STEP = 4;   // pixels per lane and step: four loads in flight

// x [N, C, HW], seg [N, HW] ids in [0, K), K <= SEG_LDS.  Block (chunk i, c, n), 64 threads: part[(n C + c) HW + i K + k] =
// sum of x over the chunk's pixels of id k, in a fixed order; counts [K] += pixels (from channel 0's blocks).
__global__ __launch_bounds__(64) void k_segment_partial(const float* __restrict__ x, const int* __restrict__ seg,
                                                        float* __restrict__ part, float* __restrict__ counts, int C, int HW,
                                                        int K, int chunk)
{
    extern __shared__ __attribute__((aligned(16))) float s_tab[];   // [K] sums, then [K] counts (channel 0 only)
    const int n = blockIdx.z, c = blockIdx.y, lane = threadIdx.x;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    const bool count = c == 0;
    float* s_cnt = s_tab + K;
    for (int k = lane; k < K; k += 64) {
        s_tab[k] = 0.f;
        if (count) s_cnt[k] = 0.f;
    }
    __syncthreads();
    const float* xp = x + ((size_t)n * C + c) * HW;
    const int* sp = seg + (size_t)n * HW;
    for (int q = p0; q < p1; q += 64 * SEG_STEP) {
        int kv[SEG_STEP];
        float vv[SEG_STEP];
#pragma unroll
        for (int j = 0; j < SEG_STEP; j++) {
            const int p = q + j * 64 + lane;
            const bool in = p < p1;
            kv[j] = in ? sp[p] : -1;
            vv[j] = in ? xp[p] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < SEG_STEP; j++) {
            unsigned long long todo = __ballot(kv[j] >= 0);
            while (todo) {   // wave-uniform: one turn per distinct id among the lanes
                const int kk = __shfl(kv[j], __ffsll((long long)todo) - 1, 64);
                const bool mine = kv[j] == kk;
                const unsigned long long match = __ballot(mine);
                const float s = wave_sum(mine ? vv[j] : 0.f);
                if (lane == 0) {
                    s_tab[kk] += s;
                    if (count) s_cnt[kk] += (float)__popcll(match);
                }
                todo &= ~match;
            }
        }
    }
    __syncthreads();
    float* dst = part + ((size_t)n * C + c) * HW + (size_t)blockIdx.x * K;
    for (int k = lane; k < K; k += 64) {
        dst[k] = s_tab[k];
        if (count && s_cnt[k] != 0.f) unsafeAtomicAdd(counts + k, s_cnt[k]);   // exact integers: any order, same sum
    }
}

constexpr int SEG_GROUPS = 16;

// sums[c, k] = the N * chunks chunk tables of channel c added in a fixed order: group g of 16 takes chunks g, g + 16, ...
// of image 0, then of image 1, ... in turn, thread (k, 0) then adds the 16 group sums in turn.  Block (k tile of 64, c), threads (64, 16).
__global__ __launch_bounds__(64 * SEG_GROUPS) void k_segment_combine(const float* __restrict__ part, float* __restrict__ sums,
                                                                     int N, int C, int HW, int K, int chunks)
{
    __shared__ float s_g[SEG_GROUPS][64];
    const int k = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y, g = threadIdx.y;
    float s = 0.f;
    if (k < K) {
        for (int n = 0; n < N; n++) {
            const float* pl = part + ((size_t)n * C + c) * HW + k;
#pragma unroll 4
            for (int i = g; i < chunks; i += SEG_GROUPS) s += pl[(size_t)i * K];
        }
    }
    s_g[g][threadIdx.x] = s;
    __syncthreads();
    if (g == 0 && k < K) {
        float t = 0.f;
        for (int j = 0; j < SEG_GROUPS; j++) t += s_g[j][threadIdx.x];
        sums[(size_t)c * K + k] = t;
    }
}

// out[n, c, p] = sums[c, seg[n, p]] / counts[seg[n, p]]
__global__ __launch_bounds__(256) void k_segment_bcast(const float* __restrict__ sums, const float* __restrict__ counts,
                                                       const int* __restrict__ seg, float* __restrict__ out, int C,
                                                       int HW, int K)
{
    const int n = blockIdx.z, c = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int k = seg[(size_t)n * HW + p];
    out[((size_t)n * C + c) * HW + p] = sums[(size_t)c * K + k] / counts[k];
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_segment_mean(const float* x, const int32_t* seg, int N, int C, int HW, int K, float* sums, float* counts,
                             float* out, sdnStream stream)
{
    if (!x || !seg || !sums || !counts || !out) return fail(SDN_EINVAL, "sdn_segment_mean: null pointer");
    if (N < 1 || C < 1 || HW < 1 || K < 1) return fail(SDN_EINVAL, "sdn_segment_mean: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const bool ordered = K <= SEG_LDS && K <= HW;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)K * sizeof(float), st);
    if (e == hipSuccess && !ordered) e = hipMemsetAsync(sums, 0, (size_t)C * K * sizeof(float), st);   // k_segment_combine writes every entry
    if (e != hipSuccess) return fail(SDN_ELAUNCH, "sdn_segment_mean: memset: %s", hipGetErrorString(e));
    if (ordered) {
        // repeatable sums.  ~4096 one-wave blocks, at least 1024 pixels each, and the chunk tables of a plane fit the plane
        if (x == out) return fail(SDN_EINVAL, "sdn_segment_mean: out is scratch for the partial sums and must not alias x");
        int chunks = 4096 / (N * C);
        if (chunks > HW / K) chunks = HW / K;
        if (chunks < 1) chunks = 1;
        int chunk = (HW + chunks - 1) / chunks;
        if (chunk < 1024) chunk = 1024;
        chunks = (HW + chunk - 1) / chunk;
        hipLaunchKernelGGL(k_segment_partial, dim3((unsigned)chunks, (unsigned)C, (unsigned)N), dim3(64),
                           2 * (size_t)K * sizeof(float), st, x, seg, out, counts, C, HW, K, chunk);
        hipLaunchKernelGGL(k_segment_combine, dim3((unsigned)((K + 63) / 64), (unsigned)C), dim3(64, SEG_GROUPS), 0, st, out, sums, N, C,
                           HW, K, chunks);
    } else {
        // ~2048 blocks in total, at least 4096 pixels each (one LDS table flush per block)
        int chunks = 2048 / (N * C);
        if (chunks < 1) chunks = 1;
        int chunk = (HW + chunks - 1) / chunks;
        if (chunk < 4096) chunk = 4096;
        chunks = (HW + chunk - 1) / chunk;
        hipLaunchKernelGGL(k_segment_sum, dim3((unsigned)chunks, (unsigned)C, (unsigned)N), dim3(256), 0, st, x, seg, sums, counts,
                           C, HW, K, chunk);
    }
    hipLaunchKernelGGL(k_segment_bcast, dim3((unsigned)((HW + 255) / 256), (unsigned)C, (unsigned)N), dim3(256), 0, st, sums,
                       counts, seg, out, C, HW, K);
    return check_launch("k_segment_mean");
}
