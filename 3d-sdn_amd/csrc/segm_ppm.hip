// The pyramid pooling module of the semantic decoders PPMBilinear / PPMBilinearDeepsup (semantic/models.py:336-346, 387-397) around
// the caller's branch modules.  The reference runs four AdaptiveAvgPool2d passes over conv5, the branches' 1 x 1 conv / BN / ReLU on
// at most 36 positions each, four bilinear upsamples back to conv5's size and a torch.cat of five tensors: nine full-tensor launches
// forward, about twice that backward, conv5 read four times and copied once, every branch map written and read again.  Here:
//   forward   k_ppm_pool      a workgroup per (b, c) plane of conv5: the plane goes through LDS in tiles of 16 rows x 256 columns,
//                             each tile is stored to cat[:, :C] as it was read (bit-identical) and a thread per (row, column bin)
//                             adds its stretch of the row in column order, fp64; after a chunk of rows a thread per bin adds its
//                             rows in row order, fp64; at the end sum / area, rounded once.  conv5 is read once.
//             (the caller's conv / BN / ReLU on the pooled tensors)
//             k_ppm_fill      cat[:, C:]: the bilinear upsampling (align_corners=False, torch's fp32 index rule, computed here) of
//                             every branch output, all branches in one launch; four adjacent pixels per lane
//   backward  k_ppm_fill_bwd  a workgroup per plane of grad_cat[:, C:]: the transposed interpolation, separable -- a thread per
//                             (row, column tap) adds its stretch of the row in column order, a thread per tap adds the rows in row
//                             order, both fp64.  Planes of a branch without a gradient are not read
//             k_ppm_pool_bwd  grad_conv5 = grad_cat[:, :C] + sum over the scales and the bins covering the pixel of
//                             grad_p / area: the bins' quotients of the plane in LDS, the covering range computed per pixel
// No atomics, nothing to zero, nothing to the host: the same bits every run.  16-byte loads and stores when w % 4 == 0 and the
// bases are 16-byte aligned (every plane then is), scalar ones otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sdn_common.h"
#include "segm_ppm_check.h"

namespace sdn {

struct PpmPtrs {   // DEVICE pointers of the branches, by value in the kernel arguments
    float* p[PPM_MAX_SCALES];
};

// static indices only: the plan stays in scalar registers
__device__ __forceinline__ int ppm_pick(const int (&a)[PPM_MAX_SCALES], int k)
{
    return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3];
}
__device__ __forceinline__ int ppm_pick5(const int (&a)[PPM_MAX_SCALES + 1], int k)
{
    return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : k == 3 ? a[3] : a[4];
}
__device__ __forceinline__ float* ppm_pickp(const PpmPtrs& a, int k)
{
    return k == 0 ? a.p[0] : k == 1 ? a.p[1] : k == 2 ? a.p[2] : a.p[3];
}
// the branch whose prefix range holds q (0 <= q < pre[S])
__device__ __forceinline__ int ppm_branch(const int (&pre)[PPM_MAX_SCALES + 1], int S, int q)
{
    int k = 0;
#pragma unroll
    for (int kk = 1; kk < PPM_MAX_SCALES; kk++) k = (kk < S && q >= pre[kk]) ? kk : k;
    return k;
}

// rows [r0, r0 + rows) x columns [c0, c0 + cols) of a plane into the tile; with COPY also to dst, as read
template <bool VEC, bool COPY>
__device__ __forceinline__ void ppm_stage(const float* __restrict__ src, float* __restrict__ dst, int w, int r0, int rows, int c0, int cols,
                                          float* __restrict__ tile)
{
    if (VEC) {   // w % 4 == 0 and c0 % 4 == 0: cols % 4 == 0
        const int cw4 = cols >> 2, n4 = rows * cw4;
        for (int g = threadIdx.x; g < n4; g += PPM_THREADS) {
            const int rr = g / cw4, c4 = g - rr * cw4;
            const long at = (long)(r0 + rr) * w + c0 + 4 * c4;
            const float4 v = *reinterpret_cast<const float4*>(src + at);
            if (COPY) *reinterpret_cast<float4*>(dst + at) = v;
            *reinterpret_cast<float4*>(tile + rr * PPM_TILE_PITCH + 4 * c4) = v;
        }
    } else {
        const int n = rows * cols;
        for (int g = threadIdx.x; g < n; g += PPM_THREADS) {
            const int rr = g / cols, cc = g - rr * cols;
            const long at = (long)(r0 + rr) * w + c0 + cc;
            const float v = src[at];
            if (COPY) dst[at] = v;
            tile[rr * PPM_TILE_PITCH + cc] = v;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_pool(const float* __restrict__ conv5, PpmPlan P, int C, int Ctot, int h, int w,
                                                          float* __restrict__ cat, float* __restrict__ pooled, long BC)
{
    __shared__ float tile[PPM_TILE_ROWS * PPM_TILE_PITCH];
    __shared__ double colsum[PPM_TILE_ROWS * PPM_MAX_COLBINS];
    const int t = threadIdx.x;
    const long plane = blockIdx.x, HW = (long)h * w;
    const int b = (int)(plane / C), c = (int)(plane - (long)b * C);
    const float* src = conv5 + plane * HW;
    float* dst = cat + ((long)b * Ctot + c) * HW;
    const int NB = P.cb[PPM_MAX_SCALES], NBINS = P.bb[PPM_MAX_SCALES], R = ppm_pool_rows(NB);

    // this thread's (row of the tile, column bin)
    const bool is_seg = t < R * NB;
    int sr = 0, sq = 0, cs = 0, ce = 0;
    if (is_seg) {
        sr = t / NB;
        sq = t - sr * NB;
        const int k = ppm_branch(P.cb, P.S, sq), s = ppm_pick(P.s, k), j = sq - ppm_pick5(P.cb, k);
        cs = ppm_bin_start(j, w, s);
        ce = ppm_bin_end(j, w, s);
    }
    // this thread's bin
    const bool is_bin = t < NBINS;
    int rs = 0, re = 0, bq = 0, area = 1;
    long out_at = 0;
    if (is_bin) {
        const int k = ppm_branch(P.bb, P.S, t), s = ppm_pick(P.s, k), rem = t - ppm_pick5(P.bb, k);
        const int i = rem / s, j = rem - i * s;
        rs = ppm_bin_start(i, h, s);
        re = ppm_bin_end(i, h, s);
        bq = ppm_pick5(P.cb, k) + j;
        area = (re - rs) * (ppm_bin_end(j, w, s) - ppm_bin_start(j, w, s));
        out_at = BC * ppm_pick5(P.bb, k) + plane * (s * s) + rem;
    }
    double bacc = 0.0;
    for (int r0 = 0; r0 < h; r0 += R) {
        const int rows = min(R, h - r0);
        double acc = 0.0;
        for (int c0 = 0; c0 < w; c0 += PPM_TILE_COLS) {
            const int cols = min(PPM_TILE_COLS, w - c0);
            ppm_stage<VEC, true>(src, dst, w, r0, rows, c0, cols, tile);
            __syncthreads();
            if (is_seg && sr < rows) {
                const int lo = max(cs, c0) - c0, hi = min(ce, c0 + cols) - c0;
                const float* row = tile + sr * PPM_TILE_PITCH;
#pragma unroll 4
                for (int x = lo; x < hi; x++) acc += (double)row[x];
            }
            __syncthreads();
        }
        if (is_seg) colsum[sr * PPM_MAX_COLBINS + sq] = acc;
        __syncthreads();
        if (is_bin) {
            const int lo = max(rs, r0), hi = min(re, r0 + rows);
            for (int y = lo; y < hi; y++) bacc += colsum[(y - r0) * PPM_MAX_COLBINS + bq];
        }
        __syncthreads();
    }
    if (is_bin) pooled[out_at] = (float)(bacc / (double)area);
}

// one output pixel of a branch plane: torch's upsample_bilinear2d, operation for operation
__device__ __forceinline__ float ppm_lerp(const float* __restrict__ y, int s, int r0, int r1, float ly, float sx, int x)
{
    int c0, c1;
    float lx;
    ppm_taps(sx, x, s, &c0, &c1, &lx);
    const float a = (1.f - lx) * y[r0 * s + c0] + lx * y[r0 * s + c1];
    const float b = (1.f - lx) * y[r1 * s + c0] + lx * y[r1 * s + c1];
    return (1.f - ly) * a + ly * b;
}

template <bool VEC>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_fill(PpmPtrs Y, PpmPlan P, int C, int Ctot, int h, int w, int chunks,
                                                          float* __restrict__ cat)
{
    const long gb = blockIdx.x, plane = gb / chunks, HW = (long)h * w;
    const int ch = (int)(gb - plane * chunks), Ksum = P.kb[PPM_MAX_SCALES];
    const int b = (int)(plane / Ksum), cc = (int)(plane - (long)b * Ksum);
    const int k = ppm_branch(P.kb, P.S, cc), s = ppm_pick(P.s, k), j = cc - ppm_pick5(P.kb, k);
    const float* y = ppm_pickp(Y, k) + ((long)b * ppm_pick(P.K, k) + j) * (s * s);
    float* out = cat + ((long)b * Ctot + C + cc) * HW;
    const float sy = (float)s / (float)h, sx = (float)s / (float)w;
    if (VEC) {
        const long p = (long)ch * PPM_CHUNK + 4 * threadIdx.x;   // w % 4 == 0: the four pixels share a row
        if (p < HW) {
            const int row = (int)(p / w), col = (int)(p - (long)row * w);
            int r0, r1;
            float ly;
            ppm_taps(sy, row, s, &r0, &r1, &ly);
            float4 v;
            v.x = ppm_lerp(y, s, r0, r1, ly, sx, col);
            v.y = ppm_lerp(y, s, r0, r1, ly, sx, col + 1);
            v.z = ppm_lerp(y, s, r0, r1, ly, sx, col + 2);
            v.w = ppm_lerp(y, s, r0, r1, ly, sx, col + 3);
            *reinterpret_cast<float4*>(out + p) = v;
        }
    } else {
        for (int m = 0; m < PPM_CHUNK / PPM_THREADS; m++) {
            const long p = (long)ch * PPM_CHUNK + m * PPM_THREADS + threadIdx.x;
            if (p < HW) {
                const int row = (int)(p / w), col = (int)(p - (long)row * w);
                int r0, r1;
                float ly;
                ppm_taps(sy, row, s, &r0, &r1, &ly);
                out[p] = ppm_lerp(y, s, r0, r1, ly, sx, col);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_fill_bwd(const float* __restrict__ gcat, PpmPtrs GY, PpmPlan P, int C, int Ctot, int h,
                                                              int w)
{
    __shared__ float tile[PPM_TILE_ROWS * PPM_TILE_PITCH];
    __shared__ double colsum[PPM_TILE_ROWS * PPM_MAX_SIDE];
    const int t = threadIdx.x;
    const long plane = blockIdx.x, HW = (long)h * w;
    const int Ksum = P.kb[PPM_MAX_SCALES];
    const int b = (int)(plane / Ksum), cc = (int)(plane - (long)b * Ksum);
    const int k = ppm_branch(P.kb, P.S, cc), s = ppm_pick(P.s, k), j0 = cc - ppm_pick5(P.kb, k);
    float* gy = ppm_pickp(GY, k);
    if (!gy) return;   // the whole workgroup: this branch has no gradient, its planes are not read
    const float* src = gcat + ((long)b * Ctot + C + cc) * HW;
    const float sy = (float)s / (float)h, sx = (float)s / (float)w;

    // this thread's (row of the tile, column tap) and the columns that may weigh on the tap
    const bool is_seg = t < PPM_TILE_ROWS * s;
    int sr = 0, sj = 0, xlo = 0, xhi = 0;
    if (is_seg) {
        sr = t / s;
        sj = t - sr * s;
        ppm_tap_range(sj, w, s, &xlo, &xhi);
    }
    // this thread's tap
    const bool is_tap = t < s * s;
    const int ti = t / s, tj = t - ti * s;
    double bacc = 0.0;
    for (int r0 = 0; r0 < h; r0 += PPM_TILE_ROWS) {
        const int rows = min(PPM_TILE_ROWS, h - r0);
        double acc = 0.0;
        for (int c0 = 0; c0 < w; c0 += PPM_TILE_COLS) {
            const int cols = min(PPM_TILE_COLS, w - c0);
            ppm_stage<VEC, false>(src, nullptr, w, r0, rows, c0, cols, tile);
            __syncthreads();
            if (is_seg && sr < rows) {
                const int lo = max(xlo, c0), hi = min(xhi, c0 + cols);
                const float* row = tile + sr * PPM_TILE_PITCH - c0;
                for (int x = lo; x < hi; x++) acc += (double)ppm_tap_weight(sx, x, s, sj) * (double)row[x];
            }
            __syncthreads();
        }
        if (is_seg) colsum[sr * PPM_MAX_SIDE + sj] = acc;
        __syncthreads();
        if (is_tap)
            for (int r = 0; r < rows; r++) {
                const float wy = ppm_tap_weight(sy, r0 + r, s, ti);
                if (wy != 0.f) bacc += (double)wy * colsum[r * PPM_MAX_SIDE + tj];
            }
        __syncthreads();
    }
    if (is_tap) gy[((long)b * ppm_pick(P.K, k) + j0) * (s * s) + t] = (float)bacc;
}

// what the bins of every scale add to one pixel: scales, rows and columns in ascending order
__device__ __forceinline__ float ppm_cover_sum(const float* __restrict__ bins, const PpmPlan& P, const PpmPtrs& GP, int h, int w, int y, int x,
                                               float v)
{
#pragma unroll
    for (int k = 0; k < PPM_MAX_SCALES; k++)
        if (k < P.S && GP.p[k]) {
            const int s = P.s[k];
            int ilo, ihi, jlo, jhi;
            ppm_cover(y, h, s, &ilo, &ihi);
            ppm_cover(x, w, s, &jlo, &jhi);
            for (int i = ilo; i <= ihi; i++)
                for (int j = jlo; j <= jhi; j++) v += bins[P.bb[k] + i * s + j];
        }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_pool_bwd(const float* __restrict__ gcat, PpmPtrs GP, PpmPlan P, int C, int Ctot, int h,
                                                              int w, int chunks, float* __restrict__ gx)
{
    __shared__ float bins[PPM_MAX_BINS];
    const int t = threadIdx.x;
    const long gb = blockIdx.x, plane = gb / chunks, HW = (long)h * w;
    const int ch = (int)(gb - plane * chunks);
    const int b = (int)(plane / C), c = (int)(plane - (long)b * C);
    if (t < P.bb[PPM_MAX_SCALES]) {
        const int k = ppm_branch(P.bb, P.S, t), s = ppm_pick(P.s, k), rem = t - ppm_pick5(P.bb, k);
        const int i = rem / s, j = rem - i * s;
        const int area = (ppm_bin_end(i, h, s) - ppm_bin_start(i, h, s)) * (ppm_bin_end(j, w, s) - ppm_bin_start(j, w, s));
        const float* gp = ppm_pickp(GP, k);
        bins[t] = gp ? gp[plane * (s * s) + rem] / (float)area : 0.f;
    }
    __syncthreads();
    const float* src = gcat ? gcat + ((long)b * Ctot + c) * HW : nullptr;
    float* dst = gx + plane * HW;
    if (VEC) {
        const long p = (long)ch * PPM_CHUNK + 4 * t;   // w % 4 == 0: the four pixels share a row
        if (p < HW) {
            const int row = (int)(p / w), col = (int)(p - (long)row * w);
            float4 v = src ? *reinterpret_cast<const float4*>(src + p) : make_float4(0.f, 0.f, 0.f, 0.f);
            v.x = ppm_cover_sum(bins, P, GP, h, w, row, col, v.x);
            v.y = ppm_cover_sum(bins, P, GP, h, w, row, col + 1, v.y);
            v.z = ppm_cover_sum(bins, P, GP, h, w, row, col + 2, v.z);
            v.w = ppm_cover_sum(bins, P, GP, h, w, row, col + 3, v.w);
            *reinterpret_cast<float4*>(dst + p) = v;
        }
    } else {
        for (int m = 0; m < PPM_CHUNK / PPM_THREADS; m++) {
            const long p = (long)ch * PPM_CHUNK + m * PPM_THREADS + t;
            if (p < HW) {
                const int row = (int)(p / w), col = (int)(p - (long)row * w);
                dst[p] = ppm_cover_sum(bins, P, GP, h, w, row, col, src ? src[p] : 0.f);
            }
        }
    }
}

static bool ppm_aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_segm_ppm_pool(const float* conv5, int B, int C, int h, int w, const int* scales, const int* branch_channels, int S,
                              float* cat, float* pooled, sdnStream stream)
{
    char why[256];
    int Ctot = 0;
    if (ppm_validate_pool(conv5, cat, pooled, scales, branch_channels, S, B, C, h, w, &Ctot, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_segm_ppm_pool: %s", why);
    PpmPlan P;
    ppm_plan_make(scales, branch_channels, S, &P);
    hipStream_t st = (hipStream_t)stream;
    const long BC = (long)B * C;
    const bool vec = (w & 3) == 0 && ppm_aligned16(conv5) && ppm_aligned16(cat);
    const dim3 grid((unsigned)BC), block(PPM_THREADS);
    if (vec) hipLaunchKernelGGL(k_ppm_pool<true>, grid, block, 0, st, conv5, P, C, Ctot, h, w, cat, pooled, BC);
    else hipLaunchKernelGGL(k_ppm_pool<false>, grid, block, 0, st, conv5, P, C, Ctot, h, w, cat, pooled, BC);
    return check_launch("k_ppm_pool");
}

SDN_API int sdn_segm_ppm_fill(const float* const* y, int B, int C, int h, int w, const int* scales, const int* branch_channels, int S,
                              float* cat, sdnStream stream)
{
    char why[256];
    int Ctot = 0;
    if (ppm_validate_fill(y, cat, scales, branch_channels, S, B, C, h, w, &Ctot, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_segm_ppm_fill: %s", why);
    PpmPlan P;
    ppm_plan_make(scales, branch_channels, S, &P);
    PpmPtrs Y = {};
    for (int k = 0; k < S; k++) Y.p[k] = const_cast<float*>(y[k]);
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)h * w;
    const int chunks = ppm_chunks(HW);
    const bool vec = (w & 3) == 0 && ppm_aligned16(cat);
    const dim3 grid((unsigned)((long)B * P.kb[PPM_MAX_SCALES] * chunks)), block(PPM_THREADS);
    if (vec) hipLaunchKernelGGL(k_ppm_fill<true>, grid, block, 0, st, Y, P, C, Ctot, h, w, chunks, cat);
    else hipLaunchKernelGGL(k_ppm_fill<false>, grid, block, 0, st, Y, P, C, Ctot, h, w, chunks, cat);
    return check_launch("k_ppm_fill");
}

SDN_API int sdn_segm_ppm_fill_bwd(const float* grad_cat, int B, int C, int h, int w, const int* scales, const int* branch_channels, int S,
                                  float* const* grad_y, sdnStream stream)
{
    char why[256];
    int Ctot = 0;
    if (ppm_validate_fill_bwd(grad_cat, grad_y, scales, branch_channels, S, B, C, h, w, &Ctot, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_segm_ppm_fill_bwd: %s", why);
    PpmPlan P;
    ppm_plan_make(scales, branch_channels, S, &P);
    PpmPtrs GY = {};
    for (int k = 0; k < S; k++) GY.p[k] = grad_y[k];
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (w & 3) == 0 && ppm_aligned16(grad_cat);
    const dim3 grid((unsigned)((long)B * P.kb[PPM_MAX_SCALES])), block(PPM_THREADS);
    if (vec) hipLaunchKernelGGL(k_ppm_fill_bwd<true>, grid, block, 0, st, grad_cat, GY, P, C, Ctot, h, w);
    else hipLaunchKernelGGL(k_ppm_fill_bwd<false>, grid, block, 0, st, grad_cat, GY, P, C, Ctot, h, w);
    return check_launch("k_ppm_fill_bwd");
}

SDN_API int sdn_segm_ppm_pool_bwd(const float* grad_cat, const float* const* grad_p, int B, int C, int h, int w, const int* scales,
                                  const int* branch_channels, int S, float* grad_conv5, sdnStream stream)
{
    char why[256];
    int Ctot = 0;
    if (ppm_validate_pool_bwd(grad_cat, grad_p, grad_conv5, scales, branch_channels, S, B, C, h, w, &Ctot, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_segm_ppm_pool_bwd: %s", why);
    PpmPlan P;
    ppm_plan_make(scales, branch_channels, S, &P);
    PpmPtrs GP = {};
    for (int k = 0; k < S && grad_p; k++) GP.p[k] = const_cast<float*>(grad_p[k]);
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)h * w;
    const int chunks = ppm_chunks(HW);
    const bool vec = (w & 3) == 0 && ppm_aligned16(grad_conv5) && (!grad_cat || ppm_aligned16(grad_cat));
    const dim3 grid((unsigned)((long)B * C * chunks)), block(PPM_THREADS);
    if (vec) hipLaunchKernelGGL(k_ppm_pool_bwd<true>, grid, block, 0, st, grad_cat, GP, P, C, Ctot, h, w, chunks, grad_conv5);
    else hipLaunchKernelGGL(k_ppm_pool_bwd<false>, grid, block, 0, st, grad_cat, GP, P, C, Ctot, h, w, chunks, grad_conv5);
    return check_launch("k_ppm_pool_bwd");
}
