// The training loss of the semantic branch: the body of SegmentationModule.forward after the network call
// (semantic/models.py:15-21, 39-45) with the decoders' log_softmax (:279-280, 412-413) and
// nn.NLLLoss(ignore_index=-1) (vkitti_train.py:133).  The reference runs log_softmax on both heads, NLLLoss twice, the scaled sum
// and pixel_acc (torch.max, two .long() masks, two sums, a division): about twenty small launches each way over [B, C, h, w]
// tensors of under 1 MB, several of them written and read again.  Here the inputs are the class SCORES of decoder.conv_last:
//   forward   k_segm_loss_partial  grid (item x chunk of SGL_PIXELS pixels), one wave per workgroup: per pixel and head the
//                                  maximum, lse = max + log(sum exp(x - max)) and -(x[label] - lse); for the main head the
//                                  arg-max of the scores (strict >: the lowest class wins a tie, NaN never wins -- segm_tail.hip's
//                                  rule); per workgroup two fp64 sums and three integer counts into scratch; lse [2, B, h, w]
//             k_segm_loss_finish   one wave: the partials in block order; out[4] = loss, acc, loss_main, loss_deepsup and
//                                  counts[3] = acc_sum, pixel_sum, bad
//   backward  k_segm_loss_grad     one launch for both heads: (exp(x - lse) - [c == label]) g / pixel_sum, 0 on ignored pixels
// A pixel's C <= 32 scores of one head live in registers, so each direction reads each score tensor once.  A lane owns four
// adjacent pixels of a plane (one 16-byte load per class) when h * w % 4 == 0 and the bases are 16-byte aligned; otherwise four
// pixels 64 apart, so that the lanes of a wave read adjacent floats.  No atomics, nothing to zero: the same bits every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "sdn_common.h"
#include "segm_loss_check.h"

namespace sdn {

// the class of a label, or -1 for an ignored pixel: -1 itself, or any label outside [0, C), which `bad` counts (the reference's
// NLLLoss raises there)
__device__ __forceinline__ int sgl_class(int64_t l, int C, int& bad)
{
    const bool ok = l >= 0 && l < (int64_t)C;
    bad += (!ok && l != -1) ? 1 : 0;
    return ok ? (int)l : -1;
}

// the scores of NP pixels for all classes (NP == 4: adjacent pixels, one 16-byte load per class; NP == 1: scalar loads);
// x points at class 0 of the first pixel
template <int CP, int NP>
__device__ __forceinline__ void sgl_load(const float* __restrict__ x, long HW, int C, float (&v)[CP][NP])
{
#pragma unroll
    for (int c = 0; c < CP; c++)
        if (c < C) {
            if constexpr (NP == 4) {
                const float4 q = *reinterpret_cast<const float4*>(x + (long)c * HW);
                v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
            } else {
                v[c][0] = x[(long)c * HW];
            }
        }
}

// per pixel: lse, the arg-max of the scores and -(x[label] - lse) (0 for an ignored pixel)
template <int CP, int NP>
__device__ __forceinline__ void sgl_stats(const float (&v)[CP][NP], int C, const int (&lab)[NP], float (&lse)[NP], int (&best)[NP],
                                          float (&nll)[NP])
{
#pragma unroll
    for (int e = 0; e < NP; e++) {
        float top = v[0][e], xl = v[0][e];
        int bi = 0;
#pragma unroll
        for (int c = 1; c < CP; c++)
            if (c < C) {
                if (v[c][e] > top) {   // strictly greater: the lowest class wins a tie, NaN never wins
                    top = v[c][e];
                    bi = c;
                }
                xl = c == lab[e] ? v[c][e] : xl;
            }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CP; c++)
            if (c < C) s += expf(v[c][e] - top);
        const float l = top + logf(s);
        lse[e] = l;
        best[e] = bi;
        nll[e] = lab[e] >= 0 ? -(xl - l) : 0.f;
    }
}

struct SglAcc {
    double s0, s1;
    int hit, pix, bad;
};

// NP pixels of item b starting at pixel p of its plane, both heads
template <int CP, int NP>
__device__ __forceinline__ void sgl_partial_group(const float* __restrict__ s0, const float* __restrict__ s1,
                                                  const int64_t* __restrict__ label, int b, long p, int C, long HW, long BHW,
                                                  float* __restrict__ lse_out, SglAcc& a)
{
    int lab[NP];
    if constexpr (NP == 4) {
        const longlong2* lp = reinterpret_cast<const longlong2*>(label + (long)b * HW + p);
        const longlong2 l0 = lp[0], l1 = lp[1];
        lab[0] = sgl_class(l0.x, C, a.bad); lab[1] = sgl_class(l0.y, C, a.bad);
        lab[2] = sgl_class(l1.x, C, a.bad); lab[3] = sgl_class(l1.y, C, a.bad);
    } else {
        lab[0] = sgl_class(label[(long)b * HW + p], C, a.bad);
    }
    float v[CP][NP], lse[NP], nll[NP];
    int best[NP];
    sgl_load<CP, NP>(s0 + (long)b * C * HW + p, HW, C, v);
    sgl_stats<CP, NP>(v, C, lab, lse, best, nll);
#pragma unroll
    for (int e = 0; e < NP; e++) {
        a.s0 += (double)nll[e];
        a.pix += lab[e] >= 0 ? 1 : 0;
        a.hit += (lab[e] >= 0 && best[e] == lab[e]) ? 1 : 0;
    }
    float* lo = lse_out + (long)b * HW + p;
    if constexpr (NP == 4) *reinterpret_cast<float4*>(lo) = make_float4(lse[0], lse[1], lse[2], lse[3]);
    else lo[0] = lse[0];
    if (s1) {
        sgl_load<CP, NP>(s1 + (long)b * C * HW + p, HW, C, v);
        sgl_stats<CP, NP>(v, C, lab, lse, best, nll);
#pragma unroll
        for (int e = 0; e < NP; e++) a.s1 += (double)nll[e];
    }
    // without a deepsup head its half of lse is written all the same: the buffer holds the same bits every run
    if constexpr (NP == 4) *reinterpret_cast<float4*>(lo + BHW) = s1 ? make_float4(lse[0], lse[1], lse[2], lse[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    else lo[BHW] = s1 ? lse[0] : 0.f;
}

// CP: the class count rounded up to 8, 16 or 32 (register arrays); VEC: 16-byte loads of four adjacent pixels
template <int CP, bool VEC>
__global__ __launch_bounds__(SGL_THREADS) void k_segm_loss_partial(const float* __restrict__ s0, const float* __restrict__ s1,
                                                                  const int64_t* __restrict__ label, int C, long HW, int chunks, long BHW,
                                                                  double* __restrict__ psum, int* __restrict__ pcnt,
                                                                  float* __restrict__ lse)
{
    const int gb = blockIdx.x, b = gb / chunks, k = gb - b * chunks, lane = threadIdx.x;
    const long p0 = (long)k * SGL_PIXELS;
    SglAcc a = {0.0, 0.0, 0, 0, 0};
    if (VEC) {
        const long p = p0 + 4 * lane;   // HW % 4 == 0: a quad lies wholly inside the plane or wholly outside
        if (p < HW) sgl_partial_group<CP, 4>(s0, s1, label, b, p, C, HW, BHW, lse, a);
    } else {
        for (int j = 0; j < SGL_PIXELS / SGL_THREADS; j++) {
            const long p = p0 + j * SGL_THREADS + lane;
            if (p < HW) sgl_partial_group<CP, 1>(s0, s1, label, b, p, C, HW, BHW, lse, a);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.s0 += __shfl_xor(a.s0, o, 64);
        a.s1 += __shfl_xor(a.s1, o, 64);
    }
    a.hit = wave_sum(a.hit);
    a.pix = wave_sum(a.pix);
    a.bad = wave_sum(a.bad);
    if (lane == 0) {
        psum[2 * (long)gb] = a.s0;
        psum[2 * (long)gb + 1] = a.s1;
        pcnt[4 * (long)gb] = a.hit;
        pcnt[4 * (long)gb + 1] = a.pix;
        pcnt[4 * (long)gb + 2] = a.bad;
        pcnt[4 * (long)gb + 3] = 0;
    }
}

__global__ __launch_bounds__(64) void k_segm_loss_finish(const double* __restrict__ psum, const int* __restrict__ pcnt, long nblk,
                                                         int deepsup, float scale, float* __restrict__ out, int64_t* __restrict__ counts)
{
    // lane l takes the workgroups l, l + 64, ... in order, then a fixed butterfly
    double s0 = 0.0, s1 = 0.0;
    long long hit = 0, pix = 0, bad = 0;
    for (long g = threadIdx.x; g < nblk; g += 64) {
        s0 += psum[2 * g];
        s1 += psum[2 * g + 1];
        hit += pcnt[4 * g];
        pix += pcnt[4 * g + 1];
        bad += pcnt[4 * g + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
        hit += __shfl_xor(hit, o, 64);
        pix += __shfl_xor(pix, o, 64);
        bad += __shfl_xor(bad, o, 64);
    }
    if (threadIdx.x == 0) {
        // NLLLoss's mean over the valid pixels: 0 / 0 = NaN when there is none, as torch gives
        const float lm = (float)(s0 / (double)pix);
        const float ld = deepsup ? (float)(s1 / (double)pix) : 0.f;
        out[0] = deepsup ? lm + ld * scale : lm;                   // models.py:42
        out[1] = (float)hit / ((float)pix + 1e-10f);               // models.py:20, in fp32 as there
        out[2] = lm;
        out[3] = ld;
        counts[0] = hit;
        counts[1] = pix;
        counts[2] = bad;
    }
}

// the gradients of NP pixels of one head: every element is written
template <int CP, int NP>
__device__ __forceinline__ void sgl_grad_group(const float* __restrict__ x, const float* __restrict__ lse, const int (&lab)[NP], int C,
                                               long HW, float gk, float* __restrict__ gx)
{
    float v[CP][NP], l[NP];
    sgl_load<CP, NP>(x, HW, C, v);
    if constexpr (NP == 4) {
        const float4 q = *reinterpret_cast<const float4*>(lse);
        l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
    } else {
        l[0] = lse[0];
    }
#pragma unroll
    for (int c = 0; c < CP; c++)
        if (c < C) {
            float o[NP];
#pragma unroll
            for (int e = 0; e < NP; e++) o[e] = lab[e] >= 0 ? (expf(v[c][e] - l[e]) - (c == lab[e] ? 1.f : 0.f)) * gk : 0.f;
            if constexpr (NP == 4) *reinterpret_cast<float4*>(gx + (long)c * HW) = make_float4(o[0], o[1], o[2], o[3]);
            else gx[(long)c * HW] = o[0];
        }
}

template <int CP, int NP>
__device__ __forceinline__ void sgl_grad_pixels(const float* __restrict__ s0, const float* __restrict__ s1,
                                                const int64_t* __restrict__ label, int b, long p, int C, long HW, long BHW,
                                                const float* __restrict__ lse, float g0, float g1, float* __restrict__ gs0,
                                                float* __restrict__ gs1)
{
    int lab[NP], bad = 0;
    if constexpr (NP == 4) {
        const longlong2* lp = reinterpret_cast<const longlong2*>(label + (long)b * HW + p);
        const longlong2 l0 = lp[0], l1 = lp[1];
        lab[0] = sgl_class(l0.x, C, bad); lab[1] = sgl_class(l0.y, C, bad);
        lab[2] = sgl_class(l1.x, C, bad); lab[3] = sgl_class(l1.y, C, bad);
    } else {
        lab[0] = sgl_class(label[(long)b * HW + p], C, bad);
    }
    const long at = (long)b * C * HW + p, la = (long)b * HW + p;
    if (gs0) sgl_grad_group<CP, NP>(s0 + at, lse + la, lab, C, HW, g0, gs0 + at);
    if (gs1) sgl_grad_group<CP, NP>(s1 + at, lse + BHW + la, lab, C, HW, g1, gs1 + at);
}

template <int CP, bool VEC>
__global__ __launch_bounds__(SGL_THREADS) void k_segm_loss_grad(const float* __restrict__ s0, const float* __restrict__ s1,
                                                               const int64_t* __restrict__ label, int C, long HW, int chunks, long BHW,
                                                               const float* __restrict__ lse, const int64_t* __restrict__ counts,
                                                               const float* __restrict__ gout, float scale, float* __restrict__ gs0,
                                                               float* __restrict__ gs1)
{
    const int gb = blockIdx.x, b = gb / chunks, k = gb - b * chunks, lane = threadIdx.x;
    const long p0 = (long)k * SGL_PIXELS;
    // d loss / d loss_main = 1, d loss / d loss_deepsup = deep_sup_scale; acc carries no gradient.  With no valid pixel the
    // quotient is never used: every pixel is ignored and gets 0.
    const float n = (float)counts[1];
    const float g0 = (gout[0] + gout[2]) / n, g1 = (gout[0] * scale + gout[3]) / n;
    if (VEC) {
        const long p = p0 + 4 * lane;
        if (p < HW) sgl_grad_pixels<CP, 4>(s0, s1, label, b, p, C, HW, BHW, lse, g0, g1, gs0, gs1);
    } else {
        for (int j = 0; j < SGL_PIXELS / SGL_THREADS; j++) {
            const long p = p0 + j * SGL_THREADS + lane;
            if (p < HW) sgl_grad_pixels<CP, 1>(s0, s1, label, b, p, C, HW, BHW, lse, g0, g1, gs0, gs1);
        }
    }
}

static bool sgl_aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_segm_loss_fwd(const float* scores, const float* scores_deepsup, const int64_t* seg_label, int B, int C, int h, int w,
                              float deep_sup_scale, void* scratch, size_t scratch_bytes, float* lse, float* out, int64_t* counts,
                              sdnStream stream)
{
    char why[256];
    if (sgl_validate_fwd(scores, seg_label, scratch, scratch_bytes, lse, out, counts, B, C, h, w, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_segm_loss_fwd: %s", why);
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)h * w, BHW = (long)B * HW, nblk = sgl_blocks(B, HW);
    const int chunks = sgl_chunks(HW);
    double* psum = reinterpret_cast<double*>(static_cast<char*>(scratch) + sgl_sum_at(0));
    int* pcnt = reinterpret_cast<int*>(static_cast<char*>(scratch) + sgl_cnt_at(nblk, 0));
    const bool vec = (HW & 3) == 0 && sgl_aligned16(scores) && sgl_aligned16(scores_deepsup) && sgl_aligned16(seg_label) && sgl_aligned16(lse);
    const dim3 grid((unsigned)nblk), block(SGL_THREADS);
#define SGL_FWD(CP)                                                                                                                  \
    do {                                                                                                                             \
        if (vec) hipLaunchKernelGGL((k_segm_loss_partial<CP, true>), grid, block, 0, st, scores, scores_deepsup, seg_label, C, HW,   \
                                    chunks, BHW, psum, pcnt, lse);                                                                   \
        else hipLaunchKernelGGL((k_segm_loss_partial<CP, false>), grid, block, 0, st, scores, scores_deepsup, seg_label, C, HW,      \
                                chunks, BHW, psum, pcnt, lse);                                                                       \
    } while (0)
    if (C <= 8) SGL_FWD(8);
    else if (C <= 16) SGL_FWD(16);
    else SGL_FWD(32);
#undef SGL_FWD
    if (int rc = check_launch("k_segm_loss_partial")) return rc;
    hipLaunchKernelGGL(k_segm_loss_finish, dim3(1), dim3(64), 0, st, psum, pcnt, nblk, scores_deepsup ? 1 : 0, deep_sup_scale, out, counts);
    return check_launch("k_segm_loss_finish");
}

SDN_API int sdn_segm_loss_bwd(const float* scores, const float* scores_deepsup, const int64_t* seg_label, int B, int C, int h, int w,
                              float deep_sup_scale, const float* lse, const int64_t* counts, const float* grad_out, float* grad_scores,
                              float* grad_scores_deepsup, sdnStream stream)
{
    char why[256];
    if (sgl_validate_bwd(scores, scores_deepsup, seg_label, lse, counts, grad_out, grad_scores, grad_scores_deepsup, B, C, h, w, why,
                         sizeof(why)))
        return fail(SDN_EINVAL, "sdn_segm_loss_bwd: %s", why);
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)h * w, BHW = (long)B * HW, nblk = sgl_blocks(B, HW);
    const int chunks = sgl_chunks(HW);
    const bool vec = (HW & 3) == 0 && sgl_aligned16(seg_label) && sgl_aligned16(lse) &&
                     (!grad_scores || (sgl_aligned16(scores) && sgl_aligned16(grad_scores))) &&
                     (!grad_scores_deepsup || (sgl_aligned16(scores_deepsup) && sgl_aligned16(grad_scores_deepsup)));
    const dim3 grid((unsigned)nblk), block(SGL_THREADS);
#define SGL_BWD(CP)                                                                                                                  \
    do {                                                                                                                             \
        if (vec) hipLaunchKernelGGL((k_segm_loss_grad<CP, true>), grid, block, 0, st, scores, scores_deepsup, seg_label, C, HW, chunks, \
                                    BHW, lse, counts, grad_out, deep_sup_scale, grad_scores, grad_scores_deepsup);                   \
        else hipLaunchKernelGGL((k_segm_loss_grad<CP, false>), grid, block, 0, st, scores, scores_deepsup, seg_label, C, HW, chunks, \
                                BHW, lse, counts, grad_out, deep_sup_scale, grad_scores, grad_scores_deepsup);                       \
    } while (0)
    if (C <= 8) SGL_BWD(8);
    else if (C <= 16) SGL_BWD(16);
    else SGL_BWD(32);
#undef SGL_BWD
    return check_launch("k_segm_loss_grad");
}
