// The RPN's outputs in one launch each way: what RPN.forward does after its convs (geometric/maskrcnn/model.py:896-911) on each of the
// pyramid's levels -- permute(0, 2, 3, 1).contiguous().view of the class map and of the box map, the softmax over (bg, fg) -- and the
// three torch.cat(dim=1) over the levels in MaskRCNN.predict (:1729-1740).  For five levels that is 18 launches forward, about as many
// strided copies backward, and every byte moves twice (the copy, then the cat).
//
// Every output element is a function of one input element (two for the softmax) at a known address:
//     level l starts at anchor k * sum_{m < l} H_m W_m;
//     anchor (y * W + x) * k + a, component j, is channel a * 2 + j (boxes: a * 4 + j) at pixel (y, x).
// So the input is channel-major and the output pixel-major: a transpose of [6k, pixels] tiles.  A workgroup owns RPO_TILE consecutive
// pixels of one level (it finds the level in the prefix table that travels in the kernel's arguments, rpn_outputs_check.h), reads
// each of the 6k channels with coalesced 4-byte loads into a padded LDS tile [pixel][channel], computes the probabilities there and
// writes its three output runs, which are contiguous, from the LDS.  A run's first float is 2k (4k) * pixels before it: with k = 1
// and a 3 x 5 level the next level's logits start at float 30, so a run is written as a scalar head up to the next 16-byte boundary,
// a body of 16-byte stores and a scalar tail.  Every element is written once: no memset, no atomics, no workspace.
//
// The probabilities are exp(x_j - max(x_0, x_1)) / (e_0 + e_1) in fp32, one expf per element; a non-finite logit follows the
// formula: (+inf, x), (-inf, -inf) and a NaN give NaN in both places, as torch's softmax does.  The build has no FMA contraction.
//
// Backward: the same tiles the other way.  The class gradient of a pair is g_logit_j + p_j * (g_p_j - (g_p_0 p_0 + g_p_1 p_1)); a NULL
// gradient counts as zero and is not read, and without grad_probs (always so in training: the proposals carry no gradient) the class
// gradient is grad_logits transposed, bit for bit.  Every element of the 2L map gradients is written once; the bits are the same
// every run.  At the reference's size (A = 261 888, k = 3) a launch moves about 15 MB: it is bound by the launch, not the memory.
#include <hip/hip_runtime.h>

#include "rpn_outputs_check.h"
#include "sdn_common.h"

namespace sdn {

struct RpoFwd {
    RpoTable T;
    const float* cls[RPO_MAX_LEVELS];
    const float* box[RPO_MAX_LEVELS];
    float *logits, *probs, *bbox;
};

struct RpoBwd {
    RpoTable T;
    const float *g_logits, *g_probs, *g_bbox, *probs;   // each may be NULL
    float* g_cls[RPO_MAX_LEVELS];
    float* g_box[RPO_MAX_LEVELS];
};

// the pixels [pix0, pix0 + n) of level l that workgroup blockIdx.x owns
__device__ __forceinline__ void rpo_tile(const RpoTable& T, int* l, int* pix0, int* n)
{
    const int t = (int)blockIdx.x;
    *l = rpo_level_of(T, t);
    *pix0 = (t - T.tile[*l]) * RPO_TILE;
    const int left = T.hw[*l] - *pix0;
    *n = left < RPO_TILE ? left : RPO_TILE;
}

// `len` floats from the padded tile `src` (rows of ch + 1) to dst[0 .. len): scalar stores up to the first 16-byte boundary of dst,
// 16-byte stores, scalar stores behind the last whole quad.  `at` is dst's offset in floats from a 16-byte aligned base.
__device__ __forceinline__ void rpo_store_run(float* __restrict__ dst, unsigned at, int len, const float* src, int ch)
{
    const int tid = (int)threadIdx.x;
    int head = (int)((4u - (at & 3u)) & 3u);
    head = head < len ? head : len;
    const int quads = (len - head) >> 2;
    if (tid < head) dst[tid] = src[rpo_padded(tid, ch)];
    for (int q = tid; q < quads; q += RPO_THREADS) {
        const int i = head + 4 * q;
        float4 v;
        v.x = src[rpo_padded(i, ch)];
        v.y = src[rpo_padded(i + 1, ch)];
        v.z = src[rpo_padded(i + 2, ch)];
        v.w = src[rpo_padded(i + 3, ch)];
        *reinterpret_cast<float4*>(dst + i) = v;
    }
    const int i = head + 4 * quads + tid;
    if (i < len) dst[i] = src[rpo_padded(i, ch)];
}

__global__ __launch_bounds__(RPO_THREADS) void k_rpo_fwd(const RpoFwd a)
{
    extern __shared__ float rpo_lds[];
    const int k = a.T.k, c2 = 2 * k, c4 = 4 * k, s2 = c2 + 1, s4 = c4 + 1;
    float* xs = rpo_lds;                 // logits [RPO_TILE][s2]
    float* ps = xs + RPO_TILE * s2;      // probabilities, same places
    float* bs = ps + RPO_TILE * s2;      // boxes [RPO_TILE][s4]
    int l, pix0, n;
    rpo_tile(a.T, &l, &pix0, &n);
    const int b = (int)blockIdx.y, hw = a.T.hw[l];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if (lane < n) {
        const float* cm = a.cls[l] + ((size_t)b * c2 * hw + pix0 + lane);
        const float* bm = a.box[l] + ((size_t)b * c4 * hw + pix0 + lane);
        for (int c = wave; c < c2; c += RPO_THREADS / 64) xs[lane * s2 + c] = cm[(size_t)c * hw];
        for (int c = wave; c < c4; c += RPO_THREADS / 64) bs[lane * s4 + c] = bm[(size_t)c * hw];
    }
    __syncthreads();
    for (int q = (int)threadIdx.x; q < n * k; q += RPO_THREADS) {   // one (bg, fg) pair each
        const int i = rpo_padded(2 * q, c2);
        const float x0 = xs[i], x1 = xs[i + 1];
        const float m = x0 > x1 ? x0 : x1;                         // a NaN reaches one of the differences either way
        const float e0 = expf(x0 - m), e1 = expf(x1 - m);
        const float sum = e0 + e1;
        ps[i] = e0 / sum;
        ps[i + 1] = e1 / sum;
    }
    __syncthreads();
    const unsigned first = (unsigned)b * (unsigned)a.T.anchors + (unsigned)k * (unsigned)(a.T.pix[l] + pix0);   // this run's first anchor
    rpo_store_run(a.logits + (size_t)first * 2, first * 2u, n * c2, xs, c2);
    rpo_store_run(a.probs + (size_t)first * 2, first * 2u, n * c2, ps, c2);
    rpo_store_run(a.bbox + (size_t)first * 4, first * 4u, n * c4, bs, c4);
}

__global__ __launch_bounds__(RPO_THREADS) void k_rpo_bwd(const RpoBwd a)
{
    extern __shared__ float rpo_lds[];
    const int k = a.T.k, c2 = 2 * k, c4 = 4 * k, s2 = c2 + 1, s4 = c4 + 1;
    float* gx = rpo_lds;                 // class gradients [RPO_TILE][s2]
    float* gb = gx + RPO_TILE * s2;      // box gradients [RPO_TILE][s4]
    int l, pix0, n;
    rpo_tile(a.T, &l, &pix0, &n);
    const int b = (int)blockIdx.y, hw = a.T.hw[l];
    const size_t first = (size_t)b * (size_t)a.T.anchors + (size_t)k * (size_t)(a.T.pix[l] + pix0);
    for (int q = (int)threadIdx.x; q < n * k; q += RPO_THREADS) {
        const size_t at = first * 2 + 2 * (size_t)q;
        float g0 = 0.0f, g1 = 0.0f;
        if (a.g_logits) {
            g0 = a.g_logits[at];
            g1 = a.g_logits[at + 1];
        }
        if (a.g_probs) {
            const float p0 = a.probs[at], p1 = a.probs[at + 1], h0 = a.g_probs[at], h1 = a.g_probs[at + 1];
            const float dot = h0 * p0 + h1 * p1;
            g0 = g0 + p0 * (h0 - dot);
            g1 = g1 + p1 * (h1 - dot);
        }
        const int i = rpo_padded(2 * q, c2);
        gx[i] = g0;
        gx[i + 1] = g1;
    }
    for (int i = (int)threadIdx.x; i < n * c4; i += RPO_THREADS) gb[rpo_padded(i, c4)] = a.g_bbox ? a.g_bbox[first * 4 + (size_t)i] : 0.0f;
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if (lane < n) {
        float* cm = a.g_cls[l] + ((size_t)b * c2 * hw + pix0 + lane);
        float* bm = a.g_box[l] + ((size_t)b * c4 * hw + pix0 + lane);
        for (int c = wave; c < c2; c += RPO_THREADS / 64) cm[(size_t)c * hw] = gx[lane * s2 + c];
        for (int c = wave; c < c4; c += RPO_THREADS / 64) bm[(size_t)c * hw] = gb[lane * s4 + c];
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_rpn_outputs_fwd(const float* const* class_maps, const float* const* bbox_maps, const int* H, const int* W, int L, int k, int B,
                                float* rpn_class_logits, float* rpn_probs, float* rpn_bbox, sdnStream stream)
{
    char why[256];
    RpoFwd a;
    if (rpo_validate_fwd((const void* const*)class_maps, (const void* const*)bbox_maps, H, W, L, k, B, rpn_class_logits, rpn_probs, rpn_bbox,
                         &a.T, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_rpn_outputs_fwd: %s", why);
    for (int l = 0; l < RPO_MAX_LEVELS; l++) {
        a.cls[l] = l < L ? class_maps[l] : nullptr;
        a.box[l] = l < L ? bbox_maps[l] : nullptr;
    }
    a.logits = rpn_class_logits;
    a.probs = rpn_probs;
    a.bbox = rpn_bbox;
    hipLaunchKernelGGL(k_rpo_fwd, dim3((unsigned)a.T.tile[L], (unsigned)B), dim3(RPO_THREADS), sizeof(float) * (size_t)rpo_lds_floats(k),
                       (hipStream_t)stream, a);
    return check_launch("sdn_rpn_outputs_fwd");
}

SDN_API int sdn_rpn_outputs_bwd(const float* grad_logits, const float* grad_probs, const float* grad_bbox, const float* rpn_probs, const int* H,
                                const int* W, int L, int k, int B, float* const* grad_class_maps, float* const* grad_bbox_maps,
                                sdnStream stream)
{
    char why[256];
    RpoBwd a;
    if (rpo_validate_bwd(grad_logits, grad_probs, grad_bbox, rpn_probs, H, W, L, k, B, (const void* const*)grad_class_maps,
                         (const void* const*)grad_bbox_maps, &a.T, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_rpn_outputs_bwd: %s", why);
    for (int l = 0; l < RPO_MAX_LEVELS; l++) {
        a.g_cls[l] = l < L ? grad_class_maps[l] : nullptr;
        a.g_box[l] = l < L ? grad_bbox_maps[l] : nullptr;
    }
    a.g_logits = grad_logits;
    a.g_probs = grad_probs;
    a.g_bbox = grad_bbox;
    a.probs = rpn_probs;
    hipLaunchKernelGGL(k_rpo_bwd, dim3((unsigned)a.T.tile[L], (unsigned)B), dim3(RPO_THREADS), sizeof(float) * (size_t)rpo_lds_floats(k),
                       (hipStream_t)stream, a);
    return check_launch("sdn_rpn_outputs_bwd");
}
