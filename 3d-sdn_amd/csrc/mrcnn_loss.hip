// The five training losses of Mask R-CNN: compute_losses (geometric/maskrcnn/model.py:1004-1147) and their sum (:1955).  The
// reference finds the contributing anchors and RoIs with four torch.nonzero calls (:1020, 1047, 1091, 1121; each waits for the
// device), gathers [A, 2], [A, 4], [R, C, 4] and [R, C, h, w] tensors through index tensors, runs cross_entropy twice,
// smooth_l1_loss twice and binary_cross_entropy once, and backward turns every gather into a zero fill and an index_put.  Here:
//   forward   k_mrl_count    one wave per chunk of MRL_CHUNK anchors: the chunk's positive anchors into a table
//             k_mrl_partial  the same chunks, then one wave per RoI.  A chunk's wave re-adds the table entries before it (no
//                            workgroup waits for another), so the k-th positive anchor in anchor order knows k, its row of the
//                            RPN box targets (:1053).  Per workgroup fp64 sums and integer counts into the workspace; the
//                            chunks' prefixes and the RoIs' log-sum-exps into `saved`
//             k_mrl_finish   one wave: the partials in block order; out[6], counts[4], the head of `saved`
//   backward  k_mrl_grad     one launch: chunks (d rpn_class_logits, d rpn_pred_bbox), RoIs (d mrcnn_class_logits, d mrcnn_bbox),
//                            (RoI, class) planes (d mrcnn_mask); every element written once, +0.0 outside the selections
// Per element the arithmetic is fp64 (the selections are a few hundred anchors and RoIs; the tensors are HBM-bound), rounded to fp32
// once.  A lane owns four adjacent anchors: one 16-byte load of rpn_match (int32), two of the logits, one per box row, when the
// bases are 16-byte aligned; mask planes likewise when h * w % 4 == 0.  No atomics, nothing to zero: the same bits every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "mrcnn_loss_check.h"
#include "sdn_common.h"

namespace sdn {

__device__ __forceinline__ void mrl_load4(const float* __restrict__ p, bool vec, float (&v)[4])
{
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

__device__ __forceinline__ void mrl_store4(float* __restrict__ p, bool vec, const float (&v)[4])
{
    if (vec) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

// the kinds (mrl_match_kind) of the four anchors from a0; an anchor beyond A is neutral
__device__ __forceinline__ void mrl_kinds(const void* __restrict__ match, int i64, bool vec, long a0, long A, int (&kind)[4])
{
    if (vec && a0 + MRL_QUAD <= A) {
        if (i64) {
            const longlong2* p = reinterpret_cast<const longlong2*>(static_cast<const int64_t*>(match) + a0);
            const longlong2 l0 = p[0], l1 = p[1];
            kind[0] = mrl_match_kind(l0.x); kind[1] = mrl_match_kind(l0.y); kind[2] = mrl_match_kind(l1.x); kind[3] = mrl_match_kind(l1.y);
        } else {
            const int4 q = *reinterpret_cast<const int4*>(static_cast<const int32_t*>(match) + a0);
            kind[0] = mrl_match_kind(q.x); kind[1] = mrl_match_kind(q.y); kind[2] = mrl_match_kind(q.z); kind[3] = mrl_match_kind(q.w);
        }
    } else {
#pragma unroll
        for (int e = 0; e < MRL_QUAD; e++) {
            const long a = a0 + e;
            long long v = 0;
            if (a < A) v = i64 ? (long long)static_cast<const int64_t*>(match)[a] : (long long)static_cast<const int32_t*>(match)[a];
            kind[e] = mrl_match_kind(v);
        }
    }
}

__device__ __forceinline__ int mrl_positives(const int (&kind)[4])
{
    return (kind[0] == 1) + (kind[1] == 1) + (kind[2] == 1) + (kind[3] == 1);
}

// the two logits of each of the four anchors from a0 (zeros beyond A)
__device__ __forceinline__ void mrl_logits(const float* __restrict__ x, bool vec, long a0, long A, float (&v)[8])
{
    if (vec && a0 + MRL_QUAD <= A) {
        const float4* p = reinterpret_cast<const float4*>(x + 2 * a0);
        const float4 q0 = p[0], q1 = p[1];
        v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    } else {
#pragma unroll
        for (int e = 0; e < 2 * MRL_QUAD; e++) v[e] = a0 + e / 2 < A ? x[2 * a0 + e] : 0.f;
    }
}

// log(exp(a) + exp(b))
__device__ __forceinline__ double mrl_lse2(double a, double b)
{
    const double m = a > b ? a : b;
    return m + log(exp(a - m) + exp(b - m));
}

// smooth L1 with beta 1 (torch: quadratic for |d| < 1) and its derivative
__device__ __forceinline__ double mrl_smooth_l1(double d)
{
    const double z = fabs(d);
    return z < 1.0 ? 0.5 * z * z : z - 0.5;
}

__device__ __forceinline__ double mrl_smooth_l1_grad(double d) { return d < -1.0 ? -1.0 : d > 1.0 ? 1.0 : d; }

// torch's binary_cross_entropy on one element: each log clamped at -100 (a NaN stays: a probability outside [0, 1])
__device__ __forceinline__ double mrl_bce(double p, double y)
{
    double l1 = log(p), l0 = log1p(-p);
    l1 = l1 < -100.0 ? -100.0 : l1;
    l0 = l0 < -100.0 ? -100.0 : l0;
    return (y - 1.0) * l0 - y * l1;
}

__device__ __forceinline__ double mrl_bce_grad(double p, double y)
{
    const double q = (1.0 - p) * p, least = (double)1e-12f;   // torch's constant is a float, whatever the tensor's type
    return (p - y) / (q > least ? q : least);
}

__device__ __forceinline__ long long mrl_id(const void* __restrict__ ids, int i64, int r)
{
    return i64 ? (long long)static_cast<const int64_t*>(ids)[r] : (long long)static_cast<const int32_t*>(ids)[r];
}

struct MrlRpn {
    const void* match;
    int match_i64;
    const float *target, *logits, *pred;
    int A, T;
    bool vec;   // match, logits, pred and target are all 16-byte aligned
};

struct MrlHead {
    const void* ids;
    int ids_i64;
    const float *logits, *deltas, *bbox, *tmask, *mask;
    int R, C;
    long HW;
    bool vec_box, vec_mask;   // deltas and bbox (and the bbox gradient) / the two mask tensors (and the gradient) aligned, HW % 4 == 0
};

// first pass: the positives of every chunk
__global__ __launch_bounds__(MRL_THREADS) void k_mrl_count(const void* __restrict__ match, int i64, bool vec, int A, int* __restrict__ table)
{
    const int chunk = blockIdx.x, lane = threadIdx.x;
    int n = 0;
#pragma unroll
    for (int s = 0; s < MRL_STEPS; s++) {
        int kind[4];
        mrl_kinds(match, i64, vec, mrl_quad_first(chunk, s, lane), A, kind);
        n += mrl_positives(kind);
    }
    n = wave_sum(n);
    if (lane == 0) table[chunk] = n;
}

__device__ __forceinline__ void mrl_rpn_partial(const MrlRpn& q, int chunk, int lane, const int* __restrict__ table, int* __restrict__ prefix,
                                                double* __restrict__ psum, int* __restrict__ pcnt)
{
    int before = 0;
    for (int i = lane; i < chunk; i += MRL_THREADS) before += table[i];
    before = wave_sum(before);
    if (lane == 0) prefix[chunk] = before;
    double s_cls = 0.0, s_box = 0.0;
    int valid = 0, used = 0, bad = 0;
    for (int s = 0; s < MRL_STEPS; s++) {
        const long a0 = mrl_quad_first(chunk, s, lane);
        int kind[4], total;
        mrl_kinds(q.match, q.match_i64, q.vec, a0, q.A, kind);
        int rank = before + wave_exclusive_sum(mrl_positives(kind), lane, total);
        before += total;
        if (a0 >= q.A) continue;
        float x[8];
        mrl_logits(q.logits, q.vec, a0, q.A, x);
#pragma unroll
        for (int e = 0; e < MRL_QUAD; e++) {
            if (kind[e] == 2) bad++;
            if (kind[e] == 1 || kind[e] == -1) {
                const double x0 = x[2 * e], x1 = x[2 * e + 1];
                s_cls += mrl_lse2(x0, x1) - (kind[e] == 1 ? x1 : x0);
                valid++;
            }
            if (kind[e] == 1) {
                if (rank < q.T) {
                    float p[4], t[4];
                    mrl_load4(q.pred + 4 * (a0 + e), q.vec, p);
                    mrl_load4(q.target + 4 * (long)rank, q.vec, t);
#pragma unroll
                    for (int k = 0; k < 4; k++) s_box += mrl_smooth_l1((double)p[k] - (double)t[k]);
                    used++;
                } else {
                    bad++;   // more positives than target rows
                }
                rank++;
            }
        }
    }
    s_cls = wave_sum(s_cls);
    s_box = wave_sum(s_box);
    valid = wave_sum(valid);
    used = wave_sum(used);
    bad = wave_sum(bad);
    if (lane == 0) {
        psum[0] = s_cls; psum[1] = s_box; psum[2] = 0.0;
        pcnt[0] = valid; pcnt[1] = used; pcnt[2] = bad; pcnt[3] = 0;
    }
}

__device__ __forceinline__ void mrl_roi_partial(const MrlHead& q, int r, int lane, double* __restrict__ lse_out, double* __restrict__ psum,
                                                int* __restrict__ pcnt)
{
    const long long id = mrl_id(q.ids, q.ids_i64, r);
    const int kind = mrl_roi_kind(id, q.C);
    // class: the row's log-sum-exp, two logits per lane
    const float* row = q.logits + (long)r * q.C;
    const double ninf = -__builtin_huge_val();
    const double x0 = lane < q.C ? (double)row[lane] : ninf, x1 = lane + 64 < q.C ? (double)row[lane + 64] : ninf;
    const double m = wave_max_greater(x0 > x1 ? x0 : x1);
    const double lse = m + log(wave_sum(exp(x0 - m) + exp(x1 - m)));
    double s_cls = 0.0, s_box = 0.0, s_mask = 0.0;
    if (kind >= 0) s_cls = lse - (double)row[id];
    if (kind == 1) {
        if (lane == 0) {
            float p[4], t[4];
            mrl_load4(q.bbox + 4 * ((long)r * q.C + id), q.vec_box, p);
            mrl_load4(q.deltas + 4 * (long)r, q.vec_box, t);
#pragma unroll
            for (int k = 0; k < 4; k++) s_box += mrl_smooth_l1((double)p[k] - (double)t[k]);
        }
        const float* pm = q.mask + ((long)r * q.C + id) * q.HW;
        const float* ym = q.tmask + (long)r * q.HW;
        if (q.vec_mask) {
            for (long i = 4 * lane; i < q.HW; i += MRL_STEP) {
                float p[4], y[4];
                mrl_load4(pm + i, true, p);
                mrl_load4(ym + i, true, y);
#pragma unroll
                for (int k = 0; k < 4; k++) s_mask += mrl_bce(p[k], y[k]);
            }
        } else {
            for (long i = lane; i < q.HW; i += MRL_THREADS) s_mask += mrl_bce(pm[i], ym[i]);
        }
        s_mask = wave_sum(s_mask);
    }
    if (lane == 0) {
        lse_out[r] = lse;
        psum[0] = s_cls; psum[1] = s_box; psum[2] = s_mask;
        pcnt[0] = kind >= 0; pcnt[1] = kind == 1; pcnt[2] = kind < 0; pcnt[3] = 0;
    }
}

__global__ __launch_bounds__(MRL_THREADS) void k_mrl_partial(MrlRpn rpn, MrlHead head, int chunks, void* __restrict__ workspace,
                                                             void* __restrict__ saved)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    const long nblk = (long)chunks + head.R;
    double* psum = reinterpret_cast<double*>(static_cast<char*>(workspace) + mrl_sum_at(g));
    int* pcnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + mrl_cnt_at(nblk, g));
    if (g < chunks) {
        const int* table = reinterpret_cast<const int*>(static_cast<char*>(workspace) + mrl_table_at(nblk));
        int* prefix = reinterpret_cast<int*>(static_cast<char*>(saved) + mrl_prefix_at(head.R, 0));
        mrl_rpn_partial(rpn, g, lane, table, prefix, psum, pcnt);
    } else {
        double* lse = reinterpret_cast<double*>(static_cast<char*>(saved) + mrl_lse_at(0));
        mrl_roi_partial(head, g - chunks, lane, lse, psum, pcnt);
    }
}

__global__ __launch_bounds__(64) void k_mrl_finish(const void* __restrict__ workspace, int chunks, int R, long HW, float* __restrict__ out,
                                                   int64_t* __restrict__ counts, void* __restrict__ saved)
{
    // lane l takes the workgroups l, l + 64, ... of each kind in order, then a fixed butterfly
    const long nblk = (long)chunks + R;
    const char* ws = static_cast<const char*>(workspace);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int n[6] = {0, 0, 0, 0, 0, 0};   // rpn valid, rpn positives used, rpn bad, roi valid, roi positive, roi bad
    for (long g = threadIdx.x; g < nblk; g += 64) {
        const double* ps = reinterpret_cast<const double*>(ws + mrl_sum_at(g));
        const int* pc = reinterpret_cast<const int*>(ws + mrl_cnt_at(nblk, g));
        if (g < chunks) {
            s[0] += ps[0]; s[1] += ps[1];
            n[0] += pc[0]; n[1] += pc[1]; n[2] += pc[2];
        } else {
            s[2] += ps[0]; s[3] += ps[1]; s[4] += ps[2];
            n[3] += pc[0]; n[4] += pc[1]; n[5] += pc[2];
        }
    }
#pragma unroll
    for (int i = 0; i < 5; i++) s[i] = wave_sum(s[i]);
#pragma unroll
    for (int i = 0; i < 6; i++) n[i] = wave_sum(n[i]);
    if (threadIdx.x == 0) {
        // torch's means: 0 / 0 = NaN over an empty selection; with R = 0 the head losses are 0 (model.py:1070, 1088, 1118)
        double l[5];
        l[0] = s[0] / (double)n[0];
        l[1] = s[1] / (4.0 * (double)n[1]);
        l[2] = R ? s[2] / (double)n[3] : 0.0;
        l[3] = R ? s[3] / (4.0 * (double)n[4]) : 0.0;
        l[4] = R ? s[4] / ((double)n[4] * (double)HW) : 0.0;
        for (int i = 0; i < 5; i++) out[i] = (float)l[i];
        out[5] = (float)(l[0] + l[1] + l[2] + l[3] + l[4]);   // model.py:1955, rounded once
        counts[0] = n[0];
        counts[1] = n[1];
        counts[2] = n[4];
        counts[3] = (int64_t)n[2] + n[5];
        int* head = static_cast<int*>(saved);
        head[0] = n[0]; head[1] = n[1]; head[2] = n[3]; head[3] = n[4];
    }
}

struct MrlGrads {
    float *rpn_logits, *rpn_pred, *logits, *bbox, *mask;
    bool vec_rpn;   // the RPN gradients given are 16-byte aligned
};

__device__ __forceinline__ void mrl_rpn_grad(const MrlRpn& q, const MrlGrads& g, int chunk, int lane, int before, double g_cls, double g_box)
{
    const bool vec = q.vec && g.vec_rpn;
    for (int s = 0; s < MRL_STEPS; s++) {
        const long a0 = mrl_quad_first(chunk, s, lane);
        int kind[4], total;
        mrl_kinds(q.match, q.match_i64, q.vec, a0, q.A, kind);
        int rank = before + wave_exclusive_sum(mrl_positives(kind), lane, total);
        before += total;
        if (a0 >= q.A) continue;
        const bool full = a0 + MRL_QUAD <= q.A;
        if (g.rpn_logits) {
            float x[8], d[8];
            mrl_logits(q.logits, q.vec, a0, q.A, x);
#pragma unroll
            for (int e = 0; e < MRL_QUAD; e++) {
                d[2 * e] = d[2 * e + 1] = 0.f;
                if (kind[e] == 1 || kind[e] == -1) {
                    const double x0 = x[2 * e], x1 = x[2 * e + 1], lse = mrl_lse2(x0, x1);
                    d[2 * e] = (float)((exp(x0 - lse) - (kind[e] == 1 ? 0.0 : 1.0)) * g_cls);
                    d[2 * e + 1] = (float)((exp(x1 - lse) - (kind[e] == 1 ? 1.0 : 0.0)) * g_cls);
                }
            }
            float* o = g.rpn_logits + 2 * a0;
            if (vec && full) {
                reinterpret_cast<float4*>(o)[0] = make_float4(d[0], d[1], d[2], d[3]);
                reinterpret_cast<float4*>(o)[1] = make_float4(d[4], d[5], d[6], d[7]);
            } else {
#pragma unroll
                for (int e = 0; e < 2 * MRL_QUAD; e++)
                    if (a0 + e / 2 < q.A) o[e] = d[e];
            }
        }
#pragma unroll
        for (int e = 0; e < MRL_QUAD; e++) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (kind[e] == 1) {
                if (rank < q.T && g.rpn_pred) {
                    float p[4], t[4];
                    mrl_load4(q.pred + 4 * (a0 + e), q.vec, p);
                    mrl_load4(q.target + 4 * (long)rank, q.vec, t);
#pragma unroll
                    for (int k = 0; k < 4; k++) d[k] = (float)(mrl_smooth_l1_grad((double)p[k] - (double)t[k]) * g_box);
                }
                rank++;
            }
            if (g.rpn_pred && a0 + e < q.A) mrl_store4(g.rpn_pred + 4 * (a0 + e), vec, d);
        }
    }
}

__device__ __forceinline__ void mrl_roi_grad(const MrlHead& q, const MrlGrads& g, int r, int lane, const double* __restrict__ lse,
                                             double g_cls, double g_box)
{
    const long long id = mrl_id(q.ids, q.ids_i64, r);
    const int kind = mrl_roi_kind(id, q.C);
    if (g.logits) {
        const float* row = q.logits + (long)r * q.C;
        const double l = lse[r];
        for (int c = lane; c < q.C; c += MRL_THREADS)
            g.logits[(long)r * q.C + c] = kind >= 0 ? (float)((exp((double)row[c] - l) - (c == id ? 1.0 : 0.0)) * g_cls) : 0.f;
    }
    if (g.bbox) {
        for (int c = lane; c < q.C; c += MRL_THREADS) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (kind == 1 && c == id) {
                float p[4], t[4];
                mrl_load4(q.bbox + 4 * ((long)r * q.C + c), q.vec_box, p);
                mrl_load4(q.deltas + 4 * (long)r, q.vec_box, t);
#pragma unroll
                for (int k = 0; k < 4; k++) d[k] = (float)(mrl_smooth_l1_grad((double)p[k] - (double)t[k]) * g_box);
            }
            mrl_store4(g.bbox + 4 * ((long)r * q.C + c), q.vec_box, d);
        }
    }
}

// one class plane of one RoI's mask gradient
__device__ __forceinline__ void mrl_mask_grad(const MrlHead& q, const MrlGrads& g, int r, int c, int lane, double g_mask)
{
    const long long id = mrl_id(q.ids, q.ids_i64, r);
    const bool sel = mrl_roi_kind(id, q.C) == 1 && c == id;
    const long at = ((long)r * q.C + c) * q.HW;
    const float* pm = q.mask + at;
    const float* ym = q.tmask + (long)r * q.HW;
    float* o = g.mask + at;
    if (q.vec_mask) {
        for (long i = 4 * lane; i < q.HW; i += MRL_STEP) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (sel) {
                float p[4], y[4];
                mrl_load4(pm + i, true, p);
                mrl_load4(ym + i, true, y);
#pragma unroll
                for (int k = 0; k < 4; k++) d[k] = (float)(mrl_bce_grad(p[k], y[k]) * g_mask);
            }
            mrl_store4(o + i, true, d);
        }
    } else {
        for (long i = lane; i < q.HW; i += MRL_THREADS) o[i] = sel ? (float)(mrl_bce_grad(pm[i], ym[i]) * g_mask) : 0.f;
    }
}

// grid: n_rpn chunk workgroups (0 when neither RPN gradient is asked for), then n_roi RoI workgroups, then R * C plane workgroups
__global__ __launch_bounds__(MRL_THREADS) void k_mrl_grad(MrlRpn rpn, MrlHead head, MrlGrads g, int n_rpn, int n_roi,
                                                          const void* __restrict__ saved, const float* __restrict__ gout)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int* cnt = static_cast<const int*>(saved);   // n_rpn_valid, n_rpn_pos, n_roi_valid, n_roi_pos
    const double top = gout[5];
    // an empty selection: the quotient is never used, every element gets +0.0
    if (b < n_rpn) {
        const int* prefix = reinterpret_cast<const int*>(static_cast<const char*>(saved) + mrl_prefix_at(head.R, 0));
        mrl_rpn_grad(rpn, g, b, lane, prefix[b], ((double)gout[0] + top) / (double)cnt[0], ((double)gout[1] + top) / (4.0 * (double)cnt[1]));
    } else if (b < n_rpn + n_roi) {
        const double* lse = reinterpret_cast<const double*>(static_cast<const char*>(saved) + mrl_lse_at(0));
        mrl_roi_grad(head, g, b - n_rpn, lane, lse, ((double)gout[2] + top) / (double)cnt[2], ((double)gout[3] + top) / (4.0 * (double)cnt[3]));
    } else {
        const int p = b - n_rpn - n_roi, r = p / head.C, c = p - r * head.C;
        mrl_mask_grad(head, g, r, c, lane, ((double)gout[4] + top) / ((double)cnt[3] * (double)head.HW));
    }
}

static bool mrl_aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

static MrlRpn mrl_rpn_of(const MrlInputs& in, int A, int T)
{
    MrlRpn q;
    q.match = in.rpn_match;
    q.match_i64 = in.match_i64;
    q.target = static_cast<const float*>(in.rpn_bbox);
    q.logits = static_cast<const float*>(in.rpn_class_logits);
    q.pred = static_cast<const float*>(in.rpn_pred_bbox);
    q.A = A;
    q.T = T;
    q.vec = mrl_aligned16(in.rpn_match) && mrl_aligned16(in.rpn_bbox) && mrl_aligned16(in.rpn_class_logits) && mrl_aligned16(in.rpn_pred_bbox);
    return q;
}

static MrlHead mrl_head_of(const MrlInputs& in, int R, int C, int h, int w, const float* g_bbox, const float* g_mask)
{
    MrlHead q;
    q.ids = in.target_class_ids;
    q.ids_i64 = in.ids_i64;
    q.logits = static_cast<const float*>(in.mrcnn_class_logits);
    q.deltas = static_cast<const float*>(in.target_deltas);
    q.bbox = static_cast<const float*>(in.mrcnn_bbox);
    q.tmask = static_cast<const float*>(in.target_mask);
    q.mask = static_cast<const float*>(in.mrcnn_mask);
    q.R = R;
    q.C = R ? C : 0;
    q.HW = R ? (long)h * w : 0;
    q.vec_box = mrl_aligned16(in.target_deltas) && mrl_aligned16(in.mrcnn_bbox) && mrl_aligned16(g_bbox);
    q.vec_mask = (q.HW & 3) == 0 && mrl_aligned16(in.target_mask) && mrl_aligned16(in.mrcnn_mask) && mrl_aligned16(g_mask);
    return q;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_mrcnn_loss_workspace_bytes(int A, int R, size_t* workspace_bytes, size_t* saved_bytes)
{
    if (!workspace_bytes || !saved_bytes) return fail(SDN_EINVAL, "sdn_mrcnn_loss_workspace_bytes: NULL result pointer");
    if (A < 1 || A > MRL_MAX_ANCHORS || R < 0) return fail(SDN_EINVAL, "sdn_mrcnn_loss_workspace_bytes: bad sizes: A %d, R %d", A, R);
    *workspace_bytes = mrl_workspace_bytes(A, R);
    *saved_bytes = mrl_saved_bytes(A, R);
    return SDN_OK;
}

SDN_API int sdn_mrcnn_loss_fwd(const void* rpn_match, int match_i64, const float* rpn_bbox, const float* rpn_class_logits,
                               const float* rpn_pred_bbox, int batch, int A, int T, const void* target_class_ids, int ids_i64,
                               const float* mrcnn_class_logits, const float* target_deltas, const float* mrcnn_bbox, const float* target_mask,
                               const float* mrcnn_mask, int R, int C, int h, int w, void* workspace, size_t workspace_bytes, void* saved,
                               size_t saved_bytes, float* out, int64_t* counts, sdnStream stream)
{
    const MrlInputs in = {rpn_match, match_i64, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, ids_i64,
                          mrcnn_class_logits, target_deltas, mrcnn_bbox, target_mask, mrcnn_mask};
    char why[256];
    if (mrl_validate_fwd(in, batch, A, T, R, C, h, w, workspace, workspace_bytes, saved, saved_bytes, out, counts, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_mrcnn_loss_fwd: %s", why);
    hipStream_t st = (hipStream_t)stream;
    const MrlRpn rpn = mrl_rpn_of(in, A, T);
    const MrlHead head = mrl_head_of(in, R, C, h, w, nullptr, nullptr);
    const int chunks = mrl_chunks(A);
    const long nblk = mrl_blocks(A, R);
    int* table = reinterpret_cast<int*>(static_cast<char*>(workspace) + mrl_table_at(nblk));
    hipLaunchKernelGGL(k_mrl_count, dim3((unsigned)chunks), dim3(MRL_THREADS), 0, st, rpn_match, match_i64, rpn.vec, A, table);
    if (int rc = check_launch("k_mrl_count")) return rc;
    hipLaunchKernelGGL(k_mrl_partial, dim3((unsigned)nblk), dim3(MRL_THREADS), 0, st, rpn, head, chunks, workspace, saved);
    if (int rc = check_launch("k_mrl_partial")) return rc;
    hipLaunchKernelGGL(k_mrl_finish, dim3(1), dim3(64), 0, st, workspace, chunks, R, head.HW, out, counts, saved);
    return check_launch("k_mrl_finish");
}

SDN_API int sdn_mrcnn_loss_bwd(const void* rpn_match, int match_i64, const float* rpn_bbox, const float* rpn_class_logits,
                               const float* rpn_pred_bbox, int batch, int A, int T, const void* target_class_ids, int ids_i64,
                               const float* mrcnn_class_logits, const float* target_deltas, const float* mrcnn_bbox, const float* target_mask,
                               const float* mrcnn_mask, int R, int C, int h, int w, const void* saved, size_t saved_bytes,
                               const float* grad_out, float* grad_rpn_class_logits, float* grad_rpn_pred_bbox,
                               float* grad_mrcnn_class_logits, float* grad_mrcnn_bbox, float* grad_mrcnn_mask, sdnStream stream)
{
    const MrlInputs in = {rpn_match, match_i64, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, ids_i64,
                          mrcnn_class_logits, target_deltas, mrcnn_bbox, target_mask, mrcnn_mask};
    const void* const gs[5] = {grad_rpn_class_logits, grad_rpn_pred_bbox, grad_mrcnn_class_logits, grad_mrcnn_bbox, grad_mrcnn_mask};
    char why[256];
    if (mrl_validate_bwd(in, batch, A, T, R, C, h, w, saved, saved_bytes, grad_out, gs, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_mrcnn_loss_bwd: %s", why);
    hipStream_t st = (hipStream_t)stream;
    const MrlRpn rpn = mrl_rpn_of(in, A, T);
    const MrlHead head = mrl_head_of(in, R, C, h, w, grad_mrcnn_bbox, grad_mrcnn_mask);
    MrlGrads g;
    g.rpn_logits = grad_rpn_class_logits;
    g.rpn_pred = grad_rpn_pred_bbox;
    g.logits = grad_mrcnn_class_logits;
    g.bbox = grad_mrcnn_bbox;
    g.mask = grad_mrcnn_mask;
    g.vec_rpn = mrl_aligned16(grad_rpn_class_logits) && mrl_aligned16(grad_rpn_pred_bbox);
    const int n_rpn = (g.rpn_logits || g.rpn_pred) ? mrl_chunks(A) : 0;
    const int n_roi = (g.logits || g.bbox) ? R : 0;
    const long n_mask = g.mask ? (long)R * C : 0;
    hipLaunchKernelGGL(k_mrl_grad, dim3((unsigned)(n_rpn + n_roi + n_mask)), dim3(MRL_THREADS), 0, st, rpn, head, g, n_rpn, n_roi, saved,
                       grad_out);
    return check_launch("k_mrl_grad");
}
