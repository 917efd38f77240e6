// The loss dict of a training step of the geometric branch: BaseNet.step_batch, /root/reference/geometric/scripts/main.py:114-154,
// with BaseNet.partial (:97-112) and Transforms.pad_like (derender3d/datasets.py:29-33).  The reference selects the items of a
// loss on the host (torch.nonzero, a branch on numel(), a branch on isnan().any(): two waits per loss, six losses), pads the
// batch's masks and ignore maps to the render size as copies and runs about a dozen element-wise launches each way.  Here
// `targets` is data and the padding is index arithmetic (train_loss_index.h):
//   forward   k_train_loss_partial  grid (item x chunk of rows): per-thread fp32 sums of (1 - ign) (render - mask)^2 and of ffd^2,
//                                   one fp64 pair per block into scratch; items outside sel_r are not read
//             k_train_loss_finish   one wave: the partials in block order, m_i, n_g, n_r, the four head losses, out[7]
//   backward  k_train_loss_grad     one launch for every gradient
// No atomics, nothing to zero: the same bits every run.  HBM-bound: one pass over _masks, masks and ignores each way.
#include <hip/hip_runtime.h>

#include "sdn_common.h"
#include "train_loss_index.h"

namespace sdn {

enum { TL_GEOMETRY = 1, TL_REPROJECT = 2 };   // TargetType.geometry / .reproject (derender3d/__init__.py)

// scratch, in doubles: n_g, n_r, m_i [B], then (sum of weighted squared errors, sum of ffd^2) per block [B * chunks]
__host__ __device__ inline long tl_partials_at(int B) { return 2 + (long)B; }

// four neighbouring pixels (y, x .. x + 3) of the padded target mask and ignore map
template <bool VS>
__device__ inline void tl_load4(const float* __restrict__ mk, const float* __restrict__ ig, int y, int x, int p, int S, float4& m,
                                float4& g)
{
    const int yy = tl_clamp(y, p, S);
    const bool yin = tl_inside(y, p, S);
    if (VS) {
        int edge = 0;
        const int v = tl_group(x, p, S, &edge);
        if (v >= 0) {
            g = *reinterpret_cast<const float4*>(ig + (long)yy * S + v);
            m = yin ? *reinterpret_cast<const float4*>(mk + (long)(y - p) * S + v) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const float e = ig[(long)yy * S + edge];
            g = make_float4(e, e, e, e);
            m = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        float mm[4], gg[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            gg[e] = ig[(long)yy * S + tl_clamp(x + e, p, S)];
            mm[e] = (yin && tl_inside(x + e, p, S)) ? mk[(long)(y - p) * S + (x + e - p)] : 0.f;
        }
        m = make_float4(mm[0], mm[1], mm[2], mm[3]);
        g = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
}

// VR: 16-byte loads of the rendered masks (R % 4 == 0, aligned); VS: of masks / ignores too (S % 4 == 0, p % 4 == 0, aligned)
template <bool VR, bool VS>
__global__ __launch_bounds__(TL_THREADS) void k_train_loss_partial(const float* __restrict__ render, const float* __restrict__ masks,
                                                                  const float* __restrict__ ignores,
                                                                  const int64_t* __restrict__ targets, const float* __restrict__ ffd,
                                                                  long nffd, int R, int S, int C, double* __restrict__ partial)
{
    __shared__ double red[2][TL_THREADS / 64];
    const int gb = blockIdx.x, item = gb / C, c = gb - item * C;
    const int p = (R - S) / 2;
    float s = 0.f, q = 0.f;
    if (targets[item] & TL_REPROJECT) {
        const int rows = tl_rows(R), y0 = c * rows, y1 = min(R, y0 + rows);
        const float* __restrict__ rd = render + (long)item * R * R;
        const float* __restrict__ mk = masks + (long)item * S * S;
        const float* __restrict__ ig = ignores + (long)item * S * S;
        if (VR) {
            const int R4 = R >> 2, n4 = (y1 - y0) * R4;
            for (int e = threadIdx.x; e < n4; e += TL_THREADS) {
                const int dy = e / R4, x = (e - dy * R4) << 2, y = y0 + dy;
                const float4 a = *reinterpret_cast<const float4*>(rd + (long)y * R + x);
                float4 m, g;
                tl_load4<VS>(mk, ig, y, x, p, S, m, g);
                s += (a.x - m.x) * (a.x - m.x) * (1.f - g.x);
                s += (a.y - m.y) * (a.y - m.y) * (1.f - g.y);
                s += (a.z - m.z) * (a.z - m.z) * (1.f - g.z);
                s += (a.w - m.w) * (a.w - m.w) * (1.f - g.w);
            }
        } else {
            const int n = (y1 - y0) * R;
            for (int e = threadIdx.x; e < n; e += TL_THREADS) {
                const int dy = e / R, x = e - dy * R, y = y0 + dy;
                const int yy = tl_clamp(y, p, S), xx = tl_clamp(x, p, S);
                const float m = (tl_inside(y, p, S) && tl_inside(x, p, S)) ? mk[(long)(y - p) * S + (x - p)] : 0.f;
                const float d = rd[(long)y * R + x] - m;
                s += d * d * (1.f - ig[(long)yy * S + xx]);
            }
        }
    }
    const long stride = (long)gridDim.x * TL_THREADS;
    for (long k = (long)gb * TL_THREADS + threadIdx.x; k < nffd; k += stride) q += ffd[k] * ffd[k];
    double ds = (double)s, dq = (double)q;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ds += __shfl_xor(ds, o, 64);
        dq += __shfl_xor(dq, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = ds;
        red[1][threadIdx.x >> 6] = dq;
    }
    __syncthreads();
    if (threadIdx.x < 2) partial[2 * (long)gb + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

struct TlHeads {   // predictions and batch entries of the four geometry terms
    const float *p_td, *p_t2, *p_ls, *p_ld, *thetas, *t2, *ls, *ld;
};

// (cos, sin) of the batch's angle, evaluated in double and rounded once: the correctly rounded fp32 target
__device__ inline void tl_theta_target(float theta, float& c, float& s)
{
    c = (float)cos((double)theta);
    s = (float)sin((double)theta);
}

__global__ __launch_bounds__(64) void k_train_loss_finish(TlHeads h, const float* __restrict__ logp, const int64_t* __restrict__ targets,
                                                          int B, int R, int C, long nffd, int mode, double mask_weight, double ffd_reg,
                                                          double* __restrict__ scratch, float* __restrict__ out)
{
    // lane l takes items l, l + 64, ... (and blocks l, l + 64, ... of the ffd partials), then a fixed butterfly
    enum { TD, T2, LS, LD, NG, NR, SM, SR, QF, NA };
    double a[NA];
#pragma unroll
    for (int k = 0; k < NA; k++) a[k] = 0.0;
    const double* __restrict__ partial = scratch + tl_partials_at(B);
    for (int i = threadIdx.x; i < B; i += 64) {
        const int64_t t = targets[i];
        if ((mode & TL_GEOMETRY) && (t & TL_GEOMETRY)) {
            float tc, ts;
            tl_theta_target(h.thetas[i], tc, ts);
            const double d0 = (double)h.p_td[2 * i] - (double)tc, d1 = (double)h.p_td[2 * i + 1] - (double)ts;
            a[TD] += d0 * d0 + d1 * d1;
            const double e0 = (double)h.p_t2[2 * i] - (double)h.t2[2 * i], e1 = (double)h.p_t2[2 * i + 1] - (double)h.t2[2 * i + 1];
            a[T2] += e0 * e0 + e1 * e1;
            double sl = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double d = (double)h.p_ls[3 * i + k] - (double)h.ls[3 * i + k];
                sl += d * d;
            }
            a[LS] += sl;
            const double dd = (double)h.p_ld[i] - (double)h.ld[i];
            a[LD] += dd * dd;
            a[NG] += 1.0;
        }
        if (mode & TL_REPROJECT) {
            double m = 0.0;
            if (t & TL_REPROJECT) {
                for (int c = 0; c < C; c++) m += partial[2 * ((long)i * C + c)];
                m = mask_weight * m / ((double)R * (double)R);
                a[NR] += 1.0;
                a[SM] += m;
                a[SR] += (double)logp[i] * m;
            }
            scratch[2 + i] = m;
        }
    }
    if (mode & TL_REPROJECT)
        for (long b = threadIdx.x; b < (long)B * C; b += 64) a[QF] += partial[2 * b + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < NA; k++) a[k] += __shfl_xor(a[k], o, 64);
    if (threadIdx.x == 0) {
        scratch[0] = a[NG];
        scratch[1] = a[NR];
        const bool g = a[NG] > 0.0, r = a[NR] > 0.0;   // an empty selection: exactly 0 (the torch.tensor(0.0) branch of `partial`)
        out[0] = g ? (float)(a[TD] / (2.0 * a[NG])) : 0.f;
        out[1] = g ? (float)(a[T2] / (2.0 * a[NG])) : 0.f;
        out[2] = g ? (float)(a[LS] / (3.0 * a[NG])) : 0.f;
        out[3] = g ? (float)(a[LD] / a[NG]) : 0.f;
        out[4] = r ? (float)(a[SR] / a[NR]) : 0.f;
        out[5] = r ? (float)(a[SM] / a[NR]) : 0.f;
        out[6] = (mode & TL_REPROJECT) ? (float)(ffd_reg * a[QF] / (double)nffd) : 0.f;
    }
}

struct TlGrads {
    float *td, *t2, *ls, *ld, *logp, *masks, *ffd;
};

template <bool VR, bool VS>
__global__ __launch_bounds__(TL_THREADS) void k_train_loss_grad(TlHeads h, const float* __restrict__ render, const float* __restrict__ masks,
                                                               const float* __restrict__ ignores, const int64_t* __restrict__ targets,
                                                               const float* __restrict__ ffd, long nffd, int B, int R, int S, int C,
                                                               int mode, double mask_weight, double ffd_reg,
                                                               const double* __restrict__ scratch, const float* __restrict__ gout,
                                                               TlGrads g)
{
    const double ng = scratch[0], nr = scratch[1];
    const int gb = blockIdx.x;
    if (g.masks) {   // grid: item x chunk of rows, as the forward's
        const int item = gb / C, c = gb - item * C;
        const int p = (R - S) / 2;
        const int rows = tl_rows(R), y0 = c * rows, y1 = min(R, y0 + rows);
        const bool sel = (mode & TL_REPROJECT) && (targets[item] & TL_REPROJECT) && nr > 0.0;
        const float sc = sel ? (float)((double)gout[5] * mask_weight * 2.0 / (nr * (double)R * (double)R)) : 0.f;
        const float* __restrict__ rd = render + (long)item * R * R;
        const float* __restrict__ mk = masks + (long)item * S * S;
        const float* __restrict__ ig = ignores + (long)item * S * S;
        float* __restrict__ gm = g.masks + (long)item * R * R;
        if (VR) {
            const int R4 = R >> 2, n4 = (y1 - y0) * R4;
            for (int e = threadIdx.x; e < n4; e += TL_THREADS) {
                const int dy = e / R4, x = (e - dy * R4) << 2, y = y0 + dy;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);   // items outside the selection: zeros, nothing is read
                if (sel) {
                    const float4 a = *reinterpret_cast<const float4*>(rd + (long)y * R + x);
                    float4 m, w;
                    tl_load4<VS>(mk, ig, y, x, p, S, m, w);
                    o = make_float4(sc * ((1.f - w.x) * (a.x - m.x)), sc * ((1.f - w.y) * (a.y - m.y)), sc * ((1.f - w.z) * (a.z - m.z)),
                                    sc * ((1.f - w.w) * (a.w - m.w)));
                }
                *reinterpret_cast<float4*>(gm + (long)y * R + x) = o;
            }
        } else {
            const int n = (y1 - y0) * R;
            for (int e = threadIdx.x; e < n; e += TL_THREADS) {
                const int dy = e / R, x = e - dy * R, y = y0 + dy;
                float o = 0.f;
                if (sel) {
                    const int yy = tl_clamp(y, p, S), xx = tl_clamp(x, p, S);
                    const float m = (tl_inside(y, p, S) && tl_inside(x, p, S)) ? mk[(long)(y - p) * S + (x - p)] : 0.f;
                    o = sc * ((1.f - ig[(long)yy * S + xx]) * (rd[(long)y * R + x] - m));
                }
                gm[(long)y * R + x] = o;
            }
        }
    }
    // the small gradients, strided over the whole grid
    const long first = (long)gb * TL_THREADS + threadIdx.x, stride = (long)gridDim.x * TL_THREADS;
    if (g.td || g.t2 || g.ls || g.ld || g.logp) {
        for (long i = first; i < B; i += stride) {
            const int64_t t = targets[i];
            const bool sg = (mode & TL_GEOMETRY) && (t & TL_GEOMETRY) && ng > 0.0;
            if (g.td) {
                float tc = 0.f, ts = 0.f;
                if (sg) tl_theta_target(h.thetas[i], tc, ts);
                const double k = sg ? (double)gout[0] / ng : 0.0;   // 2 (pred - target) / (2 n_g)
                g.td[2 * i] = sg ? (float)(k * ((double)h.p_td[2 * i] - (double)tc)) : 0.f;
                g.td[2 * i + 1] = sg ? (float)(k * ((double)h.p_td[2 * i + 1] - (double)ts)) : 0.f;
            }
            if (g.t2) {
                const double k = sg ? (double)gout[1] / ng : 0.0;
#pragma unroll
                for (int e = 0; e < 2; e++) g.t2[2 * i + e] = sg ? (float)(k * ((double)h.p_t2[2 * i + e] - (double)h.t2[2 * i + e])) : 0.f;
            }
            if (g.ls) {
                const double k = sg ? (double)gout[2] * 2.0 / (3.0 * ng) : 0.0;
#pragma unroll
                for (int e = 0; e < 3; e++) g.ls[3 * i + e] = sg ? (float)(k * ((double)h.p_ls[3 * i + e] - (double)h.ls[3 * i + e])) : 0.f;
            }
            if (g.ld) g.ld[i] = sg ? (float)((double)gout[3] * 2.0 / ng * ((double)h.p_ld[i] - (double)h.ld[i])) : 0.f;
            if (g.logp) {
                const bool sr = (mode & TL_REPROJECT) && (t & TL_REPROJECT) && nr > 0.0;
                g.logp[i] = sr ? (float)((double)gout[4] * scratch[2 + i] / nr) : 0.f;
            }
        }
    }
    if (g.ffd) {
        const bool on = (mode & TL_REPROJECT) != 0;
        const float sf = on ? (float)((double)gout[6] * 2.0 * ffd_reg / (double)nffd) : 0.f;
        for (long k = first; k < nffd; k += stride) g.ffd[k] = on ? sf * ffd[k] : 0.f;
    }
}

static bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

// 0 on success: the sizes both entry points accept
static int tl_check_sizes(const char* who, int B, int R, int S, long nffd, int mode)
{
    if (B < 1 || R < 1 || nffd < 0) return fail(SDN_EINVAL, "%s: bad sizes (B %d, R %d, nffd %ld)", who, B, R, nffd);
    if ((long)B * tl_chunks(R) > 0x7fffffffL) return fail(SDN_EINVAL, "%s: B %d x %d row chunks exceed the grid", who, B, tl_chunks(R));
    if (mode & TL_REPROJECT) {
        if (S < 1 || R < S || ((R - S) & 1))
            return fail(SDN_EINVAL, "%s: render size %d minus mask size %d must be even and >= 0 (pad_like pads (R - S) // 2 on both sides)",
                        who, R, S);
        if (nffd < 1) return fail(SDN_EINVAL, "%s: no ffd coefficients", who);
    }
    return SDN_OK;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_train_losses_scratch(int B, int R, long nffd, size_t* bytes)
{
    if (!bytes || B < 1 || R < 1 || nffd < 0) return fail(SDN_EINVAL, "sdn_train_losses_scratch: bad arguments");
    *bytes = (size_t)(tl_partials_at(B) + 2 * (long)B * tl_chunks(R)) * sizeof(double);
    return SDN_OK;
}

SDN_API int sdn_train_losses_fwd(const float* p_theta_deltas, const float* p_translation2ds, const float* p_log_scales,
                                 const float* p_log_depths, const float* p_class_log_probs, const float* p_masks, const float* p_ffd,
                                 long nffd, const float* thetas, const float* translation2ds, const float* log_scales,
                                 const float* log_depths, const float* masks, const float* ignores, const int64_t* targets, int B, int R,
                                 int S, int mode, double mask_weight, double ffd_coeff_reg, void* scratch, float* out, sdnStream stream)
{
    if (!targets || !scratch || !out || ((uintptr_t)scratch & 7)) return fail(SDN_EINVAL, "sdn_train_losses_fwd: bad arguments");
    if (int rc = tl_check_sizes("sdn_train_losses_fwd", B, R, S, nffd, mode)) return rc;
    if ((mode & TL_GEOMETRY) && (!p_theta_deltas || !p_translation2ds || !p_log_scales || !p_log_depths || !thetas || !translation2ds ||
                                 !log_scales || !log_depths))
        return fail(SDN_EINVAL, "sdn_train_losses_fwd: mode asks for the geometry terms, a pointer of theirs is NULL");
    if ((mode & TL_REPROJECT) && (!p_class_log_probs || !p_masks || !p_ffd || !masks || !ignores))
        return fail(SDN_EINVAL, "sdn_train_losses_fwd: mode asks for the reprojection terms, a pointer of theirs is NULL");
    hipStream_t st = (hipStream_t)stream;
    const int C = tl_chunks(R);
    double* sc = (double*)scratch;
    if (mode & TL_REPROJECT) {
        const bool vr = (R & 3) == 0 && aligned16(p_masks);
        const bool vs = vr && (S & 3) == 0 && (((R - S) / 2) & 3) == 0 && aligned16(masks) && aligned16(ignores);
        auto k = vs ? k_train_loss_partial<true, true> : (vr ? k_train_loss_partial<true, false> : k_train_loss_partial<false, false>);
        hipLaunchKernelGGL(k, dim3((unsigned)(B * C)), dim3(TL_THREADS), 0, st, p_masks, masks, ignores, targets, p_ffd, nffd, R, S, C,
                           sc + tl_partials_at(B));
    }
    const TlHeads h = {p_theta_deltas, p_translation2ds, p_log_scales, p_log_depths, thetas, translation2ds, log_scales, log_depths};
    hipLaunchKernelGGL(k_train_loss_finish, dim3(1), dim3(64), 0, st, h, p_class_log_probs, targets, B, R, C, nffd, mode, mask_weight,
                       ffd_coeff_reg, sc, out);
    return check_launch("k_train_loss_finish");
}

SDN_API int sdn_train_losses_bwd(const float* p_theta_deltas, const float* p_translation2ds, const float* p_log_scales,
                                 const float* p_log_depths, const float* p_masks, const float* p_ffd, long nffd, const float* thetas,
                                 const float* translation2ds, const float* log_scales, const float* log_depths, const float* masks,
                                 const float* ignores, const int64_t* targets, int B, int R, int S, int mode, double mask_weight,
                                 double ffd_coeff_reg, const void* scratch, const float* grad_out, float* grad_theta_deltas,
                                 float* grad_translation2ds, float* grad_log_scales, float* grad_log_depths, float* grad_class_log_probs,
                                 float* grad_masks, float* grad_ffd, sdnStream stream)
{
    if (!targets || !scratch || !grad_out || ((uintptr_t)scratch & 7)) return fail(SDN_EINVAL, "sdn_train_losses_bwd: bad arguments");
    if (int rc = tl_check_sizes("sdn_train_losses_bwd", B, R, S, nffd, mode)) return rc;
    const bool heads = grad_theta_deltas || grad_translation2ds || grad_log_scales || grad_log_depths;
    if (!heads && !grad_class_log_probs && !grad_masks && !grad_ffd) return fail(SDN_EINVAL, "sdn_train_losses_bwd: no gradient asked for");
    if ((mode & TL_GEOMETRY) && heads && (!p_theta_deltas || !p_translation2ds || !p_log_scales || !p_log_depths || !thetas ||
                                          !translation2ds || !log_scales || !log_depths))
        return fail(SDN_EINVAL, "sdn_train_losses_bwd: mode asks for the geometry terms, a pointer of theirs is NULL");
    if ((mode & TL_REPROJECT) && ((grad_masks && (!p_masks || !masks || !ignores)) || (grad_ffd && !p_ffd)))
        return fail(SDN_EINVAL, "sdn_train_losses_bwd: mode asks for the reprojection terms, a pointer of theirs is NULL");
    const int C = tl_chunks(R);
    long blocks = (long)B * C;
    if (!grad_masks) {
        const long small = nffd > B ? nffd : B;
        blocks = (small + TL_THREADS - 1) / TL_THREADS;
        blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    }
    const bool vr = (R & 3) == 0 && aligned16(p_masks) && aligned16(grad_masks);
    const bool vs = vr && (S & 3) == 0 && (((R - S) / 2) & 3) == 0 && aligned16(masks) && aligned16(ignores);
    auto k = vs ? k_train_loss_grad<true, true> : (vr ? k_train_loss_grad<true, false> : k_train_loss_grad<false, false>);
    const TlHeads h = {p_theta_deltas, p_translation2ds, p_log_scales, p_log_depths, thetas, translation2ds, log_scales, log_depths};
    const TlGrads g = {grad_theta_deltas, grad_translation2ds, grad_log_scales, grad_log_depths, grad_class_log_probs, grad_masks, grad_ffd};
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(TL_THREADS), 0, (hipStream_t)stream, h, p_masks, masks, ignores, targets, p_ffd, nffd,
                       B, R, S, C, mode, mask_weight, ffd_coeff_reg, (const double*)scratch, grad_out, g);
    return check_launch("k_train_loss_grad");
}
