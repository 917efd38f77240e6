// The Derenderer's heads, forward and backward: net.fc, ReLU, the cat with the two roi vectors, fc1, ReLU, fc2, ReLU, _fc3, the six
// slices, the pose pair's normalisation and the class softmax (reference: geometric/derender3d/models/derenderer.py:33-65), with the
// roi centre / extent arithmetic in front of it (geometric/derender3d/models/__init__.py:99-106).  Through torch that is about twenty
// launches forward and twice that backward for 17 MFLOP on 2.6 MB of weights; here it is four launches each way, fp32 throughout,
// without atomics, memsets or a wait of one workgroup for another.  The weights are read in nn.Linear's own [out, in] layout.
//
// Forward, one launch per layer (k_dh_fwd).  A workgroup owns DH_ROWS = 16 objects and 16 output columns: it stages the 16 input rows
// in the LDS, 256 columns at a time; each group of 16 lanes owns one output column and reads its weight row 16 bytes per lane (256
// contiguous bytes per group), so lane s of the group sums the terms k = 64 i + 4 s + c (i ascending, c = 0 .. 3) as one fmaf chain per
// object; the 16 partial sums of an (object, column) go through the LDS and are added s = 0 .. 15, then the bias.  The last layer's
// first workgroup owns the 8 + classes leading columns (two passes), so that the pose pair and the logits of an object meet in its
// LDS: delta / sqrt(r0^2 + r1^2) (a zero pair gives NaN, as the formula does) and expf(x - max) / sum with one expf per element (a
// non-finite logit follows the formula); the other workgroups write 16 coefficient columns each.
//
// Backward (k_dh_bwd), four launches.  A workgroup is one of two kinds.  An input-gradient workgroup owns 16 objects, 64 columns of
// the layer's input and one slab of DH_SLAB = 128 terms of the sum over the layer's outputs: its four waves take 64 terms of a staged
// chunk each, lane j reads W[k][j] (coalesced), the four waves' sums are added w = 0 .. 3 through the LDS and written as a partial
// sum P[slab][object][column].  Nobody waits for the other slabs: whoever consumes the hidden gradient in the NEXT launch adds the
// slabs s = 0, 1, .. itself and applies the ReLU mask (dh_g).  A weight-gradient workgroup owns 8 weight rows and 256 weight columns
// and walks the objects r = 0, 1, .. n - 1 in that order, one fmaf chain per weight; the bias gradient is the same walk.  The
// gradient of the output row is not stored either: every consumer undoes the normalisation, (g - d (d.g)) / norm, and the softmax,
// p (g - sum p g), where it stages it.  A NULL output gradient is not read; a NULL input gradient's workgroups are not launched.
//
// Every sum's order follows from the widths alone (the object walk of a weight gradient: from the object's index), so the bits are the
// same every run and an object's outputs do not depend on the batch it is in.  Built without FMA contraction: every multiply-add is
// an explicit fmaf.
#include <hip/hip_runtime.h>

#include "derender_heads_check.h"
#include "sdn_common.h"

namespace sdn {

enum { DH_HIDDEN = 0, DH_ROW = 1 };
enum { DH_G_ROW = 0, DH_G_SLABS = 1 };

constexpr int DH_FWD_LDS = DH_ROWS * DH_KC + DH_ROWS * DH_COLS * 17 + DH_ROWS * 32;   // floats: input tile, partial sums, head columns
constexpr int DH_BWD_LDS = DH_ROWS * DH_KC + 4 * DH_ROWS * DH_DCOLS;                  // floats: gradient tile, the four waves' sums

// A layer's input row: columns [0, K0) from x, then (fc1 only) the roi centre and extent, from roi_norms or as given
struct DhX {
    const float* x;
    int ldx, K0;
    const float *roi, *centre, *extent;
};

__device__ __forceinline__ float dh_x(const DhX& s, int row, int k)
{
    if (k < s.K0) return s.x[(size_t)row * s.ldx + k];
    const int c = k - s.K0;   // 0, 1: centre; 2, 3: extent
    if (s.roi) {
        const float tl = s.roi[row * 4 + (c & 1)], br = s.roi[row * 4 + 2 + (c & 1)];
        return c < 2 ? (br + tl) / 2.0f : br - tl;
    }
    return c < 2 ? s.centre[row * 2 + c] : s.extent[row * 2 + c - 2];
}

// The gradient of a layer's pre-activation.  DH_G_ROW: of the output row, from the six output gradients (each may be NULL).
// DH_G_SLABS: of a hidden layer, the slabs added in order, masked by the layer's activation.
struct DhG {
    int kind, n;
    const float *g_theta, *g_trans, *g_scales, *g_depths, *g_probs, *g_ffd, *theta, *probs, *norm;
    int classes, head, ffd_w;
    const float *P, *act;
    int S, W;
};

__device__ __forceinline__ float dh_g(const DhG& s, int row, int k)
{
    if (s.kind == DH_G_SLABS) {
        const size_t at = (size_t)row * s.W + k, step = (size_t)s.n * s.W;
        float sum = s.P[at];
        for (int i = 1; i < s.S; i++) sum += s.P[at + i * step];
        return s.act[at] > 0.0f ? sum : 0.0f;
    }
    if (k < 2) {
        if (!s.g_theta) return 0.0f;
        const float d0 = s.theta[row * 2], d1 = s.theta[row * 2 + 1], g0 = s.g_theta[row * 2], g1 = s.g_theta[row * 2 + 1];
        const float dot = fmaf(d1, g1, d0 * g0);
        return fmaf(-(k ? d1 : d0), dot, k ? g1 : g0) / s.norm[row];
    }
    if (k < 4) return s.g_trans ? s.g_trans[row * 2 + k - 2] : 0.0f;
    if (k < 7) return s.g_scales ? s.g_scales[row * 3 + k - 4] : 0.0f;
    if (k < 8) return s.g_depths ? s.g_depths[row] : 0.0f;
    if (k < s.head) {
        if (!s.g_probs) return 0.0f;
        const float* p = s.probs + (size_t)row * s.classes;
        const float* g = s.g_probs + (size_t)row * s.classes;
        float dot = 0.0f;
        for (int c = 0; c < s.classes; c++) dot = fmaf(p[c], g[c], dot);
        return p[k - 8] * (g[k - 8] - dot);
    }
    return s.g_ffd ? s.g_ffd[(size_t)row * s.ffd_w + (k - s.head)] : 0.0f;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
struct DhFwd {
    DhX X;
    int K, J, n, mode, col_tiles;     // W [J, K]
    const float *W, *b;
    float* y;                          // DH_HIDDEN: relu(x W^T + b) [n, J]
    float *centre_out, *extent_out;    // DH_HIDDEN with X.roi: the roi centre and extent [n, 2]
    int classes, head, ffd_w;          // DH_ROW
    float *theta, *trans, *scales, *depths, *probs, *ffd, *row, *norm;
};

__global__ __launch_bounds__(DH_THREADS) void k_dh_fwd(const DhFwd a)
{
    __shared__ __attribute__((aligned(16))) float lds[DH_FWD_LDS];
    float* xs = lds;                              // [DH_ROWS][DH_KC]
    float* part = xs + DH_ROWS * DH_KC;           // [DH_ROWS][DH_COLS][17]
    float* fin = part + DH_ROWS * DH_COLS * 17;   // [DH_ROWS][32]: the head columns of the output row
    const int t = (int)threadIdx.x, sub = t & 15, grp = t >> 4;
    const int ct = (int)blockIdx.x % a.col_tiles, row0 = ((int)blockIdx.x / a.col_tiles) * DH_ROWS;
    int c0, c1;
    if (a.mode == DH_ROW) {
        dh_row_col_range(ct, a.J, a.head, &c0, &c1);
    } else {
        c0 = ct * DH_COLS;
        c1 = c0 + DH_COLS < a.J ? c0 + DH_COLS : a.J;
    }
    const bool write_roi = a.centre_out && ct == 0;
    for (int p0 = c0; p0 < c1; p0 += DH_COLS) {
        const int col = p0 + grp;
        float acc[DH_ROWS];
#pragma unroll
        for (int r = 0; r < DH_ROWS; r++) acc[r] = 0.0f;
        for (int kc = 0; kc < a.K; kc += DH_KC) {
            __syncthreads();   // the previous chunk's readers are done
            for (int i = t; i < DH_ROWS * DH_KC; i += DH_THREADS) {
                const int row = row0 + i / DH_KC, k = kc + i % DH_KC;
                float v = 0.0f;
                if (row < a.n && k < a.K) {
                    v = dh_x(a.X, row, k);
                    if (write_roi && k >= a.X.K0) {
                        const int c = k - a.X.K0;
                        (c < 2 ? a.centre_out : a.extent_out)[row * 2 + (c & 1)] = v;
                    }
                }
                xs[i] = v;
            }
            __syncthreads();
            if (col < c1) {
                const float* w = a.W + (size_t)col * a.K + kc;
                for (int kq = sub * 4; kq < DH_KC && kc + kq < a.K; kq += 64) {
                    const float4 wv = *reinterpret_cast<const float4*>(w + kq);
#pragma unroll
                    for (int r = 0; r < DH_ROWS; r++) {
                        const float4 xv = *reinterpret_cast<const float4*>(xs + r * DH_KC + kq);
                        acc[r] = fmaf(wv.x, xv.x, acc[r]);
                        acc[r] = fmaf(wv.y, xv.y, acc[r]);
                        acc[r] = fmaf(wv.z, xv.z, acc[r]);
                        acc[r] = fmaf(wv.w, xv.w, acc[r]);
                    }
                }
            }
        }
        if (col < c1) {
#pragma unroll
            for (int r = 0; r < DH_ROWS; r++) part[(r * DH_COLS + grp) * 17 + sub] = acc[r];
        }
        __syncthreads();
        {   // thread (r, c): the 16 partial sums in order, the bias, and the value's place
            const int r = t >> 4, c = t & 15, row = row0 + r, j = p0 + c;
            if (j < c1) {
                const float* pp = part + (r * DH_COLS + c) * 17;
                float s = pp[0];
#pragma unroll
                for (int i = 1; i < 16; i++) s += pp[i];
                s += a.b[j];
                if (a.mode == DH_HIDDEN) {
                    if (row < a.n) a.y[(size_t)row * a.J + j] = s < 0.0f ? 0.0f : s;
                } else {
                    if (row < a.n && a.row) a.row[(size_t)row * a.J + j] = s;
                    if (ct == 0)
                        fin[r * 32 + j] = s;
                    else if (row < a.n)
                        a.ffd[(size_t)row * a.ffd_w + (j - a.head)] = s;
                }
            }
        }
    }
    if (a.mode != DH_ROW || ct != 0) return;
    __syncthreads();
    const int r = t >> 4, c = t & 15, row = row0 + r;
    float* f = fin + r * 32;
    if (row < a.n && c < DH_FIXED) {
        const float v = f[c];
        if (c < 2) {
            const float norm = sqrtf(fmaf(f[1], f[1], f[0] * f[0]));
            a.theta[row * 2 + c] = v / norm;
            if (c == 0) a.norm[row] = norm;
        } else if (c < 4) {
            a.trans[row * 2 + c - 2] = v;
        } else if (c < 7) {
            a.scales[row * 3 + c - 4] = v;
        } else {
            a.depths[row] = v;
        }
    }
    float e = 0.0f;
    if (c < a.classes) {
        float m = f[DH_FIXED];
        for (int i = 1; i < a.classes; i++) {
            const float x = f[DH_FIXED + i];
            m = x > m ? x : m;   // a NaN reaches a difference either way
        }
        e = expf(f[DH_FIXED + c] - m);
    }
    __syncthreads();
    if (c < a.classes) f[DH_FIXED + c] = e;
    __syncthreads();
    if (c < a.classes && row < a.n) {
        float sum = f[DH_FIXED];
        for (int i = 1; i < a.classes; i++) sum += f[DH_FIXED + i];
        a.probs[(size_t)row * a.classes + c] = e / sum;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// P[s][row][j] = sum over the slab's k of G[row][k] W[k * ldw + j]   (W is nn.Linear's [out = k, in = j])
struct DhDgrad {
    DhG G;
    int K, J, ldw, slab, S, n, col_tiles;
    const float* W;
    float* P;
};

__device__ __forceinline__ void dh_dgrad(const DhDgrad& a, int b, float* lds)
{
    float* xs = lds;                      // [DH_ROWS][DH_KC]
    float* red = xs + DH_ROWS * DH_KC;    // [4][DH_ROWS][DH_DCOLS]
    const int t = (int)threadIdx.x, jl = t & 63, w = t >> 6;
    const int ct = b % a.col_tiles, s = (b / a.col_tiles) % a.S, row0 = (b / (a.col_tiles * a.S)) * DH_ROWS;
    const int j = ct * DH_DCOLS + jl;
    const int k0 = s * a.slab, k1 = k0 + a.slab < a.K ? k0 + a.slab : a.K;
    float acc[DH_ROWS];
#pragma unroll
    for (int r = 0; r < DH_ROWS; r++) acc[r] = 0.0f;
    for (int kc = k0; kc < k1; kc += DH_KC) {
        const int len = k1 - kc < DH_KC ? k1 - kc : DH_KC;
        __syncthreads();
        for (int i = t; i < DH_ROWS * DH_KC; i += DH_THREADS) {
            const int row = row0 + i / DH_KC, kk = i % DH_KC;
            xs[i] = row < a.n && kk < len ? dh_g(a.G, row, kc + kk) : 0.0f;
        }
        __syncthreads();
        if (j < a.J) {
            for (int kk = w * 64; kk < w * 64 + 64 && kk < len; kk += 4) {
                float wv[4];
#pragma unroll
                for (int i = 0; i < 4; i++) wv[i] = kk + i < len ? a.W[(size_t)(kc + kk + i) * a.ldw + j] : 0.0f;
#pragma unroll
                for (int r = 0; r < DH_ROWS; r++) {
                    const float4 xv = *reinterpret_cast<const float4*>(xs + r * DH_KC + kk);
                    acc[r] = fmaf(xv.x, wv[0], acc[r]);
                    acc[r] = fmaf(xv.y, wv[1], acc[r]);
                    acc[r] = fmaf(xv.z, wv[2], acc[r]);
                    acc[r] = fmaf(xv.w, wv[3], acc[r]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < DH_ROWS; r++) red[(w * DH_ROWS + r) * DH_DCOLS + jl] = acc[r];
    __syncthreads();
    for (int i = t; i < DH_ROWS * DH_DCOLS; i += DH_THREADS) {
        const int r = i / DH_DCOLS, jj = i % DH_DCOLS, row = row0 + r, col = ct * DH_DCOLS + jj;
        float sum = red[r * DH_DCOLS + jj];
        for (int v = 1; v < 4; v++) sum += red[(v * DH_ROWS + r) * DH_DCOLS + jj];
        if (row < a.n && col < a.J) a.P[((size_t)s * a.n + row) * a.J + col] = sum;
    }
}

// gW[j][k] = sum over the objects r = 0 .. n - 1, in that order, of G[r][j] X[r][k]; gb[j] = sum of G[r][j].  Either may be NULL.
struct DhWgrad {
    DhG G;
    DhX X;
    int J, K, n, j_groups;
    float *gW, *gb;
};

__device__ __forceinline__ void dh_wgrad(const DhWgrad& a, int b, float* lds)
{
    float* gs = lds;   // [DH_WROWS][DH_WJ]
    const int t = (int)threadIdx.x;
    const int j0 = (b % a.j_groups) * DH_WJ, kt = b / a.j_groups, k = kt * DH_THREADS + t;
    const bool bias = kt == 0 && t < DH_WJ && a.gb && j0 + t < a.J, weight = a.gW && k < a.K;
    float acc[DH_WJ], bacc = 0.0f;
#pragma unroll
    for (int i = 0; i < DH_WJ; i++) acc[i] = 0.0f;
    for (int r0 = 0; r0 < a.n; r0 += DH_WROWS) {
        const int rows = a.n - r0 < DH_WROWS ? a.n - r0 : DH_WROWS;
        __syncthreads();
        for (int i = t; i < DH_WROWS * DH_WJ; i += DH_THREADS) {
            const int rr = i / DH_WJ, jj = i % DH_WJ;
            gs[i] = rr < rows && j0 + jj < a.J ? dh_g(a.G, r0 + rr, j0 + jj) : 0.0f;
        }
        __syncthreads();
        if (weight) {
            for (int rr = 0; rr < rows; rr++) {
                const float x = dh_x(a.X, r0 + rr, k);
                const float4 lo = *reinterpret_cast<const float4*>(gs + rr * DH_WJ), hi = *reinterpret_cast<const float4*>(gs + rr * DH_WJ + 4);
                acc[0] = fmaf(lo.x, x, acc[0]);
                acc[1] = fmaf(lo.y, x, acc[1]);
                acc[2] = fmaf(lo.z, x, acc[2]);
                acc[3] = fmaf(lo.w, x, acc[3]);
                acc[4] = fmaf(hi.x, x, acc[4]);
                acc[5] = fmaf(hi.y, x, acc[5]);
                acc[6] = fmaf(hi.z, x, acc[6]);
                acc[7] = fmaf(hi.w, x, acc[7]);
            }
        }
        if (bias)
            for (int rr = 0; rr < rows; rr++) bacc += gs[rr * DH_WJ + t];
    }
    if (weight) {
#pragma unroll
        for (int i = 0; i < DH_WJ; i++)
            if (j0 + i < a.J) a.gW[(size_t)(j0 + i) * a.K + k] = acc[i];
    }
    if (bias) a.gb[j0 + t] = bacc;
}

// one launch of the backward: `nd` input-gradient workgroups, then the workgroups of up to two weight gradients
struct DhBwd {
    DhDgrad d;
    DhWgrad w0, w1;
    int nd, nw0, nw1;
};

__global__ __launch_bounds__(DH_THREADS) void k_dh_bwd(const DhBwd a)
{
    __shared__ __attribute__((aligned(16))) float lds[DH_BWD_LDS];
    int b = (int)blockIdx.x;
    if (b < a.nd) {
        dh_dgrad(a.d, b, lds);
        return;
    }
    b -= a.nd;
    if (b < a.nw0)
        dh_wgrad(a.w0, b, lds);
    else
        dh_wgrad(a.w1, b - a.nw0, lds);
}

static int dh_launch_fwd(const DhFwd& a, hipStream_t st, const char* what)
{
    hipLaunchKernelGGL(k_dh_fwd, dim3((unsigned)(a.col_tiles * dh_row_tiles(a.n))), dim3(DH_THREADS), 0, st, a);
    return check_launch(what);
}

static int dh_launch_bwd(const DhBwd& a, hipStream_t st, const char* what)
{
    const long long blocks = (long long)a.nd + a.nw0 + a.nw1;
    if (blocks == 0) return SDN_OK;   // nothing of this stage is asked for
    if (blocks >= DH_LIMIT) return fail(SDN_EINVAL, "%s: %lld workgroups in one launch", what, blocks);
    hipLaunchKernelGGL(k_dh_bwd, dim3((unsigned)blocks), dim3(DH_THREADS), 0, st, a);
    return check_launch(what);
}

static DhX dh_input(const float* x, int K0, const float* roi = nullptr, const float* centre = nullptr, const float* extent = nullptr)
{
    DhX X;
    X.x = x;
    X.ldx = X.K0 = K0;
    X.roi = roi;
    X.centre = centre;
    X.extent = extent;
    return X;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_derender_heads_workspace_bytes(int n, int F, int Hd, int classes, int coeffs, size_t* bytes)
{
    char why[256];
    DhLayout L;
    if (!bytes) return fail(SDN_EINVAL, "sdn_derender_heads_workspace_bytes: bytes is NULL");
    if (dh_layout(n, F, Hd, classes, coeffs, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_derender_heads_workspace_bytes: %s", why);
    *bytes = dh_workspace_bytes(L);
    return SDN_OK;
}

SDN_API int sdn_derender_heads_fwd(const float* pooled, const float* roi_norms, const float* centre, const float* extent, const float* w0,
                                   const float* b0, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                   const float* b3, int n, int F, int Hd, int classes, int coeffs, float* out, float* centre_out,
                                   float* extent_out, float* row, float* saved, sdnStream stream)
{
    static const char* const what = "sdn_derender_heads_fwd";
    char why[256];
    DhLayout L;
    const void* const w[4] = {w0, w1, w2, w3};
    const void* const b[4] = {b0, b1, b2, b3};
    if (dh_validate_fwd(pooled, roi_norms, centre, extent, w, b, n, F, Hd, classes, coeffs, out, centre_out, extent_out, row, saved, &L, why,
                        sizeof(why)))
        return fail(SDN_EINVAL, "%s: %s", what, why);
    hipStream_t st = (hipStream_t)stream;
    float *h0 = saved + L.h0, *h1 = saved + L.h1, *h2 = saved + L.h2;
    DhFwd a = {};
    a.n = n;
    a.mode = DH_HIDDEN;
    a.J = Hd;
    a.col_tiles = (Hd + DH_COLS - 1) / DH_COLS;
    // net.fc and the ReLU (derenderer.py:27, :34)
    a.X = dh_input(pooled, F);
    a.K = F;
    a.W = w0;
    a.b = b0;
    a.y = h0;
    if (int rc = dh_launch_fwd(a, st, what)) return rc;
    // the cat with the roi centre and extent (models/__init__.py:103-104), fc1, ReLU (derenderer.py:34-35)
    a.X = dh_input(h0, Hd, roi_norms, centre, extent);
    a.K = L.K1;
    a.W = w1;
    a.b = b1;
    a.y = h1;
    a.centre_out = centre_out;
    a.extent_out = extent_out;
    if (int rc = dh_launch_fwd(a, st, what)) return rc;
    // fc2, ReLU (:36)
    a.X = dh_input(h1, Hd);
    a.K = Hd;
    a.W = w2;
    a.b = b2;
    a.y = h2;
    a.centre_out = a.extent_out = nullptr;
    if (int rc = dh_launch_fwd(a, st, what)) return rc;
    // _fc3, the slices, the unit pose pair, the softmax (:37-63)
    a.X = dh_input(h2, Hd);
    a.mode = DH_ROW;
    a.J = L.O;
    a.col_tiles = dh_row_col_tiles(L.O, L.head);
    a.W = w3;
    a.b = b3;
    a.y = nullptr;
    a.classes = classes;
    a.head = L.head;
    a.ffd_w = L.ffd_w;
    a.theta = out + L.theta;
    a.trans = out + L.trans;
    a.scales = out + L.scales;
    a.depths = out + L.depths;
    a.probs = out + L.probs;
    a.ffd = out + L.ffd;
    a.row = row;
    a.norm = saved + L.norm;
    return dh_launch_fwd(a, st, what);
}

SDN_API int sdn_derender_heads_bwd(const float* g_theta, const float* g_trans, const float* g_scales, const float* g_depths,
                                   const float* g_probs, const float* g_ffd, const float* pooled, const float* centre, const float* extent,
                                   const float* w0, const float* w1, const float* w2, const float* w3, const float* out, const float* saved,
                                   int n, int F, int Hd, int classes, int coeffs, float* g_pooled, float* g_w0, float* g_b0, float* g_w1,
                                   float* g_b1, float* g_w2, float* g_b2, float* g_w3, float* g_b3, void* workspace, size_t workspace_bytes,
                                   sdnStream stream)
{
    static const char* const what = "sdn_derender_heads_bwd";
    char why[256];
    DhLayout L;
    const void* const g[6] = {g_theta, g_trans, g_scales, g_depths, g_probs, g_ffd};
    const void* const w[4] = {w0, w1, w2, w3};
    const void* const wanted[9] = {g_pooled, g_w0, g_b0, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
    if (dh_validate_bwd(g, pooled, centre, extent, w, out, saved, n, F, Hd, classes, coeffs, wanted, workspace, workspace_bytes, &L, why,
                        sizeof(why)))
        return fail(SDN_EINVAL, "%s: %s", what, why);
    hipStream_t st = (hipStream_t)stream;
    const float *h0 = saved + L.h0, *h1 = saved + L.h1, *h2 = saved + L.h2;
    float* ws = static_cast<float*>(workspace);
    float *P2 = ws + L.p2, *P1 = ws + L.p1, *P0 = ws + L.p0;
    // which hidden gradients anybody needs: a frozen layer or a detached backbone costs nothing
    const bool need0 = g_pooled || g_w0 || g_b0, need1 = need0 || g_w1 || g_b1, need2 = need1 || g_w2 || g_b2;
    const int tiles = dh_row_tiles(n);

    DhG g_row = {};
    g_row.kind = DH_G_ROW;
    g_row.n = n;
    g_row.g_theta = g_theta;
    g_row.g_trans = g_trans;
    g_row.g_scales = g_scales;
    g_row.g_depths = g_depths;
    g_row.g_probs = g_probs;
    g_row.g_ffd = g_ffd;
    g_row.theta = out + L.theta;
    g_row.probs = out + L.probs;
    g_row.norm = saved + L.norm;
    g_row.classes = classes;
    g_row.head = L.head;
    g_row.ffd_w = L.ffd_w;
    auto slabs = [&](const float* P, int S, const float* act) {
        DhG s = {};
        s.kind = DH_G_SLABS;
        s.n = n;
        s.P = P;
        s.S = S;
        s.W = Hd;
        s.act = act;
        return s;
    };
    auto dgrad = [&](DhBwd* a, const DhG& G, int K, const float* W, int ldw, int J, int slab, float* P) {
        a->d.G = G;
        a->d.K = K;
        a->d.J = J;
        a->d.ldw = ldw;
        a->d.slab = slab;
        a->d.S = (K + slab - 1) / slab;
        a->d.n = n;
        a->d.col_tiles = (J + DH_DCOLS - 1) / DH_DCOLS;
        a->d.W = W;
        a->d.P = P;
        a->nd = a->d.col_tiles * a->d.S * tiles;
    };
    auto wgrad = [&](DhWgrad* v, int* count, const DhG& G, const DhX& X, int J, int K, float* gW, float* gb) {
        if (!gW && !gb) return;
        v->G = G;
        v->X = X;
        v->J = J;
        v->K = K;
        v->n = n;
        v->j_groups = (J + DH_WJ - 1) / DH_WJ;
        v->gW = gW;
        v->gb = gb;
        *count = v->j_groups * (gW ? (K + DH_THREADS - 1) / DH_THREADS : 1);
    };
    const DhG g_h2 = slabs(P2, L.S3, h2), g_h1 = slabs(P1, L.SH, h1), g_h0 = slabs(P0, L.SH, h0);

    DhBwd a = {};   // 1: the slabs of fc2's output gradient, from the output row's
    if (need2) dgrad(&a, g_row, L.O, w3, Hd, Hd, DH_SLAB, P2);
    if (int rc = dh_launch_bwd(a, st, what)) return rc;
    a = DhBwd{};    // 2: _fc3's weights; the slabs of fc1's output gradient
    if (need1) dgrad(&a, g_h2, Hd, w2, Hd, Hd, DH_SLAB, P1);
    wgrad(&a.w0, &a.nw0, g_row, dh_input(h2, Hd), L.O, Hd, g_w3, g_b3);
    if (int rc = dh_launch_bwd(a, st, what)) return rc;
    a = DhBwd{};    // 3: fc2's weights; the slabs of net.fc's output gradient (fc1's first Hd input columns)
    if (need0) dgrad(&a, g_h1, Hd, w1, L.K1, Hd, DH_SLAB, P0);
    wgrad(&a.w0, &a.nw0, g_h2, dh_input(h1, Hd), Hd, Hd, g_w2, g_b2);
    if (int rc = dh_launch_bwd(a, st, what)) return rc;
    a = DhBwd{};    // 4: fc1's and net.fc's weights; the pooled features' gradient, one slab, written in place
    if (g_pooled) dgrad(&a, g_h0, Hd, w0, F, F, Hd, g_pooled);
    wgrad(&a.w0, &a.nw0, g_h1, dh_input(h0, Hd, nullptr, centre, extent), Hd, L.K1, g_w1, g_b1);
    wgrad(&a.w1, &a.nw1, g_h0, dh_input(pooled, F), Hd, F, g_w0, g_b0);
    return dh_launch_bwd(a, st, what);
}
