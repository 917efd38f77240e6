// The tail of the semantic branch: from the decoder's class scores to the label map the textural branch starts from, and to
// the integers of the evaluation (semantic/vkitti_test.py:56-73, vkitti_eval.py:64-107, models.py:401-402, utils.py:101-129,
// vkitti_dataset.py:206-209, 238).
//
// The reference upsamples the scores of each of its five test scales to the full frame (bilinear), takes a softmax there, averages
// the five [1, 14, 375, 1242] tensors, copies the 26 MB sum to the host and takes torch.max on the CPU; evaluation then runs numpy
// histograms per frame over a ground-truth map made by a Python call per pixel.  Here:
//   k_segm_fuse       one launch for all scales and frames.  A workgroup owns an 8 x 32 tile of the label map, a thread one pixel.
//                     Per scale the tile's source footprint is staged into LDS, every thread interpolates its four taps for all
//                     classes, takes the softmax (maximum subtracted, expf) and adds p / S to its running sums in registers;
//                     after the last scale it writes the arg-max (lowest class on an exact tie; a NaN makes every sum of the
//                     pixel NaN, no comparison holds and the label is 0) and, when asked, the sums.  No full-resolution
//                     intermediate exists and nothing is accumulated across threads: the output is identical from run to run.
//   k_segm_colors     the ground-truth label of every pixel by a binary search of its 24-bit colour code in a sorted table in
//                     LDS; four pixels (three dwords in, one 8-byte store out) per thread.
//   k_segm_confusion  area_intersection, area_pred, area_lab, acc_sum, valid_sum and the unknown-colour count of each frame:
//                     per-wave private counters in LDS, one 64-bit integer atomic per non-zero column and workgroup.
// Compiled without FMA contraction: the interpolation is the reference's expression, operation by operation.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "device_common.h"
#include "sdn_common.h"
#include "segm_tail_check.h"

namespace sdn {

constexpr int SEG_THREADS = SEG_TILE_H * SEG_TILE_W;
static_assert(SEG_THREADS == 256 && SEG_TILE_W == 32, "a thread's pixel is (tid >> 5, tid & 31)");
static_assert(SEG_LDS_FLOATS * sizeof(float) <= 40 * 1024, "four workgroups per CU");

struct FuseParams {
    SegScale sc[SEG_MAX_SCALES];
    int S, C, H, W;
    uint8_t* labels;   // [B, 1, H, W]
    float* pred;       // [B, C, H, W] or null
};

// CP: the class count rounded up to 8, 16 or 32 -- the running sums and the scores of a pixel are register arrays
template <int CP>
__global__ __launch_bounds__(SEG_THREADS) void k_segm_fuse(const FuseParams A)
{
    __shared__ float s_foot[SEG_LDS_FLOATS];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * SEG_TILE_W, Y0 = blockIdx.y * SEG_TILE_H, b = blockIdx.z;
    const int C = A.C, H = A.H, W = A.W;
    const int px = X0 + (tid & 31), py = Y0 + (tid >> 5);
    // a thread beyond the frame's edge repeats the edge pixel (it takes part in the staging) and stores nothing
    const int x = min(px, W - 1), y = min(py, H - 1);
    const int xl = min(X0 + SEG_TILE_W - 1, W - 1), yl = min(Y0 + SEG_TILE_H - 1, H - 1);
    const float fS = (float)A.S;
    float acc[CP], v[CP];
#pragma unroll
    for (int c = 0; c < CP; c++) acc[c] = 0.f;

    for (int s = 0; s < A.S; s++) {
        const int h = A.sc[s].h, w = A.sc[s].w;
        const float* src = reinterpret_cast<const float*>(A.sc[s].scores) + (size_t)b * C * h * w;
        const float sh = seg_scale(h, H), sw = seg_scale(w, W);
        int fy, ny, fx, nx;   // the footprint: rows fy .. fy + ny - 1, columns fx .. fx + nx - 1, all inside the map
        seg_footprint(sh, Y0, yl, h, SEG_FOOT_ROWS, &fy, &ny);
        seg_footprint(sw, X0, xl, w, SEG_FOOT_COLS, &fx, &nx);
        const int npos = ny * nx;                       // <= SEG_FOOT_MAX
        const int cc = min(C, SEG_LDS_FLOATS / npos);   // classes per chunk, >= SEG_CHUNK_MIN or C
        int y0, y1, x0, x1;
        float ly, lx;
        seg_taps(sh, y, h, &y0, &y1, &ly);
        seg_taps(sw, x, w, &x0, &x1, &lx);
        const float ly0 = 1.f - ly, lx0 = 1.f - lx;
        // the taps relative to the footprint; the clamps hold every LDS index inside the staged rows whatever the sizes are
        const int ry0 = min(max(y0 - fy, 0), ny - 1), ry1 = min(max(y1 - fy, 0), ny - 1);
        const int rx0 = min(max(x0 - fx, 0), nx - 1), rx1 = min(max(x1 - fx, 0), nx - 1);
        const int o00 = ry0 * nx + rx0, o01 = ry0 * nx + rx1, o10 = ry1 * nx + rx0, o11 = ry1 * nx + rx1;
        for (int c0 = 0; c0 < C; c0 += cc) {   // uniform over the workgroup
            const int n = min(cc, C - c0);
            __syncthreads();   // the previous chunk has been read
            for (int i = tid; i < n * npos; i += SEG_THREADS) {
                const int c = i / npos, p = i - c * npos;
                const int r = p / nx, q = p - r * nx;
                s_foot[i] = src[((size_t)(c0 + c) * h + fy + r) * w + fx + q];
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CP; c++) {
                const int k = c - c0;
                if (k >= 0 && k < n) {
                    const float* f = s_foot + k * npos;
                    v[c] = ly0 * (lx0 * f[o00] + lx * f[o01]) + ly * (lx0 * f[o10] + lx * f[o11]);
                }
            }
        }
        // softmax over the classes (models.py:402), then pred + pred_tmp / len(imgSize) (vkitti_test.py:70)
        float m = v[0];
#pragma unroll
        for (int c = 1; c < CP; c++)
            if (c < C) m = fmaxf(m, v[c]);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CP; c++)
            if (c < C) {
                v[c] = expf(v[c] - m);
                sum += v[c];
            }
#pragma unroll
        for (int c = 0; c < CP; c++)
            if (c < C) acc[c] += (v[c] / sum) / fS;
    }

    if (px >= W || py >= H) return;
    int best = 0;
    float top = acc[0];
#pragma unroll
    for (int c = 1; c < CP; c++)
        if (c < C && acc[c] > top) {   // strictly greater: the lowest class wins a tie, NaN never wins
            top = acc[c];
            best = c;
        }
    const size_t HW = (size_t)H * W, at = (size_t)py * W + px;
    A.labels[(size_t)b * HW + at] = (uint8_t)best;
    if (A.pred) {
        float* out = A.pred + (size_t)b * C * HW + at;
#pragma unroll
        for (int c = 0; c < CP; c++)
            if (c < C) out[(size_t)c * HW] = acc[c];
    }
}

// ---- ground-truth labels from colours ----------------------------------------------------------------------------------------
constexpr int SEGC_THREADS = 256;

__device__ __forceinline__ int seg_label_of(const int32_t* codes, const int32_t* labels, int K, int code)
{
    const int k = seg_find(codes, K, code);
    return k < 0 ? SEG_UNKNOWN : labels[k] - 1;   // vkitti_dataset.py:238: unlabelled is -1
}

// Thread q of the grid owns the pixels 4 q .. 4 q + 3 of the flat [B H W] map: bytes 12 q .. 12 q + 11 of the scene, three
// aligned dwords; the last quad may be short.  Every wave runs every round of the loop (a lane without a quad idles), so the
// counts of unknown colours can be reduced over the wave.
__global__ __launch_bounds__(SEGC_THREADS) void k_segm_colors(const uint8_t* __restrict__ scene, const int32_t* __restrict__ table, int K,
                                                              long N, long HW, int16_t* __restrict__ out, int32_t* unknown)
{
    __shared__ int32_t s_codes[SEG_MAX_COLORS], s_labels[SEG_MAX_COLORS];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < K; i += SEGC_THREADS) {
        s_codes[i] = table[i];
        s_labels[i] = table[K + i];
    }
    __syncthreads();
    const long nq = (N + 3) >> 2;
    for (long base = (long)blockIdx.x * SEGC_THREADS; base < nq; base += (long)gridDim.x * SEGC_THREADS) {   // uniform
        const long q = base + tid, p0 = 4 * q;
        int code[4] = {0, 0, 0, 0};
        const int have = q < nq ? (int)min(4L, N - p0) : 0;
        if (have == 4) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(scene) + 3 * q;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            code[0] = (int)(w0 & 0xffffffu);
            code[1] = (int)((w0 >> 24) | ((w1 & 0xffffu) << 8));
            code[2] = (int)((w1 >> 16) | ((w2 & 0xffu) << 16));
            code[3] = (int)(w2 >> 8);
        } else {
            for (int j = 0; j < have; j++) code[j] = code24(scene + 3 * (p0 + j));
        }
        int lab[4] = {0, 0, 0, 0}, miss = 0;
        for (int j = 0; j < 4; j++) {
            if (j >= have) break;
            // neighbours mostly share their colour
            lab[j] = (j && code[j] == code[j - 1]) ? lab[j - 1] : seg_label_of(s_codes, s_labels, K, code[j]);
            miss += lab[j] == SEG_UNKNOWN ? 1 : 0;
        }
        if (have == 4) {
            uint2 o;
            o.x = ((uint32_t)lab[0] & 0xffffu) | ((uint32_t)lab[1] << 16);
            o.y = ((uint32_t)lab[2] & 0xffffu) | ((uint32_t)lab[3] << 16);
            *reinterpret_cast<uint2*>(out + p0) = o;
        } else {
            for (int j = 0; j < have; j++) out[p0 + j] = (int16_t)lab[j];
        }
        // the wave's pixels 4 (q - lane) .. : nearly always of one frame
        const long wp0 = 4 * (q - lane);
        if (wp0 >= N) continue;   // uniform over the wave
        const long wp1 = min(wp0 + 4 * 64, N) - 1;
        const long f0 = wp0 / HW;
        if (f0 == wp1 / HW) {
            const int t = wave_sum(miss);
            if (t && lane == 0) atomicAdd(unknown + f0, t);
        } else {
            for (int j = 0; j < have; j++)
                if (lab[j] == SEG_UNKNOWN) atomicAdd(unknown + (p0 + j) / HW, 1);
        }
    }
}

// ---- the integers of accuracy() and intersectionAndUnion() ----------------------------------------------------------------
constexpr int SEGF_THREADS = 256;
constexpr int SEGF_WAVES = SEGF_THREADS / 64;
constexpr int SEGF_COLS_MAX = 3 * SEG_MAX_CONF_CLASSES + 3;
constexpr int SEGF_PIXELS = SEGF_THREADS * 8;   // pixels of a workgroup when the grid is not capped

// row[key] += the number of lanes with `on` and this key, one round per distinct key among the wave's 64 pixels; `row` is the
// wave's own
__device__ __forceinline__ void seg_wave_hist(int* row, int key, bool on, int lane)
{
    unsigned long long left = __ballot(on);
    while (left) {
        const int src = __ffsll((long long)left) - 1;
        const int k0 = __shfl(key, src, 64);
        const unsigned long long same = __ballot(on && key == k0);
        left &= ~same;
        if (lane == src) atomicAdd(&row[k0], __popcll(same));
    }
}

// utils.py:101-129 on one frame: valid = gt >= 0; the prediction counts only there (imPred * (imLab > 0)); np.histogram(.,
// bins=C, range=(1, C)) of the labels + 1 drops 0 and everything above C and puts label + 1 = v into bin v - 1.
__global__ __launch_bounds__(SEGF_THREADS) void k_segm_confusion(const uint8_t* __restrict__ labels, const int16_t* __restrict__ gt, int C,
                                                                 long HW, unsigned long long* counts)
{
    __shared__ int s_cnt[SEGF_WAVES][SEGF_COLS_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int cols = 3 * C + 3;
    for (int i = tid; i < SEGF_WAVES * SEGF_COLS_MAX; i += SEGF_THREADS) (&s_cnt[0][0])[i] = 0;
    __syncthreads();
    const uint8_t* lab = labels + (size_t)b * HW;
    const int16_t* g = gt + (size_t)b * HW;
    int* row = s_cnt[wave];
    int valid = 0, hit = 0, unk = 0;
    for (long base = (long)blockIdx.x * SEGF_THREADS; base < HW; base += (long)gridDim.x * SEGF_THREADS) {   // uniform
        const long p = base + tid;
        const bool in = p < HW;
        const int gv = in ? (int)g[p] : -1, pv = in ? (int)lab[p] : 0;
        const bool ok = gv >= 0;
        valid += ok ? 1 : 0;
        hit += (ok && pv == gv) ? 1 : 0;
        unk += (in && gv == SEG_UNKNOWN) ? 1 : 0;
        seg_wave_hist(row, pv, ok && pv == gv && pv < C, lane);
        seg_wave_hist(row + C, pv, ok && pv < C, lane);
        seg_wave_hist(row + 2 * C, gv, ok && gv < C, lane);
    }
    valid = wave_sum(valid);
    hit = wave_sum(hit);
    unk = wave_sum(unk);
    if (lane == 0) {
        row[3 * C] = hit;
        row[3 * C + 1] = valid;
        row[3 * C + 2] = unk;
    }
    __syncthreads();
    for (int t = tid; t < cols; t += SEGF_THREADS) {   // never beyond the frame's row of 3 C + 3 columns
        int total = 0;   // a workgroup holds fewer than 2^31 pixels: the int sums cannot overflow
        for (int k = 0; k < SEGF_WAVES; k++) total += s_cnt[k][t];
        if (total) atomicAdd(counts + (size_t)b * cols + t, (unsigned long long)total);
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_segm_fuse(const int32_t* table_host, int S, int B, int C, int H, int W, uint8_t* labels, float* pred, sdnStream stream)
{
    if (!table_host || !labels) return fail(SDN_EINVAL, "sdn_segm_fuse: null pointer");
    if (pred && (reinterpret_cast<uintptr_t>(pred) & 3)) return fail(SDN_EINVAL, "sdn_segm_fuse: pred is not aligned to 4 bytes");
    char why[256];
    if (seg_validate_fuse(table_host, S, B, C, H, W, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_segm_fuse: %s", why);
    FuseParams A;
    for (int s = 0; s < SEG_MAX_SCALES; s++) memcpy(&A.sc[s], table_host + 4 * (size_t)(s < S ? s : 0), sizeof(SegScale));
    A.S = S; A.C = C; A.H = H; A.W = W; A.labels = labels; A.pred = pred;
    // the table travels as the kernel's argument: uploaded once, with the launch
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(W, SEG_TILE_W), cdiv(H, SEG_TILE_H), (unsigned)B);
    if (C <= 8) hipLaunchKernelGGL(k_segm_fuse<8>, grid, dim3(SEG_THREADS), 0, st, A);
    else if (C <= 16) hipLaunchKernelGGL(k_segm_fuse<16>, grid, dim3(SEG_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_segm_fuse<32>, grid, dim3(SEG_THREADS), 0, st, A);
    return check_launch("k_segm_fuse");
}

SDN_API int sdn_segm_labels_from_colors(const uint8_t* scene, int B, int H, int W, const int32_t* table_host, const int32_t* table, int K,
                                        int16_t* labels_gt, int32_t* unknown, sdnStream stream)
{
    if (!scene || !table_host || !table || !labels_gt || !unknown) return fail(SDN_EINVAL, "sdn_segm_labels_from_colors: null pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > INT_MAX || (long)B * H * W > (long)INT_MAX * 16)
        return fail(SDN_EINVAL, "sdn_segm_labels_from_colors: bad sizes");
    if ((reinterpret_cast<uintptr_t>(scene) & 3) || (reinterpret_cast<uintptr_t>(labels_gt) & 7) || (reinterpret_cast<uintptr_t>(table) & 3) ||
        (reinterpret_cast<uintptr_t>(unknown) & 3))
        return fail(SDN_EINVAL, "sdn_segm_labels_from_colors: the scene, the table and the counts must be aligned to 4 bytes, the labels to 8");
    char why[256];
    if (seg_validate_colors(table_host, K, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_segm_labels_from_colors: %s", why);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(unknown, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess)
        return fail(SDN_ELAUNCH, "sdn_segm_labels_from_colors: clearing the counts failed");
    const long N = (long)B * H * W, nq = (N + 3) / 4;
    const unsigned blocks = (unsigned)(cdiv(nq, SEGC_THREADS) < 2048u ? cdiv(nq, SEGC_THREADS) : 2048u);
    hipLaunchKernelGGL(k_segm_colors, dim3(blocks), dim3(SEGC_THREADS), 0, st, scene, table, K, N, (long)H * W, labels_gt, unknown);
    return check_launch("k_segm_colors");
}

SDN_API int sdn_segm_confusion(const uint8_t* labels, const int16_t* labels_gt, int B, int H, int W, int C, int64_t* counts,
                               sdnStream stream)
{
    if (!labels || !labels_gt || !counts) return fail(SDN_EINVAL, "sdn_segm_confusion: null pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > INT_MAX) return fail(SDN_EINVAL, "sdn_segm_confusion: bad sizes");
    if (C < 1 || C > SEG_MAX_CONF_CLASSES) return fail(SDN_EINVAL, "sdn_segm_confusion: %d classes; 1 to %d are supported", C, SEG_MAX_CONF_CLASSES);
    if ((reinterpret_cast<uintptr_t>(labels_gt) & 1) || (reinterpret_cast<uintptr_t>(counts) & 7))
        return fail(SDN_EINVAL, "sdn_segm_confusion: labels_gt must be aligned to 2 bytes, counts to 8");
    hipStream_t st = (hipStream_t)stream;
    const size_t cols = 3 * (size_t)C + 3;
    if (hipMemsetAsync(counts, 0, (size_t)B * cols * sizeof(int64_t), st) != hipSuccess)
        return fail(SDN_ELAUNCH, "sdn_segm_confusion: clearing the counts failed");
    const long HW = (long)H * W;
    const unsigned blocks = (unsigned)(cdiv(HW, SEGF_PIXELS) < 256u ? cdiv(HW, SEGF_PIXELS) : 256u);
    hipLaunchKernelGGL(k_segm_confusion, dim3(blocks, (unsigned)B), dim3(SEGF_THREADS), 0, st, labels, labels_gt, C, HW,
                       reinterpret_cast<unsigned long long*>(counts));
    return check_launch("k_segm_confusion");
}
