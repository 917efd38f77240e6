// The training items of the geometric branch, batched over several frames (geometric/derender3d/datasets.py:332-420
// VKitti.__getitem__, :37-46 roi_jitter, :141-172 transform_rgb / _mask / _ignore with Transforms.color_jitter; data_loader.py:17-37).
//
// The reference makes, per object on the host, a full-frame np.all over every object of the frame, three PIL round trips
// (crop_square, bilinear resize, to_tensor) and, when training, four ImageEnhance / HSV passes over the crop.  Here:
//   k_train_rois    the bounding box (mask_to_roi) and pixel count of B (frame, colour code) pairs, integer atomics once per wave.
//   k_train_stats   the one global quantity of the colour jitter: ImageEnhance.Contrast blends with the mean of the crop's
//                   convert('L') as the crop is at that point of the order.  Sums L over the s x s window after the ops that
//                   precede contrast (64-bit integer atomics, once per workgroup).  Launched only when an item has contrast.
//   k_train_crops   one launch for B items x (image, mask, ignore).  A workgroup owns a band of output rows of one (item, kind);
//                   the image kind carries its three channels together.  It stages the source pixels of the rows the band needs
//                   through LDS -- the colour jitter (image), the code test (mask) or the count of nearer codes (ignore) is
//                   applied THERE, once per source pixel and band --, runs Pillow's horizontal pass (ImagingResample, 22-bit
//                   fixed point, rounded to uint8 as Pillow stores it) out of the staged pixels into LDS and the vertical pass
//                   out of LDS, then to_tensor (/ 255) and, for the image, Normalize.
// The window, its padding quirk and the resize are those of scene_crops.hip; with an empty order the outputs are its outputs.
//
// The four ops are Pillow's as torchvision 0.2.1 calls them, restated operation for operation (tests/geo_train_util.py holds
// the same statements in numpy against the installed Pillow):
//   Image.blend (Blend.c)      (float)d + alpha * (float)(v - d) in fp32, truncated for alpha in [0, 1], clipped outside
//   convert('L') (Convert.c)   (19595 R + 38470 G + 7471 B + 32768) >> 16
//   convert('HSV') and back    Convert.c's rgb2hsv_row / hsv2rgb: fp32 quotients, the sums and products that involve a double
//                              literal in double
// Compiled without FMA contraction, so the fp32 / fp64 statements round as the host's do.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "sdn_common.h"
#include "train_items_common.h"

namespace sdn {

struct TrainParams {
    const uint8_t* frames;     // [Fr, 3, H, W]
    const uint8_t* scenes;     // [Fr, H, W, 3]
    const TrainWin* objs;
    const TrainItem* items;
    const int32_t* bounds;
    const int32_t* kk8;
    const uint8_t* nearer;     // [total, 3]
    unsigned long long* lsum;  // [B] sum of L over the window (items with contrast)
    int B, H, W, Si, Sm;
    float mean[3], std[3];
    float *images, *masks, *ignores;
};

// ---- rois ------------------------------------------------------------------------------------------------------------------
__global__ void k_train_rois_init(int32_t* table, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    table[5 * b] = INT_MAX;
    table[5 * b + 1] = INT_MAX;
    table[5 * b + 2] = 0;
    table[5 * b + 3] = 0;
    table[5 * b + 4] = 0;
}

// A workgroup tests 1024 pixels of one item's frame; the matches of a wave are reduced and noted with five atomics.
__global__ __launch_bounds__(TI_THREADS) void k_train_rois(const uint8_t* __restrict__ scenes, const int32_t* __restrict__ items, int Fr,
                                                           int H, int W, int32_t* table)
{
    const int b = blockIdx.y;
    const int frame = items[4 * b];
    if (frame < 0 || frame >= Fr) return;   // uniform over the workgroup; the row stays empty
    const int r = items[4 * b + 1] & 255, g = items[4 * b + 2] & 255, bl = items[4 * b + 3] & 255;
    const int HW = H * W;
    const uint8_t* scene = scenes + (size_t)frame * HW * 3;
    int ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1, cnt = 0;
    for (int j = 0; j < 4; j++) {
        const int p = blockIdx.x * (4 * TI_THREADS) + j * TI_THREADS + threadIdx.x;
        if (p >= HW) continue;
        const uint8_t* s = scene + 3 * (size_t)p;
        if (s[0] != r || s[1] != g || s[2] != bl) continue;
        const int y = p / W, x = p - y * W;
        ymin = min(ymin, y); xmin = min(xmin, x); ymax = max(ymax, y); xmax = max(xmax, x);
        cnt++;
    }
    cnt = wave_sum(cnt);
    if (cnt) {   // uniform over the wave
        ymin = wave_imin(ymin); xmin = wave_imin(xmin); ymax = wave_imax(ymax); xmax = wave_imax(xmax);
        if ((threadIdx.x & 63) == 0) {
            atomicMin(table + 5 * b, ymin);
            atomicMin(table + 5 * b + 1, xmin);
            atomicMax(table + 5 * b + 2, ymax + 1);
            atomicMax(table + 5 * b + 3, xmax + 1);
            atomicAdd(table + 5 * b + 4, cnt);
        }
    }
}

// ---- the kernels: the shared bodies (train_items_common.h) on the call's frames and scenes ------------------------------------------
struct TrainSrc {
    const TrainParams& A;
    const TrainWin& o;
    const TrainItem& it;
    __device__ __forceinline__ void rgb(int wy, int wx, int& r, int& g, int& b) const
    {
        ti_raw_rgb(o, A.frames + (size_t)it.frame * 3 * A.H * A.W, A.H, A.W, wy, wx, r, g, b);
    }
    __device__ __forceinline__ int map_byte(int kind, int wy, int wx) const
    {
        size_t p = 0;
        const int v = ti_map_outside(o, A.H, A.W, kind, wy, wx, &p);
        if (v >= 0) return v;
        return ti_code_byte(A.scenes + (size_t)it.frame * A.H * A.W * 3, p, kind, it.code, A.nearer + 3 * (size_t)it.near_off, it.near_cnt);
    }
    __device__ __forceinline__ float mean(int ch) const { return A.mean[ch]; }
    __device__ __forceinline__ float stdev(int ch) const { return A.std[ch]; }
};

__global__ __launch_bounds__(TI_THREADS) void k_train_stats(const TrainParams A)
{
    __shared__ int s_part[TI_WAVES];
    const int n = blockIdx.y;
    const TrainItem it = A.items[n];
    const TrainWin o = A.objs[n];
    ti_stats_body(TrainSrc{A, o, it}, o, it, A.lsum + n, s_part);
}

__global__ __launch_bounds__(TI_THREADS) void k_train_crops(const TrainParams A)
{
    __shared__ uint8_t s_src[3 * TI_SRC_PIXELS];
    __shared__ uint8_t s_rows[3 * TI_PLANE_BYTES];
    const int n = blockIdx.z, kind = blockIdx.y;   // kind 0: image, 1: mask, 2: ignore
    const int S = kind == 0 ? A.Si : A.Sm;
    const int r0 = blockIdx.x * TI_BAND;
    if (r0 >= S) return;
    const TrainWin o = A.objs[n];
    const TrainItem it = A.items[n];
    float* out = kind == 0 ? A.images + (size_t)n * 3 * S * S : (kind == 1 ? A.masks : A.ignores) + (size_t)n * S * S;
    ti_crops_body(TrainSrc{A, o, it}, o, it, A.bounds, A.kk8, A.lsum + n, kind, S, r0, out, s_src, s_rows);
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_train_rois(const uint8_t* scenes, const int32_t* items, int Fr, int B, int H, int W, int32_t* table, sdnStream stream)
{
    if (!scenes || !items || !table) return fail(SDN_EINVAL, "sdn_train_rois: null pointer");
    if (Fr < 1 || B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > INT_MAX / 4 || (long)Fr * H * W > INT_MAX)
        return fail(SDN_EINVAL, "sdn_train_rois: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_train_rois_init, dim3(cdiv(B, 256)), dim3(256), 0, st, table, B);
    if (int rc = check_launch("k_train_rois_init")) return rc;
    hipLaunchKernelGGL(k_train_rois, dim3(cdiv((long)H * W, 4 * TI_THREADS), (unsigned)B), dim3(TI_THREADS), 0, st, scenes, items, Fr, H,
                       W, table);
    return check_launch("k_train_rois");
}

SDN_API int sdn_train_crops(const uint8_t* frames, const uint8_t* scenes, int Fr, int H, int W, const int32_t* rois_host,
                            const int32_t* objs_host, const int32_t* objs, const int32_t* items_host, const int32_t* items, int B,
                            const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8, const uint8_t* nearer, int n_nearer,
                            int image_size, int mask_size, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                            void* workspace, float* images, float* masks, float* ignores, sdnStream stream)
{
    if (!frames || !scenes || !rois_host || !objs_host || !objs || !items_host || !items || !bounds || !kk8 || !workspace || !images ||
        !masks || !ignores || (n_nearer > 0 && !nearer))
        return fail(SDN_EINVAL, "sdn_train_crops: null pointer");
    if (Fr < 1 || B < 1 || B > 65535 || H < 1 || W < 1 || (long)Fr * H * W > INT_MAX / 3 || n_bounds < 1 || n_kk8 < 1 || n_nearer < 0)
        return fail(SDN_EINVAL, "sdn_train_crops: bad sizes");
    if (image_size < 1 || mask_size < 1 || image_size > TI_PLANE_BYTES || mask_size > TI_PLANE_BYTES)
        return fail(SDN_EINVAL, "sdn_train_crops: bad crop sizes %d, %d", image_size, mask_size);
    if (std0 == 0.f || std1 == 0.f || std2 == 0.f) return fail(SDN_EINVAL, "sdn_train_crops: std is 0");
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(SDN_EINVAL, "sdn_train_crops: workspace is not aligned to 8 bytes");
    static_assert(sizeof(TrainWin) == TI_OBJ_INTS * sizeof(int32_t), "object table row");
    static_assert(sizeof(TrainItem) == TI_ITEM_INTS * sizeof(int32_t), "item table row");
    long scon = 0;   // the widest window of an item with contrast
    for (int n = 0; n < B; n++) {
        const int32_t* r = rois_host + 4 * n;
        const int32_t* w = objs_host + (size_t)TI_OBJ_INTS * n;
        const int32_t* it = items_host + (size_t)TI_ITEM_INTS * n;
        if (r[2] <= r[0] || r[3] <= r[1])
            return fail(SDN_EINVAL, "sdn_train_crops: roi %d (%d, %d, %d, %d) is empty", n, r[0], r[1], r[2], r[3]);
        const long hh = (long)r[2] - r[0], ww = (long)r[3] - r[1];
        const long s = hh > ww ? hh : ww;
        if (s > TI_SRC_PIXELS)
            return fail(SDN_EINVAL, "sdn_train_crops: roi %d: a %ld pixel window; one source row must fit the %d pixel staging tile", n, s,
                        TI_SRC_PIXELS);
        if (w[2] != s || w[0] != r[0] - (s - hh) / 2 || w[1] != r[1] - (s - ww) / 2)
            return fail(SDN_EINVAL, "sdn_train_crops: item %d: the window (%d, %d, %d) is not crop_square's of the roi", n, w[0], w[1], w[2]);
        if (it[0] < 0 || it[0] >= Fr) return fail(SDN_EINVAL, "sdn_train_crops: item %d: frame %d outside [0, %d)", n, it[0], Fr);
        if (it[2] < 0 || it[3] < 0 || (long)it[2] + it[3] > n_nearer)
            return fail(SDN_EINVAL, "sdn_train_crops: item %d: nearer codes %d + %d outside the table of %d", n, it[2], it[3], n_nearer);
        if (it[4] < 0 || it[4] > 4 || it[9] < 0 || it[9] > 255)
            return fail(SDN_EINVAL, "sdn_train_crops: item %d: %d ops, hue shift %d", n, it[4], it[9]);
        int seen = 0;
        for (int k = 0; k < it[4]; k++) {
            const int op = (it[5] >> (4 * k)) & 15;
            if (op > TI_HUE || (seen >> op) & 1)
                return fail(SDN_EINVAL, "sdn_train_crops: item %d: order 0x%x is not a permutation of distinct ops", n, it[5]);
            seen |= 1 << op;
        }
        if ((seen >> TI_CONTRAST) & 1) {
            if (s > TI_MAX_CONTRAST_SIDE)
                return fail(SDN_EINVAL, "sdn_train_crops: item %d: contrast on a %ld pixel window (at most %d)", n, s, TI_MAX_CONTRAST_SIDE);
            scon = s > scon ? s : scon;
        }
        // Pillow's filter width for s -> S: 2 ceil(max(s / S, 1)) + 1 source rows per output row; they must fit the plane
        for (int which = 0; which < 2; which++) {
            const int S = which ? mask_size : image_size;
            const int32_t* t = w + 5 + 3 * which;
            if (s == S) {
                if (t[2] != 0) return fail(SDN_EINVAL, "sdn_train_crops: item %d: a table for the resize %ld -> %d Pillow skips", n, s, S);
                continue;
            }
            const long taps = 2 * ((s > S ? (s + S - 1) / S : 1)) + 1;
            if (taps + 1 > TI_PLANE_BYTES / S)
                return fail(SDN_EINVAL, "sdn_train_crops: roi %d: a %ld pixel window resized to %d needs %ld source rows per output "
                            "row, the LDS tile holds %d", n, s, S, taps + 1, TI_PLANE_BYTES / S);
            if (t[2] != taps || t[0] < 0 || t[1] < 0 || (long)t[0] + S > n_bounds || (long)t[1] + (long)S * taps > n_kk8)
                return fail(SDN_EINVAL, "sdn_train_crops: item %d: resampling table (%d, %d, %d) of %ld -> %d does not fit", n, t[0], t[1],
                            t[2], s, S);
        }
    }
    TrainParams A;
    A.frames = frames; A.scenes = scenes; A.objs = reinterpret_cast<const TrainWin*>(objs);
    A.items = reinterpret_cast<const TrainItem*>(items); A.bounds = bounds; A.kk8 = kk8; A.nearer = nearer;
    A.lsum = static_cast<unsigned long long*>(workspace);
    A.B = B; A.H = H; A.W = W; A.Si = image_size; A.Sm = mask_size;
    A.mean[0] = mean0; A.mean[1] = mean1; A.mean[2] = mean2; A.std[0] = std0; A.std[1] = std1; A.std[2] = std2;
    A.images = images; A.masks = masks; A.ignores = ignores;
    hipStream_t st = (hipStream_t)stream;
    if (scon) {
        if (hipMemsetAsync(workspace, 0, (size_t)B * sizeof(unsigned long long), st) != hipSuccess)
            return fail(SDN_ELAUNCH, "sdn_train_crops: clearing the sums failed");
        hipLaunchKernelGGL(k_train_stats, dim3(cdiv(scon * scon, TI_STAT_PIXELS), (unsigned)B), dim3(TI_THREADS), 0, st, A);
        if (int rc = check_launch("k_train_stats")) return rc;
    }
    const int Smax = image_size > mask_size ? image_size : mask_size;
    hipLaunchKernelGGL(k_train_crops, dim3(cdiv(Smax, TI_BAND), 3, (unsigned)B), dim3(TI_THREADS), 0, st, A);
    return check_launch("k_train_crops");
}
