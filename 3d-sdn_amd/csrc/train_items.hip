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

namespace sdn {

constexpr int TI_BITS = 22;             // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int TI_THREADS = 256;
constexpr int TI_WAVES = TI_THREADS / 64;
constexpr int TI_BAND = 8;              // output rows per workgroup
// LDS of k_train_crops, per channel (the image kind uses three, the mask and ignore kinds one):
//   staged source pixels   4 KiB: whole rows of the s-wide window, 4096 / s rows per pass (so s <= 4096)
//   resampled rows         12 KiB: the band's horizontally resampled source rows, one byte per pixel; 12288 / S rows (54 at
//                          224, 48 at 256; a band of 8 rows at the widest VKITTI window, 1242 -> 224, needs 49)
// 48 KiB per workgroup: three workgroups (12 waves) per CU in the 160 KiB of a gfx950 CU.
constexpr int TI_SRC_PIXELS = 4096;
constexpr int TI_PLANE_BYTES = 12288;
constexpr int TI_STAT_PIXELS = 2048;    // window pixels per workgroup of k_train_stats
constexpr int TI_OBJ_INTS = 12;
constexpr int TI_ITEM_INTS = 12;
constexpr int TI_MAX_CONTRAST_SIDE = 1448;   // s^2 <= 2^21: where the integer mean equals int(sum / n + 0.5) in float64

enum { TI_BRIGHTNESS = 0, TI_CONTRAST = 1, TI_SATURATION = 2, TI_HUE = 3 };

struct TrainWin {   // one row of derender3d.scene.crop_tables' object table (the layout of sdn_scene_crops)
    int oy, ox;                // frame coordinates of the window's first pixel
    int s;                     // side of the square window
    int xlim, ylim;            // frame coordinates where crop_square's padded image ends (beyond: 0)
    int boff_i, koff_i, ksize_i;   // tables of the resize s -> image_size (ksize 0: s == image_size, no resampling)
    int boff_m, koff_m, ksize_m;   // tables of the resize s -> mask_size
    int pad;
};

struct TrainItem {  // one row of the item table
    int frame;                 // index into frames / scenes
    int code;                  // r | g << 8 | b << 16 of the object's colour in the scene image
    int near_off, near_cnt;    // the item's nearer codes: rows near_off .. near_off + near_cnt of `nearer`
    int nops;                  // ops of the colour jitter, 0 .. 4
    int order;                 // op k in bits 4 k .. 4 k + 3
    float fb, fc, fs;          // brightness, contrast, saturation factors
    int hue;                   // added to H modulo 256
    int pad0, pad1;
};

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

__device__ __forceinline__ int ti_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int ti_wave_sum(int v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int ti_wave_min(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int ti_wave_max(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// ---- Pillow's arithmetic ---------------------------------------------------------------------------------------------------
// Image.blend(degenerate, image, alpha), one byte (Blend.c)
__device__ __forceinline__ int ti_blend(int d, int v, float a)
{
    const float t = (float)d + a * (float)(v - d);
    if (a >= 0.f && a <= 1.f) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int ti_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// C's round() of a value that is not negative: half away from zero, without forming x + 0.5
__device__ __forceinline__ int ti_round(double x)
{
    const double f = floor(x);
    return (int)f + ((x - f) >= 0.5 ? 1 : 0);
}

// convert('HSV'), H + shift modulo 256, convert('RGB') (Convert.c: rgb2hsv_row, hsv2rgb)
__device__ __forceinline__ void ti_hue(int shift, int& r, int& g, int& b)
{
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        double t = (double)h / 6.0 + 1.0;
        if (t >= 1.0) t = t - 1.0;   // fmod(t, 1.0) for t in [5/6, 11/6]
        h = (float)t;
        uh = ti_clip8((int)((double)h * 255.0));
        us = ti_clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double h6 = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double v = (double)(float)uv;
    const int p = ti_clip8(ti_round(v * (1.0 - (double)fs)));
    const int q = ti_clip8(ti_round(v * (1.0 - (double)(fs * f))));
    const int t = ti_clip8(ti_round(v * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// the ops [0, stop) of the item's order on one pixel; `grey` is the contrast op's solid grey
__device__ __forceinline__ void ti_jitter(const TrainItem& it, int stop, int grey, int& r, int& g, int& b)
{
    for (int k = 0; k < stop; k++) {
        const int op = (it.order >> (4 * k)) & 15;
        if (op == TI_BRIGHTNESS) {
            r = ti_blend(0, r, it.fb); g = ti_blend(0, g, it.fb); b = ti_blend(0, b, it.fb);
        } else if (op == TI_CONTRAST) {
            r = ti_blend(grey, r, it.fc); g = ti_blend(grey, g, it.fc); b = ti_blend(grey, b, it.fc);
        } else if (op == TI_SATURATION) {
            const int l = ti_luma(r, g, b);
            r = ti_blend(l, r, it.fs); g = ti_blend(l, g, it.fs); b = ti_blend(l, b, it.fs);
        } else {
            ti_hue(it.hue, r, g, b);
        }
    }
}

// position of the contrast op in the order, -1 without
__device__ __forceinline__ int ti_contrast_at(const TrainItem& it)
{
    for (int k = 0; k < it.nops; k++)
        if (((it.order >> (4 * k)) & 15) == TI_CONTRAST) return k;
    return -1;
}

// ---- the window's pixels as crop_square returns them ---------------------------------------------------------------------------
// 0: beyond the padded image (PIL's crop gives 0), 1: padding (the fill value), 2: inside the frame, *p its offset in a plane
__device__ __forceinline__ int ti_where(const TrainParams& A, const TrainWin& o, int wy, int wx, size_t* p)
{
    const int fy = o.oy + wy, fx = o.ox + wx;
    if (fx >= o.xlim || fy >= o.ylim) return 0;
    if ((unsigned)fy >= (unsigned)A.H || (unsigned)fx >= (unsigned)A.W) return 1;
    *p = (size_t)fy * A.W + fx;
    return 2;
}

__device__ __forceinline__ void ti_raw_rgb(const TrainParams& A, const TrainWin& o, const TrainItem& it, int wy, int wx, int& r,
                                           int& g, int& b)
{
    size_t p = 0;
    const int w = ti_where(A, o, wy, wx, &p);
    if (w < 2) {
        r = g = b = w ? 127 : 0;
        return;
    }
    const size_t HW = (size_t)A.H * A.W;
    const uint8_t* f = A.frames + (size_t)it.frame * 3 * HW + p;
    r = f[0];
    g = f[HW];
    b = f[2 * HW];
}

// kind 1: the mask byte, kind 2: the ignore byte np.uint8(255 * count)
__device__ __forceinline__ int ti_map_byte(const TrainParams& A, const TrainWin& o, const TrainItem& it, int kind, int wy, int wx)
{
    size_t p = 0;
    const int w = ti_where(A, o, wy, wx, &p);
    if (w < 2) return (w == 1 && kind == 2) ? 255 : 0;
    const uint8_t* s = A.scenes + ((size_t)it.frame * A.H * A.W + p) * 3;
    const int c = (int)s[0] | ((int)s[1] << 8) | ((int)s[2] << 16);
    if (kind == 1) return c == it.code ? 255 : 0;
    int count = 0;
    const uint8_t* nc = A.nearer + 3 * (size_t)it.near_off;
    for (int k = 0; k < it.near_cnt; k++) count += (c == ((int)nc[3 * k] | ((int)nc[3 * k + 1] << 8) | ((int)nc[3 * k + 2] << 16))) ? 1 : 0;
    return (255 * count) & 255;
}

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
    cnt = ti_wave_sum(cnt);
    if (cnt) {   // uniform over the wave
        ymin = ti_wave_min(ymin); xmin = ti_wave_min(xmin); ymax = ti_wave_max(ymax); xmax = ti_wave_max(xmax);
        if ((threadIdx.x & 63) == 0) {
            atomicMin(table + 5 * b, ymin);
            atomicMin(table + 5 * b + 1, xmin);
            atomicMax(table + 5 * b + 2, ymax + 1);
            atomicMax(table + 5 * b + 3, xmax + 1);
            atomicAdd(table + 5 * b + 4, cnt);
        }
    }
}

// ---- the contrast mean -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TI_THREADS) void k_train_stats(const TrainParams A)
{
    __shared__ int s_part[TI_WAVES];
    const int n = blockIdx.y, tid = threadIdx.x;
    const TrainItem it = A.items[n];
    const int at = ti_contrast_at(it);
    if (at < 0) return;
    const TrainWin o = A.objs[n];
    if (o.s < 1 || o.s > TI_MAX_CONTRAST_SIDE) return;   // the launcher checked the host's copy of the table
    const int total = o.s * o.s;
    const int i0 = blockIdx.x * TI_STAT_PIXELS;
    if (i0 >= total) return;
    const int i1 = min(i0 + TI_STAT_PIXELS, total);
    int acc = 0;   // at most 8 pixels of 255 per thread
    for (int i = i0 + tid; i < i1; i += TI_THREADS) {
        int r, g, b;
        ti_raw_rgb(A, o, it, i / o.s, i % o.s, r, g, b);
        ti_jitter(it, at, 0, r, g, b);
        acc += ti_luma(r, g, b);
    }
    acc = ti_wave_sum(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < TI_WAVES; w++) sum += s_part[w];
        if (sum) atomicAdd(A.lsum + n, (unsigned long long)sum);
    }
}

// ---- the crops -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TI_THREADS) void k_train_crops(const TrainParams A)
{
    __shared__ uint8_t s_src[3 * TI_SRC_PIXELS];
    __shared__ uint8_t s_rows[3 * TI_PLANE_BYTES];
    const int n = blockIdx.z, kind = blockIdx.y, tid = threadIdx.x;   // kind 0: image, 1: mask, 2: ignore
    const bool img = kind == 0;
    const int C = img ? 3 : 1;
    const int S = img ? A.Si : A.Sm;
    const int r0 = blockIdx.x * TI_BAND;
    if (r0 >= S) return;
    const int r1 = min(r0 + TI_BAND, S);
    const TrainWin o = A.objs[n];
    const TrainItem it = A.items[n];
    const int s = o.s;
    if (s < 1 || s > TI_SRC_PIXELS) return;   // the launcher checked the host's copy of the table; uniform over the workgroup
    const int ksize = img ? o.ksize_i : o.ksize_m;
    float* out = img ? A.images + (size_t)n * 3 * S * S : (kind == 1 ? A.masks : A.ignores) + (size_t)n * S * S;
    int grey = 0;
    if (img && ti_contrast_at(it) >= 0) {   // int(mean(L) + 0.5) = (2 sum + n) / (2 n) in integers
        const unsigned long long cnt = (unsigned long long)s * s;
        grey = (int)((2ull * A.lsum[n] + cnt) / (2ull * cnt));
    }

    if (ksize == 0) {   // s == S: Pillow skips both passes
        for (int i = tid; i < (r1 - r0) * S; i += TI_THREADS) {
            const int y = r0 + i / S, x = i % S;
            if (img) {
                int c[3];
                ti_raw_rgb(A, o, it, y, x, c[0], c[1], c[2]);
                ti_jitter(it, it.nops, grey, c[0], c[1], c[2]);
                for (int ch = 0; ch < 3; ch++)
                    out[((size_t)ch * S + y) * S + x] = ((float)c[ch] / 255.f - A.mean[ch]) / A.std[ch];
            } else {
                out[(size_t)y * S + x] = (float)ti_map_byte(A, o, it, kind, y, x) / 255.f;
            }
        }
        return;
    }
    const int* b = A.bounds + 2 * (img ? o.boff_i : o.boff_m);
    const int* k = A.kk8 + (img ? o.koff_i : o.koff_m);
    const int cap = TI_PLANE_BYTES / S;      // resampled source rows a plane holds (the launcher checked ksize < cap)
    const int per = TI_SRC_PIXELS / s;       // whole source rows staged per pass (the launcher checked s <= 4096)
    int ra = r0;
    while (ra < r1) {
        // the longest run of output rows from ra whose source rows fit the plane (uniform over the workgroup)
        const int ybase = b[2 * ra];
        int rb = ra + 1, yend = ybase + b[2 * ra + 1];
        while (rb < r1 && b[2 * rb] + b[2 * rb + 1] - ybase <= cap) {
            yend = max(yend, b[2 * rb] + b[2 * rb + 1]);
            rb++;
        }
        const int rows = max(1, min(min(yend, s) - ybase, cap));
        for (int c0 = 0; c0 < rows; c0 += per) {
            const int cn = min(per, rows - c0);
            // stage: the source rows ybase + c0 .. + cn of the window, jittered / tested once per pixel
            for (int i = tid; i < cn * s; i += TI_THREADS) {
                const int wy = min(ybase + c0 + i / s, s - 1), wx = i % s;
                if (img) {
                    int cr, cg, cb;
                    ti_raw_rgb(A, o, it, wy, wx, cr, cg, cb);
                    ti_jitter(it, it.nops, grey, cr, cg, cb);
                    s_src[i] = (uint8_t)cr;
                    s_src[TI_SRC_PIXELS + i] = (uint8_t)cg;
                    s_src[2 * TI_SRC_PIXELS + i] = (uint8_t)cb;
                } else {
                    s_src[i] = (uint8_t)ti_map_byte(A, o, it, kind, wy, wx);
                }
            }
            __syncthreads();
            // horizontal pass out of the staged rows, rounded to uint8 as Pillow stores them
            for (int i = tid; i < C * cn * S; i += TI_THREADS) {
                const int ch = i / (cn * S), j = i - ch * (cn * S);
                const int ry = j / S, x = j % S;
                const int x0 = max(b[2 * x], 0), xc = min(b[2 * x + 1], ksize);
                const uint8_t* src = s_src + ch * TI_SRC_PIXELS + ry * s;
                int acc = 1 << (TI_BITS - 1);
                for (int t = 0; t < xc; t++) acc += (int)src[min(x0 + t, s - 1)] * k[x * ksize + t];
                s_rows[ch * TI_PLANE_BYTES + (c0 + ry) * S + x] = (uint8_t)ti_clip8(acc >> TI_BITS);
            }
            __syncthreads();
        }
        // vertical pass, to_tensor, Normalize
        for (int i = tid; i < C * (rb - ra) * S; i += TI_THREADS) {
            const int ch = i / ((rb - ra) * S), j = i - ch * ((rb - ra) * S);
            const int y = ra + j / S, x = j % S;
            const int y0 = b[2 * y] - ybase, yc = min(b[2 * y + 1], ksize);
            const uint8_t* plane = s_rows + ch * TI_PLANE_BYTES;
            int acc = 1 << (TI_BITS - 1);
            for (int t = 0; t < yc; t++) acc += (int)plane[min(max(y0 + t, 0), rows - 1) * S + x] * k[y * ksize + t];
            float v = (float)ti_clip8(acc >> TI_BITS) / 255.f;
            if (img) v = (v - A.mean[ch]) / A.std[ch];
            out[((size_t)ch * S + y) * S + x] = v;
        }
        __syncthreads();
        ra = rb;
    }
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
