// Device code shared by the kernels that make training items: the tile constants, the window and item rows, and Pillow's colour
// arithmetic as torchvision 0.2.1 calls it, restated operation for operation (tests/geo_train_util.py holds the same statements
// in numpy against the installed Pillow).  What is shared, and by whom:
//   ti_resample_byte, ti_jitter, ti_contrast_at (templates over the row that carries the jitter), ti_block_sum, ti_grey   all four sources
//   ti_where, ti_raw_rgb, ti_map_outside, ti_code_byte, ti_stats_body, ti_crops_body   train_items.hip and train_hybrid.hip: the
//                                             crop_square window of one frame and the two kernel bodies over a pixel source
//   ti_luma_body, ti_band_body                segm_train.hip and training_item.hip: the whole-frame luma partials and the band
//                                             scheme of their image kernels; each keeps its own vertical pass and store
// Include only from files compiled without FMA contraction.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "device_common.h"

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

// One byte of a pass of Pillow's ImagingResample over 8-bit data (22-bit fixed point, rounded and clipped as Pillow stores it): the
// taps first .. first + count of the bytes p[i * stride], the index held inside [0, last].
__device__ __forceinline__ int ti_resample_byte(const uint8_t* p, int stride, int first, int count, int last, const int32_t* k)
{
    int acc = 1 << (TI_BITS - 1);
    for (int t = 0; t < count; t++) acc += (int)p[min(max(first + t, 0), last) * stride] * k[t];
    return clip8(acc >> TI_BITS);
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
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
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
    const int p = clip8(ti_round(v * (1.0 - (double)fs)));
    const int q = clip8(ti_round(v * (1.0 - (double)(fs * f))));
    const int t = clip8(ti_round(v * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// An Item below is any row that carries the jitter under the names nops, order, fb, fc, fs, hue: TrainItem, MixItem
// (train_hybrid_check.h), SegTrainItem (segm_train_check.h), TriPlan (training_item_check.h).
// the ops [0, stop) of the item's order on one pixel; `grey` is the contrast op's solid grey
template <class Item>
__device__ __forceinline__ void ti_jitter(const Item& it, int stop, int grey, int& r, int& g, int& b)
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
template <class Item>
__device__ __forceinline__ int ti_contrast_at(const Item& it)
{
    for (int k = 0; k < it.nops; k++)
        if (((it.order >> (4 * k)) & 15) == TI_CONTRAST) return k;
    return -1;
}

// the sum of `acc` over the workgroup, in every thread; s_part: TI_WAVES ints of LDS
__device__ __forceinline__ int ti_block_sum(int acc, int* s_part)
{
    const int tid = threadIdx.x;
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    int sum = 0;
    for (int w = 0; w < TI_WAVES; w++) sum += s_part[w];
    return sum;
}

// int(mean(L) + 0.5), the contrast op's solid grey, of `cnt` pixels whose L sum to `sum`: (2 sum + n) / (2 n) in integers
__device__ __forceinline__ int ti_grey(unsigned long long sum, unsigned long long cnt) { return (int)((2ull * sum + cnt) / (2ull * cnt)); }

// ---- the window's pixels as crop_square returns them, of a frame of H x W ------------------------------------------------------
// 0: beyond the padded image (PIL's crop gives 0), 1: padding (the fill value), 2: inside the frame, *p its offset in a plane
__device__ __forceinline__ int ti_where(const TrainWin& o, int H, int W, int wy, int wx, size_t* p)
{
    const int fy = o.oy + wy, fx = o.ox + wx;
    if (fx >= o.xlim || fy >= o.ylim) return 0;
    if ((unsigned)fy >= (unsigned)H || (unsigned)fx >= (unsigned)W) return 1;
    *p = (size_t)fy * W + fx;
    return 2;
}

// frame: uint8 [3, H, W]
__device__ __forceinline__ void ti_raw_rgb(const TrainWin& o, const uint8_t* frame, int H, int W, int wy, int wx, int& r, int& g, int& b)
{
    size_t p = 0;
    const int w = ti_where(o, H, W, wy, wx, &p);
    if (w < 2) {
        r = g = b = w ? 127 : 0;
        return;
    }
    const size_t HW = (size_t)H * W;
    const uint8_t* f = frame + p;
    r = f[0];
    g = f[HW];
    b = f[2 * HW];
}

// kind 1: the mask byte, kind 2: the ignore byte.  -1 inside the frame, where the byte comes from the item's source at *p;
// outside, the byte itself (the ignore map is padded with 255)
__device__ __forceinline__ int ti_map_outside(const TrainWin& o, int H, int W, int kind, int wy, int wx, size_t* p)
{
    const int w = ti_where(o, H, W, wy, wx, p);
    return w == 2 ? -1 : ((w == 1 && kind == 2) ? 255 : 0);
}

// the byte of a colour-coded scene [H, W, 3] at pixel p: kind 1 the test against `code`, kind 2 np.uint8(255 * count) of the
// `cnt` nearer codes at `nc`
__device__ __forceinline__ int ti_code_byte(const uint8_t* scene, size_t p, int kind, int code, const uint8_t* nc, int cnt)
{
    const int c = code24(scene + 3 * p);
    if (kind == 1) return c == code ? 255 : 0;
    int count = 0;
    for (int k = 0; k < cnt; k++) count += (c == code24(nc + 3 * k)) ? 1 : 0;
    return (255 * count) & 255;
}

// ---- the kernel bodies.  ti_stats_body and ti_crops_body are shared by k_train_stats / k_train_crops (train_items.hip) and their
// per-item-source forms (train_hybrid.hip); ti_luma_body and ti_band_body, further down, by the whole-frame image kernels of
// segm_train.hip and training_item.hip.  The LDS arrays are declared in the kernels and passed in.
// A Src is one item's source of pixels:
//   void rgb(int wy, int wx, int& r, int& g, int& b) const   the window's pixel as crop_square returns it (fill 127, beyond the
//                                                            padded image 0), before the colour jitter
//   int map_byte(int kind, int wy, int wx) const             kind 1: the mask byte, kind 2: the ignore byte
//   float mean(int ch) const, float stdev(int ch) const      Normalize's constants
// Every branch on the arguments is uniform over the workgroup.

// the sum of L over the s x s window after the ops that precede contrast; s_part: TI_WAVES ints of LDS
template <class Src, class Item>
__device__ __forceinline__ void ti_stats_body(const Src& src, const TrainWin& o, const Item& it, unsigned long long* lsum, int* s_part)
{
    const int tid = threadIdx.x;
    const int at = ti_contrast_at(it);
    if (at < 0) return;
    if (o.s < 1 || o.s > TI_MAX_CONTRAST_SIDE) return;   // the launcher checked the host's copy of the table
    const int total = o.s * o.s;
    const int i0 = blockIdx.x * TI_STAT_PIXELS;
    if (i0 >= total) return;
    const int i1 = min(i0 + TI_STAT_PIXELS, total);
    int acc = 0;   // at most 8 pixels of 255 per thread
    for (int i = i0 + tid; i < i1; i += TI_THREADS) {
        int r, g, b;
        src.rgb(i / o.s, i % o.s, r, g, b);
        ti_jitter(it, at, 0, r, g, b);
        acc += ti_luma(r, g, b);
    }
    const int sum = ti_block_sum(acc, s_part);
    if (tid == 0 && sum) atomicAdd(lsum, (unsigned long long)sum);
}

// the output rows r0 .. r0 + TI_BAND of one (item, kind): kind 0 the image [3, S, S], 1 the mask, 2 the ignore map [S, S] at `out`.
// s_src: 3 TI_SRC_PIXELS bytes of LDS, s_rows: 3 TI_PLANE_BYTES bytes.
template <class Src, class Item>
__device__ __forceinline__ void ti_crops_body(const Src& src, const TrainWin& o, const Item& it, const int32_t* bounds,
                                              const int32_t* kk8, const unsigned long long* lsum, int kind, int S, int r0, float* out,
                                              uint8_t* s_src, uint8_t* s_rows)
{
    const int tid = threadIdx.x;
    const bool img = kind == 0;
    const int C = img ? 3 : 1;
    const int r1 = min(r0 + TI_BAND, S);
    const int s = o.s;
    if (s < 1 || s > TI_SRC_PIXELS) return;   // the launcher checked the host's copy of the table; uniform over the workgroup
    const int ksize = img ? o.ksize_i : o.ksize_m;
    int grey = 0;
    if (img && ti_contrast_at(it) >= 0) grey = ti_grey(*lsum, (unsigned long long)s * s);

    if (ksize == 0) {   // s == S: Pillow skips both passes
        for (int i = tid; i < (r1 - r0) * S; i += TI_THREADS) {
            const int y = r0 + i / S, x = i % S;
            if (img) {
                int c[3];
                src.rgb(y, x, c[0], c[1], c[2]);
                ti_jitter(it, it.nops, grey, c[0], c[1], c[2]);
                for (int ch = 0; ch < 3; ch++)
                    out[((size_t)ch * S + y) * S + x] = ((float)c[ch] / 255.f - src.mean(ch)) / src.stdev(ch);
            } else {
                out[(size_t)y * S + x] = (float)src.map_byte(kind, y, x) / 255.f;
            }
        }
        return;
    }
    const int* b = bounds + 2 * (img ? o.boff_i : o.boff_m);
    const int* k = kk8 + (img ? o.koff_i : o.koff_m);
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
                    src.rgb(wy, wx, cr, cg, cb);
                    ti_jitter(it, it.nops, grey, cr, cg, cb);
                    s_src[i] = (uint8_t)cr;
                    s_src[TI_SRC_PIXELS + i] = (uint8_t)cg;
                    s_src[2 * TI_SRC_PIXELS + i] = (uint8_t)cb;
                } else {
                    s_src[i] = (uint8_t)src.map_byte(kind, wy, wx);
                }
            }
            __syncthreads();
            // horizontal pass out of the staged rows, rounded to uint8 as Pillow stores them
            for (int i = tid; i < C * cn * S; i += TI_THREADS) {
                const int ch = i / (cn * S), j = i - ch * (cn * S);
                const int ry = j / S, x = j % S;
                const int x0 = max(b[2 * x], 0), xc = min(b[2 * x + 1], ksize);
                const uint8_t* row = s_src + ch * TI_SRC_PIXELS + ry * s;
                s_rows[ch * TI_PLANE_BYTES + (c0 + ry) * S + x] = (uint8_t)ti_resample_byte(row, 1, x0, xc, s - 1, k + x * ksize);
            }
            __syncthreads();
        }
        // vertical pass, to_tensor, Normalize
        for (int i = tid; i < C * (rb - ra) * S; i += TI_THREADS) {
            const int ch = i / ((rb - ra) * S), j = i - ch * ((rb - ra) * S);
            const int y = ra + j / S, x = j % S;
            const int y0 = b[2 * y] - ybase, yc = min(b[2 * y + 1], ksize);
            const uint8_t* plane = s_rows + ch * TI_PLANE_BYTES;
            float v = (float)ti_resample_byte(plane + x, S, y0, yc, rows - 1, k + y * ksize) / 255.f;
            if (img) v = (v - src.mean(ch)) / src.stdev(ch);
            out[((size_t)ch * S + y) * S + x] = v;
        }
        __syncthreads();
        ra = rb;
    }
}

// ---- whole frames: `frame` is uint8 [H, W, 3], the jitter's grey is that of the whole frame ------------------------------------
// One partial sum of L for the contrast op: workgroup blockIdx.x sums L over TI_STAT_PIXELS pixels of the frame as it is after
// the ops that precede contrast and writes ONE int at partial[blockIdx.x]; no atomics.  s_part: TI_WAVES ints of LDS.
template <class Item>
__device__ __forceinline__ void ti_luma_body(const Item& it, const uint8_t* frame, int total, int32_t* partial, int* s_part)
{
    const int tid = threadIdx.x;
    const int at = ti_contrast_at(it);
    if (at < 0) return;   // uniform over the workgroup
    const int i0 = blockIdx.x * TI_STAT_PIXELS, i1 = min(i0 + TI_STAT_PIXELS, total);
    int acc = 0;   // at most 8 pixels of 255 per thread
    for (int i = i0 + tid; i < i1; i += TI_THREADS) {
        int r = frame[3 * (size_t)i], g = frame[3 * (size_t)i + 1], b = frame[3 * (size_t)i + 2];
        ti_jitter(it, at, 0, r, g, b);
        acc += ti_luma(r, g, b);
    }
    const int sum = ti_block_sum(acc, s_part);
    if (tid == 0) partial[blockIdx.x] = sum;
}

// The band scheme of the image kernels up to and including Pillow's horizontal pass, for the rows r0 .. rh - 1 of the frame
// resized to w columns (`it` also names Pillow's tables in T: xb, xk, xksize, yb, yksize; a ksize of 0 is a pass Pillow skips):
// the grey from the nblk partials, the frame rows ybase .. ybase + rows - 1 the band's vertical pass reads, those rows staged
// through s_src (3 TI_SRC_PIXELS bytes) with the jitter applied once per source pixel, mirrored THERE when `mirror`, and the
// horizontal pass into bytes at s_rows[ch * TI_PLANE_BYTES + (row - ybase) * w + x].  rh <= r0 (a band of padding) stages nothing
// and leaves ybase = 0, rows = 1.  False, and nothing done, on sizes the launcher's check of the host's tables excludes.
// Every branch is uniform over the workgroup.
template <class Item>
__device__ __forceinline__ bool ti_band_body(const Item& it, const int32_t* T, const uint8_t* frame, int H, int W, int w, int r0, int rh,
                                             bool mirror, const int32_t* partial, int nblk, uint8_t* s_src, uint8_t* s_rows, int* s_part,
                                             int& ybase, int& rows)
{
    const int tid = threadIdx.x;
    ybase = 0;
    rows = 1;
    if (w < 1 || w > TI_PLANE_BYTES || W > TI_SRC_PIXELS) return false;
    if (rh <= r0) return true;
    int grey = 0;
    if (ti_contrast_at(it) >= 0) {   // the sum is below 2^21 * 255
        int acc = 0;
        for (int i = tid; i < nblk; i += TI_THREADS) acc += partial[i];
        grey = ti_grey((unsigned long long)ti_block_sum(acc, s_part), (unsigned long long)H * W);
    }
    if (it.yksize == 0) {
        ybase = r0;
        rows = rh - r0;
    } else {
        const int32_t* yb = T + it.yb;
        int lo = INT_MAX, hi = 0;
        for (int y = r0; y < rh; y++) {
            lo = min(lo, yb[2 * y]);
            hi = max(hi, yb[2 * y] + yb[2 * y + 1]);
        }
        ybase = lo;
        rows = hi - lo;
    }
    ybase = min(max(ybase, 0), H - 1);
    rows = max(1, min(min(rows, H - ybase), TI_PLANE_BYTES / w));
    const int32_t* xb = T + it.xb;
    const int32_t* xk = T + it.xk;
    const int xksize = it.xksize;
    const int per = TI_SRC_PIXELS / W;   // whole frame rows staged per pass
    for (int c0 = 0; c0 < rows; c0 += per) {
        const int cn = min(per, rows - c0);
        // stage: the frame rows ybase + c0 .. + cn, jittered once per pixel
        for (int i = tid; i < cn * W; i += TI_THREADS) {
            const int ry = i / W, sx = i - ry * W;
            const int sy = min(ybase + c0 + ry, H - 1), fx = mirror ? W - 1 - sx : sx;
            const uint8_t* p = frame + ((size_t)sy * W + fx) * 3;
            int cr = p[0], cg = p[1], cb = p[2];
            ti_jitter(it, it.nops, grey, cr, cg, cb);
            s_src[i] = (uint8_t)cr;
            s_src[TI_SRC_PIXELS + i] = (uint8_t)cg;
            s_src[2 * TI_SRC_PIXELS + i] = (uint8_t)cb;
        }
        __syncthreads();
        // horizontal pass out of the staged rows, rounded to uint8 as Pillow stores them; a copy when Pillow skips it
        for (int i = tid; i < 3 * cn * w; i += TI_THREADS) {
            const int ch = i / (cn * w), j = i - ch * (cn * w);
            const int ry = j / w, x = j - ry * w;
            const uint8_t* row = s_src + ch * TI_SRC_PIXELS + ry * W;
            int v;
            if (xksize == 0) v = row[min(x, W - 1)];
            else v = ti_resample_byte(row, 1, max(xb[2 * x], 0), min(xb[2 * x + 1], xksize), W - 1, xk + x * xksize);
            s_rows[ch * TI_PLANE_BYTES + (c0 + ry) * w + x] = (uint8_t)v;
        }
        __syncthreads();
    }
    return true;
}

}  // namespace sdn
