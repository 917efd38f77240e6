// Index arithmetic, the LDS plan and HOST table validation of the semantic training batch (segm_train.hip).  Plain C++ so that a
// host program can walk the band spans and the validator without the HIP runtime (tools/segm_train_check.cpp).
#pragma once

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "check_common.h"
#include "segm_tail_check.h"   // the colour table: SEG_MAX_COLORS, seg_validate_colors, seg_find

namespace sdn {

constexpr int SGT_THREADS = 256;
constexpr int SGT_BAND = 4;                  // output rows of a workgroup of the image kernel
// LDS of k_segm_train_image, per colour plane (three planes):
//   staged source pixels   4 KiB: whole frame rows after jitter and flip, 4096 / W rows per pass (so W <= 4096)
//   resampled rows         12 KiB: the band's horizontally resampled source rows, one byte per pixel: 12288 / w rows
// 48 KiB per workgroup: three workgroups (12 waves) per CU in the 160 KiB of a gfx950 CU.  Rows a band of 4 needs at the
// reference's sizes (frames 375 x 1242, imgMaxSize 1274; tools/segm_train_check.cpp prints them from Pillow's bounds):
//   short size 100   331 bytes a row, 9 taps: 19 of the 37 that fit
//   short size 150   496 bytes a row, 7 taps: 12 of 24
//   short size 200   662 bytes a row, 5 taps:  9 of 18
//   short size 300   993 bytes a row, 5 taps:  7 of 12
//   short size 375   no resample:              4 of  9 (1242 bytes a row)
//   384 x 1273       the upscale, 3 taps:      5 of  9
// A band of 8 rows at short size 300 would need 13 rows of 993 bytes = 12 909, more than a 12 KiB plane; and a batch of two
// frames has only 2 x 26 .. 2 x 94 bands of 4 for 256 CUs, so shorter bands finish sooner than fuller ones.
constexpr int SGT_SRC_PIXELS = 4096;
constexpr int SGT_PLANE_BYTES = 12288;
constexpr int SGT_STAT_PIXELS = 2048;        // frame pixels per workgroup of k_segm_train_luma
constexpr long SGT_MAX_CONTRAST_PIXELS = 1L << 21;   // where the integer mean equals int(sum / n + 0.5) in float64; the sum fits an int
constexpr int SGT_MAX_SIDE = 16384;          // Hb, Wb
constexpr int SGT_ITEM_INTS = 20;
constexpr int SGT_BITS = 22;                 // Pillow Resample.c: PRECISION_BITS

struct SegTrainItem {   // one row of the item table, at the start of the table buffer; every offset counts ints from its start
    int h, w;                  // the item's resized size (vkitti_dataset.py:97)
    int flip;                  // 1: columns mirrored (:135-136)
    int nops, order;           // the colour jitter: op k in bits 4 k .. 4 k + 3 of order
    float fb, fc, fs;          // brightness, contrast, saturation factors
    int hue;                   // added to H modulo 256
    int xb, xk, xksize;        // Pillow's bilinear tables W -> w: bounds [w][2], coefficients [w][xksize]; xksize 0: w == W, pass skipped
    int yb, yk, yksize;        // H -> h
    int xn, yn;                // Pillow's NEAREST source indices W -> w [w] and H -> h [h]
    int ct, K;                 // the colour table: K ascending codes, then K labels
    int pad;
};
static_assert(sizeof(SegTrainItem) == SGT_ITEM_INTS * sizeof(int32_t), "item table row");

// Pillow's filter width for in -> out with the bilinear filter: 2 ceil(max(in / out, 1)) + 1
inline int sgt_taps(int in, int out) { return 2 * (in > out ? (in + out - 1) / out : 1) + 1; }

// the source rows [*first, *first + *count) the output rows r0 .. r1 - 1 read; bounds [.][2] = (first, count) per output row,
// or null for a skipped pass (row y reads row y)
inline void sgt_band_span(const int32_t* bounds, int r0, int r1, int* first, int* count)
{
    if (!bounds) {
        *first = r0;
        *count = r1 - r0;
        return;
    }
    int lo = INT_MAX, hi = 0;
    for (int y = r0; y < r1; y++) {
        const int a = bounds[2 * y], e = a + bounds[2 * y + 1];
        lo = a < lo ? a : lo;
        hi = e > hi ? e : hi;
    }
    *first = lo;
    *count = hi - lo;
}

// one resampling table of an item: its place in the buffer and every entry
inline int sgt_validate_axis(const int32_t* T, long n, long first_free, int item, const char* axis, int in, int out, int boff, int koff,
                             int ksize, char* msg, size_t cap)
{
    if (in == out) {
        if (ksize != 0) SDN_FAIL("item %d: a table for the %s resize %d -> %d, which Pillow skips", item, axis, in, out);
        return 0;
    }
    if (ksize != sgt_taps(in, out)) SDN_FAIL("item %d: %d taps for the %s resize %d -> %d, Pillow uses %d", item, ksize, axis, in, out, sgt_taps(in, out));
    if (boff < first_free || koff < first_free || (long)boff + 2L * out > n || (long)koff + (long)out * ksize > n)
        SDN_FAIL("item %d: the %s tables (%d, %d) of %d -> %d lie outside the buffer of %ld ints", item, axis, boff, koff, in, out, n);
    for (int i = 0; i < out; i++) {
        const int a = T[boff + 2 * i], c = T[boff + 2 * i + 1];
        if (a < 0 || c < 1 || c > ksize || (long)a + c > in)
            SDN_FAIL("item %d: %s bounds of output %d are (%d, %d) for %d inputs and %d taps", item, axis, i, a, c, in, ksize);
    }
    return 0;
}

// 0 when the HOST copy of the table buffer of sdn_segm_train_batch is valid and fits the LDS plan; otherwise 1 with the reason
inline int sgt_validate(const int32_t* T, long n, int B, int H, int W, int Hb, int Wb, int rate, char* msg, size_t cap)
{
    if (B < 1 || B > 65535) SDN_FAIL("%d items; 1 to 65535 are supported", B);
    if (H < 1 || W < 1 || (long)H * W > INT_MAX / 4 || (long)B * H * W > INT_MAX / 3) SDN_FAIL("bad sizes: %d frames of %d x %d", B, H, W);
    if (W > SGT_SRC_PIXELS) SDN_FAIL("frames %d pixels wide: one frame row must fit the %d pixel staging tile", W, SGT_SRC_PIXELS);
    if (Hb < 1 || Wb < 1 || Hb > SGT_MAX_SIDE || Wb > SGT_MAX_SIDE) SDN_FAIL("bad sizes: a %d x %d batch", Hb, Wb);
    if (rate < 1 || rate > Hb || rate > Wb) SDN_FAIL("label rate %d for a %d x %d batch", rate, Hb, Wb);
    const long first_free = (long)B * SGT_ITEM_INTS;
    if (n < first_free) SDN_FAIL("a buffer of %ld ints cannot hold %d item rows", n, B);
    for (int i = 0; i < B; i++) {
        SegTrainItem it;
        std::memcpy(&it, T + (size_t)i * SGT_ITEM_INTS, sizeof(it));
        if (it.h < 1 || it.w < 1 || it.h > Hb || it.w > Wb) SDN_FAIL("item %d: resized to %d x %d in a %d x %d batch", i, it.h, it.w, Hb, Wb);
        if ((it.h + rate - 1) / rate > Hb / rate || (it.w + rate - 1) / rate > Wb / rate)
            SDN_FAIL("item %d: the labels of %d x %d at rate %d do not fit the %d x %d map (the reference fails there too)", i, it.h, it.w,
                     rate, Hb / rate, Wb / rate);
        if (it.flip != 0 && it.flip != 1) SDN_FAIL("item %d: flip %d", i, it.flip);
        if (it.nops < 0 || it.nops > 4 || it.hue < 0 || it.hue > 255) SDN_FAIL("item %d: %d ops, hue shift %d", i, it.nops, it.hue);
        int seen = 0;
        for (int k = 0; k < it.nops; k++) {
            const int op = (it.order >> (4 * k)) & 15;
            if (op > 3 || (seen >> op) & 1) SDN_FAIL("item %d: order 0x%x is not a permutation of distinct ops", i, it.order);
            seen |= 1 << op;
        }
        if (((seen >> 1) & 1) && (long)H * W > SGT_MAX_CONTRAST_PIXELS)
            SDN_FAIL("item %d: contrast on a frame of %ld pixels (at most %ld)", i, (long)H * W, SGT_MAX_CONTRAST_PIXELS);
        if (sgt_validate_axis(T, n, first_free, i, "horizontal", W, it.w, it.xb, it.xk, it.xksize, msg, cap)) return 1;
        if (sgt_validate_axis(T, n, first_free, i, "vertical", H, it.h, it.yb, it.yk, it.yksize, msg, cap)) return 1;
        // the LDS plan: every band's resampled source rows in one plane
        const int rows_cap = SGT_PLANE_BYTES / it.w;
        for (int r0 = 0; r0 < it.h; r0 += SGT_BAND) {
            const int r1 = r0 + SGT_BAND < it.h ? r0 + SGT_BAND : it.h;
            int first, count;
            sgt_band_span(it.yksize ? T + it.yb : nullptr, r0, r1, &first, &count);
            if (count > rows_cap)
                SDN_FAIL("item %d: %d x %d -> %d x %d does not fit the LDS plan: the output rows %d .. %d need %d source rows of %d "
                         "bytes, a plane holds %d", i, H, W, it.h, it.w, r0, r1 - 1, count, it.w, rows_cap);
        }
        if (it.xn < first_free || it.yn < first_free || (long)it.xn + it.w > n || (long)it.yn + it.h > n)
            SDN_FAIL("item %d: the NEAREST tables (%d, %d) lie outside the buffer of %ld ints", i, it.xn, it.yn, n);
        for (int x = 0; x < it.w; x++)
            if (T[it.xn + x] < 0 || T[it.xn + x] >= W) SDN_FAIL("item %d: NEAREST column %d reads column %d of %d", i, x, T[it.xn + x], W);
        for (int y = 0; y < it.h; y++)
            if (T[it.yn + y] < 0 || T[it.yn + y] >= H) SDN_FAIL("item %d: NEAREST row %d reads row %d of %d", i, y, T[it.yn + y], H);
        if (it.K < 1 || it.K > SEG_MAX_COLORS) SDN_FAIL("item %d: %d colour codes; 1 to %d are supported", i, it.K, SEG_MAX_COLORS);
        if (it.ct < first_free || (long)it.ct + 2L * it.K > n) SDN_FAIL("item %d: the colour table at %d lies outside the buffer of %ld ints", i, it.ct, n);
        char why[160];
        if (seg_validate_colors(T + it.ct, it.K, why, sizeof(why))) SDN_FAIL("item %d: %s", i, why);
    }
    return 0;
}

}  // namespace sdn
