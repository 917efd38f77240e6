// Index arithmetic and HOST table validation of the semantic tail (segm_tail.hip).  Plain C++ so that a host program can walk
// the footprint bounds and the validators without the HIP runtime (tools/segm_tail_check.cpp).
#pragma once

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "check_common.h"

namespace sdn {

constexpr int SEG_MAX_SCALES = 8;
constexpr int SEG_MAX_CLASSES = 32;        // sdn_segm_fuse
constexpr int SEG_MAX_SIDE = 16384;        // H, W, h_s, w_s: (dst + 0.5) * scale stays far inside fp32's exact integers
constexpr int SEG_TILE_H = 8;              // output rows of a workgroup
constexpr int SEG_TILE_W = 32;             // output columns of a workgroup; SEG_TILE_H * SEG_TILE_W threads, one pixel each
// A map may be up to twice the output per axis (h_s <= 2 H: a downsampling scale keeps both of its taps).  The source
// positions of a tile's first and last row then differ by at most 2 * 7 = 14, plus less than 1 of rounding: their integer
// parts differ by at most 15, the second tap adds one row: at most 17 rows, 18 kept.  Columns: 2 * 31 = 62 -> at most 65, 66 kept.
constexpr int SEG_FOOT_ROWS = 18;
constexpr int SEG_FOOT_COLS = 66;
constexpr int SEG_FOOT_MAX = SEG_FOOT_ROWS * SEG_FOOT_COLS;   // 1188 source positions
// LDS of k_segm_fuse: the footprint of ONE scale is staged at a time, in chunks of as many classes as fit SEG_LDS_FLOATS (the
// interpolated scores of a pixel wait in registers until its last chunk): 1188 positions x 8 classes x 4 B = 38 016 B at the
// largest case (S = 8, C = 32, every map twice the output: 8 x 4 chunks), whatever S and C are.  Four workgroups of 256 threads
// fit the 160 KiB of a CU (152 KiB), twice the two asked for; an upsampling scale (ratio <= 1: at most 10 x 34 positions)
// stages all 32 classes in two chunks.
constexpr int SEG_CHUNK_MIN = 8;
constexpr int SEG_LDS_FLOATS = SEG_FOOT_MAX * SEG_CHUNK_MIN;

constexpr int SEG_MAX_COLORS = 1024;       // sdn_segm_labels_from_colors
constexpr int SEG_MAX_CONF_CLASSES = 256;  // sdn_segm_confusion: the prediction is a uint8
constexpr int SEG_UNKNOWN = -32768;

struct SegScale {   // one row of the table of sdn_segm_fuse, 4 ints
    uint64_t scores;   // address of the fp32 [B, C, h, w] map
    int h, w;
};
static_assert(sizeof(SegScale) == 4 * sizeof(int32_t), "scale table row");

// nn.functional.upsample(mode='bilinear') as semantic/models.py:401 calls it (align_corners=False, torch 0.4's default): the
// source position max(0, (dst + 0.5) * (in / out) - 0.5) with a float quotient; the taps i0, i1 and the weight l1 of the second
// (the first weighs 1 - l1)
SDN_HD float seg_scale(int in, int out) { return (float)in / (float)out; }
SDN_HD void seg_taps(float scale, int dst, int in, int* i0, int* i1, float* l1)
{
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int a = (int)src;
    if (a > in - 1) a = in - 1;   // cannot happen for scale = in / out; keeps every index inside the map regardless
    *i0 = a;
    *i1 = a + (a < in - 1 ? 1 : 0);
    *l1 = src - (float)a;
}

// first source row (column) and number of rows of the outputs d0 .. d1 (inclusive), clamped to `cap` rows
SDN_HD void seg_footprint(float scale, int d0, int d1, int in, int cap, int* first, int* count)
{
    int a0, a1, b0, b1;
    float l;
    seg_taps(scale, d0, in, &a0, &a1, &l);
    seg_taps(scale, d1, in, &b0, &b1, &l);
    int n = b1 - a0 + 1;
    if (n > cap) n = cap;
    if (n < 1) n = 1;
    *first = a0;
    *count = n;
}

// 0 when the HOST table of sdn_segm_fuse is valid; otherwise 1 with the reason in msg
inline int seg_validate_fuse(const int32_t* table, int S, int B, int C, int H, int W, char* msg, size_t cap)
{
    if (S < 1 || S > SEG_MAX_SCALES) SDN_FAIL("%d scales; 1 to %d are supported", S, SEG_MAX_SCALES);
    if (C < 1 || C > SEG_MAX_CLASSES) SDN_FAIL("%d classes; 1 to %d are supported", C, SEG_MAX_CLASSES);
    if (B < 1 || B > 65535) SDN_FAIL("%d frames; 1 to 65535 are supported", B);
    if (H < 1 || W < 1 || H > SEG_MAX_SIDE || W > SEG_MAX_SIDE) SDN_FAIL("bad sizes: a %d x %d label map", H, W);
    for (int s = 0; s < S; s++) {
        SegScale r;
        std::memcpy(&r, table + 4 * (size_t)s, sizeof(r));
        if (!r.scores) SDN_FAIL("scale %d: null address", s);
        if (r.scores & 3) SDN_FAIL("scale %d: the map is not aligned to 4 bytes", s);
        if (r.h < 1 || r.w < 1 || r.h > SEG_MAX_SIDE || r.w > SEG_MAX_SIDE) SDN_FAIL("scale %d: bad sizes: a %d x %d map", s, r.h, r.w);
        if (r.h > 2 * H || r.w > 2 * W)
            SDN_FAIL("scale %d: a %d x %d map for a %d x %d output; a map may be at most twice the output", s, r.h, r.w, H, W);
    }
    return 0;
}

// 0 when the HOST colour table (codes [K] ascending, then labels [K]) of sdn_segm_labels_from_colors is valid
inline int seg_validate_colors(const int32_t* table, int K, char* msg, size_t cap)
{
    if (K < 1 || K > SEG_MAX_COLORS) SDN_FAIL("%d colour codes; 1 to %d are supported", K, SEG_MAX_COLORS);
    for (int k = 0; k < K; k++) {
        if (table[k] < 0 || table[k] > 0xffffff) SDN_FAIL("code %d is 0x%x; a code is r | g << 8 | b << 16", k, (unsigned)table[k]);
        if (k && table[k] <= table[k - 1]) SDN_FAIL("code %d: the codes are not sorted in strictly ascending order", k);
        // vkitti_dataset.py:209 stores the label in a uint8
        if (table[K + k] < 0 || table[K + k] > 255) SDN_FAIL("code %d: label %d outside 0 .. 255", k, table[K + k]);
    }
    return 0;
}

// index of `code` in the ascending codes [K], or -1
SDN_HD int seg_find(const int32_t* codes, int K, int code)
{
    int lo = 0, hi = K;   // the answer, if any, lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (codes[mid] <= code) lo = mid; else hi = mid;
    }
    return codes[lo] == code ? lo : -1;
}

}  // namespace sdn
