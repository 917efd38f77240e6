// The item row of sdn_train_crops_mixed (train_hybrid.hip) and the validation of its HOST tables.  Plain C++ so that a host
// program can walk valid and invalid tables without the HIP runtime (tools/train_hybrid_check.cpp).
#pragma once

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "check_common.h"

namespace sdn {

constexpr int MX_ITEM_INTS = 32;
constexpr int MX_OBJ_INTS = 12;
// the tile sizes of k_train_crops (train_items_common.h; train_hybrid.hip asserts that they agree)
constexpr int MX_SRC_PIXELS = 4096;
constexpr int MX_PLANE_BYTES = 12288;
constexpr int MX_MAX_CONTRAST_SIDE = 1448;

enum { MX_MASK_NONE = 0, MX_MASK_CODE = 1, MX_MASK_ID = 2 };
enum { MX_IGNORE_ZERO = 0, MX_IGNORE_NEARER = 1, MX_IGNORE_DISPARITY = 2 };

struct MixItem {   // one row of the item table, 32 ints
    uint64_t frame;            // address of the item's uint8 [3, H, W] frame
    uint64_t mask_src;         // MX_MASK_CODE: uint8 [H, W, 3]; MX_MASK_ID: int32 [H, W]
    uint64_t ignore_src;       // MX_IGNORE_NEARER: uint8 [H, W, 3]; MX_IGNORE_DISPARITY: int32 [H, W]
    int H, W;
    int mask_kind;
    int code;                  // MX_MASK_CODE: r | g << 8 | b << 16; MX_MASK_ID: the id
    int ignore_kind;
    int thr;                   // MX_IGNORE_DISPARITY: the byte is 255 where disparity > thr
    int near_off, near_cnt;    // MX_IGNORE_NEARER: rows near_off .. near_off + near_cnt of `nearer`
    int nops, order;           // the colour jitter, as sdn_train_crops' item row
    float fb, fc, fs;
    int hue;
    float mean[3], std[3];
    int pad[6];
};
static_assert(sizeof(MixItem) == MX_ITEM_INTS * sizeof(int32_t), "item table row");

struct MixSizes {
    int B, n_bounds, n_kk8, n_nearer, image_size, mask_size;
    bool maps;                 // masks and ignores are asked for
};

// 0 when the HOST tables are valid; otherwise 1 with the reason in msg.  *scon: the widest window of an item with contrast.
inline int mx_validate(const int32_t* rois, const int32_t* objs, const int32_t* items, const MixSizes& z, long* scon, char* msg,
                       size_t cap)
{
    *scon = 0;
    if (z.B < 1 || z.B > 65535 || z.n_bounds < 1 || z.n_kk8 < 1 || z.n_nearer < 0) SDN_FAIL("bad sizes");
    if (z.image_size < 1 || z.mask_size < 1 || z.image_size > MX_PLANE_BYTES || z.mask_size > MX_PLANE_BYTES)
        SDN_FAIL("bad crop sizes %d, %d", z.image_size, z.mask_size);
    for (int n = 0; n < z.B; n++) {
        const int32_t* r = rois + 4 * (size_t)n;
        const int32_t* w = objs + (size_t)MX_OBJ_INTS * n;
        MixItem it;
        std::memcpy(&it, items + (size_t)MX_ITEM_INTS * n, sizeof(it));
        if (r[2] <= r[0] || r[3] <= r[1]) SDN_FAIL("roi %d (%d, %d, %d, %d) is empty", n, r[0], r[1], r[2], r[3]);
        const long hh = (long)r[2] - r[0], ww = (long)r[3] - r[1];
        const long s = hh > ww ? hh : ww;
        if (s > MX_SRC_PIXELS)
            SDN_FAIL("roi %d: a %ld pixel window; one source row must fit the %d pixel staging tile", n, s, MX_SRC_PIXELS);
        if (w[2] != s || w[0] != r[0] - (s - hh) / 2 || w[1] != r[1] - (s - ww) / 2)
            SDN_FAIL("item %d: the window (%d, %d, %d) is not crop_square's of the roi", n, w[0], w[1], w[2]);
        if (it.H < 1 || it.W < 1 || (long)it.H * it.W > INT_MAX / 4) SDN_FAIL("item %d: a frame of %d x %d", n, it.H, it.W);
        if (!it.frame) SDN_FAIL("item %d: null frame address", n);
        if (it.mask_kind < MX_MASK_NONE || it.mask_kind > MX_MASK_ID) SDN_FAIL("item %d: mask source kind %d", n, it.mask_kind);
        if (it.ignore_kind < MX_IGNORE_ZERO || it.ignore_kind > MX_IGNORE_DISPARITY)
            SDN_FAIL("item %d: ignore source kind %d", n, it.ignore_kind);
        if (!z.maps && (it.mask_kind != MX_MASK_NONE || it.ignore_kind != MX_IGNORE_ZERO))
            SDN_FAIL("item %d: a mask or ignore source, but no masks / ignores output", n);
        if (it.mask_kind != MX_MASK_NONE && !it.mask_src) SDN_FAIL("item %d: null mask source address", n);
        if (it.ignore_kind != MX_IGNORE_ZERO && !it.ignore_src) SDN_FAIL("item %d: null ignore source address", n);
        if ((it.mask_kind == MX_MASK_ID && (it.mask_src & 3)) || (it.ignore_kind == MX_IGNORE_DISPARITY && (it.ignore_src & 3)))
            SDN_FAIL("item %d: an int32 map is not aligned to 4 bytes", n);
        if (it.ignore_kind == MX_IGNORE_NEARER && (it.near_off < 0 || it.near_cnt < 0 || (long)it.near_off + it.near_cnt > z.n_nearer))
            SDN_FAIL("item %d: nearer codes %d + %d outside the table of %d", n, it.near_off, it.near_cnt, z.n_nearer);
        if (it.nops < 0 || it.nops > 4 || it.hue < 0 || it.hue > 255) SDN_FAIL("item %d: %d ops, hue shift %d", n, it.nops, it.hue);
        int seen = 0;
        for (int k = 0; k < it.nops; k++) {
            const int op = (it.order >> (4 * k)) & 15;
            if (op > 3 || (seen >> op) & 1) SDN_FAIL("item %d: order 0x%x is not a permutation of distinct ops", n, it.order);
            seen |= 1 << op;
        }
        if ((seen >> 1) & 1) {   // contrast
            if (s > MX_MAX_CONTRAST_SIDE) SDN_FAIL("item %d: contrast on a %ld pixel window (at most %d)", n, s, MX_MAX_CONTRAST_SIDE);
            *scon = s > *scon ? s : *scon;
        }
        if (it.std[0] == 0.f || it.std[1] == 0.f || it.std[2] == 0.f) SDN_FAIL("item %d: std is 0", n);
        // Pillow's filter width for s -> S: 2 ceil(max(s / S, 1)) + 1 source rows per output row; they must fit the plane
        for (int which = 0; which < 2; which++) {
            const int S = which ? z.mask_size : z.image_size;
            const int32_t* t = w + 5 + 3 * which;
            if (s == S) {
                if (t[2] != 0) SDN_FAIL("item %d: a table for the resize %ld -> %d Pillow skips", n, s, S);
                continue;
            }
            const long taps = 2 * ((s > S ? (s + S - 1) / S : 1)) + 1;
            if (taps + 1 > MX_PLANE_BYTES / S)
                SDN_FAIL("roi %d: a %ld pixel window resized to %d needs %ld source rows per output row, the LDS tile holds %d", n, s, S,
                        taps + 1, MX_PLANE_BYTES / S);
            if (t[2] != taps || t[0] < 0 || t[1] < 0 || (long)t[0] + S > z.n_bounds || (long)t[1] + (long)S * taps > z.n_kk8)
                SDN_FAIL("item %d: resampling table (%d, %d, %d) of %ld -> %d does not fit", n, t[0], t[1], t[2], s, S);
        }
    }
    return 0;
}

}  // namespace sdn
