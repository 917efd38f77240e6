// Host walk over the validator of sdn_train_crops_mixed (3d-sdn_amd/csrc/train_hybrid_check.h): one valid table of several items
// and, for every reason the validator names, an edit of it that must be refused with that reason.  The tables are real arrays
// of exactly the sizes the entry point is told, so an address sanitizer sees any read beyond them.  Host code only; build and
// run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/train_hybrid_check.cpp \
//       -o /tmp/train_hybrid_check && /tmp/train_hybrid_check
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "train_hybrid_check.h"

using namespace sdn;

static int failures = 0;

struct Tables {
    std::vector<int32_t> rois, objs, items;
    MixSizes z;
};

static void put(Tables& t, int n, const MixItem& it) { std::memcpy(t.items.data() + (size_t)MX_ITEM_INTS * n, &it, sizeof(it)); }
static MixItem get(const Tables& t, int n)
{
    MixItem it;
    std::memcpy(&it, t.items.data() + (size_t)MX_ITEM_INTS * n, sizeof(it));
    return it;
}

// the window row crop_square gives a roi, with resampling tables placed one after another
static void window(Tables& t, int n, int y0, int x0, int y1, int x1, int& nb, int& nk)
{
    const int h = y1 - y0, w = x1 - x0, s = h > w ? h : w;
    int32_t* r = t.rois.data() + 4 * n;
    r[0] = y0; r[1] = x0; r[2] = y1; r[3] = x1;
    int32_t* o = t.objs.data() + (size_t)MX_OBJ_INTS * n;
    o[0] = y0 - (s - h) / 2; o[1] = x0 - (s - w) / 2; o[2] = s; o[3] = 4000; o[4] = 4000;
    for (int which = 0; which < 2; which++) {
        const int S = which ? t.z.mask_size : t.z.image_size;
        int32_t* q = o + 5 + 3 * which;
        if (s == S) continue;
        const int taps = 2 * (s > S ? (s + S - 1) / S : 1) + 1;
        q[0] = nb; q[1] = nk; q[2] = taps;
        nb += S; nk += S * taps;
    }
}

static Tables valid()
{
    Tables t;
    const int B = 5;
    t.z.B = B; t.z.image_size = 224; t.z.mask_size = 256; t.z.n_nearer = 3; t.z.maps = true;
    t.rois.assign(4 * B, 0); t.objs.assign((size_t)MX_OBJ_INTS * B, 0); t.items.assign((size_t)MX_ITEM_INTS * B, 0);
    int nb = 0, nk = 0;
    window(t, 0, 10, 20, 50, 70, nb, nk);       // an upscale
    window(t, 1, -3, -2, 221, 100, nb, nk);     // s == 224
    window(t, 2, 0, 0, 100, 256, nb, nk);       // s == 256
    window(t, 3, 0, 0, 1400, 900, nb, nk);      // a downscale with contrast
    window(t, 4, 5, 5, 4101, 9, nb, nk);        // the widest window
    t.z.n_bounds = nb; t.z.n_kk8 = nk;
    for (int n = 0; n < B; n++) {
        MixItem it;
        std::memset(&it, 0, sizeof(it));
        it.frame = 0x1000; it.H = 375; it.W = 1242;
        it.mask_kind = n % 3; it.mask_src = it.mask_kind ? 0x2000 : 0;
        it.ignore_kind = (n + 1) % 3; it.ignore_src = it.ignore_kind ? 0x3000 : 0;
        it.near_off = 1; it.near_cnt = 2;
        it.nops = n == 3 ? 4 : 0; it.order = 0 | 1 << 4 | 2 << 8 | 3 << 12; it.hue = 255;
        for (int c = 0; c < 3; c++) { it.mean[c] = 0.5f; it.std[c] = 0.25f; }
        put(t, n, it);
    }
    return t;
}

static void expect(const char* what, const std::function<void(Tables&)>& edit, const char* reason)
{
    Tables t = valid();
    edit(t);
    long scon = -1;
    char msg[256] = "";
    const int rc = mx_validate(t.rois.data(), t.objs.data(), t.items.data(), t.z, &scon, msg, sizeof(msg));
    const bool ok = reason ? (rc == 1 && std::strstr(msg, reason)) : (rc == 0);
    std::printf("%-44s %s  %s\n", what, ok ? "ok  " : "FAIL", msg);
    if (!ok) failures++;
}

static std::function<void(Tables&)> item(int n, const std::function<void(MixItem&)>& f)
{
    return [=](Tables& t) { MixItem it = get(t, n); f(it); put(t, n, it); };
}

int main()
{
    {
        Tables t = valid();
        long scon = 0;
        char msg[256] = "";
        if (mx_validate(t.rois.data(), t.objs.data(), t.items.data(), t.z, &scon, msg, sizeof(msg)) || scon != 1400) {
            std::printf("the valid table: %s (contrast window %ld)\n", msg, scon);
            failures++;
        }
    }
    expect("valid", [](Tables&) {}, nullptr);
    expect("no maps, no sources", [](Tables& t) {
        t.z.maps = false;
        for (int n = 0; n < t.z.B; n++) { MixItem it = get(t, n); it.mask_kind = it.ignore_kind = 0; put(t, n, it); }
    }, nullptr);
    expect("no maps, a source", [](Tables& t) { t.z.maps = false; }, "no masks / ignores output");
    expect("B 0", [](Tables& t) { t.z.B = 0; }, "bad sizes");
    expect("crop size 0", [](Tables& t) { t.z.image_size = 0; }, "bad crop sizes");
    expect("empty roi", [](Tables& t) { t.rois[4 * 2 + 2] = t.rois[4 * 2]; }, "is empty");
    expect("window too wide", [](Tables& t) { t.rois[4 * 4 + 2] += 1; }, "staging tile");
    expect("window not of the roi", [](Tables& t) { t.objs[MX_OBJ_INTS * 1 + 1] += 1; }, "not crop_square");
    expect("frame height 0", item(0, [](MixItem& it) { it.H = 0; }), "a frame of");
    expect("frame too large", item(0, [](MixItem& it) { it.H = 40000; it.W = 40000; }), "a frame of");
    expect("null frame", item(4, [](MixItem& it) { it.frame = 0; }), "null frame");
    expect("mask kind 3", item(0, [](MixItem& it) { it.mask_kind = 3; }), "mask source kind");
    expect("mask kind -1", item(0, [](MixItem& it) { it.mask_kind = -1; }), "mask source kind");
    expect("ignore kind 3", item(0, [](MixItem& it) { it.ignore_kind = 3; }), "ignore source kind");
    expect("null mask source", item(1, [](MixItem& it) { it.mask_src = 0; }), "null mask source");
    expect("null ignore source", item(0, [](MixItem& it) { it.ignore_src = 0; }), "null ignore source");
    expect("unaligned id map", item(2, [](MixItem& it) { it.mask_src = 0x2002; }), "not aligned");
    expect("unaligned disparity map", item(1, [](MixItem& it) { it.ignore_src = 0x3001; }), "not aligned");
    expect("nearer rows past the table", item(0, [](MixItem& it) { it.near_cnt = 3; }), "nearer codes");
    expect("nearer rows negative", item(0, [](MixItem& it) { it.near_off = -1; }), "nearer codes");
    expect("five ops", item(0, [](MixItem& it) { it.nops = 5; }), "ops, hue shift");
    expect("hue shift 256", item(0, [](MixItem& it) { it.hue = 256; }), "ops, hue shift");
    expect("an op twice", item(3, [](MixItem& it) { it.order = 0 | 0 << 4 | 2 << 8 | 3 << 12; }), "permutation");
    expect("an unknown op", item(3, [](MixItem& it) { it.order = 7; }), "permutation");
    expect("contrast on a wide window", item(4, [](MixItem& it) { it.nops = 1; it.order = 1; }), "contrast on a");
    expect("std 0", item(2, [](MixItem& it) { it.std[1] = 0.f; }), "std is 0");
    expect("a table where Pillow skips", [](Tables& t) { t.objs[MX_OBJ_INTS * 1 + 7] = 3; }, "Pillow skips");
    expect("filter wider than the tile", [](Tables& t) { t.z.image_size = 3500; }, "source rows per output row");
    expect("table past bounds", [](Tables& t) { t.z.n_bounds -= 1; }, "does not fit");
    expect("table past kk8", [](Tables& t) { t.z.n_kk8 -= 1; }, "does not fit");
    expect("wrong tap count", [](Tables& t) { t.objs[MX_OBJ_INTS * 0 + 7] += 2; }, "does not fit");
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("train_hybrid_check: ok\n");
    return 0;
}
