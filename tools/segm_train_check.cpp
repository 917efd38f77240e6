// Host walk over the index arithmetic, the LDS plan and the validator of the semantic training batch
// (3d-sdn_amd/csrc/segm_train_check.h):
//   - Pillow's bilinear bounds (precompute_coeffs, box = the whole image) rebuilt here for the reference's sizes (frames
//     375 x 1242, short sizes 100 .. 375, the upscale to 1274) and for 45 x 150 at every height 1 .. 64: every band of
//     SGT_BAND output rows fits its plane, its span holds the taps of each of its rows, and a whole table buffer built from
//     them passes sgt_validate;
//   - for every reason the validator names, an edit of a valid buffer that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/segm_train_check.cpp \
//       -o /tmp/segm_train_check && /tmp/segm_train_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "segm_train_check.h"

using namespace sdn;

static int failures = 0;

struct Batch {
    std::vector<int32_t> T;
    int B, H, W, Hb, Wb, rate;
};

static int append(std::vector<int32_t>& T, const std::vector<int32_t>& a)
{
    const int at = (int)T.size();
    T.insert(T.end(), a.begin(), a.end());
    return at;
}

// Resample.c: precompute_coeffs for the bilinear filter; bounds only, coefficients 0 (the validator does not read them)
static void bilinear(std::vector<int32_t>& T, int in, int out, int* boff, int* koff, int* ksize)
{
    if (in == out) {
        *boff = *koff = *ksize = 0;
        return;
    }
    const double scale = (double)in / out, fscale = scale < 1.0 ? 1.0 : scale, support = fscale;
    const int k = (int)std::ceil(support) * 2 + 1;
    std::vector<int32_t> b(2 * (size_t)out);
    for (int x = 0; x < out; x++) {
        const double center = (x + 0.5) * scale;
        int xmin = (int)(center - support + 0.5), xmax = (int)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > in) xmax = in;
        b[2 * x] = xmin;
        b[2 * x + 1] = xmax - xmin;
    }
    *boff = append(T, b);
    *koff = append(T, std::vector<int32_t>((size_t)out * k, 0));
    *ksize = k;
}

static int nearest(std::vector<int32_t>& T, int in, int out)
{
    std::vector<int32_t> t(out);
    const double a = (double)in / out;
    double xo = a * 0.5;
    for (int x = 0; x < out; x++) {
        t[x] = (int)xo < in - 1 ? (int)xo : in - 1;
        xo += a;
    }
    return append(T, t);
}

static Batch make(int H, int W, int h, int w, int B, int order = 0x2013, int nops = 4)
{
    Batch t;
    t.B = B; t.H = H; t.W = W; t.rate = 8;
    t.Hb = (h + 7) / 8 * 8; t.Wb = (w + 7) / 8 * 8;
    t.T.assign((size_t)B * SGT_ITEM_INTS, 0);
    for (int i = 0; i < B; i++) {
        SegTrainItem it;
        std::memset(&it, 0, sizeof(it));
        it.h = h; it.w = w; it.flip = i & 1; it.nops = nops; it.order = order; it.fb = it.fc = it.fs = 1.1f; it.hue = 40;
        bilinear(t.T, W, w, &it.xb, &it.xk, &it.xksize);
        bilinear(t.T, H, h, &it.yb, &it.yk, &it.yksize);
        it.xn = nearest(t.T, W, w);
        it.yn = nearest(t.T, H, h);
        it.K = 3;
        it.ct = append(t.T, {5, 70000, 0xffffff, 1, 0, 255});
        std::memcpy(t.T.data() + (size_t)i * SGT_ITEM_INTS, &it, sizeof(it));
    }
    return t;
}

static int validate(const Batch& t, char* msg, size_t cap)
{
    return sgt_validate(t.T.data(), (long)t.T.size(), t.B, t.H, t.W, t.Hb, t.Wb, t.rate, msg, cap);
}

// the plan of one size pair: the validator accepts it, and every band's span holds its rows' taps within the plane
static void walk(int H, int W, int h, int w, bool print)
{
    Batch t = (long)H * W > SGT_MAX_CONTRAST_PIXELS ? make(H, W, h, w, 1, 0x203, 3) : make(H, W, h, w, 1);
    char msg[256] = "";
    bool ok = validate(t, msg, sizeof(msg)) == 0;
    SegTrainItem it;
    std::memcpy(&it, t.T.data(), sizeof(it));
    int most = 0;
    for (int r0 = 0; r0 < h && ok; r0 += SGT_BAND) {
        const int r1 = r0 + SGT_BAND < h ? r0 + SGT_BAND : h;
        int first, count;
        sgt_band_span(it.yksize ? t.T.data() + it.yb : nullptr, r0, r1, &first, &count);
        ok = first >= 0 && count >= 1 && first + count <= H && (long)count * w <= SGT_PLANE_BYTES;
        for (int y = r0; y < r1 && ok && it.yksize; y++) {
            const int a = t.T[it.yb + 2 * y], c = t.T[it.yb + 2 * y + 1];
            ok = a >= first && a + c <= first + count;
        }
        most = count > most ? count : most;
    }
    if (print || !ok)
        std::printf("%4d x %4d -> %4d x %4d: %2d / %2d taps, at most %2d of %2d rows a plane holds  %s %s\n", H, W, h, w, it.xksize, it.yksize,
                    most, SGT_PLANE_BYTES / w, ok ? "ok" : "FAIL", msg);
    if (!ok) failures++;
}

static void expect(const char* what, const std::function<void(Batch&, SegTrainItem&)>& edit, const char* reason)
{
    Batch t = make(45, 150, 20, 66, 2);
    SegTrainItem it;
    std::memcpy(&it, t.T.data() + SGT_ITEM_INTS, sizeof(it));
    edit(t, it);
    std::memcpy(t.T.data() + SGT_ITEM_INTS, &it, sizeof(it));
    char msg[256] = "";
    const int rc = validate(t, msg, sizeof(msg));
    const bool ok = reason ? (rc == 1 && std::strstr(msg, reason)) : (rc == 0);
    std::printf("%-36s %s  %s\n", what, ok ? "ok  " : "FAIL", msg);
    if (!ok) failures++;
}

int main()
{
    // the reference's defaults: vkitti_dataset.py:91-97 with imgSize 100 .. 375 and imgMaxSize 1274
    const int shorts[] = {100, 150, 200, 300, 375, 385, 400};
    for (int s : shorts) {
        const double a = s / 375.0, b = 1274 / 1242.0, scale = a < b ? a : b;
        walk(375, 1242, (int)(375 * scale), (int)(1242 * scale), true);
    }
    for (int h = 1; h <= 64; h++) walk(45, 150, h, (h * 150) / 45 > 0 ? (h * 150) / 45 : 1, false);
    for (int w = 1; w <= 400; w += 7) walk(45, 150, 45, w, false);   // one pass skipped
    walk(4096, 4096, 4096, 3072, true);                              // the widest row that holds a band
    std::printf("plans: %s\n", failures ? "FAIL" : "ok");

    expect("valid", [](Batch&, SegTrainItem&) {}, nullptr);
    expect("B 0", [](Batch& t, SegTrainItem&) { t.B = 0; }, "items");
    expect("frame wider than the staging tile", [](Batch& t, SegTrainItem&) { t.W = SGT_SRC_PIXELS + 1; }, "staging tile");
    expect("batch height 0", [](Batch& t, SegTrainItem&) { t.Hb = 0; }, "bad sizes");
    expect("rate 0", [](Batch& t, SegTrainItem&) { t.rate = 0; }, "label rate");
    expect("buffer shorter than the rows", [](Batch& t, SegTrainItem&) { t.T.resize(SGT_ITEM_INTS); t.B = 2; }, "cannot hold");
    expect("item higher than the batch", [](Batch&, SegTrainItem& it) { it.h = 25; }, "resized to");
    expect("labels beyond the map", [](Batch& t, SegTrainItem&) { t.rate = 7; t.Hb = 20; }, "do not fit");
    expect("flip 2", [](Batch&, SegTrainItem& it) { it.flip = 2; }, "flip");
    expect("five ops", [](Batch&, SegTrainItem& it) { it.nops = 5; }, "ops");
    expect("hue 256", [](Batch&, SegTrainItem& it) { it.hue = 256; }, "hue shift");
    expect("an op twice", [](Batch&, SegTrainItem& it) { it.order = 0x2113; }, "permutation");
    expect("op 4", [](Batch&, SegTrainItem& it) { it.order = 0x2014; }, "permutation");
    expect("contrast on a large frame", [](Batch& t, SegTrainItem&) { t = make(1024, 2049, 1024, 2049, 2); }, "contrast on a frame");
    expect("no contrast on a large frame", [](Batch& t, SegTrainItem& it) {
        t = make(1024, 2049, 1024, 2049, 2, 0x203, 3);
        std::memcpy(&it, t.T.data() + SGT_ITEM_INTS, sizeof(it));
    }, nullptr);
    expect("wrong tap count", [](Batch&, SegTrainItem& it) { it.xksize = 5; }, "taps");
    expect("a table for a skipped pass", [](Batch& t, SegTrainItem& it) {
        t = make(45, 150, 45, 150, 2);
        std::memcpy(&it, t.T.data() + SGT_ITEM_INTS, sizeof(it));
        it.yksize = 3;
    }, "Pillow skips");
    expect("bounds before the tables", [](Batch&, SegTrainItem& it) { it.yb = 3; }, "outside the buffer");
    expect("coefficients past the end", [](Batch& t, SegTrainItem& it) { it.xk = (int)t.T.size() - 10; }, "outside the buffer");
    expect("a bound past the frame", [](Batch& t, SegTrainItem& it) { t.T[it.xb + 2 * 65] = 149; }, "bounds of output 65");
    expect("a bound with no tap", [](Batch& t, SegTrainItem& it) { t.T[it.yb + 1] = 0; }, "bounds of output 0");
    expect("NEAREST table past the end", [](Batch& t, SegTrainItem& it) { it.yn = (int)t.T.size() - 5; }, "NEAREST tables");
    expect("NEAREST column outside", [](Batch& t, SegTrainItem& it) { t.T[it.xn + 7] = 150; }, "reads column 150");
    expect("NEAREST row negative", [](Batch& t, SegTrainItem& it) { t.T[it.yn] = -1; }, "reads row -1");
    expect("K 1025", [](Batch&, SegTrainItem& it) { it.K = SEG_MAX_COLORS + 1; }, "colour codes");
    expect("colour table past the end", [](Batch& t, SegTrainItem& it) { it.ct = (int)t.T.size() - 4; }, "colour table");
    expect("unsorted colours", [](Batch& t, SegTrainItem& it) { t.T[it.ct] = 80000; }, "not sorted");
    expect("a plane too small", [](Batch& t, SegTrainItem& it) {
        t = make(4000, 3000, 400, 3000, 2, 0x203, 3);
        std::memcpy(&it, t.T.data() + SGT_ITEM_INTS, sizeof(it));
    }, "does not fit the LDS plan");
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("segm_train_check: ok\n");
    return 0;
}
