// Host walk over the key images, the caps, the workspace layout and the validators of the RPN targets
// (3d-sdn_amd/csrc/rpn_targets_check.h):
//   - the IoU image: a double comes back from its image; the images order as the doubles do; -0.0 and +0.0 share one image; every NaN
//     has the one largest image; no image is 0; the arg-max rule takes the first maximum and the first NaN;
//   - the sampling key: image and anchor come back; keys order by the float's image, then by the anchor; the digits of the four radix
//     passes put the image together again, and a radix select over 256-bin histograms finds the exact cut of a small sample;
//   - the caps: T / 2 positives, T - n_pos negatives, never more than T in all, both at least 1 for every T the validator lets in;
//   - the layout: the ranges lie inside `total`, start on 16 bytes and do not overlap;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/rpn_targets_check.cpp
//       -o /tmp/rpn_targets_check && /tmp/rpn_targets_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rpn_targets_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static uint32_t bits_of(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}

static void walk_images()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double values[] = {-inf, -2.5, -1e-310, 0.0, 5e-324, 0.3, 0.7, 896.0 / 1280.0 + 1e-16, 1.0, inf};   // ascending
    const size_t n = sizeof(values) / sizeof(values[0]);
    bool ok = true;
    for (size_t i = 0; i < n; i++) {
        const uint64_t image = rt_image(values[i]);
        ok = ok && image != 0ull && image != RT_IMAGE_NAN && rt_image_value(image) == values[i];
        if (i + 1 < n) ok = ok && image < rt_image(values[i + 1]);
    }
    expect(ok, "a double comes back from its image, the images ascend with the doubles and none is 0");
    expect(rt_image(-0.0) == rt_image(0.0) && rt_image(0.0) == RT_IMAGE_ZERO, "-0.0 and +0.0 share the image of zero");
    expect(rt_image(nan) == RT_IMAGE_NAN && rt_image(-nan) == RT_IMAGE_NAN && rt_image(inf) < RT_IMAGE_NAN, "every NaN has the largest image");
    expect(896.0 / 1280.0 == 0.7 && 660.0 / 2200.0 == 0.3, "the threshold cases' quotients are the doubles 0.7 and 0.3");
    // np.argmax over a row
    const double row[] = {0.2, 0.5, 0.5, nan, 0.9, nan};
    bool have = false;
    double best = 0.0;
    int at = -1;
    for (int g = 0; g < 6; g++)
        if (rt_argmax_takes(have, best, row[g])) {
            best = row[g];
            at = g;
            have = true;
        }
    expect(at == 3, "the first NaN is the arg-max");
    have = false;
    at = -1;
    for (int g = 0; g < 3; g++)
        if (rt_argmax_takes(have, best, row[g])) {
            best = row[g];
            at = g;
            have = true;
        }
    expect(at == 1, "the first maximum is the arg-max");
}

static void walk_sample_keys()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float keys[] = {-inf, -1.0f, -1e-45f, -0.0f, 0.0f, 1e-45f, 0.25f, 0.25f, 0.99999994f, 1.0f, inf};   // ascending, one tie
    const uint32_t anchors[] = {0u, 1u, 65535u, 65536u, 261887u, (uint32_t)RT_MAX_ANCHORS - 1u};
    bool ok = true;
    std::vector<uint64_t> all;
    for (size_t k = 0; k < sizeof(keys) / sizeof(keys[0]); k++)
        for (uint32_t a : anchors) {
            const uint64_t key = rt_sample_key(bits_of(keys[k]), a);
            const uint32_t image = dt_image(bits_of(keys[k]));
            ok = ok && rt_sample_key_image(key) == image && rt_sample_key_anchor(key) == a;
            uint32_t again = 0u;
            for (int p = 0; p < RT_PASSES; p++) {
                ok = ok && rt_prefix(image, p) == again;
                again = (again << 8) | rt_digit(image, p);
            }
            ok = ok && again == image;
            all.push_back(key);
        }
    expect(ok, "image and anchor come back from a sampling key and the four digits are the image");
    ok = true;
    for (size_t i = 0; i < all.size(); i++)
        for (size_t j = 0; j < all.size(); j++) {
            const size_t ki = i / 6, kj = j / 6;
            if (keys[ki] < keys[kj] || (bits_of(keys[ki]) == bits_of(keys[kj]) && i % 6 < j % 6)) ok = ok && all[i] < all[j];
        }
    expect(ok, "smaller key first, equal keys lower anchor first");

    // an exact radix select the way the kernels run it: 4 passes of 256 bins, then the rank among the anchors AT the cut
    std::vector<uint32_t> images;
    uint32_t state = 12345u;
    for (int i = 0; i < 5000; i++) {
        state = state * 1664525u + 1013904223u;
        images.push_back(dt_image(bits_of((float)((state >> 8) % 97) / 97.0f)));   // 97 distinct keys: the cut is shared
    }
    ok = true;
    for (int cap : {1, 2, 128, 256, 4999}) {
        long rank = cap - 1;
        uint32_t cut = 0u;
        for (int p = 0; p < RT_PASSES; p++) {
            long hist[RT_BINS] = {0};
            for (uint32_t image : images)
                if (rt_prefix(image, p) == cut) hist[rt_digit(image, p)]++;
            int bin = 0;
            while (rank >= hist[bin]) rank -= hist[bin++];
            cut = (cut << 8) | (uint32_t)bin;
        }
        const long stay = rank + 1;
        std::vector<uint32_t> sorted = images;
        std::sort(sorted.begin(), sorted.end());
        long below = 0, at_cut = 0;
        for (uint32_t image : images) {
            below += image < cut;
            at_cut += image == cut;
        }
        ok = ok && sorted[cap - 1] == cut && below + stay == cap && stay <= at_cut;
    }
    expect(ok, "four 256-bin passes find the cut key and how many anchors at it stay");
}

static void walk_caps()
{
    bool ok = true;
    for (int T = 2; T <= RT_MAX_TARGETS; T++)
        for (int n_pos : {0, 1, T / 2 - 1, T / 2, T / 2 + 1, T, 1 << 20}) {
            if (n_pos < 0) continue;
            const int kept = rt_positives_kept(T, n_pos);
            ok = ok && kept <= T / 2 && kept <= n_pos && rt_positive_cap(T) >= 1 && rt_negative_cap(T, kept) >= 1;
            for (int n_neg : {0, 1, T - kept, T - kept + 1, 1 << 24}) {
                const int neg = rt_negatives_kept(T, kept, n_neg);
                ok = ok && neg <= n_neg && kept + neg <= T && (n_neg < T - kept || kept + neg == T);
            }
        }
    expect(ok, "the caps: T / 2 positives, then T - n_pos negatives, never more than T");
    expect(rt_positives_kept(256, 200) == 128 && rt_negatives_kept(256, 20, 3342) == 236 && rt_negatives_kept(257, 128, 1000) == 129, "the caps of T = 256 and 257");
    expect(rt_chunks(1) == 1 && rt_chunks(RT_CHUNK) == 1 && rt_chunks(RT_CHUNK + 1) == 2 && rt_chunks(261888) == 256 && rt_chunks(RT_MAX_ANCHORS) == 16384, "the chunks");
}

static void walk_layout()
{
    char msg[256];
    bool ok = true;
    const int sizes[][3] = {{1, 1, 2}, {4092, 8, 256}, {16368, 128, 256}, {261888, 100, 256}, {RT_MAX_ANCHORS, RT_MAX_BOXES, RT_MAX_TARGETS}};
    for (auto& s : sizes) {
        RtLayout L;
        ok = ok && rt_layout(s[0], s[1], s[2], &L, msg, sizeof(msg)) == 0;
        const size_t chunks = (size_t)rt_chunks(s[0]);
        const size_t at[] = {L.hist, L.best, L.counts, L.tab_image, L.tab_anchor, L.argmax, L.total};
        const size_t need[] = {4 * (size_t)RT_HIST_INTS, 4 * (size_t)s[1], 12 * chunks, 8 * chunks * s[1], 4 * chunks * s[1], (size_t)s[0]};
        for (int k = 0; k < 6; k++) ok = ok && at[k] % 16 == 0 && at[k] + need[k] <= at[k + 1];
        ok = ok && L.hist == 0 && L.total % 16 == 0;
    }
    expect(ok, "the workspace's ranges start on 16 bytes, hold what they must and do not overlap");
    RtLayout L;
    rt_layout(261888, 100, 256, &L, msg, sizeof(msg));
    std::printf("workspace 261888 100 256 %zu\n", L.total);
    expect(rt_layout(10, 3, 256, nullptr, msg, sizeof(msg)) == 1 && std::strstr(msg, "layout is NULL"), "a NULL layout is refused");
}

struct Call {
    const void *anchors, *ids, *boxes, *keys, *gt_count, *match, *bbox, *rows, *counts, *ws;
    int A, G, ids64, T;
    const double* std_dev;
    size_t ws_bytes;
};

static int run(const Call& c, char* msg, size_t cap)
{
    return rt_validate(c.anchors, c.ids, c.boxes, c.keys, c.A, c.G, c.ids64, c.gt_count, c.T, c.std_dev, c.match, c.bbox, c.rows,
                       c.counts, c.ws, c.ws_bytes, msg, cap);
}

static void refused(Call c, const char* reason, const char* what)
{
    char msg[256] = "";
    const bool ok = run(c, msg, sizeof(msg)) == 1 && std::strstr(msg, reason) != nullptr;
    if (!ok) std::printf("  got: %s\n", msg);
    expect(ok, what);
}

static void walk_validators()
{
    static const double std_dev[4] = {0.1, 0.1, 0.2, 0.2};
    static const double bad_std[4] = {0.1, 0.0, 0.2, 0.2};
    const void* p = reinterpret_cast<const void*>(0x10000);   // never dereferenced
    const auto off = [](const void* q, int n) { return reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(q) + n); };
    const Call good = {p, p, p, p, nullptr, p, p, p, p, p, 261888, 100, 0, 256, std_dev, (size_t)1 << 24};
    char msg[256] = "";
    expect(run(good, msg, sizeof(msg)) == 0, "a valid call passes");
    Call c = good;
    c.gt_count = p, c.ids64 = 1, c.A = RT_MAX_ANCHORS, c.G = RT_MAX_BOXES, c.T = RT_MAX_TARGETS, c.ws_bytes = (size_t)1 << 30;
    expect(run(c, msg, sizeof(msg)) == 0, "the largest sizes pass");
    c = good, c.A = 0, refused(c, "A 0; 1 to 16777215", "A = 0");
    c = good, c.A = 1 << 24, refused(c, "A 16777216; 1 to 16777215", "A = 2^24");
    c = good, c.G = 0, refused(c, "G 0; 1 to 128", "G = 0");
    c = good, c.G = 129, refused(c, "G 129; 1 to 128", "G = 129");
    c = good, c.T = 1, refused(c, "T 1; 2 to 8192", "T = 1");
    c = good, c.T = 8193, refused(c, "T 8193; 2 to 8192", "T = 8193");
    c = good, c.std_dev = nullptr, refused(c, "std_dev is NULL", "std_dev NULL");
    c = good, c.std_dev = bad_std, refused(c, "std_dev[1] is 0", "std_dev 0");
    c = good, c.anchors = nullptr, refused(c, "anchors, gt_class_ids, gt_boxes or keys is NULL", "anchors NULL");
    c = good, c.ids = nullptr, refused(c, "anchors, gt_class_ids, gt_boxes or keys is NULL", "ids NULL");
    c = good, c.boxes = nullptr, refused(c, "anchors, gt_class_ids, gt_boxes or keys is NULL", "boxes NULL");
    c = good, c.keys = nullptr, refused(c, "anchors, gt_class_ids, gt_boxes or keys is NULL", "keys NULL");
    c = good, c.match = nullptr, refused(c, "rpn_match, rpn_bbox, rows or counts is NULL", "rpn_match NULL");
    c = good, c.bbox = nullptr, refused(c, "rpn_match, rpn_bbox, rows or counts is NULL", "rpn_bbox NULL");
    c = good, c.rows = nullptr, refused(c, "rpn_match, rpn_bbox, rows or counts is NULL", "rows NULL");
    c = good, c.counts = nullptr, refused(c, "rpn_match, rpn_bbox, rows or counts is NULL", "counts NULL");
    c = good, c.ws = nullptr, refused(c, "workspace is NULL", "workspace NULL");
    c = good, c.ws_bytes = 100, refused(c, "workspace 100 <", "workspace too small");
    c = good, c.anchors = off(p, 8), refused(c, "anchors must be aligned to 16 bytes", "anchors misaligned");
    c = good, c.boxes = off(p, 2), refused(c, "gt_boxes and keys must be aligned to 4 bytes", "boxes misaligned");
    c = good, c.keys = off(p, 1), refused(c, "gt_boxes and keys must be aligned to 4 bytes", "keys misaligned");
    c = good, c.ids = off(p, 2), refused(c, "gt_class_ids must be aligned to 4 bytes", "ids misaligned");
    c = good, c.ids = off(p, 4), c.ids64 = 1, refused(c, "gt_class_ids must be aligned to 8 bytes", "int64 ids misaligned");
    c = good, c.gt_count = off(p, 2), refused(c, "gt_count must be aligned to 4 bytes", "gt_count misaligned");
    c = good, c.match = off(p, 2), refused(c, "rpn_match, rows and counts must be aligned to 4 bytes", "rpn_match misaligned");
    c = good, c.rows = off(p, 1), refused(c, "rpn_match, rows and counts must be aligned to 4 bytes", "rows misaligned");
    c = good, c.counts = off(p, 3), refused(c, "rpn_match, rows and counts must be aligned to 4 bytes", "counts misaligned");
    c = good, c.bbox = off(p, 4), refused(c, "rpn_bbox and workspace must be aligned to 16 bytes", "rpn_bbox misaligned");
    c = good, c.ws = off(p, 8), refused(c, "rpn_bbox and workspace must be aligned to 16 bytes", "workspace misaligned");
    std::printf("the validators: walked\n");
}

int main()
{
    walk_images();
    walk_sample_keys();
    walk_caps();
    walk_layout();
    walk_validators();
    std::printf("rpn_targets_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
