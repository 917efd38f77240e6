// Host walk over the index arithmetic and the validators of the semantic tail (3d-sdn_amd/csrc/segm_tail_check.h):
//   - for output sizes 1 .. 200 and every map size up to twice the output, plus the sizes of the VKITTI frame and the limits: the
//     footprint of every tile fits SEG_FOOT_ROWS / SEG_FOOT_COLS without its cap, lies inside the map and holds both taps of
//     every pixel of the tile; the taps are those of the float64 formula wherever that is not within a few fp32 ulp of an integer;
//   - the table validators: one valid table and, for every reason they name, an edit that must be refused with that reason;
//   - seg_find on real arrays of exactly K elements.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/segm_tail_check.cpp \
//       -o /tmp/segm_tail_check && /tmp/segm_tail_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "segm_tail_check.h"

using namespace sdn;

static int failures = 0;

static void walk_axis(int in, int out, int tile, int cap)
{
    const float scale = seg_scale(in, out);
    for (int d0 = 0; d0 < out; d0 += tile) {
        const int d1 = (d0 + tile - 1 < out ? d0 + tile - 1 : out - 1);
        int first, count, uncapped;
        seg_footprint(scale, d0, d1, in, cap, &first, &count);
        seg_footprint(scale, d0, d1, in, INT_MAX, &first, &uncapped);
        bool ok = count == uncapped && first >= 0 && first + count <= in;
        for (int d = d0; d <= d1 && ok; d++) {
            int i0, i1;
            float l1;
            seg_taps(scale, d, in, &i0, &i1, &l1);
            ok = i0 >= first && i1 <= first + count - 1 && i1 >= i0 && i1 <= i0 + 1 && l1 >= 0.f && l1 < 1.f;
            double src = ((double)d + 0.5) * ((double)in / out) - 0.5;
            if (src < 0) src = 0;
            // fp32 places the position within a few ulp of the float64 value: compare the taps away from the integers
            if (ok && std::fabs(src - std::round(src)) > 1e-4 + 4.0 * src * 1.2e-7) ok = i0 == (int)src;
        }
        if (!ok) {
            if (failures < 20) std::printf("axis %d -> %d, tile at %d: rows %d .. +%d (uncapped %d)  FAIL\n", in, out, d0, first, count, uncapped);
            failures++;
        }
    }
}

struct Fuse {
    std::vector<int32_t> table;
    int S, B, C, H, W;
};

static void put(Fuse& t, int s, uint64_t addr, int h, int w)
{
    SegScale r;
    r.scores = addr; r.h = h; r.w = w;
    std::memcpy(t.table.data() + 4 * (size_t)s, &r, sizeof(r));
}

static Fuse valid_fuse()
{
    Fuse t;
    t.S = 5; t.B = 1; t.C = 14; t.H = 375; t.W = 1242;
    t.table.assign(4 * (size_t)t.S, 0);
    const int hs[5] = {13, 19, 25, 38, 47}, ws[5] = {42, 63, 83, 125, 156};
    for (int s = 0; s < 5; s++) put(t, s, 0x1000 * (s + 1), hs[s], ws[s]);
    return t;
}

static void expect_fuse(const char* what, const std::function<void(Fuse&)>& edit, const char* reason)
{
    Fuse t = valid_fuse();
    edit(t);
    char msg[256] = "";
    const int rc = seg_validate_fuse(t.table.data(), t.S, t.B, t.C, t.H, t.W, msg, sizeof(msg));
    const bool ok = reason ? (rc == 1 && std::strstr(msg, reason)) : (rc == 0);
    std::printf("%-36s %s  %s\n", what, ok ? "ok  " : "FAIL", msg);
    if (!ok) failures++;
}

static void expect_colors(const char* what, std::vector<int32_t> table, int K, const char* reason)
{
    char msg[256] = "";
    const int rc = seg_validate_colors(table.data(), K, msg, sizeof(msg));
    const bool ok = reason ? (rc == 1 && std::strstr(msg, reason)) : (rc == 0);
    std::printf("%-36s %s  %s\n", what, ok ? "ok  " : "FAIL", msg);
    if (!ok) failures++;
}

int main()
{
    for (int out = 1; out <= 200; out++)
        for (int in = 1; in <= 2 * out; in++) {
            walk_axis(in, out, SEG_TILE_H, SEG_FOOT_ROWS);
            walk_axis(in, out, SEG_TILE_W, SEG_FOOT_COLS);
        }
    const int outs[] = {375, 1242, 1000, 4097, SEG_MAX_SIDE};
    for (int out : outs) {
        const int ins[] = {1, 2, 13, 47, 156, out / 8, out / 3, out - 1, out, out + 1, (3 * out) / 2, 2 * out - 1, 2 * out};
        for (int in : ins) {
            if (in < 1 || in > SEG_MAX_SIDE) continue;
            walk_axis(in, out, SEG_TILE_H, SEG_FOOT_ROWS);
            walk_axis(in, out, SEG_TILE_W, SEG_FOOT_COLS);
        }
    }
    std::printf("footprints: %s\n", failures ? "FAIL" : "ok");

    expect_fuse("valid", [](Fuse&) {}, nullptr);
    expect_fuse("8 scales, 32 classes", [](Fuse& t) {
        t.S = 8; t.C = 32; t.table.assign(32, 0);
        for (int s = 0; s < 8; s++) put(t, s, 0x1000, 750, 2484);
    }, nullptr);
    expect_fuse("S 0", [](Fuse& t) { t.S = 0; }, "scales");
    expect_fuse("S 9", [](Fuse& t) { t.S = 9; t.table.resize(36, 0); }, "scales");
    expect_fuse("C 0", [](Fuse& t) { t.C = 0; }, "classes");
    expect_fuse("C 33", [](Fuse& t) { t.C = 33; }, "classes");
    expect_fuse("B 0", [](Fuse& t) { t.B = 0; }, "frames");
    expect_fuse("H 0", [](Fuse& t) { t.H = 0; }, "bad sizes");
    expect_fuse("W too large", [](Fuse& t) { t.W = SEG_MAX_SIDE + 1; }, "bad sizes");
    expect_fuse("null map", [](Fuse& t) { put(t, 2, 0, 25, 83); }, "null address");
    expect_fuse("unaligned map", [](Fuse& t) { put(t, 4, 0x1002, 47, 156); }, "not aligned");
    expect_fuse("map height 0", [](Fuse& t) { put(t, 0, 0x1000, 0, 42); }, "bad sizes");
    expect_fuse("map more than twice the output", [](Fuse& t) { put(t, 1, 0x1000, 751, 63); }, "at most twice");
    expect_fuse("map width more than twice", [](Fuse& t) { put(t, 1, 0x1000, 19, 2485); }, "at most twice");

    expect_colors("valid colours", {5, 70000, 0xffffff, 1, 0, 255}, 3, nullptr);
    expect_colors("K 0", {0, 0}, 0, "colour codes");
    expect_colors("K 1025", std::vector<int32_t>(2050, 0), 1025, "colour codes");
    expect_colors("code beyond 24 bits", {5, 0x1000000, 1, 2}, 2, "a code is");
    expect_colors("negative code", {-1, 5, 1, 2}, 2, "a code is");
    expect_colors("unsorted", {7, 5, 1, 2}, 2, "not sorted");
    expect_colors("a code twice", {5, 5, 1, 2}, 2, "not sorted");
    expect_colors("label 256", {5, 6, 1, 256}, 2, "outside 0 .. 255");
    expect_colors("label -1", {5, 6, -1, 2}, 2, "outside 0 .. 255");

    for (int K : {1, 2, 3, 7, 64, 1000, SEG_MAX_COLORS}) {
        std::vector<int32_t> codes(K);
        for (int k = 0; k < K; k++) codes[k] = 3 * k + 1;
        bool ok = seg_find(codes.data(), K, 0) == -1 && seg_find(codes.data(), K, 3 * K + 5) == -1;
        for (int k = 0; k < K && ok; k++)
            ok = seg_find(codes.data(), K, codes[k]) == k && seg_find(codes.data(), K, codes[k] + 1) == -1;
        std::printf("seg_find, K %-4d                     %s\n", K, ok ? "ok  " : "FAIL");
        if (!ok) failures++;
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("segm_tail_check: ok\n");
    return 0;
}
