// Host walk over the coefficient arithmetic, the caps, the workspace layout and the validators of the Mask R-CNN training item
// (3d-sdn_amd/csrc/training_item_check.h):
//   - the coefficients the mini-mask kernel computes per box (tri_ksize, tri_coeffs): for every source size 1 .. 1024 to 56, 28, 7 and 1
//     outputs the filter width is the band plan's (sgt_taps), the taps lie inside the source, out * ksize fits TRI_COEF_INTS, the
//     fixed-point weights of an output sum to 2^22 within one unit per tap; a few values are known by hand; a hash of every table
//     to 56 and to 28 is printed, which tests/test_training_item_host.py compares with Pillow's tables as sdn_hip/pillow.py states them;
//   - the layout: the ranges lie inside `total`, start on 16 bytes and do not overlap;
//   - the validators: a valid plan built here passes, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/training_item_check.cpp
//       -o /tmp/training_item_check && /tmp/training_item_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "training_item_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static uint64_t fnv(uint64_t h, int32_t v) { return (h ^ (uint64_t)(uint32_t)v) * 1099511628211ull; }

static uint64_t walk_tables(int out, int max_in, bool* ok)
{
    uint64_t h = 1469598103934665603ull;
    for (int in = 1; in <= max_in; in++) {
        const int ksize = tri_ksize(in, out);
        *ok = *ok && ksize == sgt_taps(in, out) && (long)out * ksize <= TRI_COEF_INTS;
        h = fnv(h, ksize);
        std::vector<int32_t> k((size_t)ksize);
        for (int xx = 0; xx < out; xx++) {
            int first = -1, count = -1;
            tri_coeffs(in, out, xx, ksize, &first, &count, k.data());
            long sum = 0;
            for (int t = 0; t < ksize; t++) {
                sum += k[t];
                *ok = *ok && k[t] >= 0 && (t < count || k[t] == 0);
                h = fnv(h, k[t]);
            }
            h = fnv(fnv(h, first), count);
            *ok = *ok && first >= 0 && count >= 1 && count <= ksize && first + count <= in && std::labs(sum - (1L << SGT_BITS)) <= count;
        }
    }
    return h;
}

static void walk_coefficients()
{
    bool ok = true;
    const uint64_t h56 = walk_tables(56, TRI_MAX_DIM, &ok), h28 = walk_tables(28, 64, &ok);
    walk_tables(7, TRI_MAX_DIM, &ok);
    walk_tables(1, TRI_MAX_DIM, &ok);
    expect(ok, "the width is the band plan's, the taps lie inside the source and fit the LDS, the weights sum to 2^22");
    std::printf("tables 56 %016llx\ntables 28 %016llx\n", (unsigned long long)h56, (unsigned long long)h28);
    int32_t k[8];
    int first, count;
    tri_coeffs(2, 1, 0, tri_ksize(2, 1), &first, &count, k);
    expect(tri_ksize(2, 1) == 5 && first == 0 && count == 2 && k[0] == 2097152 && k[1] == 2097152 && k[2] == 0, "2 -> 1: two halves");
    tri_coeffs(1, 2, 1, tri_ksize(1, 2), &first, &count, k);
    expect(tri_ksize(1, 2) == 3 && first == 0 && count == 1 && k[0] == 4194304, "1 -> 2: the one pixel");
    tri_coeffs(4, 2, 0, tri_ksize(4, 2), &first, &count, k);
    expect(tri_ksize(4, 2) == 5 && first == 0 && count == 3 && k[0] == 1797559 && k[1] == 1797559 && k[2] == 599186, "4 -> 2: 3/7, 3/7, 1/7");
    expect(tri_ksize(1024, 56) == 39 && tri_ksize(1024, 28) == 75 && tri_ksize(56, 56) == 3, "39 taps for 1024 rows to 56");
    expect((long)TRI_MAX_DIM * TRI_MAX_MINI == 57344, "the horizontal result of a 1024-row box is 56 KiB");
}

static void walk_layout()
{
    char msg[256];
    bool ok = true;
    const int sizes[][4] = {{1, 1, 1, 1}, {1, 375, 1242, 24}, {4, 128, 128, 0}, {1, 1024, 2048, TRI_MAX_BOXES}};
    for (auto& s : sizes) {
        TriLayout L;
        ok = ok && tri_layout(s[0], s[1], s[2], s[3], &L, msg, sizeof(msg)) == 0;
        const size_t nblk = ((size_t)s[1] * s[2] + SGT_STAT_PIXELS - 1) / SGT_STAT_PIXELS;
        ok = ok && L.partial == 0 && L.acc % 16 == 0 && L.total % 16 == 0 && L.partial + 4 * s[0] * nblk <= L.acc &&
             L.acc + 4 * (size_t)TRI_ACC_ROWS * s[3] <= L.total;
    }
    expect(ok, "the workspace's ranges start on 16 bytes, hold what they must and do not overlap");
    expect(tri_layout(1, 10, 10, 1, nullptr, msg, sizeof(msg)) == 1 && std::strstr(msg, "layout is NULL"), "a NULL layout is refused");
}

// ndimage.zoom(order=0): the index table of an axis (geometric/maskrcnn/training_item.py: zoom_table)
static void zoom_table(int n_in, int n_out, int32_t* t)
{
    for (int i = 0; i < n_out; i++) {
        const double c = n_out > 1 ? (double)i * ((double)(n_in - 1) / (double)(n_out - 1)) : 0.0;
        t[i] = c > (double)(n_in - 1) ? -1 : (int32_t)std::floor(c + 0.5);
    }
}

// a parameter block for H x W -> oh x ow in M x M, laid out as plan_block does
static std::vector<int32_t> make_plan(int H, int W, int oh, int ow, int M)
{
    std::vector<int32_t> T((size_t)TRI_PLAN_INTS, 0);
    TriPlan p;
    std::memset(&p, 0, sizeof(p));
    p.H = H, p.W = W, p.oh = oh, p.ow = ow, p.M = M, p.top = (M - oh) / 2, p.left = (M - ow) / 2;
    p.fb = p.fc = p.fs = 1.0f;
    const auto axis = [&T](int in, int out, int* boff, int* koff, int* ksize) {
        *boff = *koff = *ksize = 0;
        if (in == out) return;
        *ksize = tri_ksize(in, out);
        *boff = (int)T.size();
        T.resize(T.size() + 2 * (size_t)out);
        *koff = (int)T.size();
        T.resize(T.size() + (size_t)out * *ksize);
        for (int xx = 0; xx < out; xx++) tri_coeffs(in, out, xx, *ksize, &T[*boff + 2 * xx], &T[*boff + 2 * xx + 1], &T[*koff + (size_t)xx * *ksize]);
    };
    axis(W, ow, &p.xb, &p.xk, &p.xksize);
    axis(H, oh, &p.yb, &p.yk, &p.yksize);
    p.ytab = (int)T.size();
    T.resize(T.size() + (size_t)oh);
    zoom_table(H, oh, &T[p.ytab]);
    p.xtab = (int)T.size();
    T.resize(T.size() + (size_t)ow);
    zoom_table(W, ow, &T[p.xtab]);
    p.mean = (int)T.size();
    T.resize(T.size() + TRI_MEAN_INTS);
    std::memcpy(T.data(), &p, sizeof(p));
    return T;
}

static TriPlan head_of(const std::vector<int32_t>& T)
{
    TriPlan p;
    std::memcpy(&p, T.data(), sizeof(p));
    return p;
}

static void plan_refused(std::vector<int32_t> T, const TriPlan& p, int H, int W, const char* reason, const char* what)
{
    std::memcpy(T.data(), &p, sizeof(p));
    char msg[320] = "";
    const bool ok = tri_validate_plan(T.data(), (long)T.size(), H, W, msg, sizeof(msg)) == 1 && std::strstr(msg, reason) != nullptr;
    if (!ok) std::printf("  got: %s\n", msg);
    expect(ok, what);
}

static void walk_validators()
{
    char msg[320] = "";
    const std::vector<int32_t> down = make_plan(75, 248, 58, 192, 192), real = make_plan(375, 1242, 309, 1024, 1024),
                               same = make_plan(99, 121, 99, 121, 128), up = make_plan(40, 60, 96, 144, 192);
    expect(tri_validate_plan(down.data(), (long)down.size(), 75, 248, msg, sizeof(msg)) == 0, "75 x 248 -> 58 x 192 passes");
    expect(tri_validate_plan(real.data(), (long)real.size(), 375, 1242, msg, sizeof(msg)) == 0, "375 x 1242 -> 309 x 1024 passes");
    expect(tri_validate_plan(same.data(), (long)same.size(), 99, 121, msg, sizeof(msg)) == 0, "a plan without a resize passes");
    expect(tri_validate_plan(up.data(), (long)up.size(), 40, 60, msg, sizeof(msg)) == 0, "an upscale passes");
    expect(down[head_of(down).xtab + 191] == -1 && down[head_of(down).xtab + 190] == 246, "248 -> 192: the last column is the constant");
    expect(real[head_of(real).xtab + 1023] == 1241 && real[head_of(real).ytab + 308] == 374, "1242 -> 1024 and 375 -> 309: the last index is read");
    TriPlan p = head_of(down);
    p.M = 2048, plan_refused(down, p, 75, 248, "IMAGE_MAX_DIM 2048; 1 to 1024", "M too large");
    p = head_of(down), p.oh = 200, plan_refused(down, p, 75, 248, "resized to 200 x 192", "resized above M");
    p = head_of(down), p.top = 3, plan_refused(down, p, 75, 248, "padding (3, 0)", "a wrong pad");
    p = head_of(down), p.flip = 2, plan_refused(down, p, 75, 248, "flip 2", "flip 2");
    p = head_of(down), p.nops = 5, plan_refused(down, p, 75, 248, "5 ops", "five ops");
    p = head_of(down), p.nops = 2, p.order = 0x11, plan_refused(down, p, 75, 248, "not a permutation", "an op twice");
    p = head_of(down), p.hue = 256, plan_refused(down, p, 75, 248, "hue shift 256", "hue 256");
    p = head_of(down), p.xksize = 3, plan_refused(down, p, 75, 248, "3 taps for the horizontal resize", "a wrong filter width");
    p = head_of(down), p.xk = (int)down.size(), plan_refused(down, p, 75, 248, "lie outside the buffer", "coefficients outside");
    p = head_of(down), p.ytab = (int)down.size() - 10, plan_refused(down, p, 75, 248, "zoom tables", "zoom table outside");
    p = head_of(down), p.mean = (int)down.size() - 10, plan_refused(down, p, 75, 248, "mean table", "mean table outside");
    plan_refused(down, head_of(down), 75, 250, "the frames are 75 x 250", "another frame size");
    std::vector<int32_t> bad = down;
    bad[head_of(down).xtab + 5] = 248;
    plan_refused(bad, head_of(down), 75, 248, "zoom column 5 reads column 248", "a zoom index outside the frame");
    bad = down, bad[head_of(down).xb + 1] = 0;
    plan_refused(bad, head_of(down), 75, 248, "bounds of output 0", "an empty tap range");
    std::vector<int32_t> big = make_plan(2048, 2048, 1024, 1024, 1024);
    TriPlan pb = head_of(big);
    pb.nops = 1, pb.order = 1, plan_refused(big, pb, 2048, 2048, "contrast on a frame of 4194304 pixels", "contrast on too large a frame");
    expect(tri_validate_plan(big.data(), (long)big.size(), 2048, 2048, msg, sizeof(msg)) == 0, "2048 x 2048 -> 1024 x 1024 fits the band plan");
    expect(tri_validate_plan(down.data(), 10, 75, 248, msg, sizeof(msg)) == 1 && std::strstr(msg, "cannot hold its head"), "a short block");
    expect(tri_validate_plan(nullptr, 100, 75, 248, msg, sizeof(msg)) == 1 && std::strstr(msg, "is NULL"), "a NULL block");

    const void* q = reinterpret_cast<const void*>(0x10000);   // never dereferenced
    const auto off = [](const void* r, int n) { return reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(r) + n); };
    const auto item = [&](const void* frame, const void* ids, int G, int mini, int mh, int mw, const void* ws, size_t ws_bytes, const void* masks,
                          const void* bad_ptr, const char* reason) {
        char m[320] = "";
        const int rc = tri_validate_item(frame, q, ids, 75, 248, G, down.data(), q, (long)down.size(), mini, mh, mw, ws, ws_bytes, q, q, q, q, masks, q,
                                         bad_ptr, m, sizeof(m));
        if (!reason) return rc == 0;
        const bool ok = rc == 1 && std::strstr(m, reason) != nullptr;
        if (!ok) std::printf("  got: %s\n", m);
        return ok;
    };
    expect(item(q, q, 7, 1, 56, 56, q, 1 << 20, q, q, nullptr), "a valid item passes");
    expect(item(q, q, 128, 0, 0, 0, q, 1 << 20, q, q, nullptr), "G = 128 without mini-masks passes");
    expect(item(q, q, 0, 1, 56, 56, q, 1 << 20, q, q, "G 0; 1 to 128"), "G = 0");
    expect(item(q, q, 129, 1, 56, 56, q, 1 << 20, q, q, "G 129; 1 to 128"), "G = 129");
    expect(item(q, q, 7, 1, 57, 56, q, 1 << 20, q, q, "mini-masks of 57 x 56"), "a mini-mask side of 57");
    expect(item(q, q, 7, 1, 56, 0, q, 1 << 20, q, q, "mini-masks of 56 x 0"), "a mini-mask side of 0");
    expect(item(nullptr, q, 7, 1, 56, 56, q, 1 << 20, q, q, "frame, inst_map, ids, plan or image is NULL"), "frame NULL");
    expect(item(q, nullptr, 7, 1, 56, 56, q, 1 << 20, q, q, "frame, inst_map, ids, plan or image is NULL"), "ids NULL");
    expect(item(q, q, 7, 1, 56, 56, q, 1 << 20, nullptr, q, "boxes_int, boxes, boxes_norm, masks, areas or bad is NULL"), "masks NULL");
    expect(item(q, q, 7, 1, 56, 56, q, 1 << 20, q, nullptr, "boxes_int, boxes, boxes_norm, masks, areas or bad is NULL"), "bad NULL");
    expect(item(q, q, 7, 1, 56, 56, nullptr, 1 << 20, q, q, "workspace is NULL"), "workspace NULL");
    expect(item(q, q, 7, 1, 56, 56, q, 16, q, q, "workspace 16 <"), "workspace too small");
    expect(item(q, off(q, 2), 7, 1, 56, 56, q, 1 << 20, q, q, "inst_map, ids, plan and image must be aligned to 4 bytes"), "ids misaligned");
    expect(item(q, q, 7, 1, 56, 56, q, 1 << 20, off(q, 2), q, "must be aligned to 4 bytes"), "masks misaligned");
    expect(item(q, q, 7, 1, 56, 56, off(q, 8), 1 << 20, q, q, "workspace must be aligned to 16 bytes"), "workspace misaligned");
    char m[320] = "";
    expect(tri_validate_image(q, 2, 75, 248, down.data(), q, (long)down.size(), q, 1 << 20, q, m, sizeof(m)) == 0, "a valid image call passes");
    expect(tri_validate_image(q, 0, 75, 248, down.data(), q, (long)down.size(), q, 1 << 20, q, m, sizeof(m)) == 1 && std::strstr(m, "0 frames"), "no frame");
    expect(tri_validate_image(q, 1, 75, 5000, down.data(), q, (long)down.size(), q, 1 << 20, q, m, sizeof(m)) == 1 && std::strstr(m, "5000 pixels wide"), "too wide a frame");
    expect(tri_validate_image(q, 1, 75, 248, down.data(), q, (long)down.size(), q, 1 << 20, nullptr, m, sizeof(m)) == 1 && std::strstr(m, "frames, plan or image is NULL"), "image NULL");
    std::printf("the validators: walked\n");
}

int main()
{
    walk_coefficients();
    walk_layout();
    walk_validators();
    std::printf("training_item_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
