// Host walk over the layout, the level rule and the validators of the pyramid RoIAlign (3d-sdn_amd/csrc/pyramid_roi_align_check.h):
//   - the gradient buffer: for many (C, H[4], W[4]) the four ranges lie inside `total`, each starts on 16 bytes, they share no float
//     and the padding between them is less than four floats;
//   - the (channel, sample) walk of a workgroup as the kernels advance it without a division, against the division, for every pool
//     1 .. 32 and several channel counts: every element of every chunk exactly once, none outside the box's block;
//   - the level rule: rounding half to even, the clamp, the non-finite values, boxes of area 0 and below;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/pyramid_roi_align_check.cpp
//       -o /tmp/pyramid_roi_align_check && /tmp/pyramid_roi_align_check
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pyramid_roi_align_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static void walk_layout(int C, const int* H, const int* W)
{
    char msg[256];
    size_t off[PRA_LEVELS], total = 0;
    bool ok = pra_grad_layout(C, H, W, off, &total, msg, sizeof(msg)) == 0 && total % PRA_ALIGN_FLOATS == 0;
    std::vector<unsigned char> buf(ok ? total : 0, 0);   // real memory, so that ASan sees a range that leaves it
    size_t used = 0;
    for (int l = 0; l < PRA_LEVELS && ok; l++) {
        const size_t n = (size_t)C * H[l] * W[l];
        ok = off[l] % PRA_ALIGN_FLOATS == 0 && off[l] + n <= total && (l == 0 ? off[l] == 0 : off[l] >= off[l - 1]);
        for (size_t i = 0; i < n && ok; i++) buf[off[l] + i] += 1;
        used += n;
    }
    size_t once = 0;
    for (size_t i = 0; i < buf.size() && ok; i++) {
        ok = buf[i] <= 1;
        once += buf[i];
    }
    expect(ok && once == used && total - used < (size_t)PRA_LEVELS * PRA_ALIGN_FLOATS, "the four gradient ranges tile the buffer");
}

static void walk_chunks(int C, int pool)
{
    const int pp = pool * pool, chunks = pra_chunks(C);
    std::vector<unsigned char> block((size_t)C * pp, 0);   // one box's output block
    bool ok = chunks >= 1 && (chunks - 1) * PRA_CHANNELS < C && chunks * PRA_CHANNELS >= C;
    for (int chunk = 0; chunk < chunks && ok; chunk++) {
        const int c0 = chunk * PRA_CHANNELS, nc = (C - c0 < PRA_CHANNELS ? C - c0 : PRA_CHANNELS), total = nc * pp;
        const int dc = PRA_THREADS / pp, ds = PRA_THREADS - dc * pp;
        for (int tid = 0; tid < PRA_THREADS && ok; tid++) {
            int c = tid / pp, s = tid - c * pp;
            for (int i = tid; i < total && ok; i += PRA_THREADS) {
                ok = c == i / pp && s == i % pp && c < nc && s < pp;
                if (ok) block[((size_t)c0 + c) * pp + s] += 1;
                c += dc;
                s += ds;
                if (s >= pp) {
                    s -= pp;
                    c++;
                }
            }
        }
    }
    for (size_t i = 0; i < block.size() && ok; i++) ok = block[i] == 1;
    expect(ok && pra_table_bytes(pool) == (size_t)pp * 28 && pra_table_bytes(pool) <= 64 * 1024, "the chunks' walks cover the box's block once");
}

static void walk_levels()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    expect(pra_level_of(2.5f) == 2 && pra_level_of(3.5f) == 4 && pra_level_of(4.5f) == 4 && pra_level_of(5.5f) == 5, "half to even");
    expect(pra_level_of(2.4999f) == 2 && pra_level_of(2.5001f) == 3 && pra_level_of(4.5001f) == 5, "beside the halves");
    expect(pra_level_of(-40.0f) == 2 && pra_level_of(1.0f) == 2 && pra_level_of(6.0f) == 5 && pra_level_of(3e38f) == 5 && pra_level_of(-3e38f) == 2, "the clamp");
    expect(pra_level_of(nan) == 2 && pra_level_of(inf) == 2 && pra_level_of(-inf) == 2, "non-finite values give level 2");
    const float area = 1024.0f * 1024.0f;
    // a 224 x 224 pixel box of a 1024 x 1024 image maps to P4 (model.py:451)
    expect(pra_level_of(pra_level_value(0.0f, 0.0f, 0.21875f, 0.21875f, area)) == 4, "224 pixels map to P4");
    expect(pra_level_of(pra_level_value(0.0f, 0.0f, 0.4375f, 0.4375f, area)) == 5 && pra_level_of(pra_level_value(0.0f, 0.0f, 0.109375f, 0.109375f, area)) == 3 &&
               pra_level_of(pra_level_value(0.0f, 0.0f, 0.0546875f, 0.0546875f, area)) == 2, "halving the side lowers the level by one");
    expect(pra_level_of(pra_level_value(0.2f, 0.3f, 0.2f, 0.7f, area)) == 2, "area 0: log(0) = -inf gives level 2");
    expect(pra_level_of(pra_level_value(0.7f, 0.2f, 0.3f, 0.8f, area)) == 2, "area below 0: sqrt gives NaN, level 2");
    expect(pra_level_of(pra_level_value(nan, 0.2f, 0.3f, 0.8f, area)) == 2, "a NaN coordinate gives level 2");
    expect(pra_level_of(pra_level_value(0.0f, 0.0f, 1e-30f, 1e-30f, area)) == 2 && pra_level_of(pra_level_value(0.0f, 0.0f, 1e19f, 1e19f, area)) == 5 &&
               pra_level_of(pra_level_value(0.0f, 0.0f, 3e20f, 3e20f, area)) == 2, "underflow to 0, a huge box, overflow to inf");
}

static bool refused(int rc, const char* msg, const char* reason)
{
    return rc == 1 && std::strstr(msg, reason) != nullptr;
}

static void walk_validators()
{
    char msg[256];
    const int H[4] = {24, 12, 6, 3}, W[4] = {20, 10, 5, 3};
    float store[8] = {};
    const void* maps[4] = {store, store, store, store};
    const float area = 1048576.0f;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    size_t off[4], total;
    expect(pra_validate_fwd(store, maps, H, W, 5, 67, 7, area, store, store, msg, sizeof(msg)) == 0, "a valid forward call");
    alignas(16) float g16[4] = {};
    expect(pra_validate_bwd(store, store, H, W, 5, 67, 14, area, g16, msg, sizeof(msg)) == 0, "a valid backward call");
    expect(pra_validate_fwd(nullptr, nullptr, H, W, 0, 3, 7, area, nullptr, nullptr, msg, sizeof(msg)) == 0, "R = 0 reads and writes nothing");
    expect(pra_validate_bwd(nullptr, nullptr, H, W, 0, 3, 7, area, g16, msg, sizeof(msg)) == 0, "R = 0 backward still has a buffer to zero");
    expect(refused(pra_validate_bwd(nullptr, nullptr, H, W, 0, 3, 7, area, nullptr, msg, sizeof(msg)), msg, "grad_maps is NULL"), "R = 0 backward, no buffer");
    // every rejection
    expect(refused(pra_validate_fwd(store, maps, H, W, -1, 3, 7, area, store, store, msg, sizeof(msg)), msg, "bad sizes: R -1"), "R < 0");
    expect(refused(pra_validate_fwd(store, maps, H, W, 5, 0, 7, area, store, store, msg, sizeof(msg)), msg, "bad sizes: C 0"), "C = 0");
    expect(refused(pra_validate_fwd(store, maps, H, W, 5, -4, 7, area, store, store, msg, sizeof(msg)), msg, "bad sizes: C -4"), "C < 0");
    expect(refused(pra_validate_fwd(store, maps, nullptr, W, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "H or W is NULL"), "H NULL");
    expect(refused(pra_validate_fwd(store, maps, H, nullptr, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "H or W is NULL"), "W NULL");
    for (int l = 0; l < 4; l++) {
        int h[4] = {24, 12, 6, 3}, w[4] = {20, 10, 5, 3};
        h[l] = 0;
        expect(refused(pra_validate_fwd(store, maps, h, w, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "bad sizes: level P"), "H = 0");
        h[l] = 4;
        w[l] = -2;
        expect(refused(pra_validate_bwd(store, store, h, w, 5, 3, 7, area, g16, msg, sizeof(msg)), msg, "bad sizes: level P"), "W < 0");
        w[l] = 4;
        const void* m[4] = {store, store, store, store};
        m[l] = nullptr;
        expect(refused(pra_validate_fwd(store, m, h, w, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "is NULL with R > 0"), "a map NULL");
        m[l] = reinterpret_cast<const unsigned char*>(store) + 2;
        expect(refused(pra_validate_fwd(store, m, h, w, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "aligned to 4"), "a map misaligned");
        h[l] = 65536;
        w[l] = 32768;                                                       // H * W = 2^31
        expect(refused(pra_validate_fwd(store, maps, h, w, 5, 1, 7, area, store, store, msg, sizeof(msg)), msg, "below 2^31"), "H * W = 2^31");
        h[l] = 0x7fffffff;
        w[l] = 0x7fffffff;                                                  // the check itself must not overflow
        expect(refused(pra_validate_fwd(store, maps, h, w, 5, 0x7fffffff, 7, area, store, store, msg, sizeof(msg)), msg, "below 2^31"), "huge sizes");
        h[l] = 1024;
        w[l] = 1024;
        expect(refused(pra_grad_layout(2048, h, w, off, &total, msg, sizeof(msg)), msg, "below 2^31"), "C * H * W = 2^31");
        expect(pra_grad_layout(2047, h, w, off, &total, msg, sizeof(msg)) == 0, "C * H * W just below 2^31");
    }
    expect(refused(pra_validate_fwd(store, maps, H, W, 5, 3, 0, area, store, store, msg, sizeof(msg)), msg, "pool 0; 1 to 32"), "pool 0");
    expect(refused(pra_validate_fwd(store, maps, H, W, 5, 3, 33, area, store, store, msg, sizeof(msg)), msg, "pool 33; 1 to 32"), "pool 33");
    expect(refused(pra_validate_bwd(store, store, H, W, 5, 3, -7, area, g16, msg, sizeof(msg)), msg, "pool -7"), "pool < 0");
    expect(pra_validate_fwd(store, maps, H, W, 5, 3, 32, area, store, store, msg, sizeof(msg)) == 0, "pool 32");
    const float bad_area[5] = {0.0f, -1.0f, inf, -inf, nan};
    for (float a : bad_area) {
        expect(refused(pra_validate_fwd(store, maps, H, W, 5, 3, 7, a, store, store, msg, sizeof(msg)), msg, "must be finite and positive"), "image_area fwd");
        expect(refused(pra_validate_bwd(store, store, H, W, 5, 3, 7, a, g16, msg, sizeof(msg)), msg, "must be finite and positive"), "image_area bwd");
    }
    const int h1[4] = {1, 1, 1, 1};
    expect(refused(pra_validate_fwd(store, maps, h1, h1, 5, 3000000, 32, area, store, store, msg, sizeof(msg)), msg, "C * pool * pool"), "C * pool^2 = 3e9");
    expect(refused(pra_validate_fwd(store, maps, h1, h1, 0x7fffffff, 2000000, 7, area, store, store, msg, sizeof(msg)), msg, "workgroups"), "R * chunks");
    expect(refused(pra_validate_fwd(nullptr, maps, H, W, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "is NULL with R > 0"), "boxes NULL");
    expect(refused(pra_validate_fwd(store, maps, H, W, 5, 3, 7, area, nullptr, store, msg, sizeof(msg)), msg, "is NULL with R > 0"), "pooled NULL");
    expect(refused(pra_validate_fwd(store, maps, H, W, 5, 3, 7, area, store, nullptr, msg, sizeof(msg)), msg, "is NULL with R > 0"), "levels NULL");
    expect(refused(pra_validate_fwd(store, nullptr, H, W, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg, "maps is NULL"), "maps NULL");
    expect(refused(pra_validate_fwd(reinterpret_cast<const unsigned char*>(store) + 1, maps, H, W, 5, 3, 7, area, store, store, msg, sizeof(msg)), msg,
                   "aligned to 4"), "boxes misaligned");
    expect(refused(pra_validate_bwd(nullptr, store, H, W, 5, 3, 7, area, g16, msg, sizeof(msg)), msg, "grads or boxes is NULL"), "grads NULL");
    expect(refused(pra_validate_bwd(store, nullptr, H, W, 5, 3, 7, area, g16, msg, sizeof(msg)), msg, "grads or boxes is NULL"), "boxes NULL, backward");
    expect(refused(pra_validate_bwd(store, store, H, W, 5, 3, 7, area, g16 + 1, msg, sizeof(msg)), msg, "aligned to 16"), "grad_maps misaligned");
    expect(refused(pra_grad_layout(3, H, W, nullptr, &total, msg, sizeof(msg)), msg, "offsets or total is NULL"), "offsets NULL");
    expect(refused(pra_grad_layout(3, H, W, off, nullptr, msg, sizeof(msg)), msg, "offsets or total is NULL"), "total NULL");
    expect(refused(pra_grad_layout(0, H, W, off, &total, msg, sizeof(msg)), msg, "bad sizes: C 0"), "layout, C = 0");
}

int main()
{
    const int shapes[6][8] = {{24, 12, 6, 3, 20, 10, 5, 3}, {1, 12, 6, 1, 20, 1, 5, 1}, {1, 1, 1, 1, 1, 1, 1, 1},
                              {7, 3, 5, 2, 3, 3, 1, 9},     {256, 128, 64, 32, 256, 128, 64, 32}, {5, 5, 5, 5, 5, 5, 5, 5}};
    int layouts = 0;
    for (const auto& s : shapes)
        for (int C = 1; C <= 70; C += (s[0] == 256 ? 23 : 1)) {
            walk_layout(C, s, s + 4);
            layouts++;
        }
    int walks = 0;
    for (int pool = 1; pool <= PRA_MAX_POOL; pool++)
        for (int C : {1, 3, 63, 64, 65, 67, 128, 200}) {
            walk_chunks(C, pool);
            walks++;
        }
    walk_levels();
    walk_validators();
    std::printf("pyramid_roi_align_check: %d layouts, %d chunk walks, the level rule, the validators: %d failures\n", layouts, walks, failures);
    return failures ? 1 : 0;
}
