// Host walk over the level prefix table, the index map and the validators of the fused RPN output kernels
// (3d-sdn_amd/csrc/rpn_outputs_check.h):
//   - the table: over level lists of every length 1 .. 8 the workgroups tile every level's pixels exactly once, rpo_level_of finds the
//     owner, and the three output runs of the workgroups, in order, tile [0, B * A * comps) without a gap or an overlap;
//   - the index map: every (level, image, pixel, anchor, component) lands in its own output element and comes from its own map
//     element, and the run a workgroup writes holds exactly its pixels' elements in the padded tile's order (rpo_padded);
//   - the store split: for every offset and length the scalar head, the 16-byte body and the scalar tail write every float once and
//     every 16-byte store is aligned;
//   - the LDS tile: the three padded ranges lie inside rpo_lds_floats(k) for k = 1 .. 16, below 64 KiB;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/rpn_outputs_check.cpp
//       -o /tmp/rpn_outputs_check && /tmp/rpn_outputs_check
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rpn_outputs_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static void walk_table(const std::vector<int>& H, const std::vector<int>& W, int k, int B)
{
    char msg[256] = "";
    RpoTable T;
    const int L = (int)H.size();
    bool ok = rpo_table(H.data(), W.data(), L, k, B, &T, msg, sizeof(msg)) == 0;
    if (!ok) {
        expect(false, "a valid level list has a table");
        return;
    }
    long long pixels = 0;
    for (int l = 0; l < L; l++) {
        ok = ok && T.hw[l] == H[(size_t)l] * W[(size_t)l] && T.pix[l] == pixels && T.tile[l + 1] - T.tile[l] == rpo_tiles(T.hw[l]);
        pixels += T.hw[l];
    }
    ok = ok && T.pix[L] == pixels && T.anchors == k * pixels && T.tile[0] == 0 && T.L == L && T.k == k && T.B == B;
    expect(ok, "the prefix sums are the levels' sizes");
    for (int comps : {2, 4}) {
        const size_t total = (size_t)B * (size_t)T.anchors * (size_t)comps;
        std::vector<unsigned char> out(total, 0);   // real memory, so that ASan sees an index that leaves it
        std::vector<std::vector<unsigned char>> maps;
        for (int l = 0; l < L; l++) maps.emplace_back((size_t)B * (size_t)(comps * k) * (size_t)T.hw[l], 0);
        bool fine = true;
        for (int b = 0; b < B; b++)
            for (int t = 0; t < T.tile[L]; t++) {
                const int l = rpo_level_of(T, t);
                fine = fine && l >= 0 && l < L && t >= T.tile[l] && t < T.tile[l + 1];
                const int pix0 = (t - T.tile[l]) * RPO_TILE, n = std::min(RPO_TILE, T.hw[l] - pix0), ch = comps * k;
                fine = fine && n >= 1;
                const long long first = ((long long)b * T.anchors + (long long)k * (T.pix[l] + pix0)) * comps;   // the kernel's run
                std::vector<int> tile((size_t)(RPO_TILE * (ch + 1)), -1);
                for (int p = 0; p < n; p++)
                    for (int c = 0; c < ch; c++) tile[(size_t)(p * (ch + 1) + c)] = p * ch + c;
                for (int i = 0; i < n * ch; i++) {
                    const int p = i / ch, c = i % ch, a = c / comps, j = c % comps;
                    const long long o = rpo_out_index(T, l, b, pix0 + p, a, j, comps);
                    const long long m = rpo_map_index(T, l, b, pix0 + p, a, j, comps);
                    fine = fine && o == first + i && tile[(size_t)rpo_padded(i, ch)] == i;
                    out[(size_t)o] += 1;
                    maps[(size_t)l][(size_t)m] += 1;
                }
            }
        for (unsigned char v : out) fine = fine && v == 1;
        for (const auto& m : maps)
            for (unsigned char v : m) fine = fine && v == 1;
        expect(fine, "every output element is written once, from its own map element, in the run of its workgroup");
    }
}

static void walk_split()
{
    bool ok = true;
    for (unsigned at = 0; at < 8; at++)
        for (int len = 0; len <= 70; len++) {
            std::vector<unsigned char> hit((size_t)len, 0);
            int head = (int)((4u - (at & 3u)) & 3u);
            head = head < len ? head : len;
            const int quads = (len - head) >> 2;
            for (int i = 0; i < head; i++) hit[(size_t)i] += 1;
            for (int q = 0; q < quads; q++) {
                const int i = head + 4 * q;
                ok = ok && ((at + (unsigned)i) & 3u) == 0;
                for (int e = 0; e < 4; e++) hit[(size_t)(i + e)] += 1;
            }
            for (int t = 0; t < RPO_THREADS; t++) {
                const int i = head + 4 * quads + t;
                if (i < len) hit[(size_t)i] += 1;
            }
            ok = ok && head <= 3 && len - head - 4 * quads <= 3;
            for (unsigned char v : hit) ok = ok && v == 1;
        }
    expect(ok, "head, body and tail write every float once and the 16-byte stores are aligned");
}

static void walk_lds()
{
    bool ok = RPO_THREADS % 64 == 0 && RPO_TILE == 64;
    for (int k = 1; k <= RPO_MAX_K; k++) {
        const int c2 = 2 * k, c4 = 4 * k;
        const int last2 = rpo_padded(RPO_TILE * c2 - 1, c2), last4 = rpo_padded(RPO_TILE * c4 - 1, c4);
        ok = ok && last2 < RPO_TILE * (c2 + 1) && last4 < RPO_TILE * (c4 + 1);
        ok = ok && 2 * RPO_TILE * (c2 + 1) + RPO_TILE * (c4 + 1) == rpo_lds_floats(k) && sizeof(float) * (size_t)rpo_lds_floats(k) <= 64u * 1024u;
    }
    expect(ok, "the padded tiles lie inside the LDS range, below 64 KiB");
}

static bool refused(int rc, const char* msg, const char* reason)
{
    const bool ok = rc == 1 && std::strstr(msg, reason) != nullptr;
    if (!ok) std::printf("  rc %d, message \"%s\", wanted \"%s\"\n", rc, msg, reason);
    return ok;
}

static void walk_validators()
{
    char msg[256] = "";
    alignas(16) static unsigned char mem[64];
    const void* p = mem;
    const void* odd = mem + 2;
    const void* four = mem + 4;
    const int H[8] = {256, 128, 64, 32, 16, 3, 2, 1}, W[8] = {256, 128, 64, 32, 16, 5, 3, 1};
    const void* maps[8] = {p, p, p, p, p, four, four, p};
    RpoTable T;
    auto fwd = [&](const void* const* c, const void* const* b, const int* h, const int* w, int L, int k, int B, const void* o0, const void* o1,
                   const void* o2) { return rpo_validate_fwd(c, b, h, w, L, k, B, o0, o1, o2, &T, msg, sizeof(msg)); };
    expect(fwd(maps, maps, H, W, 5, 3, 1, p, p, p) == 0 && T.anchors == 261888 && T.tile[5] == 1024 + 256 + 64 + 16 + 4,
           "the reference's size passes: 261 888 anchors in 1364 workgroups");
    expect(fwd(maps, maps, H, W, 8, 16, 2, p, p, p) == 0, "eight levels, k = 16, maps on 4 bytes");
    expect(fwd(maps, maps, H + 7, W + 7, 1, 1, 1, p, p, p) == 0 && T.anchors == 1 && T.tile[1] == 1, "one level of one pixel");
    expect(refused(fwd(maps, maps, H, W, 0, 3, 1, p, p, p), msg, "L 0; 1 to 8 levels"), "L = 0");
    expect(refused(fwd(maps, maps, H, W, 9, 3, 1, p, p, p), msg, "L 9; 1 to 8 levels"), "L = 9");
    expect(refused(fwd(maps, maps, H, W, -1, 3, 1, p, p, p), msg, "L -1"), "L < 0");
    expect(refused(fwd(maps, maps, H, W, 5, 0, 1, p, p, p), msg, "k 0; 1 to 16 anchors"), "k = 0");
    expect(refused(fwd(maps, maps, H, W, 5, 17, 1, p, p, p), msg, "k 17; 1 to 16 anchors"), "k = 17");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 0, p, p, p), msg, "B 0; 1 to 65535"), "B = 0");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 65536, p, p, p), msg, "B 65536"), "B = 65536");
    expect(refused(fwd(maps, maps, nullptr, W, 5, 3, 1, p, p, p), msg, "H or W is NULL"), "H NULL");
    expect(refused(fwd(maps, maps, H, nullptr, 5, 3, 1, p, p, p), msg, "H or W is NULL"), "W NULL");
    const int Hbad[3] = {4, 0, 2}, Wneg[3] = {4, 4, -2}, W3[3] = {4, 4, 4}, H3[3] = {4, 4, 4};
    expect(refused(fwd(maps, maps, Hbad, W3, 3, 3, 1, p, p, p), msg, "level 1 is 0 x 4"), "a level without rows");
    expect(refused(fwd(maps, maps, H3, Wneg, 3, 3, 1, p, p, p), msg, "level 2 is 4 x -2"), "a level of negative width");
    const int big = std::numeric_limits<int>::max(), Hbig[2] = {big, 1 << 14}, Wbig[2] = {big, 1 << 14};
    expect(refused(fwd(maps, maps, Hbig, Wbig, 1, 1, 1, p, p, p), msg, "H * W ="), "H * W of a level at 2^62");
    expect(refused(fwd(maps, maps, Hbig + 1, Wbig + 1, 1, 2, 1, p, p, p), msg, "B * A * 4 = 2147483648 must stay below 2^31"), "B * A * 4 = 2^31");
    expect(fwd(maps, maps, Hbig + 1, Wbig + 1, 1, 1, 1, p, p, p) == 0, "B * A * 4 = 2^30 passes");
    expect(refused(fwd(maps, maps, Hbig + 1, Wbig + 1, 1, 1, 2, p, p, p), msg, "must stay below 2^31"), "the batch counts in the product");
    expect(refused(fwd(nullptr, maps, H, W, 5, 3, 1, p, p, p), msg, "class_maps is NULL"), "class_maps NULL");
    expect(refused(fwd(maps, nullptr, H, W, 5, 3, 1, p, p, p), msg, "bbox_maps is NULL"), "bbox_maps NULL");
    const void* hole[8] = {p, p, nullptr, p, p, p, p, p};
    const void* bent[8] = {p, p, p, odd, p, p, p, p};
    expect(refused(fwd(hole, maps, H, W, 5, 3, 1, p, p, p), msg, "class_maps[2] is NULL"), "one class map NULL");
    expect(refused(fwd(maps, hole, H, W, 5, 3, 1, p, p, p), msg, "bbox_maps[2] is NULL"), "one box map NULL");
    expect(fwd(hole, hole, H, W, 2, 3, 1, p, p, p) == 0, "pointers behind L are not looked at");
    expect(refused(fwd(bent, maps, H, W, 5, 3, 1, p, p, p), msg, "class_maps[3] must be aligned to 4 bytes"), "a class map on 2 bytes");
    expect(refused(fwd(maps, bent, H, W, 5, 3, 1, p, p, p), msg, "bbox_maps[3] must be aligned to 4 bytes"), "a box map on 2 bytes");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 1, nullptr, p, p), msg, "rpn_class_logits, rpn_probs or rpn_bbox is NULL"), "logits NULL");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 1, p, nullptr, p), msg, "rpn_class_logits, rpn_probs or rpn_bbox is NULL"), "probs NULL");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 1, p, p, nullptr), msg, "rpn_class_logits, rpn_probs or rpn_bbox is NULL"), "bbox NULL");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 1, four, p, p), msg, "must be aligned to 16 bytes"), "logits on 4 bytes");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 1, p, four, p), msg, "must be aligned to 16 bytes"), "probs on 4 bytes");
    expect(refused(fwd(maps, maps, H, W, 5, 3, 1, p, p, four), msg, "must be aligned to 16 bytes"), "bbox on 4 bytes");
    expect(rpo_table(H, W, 5, 3, 1, nullptr, msg, sizeof(msg)) == 1, "a NULL table");

    auto bwd = [&](const void* g0, const void* g1, const void* g2, const void* pr, int L, int k, int B, const void* const* c, const void* const* b) {
        return rpo_validate_bwd(g0, g1, g2, pr, H, W, L, k, B, c, b, &T, msg, sizeof(msg));
    };
    expect(bwd(p, p, p, p, 5, 3, 1, maps, maps) == 0, "a valid backward call passes");
    expect(bwd(four, nullptr, four, nullptr, 5, 3, 1, maps, maps) == 0, "training: no grad_probs, no rpn_probs, gradients on 4 bytes");
    expect(bwd(nullptr, nullptr, nullptr, nullptr, 5, 3, 1, maps, maps) == 0, "no gradient at all: the maps' gradients are zeros");
    expect(refused(bwd(p, p, p, nullptr, 5, 3, 1, maps, maps), msg, "rpn_probs is NULL although grad_probs is given"), "grad_probs without probs");
    expect(refused(bwd(odd, p, p, p, 5, 3, 1, maps, maps), msg, "must be aligned to 4 bytes"), "grad_logits on 2 bytes");
    expect(refused(bwd(p, odd, p, p, 5, 3, 1, maps, maps), msg, "must be aligned to 4 bytes"), "grad_probs on 2 bytes");
    expect(refused(bwd(p, p, odd, p, 5, 3, 1, maps, maps), msg, "must be aligned to 4 bytes"), "grad_bbox on 2 bytes");
    expect(refused(bwd(p, p, p, odd, 5, 3, 1, maps, maps), msg, "must be aligned to 4 bytes"), "rpn_probs on 2 bytes");
    expect(refused(bwd(p, p, p, p, 5, 3, 1, nullptr, maps), msg, "grad_class_maps is NULL"), "grad_class_maps NULL");
    expect(refused(bwd(p, p, p, p, 5, 3, 1, maps, hole), msg, "grad_bbox_maps[2] is NULL"), "one box gradient NULL");
    expect(refused(bwd(p, p, p, p, 5, 3, 1, bent, maps), msg, "grad_class_maps[3] must be aligned to 4 bytes"), "a class gradient on 2 bytes");
    expect(refused(bwd(p, p, p, p, 9, 3, 1, maps, maps), msg, "L 9"), "backward: L = 9");
    expect(refused(bwd(p, p, p, p, 5, 0, 1, maps, maps), msg, "k 0"), "backward: k = 0");
    expect(refused(bwd(p, p, p, p, 5, 3, 0, maps, maps), msg, "B 0"), "backward: B = 0");
}

int main()
{
    const std::vector<int> H5 = {24, 12, 6, 3, 2}, W5 = {40, 20, 10, 5, 3};
    for (int k : {1, 3, 5, 16})
        for (int B : {1, 2}) walk_table(H5, W5, k, B);
    walk_table({1}, {1}, 3, 1);
    walk_table({64}, {64}, 3, 1);
    walk_table({3, 5}, {5, 13}, 1, 3);
    walk_table({1, 1, 1, 1, 1, 1, 1, 1}, {1, 63, 64, 65, 127, 128, 129, 2}, 2, 1);
    std::printf("the table and the index map: %d failures so far\n", failures);
    walk_split();
    walk_lds();
    std::printf("the store split and the LDS tile: %d failures so far\n", failures);
    walk_validators();
    std::printf("the validators: %d failures so far\n", failures);
    std::printf("rpn_outputs_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
