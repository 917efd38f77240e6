// Host walk over the layouts, the tilings and the validators of the Derenderer's heads (3d-sdn_amd/csrc/derender_heads_check.h):
//   - the output buffer: the six groups tile [0, n * O) without a gap or an overlap; the saved buffer and the workspace likewise;
//   - the forward's last layer: the column ranges of its workgroups tile [0, O), the first one holds the 8 + classes head columns
//     within the 32 the LDS keeps, every other one at most 16;
//   - the slabs: they tile the terms of a sum, the four waves' 64-term shares tile a staged chunk;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/derender_heads_check.cpp
//       -o /tmp/derender_heads_check && /tmp/derender_heads_check
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "derender_heads_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static void mark(std::vector<unsigned char>& mem, long long at, long long count)
{
    for (long long i = 0; i < count; i++) mem[(size_t)(at + i)] += 1;   // real memory, so that ASan sees an index that leaves it
}

static void walk_layout(int n, int F, int Hd, int classes, int coeffs)
{
    char msg[256] = "";
    DhLayout L;
    if (dh_layout(n, F, Hd, classes, coeffs, &L, msg, sizeof(msg))) {
        expect(false, "a valid problem has a layout");
        return;
    }
    expect(L.O == 8 + classes + classes * coeffs && L.head == 8 + classes && L.K1 == Hd + 4 && L.ffd_w == classes * coeffs, "the widths");
    std::vector<unsigned char> out((size_t)L.out_floats, 0), saved((size_t)L.saved_floats, 0), ws((size_t)L.ws_floats, 0);
    const long long N = n;
    mark(out, L.theta, 2 * N);
    mark(out, L.trans, 2 * N);
    mark(out, L.scales, 3 * N);
    mark(out, L.depths, N);
    mark(out, L.probs, N * classes);
    mark(out, L.ffd, N * L.ffd_w);
    mark(saved, L.h0, N * Hd);
    mark(saved, L.h1, N * Hd);
    mark(saved, L.h2, N * Hd);
    mark(saved, L.norm, N);
    mark(ws, L.p2, (long long)L.S3 * N * Hd);
    mark(ws, L.p1, (long long)L.SH * N * Hd);
    mark(ws, L.p0, (long long)L.SH * N * Hd);
    bool fine = true;
    for (const auto* mem : {&out, &saved, &ws})
        for (unsigned char v : *mem) fine = fine && v == 1;
    expect(fine, "the pieces of out, saved and the workspace tile their buffers");
    expect(dh_workspace_bytes(L) >= sizeof(float) * (size_t)L.ws_floats && dh_workspace_bytes(L) % 256 == 0, "the workspace bytes");

    std::vector<unsigned char> cols((size_t)L.O, 0);
    const int tiles = dh_row_col_tiles(L.O, L.head);
    fine = true;
    for (int ct = 0; ct < tiles; ct++) {
        int c0, c1;
        dh_row_col_range(ct, L.O, L.head, &c0, &c1);
        fine = fine && c0 < c1 && c1 <= L.O && (ct == 0 ? c0 == 0 && c1 == L.head && c1 <= 32 : c1 - c0 <= DH_COLS && c0 >= L.head);
        for (int c = c0; c < c1 && c < L.O; c++) cols[(size_t)c] += 1;
    }
    for (unsigned char v : cols) fine = fine && v == 1;
    expect(fine, "the last layer's workgroups tile the columns, the head in the first");

    for (int K : {L.O, Hd}) {
        std::vector<unsigned char> terms((size_t)K, 0);
        const int S = dh_slabs(K);
        for (int s = 0; s < S; s++) {
            const int k0 = s * DH_SLAB, k1 = std::min(k0 + DH_SLAB, K);
            for (int kc = k0; kc < k1; kc += DH_KC) {
                const int len = std::min(k1 - kc, DH_KC);
                for (int w = 0; w < 4; w++)
                    for (int kk = w * 64; kk < w * 64 + 64 && kk < len; kk += 4)
                        for (int i = 0; i < 4; i++)
                            if (kk + i < len) terms[(size_t)(kc + kk + i)] += 1;
            }
        }
        fine = true;
        for (unsigned char v : terms) fine = fine && v == 1;
        expect(fine, "the slabs and the waves' shares tile the terms of a sum");
    }
    expect(dh_row_tiles(n) * DH_ROWS >= n && (dh_row_tiles(n) - 1) * DH_ROWS < n, "the row tiles");
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
    DhLayout L;
    auto sizes = [&](int n, int F, int Hd, int classes, int coeffs) { return dh_layout(n, F, Hd, classes, coeffs, &L, msg, sizeof(msg)); };
    expect(sizes(16, 512, 256, 8, 192) == 0 && L.O == 1552 && L.S3 == 13 && L.SH == 2, "the real widths: O = 1552, 13 and 2 slabs");
    expect(sizes(65535, 512, 256, 8, 192) == 0, "65535 objects");
    expect(sizes(1, 4, 4, 1, 1) == 0 && L.O == 10, "the smallest problem");
    expect(refused(sizes(0, 512, 256, 8, 192), msg, "n 0; 1 to 65535"), "n = 0");
    expect(refused(sizes(65536, 512, 256, 8, 192), msg, "n 65536"), "n = 65536");
    expect(refused(sizes(16, 510, 256, 8, 192), msg, "F 510; a positive multiple of 4"), "F % 4");
    expect(refused(sizes(16, 0, 256, 8, 192), msg, "F 0"), "F = 0");
    expect(refused(sizes(16, 512, 254, 8, 192), msg, "Hd 254; a positive multiple of 4"), "Hd % 4");
    expect(refused(sizes(16, 512, -4, 8, 192), msg, "Hd -4"), "Hd < 0");
    expect(refused(sizes(16, 512, 256, 0, 192), msg, "classes 0; 1 to 16"), "no class");
    expect(refused(sizes(16, 512, 256, 17, 192), msg, "classes 17; 1 to 16"), "17 classes");
    expect(refused(sizes(16, 512, 256, 8, 0), msg, "coeffs 0; at least 1"), "no coefficient");
    expect(refused(sizes(65535, 512, 256, 16, 1 << 20), msg, "n * O"), "n * O at 2^40");
    expect(refused(sizes(1, 512, 256, 16, 1 << 27), msg, "n * O"), "O at 2^31");
    expect(refused(sizes(8, 1 << 28, 4, 1, 1), msg, "n * F = 2147483648"), "n * F = 2^31");
    expect(refused(sizes(1, 4, 1 << 16, 16, 3000), msg, "O * Hd"), "O * Hd above 2^31");
    expect(refused(sizes(1, 1 << 20, 1 << 11, 1, 1), msg, "Hd * F = 2147483648"), "Hd * F = 2^31");
    expect(refused(sizes(1, 4, 1 << 16, 1, 1), msg, "Hd * (Hd + 4)"), "Hd * (Hd + 4) above 2^31");
    expect(refused(sizes(60000, 4, 4096, 16, 1), msg, "the workspace of"), "a workspace at 2^31 floats");
    expect(dh_layout(16, 512, 256, 8, 192, nullptr, msg, sizeof(msg)) == 1, "a NULL layout");

    const void* w[4] = {p, p, p, p};
    const void* hole[4] = {p, p, nullptr, p};
    const void* bent[4] = {p, four, p, p};
    auto fwd = [&](const void* pooled, const void* roi, const void* c, const void* e, const void* const* ws, const void* const* bs, const void* out,
                   const void* co, const void* eo, const void* row, const void* saved) {
        return dh_validate_fwd(pooled, roi, c, e, ws, bs, 16, 512, 256, 8, 192, out, co, eo, row, saved, &L, msg, sizeof(msg));
    };
    expect(fwd(p, p, nullptr, nullptr, w, w, p, p, p, nullptr, p) == 0, "roi_norms with centre_out and extent_out");
    expect(fwd(four, nullptr, four, four, w, w, four, nullptr, nullptr, four, four) == 0, "centre and extent as given, on 4 bytes");
    expect(refused(fwd(nullptr, p, nullptr, nullptr, w, w, p, p, p, nullptr, p), msg, "pooled is NULL"), "pooled NULL");
    expect(refused(fwd(p, p, p, p, w, w, p, p, p, nullptr, p), msg, "exactly one roi form"), "both roi forms");
    expect(refused(fwd(p, nullptr, nullptr, nullptr, w, w, p, nullptr, nullptr, nullptr, p), msg, "exactly one roi form"), "no roi form");
    expect(refused(fwd(p, nullptr, p, nullptr, w, w, p, nullptr, nullptr, nullptr, p), msg, "exactly one roi form"), "centre without extent");
    expect(refused(fwd(p, p, nullptr, nullptr, w, w, p, nullptr, p, nullptr, p), msg, "centre_out and extent_out go with roi_norms"), "no centre_out");
    expect(refused(fwd(p, nullptr, p, p, w, w, p, p, nullptr, nullptr, p), msg, "centre_out and extent_out go with roi_norms"), "a stray centre_out");
    expect(refused(fwd(p, p, nullptr, nullptr, hole, w, p, p, p, nullptr, p), msg, "w2 is NULL"), "a weight NULL");
    expect(refused(fwd(p, p, nullptr, nullptr, w, hole, p, p, p, nullptr, p), msg, "b2 is NULL"), "a bias NULL");
    expect(refused(fwd(p, p, nullptr, nullptr, bent, w, p, p, p, nullptr, p), msg, "w1 must be aligned to 16 bytes"), "a weight on 4 bytes");
    const void* bent_b[4] = {p, p, p, odd};
    expect(refused(fwd(p, p, nullptr, nullptr, w, bent_b, p, p, p, nullptr, p), msg, "b3 must be aligned to 4 bytes"), "a bias on 2 bytes");
    expect(refused(fwd(p, p, nullptr, nullptr, w, w, nullptr, p, p, nullptr, p), msg, "out or saved is NULL"), "out NULL");
    expect(refused(fwd(p, p, nullptr, nullptr, w, w, p, p, p, nullptr, nullptr), msg, "out or saved is NULL"), "saved NULL");
    expect(refused(fwd(odd, p, nullptr, nullptr, w, w, p, p, p, nullptr, p), msg, "aligned to 4 bytes"), "pooled on 2 bytes");
    expect(refused(fwd(p, p, nullptr, nullptr, w, w, p, p, p, odd, p), msg, "aligned to 4 bytes"), "row on 2 bytes");
    expect(refused(fwd(p, p, nullptr, nullptr, w, w, odd, p, p, nullptr, p), msg, "aligned to 4 bytes"), "out on 2 bytes");

    const size_t need = dh_workspace_bytes(L);
    const void* g[6] = {p, nullptr, four, nullptr, p, p};
    const void* none[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const void* all[9] = {p, p, p, p, p, p, p, p, p};
    const void* few[9] = {nullptr, nullptr, nullptr, four, nullptr, nullptr, nullptr, nullptr, p};
    auto bwd = [&](const void* const* gs, const void* pooled, const void* c, const void* e, const void* const* ws, const void* out,
                   const void* saved, const void* const* wanted, const void* space, size_t bytes) {
        return dh_validate_bwd(gs, pooled, c, e, ws, out, saved, 16, 512, 256, 8, 192, wanted, space, bytes, &L, msg, sizeof(msg));
    };
    expect(bwd(g, p, p, p, w, p, p, all, p, need) == 0, "a valid backward call");
    expect(bwd(none, p, p, p, bent, p, p, few, p, need + 1) == 0, "no output gradient, two input gradients, weights on 4 bytes");
    expect(refused(bwd(nullptr, p, p, p, w, p, p, all, p, need), msg, "the gradient lists are NULL"), "no gradient list");
    expect(refused(bwd(g, nullptr, p, p, w, p, p, all, p, need), msg, "pooled, centre or extent is NULL"), "pooled NULL");
    expect(refused(bwd(g, p, p, nullptr, w, p, p, all, p, need), msg, "pooled, centre or extent is NULL"), "extent NULL");
    expect(refused(bwd(g, p, p, p, hole, p, p, all, p, need), msg, "w2 is NULL"), "a weight NULL");
    expect(refused(bwd(g, p, p, p, w, nullptr, p, all, p, need), msg, "out or saved is NULL"), "out NULL");
    expect(refused(bwd(g, p, p, p, w, p, nullptr, all, p, need), msg, "out or saved is NULL"), "saved NULL");
    const void* g_odd[6] = {p, nullptr, odd, nullptr, p, p};
    const void* want_odd[9] = {p, p, p, p, odd, p, p, p, p};
    expect(refused(bwd(g_odd, p, p, p, w, p, p, all, p, need), msg, "output gradient 2 must be aligned to 4 bytes"), "a gradient on 2 bytes");
    expect(refused(bwd(g, p, p, p, w, p, p, want_odd, p, need), msg, "input gradient 4 must be aligned to 4 bytes"), "an input gradient on 2 bytes");
    expect(refused(bwd(g, p, odd, p, w, p, p, all, p, need), msg, "aligned to 4 bytes"), "centre on 2 bytes");
    expect(refused(bwd(g, p, p, p, w, p, p, all, nullptr, need), msg, "workspace is NULL"), "no workspace");
    expect(refused(bwd(g, p, p, p, w, p, p, all, four, need), msg, "workspace must be aligned to 16 bytes"), "a workspace on 4 bytes");
    expect(refused(bwd(g, p, p, p, w, p, p, all, p, need - 1), msg, "are needed"), "a workspace one byte short");
}

int main()
{
    for (int n : {1, 16, 17, 67}) walk_layout(n, 512, 256, 8, 192);
    walk_layout(19, 8, 4, 1, 3);
    walk_layout(19, 36, 20, 3, 24);
    walk_layout(19, 16, 8, 16, 3);
    walk_layout(3, 4, 132, 16, 1);
    std::printf("the layouts and the tilings: %d failures so far\n", failures);
    walk_validators();
    std::printf("the validators: %d failures so far\n", failures);
    std::printf("derender_heads_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
