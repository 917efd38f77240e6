// Host walk over the integer image, the keys, the sorting network, the scan's word assignment, the workspace layout and the validators
// of the proposal layer (3d-sdn_amd/csrc/proposal_layer_check.h):
//   - the image: over a ladder of floats (both infinities, both zeros, denormals, NaNs of either sign) it orders as the floats do, the
//     two zeros share one image, every NaN shares the largest one, and no image is 0;
//   - the keys: descending keys are descending images with the lower index first, the index comes back, no key is 0;
//   - the sorting network: for every size 1 .. 8192 every step's compare-exchanges touch every element exactly once and none outside,
//     and the network sorts random keys best first;
//   - the scan: for every word count 1 .. 128 and every word, the two words per lane reach every later word exactly once;
//   - the layout: the five ranges lie inside `total`, start on 16 bytes and share no byte;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/proposal_layer_check.cpp
//       -o /tmp/proposal_layer_check && /tmp/proposal_layer_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "proposal_layer_check.h"

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

static float float_of(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

static void walk_image()
{
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> ladder = {-inf, -3.0e38f, -2.5f, -1.0f, -1e-30f, -1e-45f, 0.0f, 1e-45f, 1e-38f, 1e-30f, 0.25f, 0.5f, 0.99999994f, 1.0f, 2.5f, 3.0e38f, inf};
    bool ok = true;
    for (size_t i = 0; i + 1 < ladder.size(); i++) ok = ok && prop_image(bits_of(ladder[i])) < prop_image(bits_of(ladder[i + 1]));
    expect(ok, "the image orders as the floats do");
    expect(prop_image(bits_of(-0.0f)) == prop_image(bits_of(0.0f)) && bits_of(-0.0f) != bits_of(0.0f), "both zeros share one image");
    const uint32_t nans[] = {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu};
    ok = true;
    for (uint32_t n : nans) ok = ok && std::isnan(float_of(n)) && prop_image(n) == 0xffffffffu && prop_image(n) > prop_image(bits_of(inf));
    expect(ok, "every NaN has the largest image");
    // neighbours in the float order stay neighbours in the image order, across the whole range (a stride walk over the bit patterns)
    ok = true;
    for (uint64_t u = 0; u < 0x7f800000ull && ok; u += 0x3fff1ull) {
        const uint32_t a = (uint32_t)u, b = a + 1;
        ok = prop_image(b) == prop_image(a) + 1 || a == 0;                                        // positive: ascending
        ok = ok && (a == 0 || prop_image(b | 0x80000000u) + 1 == prop_image(a | 0x80000000u));   // negative: descending
        ok = ok && prop_image(a) != 0 && prop_image(a | 0x80000000u) != 0;
    }
    expect(ok, "adjacent floats have adjacent images, none of them 0");
}

static void walk_keys()
{
    bool ok = true;
    const uint32_t images[] = {0x007fffffu, 0x80000000u, 0xbf000000u, 0xff800000u, 0xffffffffu};
    const uint32_t indices[] = {0u, 1u, 1023u, 1024u, (uint32_t)PROP_MAX_ANCHORS - 1u};
    for (uint32_t ia : images)
        for (uint32_t ib : images)
            for (uint32_t xa : indices)
                for (uint32_t xb : indices) {
                    const uint64_t a = prop_key(ia, xa), b = prop_key(ib, xb);
                    const bool first = ia > ib || (ia == ib && xa < xb);   // a comes before b in the result
                    ok = ok && (a > b) == first && a != 0 && prop_key_index(a) == xa;
                }
    expect(ok, "descending keys are descending images, lower index first");
}

static void walk_network()
{
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    for (int K = 1; K <= PROP_MAX_PRE_NMS; K = K < 70 ? K + 1 : K + K / 3 + 1) {
        const int N = prop_sort_size(K);
        bool ok = N >= K && N <= PROP_MAX_PRE_NMS && (N & (N - 1)) == 0 && (N == 1 || N / 2 < K);
        std::vector<uint64_t> s((size_t)N, 0ull), want;
        for (int i = 0; i < K; i++) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            s[(size_t)i] = prop_key((uint32_t)(seed >> 40) | 1u, (uint32_t)i);   // few distinct images: ties decided by the index
        }
        want.assign(s.begin(), s.begin() + K);
        std::sort(want.begin(), want.end(), [](uint64_t a, uint64_t b) { return a > b; });
        std::vector<unsigned char> seen((size_t)N);
        for (int k = 2; k <= N && ok; k <<= 1)
            for (int j = k >> 1; j > 0 && ok; j >>= 1) {
                std::fill(seen.begin(), seen.end(), 0);
                for (int t = 0; t < N / 2 && ok; t++) {
                    int i, l;
                    bool descending;
                    prop_bitonic_pair(t, j, k, &i, &l, &descending);
                    ok = i >= 0 && l == i + j && l < N;
                    if (!ok) break;
                    seen[(size_t)i]++;
                    seen[(size_t)l]++;
                    const uint64_t a = s[(size_t)i], b = s[(size_t)l];
                    if (descending ? a < b : a > b) {
                        s[(size_t)i] = b;
                        s[(size_t)l] = a;
                    }
                }
                for (int i = 0; i < N && ok; i++) ok = seen[(size_t)i] == 1;
            }
        for (int i = 0; i < K && ok; i++) ok = s[(size_t)i] == want[(size_t)i];
        for (int i = K; i < N && ok; i++) ok = s[(size_t)i] == 0ull;   // the padding sorts behind every key
        expect(ok, "the network touches every element once per step and sorts best first");
    }
}

static void walk_scan_words()
{
    bool ok = prop_words(1) == 1 && prop_words(64) == 1 && prop_words(65) == 2 && prop_words(PROP_MAX_PRE_NMS) == 128;
    for (int nb = 1; nb <= prop_words(PROP_MAX_PRE_NMS) && ok; nb++)
        for (int blk = 0; blk < nb && ok; blk++) {
            std::vector<unsigned char> seen((size_t)nb, 0);
            for (int lane = 0; lane < 64; lane++) {
                const int j0 = blk + 1 + lane, j1 = j0 + 64;   // nms_scan_words (nms_mask.h)
                if (j0 < nb) seen[(size_t)j0]++;
                if (j1 < nb) seen[(size_t)j1]++;
            }
            for (int j = 0; j < nb && ok; j++) ok = seen[(size_t)j] == (j > blk ? 1 : 0);
        }
    expect(ok, "two words per lane reach every later word exactly once");
}

static void walk_layout(int A, int K, int P)
{
    char msg[256];
    PropLayout L;
    bool ok = prop_layout(A, K, P, &L, msg, sizeof(msg)) == 0;
    std::vector<unsigned char> buf(ok ? L.total : 0, 0);   // real memory, so that ASan sees a range that leaves it
    if (ok) {
        const size_t at[5] = {L.head, L.ties, L.keys, L.areas, L.mask};
        const size_t len[5] = {sizeof(int32_t) * (size_t)PROP_HEAD_INTS, sizeof(int32_t) * (size_t)prop_chunks(A), sizeof(uint64_t) * (size_t)K,
                               sizeof(float) * (size_t)K, sizeof(uint64_t) * (size_t)K * (size_t)prop_words(K)};
        size_t used = 0;
        for (int r = 0; r < 5 && ok; r++) {
            ok = at[r] % PROP_ALIGN == 0 && at[r] + len[r] <= L.total && (r == 0 ? at[r] == 0 : at[r] >= at[r - 1] + len[r - 1]);
            for (size_t i = 0; i < len[r] && ok; i++) buf[at[r] + i] += 1;
            used += len[r];
        }
        size_t once = 0;
        for (size_t i = 0; i < buf.size() && ok; i++) {
            ok = buf[i] <= 1;
            once += buf[i];
        }
        ok = ok && once == used && L.total - used < 5 * (size_t)PROP_ALIGN && L.total % PROP_ALIGN == 0;
        ok = ok && (size_t)prop_chunks(A) * PROP_CHUNK >= (size_t)A && ((size_t)prop_chunks(A) - 1) * PROP_CHUNK < (size_t)A;
    }
    expect(ok, "the five ranges tile the workspace");
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
    const float std_dev[4] = {0.1f, 0.1f, 0.2f, 0.2f};
    PropLayout L;
    expect(prop_layout(261888, 6000, 2000, &L, msg, sizeof(msg)) == 0 && L.total > 0, "the reference's size has a layout");
    const size_t big = L.total;
    auto call = [&](const void* probs, const void* bbox, const void* anchors, int A, const float* sd, int h, int w, int K, int P, const void* order,
                    const void* boxes, const void* keep, const void* count, const void* rois, const void* ws, size_t bytes) {
        return prop_validate(probs, bbox, anchors, A, sd, h, w, K, P, order, boxes, keep, count, rois, ws, bytes, msg, sizeof(msg));
    };
    expect(call(p, p, p, 261888, std_dev, 1024, 1024, 6000, 2000, p, p, p, p, p, p, big) == 0, "a valid call passes");
    expect(call(four, four, four, 1, std_dev, 1, 1, 1, 1, four, p, four, four, p, p, big) == 0, "the smallest call passes, inputs on 4 bytes");
    expect(call(p, p, p, PROP_MAX_ANCHORS - 1, std_dev, 8, 8, PROP_MAX_PRE_NMS, PROP_MAX_PRE_NMS, p, p, p, p, p, p, (size_t)64 << 20) == 0, "the largest call passes");
    expect(refused(call(p, p, p, 0, std_dev, 8, 8, 1, 1, p, p, p, p, p, p, big), msg, "A 0 (no anchors)"), "A = 0");
    expect(refused(call(p, p, p, -5, std_dev, 8, 8, 1, 1, p, p, p, p, p, p, big), msg, "A -5"), "A < 0");
    expect(refused(call(p, p, p, PROP_MAX_ANCHORS, std_dev, 8, 8, 1, 1, p, p, p, p, p, p, big), msg, "fewer than 2^24"), "A = 2^24");
    expect(refused(call(p, p, p, std::numeric_limits<int>::max(), std_dev, 8, 8, 1, 1, p, p, p, p, p, p, big), msg, "fewer than 2^24"), "A = INT_MAX");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 0, 1, p, p, p, p, p, p, big), msg, "K 0; 1 to 8192"), "K = 0");
    expect(refused(call(p, p, p, 100000, std_dev, 8, 8, 8193, 1, p, p, p, p, p, p, big), msg, "K 8193; 1 to 8192"), "K = 8193");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 101, 1, p, p, p, p, p, p, big), msg, "K 101 exceeds A 100"), "K > A");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 0, p, p, p, p, p, p, big), msg, "P 0; 1 to 8192"), "P = 0");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 8193, p, p, p, p, p, p, big), msg, "P 8193"), "P = 8193");
    expect(refused(call(p, p, p, 100, std_dev, 0, 8, 10, 5, p, p, p, p, p, p, big), msg, "image 0 x 8"), "height 0");
    expect(refused(call(p, p, p, 100, std_dev, 8, -1, 10, 5, p, p, p, p, p, p, big), msg, "image 8 x -1"), "width < 0");
    expect(refused(call(p, p, p, 100, nullptr, 8, 8, 10, 5, p, p, p, p, p, p, big), msg, "std_dev is NULL"), "std_dev");
    expect(refused(call(nullptr, p, p, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, p, big), msg, "rpn_probs, rpn_bbox or anchors is NULL"), "probs NULL");
    expect(refused(call(p, p, nullptr, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, p, big), msg, "rpn_probs, rpn_bbox or anchors is NULL"), "anchors NULL");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, p, nullptr, p, p, p, big), msg, "keep, count or rois is NULL"), "keep NULL");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, nullptr, big), msg, "workspace is NULL"), "workspace NULL");
    expect(prop_layout(100, 10, 5, &L, msg, sizeof(msg)) == 0, "a small layout");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, p, L.total - 1), msg, "workspace"), "workspace one byte short");
    expect(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, p, L.total) == 0, "workspace exactly enough");
    expect(refused(call(p, odd, p, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, p, big), msg, "aligned to 4 bytes"), "rpn_bbox on 2 bytes");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, p, p, odd, p, p, big), msg, "aligned to 4 bytes"), "count on 2 bytes");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, four, p, p, p, p, big), msg, "aligned to 16 bytes"), "boxes_px on 4 bytes");
    expect(refused(call(p, p, p, 100, std_dev, 8, 8, 10, 5, p, p, p, p, p, four, big), msg, "aligned to 16 bytes"), "workspace on 4 bytes");
    expect(prop_layout(100, 10, 5, nullptr, msg, sizeof(msg)) == 1, "a NULL layout");
}

int main()
{
    walk_image();
    walk_keys();
    std::printf("the image and the keys: %d failures so far\n", failures);
    walk_network();
    walk_scan_words();
    std::printf("the sorting network and the scan's words: %d failures so far\n", failures);
    const int sizes[][3] = {{1, 1, 1}, {37, 37, 10}, {1024, 100, 20}, {1025, 300, 50}, {2049, 63, 30}, {2049, 64, 64}, {2049, 65, 8192},
                            {16368, 2048, 1000}, {261888, 6000, 2000}, {PROP_MAX_ANCHORS - 1, PROP_MAX_PRE_NMS, PROP_MAX_PRE_NMS}};
    for (const auto& s : sizes) walk_layout(s[0], s[1], s[2]);
    std::printf("the layout: %d failures so far\n", failures);
    walk_validators();
    std::printf("the validators: %d failures so far\n", failures);
    std::printf("proposal_layer_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
