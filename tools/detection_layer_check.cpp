// Host walk over the workspace layout and the validators of the detection layer (3d-sdn_amd/csrc/detection_layer_check.h; the image,
// the keys and the sorting network it takes from proposal_layer_check.h are walked by tools/proposal_layer_check.cpp):
//   - the keys of the rows: over N = 8192 rows the key of a valid row is never 0, so key 0 (a row that is no detection) sorts behind
//     every valid row, and among equal scores the lower row comes first;
//   - the arg-max: over rows of few distinct values, NaNs of either sign, infinities and both zeros, for C = 1 .. 200, the merge of
//     eight lanes' walks over every eighth class (k_det_rows) gives the first index of the maximum as one walk over all classes
//     does, a NaN counting as the maximum and the first NaN winning;
//   - the scan: for every valid count M the word count ceil(M / 64) stays within the mask's row stride ceil(N / 64) <= 128;
//   - the layout: the seven ranges lie inside `total`, start on 16 bytes and share no byte;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/detection_layer_check.cpp
//       -o /tmp/detection_layer_check && /tmp/detection_layer_check
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "detection_layer_check.h"

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

static void walk_keys()
{
    const float scores[] = {0.0f, 1e-45f, 0.3f, 0.7f, 0.99999994f, 1.0f, std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::quiet_NaN()};
    bool ok = true;
    std::vector<uint64_t> keys;
    for (float s : scores)
        for (uint32_t row : {0u, 1u, 63u, 64u, (uint32_t)DET_MAX_ROIS - 1u}) {
            const uint64_t k = prop_key(prop_image(bits_of(s)), row);
            ok = ok && k != 0ull && prop_key_index(k) == row;
            keys.push_back(k);
        }
    expect(ok, "no valid row has key 0 and the row comes back");
    keys.push_back(0ull);
    keys.push_back(0ull);
    std::vector<uint64_t> sorted = keys;
    std::sort(sorted.begin(), sorted.end(), [](uint64_t a, uint64_t b) { return a > b; });
    ok = sorted[sorted.size() - 1] == 0ull && sorted[sorted.size() - 2] == 0ull && sorted[sorted.size() - 3] != 0ull;
    for (size_t i = 0; i + 3 < sorted.size(); i++) {
        const uint32_t ia = (uint32_t)(sorted[i] >> 32), ib = (uint32_t)(sorted[i + 1] >> 32);
        ok = ok && (ia > ib || (ia == ib && prop_key_index(sorted[i]) < prop_key_index(sorted[i + 1])));
    }
    expect(ok, "key 0 sorts behind every row; equal scores put the lower row first");
}

static void walk_argmax()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float values[] = {0.0f, -0.0f, 0.25f, 0.25f, 0.5f, 0.5f, 0.75f, -1.0f, inf, -inf, nan, -nan};
    uint64_t seed = 0x2545f4914f6cdd1dull;
    bool ok = true;
    for (int C = 1; C <= 200 && ok; C++)
        for (int trial = 0; trial < 40 && ok; trial++) {
            const int kinds = trial < 10 ? 4 : (trial < 20 ? 8 : 12);   // no special values, then infinities, then NaNs
            std::vector<float> p((size_t)C);
            for (float& v : p) {
                seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                v = values[(seed >> 33) % (uint64_t)kinds];
            }
            if (trial == 39) std::fill(p.begin(), p.end(), -inf);
            if (trial == 38) std::fill(p.begin(), p.end(), nan);
            // torch.max on the CPU: the first element, then a later one only if it is greater or the first NaN
            float want = p[0];
            int at = 0;
            for (int c = 1; c < C; c++)
                if (!std::isnan(want) && (p[(size_t)c] > want || std::isnan(p[(size_t)c]))) {
                    want = p[(size_t)c];
                    at = c;
                }
            float score[DET_ROW_LANES];
            int cls[DET_ROW_LANES];
            for (int sub = 0; sub < DET_ROW_LANES; sub++) {
                score[sub] = -inf;
                cls[sub] = INT_MAX;
                for (int c = sub; c < C; c += DET_ROW_LANES)
                    if (det_argmax_takes(score[sub], cls[sub], p[(size_t)c], c)) {
                        score[sub] = p[(size_t)c];
                        cls[sub] = c;
                    }
            }
            for (int m = 1; m < DET_ROW_LANES; m <<= 1) {   // the exchange with lane sub ^ m, all lanes at once
                float s2[DET_ROW_LANES];
                int c2[DET_ROW_LANES];
                for (int sub = 0; sub < DET_ROW_LANES; sub++) {
                    const bool take = det_argmax_takes(score[sub], cls[sub], score[sub ^ m], cls[sub ^ m]);
                    s2[sub] = take ? score[sub ^ m] : score[sub];
                    c2[sub] = take ? cls[sub ^ m] : cls[sub];
                }
                std::copy(s2, s2 + DET_ROW_LANES, score);
                std::copy(c2, c2 + DET_ROW_LANES, cls);
            }
            for (int sub = 0; sub < DET_ROW_LANES && ok; sub++)
                ok = cls[sub] == at && bits_of(score[sub]) == bits_of(want);
        }
    expect(ok, "eight lanes' walks merged give torch.max's first index and its element");
    expect((DET_ROW_LANES & (DET_ROW_LANES - 1)) == 0 && 64 % DET_ROW_LANES == 0 && DET_ROWS_PER_WAVE * DET_ROW_LANES == DET_ROW_THREADS,
           "a row's lanes are a power of two inside one wave");
}

static void walk_words()
{
    bool ok = DET_MAX_WORDS == prop_words(DET_MAX_ROIS) && DET_MAX_WORDS == 128 && prop_sort_size(DET_MAX_ROIS) == DET_MAX_ROIS;
    ok = ok && sizeof(uint64_t) * (size_t)DET_MAX_ROIS <= 64u * 1024u && DET_SORT_THREADS <= 1024 && DET_ROW_THREADS % 64 == 0;
    for (int N = 1; N <= DET_MAX_ROIS && ok; N = N < 200 ? N + 1 : N + N / 5)
        for (int M = 0; M <= N && ok; M = M < 200 ? M + 1 : M + M / 7) ok = prop_words(M) <= prop_words(N) && prop_words(N) <= DET_MAX_WORDS;
    expect(ok, "the scan's words stay inside the mask's rows");
}

static void walk_layout(int N, int C, int D)
{
    char msg[256];
    DetLayout L;
    bool ok = det_layout(N, C, D, &L, msg, sizeof(msg)) == 0;
    std::vector<unsigned char> buf(ok ? L.total : 0, 0);   // real memory, so that ASan sees a range that leaves it
    if (ok) {
        const int R = 7;
        const size_t at[R] = {L.head, L.keys, L.boxes, L.areas, L.classes, L.rows, L.mask};
        const size_t n = (size_t)N;
        const size_t len[R] = {sizeof(int32_t) * (size_t)DET_HEAD_INTS, sizeof(uint64_t) * n, 4 * sizeof(float) * n, sizeof(float) * n,
                               sizeof(int32_t) * n, sizeof(int32_t) * n, sizeof(uint64_t) * n * (size_t)prop_words(N)};
        size_t used = 0;
        for (int r = 0; r < R && ok; r++) {
            ok = at[r] % PROP_ALIGN == 0 && at[r] + len[r] <= L.total && (r == 0 ? at[r] == 0 : at[r] >= at[r - 1] + len[r - 1]);
            for (size_t i = 0; i < len[r] && ok; i++) buf[at[r] + i] += 1;
            used += len[r];
        }
        size_t once = 0;
        for (size_t i = 0; i < buf.size() && ok; i++) {
            ok = buf[i] <= 1;
            once += buf[i];
        }
        ok = ok && once == used && L.total - used < R * (size_t)PROP_ALIGN && L.total % PROP_ALIGN == 0;
    }
    expect(ok, "the seven ranges tile the workspace");
}

static bool refused(int rc, const char* msg, const char* reason)
{
    const bool ok = rc == 1 && std::strstr(msg, reason) != nullptr;
    if (!ok) std::printf("  rc %d, message \"%s\", wanted \"%s\"\n", rc, msg, reason);
    return ok;
}

struct Call {
    const void *rois, *probs, *deltas;
    int N, C;
    const float *window, *std_dev;
    int height, width, D;
    const void *roi_count, *class_ids, *scores, *boxes_px, *keep, *count, *detections, *boxes_norm, *ws;
    size_t bytes;
};

static void walk_validators()
{
    char msg[256] = "";
    alignas(16) static unsigned char mem[64];
    const void* p = mem;
    const void* odd = mem + 2;
    const void* four = mem + 4;
    const float std_dev[4] = {0.1f, 0.1f, 0.2f, 0.2f};
    const float window[4] = {128.0f, 0.0f, 896.0f, 1024.0f};
    DetLayout L;
    expect(det_layout(1000, 81, 100, &L, msg, sizeof(msg)) == 0 && L.total > 0, "the reference's size has a layout");
    const size_t big = (size_t)16 << 20;
    const Call good = {p, p, p, 1000, 81, window, std_dev, 1024, 1024, 100, nullptr, p, p, p, p, p, p, p, p, big};
    auto run = [&](const Call& c) {
        return det_validate(c.rois, c.probs, c.deltas, c.N, c.C, c.window, c.std_dev, c.height, c.width, c.D, c.roi_count, c.class_ids, c.scores,
                            c.boxes_px, c.keep, c.count, c.detections, c.boxes_norm, c.ws, c.bytes, msg, sizeof(msg));
    };
    auto with = [&](auto change) {
        Call c = good;
        change(c);
        return run(c);
    };
    expect(run(good) == 0, "a valid call passes");
    expect(with([&](Call& c) { c.roi_count = four; }) == 0, "a valid call with roi_count passes");
    expect(with([&](Call& c) { c.N = c.C = c.D = c.height = c.width = 1; c.rois = c.probs = c.deltas = c.class_ids = c.scores = c.keep = c.count = c.detections = four; }) == 0,
           "the smallest call passes, inputs on 4 bytes");
    expect(with([&](Call& c) { c.N = DET_MAX_ROIS; c.D = DET_MAX_INSTANCES; c.C = 1 << 20; }) == 0, "the largest call passes");
    expect(refused(with([&](Call& c) { c.N = 0; }), msg, "N 0; 1 to 8192"), "N = 0");
    expect(refused(with([&](Call& c) { c.N = -7; }), msg, "N -7; 1 to 8192"), "N < 0");
    expect(refused(with([&](Call& c) { c.N = 8193; }), msg, "N 8193; 1 to 8192"), "N = 8193");
    expect(refused(with([&](Call& c) { c.N = std::numeric_limits<int>::max(); }), msg, "1 to 8192"), "N = INT_MAX");
    expect(refused(with([&](Call& c) { c.C = 0; }), msg, "C 0 (no classes)"), "C = 0");
    expect(refused(with([&](Call& c) { c.C = -1; }), msg, "C -1"), "C < 0");
    expect(refused(with([&](Call& c) { c.D = 0; }), msg, "D 0; 1 to 8192"), "D = 0");
    expect(refused(with([&](Call& c) { c.D = 8193; }), msg, "D 8193; 1 to 8192"), "D = 8193");
    expect(refused(with([&](Call& c) { c.height = 0; }), msg, "image 0 x 1024"), "height 0");
    expect(refused(with([&](Call& c) { c.width = -1; }), msg, "image 1024 x -1"), "width < 0");
    expect(refused(with([&](Call& c) { c.window = nullptr; }), msg, "window is NULL"), "window");
    expect(refused(with([&](Call& c) { c.std_dev = nullptr; }), msg, "std_dev is NULL"), "std_dev");
    expect(refused(with([&](Call& c) { c.rois = nullptr; }), msg, "rois, probs or deltas is NULL"), "rois NULL");
    expect(refused(with([&](Call& c) { c.probs = nullptr; }), msg, "rois, probs or deltas is NULL"), "probs NULL");
    expect(refused(with([&](Call& c) { c.deltas = nullptr; }), msg, "rois, probs or deltas is NULL"), "deltas NULL");
    expect(refused(with([&](Call& c) { c.class_ids = nullptr; }), msg, "class_ids, scores or boxes_px is NULL"), "class_ids NULL");
    expect(refused(with([&](Call& c) { c.scores = nullptr; }), msg, "class_ids, scores or boxes_px is NULL"), "scores NULL");
    expect(refused(with([&](Call& c) { c.boxes_px = nullptr; }), msg, "class_ids, scores or boxes_px is NULL"), "boxes_px NULL");
    expect(refused(with([&](Call& c) { c.keep = nullptr; }), msg, "keep, count, detections or boxes_norm is NULL"), "keep NULL");
    expect(refused(with([&](Call& c) { c.count = nullptr; }), msg, "keep, count, detections or boxes_norm is NULL"), "count NULL");
    expect(refused(with([&](Call& c) { c.detections = nullptr; }), msg, "keep, count, detections or boxes_norm is NULL"), "detections NULL");
    expect(refused(with([&](Call& c) { c.boxes_norm = nullptr; }), msg, "keep, count, detections or boxes_norm is NULL"), "boxes_norm NULL");
    expect(refused(with([&](Call& c) { c.ws = nullptr; }), msg, "workspace is NULL"), "workspace NULL");
    expect(refused(with([&](Call& c) { c.bytes = L.total - 1; }), msg, "workspace"), "workspace one byte short");
    expect(with([&](Call& c) { c.bytes = L.total; }) == 0, "workspace exactly enough");
    expect(refused(with([&](Call& c) { c.probs = odd; }), msg, "rois, probs and deltas must be aligned to 4 bytes"), "probs on 2 bytes");
    expect(refused(with([&](Call& c) { c.roi_count = odd; }), msg, "roi_count must be aligned to 4 bytes"), "roi_count on 2 bytes");
    expect(refused(with([&](Call& c) { c.count = odd; }), msg, "detections must be aligned to 4 bytes"), "count on 2 bytes");
    expect(refused(with([&](Call& c) { c.detections = odd; }), msg, "detections must be aligned to 4 bytes"), "detections on 2 bytes");
    expect(refused(with([&](Call& c) { c.boxes_px = four; }), msg, "aligned to 16 bytes"), "boxes_px on 4 bytes");
    expect(refused(with([&](Call& c) { c.boxes_norm = four; }), msg, "aligned to 16 bytes"), "boxes_norm on 4 bytes");
    expect(refused(with([&](Call& c) { c.ws = four; }), msg, "aligned to 16 bytes"), "workspace on 4 bytes");
    expect(det_layout(100, 3, 5, nullptr, msg, sizeof(msg)) == 1, "a NULL layout");
}

int main()
{
    walk_keys();
    walk_argmax();
    walk_words();
    std::printf("the keys, the arg-max and the scan's words: %d failures so far\n", failures);
    const int sizes[][3] = {{1, 1, 1}, {1, 2, 3}, {63, 3, 30}, {64, 3, 30}, {65, 3, 30}, {1000, 3, 100}, {1000, 81, 100}, {4097, 7, 8192},
                            {DET_MAX_ROIS, 81, DET_MAX_INSTANCES}};
    for (const auto& s : sizes) walk_layout(s[0], s[1], s[2]);
    std::printf("the layout: %d failures so far\n", failures);
    walk_validators();
    std::printf("the validators: %d failures so far\n", failures);
    std::printf("detection_layer_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
