// Host walk over the bin and tap arithmetic and the validators of the pyramid pooling module (3d-sdn_amd/csrc/segm_ppm_check.h):
//   - for h, w in 1 .. 20 and s in 1 .. 8: the bins are torch's (floor / ceil in exact integers), none is empty, every position
//     is covered, the areas add up; the covering range of every position, in closed form, is exactly the set of bins that hold it
//     (more than two when n < s); the transposed sum over covering bins equals the forward sum over bins;
//   - for n in 1 .. 400 and s in 1 .. 8: the taps stay inside the map, the two weights add to 1, and the column range of a tap
//     (k_ppm_fill_bwd) holds every position with a weight on it;
//   - the tiles of k_ppm_pool: every (row, column bin) and every bin has a thread, the tile and the sums stay inside their arrays;
//   - the pooled buffer's segments tile it; the validators: valid calls and one refused call per reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/segm_ppm_check.cpp \
//       -o /tmp/segm_ppm_check && /tmp/segm_ppm_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "segm_ppm_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static long walked_bins = 0, walked_taps = 0;

static void walk_bins(int n, int s)
{
    std::vector<int> count(n, 0);
    bool ok = true;
    for (int i = 0; i < s; i++) {
        const int a = ppm_bin_start(i, n, s), b = ppm_bin_end(i, n, s);
        ok = ok && a == (int)std::floor((double)i * n / s) && b == (int)std::ceil((double)(i + 1) * n / s);
        ok = ok && a >= 0 && b <= n && b > a;
        for (int y = a; y < b && ok; y++) count[y]++;
        walked_bins++;
    }
    ok = ok && ppm_bin_start(0, n, s) == 0 && ppm_bin_end(s - 1, n, s) == n;
    for (int y = 0; y < n && ok; y++) {
        int lo, hi;
        ppm_cover(y, n, s, &lo, &hi);
        ok = lo >= 0 && hi < s && lo <= hi && hi - lo + 1 == count[y] && count[y] >= 1;
        for (int i = 0; i < s && ok; i++) {
            const bool holds = ppm_bin_start(i, n, s) <= y && y < ppm_bin_end(i, n, s);
            ok = holds == (i >= lo && i <= hi);
        }
        if (n >= s) ok = ok && count[y] <= 2;
    }
    if (n == 1) {
        int lo, hi;
        ppm_cover(0, 1, s, &lo, &hi);
        ok = ok && lo == 0 && hi == s - 1;
    }
    if (!ok) {
        if (failures < 20) std::printf("bins: n %d, s %d  FAIL\n", n, s);
        failures++;
    }
}

// forward and backward agree on a plane: sum_bins g[bin] * mean(x over bin) == sum_pixels x * (sum over covering bins g / area)
static void walk_plane(int h, int w, int s)
{
    std::vector<double> x((size_t)h * w), g((size_t)s * s);
    for (size_t i = 0; i < x.size(); i++) x[i] = (double)((i * 37 + 11) % 23) - 11.0;
    for (size_t i = 0; i < g.size(); i++) g[i] = (double)((i * 13 + 5) % 17) - 8.0;
    double fwd = 0.0, bwd = 0.0;
    long area_sum = 0;
    for (int i = 0; i < s; i++)
        for (int j = 0; j < s; j++) {
            const int r0 = ppm_bin_start(i, h, s), r1 = ppm_bin_end(i, h, s), c0 = ppm_bin_start(j, w, s), c1 = ppm_bin_end(j, w, s);
            double sum = 0.0;
            for (int y = r0; y < r1; y++)
                for (int c = c0; c < c1; c++) sum += x[(size_t)y * w + c];
            area_sum += (long)(r1 - r0) * (c1 - c0);
            fwd += g[(size_t)i * s + j] * sum / ((r1 - r0) * (c1 - c0));
        }
    long cover_sum = 0;
    for (int y = 0; y < h; y++)
        for (int c = 0; c < w; c++) {
            int ilo, ihi, jlo, jhi;
            ppm_cover(y, h, s, &ilo, &ihi);
            ppm_cover(c, w, s, &jlo, &jhi);
            double v = 0.0;
            for (int i = ilo; i <= ihi; i++)
                for (int j = jlo; j <= jhi; j++) {
                    const int area = (ppm_bin_end(i, h, s) - ppm_bin_start(i, h, s)) * (ppm_bin_end(j, w, s) - ppm_bin_start(j, w, s));
                    v += g[(size_t)i * s + j] / area;
                    cover_sum++;
                }
            bwd += x[(size_t)y * w + c] * v;
        }
    if (area_sum != cover_sum || std::fabs(fwd - bwd) > 1e-9 * (1.0 + std::fabs(fwd))) {
        if (failures < 20) std::printf("plane %d x %d, s %d: forward %.17g, transposed %.17g, areas %ld / %ld  FAIL\n", h, w, s, fwd, bwd, area_sum, cover_sum);
        failures++;
    }
}

static void walk_taps(int n, int s)
{
    const float scale = (float)s / (float)n;
    bool ok = true;
    std::vector<int> lo(s), hi(s);
    for (int j = 0; j < s; j++) {
        ppm_tap_range(j, n, s, &lo[j], &hi[j]);
        ok = ok && lo[j] >= 0 && hi[j] <= n && lo[j] <= hi[j];
    }
    int last = 0;
    for (int o = 0; o < n && ok; o++) {
        int i0, i1;
        float lam;
        ppm_taps(scale, o, s, &i0, &i1, &lam);
        ok = i0 >= 0 && i0 < s && i1 >= i0 && i1 < s && i1 <= i0 + 1 && lam >= 0.f && lam < 1.f && i0 >= last;
        last = i0;
        float sum = 0.f;
        for (int j = 0; j < s && ok; j++) {
            const float wt = ppm_tap_weight(scale, o, s, j);
            sum += wt;
            if (wt != 0.f) ok = o >= lo[j] && o < hi[j];     // the range holds every position that weighs on the tap
            if (j != i0 && j != i1) ok = ok && wt == 0.f;
        }
        ok = ok && sum == 1.f;
        walked_taps++;
    }
    if (n == s)   // the identity: every position is its own tap
        for (int o = 0; o < n && ok; o++) ok = ppm_tap_weight(scale, o, s, o) == 1.f;
    if (!ok) {
        if (failures < 20) std::printf("taps: n %d, s %d  FAIL\n", n, s);
        failures++;
    }
}

// the threads and the LDS arrays of k_ppm_pool / k_ppm_fill_bwd for a set of scales and a plane
static void walk_tiles(const int* scales, int S, int h, int w)
{
    PpmPlan P;
    ppm_plan_make(scales, nullptr, S, &P);
    const int NB = P.cb[PPM_MAX_SCALES], NBINS = P.bb[PPM_MAX_SCALES], R = ppm_pool_rows(NB);
    std::vector<unsigned char> tile((size_t)PPM_TILE_ROWS * PPM_TILE_PITCH, 0), colsum((size_t)PPM_TILE_ROWS * PPM_MAX_COLBINS, 0);
    bool ok = R >= 1 && R <= PPM_TILE_ROWS && R * NB <= PPM_THREADS && NBINS <= PPM_THREADS && NB <= PPM_MAX_COLBINS;
    long staged = 0;
    for (int r0 = 0; r0 < h && ok; r0 += R) {
        const int rows = R < h - r0 ? R : h - r0;
        for (int c0 = 0; c0 < w && ok; c0 += PPM_TILE_COLS) {
            const int cols = PPM_TILE_COLS < w - c0 ? PPM_TILE_COLS : w - c0;
            for (int rr = 0; rr < rows; rr++)
                for (int cc = 0; cc < cols; cc++) tile.at((size_t)rr * PPM_TILE_PITCH + cc) = 1;   // at(): inside the array
            staged += (long)rows * cols;
            for (int t = 0; t < R * NB; t++) {
                const int sr = t / NB, sq = t - sr * NB;
                colsum.at((size_t)sr * PPM_MAX_COLBINS + sq) = 1;
            }
        }
    }
    ok = ok && staged == (long)h * w;
    // the pooled buffer: the segments of the branches follow one another
    const int B = 2, C = 3;
    long at = 0;
    for (int k = 0; k < S; k++) {
        ok = ok && (long)B * C * P.bb[k] == at;
        at += (long)B * C * scales[k] * scales[k];
    }
    ok = ok && at == ppm_pooled_floats(B, C, NBINS);
    if (!ok) {
        if (failures < 20) std::printf("tiles: S %d, first scale %d, plane %d x %d  FAIL\n", S, scales[0], h, w);
        failures++;
    }
}

static bool refused(int rc, const char* msg, const char* reason)
{
    return rc == 1 && std::strstr(msg, reason) != nullptr;
}

int main()
{
    for (int s = 1; s <= PPM_MAX_SIDE; s++) {
        for (int n = 1; n <= 20; n++) walk_bins(n, s);
        for (int n : {47, 156, 157, 1000, 46340, 2147483647}) {
            // large sizes: the closed forms stay inside 64 bits; every bin non-empty, the ends meet the plane
            bool ok = ppm_bin_start(0, n, s) == 0 && ppm_bin_end(s - 1, n, s) == n;
            for (int i = 0; i < s; i++) ok = ok && ppm_bin_end(i, n, s) > ppm_bin_start(i, n, s);
            int lo, hi;
            ppm_cover(n - 1, n, s, &lo, &hi);
            ok = ok && hi == s - 1 && lo <= hi;
            ppm_cover(0, n, s, &lo, &hi);
            ok = ok && lo == 0;
            expect(ok, "bins of a large side");
        }
        for (int h = 1; h <= 20; h++)
            for (int w = 1; w <= 20; w++) walk_plane(h, w, s);
        for (int n = 1; n <= 400; n++) walk_taps(n, s);
        for (int n : {1000, 4096, 16384, 100003}) walk_taps(n, s);
    }
    const int ref[4] = {1, 2, 3, 6}, big[4] = {8, 8, 8, 8}, one[1] = {1}, two[2] = {1, 8};
    for (int h : {1, 5, 16, 17, 47})
        for (int w : {1, 3, 156, 256, 257, 600}) {
            walk_tiles(ref, 4, h, w);
            walk_tiles(big, 4, h, w);
            walk_tiles(one, 1, h, w);
            walk_tiles(two, 2, h, w);
        }

    char msg[256];
    alignas(16) static char mem[64];
    const void* p = mem;
    const float* fp = reinterpret_cast<const float*>(mem);
    float* fpm = reinterpret_cast<float*>(mem);
    const int K[4] = {512, 512, 512, 512}, K0[4] = {4, 0, 4, 4}, s9[4] = {1, 2, 3, 9}, s0[4] = {0, 2, 3, 6};
    const float* ys[4] = {fp, fp, fp, fp};
    const float* ys_null[4] = {fp, nullptr, fp, fp};
    const float* ys_odd[4] = {fp, reinterpret_cast<const float*>(mem + 2), fp, fp};
    float* gys[4] = {nullptr, fpm, nullptr, nullptr};
    float* gys_none[4] = {nullptr, nullptr, nullptr, nullptr};
    const float* gps[4] = {nullptr, nullptr, fp, nullptr};
    const float* gps_none[4] = {nullptr, nullptr, nullptr, nullptr};
    int ct = 0;
    // valid calls
    expect(ppm_validate_sizes(ref, K, 4, 2, 2048, 47, 156, &ct, msg, sizeof(msg)) == 0 && ct == 4096, "the decoder's size");
    expect(ppm_validate_sizes(two, K, 2, 1, 1, 1, 1, &ct, msg, sizeof(msg)) == 0 && ct == 1025, "one pixel, two branches");
    expect(ppm_validate_pool(p, p, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)) == 0, "a valid pool call");
    expect(ppm_validate_fill(ys, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)) == 0, "a valid fill call");
    expect(ppm_validate_fill_bwd(p, gys, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)) == 0, "a valid fill_bwd call, one branch");
    expect(ppm_validate_pool_bwd(p, nullptr, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)) == 0, "pool_bwd with grad_cat alone");
    expect(ppm_validate_pool_bwd(nullptr, gps, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)) == 0, "pool_bwd with one grad_p alone");
    // refusals
    expect(refused(ppm_validate_sizes(ref, K, 0, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "0 scales"), "S = 0");
    expect(refused(ppm_validate_sizes(ref, K, 5, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "5 scales"), "S = 5");
    expect(refused(ppm_validate_sizes(nullptr, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "scales is NULL"), "null scales");
    expect(refused(ppm_validate_sizes(ref, nullptr, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "branch_channels is NULL"), "null K");
    expect(refused(ppm_validate_sizes(s9, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "scale 3 is 9"), "scale 9");
    expect(refused(ppm_validate_sizes(s0, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "scale 0 is 0"), "scale 0");
    expect(refused(ppm_validate_sizes(ref, K0, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "branch 1 has 0"), "K = 0");
    expect(refused(ppm_validate_sizes(ref, K, 4, 0, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "bad sizes"), "B = 0");
    expect(refused(ppm_validate_sizes(ref, K, 4, 2, 8, -7, 13, &ct, msg, sizeof(msg)), msg, "bad sizes"), "h < 0");
    expect(refused(ppm_validate_sizes(ref, K, 4, 2, 2048, 512, 512, &ct, msg, sizeof(msg)), msg, "below 2^31"), "exactly 2^31");
    expect(refused(ppm_validate_sizes(ref, K, 4, 2147483647, 2147483647, 2147483647, 2147483647, &ct, msg, sizeof(msg)), msg, "below 2^31"),
           "factors near 2^31");
    const int Kbig[4] = {2147483647, 2147483647, 1, 1};
    expect(refused(ppm_validate_sizes(ref, Kbig, 4, 1, 1, 1, 1, &ct, msg, sizeof(msg)), msg, "below 2^31"), "sum K overflows an int");
    expect(refused(ppm_validate_pool(nullptr, p, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "conv5 is NULL"), "null conv5");
    expect(refused(ppm_validate_pool(p, p, nullptr, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "NULL"), "null pooled");
    expect(refused(ppm_validate_pool(p, mem + 2, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "aligned to 4"), "a misaligned cat");
    expect(refused(ppm_validate_fill(nullptr, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "y is NULL"), "null y");
    expect(refused(ppm_validate_fill(ys_null, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "y[1] is NULL"), "null y[1]");
    expect(refused(ppm_validate_fill(ys_odd, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "y[1] is not aligned"), "a misaligned y[1]");
    expect(refused(ppm_validate_fill(ys, nullptr, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "cat is NULL"), "fill: null cat");
    expect(refused(ppm_validate_fill_bwd(nullptr, gys, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "grad_cat is NULL"), "fill_bwd: null grad_cat");
    expect(refused(ppm_validate_fill_bwd(p, gys_none, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "no gradient"), "fill_bwd: nothing asked");
    expect(refused(ppm_validate_pool_bwd(nullptr, gps_none, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "neither"), "pool_bwd: nothing given");
    expect(refused(ppm_validate_pool_bwd(nullptr, nullptr, p, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "neither"), "pool_bwd: both NULL");
    expect(refused(ppm_validate_pool_bwd(p, gps, nullptr, ref, K, 4, 2, 8, 7, 13, &ct, msg, sizeof(msg)), msg, "grad_conv5 is NULL"), "pool_bwd: no output");
    // a message longer than its buffer is cut, not overrun
    char tiny[8];
    expect(ppm_validate_sizes(ref, K, 5, 2, 8, 7, 13, &ct, tiny, sizeof(tiny)) == 1 && std::strlen(tiny) == 7, "a short message buffer");

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("segm_ppm_check: %ld bins, 3200 planes, %ld tap positions, 120 tile walks and 31 validator cases ok\n", walked_bins, walked_taps);
    return 0;
}
