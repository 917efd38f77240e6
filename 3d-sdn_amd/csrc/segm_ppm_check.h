// Bin and tap arithmetic, buffer layout and HOST argument validation of the pyramid pooling module (segm_ppm.hip).  Plain C++ so
// that a host program can walk the bins, the covering ranges, the tap ranges and the validators without the HIP runtime
// (tools/segm_ppm_check.cpp).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"

namespace sdn {

constexpr int PPM_MAX_SCALES = 4;     // branches of the module; the decoders use (1, 2, 3, 6)
constexpr int PPM_MAX_SIDE = 8;       // s_k: an s x s pooled map
constexpr int PPM_THREADS = 256;
constexpr int PPM_TILE_ROWS = 16;     // rows of a plane staged in LDS at a time (k_ppm_pool, k_ppm_fill_bwd)
constexpr int PPM_TILE_COLS = 256;    // columns of such a tile; a wider plane takes several tiles per row chunk
constexpr int PPM_TILE_PITCH = PPM_TILE_COLS + 4;   // floats per tile row: 16-byte aligned rows, four banks apart
constexpr int PPM_MAX_COLBINS = PPM_MAX_SCALES * PPM_MAX_SIDE;                 // 32 column bins of a row, all scales
constexpr int PPM_MAX_BINS = PPM_MAX_SCALES * PPM_MAX_SIDE * PPM_MAX_SIDE;     // 256 bins of a plane: one thread each
constexpr int PPM_CHUNK = 4 * PPM_THREADS;   // pixels of a plane per workgroup of k_ppm_fill / k_ppm_pool_bwd
static_assert(PPM_MAX_BINS <= PPM_THREADS, "a thread per bin");
static_assert(PPM_TILE_ROWS * PPM_MAX_SIDE <= PPM_THREADS && PPM_THREADS / PPM_MAX_COLBINS >= 1, "a thread per (row, column bin)");
static_assert(PPM_TILE_COLS % 4 == 0 && PPM_TILE_PITCH % 4 == 0, "16-byte tile rows");

// nn.AdaptiveAvgPool2d's bin i of s over n positions: [floor(i n / s), ceil((i + 1) n / s))
SDN_HD int ppm_bin_start(int i, int n, int s) { return (int)(((long)i * n) / s); }
SDN_HD int ppm_bin_end(int i, int n, int s) { return (int)((((long)i + 1) * n + s - 1) / s); }
// the bins lo .. hi (inclusive) that cover position y: start(i) <= y  <=>  i n < (y + 1) s;  end(i) > y  <=>  (i + 1) n > y s.
// For n >= s these are one or two bins; for n < s more (all s when n == 1).
SDN_HD void ppm_cover(int y, int n, int s, int* lo, int* hi)
{
    *lo = (int)(((long)y * s) / n);
    long h = (((long)y + 1) * s - 1) / n;
    *hi = h > s - 1 ? s - 1 : (int)h;
}

// bilinear taps of output position o of n over a map of s, align_corners=False, torch's fp32 rule (UpSample.h:
// area_pixel_compute_source_index): scale = (float)s / n
SDN_HD void ppm_taps(float scale, int o, int s, int* i0, int* i1, float* lam)
{
    float src = scale * ((float)o + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int a = (int)src;
    if (a > s - 1) a = s - 1;   // cannot happen for scale = s / n; keeps every index inside the map regardless
    *i0 = a;
    *i1 = a + 1 < s - 1 ? a + 1 : s - 1;
    *lam = src - (float)a;
}
// the weight of output position o on tap j
SDN_HD float ppm_tap_weight(float scale, int o, int s, int j)
{
    int i0, i1;
    float lam;
    ppm_taps(scale, o, s, &i0, &i1, &lam);
    return (i0 == j ? 1.f - lam : 0.f) + (i1 == j ? lam : 0.f);
}
// a range [lo, hi) of output positions that holds every position with a weight on tap j: those whose source position lies in
// [j - 1, j + 1), widened by a position either way against the rounding of the fp32 rule (tools/segm_ppm_check.cpp walks it)
SDN_HD void ppm_tap_range(int j, int n, int s, int* lo, int* hi)
{
    const double r = (double)n / (double)s;
    long a = (long)(((double)j - 0.5) * r - 0.5) - 2;
    long b = (long)(((double)j + 1.5) * r - 0.5) + 3;
    if (a < 0) a = 0;
    if (b > n) b = n;
    if (b < a) b = a;
    *lo = (int)a;
    *hi = (int)b;
}

// the branches of a call, by value in the kernel arguments
struct PpmPlan {
    int S;
    int s[PPM_MAX_SCALES];        // side of branch k's pooled map
    int K[PPM_MAX_SCALES];        // channels of branch k (0 where the call does not use them)
    int cb[PPM_MAX_SCALES + 1];   // column bins before branch k: sum of s;    cb[S]: all
    int bb[PPM_MAX_SCALES + 1];   // bins before branch k: sum of s * s;       bb[S]: all
    int kb[PPM_MAX_SCALES + 1];   // channels before branch k: sum of K;       kb[S]: all
};

inline void ppm_plan_make(const int* scales, const int* K, int S, PpmPlan* p)
{
    *p = PpmPlan{};
    p->S = S;
    for (int k = 0; k < S; k++) {
        p->s[k] = scales[k];
        p->K[k] = K ? K[k] : 0;
        p->cb[k + 1] = p->cb[k] + scales[k];
        p->bb[k + 1] = p->bb[k] + scales[k] * scales[k];
        p->kb[k + 1] = p->kb[k] + p->K[k];
    }
    for (int k = S; k < PPM_MAX_SCALES; k++) {
        p->cb[k + 1] = p->cb[k];
        p->bb[k + 1] = p->bb[k];
        p->kb[k + 1] = p->kb[k];
    }
}

// floats of the pooled buffer: p_k [B, C, s_k, s_k] one after the other; p_k begins at B * C * bb[k]
SDN_HD long ppm_pooled_floats(int B, int C, int bins) { return (long)B * C * bins; }
SDN_HD int ppm_chunks(long HW) { return (int)((HW + PPM_CHUNK - 1) / PPM_CHUNK); }   // workgroups per plane (fill, pool_bwd)
// rows of a tile of k_ppm_pool: a thread per (row, column bin)
SDN_HD int ppm_pool_rows(int colbins) { const int r = PPM_THREADS / colbins; return r < PPM_TILE_ROWS ? r : PPM_TILE_ROWS; }

// 0 when scales [S] (and K [S], unless NULL) and the sizes are valid; *ctot = C + sum K.  Otherwise 1 with the reason in msg
inline int ppm_validate_sizes(const int* scales, const int* K, int S, int B, int C, int h, int w, int* ctot, char* msg, size_t cap)
{
    if (S < 1 || S > PPM_MAX_SCALES) SDN_FAIL("%d scales; 1 to %d are supported", S, PPM_MAX_SCALES);
    if (!scales) SDN_FAIL("scales is NULL");
    if (!K) SDN_FAIL("branch_channels is NULL");
    if (B < 1 || C < 1 || h < 1 || w < 1) SDN_FAIL("bad sizes: B %d, C %d, h %d, w %d", B, C, h, w);
    long ct = C;
    for (int k = 0; k < S; k++) {
        if (scales[k] < 1 || scales[k] > PPM_MAX_SIDE) SDN_FAIL("scale %d is %d; 1 to %d are supported", k, scales[k], PPM_MAX_SIDE);
        if (K[k] < 1) SDN_FAIL("branch %d has %d channels", k, K[k]);
        ct += K[k];
        if (ct > INT_MAX) SDN_FAIL("C + sum K must stay below 2^31");
    }
    // no product overflows: every factor is below 2^31 and the running product is checked before the next factor
    const long hw = (long)h * (long)w;
    if (hw > INT_MAX || hw * ct > INT_MAX || hw * ct * B > INT_MAX)
        SDN_FAIL("B * Ctot * h * w = %d * %ld * %d * %d must stay below 2^31", B, ct, h, w);
    *ctot = (int)ct;   // (the pooled buffer, B * C * sum s^2 floats, is indexed in 64 bits)
    return 0;
}

inline int ppm_validate_pool(const void* conv5, const void* cat, const void* pooled, const int* scales, const int* K, int S, int B, int C,
                             int h, int w, int* ctot, char* msg, size_t cap)
{
    if (!conv5) SDN_FAIL("conv5 is NULL");
    if (!cat || !pooled) SDN_FAIL("cat or pooled is NULL");
    if ((reinterpret_cast<uintptr_t>(conv5) | reinterpret_cast<uintptr_t>(cat) | reinterpret_cast<uintptr_t>(pooled)) & 3)
        SDN_FAIL("conv5, cat and pooled must be aligned to 4 bytes");
    return ppm_validate_sizes(scales, K, S, B, C, h, w, ctot, msg, cap);
}

// y [S]: HOST array of DEVICE pointers
inline int ppm_validate_fill(const float* const* y, const void* cat, const int* scales, const int* K, int S, int B, int C, int h, int w,
                             int* ctot, char* msg, size_t cap)
{
    if (!y) SDN_FAIL("y is NULL");
    if (!cat) SDN_FAIL("cat is NULL");
    if (ppm_validate_sizes(scales, K, S, B, C, h, w, ctot, msg, cap)) return 1;
    for (int k = 0; k < S; k++) {
        if (!y[k]) SDN_FAIL("y[%d] is NULL", k);
        if (reinterpret_cast<uintptr_t>(y[k]) & 3) SDN_FAIL("y[%d] is not aligned to 4 bytes", k);
    }
    if (reinterpret_cast<uintptr_t>(cat) & 3) SDN_FAIL("cat must be aligned to 4 bytes");
    return 0;
}

// grad_y [S]: HOST array of DEVICE pointers, any may be NULL but not all
inline int ppm_validate_fill_bwd(const void* grad_cat, float* const* grad_y, const int* scales, const int* K, int S, int B, int C, int h,
                                 int w, int* ctot, char* msg, size_t cap)
{
    if (!grad_cat) SDN_FAIL("grad_cat is NULL");
    if (!grad_y) SDN_FAIL("grad_y is NULL");
    if (ppm_validate_sizes(scales, K, S, B, C, h, w, ctot, msg, cap)) return 1;
    int asked = 0;
    for (int k = 0; k < S; k++) {
        if (reinterpret_cast<uintptr_t>(grad_y[k]) & 3) SDN_FAIL("grad_y[%d] is not aligned to 4 bytes", k);
        asked += grad_y[k] ? 1 : 0;
    }
    if (!asked) SDN_FAIL("no gradient asked for");
    if (reinterpret_cast<uintptr_t>(grad_cat) & 3) SDN_FAIL("grad_cat must be aligned to 4 bytes");
    return 0;
}

// grad_cat may be NULL, and any grad_p[k] (grad_p itself too), but not all of them
inline int ppm_validate_pool_bwd(const void* grad_cat, const float* const* grad_p, const void* grad_conv5, const int* scales, const int* K,
                                 int S, int B, int C, int h, int w, int* ctot, char* msg, size_t cap)
{
    if (!grad_conv5) SDN_FAIL("grad_conv5 is NULL");
    if (ppm_validate_sizes(scales, K, S, B, C, h, w, ctot, msg, cap)) return 1;
    int given = grad_cat ? 1 : 0;
    for (int k = 0; k < S && grad_p; k++) {
        if (reinterpret_cast<uintptr_t>(grad_p[k]) & 3) SDN_FAIL("grad_p[%d] is not aligned to 4 bytes", k);
        given += grad_p[k] ? 1 : 0;
    }
    if (!given) SDN_FAIL("neither grad_cat nor any grad_p is given");
    if ((reinterpret_cast<uintptr_t>(grad_cat) | reinterpret_cast<uintptr_t>(grad_conv5)) & 3)
        SDN_FAIL("grad_cat and grad_conv5 must be aligned to 4 bytes");
    return 0;
}

}  // namespace sdn
