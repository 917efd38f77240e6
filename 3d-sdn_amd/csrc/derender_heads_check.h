// Constants, the buffer layouts and HOST argument validation of the Derenderer's heads (derender_heads.hip).  Plain C++ so that a host
// program can walk the layouts, the tilings and the validators without the HIP runtime (tools/derender_heads_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"

namespace sdn {

constexpr int DH_THREADS = 256;
constexpr int DH_ROWS = 16;            // objects of one row tile: every workgroup owns 16 rows of its layer's input in the LDS
constexpr int DH_COLS = 16;            // forward: output columns of one pass, one per 16-lane group (the lanes split a weight row)
constexpr int DH_KC = 256;             // input columns staged at a time
constexpr int DH_DCOLS = 64;           // backward, input gradient: output columns of a workgroup, one per lane
constexpr int DH_SLAB = 128;           // backward, input gradient: terms of one partial sum (a slab); the consumer adds the slabs in order
constexpr int DH_WJ = 8;               // backward, weight gradient: weight rows of a workgroup
constexpr int DH_WROWS = 64;           // backward, weight gradient: objects staged at a time
constexpr int DH_FIXED = 8;            // leading columns of the output row: pose delta 2, offset 2, log scale 3, log depth 1
constexpr int DH_MAX_CLASSES = 16;
constexpr int DH_MAX_N = 65535;
constexpr long long DH_LIMIT = 1ll << 31;   // every element count stays below it

// Widths and where everything lies, in floats.  `out` [n * O]: the six output groups one after the other, each contiguous;
// `saved` [n * (3 Hd + 1)]: the three post-ReLU activations [n, Hd] and the pose pair's norm [n]; the backward's workspace: the
// partial sums (slabs) of the three hidden gradients, [S3][n][Hd], [SH][n][Hd], [SH][n][Hd].
struct DhLayout {
    int n, F, Hd, classes, coeffs;
    int O, head, K1, ffd_w;            // O = 8 + classes + classes * coeffs; head = 8 + classes; K1 = Hd + 4; ffd_w = classes * coeffs
    int S3, SH;                        // slabs of a sum over O terms, over Hd terms
    long long theta, trans, scales, depths, probs, ffd, out_floats;
    long long h0, h1, h2, norm, saved_floats;
    long long p2, p1, p0, ws_floats;
};

SDN_HD int dh_slabs(int K) { return (K + DH_SLAB - 1) / DH_SLAB; }
SDN_HD int dh_row_tiles(int n) { return (n + DH_ROWS - 1) / DH_ROWS; }
// forward, last layer: workgroup 0 owns the `head` leading columns (the pose pair and the class logits must meet in one LDS), the
// others 16 coefficient columns each
SDN_HD int dh_row_col_tiles(int O, int head) { return 1 + (O - head + DH_COLS - 1) / DH_COLS; }
SDN_HD void dh_row_col_range(int ct, int O, int head, int* c0, int* c1)
{
    *c0 = ct == 0 ? 0 : head + (ct - 1) * DH_COLS;
    *c1 = ct == 0 ? head : (*c0 + DH_COLS < O ? *c0 + DH_COLS : O);
}

// 0 with the layout filled when the sizes are a valid problem; otherwise 1 with the reason in msg
inline int dh_layout(int n, int F, int Hd, int classes, int coeffs, DhLayout* L, char* msg, size_t cap)
{
    if (!L) SDN_FAIL("the layout is NULL");
    if (n < 1 || n > DH_MAX_N) SDN_FAIL("n %d; 1 to %d objects are supported", n, DH_MAX_N);
    if (F < 4 || F % 4) SDN_FAIL("F %d; a positive multiple of 4 is supported", F);
    if (Hd < 4 || Hd % 4) SDN_FAIL("Hd %d; a positive multiple of 4 is supported", Hd);
    if (classes < 1 || classes > DH_MAX_CLASSES) SDN_FAIL("classes %d; 1 to %d are supported", classes, DH_MAX_CLASSES);
    if (coeffs < 1) SDN_FAIL("coeffs %d; at least 1 per class", coeffs);
    const long long O = DH_FIXED + classes + (long long)classes * coeffs;
    if (O >= DH_LIMIT || (long long)n * O >= DH_LIMIT) SDN_FAIL("n * O = %lld must stay below 2^31", (long long)n * O);
    if ((long long)n * F >= DH_LIMIT) SDN_FAIL("n * F = %lld must stay below 2^31", (long long)n * F);
    if (O * Hd >= DH_LIMIT) SDN_FAIL("O * Hd = %lld must stay below 2^31", O * Hd);
    if ((long long)Hd * F >= DH_LIMIT) SDN_FAIL("Hd * F = %lld must stay below 2^31", (long long)Hd * F);
    if ((long long)Hd * (Hd + 4) >= DH_LIMIT) SDN_FAIL("Hd * (Hd + 4) = %lld must stay below 2^31", (long long)Hd * (Hd + 4));
    L->n = n;
    L->F = F;
    L->Hd = Hd;
    L->classes = classes;
    L->coeffs = coeffs;
    L->O = (int)O;
    L->head = DH_FIXED + classes;
    L->K1 = Hd + 4;
    L->ffd_w = classes * coeffs;
    L->S3 = dh_slabs(L->O);
    L->SH = dh_slabs(Hd);
    const long long N = n;
    L->theta = 0;
    L->trans = 2 * N;
    L->scales = 4 * N;
    L->depths = 7 * N;
    L->probs = 8 * N;
    L->ffd = (8 + classes) * N;
    L->out_floats = N * O;
    L->h0 = 0;
    L->h1 = N * Hd;
    L->h2 = 2 * N * Hd;
    L->norm = 3 * N * Hd;
    L->saved_floats = 3 * N * Hd + N;
    L->p2 = 0;
    L->p1 = L->p2 + (long long)L->S3 * N * Hd;
    L->p0 = L->p1 + (long long)L->SH * N * Hd;
    L->ws_floats = L->p0 + (long long)L->SH * N * Hd;
    if (L->ws_floats >= DH_LIMIT) SDN_FAIL("the workspace of %lld floats must stay below 2^31", L->ws_floats);
    return 0;
}

inline size_t dh_workspace_bytes(const DhLayout& L) { return round_up(sizeof(float) * (size_t)L.ws_floats, 256); }

// the four weight / bias pairs, nn.Linear's [out, in]: none NULL; vec: the weights are read 16 bytes per lane
inline int dh_validate_weights(const void* const* w, const void* const* b, bool vec, char* msg, size_t cap)
{
    for (int l = 0; l < 4; l++) {
        if (!w[l]) SDN_FAIL("w%d is NULL", l);
        if (misaligned(w[l], vec ? 16 : 4)) SDN_FAIL("w%d must be aligned to %d bytes", l, vec ? 16 : 4);
        if (b && !b[l]) SDN_FAIL("b%d is NULL", l);
        if (b && misaligned(b[l], 4)) SDN_FAIL("b%d must be aligned to 4 bytes", l);
    }
    return 0;
}

inline int dh_validate_fwd(const void* pooled, const void* roi_norms, const void* centre, const void* extent, const void* const* w,
                           const void* const* b, int n, int F, int Hd, int classes, int coeffs, const void* out, const void* centre_out,
                           const void* extent_out, const void* row, const void* saved, DhLayout* L, char* msg, size_t cap)
{
    if (dh_layout(n, F, Hd, classes, coeffs, L, msg, cap)) return 1;
    if (!pooled) SDN_FAIL("pooled is NULL");
    if (roi_norms ? (centre || extent) : (!centre || !extent))
        SDN_FAIL("exactly one roi form: roi_norms [n, 4], or centre and extent [n, 2] each");
    if (roi_norms ? (!centre_out || !extent_out) : (centre_out || extent_out))
        SDN_FAIL("centre_out and extent_out go with roi_norms: both with it, neither without");
    if (dh_validate_weights(w, b, true, msg, cap)) return 1;
    if (!out || !saved) SDN_FAIL("out or saved is NULL");
    if (misaligned(pooled, 4) || misaligned(roi_norms, 4) || misaligned(centre, 4) || misaligned(extent, 4) || misaligned(out, 4) ||
        misaligned(centre_out, 4) || misaligned(extent_out, 4) || misaligned(row, 4) || misaligned(saved, 4))
        SDN_FAIL("pooled, the roi tensors, out, row and saved must be aligned to 4 bytes");
    return 0;
}

// g: the six output gradients (any may be NULL: not read); wanted: g_pooled, g_w0, g_b0, .., g_w3, g_b3 (each written only if given)
inline int dh_validate_bwd(const void* const* g, const void* pooled, const void* centre, const void* extent, const void* const* w,
                           const void* out, const void* saved, int n, int F, int Hd, int classes, int coeffs, const void* const* wanted,
                           const void* workspace, size_t workspace_bytes, DhLayout* L, char* msg, size_t cap)
{
    if (dh_layout(n, F, Hd, classes, coeffs, L, msg, cap)) return 1;
    if (!g || !wanted) SDN_FAIL("the gradient lists are NULL");
    if (!pooled || !centre || !extent) SDN_FAIL("pooled, centre or extent is NULL");
    if (dh_validate_weights(w, nullptr, false, msg, cap)) return 1;
    if (!out || !saved) SDN_FAIL("out or saved is NULL (the forward's buffers)");
    for (int i = 0; i < 6; i++)
        if (misaligned(g[i], 4)) SDN_FAIL("output gradient %d must be aligned to 4 bytes", i);
    for (int i = 0; i < 9; i++)
        if (misaligned(wanted[i], 4)) SDN_FAIL("input gradient %d must be aligned to 4 bytes", i);
    if (misaligned(pooled, 4) || misaligned(centre, 4) || misaligned(extent, 4) || misaligned(out, 4) || misaligned(saved, 4))
        SDN_FAIL("pooled, centre, extent, out and saved must be aligned to 4 bytes");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (misaligned(workspace, 16)) SDN_FAIL("workspace must be aligned to 16 bytes");
    if (workspace_bytes < dh_workspace_bytes(*L))
        SDN_FAIL("workspace of %zu bytes; %zu are needed (sdn_derender_heads_workspace_bytes)", workspace_bytes, dh_workspace_bytes(*L));
    return 0;
}

}  // namespace sdn
