// The caps, the parameter block, Pillow's coefficient arithmetic and HOST argument validation of the Mask R-CNN training item
// (training_item.hip).  Plain C++ so that a host program can walk them without the HIP runtime (tools/training_item_check.cpp).  The
// band plan of the image kernel and the validation of its resampling tables are the semantic batch's (segm_train_check.h).
#pragma once

#include <cmath>
#include <cstring>

#include "detection_targets_check.h"   // DT_MAX_BOXES, PROP_ALIGN
#include "segm_train_check.h"

namespace sdn {

constexpr int TRI_THREADS = SGT_THREADS;
constexpr int TRI_MINI_THREADS = 1024;             // k_tri_mini's workgroup: one per instance, sixteen waves
constexpr int TRI_BAND = SGT_BAND;                // padded output rows of a workgroup of the image kernel
constexpr int TRI_MAX_DIM = 1024;                 // M = IMAGE_MAX_DIM: a box has at most M rows, whose horizontal pass lies in the LDS
constexpr int TRI_MAX_MINI = 56;                  // either side of MINI_MASK_SHAPE: 1024 rows of 56 bytes are 56 KiB
constexpr int TRI_MAX_BOXES = DT_MAX_BOXES;       // G: the ids and the box accumulators lie in the LDS
constexpr int TRI_MAX_FRAMES = 65535;             // frames of one size in one launch of the image kernel (grid.y)
constexpr int TRI_BOX_RUN = 8;                    // consecutive resized pixels of a lane of k_tri_boxes
constexpr int TRI_BOX_PIXELS = TRI_THREADS * TRI_BOX_RUN;   // resized pixels per workgroup of k_tri_boxes
constexpr int TRI_MASK_PIXELS = 1024;             // padded pixels per workgroup of k_tri_full
constexpr int TRI_STAGE_BYTES = 4096;             // k_tri_mini: staged crop rows, 4096 / box width rows per pass
// taps of one axis of the mini-mask resize: out * ksize <= 2 in + 3 out for in > out, 3 out otherwise
constexpr int TRI_COEF_INTS = 2 * TRI_MAX_DIM + 3 * TRI_MAX_MINI;
constexpr int TRI_ACC_ROWS = 5;                   // per instance: first row, first column, last row, last column, pixels
constexpr int TRI_PLAN_INTS = 24;
constexpr int TRI_MEAN_INTS = 3 * 256;            // fp32(fp64(byte) - MEAN_PIXEL[c]) as bits

struct TriPlan {   // the head of the parameter block; every offset counts ints from its start
    int H, W;                  // the frame
    int oh, ow;                // the resized frame (utils.py:308)
    int M;                     // the padded side, IMAGE_MAX_DIM
    int top, left;             // the zero padding before the resized frame (:313, :315)
    int flip;                  // 1: the PADDED image and masks are mirrored (model.py:1189-1190)
    int nops, order;           // the colour jitter: op k in bits 4 k .. 4 k + 3 of order
    float fb, fc, fs;          // brightness, contrast, saturation factors
    int hue;                   // added to H modulo 256
    int xb, xk, xksize;        // Pillow's bilinear tables W -> ow: bounds [ow][2], coefficients [ow][xksize]; xksize 0: pass skipped
    int yb, yk, yksize;        // H -> oh
    int ytab, xtab;            // ndimage.zoom(order=0): the source row of every resized row [oh] and column [ow], -1: the constant 0
    int mean;                  // [3][256] floats as bits
    int pad;
};
static_assert(sizeof(TriPlan) == TRI_PLAN_INTS * sizeof(int32_t), "parameter block head");

// ---- Pillow's precompute_coeffs and normalize_coeffs_8bpc for the bilinear filter (Resample.c), the box being the whole image:
// operation for operation sdn_hip/pillow.py's resample_tables and fixed_point.  Only + - * /, ceil and truncation occur.
SDN_HD double tri_scale(int in, int out) { return (double)((float)in - 0.0f) / (double)out; }
SDN_HD int tri_ksize(int in, int out)
{
    const double scale = tri_scale(in, out);
    const double support = 1.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}
SDN_HD double tri_weight(int x, int xmin, double center, double ss)
{
    double arg = ((double)(x + xmin) - center + 0.5) * ss;
    if (arg < 0.0) arg = -arg;
    return arg < 1.0 ? 1.0 - arg : 0.0;
}
// output xx of the resize in -> out: the first source index, the number of taps and the ksize fixed-point coefficients
SDN_HD void tri_coeffs(int in, int out, int xx, int ksize, int* first, int* count, int32_t* k)
{
    const double scale = tri_scale(in, out);
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double center = 0.0 + ((double)xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;   // never: ksize is the filter's width
    double ww = 0.0;
    for (int x = 0; x < xmax; x++) ww += tri_weight(x, xmin, center, ss);
    for (int x = 0; x < xmax; x++) {
        double w = tri_weight(x, xmin, center, ss);
        if (ww != 0.0) w /= ww;
        k[x] = (int32_t)(0.5 + w * (double)(1 << SGT_BITS));   // the bilinear weights are not negative
    }
    for (int x = xmax; x < ksize; x++) k[x] = 0;
    *first = xmin;
    *count = xmax;
}

struct TriLayout {
    size_t partial;   // int32 [B][nblk]: sums of L per SGT_STAT_PIXELS pixels (frames with contrast)
    size_t acc;       // int32 [TRI_ACC_ROWS][G]: the box accumulators
    size_t total;
};

inline int tri_validate_sizes(int B, int H, int W, int G, char* msg, size_t cap)
{
    if (B < 1 || B > TRI_MAX_FRAMES) SDN_FAIL("%d frames; 1 to %d of one size are supported", B, TRI_MAX_FRAMES);
    if (H < 1 || W < 1 || (long)H * W > INT_MAX / 4 || (long)B * H * W > INT_MAX / 3) SDN_FAIL("bad sizes: %d frames of %d x %d", B, H, W);
    if (W > SGT_SRC_PIXELS) SDN_FAIL("frames %d pixels wide: one frame row must fit the %d pixel staging tile", W, SGT_SRC_PIXELS);
    if (G < 0 || G > TRI_MAX_BOXES) SDN_FAIL("G %d; 1 to %d instances are supported", G, TRI_MAX_BOXES);
    return 0;
}

inline int tri_layout(int B, int H, int W, int G, TriLayout* L, char* msg, size_t cap)
{
    if (tri_validate_sizes(B, H, W, G, msg, cap)) return 1;
    if (!L) SDN_FAIL("the layout is NULL");
    const size_t nblk = (size_t)(((long)H * W + SGT_STAT_PIXELS - 1) / SGT_STAT_PIXELS);
    size_t at = 0;
    L->partial = at;
    at += round_up(sizeof(int32_t) * (size_t)B * nblk, PROP_ALIGN);
    L->acc = at;
    at += round_up(sizeof(int32_t) * (size_t)TRI_ACC_ROWS * (size_t)(G > 0 ? G : 1), PROP_ALIGN);
    L->total = at;
    return 0;
}

// 0 when the HOST copy of the parameter block is valid for frames of H x W and fits the LDS plan; otherwise 1 with the reason
inline int tri_validate_plan(const int32_t* T, long n, int H, int W, char* msg, size_t cap)
{
    if (!T) SDN_FAIL("the host copy of the parameter block is NULL");
    if (n < TRI_PLAN_INTS) SDN_FAIL("a parameter block of %ld ints cannot hold its head of %d", n, TRI_PLAN_INTS);
    TriPlan p;
    std::memcpy(&p, T, sizeof(p));
    if (p.H != H || p.W != W) SDN_FAIL("the plan is for frames of %d x %d, the frames are %d x %d", p.H, p.W, H, W);
    if (p.M < 1 || p.M > TRI_MAX_DIM) SDN_FAIL("IMAGE_MAX_DIM %d; 1 to %d is supported", p.M, TRI_MAX_DIM);
    if (p.oh < 1 || p.ow < 1 || p.oh > p.M || p.ow > p.M) SDN_FAIL("resized to %d x %d in a %d x %d image", p.oh, p.ow, p.M, p.M);
    if (p.top != (p.M - p.oh) / 2 || p.left != (p.M - p.ow) / 2)
        SDN_FAIL("padding (%d, %d) before a %d x %d frame in a %d x %d image", p.top, p.left, p.oh, p.ow, p.M, p.M);
    if (p.flip != 0 && p.flip != 1) SDN_FAIL("flip %d", p.flip);
    if (p.nops < 0 || p.nops > 4 || p.hue < 0 || p.hue > 255) SDN_FAIL("%d ops, hue shift %d", p.nops, p.hue);
    int seen = 0;
    for (int k = 0; k < p.nops; k++) {
        const int op = (p.order >> (4 * k)) & 15;
        if (op > 3 || (seen >> op) & 1) SDN_FAIL("order 0x%x is not a permutation of distinct ops", p.order);
        seen |= 1 << op;
    }
    if (((seen >> 1) & 1) && (long)H * W > SGT_MAX_CONTRAST_PIXELS)
        SDN_FAIL("contrast on a frame of %ld pixels (at most %ld)", (long)H * W, SGT_MAX_CONTRAST_PIXELS);
    if (sgt_validate_axis(T, n, TRI_PLAN_INTS, 0, "horizontal", W, p.ow, p.xb, p.xk, p.xksize, msg, cap)) return 1;
    if (sgt_validate_axis(T, n, TRI_PLAN_INTS, 0, "vertical", H, p.oh, p.yb, p.yk, p.yksize, msg, cap)) return 1;
    const int rows_cap = SGT_PLANE_BYTES / p.ow;
    for (int Y0 = 0; Y0 < p.M; Y0 += TRI_BAND) {   // the bands are cut in the PADDED image
        const int Y1 = Y0 + TRI_BAND < p.M ? Y0 + TRI_BAND : p.M;
        const int r0 = Y0 - p.top > 0 ? Y0 - p.top : 0, r1 = Y1 - p.top < p.oh ? Y1 - p.top : p.oh;
        if (r1 <= r0) continue;
        int first, count;
        sgt_band_span(p.yksize ? T + p.yb : nullptr, r0, r1, &first, &count);
        if (count > rows_cap)
            SDN_FAIL("%d x %d -> %d x %d does not fit the LDS plan: the output rows %d .. %d need %d source rows of %d bytes, a plane "
                      "holds %d", H, W, p.oh, p.ow, r0, r1 - 1, count, p.ow, rows_cap);
    }
    if (p.ytab < TRI_PLAN_INTS || p.xtab < TRI_PLAN_INTS || (long)p.ytab + p.oh > n || (long)p.xtab + p.ow > n)
        SDN_FAIL("the zoom tables (%d, %d) lie outside the block of %ld ints", p.ytab, p.xtab, n);
    for (int y = 0; y < p.oh; y++)
        if (T[p.ytab + y] < -1 || T[p.ytab + y] >= H) SDN_FAIL("zoom row %d reads row %d of %d", y, T[p.ytab + y], H);
    for (int x = 0; x < p.ow; x++)
        if (T[p.xtab + x] < -1 || T[p.xtab + x] >= W) SDN_FAIL("zoom column %d reads column %d of %d", x, T[p.xtab + x], W);
    if (p.mean < TRI_PLAN_INTS || (long)p.mean + TRI_MEAN_INTS > n) SDN_FAIL("the mean table at %d lies outside the block of %ld ints", p.mean, n);
    return 0;
}

inline int tri_validate_image(const void* frames, int B, int H, int W, const int32_t* plan_host, const void* plan, long n_plan,
                              const void* workspace, size_t workspace_bytes, const void* image, char* msg, size_t cap)
{
    TriLayout L;
    if (tri_layout(B, H, W, 0, &L, msg, cap)) return 1;
    if (!frames || !plan || !image) SDN_FAIL("frames, plan or image is NULL");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (workspace_bytes < L.total) SDN_FAIL("workspace %zu < %zu bytes", workspace_bytes, L.total);
    if (misaligned(plan, 4) || misaligned(image, 4)) SDN_FAIL("plan and image must be aligned to 4 bytes");
    if (misaligned(workspace, 16)) SDN_FAIL("workspace must be aligned to 16 bytes");
    return tri_validate_plan(plan_host, n_plan, H, W, msg, cap);
}

inline int tri_validate_item(const void* frame, const void* inst_map, const void* ids, int H, int W, int G, const int32_t* plan_host,
                             const void* plan, long n_plan, int use_mini, int mh, int mw, const void* workspace, size_t workspace_bytes,
                             const void* image, const void* boxes_int, const void* boxes, const void* boxes_norm, const void* masks,
                             const void* areas, const void* bad, char* msg, size_t cap)
{
    TriLayout L;
    if (tri_layout(1, H, W, G, &L, msg, cap)) return 1;
    if (G < 1) SDN_FAIL("G %d; 1 to %d instances are supported", G, TRI_MAX_BOXES);
    if (use_mini && (mh < 1 || mw < 1 || mh > TRI_MAX_MINI || mw > TRI_MAX_MINI))
        SDN_FAIL("mini-masks of %d x %d; each side 1 to %d is supported", mh, mw, TRI_MAX_MINI);
    if (!frame || !inst_map || !ids || !plan || !image) SDN_FAIL("frame, inst_map, ids, plan or image is NULL");
    if (!boxes_int || !boxes || !boxes_norm || !masks || !areas || !bad) SDN_FAIL("boxes_int, boxes, boxes_norm, masks, areas or bad is NULL");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (workspace_bytes < L.total) SDN_FAIL("workspace %zu < %zu bytes", workspace_bytes, L.total);
    if (misaligned(inst_map, 4) || misaligned(ids, 4) || misaligned(plan, 4) || misaligned(image, 4))
        SDN_FAIL("inst_map, ids, plan and image must be aligned to 4 bytes");
    if (misaligned(boxes_int, 4) || misaligned(boxes, 4) || misaligned(boxes_norm, 4) || misaligned(masks, 4) ||
        misaligned(areas, 4) || misaligned(bad, 4))
        SDN_FAIL("boxes_int, boxes, boxes_norm, masks, areas and bad must be aligned to 4 bytes");
    if (misaligned(workspace, 16)) SDN_FAIL("workspace must be aligned to 16 bytes");
    return tri_validate_plan(plan_host, n_plan, H, W, msg, cap);
}

}  // namespace sdn
