// The training item of Mask R-CNN for gfx950: what Dataset.__getitem__ (geometric/maskrcnn/model.py:1371-1409) makes on the host
// through load_image_gt (:1154-1211) -- utils.resize_image (utils.py:272-320), resize_mask (:323-335), np.fliplr, extract_bboxes
// (:26-49), minimize_mask (:338-353), mold_image (model.py:2196-2201) -- and the image half of mold_inputs (:2046-2082).
//
// The parameter block (training_item_check.h: TriPlan and the tables it names) is built on the host from the frame's SIZE alone and
// uploaded in one copy; nothing is read back.  A training item is three launches on the caller's stream, four with a contrast op:
//   k_tri_luma    only when contrast is among the jitter's ops: partial sums of L, one per 2048 pixels, no atomics (ti_luma_body of
//                 train_items_common.h, shared with k_segm_train_luma).
//   k_tri_image   a workgroup owns a band of four rows of the PADDED image, three channels.  The band scheme is shared with k_segm_train_image (ti_band_body):
//                 the frame rows the band needs are staged through LDS with the jitter applied once per source pixel, Pillow's
//                 horizontal pass goes into bytes in LDS, the vertical pass (tri_pixel, this kernel's own) reads them.  The zero padding is placed first and the
//                 padded image mirrored then (model.py:1189), so with an odd pad the two sides differ.  The value is a look-up in
//                 the host's table fp32(fp64(byte) - MEAN_PIXEL[c]); a padding pixel is the table's entry of 0.  Its first workgroup
//                 resets the box accumulators and `bad` for the launches behind it.
//   k_tri_boxes   ndimage.zoom(order=0) is a gather, so zoom(inst_map == id) == (zoom(inst_map) == id): a workgroup walks 2048 pixels
//                 of the resized id map through the two index tables (-1: the constant 0), eight consecutive pixels per lane, finds
//                 first / last row and column and the pixel count of every id in LDS with integer atomics (one set per run of an
//                 id) and adds its part to the workspace with integer atomics: any order gives the same bits.  No [H, W, G] stack exists.
//   k_tri_mini    one workgroup of 1024 lanes per instance (sixteen waves hide the latency of the gather that stages the crop): Pillow's precompute_coeffs and normalize_coeffs_8bpc for (y2 - y1) -> mh and
//                 (x2 - x1) -> mw in fp64 into LDS (tri_coeffs; the box is known only here), the crop's rows staged as 0 / 255 bytes
//                 (bytescale of the 0 / 1 crop), the horizontal pass of every row of the crop into bytes in LDS (up to 1024 x 56),
//                 the vertical pass and `>= 128`.  A crop whose every pixel is set has cmax == cmin in bytescale and gives an
//                 all-zero mini-mask, as the reference does; an instance without a pixel gives zeros and counts in `bad`.
//   k_tri_full    instead of k_tri_mini without mini-masks: the gathered mask itself, fp32 [G, M, M].
// The last launch also writes the boxes in their three forms and the areas.  Compiled without FMA contraction; fp64 division is IEEE.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "sdn_common.h"
#include "train_items_common.h"
#include "training_item_check.h"

namespace sdn {

static_assert(TRI_THREADS == TI_THREADS && SGT_BITS == TI_BITS, "the wave helpers and the fixed point of train_items_common.h");
static_assert(SGT_SRC_PIXELS == TI_SRC_PIXELS && SGT_PLANE_BYTES == TI_PLANE_BYTES && SGT_STAT_PIXELS == TI_STAT_PIXELS,
              "the tiles of ti_luma_body and ti_band_body");
static_assert(TRI_MAX_BOXES <= TRI_THREADS && 2 * 64 <= TRI_THREADS && TRI_MAX_MINI <= 64, "a lane per instance; a wave per axis of the coefficients");

struct TriArgs {
    const uint8_t* frames;     // [B, H, W, 3]
    const int32_t* P;          // the parameter block on the device
    int32_t* partial;          // [B, nblk] sums of L
    int32_t* acc;              // [TRI_ACC_ROWS, G] or NULL (image only)
    float* image;              // [B, 3, M, M]
    int B, nblk, G;
    const void* inst_map;      // int32 [H, W] or uint8 [H, W, 3]
    int map_rgb;
    const int32_t* ids;        // [G]
    int mh, mw;
    int32_t* boxes_int;        // [G, 4]
    float* boxes;              // [G, 4]
    float* boxes_norm;         // [G, 4]
    float* masks;              // [G, mh, mw] or [G, M, M]
    int32_t* areas;            // [G]
    int32_t* bad;              // [1]
};

__device__ __forceinline__ TriPlan tri_plan(const TriArgs& A) { return *reinterpret_cast<const TriPlan*>(A.P); }

__global__ __launch_bounds__(TRI_THREADS) void k_tri_luma(const TriArgs A)
{
    __shared__ int s_part[TI_WAVES];
    const TriPlan pl = tri_plan(A);
    const int b = blockIdx.y, total = pl.H * pl.W;
    ti_luma_body(pl, A.frames + (size_t)b * total * 3, total, A.partial + (size_t)b * A.nblk, s_part);
}

// the molded pixel (Y, X) of channel ch of the padded, mirrored image
__device__ __forceinline__ float tri_pixel(const TriArgs& A, const TriPlan& pl, const uint8_t* s_rows, int ybase, int rows, int ch, int Y, int X)
{
    const float* mean = reinterpret_cast<const float*>(A.P + pl.mean) + ch * 256;
    const int y = Y - pl.top, x = (pl.flip ? pl.M - 1 - X : X) - pl.left;
    if (y < 0 || y >= pl.oh || x < 0 || x >= pl.ow) return mean[0];
    const uint8_t* plane = s_rows + ch * SGT_PLANE_BYTES;
    int v;
    if (pl.yksize == 0) {
        v = plane[min(max(y - ybase, 0), rows - 1) * pl.ow + x];
    } else {
        const int32_t* yb = A.P + pl.yb;
        v = ti_resample_byte(plane + x, pl.ow, yb[2 * y] - ybase, min(yb[2 * y + 1], pl.yksize), rows - 1, A.P + pl.yk + y * pl.yksize);
    }
    return mean[v];
}

__global__ __launch_bounds__(TRI_THREADS) void k_tri_image(const TriArgs A)
{
    __shared__ uint8_t s_src[3 * SGT_SRC_PIXELS];
    __shared__ uint8_t s_rows[3 * SGT_PLANE_BYTES];
    __shared__ int s_part[TI_WAVES];
    const int tid = threadIdx.x, b = blockIdx.y;
    const TriPlan pl = tri_plan(A);
    const int H = pl.H, W = pl.W, M = pl.M;
    const int Y0 = blockIdx.x * TRI_BAND;
    if (Y0 >= M) return;
    if (blockIdx.x == 0 && b == 0 && A.acc) {   // k_tri_boxes, next in the stream, accumulates into them
        if (tid < A.G) {
            A.acc[tid] = INT_MAX;
            A.acc[A.G + tid] = INT_MAX;
            A.acc[2 * A.G + tid] = -1;
            A.acc[3 * A.G + tid] = -1;
            A.acc[4 * A.G + tid] = 0;
        }
        if (tid == 0) *A.bad = 0;
    }
    const int Y1 = min(Y0 + TRI_BAND, M);
    const int r0 = max(Y0 - pl.top, 0), rh = min(Y1 - pl.top, pl.oh);   // the resized rows r0 .. rh - 1 hold pixels
    // the band's source rows, staged as they lie (tri_pixel mirrors the PADDED image), and the horizontal pass (train_items_common.h)
    int ybase, rows;
    if (!ti_band_body(pl, A.P, A.frames + (size_t)b * H * W * 3, H, W, pl.ow, r0, rh, false, A.partial + (size_t)b * A.nblk, A.nblk, s_src,
                      s_rows, s_part, ybase, rows))
        return;

    // vertical pass, the mirror, the mean and the padding: every element of the band's rows is written
    float* out = A.image + (size_t)b * 3 * M * M;
    const int nr = Y1 - Y0;
    for (int i = tid; i < 3 * nr * M; i += TRI_THREADS) {
        const int ch = i / (nr * M), j = i - ch * (nr * M);
        const int Y = Y0 + j / M, X = j % M;
        out[((size_t)ch * M + Y) * M + X] = tri_pixel(A, pl, s_rows, ybase, rows, ch, Y, X);
    }
}

// the id of the resized, padded and mirrored map at (Y, X); false where the mask of every instance is 0 (the padding, the constant)
__device__ __forceinline__ bool tri_resized_id(const TriArgs& A, const TriPlan& pl, int y, int x, int& id)
{
    const int sy = A.P[pl.ytab + y], sx = A.P[pl.xtab + x];
    if (sy < 0 || sx < 0) return false;
    const size_t at = (size_t)min(sy, pl.H - 1) * pl.W + min(sx, pl.W - 1);
    if (A.map_rgb) {
        const uint8_t* p = static_cast<const uint8_t*>(A.inst_map) + 3 * at;
        id = ((int)p[0] << 16) | ((int)p[1] << 8) | (int)p[2];
    } else {
        id = static_cast<const int32_t*>(A.inst_map)[at];
    }
    return true;
}
__device__ __forceinline__ bool tri_padded_id(const TriArgs& A, const TriPlan& pl, int Y, int X, int& id)
{
    const int y = Y - pl.top, x = (pl.flip ? pl.M - 1 - X : X) - pl.left;
    if (y < 0 || y >= pl.oh || x < 0 || x >= pl.ow) return false;
    return tri_resized_id(A, pl, y, x, id);
}

__global__ __launch_bounds__(TRI_THREADS) void k_tri_boxes(const TriArgs A)
{
    __shared__ int s_ids[TRI_MAX_BOXES];
    __shared__ int s_acc[TRI_ACC_ROWS][TRI_MAX_BOXES];
    const int tid = threadIdx.x, G = A.G;
    const TriPlan pl = tri_plan(A);
    if (tid < G) {
        s_ids[tid] = A.ids[tid];
        s_acc[0][tid] = INT_MAX;
        s_acc[1][tid] = INT_MAX;
        s_acc[2][tid] = -1;
        s_acc[3][tid] = -1;
        s_acc[4][tid] = 0;
    }
    __syncthreads();
    const int total = pl.oh * pl.ow;
    // a lane walks TRI_BOX_RUN consecutive pixels and keeps the extent of the run of one id in registers: the LDS atomics, which
    // serialise on an instance's five words, are paid once per run and not once per pixel
    const int i0 = blockIdx.x * TRI_BOX_PIXELS + tid * TRI_BOX_RUN, i1 = min(i0 + TRI_BOX_RUN, total);
    bool have = false;
    int cur = 0, ylo = 0, xlo = 0, yhi = 0, xhi = 0, cnt = 0;
    const auto flush = [&]() {
        if (!have) return;
        for (int g = 0; g < G; g++)   // equal ids get equal boxes
            if (s_ids[g] == cur) {
                atomicMin(&s_acc[0][g], ylo);
                atomicMin(&s_acc[1][g], xlo);
                atomicMax(&s_acc[2][g], yhi);
                atomicMax(&s_acc[3][g], xhi);
                atomicAdd(&s_acc[4][g], cnt);
            }
    };
    for (int i = i0; i < i1; i++) {
        const int y = i / pl.ow, x = i - y * pl.ow;
        int id;
        if (!tri_resized_id(A, pl, y, x, id)) continue;
        const int Y = y + pl.top, X = pl.flip ? pl.M - 1 - (x + pl.left) : x + pl.left;
        if (have && id == cur) {
            ylo = min(ylo, Y), xlo = min(xlo, X), yhi = max(yhi, Y), xhi = max(xhi, X), cnt++;
        } else {
            flush();
            have = true, cur = id, ylo = yhi = Y, xlo = xhi = X, cnt = 1;
        }
    }
    flush();
    __syncthreads();
    if (tid < G && s_acc[4][tid] > 0) {
        atomicMin(A.acc + tid, s_acc[0][tid]);
        atomicMin(A.acc + G + tid, s_acc[1][tid]);
        atomicMax(A.acc + 2 * G + tid, s_acc[2][tid]);
        atomicMax(A.acc + 3 * G + tid, s_acc[3][tid]);
        atomicAdd(A.acc + 4 * G + tid, s_acc[4][tid]);
    }
}

// extract_bboxes (utils.py:36-48) of instance g from the accumulators: (y1, x1, y2, x2), the last ones plus 1; zeros without a pixel
__device__ __forceinline__ int tri_box(const TriArgs& A, int g, int& y1, int& x1, int& y2, int& x2)
{
    const int G = A.G, cnt = A.acc[4 * G + g];
    y1 = x1 = y2 = x2 = 0;
    if (cnt > 0) {
        y1 = A.acc[g];
        x1 = A.acc[G + g];
        y2 = A.acc[2 * G + g] + 1;
        x2 = A.acc[3 * G + g] + 1;
    }
    return cnt;
}

// one lane: the boxes as int32 (:49), as fp32 pixels (model.py:1406) and divided in fp32 by (M, M, M, M) (:1790-1794); the area
__device__ __forceinline__ void tri_write_box(const TriArgs& A, const TriPlan& pl, int g, int y1, int x1, int y2, int x2, int cnt)
{
    const int v[4] = {y1, x1, y2, x2};
    const float m = (float)pl.M;
    for (int k = 0; k < 4; k++) {
        A.boxes_int[4 * g + k] = v[k];
        A.boxes[4 * g + k] = (float)v[k];
        A.boxes_norm[4 * g + k] = (float)v[k] / m;
    }
    A.areas[g] = cnt;
    if (cnt == 0) atomicAdd(A.bad, 1);
}

__global__ __launch_bounds__(TRI_MINI_THREADS) void k_tri_mini(const TriArgs A)
{
    __shared__ int32_t s_kx[TRI_COEF_INTS], s_ky[TRI_COEF_INTS];
    __shared__ int s_bx[2 * TRI_MAX_MINI], s_by[2 * TRI_MAX_MINI];
    __shared__ uint8_t s_src[TRI_STAGE_BYTES];
    __shared__ uint8_t s_h[TRI_MAX_DIM * TRI_MAX_MINI];
    const int tid = threadIdx.x, g = blockIdx.x;
    const TriPlan pl = tri_plan(A);
    const int mh = A.mh, mw = A.mw;
    int y1, x1, y2, x2;
    const int cnt = tri_box(A, g, y1, x1, y2, x2);
    if (tid == 0) tri_write_box(A, pl, g, y1, x1, y2, x2, cnt);
    float* out = A.masks + (size_t)g * mh * mw;
    const int bh = y2 - y1, bw = x2 - x1;
    // no pixel (the reference raises), a solid crop (bytescale: cmax == cmin, every byte 0); sizes the launcher's caps exclude
    if (cnt == 0 || cnt == bh * bw || bh > TRI_MAX_DIM || bw > TRI_MAX_DIM || mh > TRI_MAX_MINI || mw > TRI_MAX_MINI) {
        for (int i = tid; i < mh * mw; i += TRI_MINI_THREADS) out[i] = 0.f;
        return;
    }
    const int id = A.ids[g];
    const int kxs = bw == mw ? 0 : tri_ksize(bw, mw), kys = bh == mh ? 0 : tri_ksize(bh, mh);   // Pillow skips a pass of equal sizes
    if ((long)kxs * mw > TRI_COEF_INTS || (long)kys * mh > TRI_COEF_INTS) {   // never: training_item_check.h, TRI_COEF_INTS
        for (int i = tid; i < mh * mw; i += TRI_MINI_THREADS) out[i] = 0.f;
        return;
    }
    if (kxs && tid < mw) tri_coeffs(bw, mw, tid, kxs, &s_bx[2 * tid], &s_bx[2 * tid + 1], s_kx + tid * kxs);
    if (kys && tid >= 64 && tid - 64 < mh) tri_coeffs(bh, mh, tid - 64, kys, &s_by[2 * (tid - 64)], &s_by[2 * (tid - 64) + 1], s_ky + (tid - 64) * kys);
    __syncthreads();
    // the horizontal pass of every row of the crop (the vertical pass of a whole-image box reads them all) into bytes
    const int per = TRI_STAGE_BYTES / bw;
    for (int c0 = 0; c0 < bh; c0 += per) {
        const int cn = min(per, bh - c0);
        for (int i = tid; i < cn * bw; i += TRI_MINI_THREADS) {   // bytescale of the crop: 0 / 255
            const int r = i / bw, x = i - r * bw;
            int v;
            s_src[i] = (tri_padded_id(A, pl, y1 + c0 + r, x1 + x, v) && v == id) ? 255 : 0;
        }
        __syncthreads();
        for (int i = tid; i < cn * mw; i += TRI_MINI_THREADS) {
            const int r = i / mw, ox = i - r * mw;
            const uint8_t* row = s_src + r * bw;
            s_h[(c0 + r) * mw + ox] = (uint8_t)(kxs ? ti_resample_byte(row, 1, s_bx[2 * ox], s_bx[2 * ox + 1], bw - 1, s_kx + ox * kxs) : row[ox]);
        }
        __syncthreads();
    }
    for (int i = tid; i < mh * mw; i += TRI_MINI_THREADS) {
        const int oy = i / mw, ox = i - oy * mw;
        const int v = kys ? ti_resample_byte(s_h + ox, mw, s_by[2 * oy], s_by[2 * oy + 1], bh - 1, s_ky + oy * kys) : s_h[oy * mw + ox];
        out[i] = v >= 128 ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(TRI_THREADS) void k_tri_full(const TriArgs A)
{
    const int tid = threadIdx.x, g = blockIdx.y;
    const TriPlan pl = tri_plan(A);
    if (blockIdx.x == 0 && tid == 0) {
        int y1, x1, y2, x2;
        const int cnt = tri_box(A, g, y1, x1, y2, x2);
        tri_write_box(A, pl, g, y1, x1, y2, x2, cnt);
    }
    const int id = A.ids[g];
    const int total = pl.M * pl.M;
    const int i0 = blockIdx.x * TRI_MASK_PIXELS, i1 = min(i0 + TRI_MASK_PIXELS, total);
    float* out = A.masks + (size_t)g * total;
    for (int i = i0 + tid; i < i1; i += TRI_THREADS) {
        const int Y = i / pl.M, X = i - Y * pl.M;
        int v;
        out[i] = (tri_padded_id(A, pl, Y, X, v) && v == id) ? 1.f : 0.f;
    }
}

static bool tri_has_contrast(const int32_t* plan_host)
{
    TriPlan p;
    memcpy(&p, plan_host, sizeof(p));
    for (int k = 0; k < p.nops; k++)
        if (((p.order >> (4 * k)) & 15) == TI_CONTRAST) return true;
    return false;
}

static int tri_launch_image(const TriArgs& A, const int32_t* plan_host, hipStream_t st)
{
    TriPlan p;
    memcpy(&p, plan_host, sizeof(p));
    if (tri_has_contrast(plan_host)) {
        hipLaunchKernelGGL(k_tri_luma, dim3((unsigned)A.nblk, (unsigned)A.B), dim3(TRI_THREADS), 0, st, A);
        if (int rc = check_launch("k_tri_luma")) return rc;
    }
    hipLaunchKernelGGL(k_tri_image, dim3(cdiv(p.M, TRI_BAND), (unsigned)A.B), dim3(TRI_THREADS), 0, st, A);
    return check_launch("k_tri_image");
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_training_item_workspace_bytes(int B, int H, int W, int G, size_t* out)
{
    if (!out) return fail(SDN_EINVAL, "sdn_training_item_workspace_bytes: out is NULL");
    char why[256];
    TriLayout L;
    if (tri_layout(B, H, W, G, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_training_item_workspace_bytes: %s", why);
    *out = L.total;
    return SDN_OK;
}

SDN_API int sdn_training_item_image(const uint8_t* frames, int B, int H, int W, const int32_t* plan_host, const int32_t* plan, long n_plan,
                                    void* workspace, size_t workspace_bytes, float* image, sdnStream stream)
{
    char why[256];
    if (tri_validate_image(frames, B, H, W, plan_host, plan, n_plan, workspace, workspace_bytes, image, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_training_item_image: %s", why);
    TriLayout L;
    tri_layout(B, H, W, 0, &L, why, sizeof(why));
    TriArgs A = {};
    A.frames = frames; A.P = plan; A.partial = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.partial);
    A.acc = nullptr; A.image = image; A.B = B; A.nblk = (int)cdiv((long)H * W, SGT_STAT_PIXELS); A.G = 0;
    return tri_launch_image(A, plan_host, (hipStream_t)stream);
}

SDN_API int sdn_training_item(const uint8_t* frame, const void* inst_map, int map_rgb, const int32_t* ids, int H, int W, int G,
                              const int32_t* plan_host, const int32_t* plan, long n_plan, int use_mini_mask, int mini_h, int mini_w,
                              void* workspace, size_t workspace_bytes, float* image, int32_t* gt_boxes_int, float* gt_boxes,
                              float* gt_boxes_norm, float* gt_masks, int32_t* areas, int32_t* bad, sdnStream stream)
{
    char why[256];
    if (tri_validate_item(frame, inst_map, ids, H, W, G, plan_host, plan, n_plan, use_mini_mask, mini_h, mini_w, workspace, workspace_bytes,
                          image, gt_boxes_int, gt_boxes, gt_boxes_norm, gt_masks, areas, bad, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_training_item: %s", why);
    TriLayout L;
    tri_layout(1, H, W, G, &L, why, sizeof(why));
    TriPlan p;
    memcpy(&p, plan_host, sizeof(p));
    TriArgs A = {};
    A.frames = frame; A.P = plan; A.partial = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.partial);
    A.acc = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.acc);
    A.image = image; A.B = 1; A.nblk = (int)cdiv((long)H * W, SGT_STAT_PIXELS); A.G = G;
    A.inst_map = inst_map; A.map_rgb = map_rgb ? 1 : 0; A.ids = ids; A.mh = mini_h; A.mw = mini_w;
    A.boxes_int = gt_boxes_int; A.boxes = gt_boxes; A.boxes_norm = gt_boxes_norm; A.masks = gt_masks; A.areas = areas; A.bad = bad;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = tri_launch_image(A, plan_host, st)) return rc;
    hipLaunchKernelGGL(k_tri_boxes, dim3(cdiv((long)p.oh * p.ow, TRI_BOX_PIXELS)), dim3(TRI_THREADS), 0, st, A);
    if (int rc = check_launch("k_tri_boxes")) return rc;
    if (use_mini_mask) {
        hipLaunchKernelGGL(k_tri_mini, dim3((unsigned)G), dim3(TRI_MINI_THREADS), 0, st, A);
        return check_launch("k_tri_mini");
    }
    hipLaunchKernelGGL(k_tri_full, dim3(cdiv((long)p.M * p.M, TRI_MASK_PIXELS), (unsigned)G), dim3(TRI_THREADS), 0, st, A);
    return check_launch("k_tri_full");
}
