// The training batch of the semantic branch (semantic/vkitti_dataset.py:74-163, TrainDataset.__getitem__).
//
// The reference builds every item on the host: a Python call per pixel for the label (:120), torchvision's ColorJitter through
// Pillow (:124), cv2.flip (:132-136), three scipy.misc.imresize calls (:139-150), the BGR swap and Normalize (:152-154) and the
// copy into the zero-padded batch tensors (:156-159).  Here a batch is at most three launches:
//   k_segm_train_luma    the one global quantity of the colour jitter: ImageEnhance.Contrast blends with int(mean(L) + 0.5) of
//                        the whole frame as it is after the ops that precede contrast.  A workgroup sums L over 2048 pixels and
//                        writes ONE partial sum; no atomics.  Launched only when an item has a contrast op.
//   k_segm_train_image   a workgroup owns a band of output rows of one item, all three channels, the whole batch width.  It
//                        stages the frame rows the band needs through LDS -- jitter and flip applied THERE, once per source
//                        pixel and band --, runs Pillow's horizontal pass (ImagingResample, 22-bit fixed point, rounded to
//                        uint8 as Pillow stores it) out of the staged pixels into LDS and the vertical pass out of LDS, then
//                        writes (float(px[2 - c]) - m_c) / s_c, and 0 wherever the item ends: the padding is written here,
//                        there is no memset.  A pass Pillow skips (equal sizes) copies.
//   k_segm_train_labels  the two NEAREST resizes and the padding between them as one gather (:140-150): the label at (y, x)
//                        is the table label of the scene pixel (ytab[rate y + rate / 2], flip(xtab[rate x + rate / 2])) - 1
//                        where both indices lie inside the item, -1 elsewhere.  A colour outside the table (the reference
//                        raises KeyError) gives -1 and is counted, one integer atomic per wave.
// The colour arithmetic is train_items_common.h's, and so are the body of the luma kernel (ti_luma_body) and the image kernel's band
// scheme up to and including the horizontal pass (ti_band_body), both shared with training_item.hip; the vertical pass, BGR,
// Normalize and the padding (sgt_pixel) are this kernel's own.  Compiled without FMA contraction.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "sdn_common.h"
#include "segm_train_check.h"
#include "train_items_common.h"

namespace sdn {

static_assert(SGT_THREADS == TI_THREADS && SGT_BITS == TI_BITS, "the wave helpers and the fixed point of train_items_common.h");
static_assert(SGT_SRC_PIXELS == TI_SRC_PIXELS && SGT_PLANE_BYTES == TI_PLANE_BYTES && SGT_STAT_PIXELS == TI_STAT_PIXELS,
              "the tiles of ti_luma_body and ti_band_body");
static_assert(3 * (SGT_SRC_PIXELS + SGT_PLANE_BYTES) <= 48 * 1024, "three workgroups per CU");

struct SegTrainParams {
    const uint8_t* frames;     // [B, H, W, 3]
    const uint8_t* scenes;     // [B, H, W, 3]
    const int32_t* T;          // the table buffer; B item rows first
    int32_t* partial;          // [B, nblk] sums of L (items with contrast)
    int B, H, W, Hb, Wb, rate, nblk, vec;
    float mean[3], std[3];
    float* img;                // [B, 3, Hb, Wb]
    long long* labels;         // [B, Hb / rate, Wb / rate]
    int32_t* unknown;          // [B]
};

__device__ __forceinline__ SegTrainItem sgt_item(const SegTrainParams& A, int b)
{
    return reinterpret_cast<const SegTrainItem*>(A.T)[b];
}

__global__ __launch_bounds__(SGT_THREADS) void k_segm_train_luma(const SegTrainParams A)
{
    __shared__ int s_part[TI_WAVES];
    const int b = blockIdx.y, total = A.H * A.W;
    ti_luma_body(sgt_item(A, b), A.frames + (size_t)b * total * 3, total, A.partial + (size_t)b * A.nblk, s_part);
}

// the finished pixel (y, x) of output channel ch: the vertical pass over colour plane 2 - ch (RGB to BGR, :152), then Normalize
// with the constants of the OUTPUT channel (:154)
__device__ __forceinline__ float sgt_pixel(const SegTrainParams& A, const SegTrainItem& it, const uint8_t* s_rows, int ybase, int rows,
                                           int ch, int y, int x)
{
    if (y >= it.h || x >= it.w) return 0.f;
    const uint8_t* plane = s_rows + (2 - ch) * SGT_PLANE_BYTES;
    int v;
    if (it.yksize == 0) {
        v = plane[min(max(y - ybase, 0), rows - 1) * it.w + x];
    } else {
        const int32_t* yb = A.T + it.yb;
        const int32_t* k = A.T + it.yk + y * it.yksize;
        const int y0 = yb[2 * y] - ybase, yc = min(yb[2 * y + 1], it.yksize);
        v = ti_resample_byte(plane + x, it.w, y0, yc, rows - 1, k);
    }
    return ((float)v - A.mean[ch]) / A.std[ch];
}

__global__ __launch_bounds__(SGT_THREADS) void k_segm_train_image(const SegTrainParams A)
{
    __shared__ uint8_t s_src[3 * SGT_SRC_PIXELS];
    __shared__ uint8_t s_rows[3 * SGT_PLANE_BYTES];
    __shared__ int s_part[TI_WAVES];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int r0 = blockIdx.x * SGT_BAND;
    const int H = A.H, W = A.W, Hb = A.Hb, Wb = A.Wb;
    if (r0 >= Hb) return;
    const SegTrainItem it = sgt_item(A, b);
    if (blockIdx.x == 0 && tid == 0) A.unknown[b] = 0;   // k_segm_train_labels, next in the stream, counts into it
    const int r1 = min(r0 + SGT_BAND, Hb);
    const int rh = min(r1, it.h);   // the rows r0 .. rh - 1 hold pixels
    // the band's source rows, staged mirrored when the item is flipped, and the horizontal pass (train_items_common.h)
    int ybase, rows;
    if (!ti_band_body(it, A.T, A.frames + (size_t)b * H * W * 3, H, W, it.w, r0, rh, it.flip != 0, A.partial + (size_t)b * A.nblk, A.nblk,
                      s_src, s_rows, s_part, ybase, rows))
        return;

    // vertical pass, BGR, Normalize, and the zeros of the padding: every element of the band's rows is written
    float* out = A.img + (size_t)b * 3 * Hb * Wb;
    const int nr = r1 - r0;
    if (A.vec) {   // Wb is a multiple of 4 and img is aligned to 16 bytes: one 128-bit store per thread and round
        const int n4 = Wb >> 2;
        for (int i = tid; i < 3 * nr * n4; i += SGT_THREADS) {
            const int ch = i / (nr * n4), j = i - ch * (nr * n4);
            const int y = r0 + j / n4, x = (j % n4) << 2;
            float4 v;
            v.x = sgt_pixel(A, it, s_rows, ybase, rows, ch, y, x);
            v.y = sgt_pixel(A, it, s_rows, ybase, rows, ch, y, x + 1);
            v.z = sgt_pixel(A, it, s_rows, ybase, rows, ch, y, x + 2);
            v.w = sgt_pixel(A, it, s_rows, ybase, rows, ch, y, x + 3);
            *reinterpret_cast<float4*>(out + ((size_t)ch * Hb + y) * Wb + x) = v;
        }
    } else {
        for (int i = tid; i < 3 * nr * Wb; i += SGT_THREADS) {
            const int ch = i / (nr * Wb), j = i - ch * (nr * Wb);
            const int y = r0 + j / Wb, x = j % Wb;
            out[((size_t)ch * Hb + y) * Wb + x] = sgt_pixel(A, it, s_rows, ybase, rows, ch, y, x);
        }
    }
}

__global__ __launch_bounds__(SGT_THREADS) void k_segm_train_labels(const SegTrainParams A)
{
    __shared__ int32_t s_codes[SEG_MAX_COLORS], s_labels[SEG_MAX_COLORS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const SegTrainItem it = sgt_item(A, b);
    const int K = min(max(it.K, 1), SEG_MAX_COLORS);
    for (int i = tid; i < K; i += SGT_THREADS) {
        s_codes[i] = A.T[it.ct + i];
        s_labels[i] = A.T[it.ct + K + i];
    }
    __syncthreads();
    const int Hl = A.Hb / A.rate, Wl = A.Wb / A.rate;
    const int i = blockIdx.x * SGT_THREADS + tid;
    const bool in = i < Hl * Wl;
    int lab = -1, miss = 0;   // outside the item: the zero padding of :145-146 and :108, minus 1 (:159)
    if (in) {
        const int y = i / Wl, x = i - y * Wl;
        const int sy = A.rate * y + A.rate / 2, sx = A.rate * x + A.rate / 2;   // the second resize's index: its factor is exactly rate
        if (sy < it.h && sx < it.w) {
            const int fy = min(max(A.T[it.yn + sy], 0), A.H - 1);
            int fx = min(max(A.T[it.xn + sx], 0), A.W - 1);
            if (it.flip) fx = A.W - 1 - fx;
            const int code = code24(A.scenes + (((size_t)b * A.H + fy) * A.W + fx) * 3);
            const int k = seg_find(s_codes, K, code);
            if (k < 0) miss = 1;
            else lab = s_labels[k] - 1;
        }
        A.labels[(size_t)b * Hl * Wl + i] = (long long)lab;
    }
    miss = wave_sum(miss);   // every wave of the workgroup gets here
    if (miss && (tid & 63) == 0) atomicAdd(A.unknown + b, miss);
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_segm_train_batch(const uint8_t* frames, const uint8_t* scenes, int B, int H, int W, const int32_t* tables_host,
                                 const int32_t* tables, long n_tables, int Hb, int Wb, int rate, float mean0, float mean1, float mean2,
                                 float std0, float std1, float std2, int32_t* workspace, long n_workspace, float* img_data,
                                 int64_t* seg_label, int32_t* unknown, sdnStream stream)
{
    if (!frames || !scenes || !tables_host || !tables || !workspace || !img_data || !seg_label || !unknown)
        return fail(SDN_EINVAL, "sdn_segm_train_batch: null pointer");
    if (std0 == 0.f || std1 == 0.f || std2 == 0.f) return fail(SDN_EINVAL, "sdn_segm_train_batch: std is 0");
    if ((reinterpret_cast<uintptr_t>(tables) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 3) || (reinterpret_cast<uintptr_t>(img_data) & 3) ||
        (reinterpret_cast<uintptr_t>(seg_label) & 7) || (reinterpret_cast<uintptr_t>(unknown) & 3))
        return fail(SDN_EINVAL, "sdn_segm_train_batch: tables, workspace, img_data and unknown must be aligned to 4 bytes, seg_label to 8");
    char why[256];
    if (sgt_validate(tables_host, n_tables, B, H, W, Hb, Wb, rate, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_segm_train_batch: %s", why);
    const int nblk = (int)cdiv((long)H * W, SGT_STAT_PIXELS);
    bool contrast = false;
    for (int i = 0; i < B; i++) {
        SegTrainItem it;
        memcpy(&it, tables_host + (size_t)i * SGT_ITEM_INTS, sizeof(it));
        for (int k = 0; k < it.nops; k++) contrast = contrast || ((it.order >> (4 * k)) & 15) == TI_CONTRAST;
    }
    if (contrast && n_workspace < (long)B * nblk)
        return fail(SDN_EINVAL, "sdn_segm_train_batch: a workspace of %ld ints; %d items of %d x %d with contrast need %ld", n_workspace, B, H, W,
                    (long)B * nblk);
    SegTrainParams A;
    A.frames = frames; A.scenes = scenes; A.T = tables; A.partial = workspace;
    A.B = B; A.H = H; A.W = W; A.Hb = Hb; A.Wb = Wb; A.rate = rate; A.nblk = nblk;
    A.vec = ((Wb & 3) == 0 && (reinterpret_cast<uintptr_t>(img_data) & 15) == 0) ? 1 : 0;
    A.mean[0] = mean0; A.mean[1] = mean1; A.mean[2] = mean2; A.std[0] = std0; A.std[1] = std1; A.std[2] = std2;
    A.img = img_data; A.labels = reinterpret_cast<long long*>(seg_label); A.unknown = unknown;
    hipStream_t st = (hipStream_t)stream;
    if (contrast) {
        hipLaunchKernelGGL(k_segm_train_luma, dim3((unsigned)nblk, (unsigned)B), dim3(SGT_THREADS), 0, st, A);
        if (int rc = check_launch("k_segm_train_luma")) return rc;
    }
    hipLaunchKernelGGL(k_segm_train_image, dim3(cdiv(Hb, SGT_BAND), (unsigned)B), dim3(SGT_THREADS), 0, st, A);
    if (int rc = check_launch("k_segm_train_image")) return rc;
    const long nl = (long)(Hb / rate) * (Wb / rate);
    hipLaunchKernelGGL(k_segm_train_labels, dim3(cdiv(nl, SGT_THREADS), (unsigned)B), dim3(SGT_THREADS), 0, st, A);
    return check_launch("k_segm_train_labels");
}
