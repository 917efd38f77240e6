// Mask R-CNN's detection targets for gfx950: detection_target_layer of the reference's geometric/maskrcnn/model.py:545-724 with
// bbox_overlaps (:508-542) and utils.box_refinement (utils.py:92-113) -- the step between the proposal layer and the two heads of a
// training step, once per image.
//
// The reference builds an N x G IoU matrix from repeated copies, asks .any() three or four times and nonzero three times (each a
// device wait), shuffles twice with a host randperm, gathers a dozen times, refines the boxes in about fifteen element-wise launches,
// crops the masks and concatenates up to four times.  The sizes of its results depend on the data.  Here the randomness comes in as
// data (keys fp32 [2, N]: the chosen rows are those with the smallest keys, which is randperm(n)[:k] when randperm is the stable
// argsort of the keys), every output has the fixed size R = TRAIN_ROIS_PER_IMAGE with the counts beside it, and nothing is read back.
//
//   k_dt_sample  ONE workgroup of 1024 lanes.  Boxes, areas, ids and each box's kind (ground truth, crowd, dropped: :579-586) lie in
//                the LDS.  Each lane walks its rows against the G boxes: the IoU of bbox_overlaps in fp32 operation by operation
//                (this file is built without FMA contraction and with correctly rounded division), the first-index maximum over the
//                ground truth (a NaN is the maximum: torch.max), the maximum over the crowd.  The row's class (positive: max >= 0.5;
//                negative: max < 0.5 and crowd max < 0.001; neither), its sampling key, its number and its matched box make one 64-bit
//                key (detection_targets_check.h); prop_sort_keys of prop_device.h sorts them, best first: the positives by ascending sampling key,
//                then the negatives likewise.  Two lanes find where the classes end; P = min(cap, positives) and the negative count
//                int((1 / ratio) P - P) of :669-670 in fp64 follow, and the lanes write rows, assign, rois, target_class_ids,
//                target_deltas (box_refinement / std_dev, logf) and, for the mask kernel, the crop box of every positive (:642-650).
//   k_dt_mask    one workgroup per output row: reads n_pos from the device; a positive's H + W sample coordinates (crop_sample.h) go
//                into a per-row table, then every element is the bilinear sample of the matched mask, rounded half to even (:659);
//                every other row is +0.0.
//
// Two dependent launches, no memset, no atomics, no float reductions: two runs give the same bits.  Every launch goes to the caller's
// stream; nothing is read back.  logf is the only operation whose last bit can differ from the reference's CPU run.
#include <hip/hip_runtime.h>

#include "crop_sample.h"
#include "detection_targets_check.h"
#include "device_common.h"
#include "prop_device.h"
#include "sdn_common.h"

namespace sdn {

struct DtSample {
    const float* proposals;    // [N, 4] normalised
    const void* gt_class_ids;  // [G] int32 or int64
    const float* gt_boxes;     // [G, 4] normalised
    const float* keys;         // [2, N]: row 0 orders the positives, row 1 the negatives
    const int32_t* roi_count;  // [1] or NULL
    int N, G, S, R, cap, ids_int64, mini_mask;
    double ratio;
    float std_dev[4];
    float4* rois;              // [R]
    int32_t* target_class_ids; // [R]
    float4* target_deltas;     // [R]
    int32_t* rows;             // [R]
    int32_t* assign;           // [R]
    int32_t* count;            // [1]
    int32_t* n_pos;            // [1]
    float4* crop;              // [R] workspace
};

constexpr int DT_KIND_DROPPED = 0, DT_KIND_GT = 1, DT_KIND_CROWD = 2;

__global__ __launch_bounds__(DT_THREADS) void k_dt_sample(const DtSample D)
{
    __shared__ uint64_t s[DT_MAX_ROIS];
    __shared__ float4 s_box[DT_MAX_BOXES];
    __shared__ float s_area[DT_MAX_BOXES];
    __shared__ int s_id[DT_MAX_BOXES];
    __shared__ int s_kind[DT_MAX_BOXES];
    __shared__ int s_any_crowd, s_pos_end, s_neg_end;
    const int tid = threadIdx.x;
    if (tid < D.G) {
        const float* b = D.gt_boxes + 4 * (size_t)tid;
        const float4 g = make_float4(b[0], b[1], b[2], b[3]);
        s_box[tid] = g;
        s_area[tid] = (g.z - g.x) * (g.w - g.y);   // :535
        const long long id = D.ids_int64 ? ((const long long*)D.gt_class_ids)[tid] : (long long)((const int32_t*)D.gt_class_ids)[tid];
        s_id[tid] = id < INT_MIN ? INT_MIN : (id > INT_MAX ? INT_MAX : (int)id);
    }
    if (tid == 0) {
        s_pos_end = 0;
        s_neg_end = 0;
    }
    __syncthreads();
    if (tid == 0) {   // :579
        int any = 0;
        for (int g = 0; g < D.G; g++) any |= s_id[g] < 0;
        s_any_crowd = any;
    }
    __syncthreads();
    const bool crowd = s_any_crowd != 0;
    if (tid < D.G) s_kind[tid] = !crowd ? DT_KIND_GT : (s_id[tid] < 0 ? DT_KIND_CROWD : (s_id[tid] > 0 ? DT_KIND_GT : DT_KIND_DROPPED));   // :580-581
    __syncthreads();
    int limit = D.N;
    if (D.roi_count) limit = min(max(*D.roi_count, 0), D.N);
    for (int i = tid; i < D.S; i += DT_THREADS) {
        uint64_t key = 0ull;
        if (i < limit) {
            const float* p = D.proposals + 4 * (size_t)i;
            const float py1 = p[0], px1 = p[1], py2 = p[2], px2 = p[3];
            const float p_area = (py2 - py1) * (px2 - px1);   // :534
            float best = -INFINITY, crowd_best = -INFINITY;
            int best_g = INT_MAX, crowd_g = INT_MAX;
            for (int g = 0; g < D.G; g++) {
                const int kind = s_kind[g];
                if (kind == DT_KIND_DROPPED) continue;
                const float4 b = s_box[g];
                // bbox_overlaps, :524-539
                const float y1 = nan_first_max(py1, b.x), x1 = nan_first_max(px1, b.y);
                const float y2 = nan_first_min(py2, b.z), x2 = nan_first_min(px2, b.w);
                const float inter = nan_first_max(x2 - x1, 0.0f) * nan_first_max(y2 - y1, 0.0f);
                const float uni = p_area + s_area[g] - inter;
                const float iou = inter / uni;
                if (kind == DT_KIND_GT) {
                    if (det_argmax_takes(best, best_g, iou, g)) {   // :601, :623: the first index of the maximum, a NaN is the maximum
                        best = iou;
                        best_g = g;
                    }
                } else if (det_argmax_takes(crowd_best, crowd_g, iou, g)) {   // :590
                    crowd_best = iou;
                    crowd_g = g;
                }
            }
            if (best_g != INT_MAX) {   // a ground-truth box is left (the reference raises where none is)
                if (best >= 0.5f)      // :604
                    key = dt_key(DT_POSITIVE, __float_as_uint(D.keys[i]), (uint32_t)i, (uint32_t)best_g);
                else if (best < 0.5f && (!crowd || crowd_best < 0.001f))   // :664-665, :591
                    key = dt_key(DT_NEGATIVE, __float_as_uint(D.keys[(size_t)D.N + i]), (uint32_t)i, 0u);
            }
        }
        s[i] = key;
    }
    __syncthreads();
    prop_sort_keys(s, D.S, tid, DT_THREADS);
    // where the positives and the negatives end: at most one place each is the last of its class
    for (int i = tid; i < D.S; i += DT_THREADS) {
        const uint64_t c = dt_key_class(s[i]), next = i + 1 < D.S ? dt_key_class(s[i + 1]) : DT_NEITHER;
        if (c == DT_POSITIVE && next != DT_POSITIVE) s_pos_end = i + 1;
        if (c != DT_NEITHER && next == DT_NEITHER) s_neg_end = i + 1;
    }
    __syncthreads();
    const int pos_all = s_pos_end, neg_all = max(s_neg_end - s_pos_end, 0);
    const int P = dt_positives_taken(D.cap, pos_all);                 // :613-618
    const int Q = dt_negatives_taken(D.ratio, D.R, P, neg_all);       // :667-676
    if (tid == 0) {
        *D.count = P + Q;
        *D.n_pos = P;
    }
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int r = tid; r < D.R; r += DT_THREADS) {
        float4 roi = zero, delta = zero, crop = zero;
        int cls = -1, row = -1, assign = -1;
        if (r < P + Q) {
            const uint64_t key = r < P ? s[r] : s[pos_all + (r - P)];
            row = (int)dt_key_row(key);
            const float* p = D.proposals + 4 * (size_t)row;
            roi = make_float4(p[0], p[1], p[2], p[3]);
            cls = 0;
        }
        if (r < P) {
            assign = (int)dt_key_assign(s[r]);
            const float4 g = s_box[assign];
            cls = s_id[assign];   // :625
            // utils.box_refinement, utils.py:97-110
            const float height = roi.z - roi.x, width = roi.w - roi.y;
            const float cy = roi.x + 0.5f * height, cx = roi.y + 0.5f * width;
            const float gh = g.z - g.x, gw = g.w - g.y;
            const float gcy = g.x + 0.5f * gh, gcx = g.y + 0.5f * gw;
            const float dy = (gcy - cy) / height, dx = (gcx - cx) / width;
            const float dh = logf(gh / height), dw = logf(gw / width);
            delta = make_float4(dy / D.std_dev[0], dx / D.std_dev[1], dh / D.std_dev[2], dw / D.std_dev[3]);   // :632
            // :642-650: the roi in the frame of its box's mini-mask; otherwise the roi itself, on a full-size mask
            crop = D.mini_mask ? make_float4((roi.x - g.x) / gh, (roi.y - g.y) / gw, (roi.z - g.x) / gh, (roi.w - g.y) / gw) : roi;
        }
        D.rois[r] = roi;
        D.target_deltas[r] = delta;
        D.crop[r] = crop;
        D.target_class_ids[r] = cls;
        D.rows[r] = row;
        D.assign[r] = assign;
    }
}

struct DtMask {
    const float* gt_masks;     // [G, mh, mw]
    const float4* crop;        // [R]
    const int32_t* assign;     // [R]
    const int32_t* n_pos;      // [1]
    int mh, mw, H, W;
    float* target_mask;        // [R, H, W]
};

__global__ __launch_bounds__(DT_MASK_THREADS) void k_dt_mask(const DtMask M)
{
    // the row's sample table: entries 0 .. H - 1 for the output rows, H .. H + W - 1 for the columns
    __shared__ int t_lo[2 * DT_MAX_MASK_SIDE], t_hi[2 * DT_MAX_MASK_SIDE], t_inside[2 * DT_MAX_MASK_SIDE];
    __shared__ float t_lerp[2 * DT_MAX_MASK_SIDE];
    const int r = blockIdx.x, tid = threadIdx.x, HW = M.H * M.W;
    float* out = M.target_mask + (size_t)r * HW;
    if (r >= *M.n_pos) {   // the same in every lane: negatives and the rows behind count
        for (int i = tid; i < HW; i += DT_MASK_THREADS) out[i] = 0.0f;
        return;
    }
    const float4 box = M.crop[r];
    for (int e = tid; e < M.H + M.W; e += DT_MASK_THREADS) {
        const bool is_y = e < M.H;
        const int extent = is_y ? M.mh : M.mw;
        const float in = is_y ? axis_in(box.x, box.z, M.mh, M.H, e) : axis_in(box.y, box.w, M.mw, M.W, e - M.H);
        const bool inside = axis_inside(in, extent);
        int lo = 0, hi = 0;
        float lerp = 0.0f;
        if (inside) {   // 0 <= in <= extent - 1, so floor and ceil are rows and columns of the mask
            lo = (int)floorf(in);
            hi = (int)ceilf(in);
            lerp = in - (float)lo;
        }
        t_lo[e] = lo;
        t_hi[e] = hi;
        t_lerp[e] = lerp;
        t_inside[e] = inside ? 1 : 0;
    }
    __syncthreads();
    const float* mask = M.gt_masks + (size_t)M.assign[r] * M.mh * M.mw;
    for (int i = tid; i < HW; i += DT_MASK_THREADS) {
        const int y = i / M.W, x = M.H + (i - y * M.W);
        float v = 0.0f;   // the extrapolation value
        if (t_inside[y] && t_inside[x]) {
            const float* top_row = mask + (size_t)t_lo[y] * M.mw;
            const float* bottom_row = mask + (size_t)t_hi[y] * M.mw;
            const float tl = top_row[t_lo[x]], tr = top_row[t_hi[x]], bl = bottom_row[t_lo[x]], br = bottom_row[t_hi[x]];
            const float top = tl + (tr - tl) * t_lerp[x];
            const float bottom = bl + (br - bl) * t_lerp[x];
            v = top + (bottom - top) * t_lerp[y];
        }
        out[i] = rintf(v);   // :659 torch.round: half to even
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_detection_targets_workspace_bytes(int N, int G, int mask_h, int mask_w, int R, int H, int W, size_t* out)
{
    char why[256];
    DtLayout L;
    if (!out) return fail(SDN_EINVAL, "sdn_detection_targets_workspace_bytes: out is NULL");
    if (dt_layout(N, G, mask_h, mask_w, R, H, W, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_detection_targets_workspace_bytes: %s", why);
    *out = L.total;
    return SDN_OK;
}

SDN_API int sdn_detection_targets(const float* proposals, const void* gt_class_ids, const float* gt_boxes, const float* gt_masks,
                                  const float* keys, int N, int G, int mask_h, int mask_w, int ids_int64, const int32_t* roi_count, int R,
                                  double positive_ratio, const float* std_dev, int H, int W, int use_mini_mask, float* rois,
                                  int32_t* target_class_ids, float* target_deltas, float* target_mask, int32_t* rows, int32_t* assign,
                                  int32_t* count, int32_t* n_pos, void* workspace, size_t workspace_bytes, sdnStream stream)
{
    char why[256];
    if (dt_validate(proposals, gt_class_ids, gt_boxes, gt_masks, keys, N, G, mask_h, mask_w, ids_int64, roi_count, R, positive_ratio, std_dev, H,
                    W, rois, target_class_ids, target_deltas, target_mask, rows, assign, count, n_pos, workspace, workspace_bytes, why,
                    sizeof(why)))
        return fail(SDN_EINVAL, "sdn_detection_targets: %s", why);
    DtLayout L;
    if (dt_layout(N, G, mask_h, mask_w, R, H, W, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_detection_targets: %s", why);
    hipStream_t st = (hipStream_t)stream;
    DtSample D;
    D.proposals = proposals;
    D.gt_class_ids = gt_class_ids;
    D.gt_boxes = gt_boxes;
    D.keys = keys;
    D.roi_count = roi_count;
    D.N = N;
    D.G = G;
    D.S = prop_sort_size(N);
    D.R = R;
    D.cap = dt_positive_cap(R, positive_ratio);
    D.ids_int64 = ids_int64 ? 1 : 0;
    D.mini_mask = use_mini_mask ? 1 : 0;
    D.ratio = positive_ratio;
    for (int k = 0; k < 4; k++) D.std_dev[k] = std_dev[k];
    D.rois = (float4*)rois;
    D.target_class_ids = target_class_ids;
    D.target_deltas = (float4*)target_deltas;
    D.rows = rows;
    D.assign = assign;
    D.count = count;
    D.n_pos = n_pos;
    D.crop = (float4*)((char*)workspace + L.crop);
    hipLaunchKernelGGL(k_dt_sample, dim3(1), dim3(DT_THREADS), 0, st, D);
    DtMask M;
    M.gt_masks = gt_masks;
    M.crop = D.crop;
    M.assign = assign;
    M.n_pos = n_pos;
    M.mh = mask_h;
    M.mw = mask_w;
    M.H = H;
    M.W = W;
    M.target_mask = target_mask;
    hipLaunchKernelGGL(k_dt_mask, dim3((unsigned)R), dim3(DT_MASK_THREADS), 0, st, M);
    return check_launch("sdn_detection_targets");
}
