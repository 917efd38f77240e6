// Mask R-CNN's RPN targets for gfx950: build_rpn_targets of the reference's geometric/maskrcnn/model.py:1214-1322 with compute_overlaps
// and compute_iou (utils.py:52-89) -- the rpn_match and rpn_bbox arguments of the training losses, once per image.
//
// The reference is numpy in float64 on the host: an [A, G] IoU matrix column by column (210 MB at A = 261 888, G = 100), two arg-maxes,
// three masked writes, np.random.choice twice and a Python loop over the positive anchors.  Here no matrix exists, the randomness comes
// in as data (keys fp32 [2, A]: of too many positives the T / 2 with the smallest keys of row 0 stay, of too many negatives the
// T - n_pos with the smallest keys of row 1; equal keys keep the lower anchor), every output has a fixed size and nothing is read back.
// All arithmetic is fp64, operation for operation the reference's (this file is built without FMA contraction; fp64 division is
// IEEE); only the final rpn_bbox is rounded to fp32, as the reference's Dataset does (:1404).
//
// A chunk is RT_CHUNK = 1024 consecutive anchors: one workgroup of 1024 lanes in k_rt_match (one anchor per lane; sixteen waves hide
// the latency of the fp64 division), one of 256 lanes with four anchors per lane in the other kernels.
//
//   k_rt_match   per chunk.  The boxes, widened to fp64, their areas and kinds (box, crowd, dropped: :1235-1241) lie in the LDS.  A lane
//                walks the G boxes for each of its anchors: compute_iou, the maximum and its FIRST index (np.argmax: the first NaN is a
//                maximum), the maximum over the crowd (np.amax: a NaN stays).  It writes the provisional label (:1265, :1271) and the
//                arg-max byte.  Per box a wave reduces (IoU image, lowest anchor) -- without a shuffle where the whole wave's IoU is
//                0 -- and the workgroup writes its row of the [chunks, G] table.
//   k_rt_best    per box: the table's column reduced to gt_iou_argmax (:1268), the first anchor of the largest IoU.  Zeroes the
//                histograms.
//   k_rt_label   per chunk: :1269, every box's best anchor becomes positive; the labels before sampling are final.  256-bin histograms
//                of the highest byte of the key image, one for the positives and one for the negatives (integer atomics: any order
//                gives the same sums).  Their totals decide everywhere below whether a class is over its cap.
//   k_rt_pass    three launches, radix passes 1 to 3 of the exact select of the cut key: every workgroup finds the digits so far with
//                ids_find (rank_select.h) and counts the next digit of the anchors that share them.  A class under its cap is left out.
//   k_rt_ties    per chunk: the positives below the cut key, the positives at it, the negatives at it.
//   k_rt_final   per chunk: the counts of the chunks before it and ballots inside it give every anchor at the cut key its rank in anchor
//                order (the first `residual + 1` stay) and every positive that stays its row k: the unsampled anchors go back to 0
//                (:1280, :1288), the deltas of :1295-1320 are written to row k with the anchor beside them; workgroup 0 writes the
//                padding behind n_pos and the two counts.
//
// Eight dependent launches on the caller's stream, no memset, no floating-point atomics, no float reductions: two runs give the same
// bits.  log is the only operation whose last bit can differ from the reference's CPU run.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "rank_select.h"
#include "rpn_targets_check.h"
#include "sdn_common.h"

namespace sdn {

constexpr int RT_KIND_DROPPED = 0, RT_KIND_BOX = 1, RT_KIND_CROWD = 2;

struct RtArgs {
    const double* anchors;     // [A, 4]
    const void* gt_class_ids;  // [G] int32 or int64
    const void* gt_boxes;      // [G, 4] fp32 or int32, pixels
    const float* keys;         // [2, A]
    const int32_t* gt_count;   // [1] or NULL
    int A, G, T, chunks, ids_int64, boxes_int32;
    double std_dev[4];
    int32_t* rpn_match;        // [A]
    float4* rpn_bbox;          // [T]
    int32_t* rows;             // [T]
    int32_t* counts;           // [2]
    int32_t* hist;             // workspace, RtLayout
    int32_t* best;
    int32_t* chunk_counts;
    uint64_t* tab_image;
    int32_t* tab_anchor;
    uint8_t* argmax;
};

__device__ __forceinline__ double rt_box_coord(const RtArgs& R, int g, int k)
{
    return R.boxes_int32 ? (double)((const int32_t*)R.gt_boxes)[4 * g + k] : (double)((const float*)R.gt_boxes)[4 * g + k];
}

__global__ __launch_bounds__(RT_MATCH_THREADS) void k_rt_match(const RtArgs R)
{
    __shared__ double s_box[RT_MAX_BOXES][4];
    __shared__ double s_area[RT_MAX_BOXES];
    __shared__ long long s_id[RT_MAX_BOXES];
    __shared__ int s_kind[RT_MAX_BOXES];
    __shared__ uint64_t s_tab_image[RT_MATCH_WAVES][RT_MAX_BOXES];
    __shared__ int s_tab_anchor[RT_MATCH_WAVES][RT_MAX_BOXES];
    __shared__ int s_any_crowd;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int limit = R.G;
    if (R.gt_count) limit = min(max(*R.gt_count, 0), R.G);
    if (tid < R.G) {
        long long id = 0;
        double b[4] = {0.0, 0.0, 0.0, 0.0};
        if (tid < limit) {   // rows at or behind gt_count are not read
            id = R.ids_int64 ? ((const long long*)R.gt_class_ids)[tid] : (long long)((const int32_t*)R.gt_class_ids)[tid];
            for (int k = 0; k < 4; k++) b[k] = rt_box_coord(R, tid, k);
        }
        s_id[tid] = id;
        for (int k = 0; k < 4; k++) s_box[tid][k] = b[k];
        s_area[tid] = (b[2] - b[0]) * (b[3] - b[1]);   // utils.py:81
    }
    __syncthreads();
    if (tid == 0) {   // :1235
        int any = 0;
        for (int g = 0; g < limit; g++) any |= s_id[g] < 0;
        s_any_crowd = any;
    }
    __syncthreads();
    const bool crowd = s_any_crowd != 0;
    if (tid < R.G)   // :1238-1241: only with a crowd are the ids of 0 dropped as well
        s_kind[tid] = tid >= limit ? RT_KIND_DROPPED : (!crowd ? RT_KIND_BOX : (s_id[tid] < 0 ? RT_KIND_CROWD : (s_id[tid] > 0 ? RT_KIND_BOX : RT_KIND_DROPPED)));
    __syncthreads();
    {
        const long long first = (long long)blockIdx.x * RT_CHUNK + w * 64, i = first + lane;   // `first` is the same in every lane of the wave
        const bool valid = i < R.A;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (valid) {
            const double2 lo = ((const double2*)R.anchors)[2 * i], hi = ((const double2*)R.anchors)[2 * i + 1];
            a0 = lo.x, a1 = lo.y, a2 = hi.x, a3 = hi.y;
        }
        const double a_area = (a2 - a0) * (a3 - a1);   // utils.py:80
        bool have = false, have_crowd = false;
        double best = 0.0, crowd_best = 0.0;
        int best_g = 0;
        for (int g = 0; g < R.G; g++) {
            const int kind = s_kind[g];   // the same in every lane
            if (kind == RT_KIND_DROPPED) continue;
            // compute_iou, utils.py:63-69: the box is the ground truth's, the boxes are the anchors
            const double y1 = nan_first_max(s_box[g][0], a0), y2 = nan_first_min(s_box[g][2], a2);
            const double x1 = nan_first_max(s_box[g][1], a1), x2 = nan_first_min(s_box[g][3], a3);
            const double inter = nan_first_max(x2 - x1, 0.0) * nan_first_max(y2 - y1, 0.0);
            const double uni = s_area[g] + a_area - inter;
            const double iou = inter / uni;
            if (kind == RT_KIND_CROWD) {   // :1244 np.amax
                crowd_best = have_crowd ? nan_first_max(crowd_best, iou) : iou;
                have_crowd = true;
                continue;
            }
            if (rt_argmax_takes(have, best, iou)) {   // :1263
                best = iou;
                best_g = g;
                have = true;
            }
            // :1268, this wave's part: the largest image and the lowest anchor that has it
            const uint64_t image = valid ? rt_image(iou) : 0ull;
            uint64_t m = RT_IMAGE_ZERO;
            int at = 0;
            if (__ballot(valid && image != RT_IMAGE_ZERO) != 0ull) {
                m = image;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint64_t o = __shfl_xor(m, d, 64);
                    m = o > m ? o : m;
                }
                at = __ffsll((long long)__ballot(valid && image == m)) - 1;
            }
            if (lane == 0) {
                s_tab_image[w][g] = first < R.A ? m : 0ull;
                s_tab_anchor[w][g] = (int)first + at;
            }
        }
        if (valid) {
            const double mx = have ? best : 0.0;   // no box is left: every maximum counts as 0 (the reference raises)
            const bool no_crowd = !crowd || crowd_best < 0.001;   // :1245
            int label = 0;
            if (mx < 0.3 && no_crowd) label = -1;   // :1265
            if (have && mx >= 0.7) label = 1;       // :1271
            R.rpn_match[i] = label;
            R.argmax[i] = (uint8_t)best_g;
        }
    }
    __syncthreads();
    if (tid < R.G && s_kind[tid] != RT_KIND_BOX) {   // no wave wrote this column
        R.tab_image[(size_t)blockIdx.x * R.G + tid] = 0ull;
        R.tab_anchor[(size_t)blockIdx.x * R.G + tid] = -1;
    } else if (tid < R.G) {   // the waves in anchor order: only a larger image takes
        uint64_t m = 0ull;
        int at = -1;
        for (int v = 0; v < RT_MATCH_WAVES; v++)
            if (s_tab_image[v][tid] > m) {
                m = s_tab_image[v][tid];
                at = s_tab_anchor[v][tid];
            }
        R.tab_image[(size_t)blockIdx.x * R.G + tid] = m;
        R.tab_anchor[(size_t)blockIdx.x * R.G + tid] = at;
    }
}

__global__ __launch_bounds__(RT_THREADS) void k_rt_best(const RtArgs R)
{
    __shared__ uint64_t s_image[RT_THREADS];
    __shared__ int s_anchor[RT_THREADS];
    const int tid = threadIdx.x, g = blockIdx.x;
    if (g == 0)
        for (int e = tid; e < RT_HIST_INTS; e += RT_THREADS) R.hist[e] = 0;
    uint64_t m = 0ull;
    int at = -1;
    for (int c = tid; c < R.chunks; c += RT_THREADS) {   // ascending chunks are ascending anchors
        const uint64_t image = R.tab_image[(size_t)c * R.G + g];
        if (image > m) {
            m = image;
            at = R.tab_anchor[(size_t)c * R.G + g];
        }
    }
    s_image[tid] = m;
    s_anchor[tid] = at;
    __syncthreads();
    for (int d = RT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) {
            const uint64_t o = s_image[tid + d];
            const int oa = s_anchor[tid + d];
            if (o > s_image[tid] || (o == s_image[tid] && o != 0ull && oa < s_anchor[tid])) {
                s_image[tid] = o;
                s_anchor[tid] = oa;
            }
        }
        __syncthreads();
    }
    if (tid == 0) R.best[g] = s_anchor[0];
}

// the class of a label: the positives are sampled by row 0 of the keys, the negatives by row 1
__device__ __forceinline__ int rt_class(int label) { return label == 1 ? RT_POS : (label == -1 ? RT_NEG : -1); }

__global__ __launch_bounds__(RT_THREADS) void k_rt_label(const RtArgs R)
{
    __shared__ int s_flag[RT_CHUNK];
    __shared__ int s_hist[2][RT_BINS];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * RT_CHUNK;
    for (int e = tid; e < RT_CHUNK; e += RT_THREADS) s_flag[e] = 0;
    for (int e = tid; e < 2 * RT_BINS; e += RT_THREADS) (&s_hist[0][0])[e] = 0;
    __syncthreads();
    if (tid < R.G) {
        const long long b = R.best[tid];
        if (b >= base && b < base + RT_CHUNK) s_flag[b - base] = 1;   // :1269
    }
    __syncthreads();
    for (int e = tid; e < RT_CHUNK; e += RT_THREADS) {
        const long long i = base + e;
        if (i >= R.A) break;
        int label = R.rpn_match[i];
        if (s_flag[e]) {
            label = 1;
            R.rpn_match[i] = 1;
        }
        const int s = rt_class(label);
        if (s >= 0) atomicAdd(&s_hist[s][rt_digit(dt_image(__float_as_uint(R.keys[(size_t)s * R.A + i])), 0)], 1);
    }
    __syncthreads();
    for (int e = tid; e < 2 * RT_BINS; e += RT_THREADS) {
        const int n = (&s_hist[0][0])[e];
        if (n) atomicAdd(&R.hist[e], n);
    }
}

// What the histograms of `passes` radix passes say about the two selects; computed by one wave, all 64 lanes.
struct RtSelect {
    int need[2];       // the class is over its cap
    int kept[2];       // the anchors of the class that stay
    uint32_t cut[2];   // the digits of the cut key found so far; after RT_PASSES the key image itself
    int residual[2];   // the rank left inside the last bin; after RT_PASSES, residual + 1 anchors AT the cut key stay
};

__device__ __forceinline__ void rt_select(const int32_t* hist, int T, int passes, int lane, RtSelect* S)
{
    int total[2];
    for (int s = 0; s < 2; s++) {
        int n = 0;
        for (int k = 0; k < 4; k++) n += hist[s * RT_BINS + 4 * lane + k];
        for (int d = 1; d < 64; d <<= 1) n += __shfl_xor(n, d, 64);
        total[s] = n;
    }
    const int kept_pos = rt_positives_kept(T, total[RT_POS]);
    const int cap[2] = {rt_positive_cap(T), rt_negative_cap(T, kept_pos)};
    for (int s = 0; s < 2; s++) {
        const bool need = total[s] > cap[s];
        uint32_t cut = 0xffffffffu;
        int residual = INT_MAX - 1;
        if (need) {   // the same in every lane
            long rank = cap[s] - 1;   // caps are at least 1: T >= 2
            cut = 0u;
            residual = (int)rank;
            for (int p = 0; p < passes; p++) {
                int bin, r;
                ids_find(hist + (p * 2 + s) * RT_BINS, rank, lane, &bin, &r);
                cut = (cut << 8) | (uint32_t)bin;
                rank = r;
                residual = r;
            }
        }
        if (lane == 0) {
            S->need[s] = need ? 1 : 0;
            S->kept[s] = need ? cap[s] : total[s];
            S->cut[s] = cut;
            S->residual[s] = residual;
        }
    }
}

__global__ __launch_bounds__(RT_THREADS) void k_rt_pass(const RtArgs R, int p)
{
    __shared__ RtSelect S;
    __shared__ int s_hist[2][RT_BINS];
    const int tid = threadIdx.x;
    if (tid < 64) rt_select(R.hist, R.T, p, tid, &S);
    for (int e = tid; e < 2 * RT_BINS; e += RT_THREADS) (&s_hist[0][0])[e] = 0;
    __syncthreads();
    if (!S.need[0] && !S.need[1]) return;   // the same in every lane
    const long long base = (long long)blockIdx.x * RT_CHUNK;
    for (int e = tid; e < RT_CHUNK; e += RT_THREADS) {
        const long long i = base + e;
        if (i >= R.A) break;
        const int s = rt_class(R.rpn_match[i]);
        if (s < 0 || !S.need[s]) continue;
        const uint32_t image = dt_image(__float_as_uint(R.keys[(size_t)s * R.A + i]));
        if (rt_prefix(image, p) == S.cut[s]) atomicAdd(&s_hist[s][rt_digit(image, p)], 1);
    }
    __syncthreads();
    for (int e = tid; e < 2 * RT_BINS; e += RT_THREADS) {
        const int n = (&s_hist[0][0])[e];
        if (n) atomicAdd(&R.hist[p * 2 * RT_BINS + e], n);
    }
}

__global__ __launch_bounds__(RT_THREADS) void k_rt_ties(const RtArgs R)
{
    __shared__ RtSelect S;
    __shared__ int s_count[3];
    const int tid = threadIdx.x;
    if (tid < 64) rt_select(R.hist, R.T, RT_PASSES, tid, &S);
    if (tid < 3) s_count[tid] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * RT_CHUNK;
    int less = 0, tie_pos = 0, tie_neg = 0;
    for (int e = tid; e < RT_CHUNK; e += RT_THREADS) {
        const long long i = base + e;
        if (i >= R.A) break;
        const int s = rt_class(R.rpn_match[i]);
        if (s < 0) continue;
        const uint32_t image = dt_image(__float_as_uint(R.keys[(size_t)s * R.A + i]));
        if (s == RT_POS) {
            less += image < S.cut[RT_POS];
            tie_pos += image == S.cut[RT_POS];
        } else {
            tie_neg += image == S.cut[RT_NEG];
        }
    }
    if (less) atomicAdd(&s_count[0], less);
    if (tie_pos) atomicAdd(&s_count[1], tie_pos);
    if (tie_neg) atomicAdd(&s_count[2], tie_neg);
    __syncthreads();
    if (tid < 3) R.chunk_counts[(size_t)tid * R.chunks + blockIdx.x] = s_count[tid];
}

__global__ __launch_bounds__(RT_THREADS) void k_rt_final(const RtArgs R)
{
    __shared__ RtSelect S;
    __shared__ int s_before[3];
    __shared__ int s_wave[RT_PER_LANE][3][RT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 64) rt_select(R.hist, R.T, RT_PASSES, tid, &S);
    if (tid < 3) s_before[tid] = 0;
    __syncthreads();
    {   // the chunks before this one
        int n[3] = {0, 0, 0};
        for (int c = tid; c < (int)blockIdx.x; c += RT_THREADS)
            for (int k = 0; k < 3; k++) n[k] += R.chunk_counts[(size_t)k * R.chunks + c];
        for (int k = 0; k < 3; k++)
            if (n[k]) atomicAdd(&s_before[k], n[k]);
    }
    __syncthreads();
    const int stay[2] = {S.residual[0] + 1, S.residual[1] + 1};   // anchors AT the cut key that stay, lowest anchors first
    int tie_rank[2] = {s_before[1], s_before[2]};
    int row = s_before[0] + min(stay[RT_POS], s_before[1]);
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long base = (long long)blockIdx.x * RT_CHUNK;
    for (int round = 0; round < RT_PER_LANE; round++) {
        const long long i = base + round * RT_THREADS + tid;
        const bool valid = i < R.A;
        const int label = valid ? R.rpn_match[i] : 0;
        const int s = rt_class(label);
        uint32_t image = 0u;
        if (s >= 0) image = dt_image(__float_as_uint(R.keys[(size_t)s * R.A + i]));
        const bool tie = s >= 0 && image == S.cut[s];
        const unsigned long long t0 = __ballot(tie && s == RT_POS), t1 = __ballot(tie && s == RT_NEG);
        if (lane == 0) {
            s_wave[round][0][w] = __popcll(t0);
            s_wave[round][1][w] = __popcll(t1);
        }
        __syncthreads();
        bool keep = false;
        if (s >= 0) {
            int rank = tie_rank[s] + __popcll((s == RT_POS ? t0 : t1) & below);
            for (int v = 0; v < w; v++) rank += s_wave[round][s][v];
            keep = image < S.cut[s] || (tie && rank < stay[s]);
        }
        const bool positive = keep && s == RT_POS;
        const unsigned long long pb = __ballot(positive);
        if (lane == 0) s_wave[round][2][w] = __popcll(pb);
        if (valid && s >= 0 && !keep) R.rpn_match[i] = 0;   // :1280, :1288
        __syncthreads();
        if (positive) {
            int k = row + __popcll(pb & below);
            for (int v = 0; v < w; v++) k += s_wave[round][2][v];
            if (k < R.T) {
                const double2 lo = ((const double2*)R.anchors)[2 * i], hi = ((const double2*)R.anchors)[2 * i + 1];
                const int g = R.argmax[i];   // :1297: the closest box, which may not be the one that made the anchor positive
                const double g0 = rt_box_coord(R, g, 0), g1 = rt_box_coord(R, g, 1), g2 = rt_box_coord(R, g, 2), g3 = rt_box_coord(R, g, 3);
                // :1301-1319
                const double gt_h = g2 - g0, gt_w = g3 - g1;
                const double gt_cy = g0 + 0.5 * gt_h, gt_cx = g1 + 0.5 * gt_w;
                const double a_h = hi.x - lo.x, a_w = hi.y - lo.y;
                const double a_cy = lo.x + 0.5 * a_h, a_cx = lo.y + 0.5 * a_w;
                const double dy = (gt_cy - a_cy) / a_h, dx = (gt_cx - a_cx) / a_w;
                const double dh = log(gt_h / a_h), dw = log(gt_w / a_w);
                R.rpn_bbox[k] = make_float4((float)(dy / R.std_dev[0]), (float)(dx / R.std_dev[1]), (float)(dh / R.std_dev[2]),
                                            (float)(dw / R.std_dev[3]));   // :1404 .float()
                R.rows[k] = (int)i;
            }
        }
        for (int v = 0; v < RT_WAVES; v++) {
            tie_rank[0] += s_wave[round][0][v];
            tie_rank[1] += s_wave[round][1][v];
            row += s_wave[round][2][v];
        }
    }
    if (blockIdx.x == 0) {
        for (int k = S.kept[RT_POS] + tid; k < R.T; k += RT_THREADS) {
            R.rpn_bbox[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            R.rows[k] = -1;
        }
        if (tid < 2) R.counts[tid] = S.kept[tid];
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_rpn_targets_workspace_bytes(int A, int G, int T, size_t* out)
{
    char why[256];
    RtLayout L;
    if (!out) return fail(SDN_EINVAL, "sdn_rpn_targets_workspace_bytes: out is NULL");
    if (rt_layout(A, G, T, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_rpn_targets_workspace_bytes: %s", why);
    *out = L.total;
    return SDN_OK;
}

SDN_API int sdn_rpn_targets(const double* anchors, const void* gt_class_ids, const void* gt_boxes, const float* keys, int A, int G,
                            int ids_int64, int boxes_int32, const int32_t* gt_count, int T, const double* std_dev, int32_t* rpn_match,
                            float* rpn_bbox, int32_t* rows, int32_t* counts, void* workspace, size_t workspace_bytes, sdnStream stream)
{
    char why[256];
    if (rt_validate(anchors, gt_class_ids, gt_boxes, keys, A, G, ids_int64, gt_count, T, std_dev, rpn_match, rpn_bbox, rows, counts,
                    workspace, workspace_bytes, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_rpn_targets: %s", why);
    RtLayout L;
    if (rt_layout(A, G, T, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_rpn_targets: %s", why);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    RtArgs R;
    R.anchors = anchors;
    R.gt_class_ids = gt_class_ids;
    R.gt_boxes = gt_boxes;
    R.keys = keys;
    R.gt_count = gt_count;
    R.A = A;
    R.G = G;
    R.T = T;
    R.chunks = rt_chunks(A);
    R.ids_int64 = ids_int64 ? 1 : 0;
    R.boxes_int32 = boxes_int32 ? 1 : 0;
    for (int k = 0; k < 4; k++) R.std_dev[k] = std_dev[k];
    R.rpn_match = rpn_match;
    R.rpn_bbox = (float4*)rpn_bbox;
    R.rows = rows;
    R.counts = counts;
    R.hist = (int32_t*)(ws + L.hist);
    R.best = (int32_t*)(ws + L.best);
    R.chunk_counts = (int32_t*)(ws + L.counts);
    R.tab_image = (uint64_t*)(ws + L.tab_image);
    R.tab_anchor = (int32_t*)(ws + L.tab_anchor);
    R.argmax = (uint8_t*)(ws + L.argmax);
    const dim3 grid((unsigned)R.chunks), block(RT_THREADS);
    hipLaunchKernelGGL(k_rt_match, grid, dim3(RT_MATCH_THREADS), 0, st, R);
    hipLaunchKernelGGL(k_rt_best, dim3((unsigned)G), block, 0, st, R);
    hipLaunchKernelGGL(k_rt_label, grid, block, 0, st, R);
    for (int p = 1; p < RT_PASSES; p++) hipLaunchKernelGGL(k_rt_pass, grid, block, 0, st, R, p);
    hipLaunchKernelGGL(k_rt_ties, grid, block, 0, st, R);
    hipLaunchKernelGGL(k_rt_final, grid, block, 0, st, R);
    return check_launch("sdn_rpn_targets");
}
