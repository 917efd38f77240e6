// Mask R-CNN's detection layer for gfx950: refine_detections of the reference's geometric/maskrcnn/model.py:744-837 with
// apply_box_deltas (:307-328) and clip_to_window (:731-741) -- the step between the classifier head and the mask head, once per image.
//
// The reference takes an arg-max and two fancy gathers, decodes, scales, clips and rounds in about fifteen element-wise launches, and
// then loops in Python over the classes present: a nonzero, a sort, three gathers, an NMS whose CUDA path copies the pair mask to the
// host, a concatenation and a sorted unique per class, an intersect built from a sort, and a final sort.  Every nonzero and every NMS
// makes the host wait, and all of it produces at most D = 100 rows from N = 1000.
//
// No loop over classes is needed.  Per-class greedy NMS visits the rows of one class in descending score order, and a row's fate
// depends only on the kept rows of ITS class before it.  Put all valid rows into ONE order by (score descending, row ascending): the
// rows of every class appear in it in their per-class order, so a greedy scan whose pair test also requires EQUAL CLASS IDS decides
// every row exactly as its class's own NMS does.  The reference then takes the best D of the kept rows by score (:828) -- the first D
// the scan keeps, since it walks in score order and a later decision never changes an earlier one.  So the scan stops at D, as
// k_prop_scan stops at P.  tests/detection_layer_util.py restates both forms in numpy and a host test asserts them equal.
//
//   k_det_rows   eight lanes per row, eight rows per wave: first-index arg-max over the C classes (a NaN is the maximum, the first NaN
//                wins: torch.max on the CPU) -- each lane walks every eighth class, so the wave reads 32 contiguous bytes per row
//                and step instead of one float per lane 4 C bytes apart, and three exchanges inside the row's lanes combine the
//                candidates by the same rule.  The row's first lane then takes the class's deltas times std_dev, apply_box_deltas
//                in normalised coordinates (prop_apply_deltas of prop_device.h), times (h, w, h, w), the clamp to the window (NaN
//                stays NaN) and rintf (torch.round: half to even), all in fp32 operation by operation (this file is built without
//                FMA contraction; the decode's expf() is the only operation that can differ from the reference's CPU run).  Writes
//                class_ids, scores, boxes_px for EVERY row and the row's 64-bit key (score image high, inverted row low;
//                proposal_layer_check.h), 0 for a row that is no detection: at or behind roi_count, background, under the
//                confidence.
//   k_det_sort   ONE workgroup sorts the keys in LDS (prop_sort_keys of prop_device.h: bitonic, best first), finds the valid count
//                M (the keys that are not 0) and gathers boxes, areas, class ids and rows of the first M places.  M is never known
//                on the host.
//   k_det_mask   the pair mask over ceil(N / 64)^2 blocks; blocks at or past M leave at once.  suppresses() of nms_mask.h plus the
//                class test.
//   k_det_scan   ONE wave: the word scan of k_prop_scan (nms_scan_words of nms_mask.h) over the M rows, stopped at D; writes keep,
//                count, detections and boxes_norm with their padding.
//
// Four launches where a single fused one would be possible at N = 1000 (the whole mask, 1000 x 16 words, fits the LDS of one
// workgroup): the mask is 16 x 16 = 256 independent blocks of 64 x 64 pair tests, 136 of them on or above the diagonal, which 136
// waves on as many compute units finish in the time one workgroup of 16 waves would need for 9 blocks each; the fused form would
// trade three launch gaps of a few microseconds for that, and would not cover N > 1100.  profiles/detection_layer.md has the times.
//
// No atomics at all, no float reductions: two runs give the same bits.  Every launch goes to the caller's stream; nothing is read back.
#include <hip/hip_runtime.h>

#include "detection_layer_check.h"
#include "nms_mask.h"
#include "prop_device.h"
#include "sdn_common.h"

namespace sdn {

struct DetRows {
    const float* rois;         // [N, 4] normalised
    const float* probs;        // [N, C]
    const float* deltas;       // [N, C, 4]
    const int32_t* roi_count;  // [1] or NULL
    int N, C;
    float std_dev[4];
    float window[4];
    float height, width;
    float min_confidence;      // 0: no confidence test (:796)
    int32_t* class_ids;        // [N]
    float* scores;             // [N]
    float4* boxes_px;          // [N]
    uint64_t* keys;            // [N]
};

__global__ __launch_bounds__(DET_ROW_THREADS) void k_det_rows(const DetRows R)
{
    const int r = blockIdx.x * DET_ROWS_PER_WAVE + threadIdx.x / DET_ROW_LANES, sub = threadIdx.x % DET_ROW_LANES;
    if (r >= R.N) return;   // the DET_ROW_LANES lanes of a row leave together: the exchanges below stay inside a row's lanes
    // :760 torch.max(dim=1) on the CPU (det_argmax_takes).  Lane `sub` walks the classes sub, sub + DET_ROW_LANES, ... in that order;
    // a lane without a class keeps (-inf, INT_MAX), which loses to every class.
    const float* p = R.probs + (size_t)r * R.C;
    float score = -INFINITY;
    int cls = INT_MAX;
    for (int c = sub; c < R.C; c += DET_ROW_LANES) {
        const float v = p[c];
        if (det_argmax_takes(score, cls, v, c)) {
            score = v;
            cls = c;
        }
    }
    // the lanes' candidates into one, by the same rule
    for (int m = 1; m < DET_ROW_LANES; m <<= 1) {
        const float v = __shfl_xor(score, m, 64);
        const int c = __shfl_xor(cls, m, 64);
        if (det_argmax_takes(score, cls, v, c)) {
            score = v;
            cls = c;
        }
    }
    if (sub != 0) return;
    const float* a = R.rois + 4 * (size_t)r;
    const float* d = R.deltas + 4 * ((size_t)r * R.C + cls);
    const float ay1 = a[0], ax1 = a[1], ay2 = a[2], ax2 = a[3];
    const float d0 = d[0] * R.std_dev[0], d1 = d[1] * R.std_dev[1], d2 = d[2] * R.std_dev[2], d3 = d[3] * R.std_dev[3];   // :775
    const float4 box = prop_apply_deltas(ay1, ax1, ay2, ax2, d0, d1, d2, d3);   // apply_box_deltas, :313-326
    float y1 = box.x, x1 = box.y, y2 = box.z, x2 = box.w;
    // :782
    y1 = y1 * R.height;
    x1 = x1 * R.width;
    y2 = y2 * R.height;
    x2 = x2 * R.width;
    // clip_to_window, :736-739
    y1 = prop_clamp(y1, R.window[0], R.window[2]);
    x1 = prop_clamp(x1, R.window[1], R.window[3]);
    y2 = prop_clamp(y2, R.window[0], R.window[2]);
    x2 = prop_clamp(x2, R.window[1], R.window[3]);
    // :788 torch.round: half to even
    y1 = rintf(y1);
    x1 = rintf(x1);
    y2 = rintf(y2);
    x2 = rintf(x2);
    R.class_ids[r] = cls;
    R.scores[r] = score;
    R.boxes_px[r] = make_float4(y1, x1, y2, x2);
    int limit = R.N;
    if (R.roi_count) limit = min(max(*R.roi_count, 0), R.N);
    bool valid = r < limit && cls > 0;                                                   // :793
    if (R.min_confidence != 0.0f) valid = valid && score >= R.min_confidence;            // :796-797
    R.keys[r] = valid ? prop_key(prop_image(__float_as_uint(score)), (uint32_t)r) : 0ull;   // 0 sorts behind every key
}

struct DetSort {
    const uint64_t* keys;       // [N]
    const int32_t* class_ids;   // [N]
    const float4* boxes_px;     // [N]
    int N, S;                   // S: the sorting network's size, a power of two >= N
    int32_t* head;              // [0] = M
    float4* boxes;              // [N] in score order, the first M written
    float* areas;
    int32_t* classes;
    int32_t* rows;
};

__global__ __launch_bounds__(DET_SORT_THREADS) void k_det_sort(const DetSort D)
{
    __shared__ uint64_t s[DET_MAX_ROIS];
    const int tid = threadIdx.x;
    for (int i = tid; i < D.S; i += DET_SORT_THREADS) s[i] = i < D.N ? D.keys[i] : 0ull;
    __syncthreads();
    prop_sort_keys(s, D.S, tid, DET_SORT_THREADS);
    if (tid == 0 && s[0] == 0ull) D.head[0] = 0;
    for (int r = tid; r < D.N; r += DET_SORT_THREADS) {
        const uint64_t key = s[r];
        if (key == 0ull) continue;
        if (r + 1 == D.N || s[r + 1] == 0ull) D.head[0] = r + 1;   // exactly one place is the last valid one (s has S >= N entries)
        const uint32_t row = prop_key_index(key);
        const float4 b = D.boxes_px[row];
        D.boxes[r] = b;
        D.areas[r] = (b.w - b.y + 1.0f) * (b.z - b.x + 1.0f);   // pth_nms.py:32
        D.classes[r] = D.class_ids[row];
        D.rows[r] = (int32_t)row;
    }
}

// mask [N, nb] over the first M = head[0] places of the score order: bit c of word (i, bx) is set when place i suppresses place
// j = 64 bx + c > i, which takes equal class ids.  Only the words (i < M, bx < ceil(M / 64)) are written; the scan reads no others.
__global__ __launch_bounds__(64) void k_det_mask(const float4* __restrict__ boxes, const float* __restrict__ areas,
                                                 const int32_t* __restrict__ classes, const int32_t* __restrict__ head, float thresh,
                                                 unsigned long long* __restrict__ mask, int nb, int strict)
{
    __shared__ float4 cb[64];
    __shared__ float ca[64];
    __shared__ int cc[64];
    const int n = head[0];
    const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64, lane = threadIdx.x;
    if (row0 >= n || col0 >= n) return;
    if (col0 + 63 <= row0 && blockIdx.x != blockIdx.y) {  // every column precedes every row: nothing to suppress
        if (row0 + lane < n) mask[(size_t)(row0 + lane) * nb + blockIdx.x] = 0ull;
        return;
    }
    if (col0 + lane < n) {
        cb[lane] = boxes[col0 + lane];
        ca[lane] = areas[col0 + lane];
        cc[lane] = classes[col0 + lane];
    }
    __syncthreads();
    const int i = row0 + lane;
    if (i >= n) return;
    const float4 bi = boxes[i];
    const float ai = areas[i];
    const int ci = classes[i];
    const int cols = min(64, n - col0);
    unsigned long long t = 0ull;
    for (int c = 0; c < cols; c++) {
        const int j = col0 + c;
        if (j <= i || cc[c] != ci) continue;
        if (suppresses(bi, ai, cb[c], ca[c], thresh, strict)) t |= 1ull << c;
    }
    mask[(size_t)i * nb + blockIdx.x] = t;
}

struct DetScan {
    const unsigned long long* mask;   // [N, nb]
    const int32_t* head;              // [0] = M
    const float4* boxes;              // [N] in score order
    const int32_t* classes;
    const int32_t* rows;
    const float* scores;              // [N] by row
    int nb, D;
    float height, width;
    int32_t* keep;                    // [D]
    int32_t* count;                   // [1]
    float* detections;                // [D, 6]
    float4* boxes_norm;               // [D]
};

__global__ __launch_bounds__(64) void k_det_scan(const DetScan S)
{
    __shared__ unsigned long long remv[DET_MAX_WORDS];
    __shared__ int s_keep[DET_MAX_INSTANCES];
    const int lane = threadIdx.x;
    const int D = S.D;
    const int kept = nms_scan_words(S.mask, S.nb, S.head[0], D, remv, s_keep);   // M = head[0] rows take part
    if (lane == 0) *S.count = kept;
    for (int r = lane; r < D; r += 64) {
        float* det = S.detections + 6 * (size_t)r;
        if (r < kept) {
            const int k = s_keep[r];
            const int row = S.rows[k];
            const float4 b = S.boxes[k];
            S.keep[r] = row;
            det[0] = b.x;
            det[1] = b.y;
            det[2] = b.z;
            det[3] = b.w;
            det[4] = (float)S.classes[k];   // :834
            det[5] = S.scores[row];
            S.boxes_norm[r] = make_float4(b.x / S.height, b.y / S.width, b.z / S.height, b.w / S.width);   // :1769: a division
        } else {
            S.keep[r] = -1;
            for (int k = 0; k < 6; k++) det[k] = 0.0f;
            S.boxes_norm[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_detection_layer_workspace_bytes(int N, int C, int D, size_t* out)
{
    char why[256];
    DetLayout L;
    if (!out) return fail(SDN_EINVAL, "sdn_detection_layer_workspace_bytes: out is NULL");
    if (det_layout(N, C, D, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_detection_layer_workspace_bytes: %s", why);
    *out = L.total;
    return SDN_OK;
}

SDN_API int sdn_detection_layer(const float* rois, const float* probs, const float* deltas, int N, int C, const float* window,
                                const float* std_dev, int height, int width, float min_confidence, float nms_threshold, int D, int strict,
                                const int32_t* roi_count, int32_t* class_ids, float* scores, float* boxes_px, int32_t* keep, int32_t* count,
                                float* detections, float* boxes_norm, void* workspace, size_t workspace_bytes, sdnStream stream)
{
    char why[256];
    if (det_validate(rois, probs, deltas, N, C, window, std_dev, height, width, D, roi_count, class_ids, scores, boxes_px, keep, count,
                     detections, boxes_norm, workspace, workspace_bytes, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_detection_layer: %s", why);
    DetLayout L;
    if (det_layout(N, C, D, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_detection_layer: %s", why);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* head = (int32_t*)(ws + L.head);
    DetRows R;
    R.rois = rois;
    R.probs = probs;
    R.deltas = deltas;
    R.roi_count = roi_count;
    R.N = N;
    R.C = C;
    for (int k = 0; k < 4; k++) {
        R.std_dev[k] = std_dev[k];
        R.window[k] = window[k];
    }
    R.height = (float)height;
    R.width = (float)width;
    R.min_confidence = min_confidence;
    R.class_ids = class_ids;
    R.scores = scores;
    R.boxes_px = (float4*)boxes_px;
    R.keys = (uint64_t*)(ws + L.keys);
    hipLaunchKernelGGL(k_det_rows, dim3((unsigned)((N + DET_ROWS_PER_WAVE - 1) / DET_ROWS_PER_WAVE)), dim3(DET_ROW_THREADS), 0, st, R);
    DetSort S;
    S.keys = R.keys;
    S.class_ids = class_ids;
    S.boxes_px = R.boxes_px;
    S.N = N;
    S.S = prop_sort_size(N);
    S.head = head;
    S.boxes = (float4*)(ws + L.boxes);
    S.areas = (float*)(ws + L.areas);
    S.classes = (int32_t*)(ws + L.classes);
    S.rows = (int32_t*)(ws + L.rows);
    hipLaunchKernelGGL(k_det_sort, dim3(1), dim3(DET_SORT_THREADS), 0, st, S);
    if (int rc = check_launch("sdn_detection_layer: rows and sort")) return rc;
    const int nb = prop_words(N);
    unsigned long long* mask = (unsigned long long*)(ws + L.mask);
    hipLaunchKernelGGL(k_det_mask, dim3(nb, nb), dim3(64), 0, st, (const float4*)S.boxes, (const float*)S.areas, (const int32_t*)S.classes,
                       (const int32_t*)head, nms_threshold, mask, nb, strict ? 1 : 0);
    DetScan Q;
    Q.mask = mask;
    Q.head = head;
    Q.boxes = S.boxes;
    Q.classes = S.classes;
    Q.rows = S.rows;
    Q.scores = scores;
    Q.nb = nb;
    Q.D = D;
    Q.height = R.height;
    Q.width = R.width;
    Q.keep = keep;
    Q.count = count;
    Q.detections = detections;
    Q.boxes_norm = (float4*)boxes_norm;
    hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(64), 0, st, Q);
    return check_launch("sdn_detection_layer");
}
