// Mask R-CNN's proposal layer for gfx950: proposal_layer of the reference's geometric/maskrcnn/model.py:344-407 with apply_box_deltas
// (:307-328) and clip_boxes (:331-341) -- the step between the RPN heads and pyramid_roi_align, once per image.
//
// The reference sorts all A anchor scores, gathers three times, decodes and clips in about twenty element-wise launches and runs an
// NMS whose CUDA path copies the pair mask to the host.  Only the K = min(pre_nms_limit, A) best scores are needed (6000 of 261 888
// for a 1024 x 1024 image) and no step needs the host:
//
//   k_prop_hist x 4  exact radix select of the K-th largest score: a 256-bin histogram per byte of the score's order-preserving
//                    integer image (proposal_layer_check.h: prop_image), most significant byte first.  Every workgroup of pass p
//                    re-derives the prefix from the finished histograms of the passes before it (ids_find of rank_select.h), so no
//                    workgroup waits for another.  The fg column is read in place with stride 2.
//   k_prop_ties      scores equal to the threshold T, counted per chunk of PROP_CHUNK anchors.
//   k_prop_compact   the K survivors as 64-bit keys (image high, inverted index low): every score above T, and of the scores equal to
//                    T the `need` lowest indices -- a tie's ordinal is the ties of the chunks before it, re-added, plus an ordered
//                    prefix inside the chunk.  The keys are unique, so their order in the buffer does not matter.
//   k_prop_sort      ONE workgroup sorts the keys in LDS (prop_sort_keys of prop_device.h: bitonic, best first:
//                    torch.sort(descending=True, stable=True)), writes `order`, gathers the anchor and delta rows, decodes
//                    (prop_apply_deltas of prop_device.h) and clips operation by operation in fp32 (this file is built without FMA
//                    contraction; the decode's expf() is the only operation that can differ from the reference's CPU run) and
//                    writes boxes_px and the areas.
//   k_prop_mask      the pair mask of raster_boxes.hip's NMS (nms_mask.h), over the K boxes.
//   k_prop_scan      ONE wave walks the boxes word by word (nms_scan_words of nms_mask.h, shared with detection_layer.hip) until P
//                    are kept, and writes keep, count and rois with their padding.
//
// Integer atomics build the histograms and hand out compaction slots; both are order-independent in what they produce, so two runs
// give the same bits.  Every launch goes to the caller's stream; nothing is read back.
#include "nms_mask.h"
#include "prop_device.h"
#include "proposal_layer_check.h"
#include "rank_select.h"
#include "sdn_common.h"

namespace sdn {

struct PropSelect {
    const float* probs;   // [A, 2]: (bg, fg)
    int A, K;
    int32_t* head;        // PROP_HEAD_INTS: hist[4][256], cursor
    int32_t* ties;        // [chunks]
    uint64_t* keys;       // [K]
};

constexpr int PROP_CURSOR = 4 * 256;

__device__ __forceinline__ uint32_t prop_score_image(const float* __restrict__ probs, int i)
{
    return prop_image(__float_as_uint(probs[2 * (size_t)i + 1]));
}

// One wave: the leading `passes` bytes of the K-th largest image and its ascending rank among the scores that share them.
__device__ __forceinline__ void prop_prefix(const int32_t* head, int A, int K, int passes, int lane, uint32_t* prefix, int* rank)
{
    long r = (long)A - K;
    uint32_t p = 0;
    for (int q = 0; q < passes; q++) {
        int bin, res;
        ids_find(head + 256 * q, r, lane, &bin, &res);
        p = (p << 8) | (uint32_t)bin;
        r = res;
    }
    *prefix = p;
    *rank = (int)r;
}

// Zeroes the histograms and the cursor.  A kernel, not hipMemsetAsync: the call is then a plain chain of kernel launches, which a
// captured graph replays in order (a replay that left the head of the previous replay in place selected fewer than K keys).
__global__ __launch_bounds__(PROP_THREADS) void k_prop_clear(int32_t* __restrict__ head)
{
    for (int i = threadIdx.x; i < PROP_HEAD_INTS; i += PROP_THREADS) head[i] = 0;
}

__global__ __launch_bounds__(PROP_THREADS) void k_prop_hist(const PropSelect S, const int pass)
{
    __shared__ int h[256];
    __shared__ uint32_t s_prefix;
    const int tid = threadIdx.x;
    h[tid] = 0;
    if (tid < 64) {
        uint32_t prefix;
        int rank;
        prop_prefix(S.head, S.A, S.K, pass, tid, &prefix, &rank);
        if (tid == 0) s_prefix = prefix;
    }
    __syncthreads();
    const uint32_t prefix = s_prefix;
    const int base = blockIdx.x * PROP_CHUNK;
    for (int k = 0; k < PROP_CHUNK / PROP_THREADS; k++) {
        const int i = base + k * PROP_THREADS + tid;
        if (i >= S.A) break;
        const uint32_t img = prop_score_image(S.probs, i);
        if (pass == 0 || (img >> (32 - 8 * pass)) == prefix) atomicAdd(&h[(img >> (24 - 8 * pass)) & 255u], 1);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&S.head[256 * pass + tid], h[tid]);
}

__global__ __launch_bounds__(PROP_THREADS) void k_prop_ties(const PropSelect S)
{
    __shared__ uint32_t s_T;
    __shared__ int s_n;
    const int tid = threadIdx.x;
    if (tid < 64) {
        uint32_t T;
        int rank;
        prop_prefix(S.head, S.A, S.K, 4, tid, &T, &rank);
        if (tid == 0) {
            s_T = T;
            s_n = 0;
        }
    }
    __syncthreads();
    const uint32_t T = s_T;
    const int base = blockIdx.x * PROP_CHUNK + 4 * tid;
    int c = 0;
    for (int k = 0; k < 4; k++)
        if (base + k < S.A && prop_score_image(S.probs, base + k) == T) c++;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((tid & 63) == 0 && c) atomicAdd(&s_n, c);
    __syncthreads();
    if (tid == 0) S.ties[blockIdx.x] = s_n;
}

__global__ __launch_bounds__(PROP_THREADS) void k_prop_compact(const PropSelect S)
{
    __shared__ uint32_t s_T;
    __shared__ int s_need, s_before, s_count, s_base;
    __shared__ int s_wave[PROP_THREADS / 64];
    __shared__ uint64_t s_list[PROP_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {
        uint32_t T;
        int rank;
        prop_prefix(S.head, S.A, S.K, 4, tid, &T, &rank);
        if (tid == 0) {
            s_T = T;
            s_need = S.head[256 * 3 + (int)(T & 255u)] - rank;   // of the scores equal to T, the `need` lowest indices are selected
            s_before = 0;
            s_count = 0;
        }
    }
    __syncthreads();
    const uint32_t T = s_T;
    const int need = s_need;
    // ties of the chunks before this one
    int before = 0;
    for (int j = tid; j < (int)blockIdx.x; j += PROP_THREADS) before += S.ties[j];
    for (int d = 32; d > 0; d >>= 1) before += __shfl_down(before, d, 64);
    if (lane == 0 && before) atomicAdd(&s_before, before);
    // this thread's four consecutive anchors
    const int base = blockIdx.x * PROP_CHUNK + 4 * tid;
    uint32_t img[4];
    int mine = 0;
    for (int k = 0; k < 4; k++) {
        img[k] = base + k < S.A ? prop_score_image(S.probs, base + k) : 0u;   // image 0 is no score's image
        if (base + k < S.A && img[k] == T) mine++;
    }
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int ordinal = s_before + incl - mine;
    for (int w = 0; w < wave; w++) ordinal += s_wave[w];
    for (int k = 0; k < 4; k++) {
        if (base + k >= S.A) break;
        bool take = img[k] > T;
        if (img[k] == T) {
            take = ordinal < need;
            ordinal++;
        }
        if (take) s_list[atomicAdd(&s_count, 1)] = prop_key(img[k], (uint32_t)(base + k));
    }
    __syncthreads();
    const int count = s_count;
    if (tid == 0 && count) s_base = atomicAdd(&S.head[PROP_CURSOR], count);
    __syncthreads();
    if (!count) return;
    const int at = s_base;
    for (int p = tid; p < count; p += PROP_THREADS)
        if (at + p < S.K) S.keys[at + p] = s_list[p];   // exactly K are selected; the bound only keeps a broken count inside the buffer
}

struct PropDecode {
    const uint64_t* keys;    // [K] unsorted
    const float* deltas;     // [A, 4]
    const float* anchors;    // [A, 4]
    uint32_t A;
    float std_dev[4];
    float height, width;
    int K, N;                // N: the sorting network's size, a power of two >= K
    int32_t* order;          // [K]
    float4* boxes_px;        // [K]
    float* areas;            // [K]
};

__global__ __launch_bounds__(PROP_SORT_THREADS) void k_prop_sort(const PropDecode D)
{
    __shared__ uint64_t s[PROP_MAX_PRE_NMS];
    const int tid = threadIdx.x;
    for (int i = tid; i < D.N; i += PROP_SORT_THREADS) s[i] = i < D.K ? D.keys[i] : 0ull;   // 0 sorts behind every key
    __syncthreads();
    prop_sort_keys(s, D.N, tid, PROP_SORT_THREADS);
    for (int r = tid; r < D.K; r += PROP_SORT_THREADS) {
        uint32_t idx = prop_key_index(s[r]);
        if (idx >= D.A) idx = D.A - 1u;   // every selected key names an anchor; the bound only keeps a broken key inside the buffers
        D.order[r] = (int32_t)idx;
        const float* a = D.anchors + 4 * (size_t)idx;
        const float* d = D.deltas + 4 * (size_t)idx;
        const float ay1 = a[0], ax1 = a[1], ay2 = a[2], ax2 = a[3];
        const float d0 = d[0] * D.std_dev[0], d1 = d[1] * D.std_dev[1], d2 = d[2] * D.std_dev[2], d3 = d[3] * D.std_dev[3];   // :370
        const float4 box = prop_apply_deltas(ay1, ax1, ay2, ax2, d0, d1, d2, d3);   // apply_box_deltas, :313-326
        float y1 = box.x, x1 = box.y, y2 = box.z, x2 = box.w;
        // clip_boxes, :336-340
        y1 = prop_clamp(y1, 0.0f, D.height);
        x1 = prop_clamp(x1, 0.0f, D.width);
        y2 = prop_clamp(y2, 0.0f, D.height);
        x2 = prop_clamp(x2, 0.0f, D.width);
        D.boxes_px[r] = make_float4(y1, x1, y2, x2);
        D.areas[r] = (x2 - x1 + 1.0f) * (y2 - y1 + 1.0f);   // pth_nms.py:32
    }
}

__global__ __launch_bounds__(64) void k_prop_mask(const float4* __restrict__ boxes, const float* __restrict__ areas, int n, float thresh,
                                                  unsigned long long* __restrict__ mask, int nb, int strict)
{
    __shared__ float4 cb[64];
    __shared__ float ca[64];
    nms_mask_block(boxes, areas, n, thresh, mask, nb, strict, cb, ca);
}

constexpr int PROP_MAX_WORDS = PROP_MAX_PRE_NMS / 64;

// mask [K, nb] of k_prop_mask; boxes_px [K]; keep [P], count [1], rois [P]
__global__ __launch_bounds__(64) void k_prop_scan(const unsigned long long* __restrict__ mask, const float4* __restrict__ boxes_px, int K, int nb,
                                                  int P, float height, float width, int32_t* __restrict__ keep, int32_t* __restrict__ count,
                                                  float4* __restrict__ rois)
{
    __shared__ unsigned long long remv[PROP_MAX_WORDS];
    __shared__ int s_keep[PROP_MAX_PRE_NMS];
    const int lane = threadIdx.x;
    const int kept = nms_scan_words(mask, nb, K, P, remv, s_keep);   // every row takes part: prop_words(K) == nb
    if (lane == 0) *count = kept;
    for (int r = lane; r < P; r += 64) {
        if (r < kept) {
            const int k = s_keep[r];
            const float4 b = boxes_px[k];
            keep[r] = k;
            rois[r] = make_float4(b.x / height, b.y / width, b.z / height, b.w / width);   // :402: a division, not a reciprocal multiply
        } else {
            keep[r] = -1;
            rois[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_proposal_layer_workspace_bytes(int A, int K, int P, size_t* out)
{
    char why[256];
    PropLayout L;
    if (!out) return fail(SDN_EINVAL, "sdn_proposal_layer_workspace_bytes: out is NULL");
    if (prop_layout(A, K, P, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_proposal_layer_workspace_bytes: %s", why);
    *out = L.total;
    return SDN_OK;
}

SDN_API int sdn_proposal_layer(const float* rpn_probs, const float* rpn_bbox, const float* anchors, int A, const float* std_dev, int height,
                               int width, int K, int P, float nms_threshold, int strict, int32_t* order, float* boxes_px, int32_t* keep,
                               int32_t* count, float* rois, void* workspace, size_t workspace_bytes, sdnStream stream)
{
    char why[256];
    if (prop_validate(rpn_probs, rpn_bbox, anchors, A, std_dev, height, width, K, P, order, boxes_px, keep, count, rois, workspace,
                      workspace_bytes, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_proposal_layer: %s", why);
    PropLayout L;
    if (prop_layout(A, K, P, &L, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_proposal_layer: %s", why);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    PropSelect S;
    S.probs = rpn_probs;
    S.A = A;
    S.K = K;
    S.head = (int32_t*)(ws + L.head);
    S.ties = (int32_t*)(ws + L.ties);
    S.keys = (uint64_t*)(ws + L.keys);
    float* areas = (float*)(ws + L.areas);
    unsigned long long* mask = (unsigned long long*)(ws + L.mask);
    hipLaunchKernelGGL(k_prop_clear, dim3(1), dim3(PROP_THREADS), 0, st, S.head);
    const unsigned chunks = (unsigned)prop_chunks(A);
    for (int pass = 0; pass < 4; pass++) hipLaunchKernelGGL(k_prop_hist, dim3(chunks), dim3(PROP_THREADS), 0, st, S, pass);
    hipLaunchKernelGGL(k_prop_ties, dim3(chunks), dim3(PROP_THREADS), 0, st, S);
    hipLaunchKernelGGL(k_prop_compact, dim3(chunks), dim3(PROP_THREADS), 0, st, S);
    if (int rc = check_launch("sdn_proposal_layer: selection")) return rc;
    PropDecode D;
    D.keys = S.keys;
    D.deltas = rpn_bbox;
    D.anchors = anchors;
    D.A = (uint32_t)A;
    for (int k = 0; k < 4; k++) D.std_dev[k] = std_dev[k];
    D.height = (float)height;
    D.width = (float)width;
    D.K = K;
    D.N = prop_sort_size(K);
    D.order = order;
    D.boxes_px = (float4*)boxes_px;
    D.areas = areas;
    hipLaunchKernelGGL(k_prop_sort, dim3(1), dim3(PROP_SORT_THREADS), 0, st, D);
    const int nb = prop_words(K);
    hipLaunchKernelGGL(k_prop_mask, dim3(nb, nb), dim3(64), 0, st, (const float4*)boxes_px, (const float*)areas, K, nms_threshold, mask, nb,
                       strict ? 1 : 0);
    hipLaunchKernelGGL(k_prop_scan, dim3(1), dim3(64), 0, st, (const unsigned long long*)mask, (const float4*)boxes_px, K, nb, P, D.height,
                       D.width, keep, count, (float4*)rois);
    return check_launch("sdn_proposal_layer");
}
