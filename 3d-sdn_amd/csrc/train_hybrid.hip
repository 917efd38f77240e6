// The training items of the real-image sets and of the hybrid batches of the geometric branch (geometric/derender3d/
// datasets.py:549-606 KittiObject, :737-769 KittiSemantics, :930-971 CityscapesSemantics, :1077-1112 CityscapesMaskRCNN beside
// :332-420 VKitti; data_loader.py:17-37 collate_fn).  A batch mixes frames of several sizes, two normalisations, masks from a
// colour code or from an instance-id map, and ignore maps from nearer codes, from a disparity percentile, or all zero.
//   sdn_train_id_stats      CityscapesSemantics.__getitem__ :938-955 for B items over several frames in one chain of five
//                           launches: area, mask_to_roi's box, the count n of non-zero disparities under the mask and the two
//                           order statistics np.percentile(., 95) interpolates between.  The exact two-level radix select of
//                           scene_ids.hip, per ITEM (one id of one frame) instead of per id of one frame: blockIdx.y is the
//                           item, its 256-bin histograms live in the workgroup's LDS and are added once to global memory.
//                           Integer atomics only; nothing goes to the host.
//   sdn_train_crops_mixed   the kernel body of k_train_crops (train_items_common.h: ti_crops_body, instantiated here on a
//                           per-item source) with every per-call quantity moved into the item row: the frame's address and
//                           size, the sources of the mask and of the ignore map, mean and std.  A plane without a source is
//                           written as 0.0 by its workgroups, without staging.
// The id and disparity maps are 4-byte elements: the lanes of a wave read consecutive pixels of a source row, one dword each.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "rank_select.h"
#include "sdn_common.h"
#include "train_hybrid_check.h"
#include "train_items_common.h"

namespace sdn {

static_assert(MX_SRC_PIXELS == TI_SRC_PIXELS && MX_PLANE_BYTES == TI_PLANE_BYTES && MX_MAX_CONTRAST_SIDE == TI_MAX_CONTRAST_SIDE &&
              MX_OBJ_INTS == TI_OBJ_INTS, "the validator's constants are the kernels'");

// ---- statistics of B (frame, id) items -----------------------------------------------------------------------------------------
constexpr int TID_COLS = 8;                          // area, y0, x0, y1, x1, n, lo, hi
constexpr int TID_BINS = 256;
constexpr int TID_THREADS = 256;
constexpr int TID_ITERS = 8;
constexpr int TID_CHUNK = TID_THREADS * TID_ITERS;   // pixels of one pass of a workgroup, consecutive
constexpr int TID_ITEM_INTS = 8;
// the workspace, in ints: high-byte histograms [B][256], the select records [B][4], low-byte histograms [B][2][256]
constexpr size_t TID_WS_PER_ITEM = TID_BINS + 4 + 2 * TID_BINS;
static_assert(TID_THREADS == TID_BINS, "a workgroup flushes one bin per thread");

struct IdItem {   // one row of the item table, 8 ints
    uint64_t ids;          // address of the int32 [H, W] id map
    uint64_t disparity;    // address of the int32 [H, W] disparity map, or 0
    int H, W;
    int id;
    int pad;
};
static_assert(sizeof(IdItem) == TID_ITEM_INTS * sizeof(int32_t), "id item row");

__global__ __launch_bounds__(256) void k_tid_init(int32_t* table, int32_t* ws, int B)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * TID_WS_PER_ITEM) ws[i] = 0;
    if (i < (size_t)B * TID_COLS) {
        const int c = (int)(i & 7);
        table[i] = (c == 1 || c == 2) ? INT_MAX : 0;   // the invalid roi of sdn_scene_id_stats
    }
}

__global__ __launch_bounds__(TID_THREADS) void k_tid_range(const IdItem* __restrict__ items, int* bad)
{
    const IdItem it = items[blockIdx.y];
    const int32_t* disp = reinterpret_cast<const int32_t*>(it.disparity);
    if (!disp || it.H < 1 || it.W < 1) return;
    const long HW = (long)it.H * it.W;
    for (long p = (long)blockIdx.x * TID_THREADS + threadIdx.x; p < HW; p += (long)gridDim.x * TID_THREADS)
        if (disp[p] < 0 || disp[p] > 65535) atomicAdd(bad, 1);
}

// blockIdx.y is the item; a workgroup walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of its frame.  Thread t holds
// the pixels chunk + k 256 + t: the lanes of a wave are 64 neighbours, which mostly share the high byte of their disparity:
// they are grouped by ballot on equal bins and a group adds once into the LDS histogram.
__global__ __launch_bounds__(TID_THREADS) void k_tid_pass_a(const IdItem* __restrict__ items, int32_t* table, int32_t* hist_hi)
{
    __shared__ int s_hist[TID_BINS];
    __shared__ int s_stat[6];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const IdItem it = items[b];
    const int32_t* ids = reinterpret_cast<const int32_t*>(it.ids);
    const int32_t* disp = reinterpret_cast<const int32_t*>(it.disparity);
    if (!ids || it.H < 1 || it.W < 1) return;   // uniform over the workgroup; the row stays empty
    const long HW = (long)it.H * it.W;
    if ((long)blockIdx.x * TID_CHUNK >= HW) return;
    s_hist[tid] = 0;
    if (tid == 0) {
        s_stat[0] = 0; s_stat[1] = INT_MAX; s_stat[2] = INT_MAX; s_stat[3] = 0; s_stat[4] = 0; s_stat[5] = 0;
    }
    __syncthreads();
    int area = 0, ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1, n = 0;
    for (long c0 = (long)blockIdx.x * TID_CHUNK; c0 < HW; c0 += (long)gridDim.x * TID_CHUNK) {   // uniform over the workgroup
        for (int k = 0; k < TID_ITERS; k++) {
            const long p = c0 + (long)k * TID_THREADS + tid;
            const bool mine = p < HW && ids[p] == it.id;
            const int d = (mine && disp) ? disp[p] : 0;
            if (mine) {
                const unsigned up = (unsigned)p;   // H W fits an int (the launcher's max_pixels; the host checks)
                const int y = (int)(up / (unsigned)it.W), x = (int)(up - (unsigned)y * (unsigned)it.W);
                ymin = min(ymin, y); xmin = min(xmin, x); ymax = max(ymax, y); xmax = max(xmax, x);
                area++;
            }
            const bool nz = mine && d != 0;
            n += nz ? 1 : 0;
            const int bin = (d >> 8) & (TID_BINS - 1);   // the mask keeps a value outside 0 .. 65535 (a broken precondition) in bounds
            unsigned long long left = __ballot(nz);
            while (left) {   // one round per distinct high byte among the wave's 64 pixels
                const int src = __ffsll((long long)left) - 1;
                const int b0 = __shfl(bin, src, 64);
                const unsigned long long mb = __ballot(nz && bin == b0);
                left &= ~mb;
                if (lane == src) atomicAdd(&s_hist[b0], __popcll(mb));
            }
        }
    }
    area = wave_sum(area);
    n = wave_sum(n);
    ymin = wave_imin(ymin); xmin = wave_imin(xmin); ymax = wave_imax(ymax); xmax = wave_imax(xmax);
    if (lane == 0 && area) {
        atomicAdd(&s_stat[0], area);
        atomicMin(&s_stat[1], ymin);
        atomicMin(&s_stat[2], xmin);
        atomicMax(&s_stat[3], ymax + 1);
        atomicMax(&s_stat[4], xmax + 1);
        atomicAdd(&s_stat[5], n);
    }
    __syncthreads();
    if (!s_stat[0]) return;   // uniform: no pixel of the item in this workgroup's chunks
    if (tid == 0) {
        int32_t* row = table + TID_COLS * (size_t)b;
        atomicAdd(row, s_stat[0]);
        atomicMin(row + 1, s_stat[1]);
        atomicMin(row + 2, s_stat[2]);
        atomicMax(row + 3, s_stat[3]);
        atomicMax(row + 4, s_stat[4]);
        if (s_stat[5]) atomicAdd(row + 5, s_stat[5]);
    }
    const int c = s_hist[tid];
    if (c) atomicAdd(hist_hi + (size_t)b * TID_BINS + tid, c);
}

__global__ __launch_bounds__(64) void k_tid_select(const int32_t* __restrict__ table, const int32_t* __restrict__ hist_hi, int32_t* sel)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const long n = table[TID_COLS * (size_t)b + 5];
    int4 out = make_int4(-1, 0, -1, 0);
    if (n > 0) {   // uniform over the wave
        const long i = (19 * (n - 1)) / 20;   // floor((n - 1) 0.95), in integers
        const long i1 = min(i + 1, n - 1);
        ids_find(hist_hi + (size_t)b * TID_BINS, i, lane, &out.x, &out.y);
        ids_find(hist_hi + (size_t)b * TID_BINS, i1, lane, &out.z, &out.w);
    }
    if (lane == 0) reinterpret_cast<int4*>(sel)[b] = out;
}

__global__ __launch_bounds__(TID_THREADS) void k_tid_pass_b(const IdItem* __restrict__ items, const int32_t* __restrict__ sel,
                                                            int32_t* hist_lo)
{
    __shared__ int s_lo[2][TID_BINS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const IdItem it = items[b];
    const int32_t* ids = reinterpret_cast<const int32_t*>(it.ids);
    const int32_t* disp = reinterpret_cast<const int32_t*>(it.disparity);
    const int4 rec = reinterpret_cast<const int4*>(sel)[b];
    if (!ids || !disp || it.H < 1 || it.W < 1 || rec.x < 0) return;   // uniform; rec.x < 0: n == 0
    const long HW = (long)it.H * it.W;
    if ((long)blockIdx.x * TID_CHUNK >= HW) return;
    s_lo[0][tid] = 0;
    s_lo[1][tid] = 0;
    __syncthreads();
    for (long c0 = (long)blockIdx.x * TID_CHUNK; c0 < HW; c0 += (long)gridDim.x * TID_CHUNK)
        for (int k = 0; k < TID_ITERS; k++) {
            const long p = c0 + (long)k * TID_THREADS + tid;
            if (p >= HW || ids[p] != it.id) continue;
            const int d = disp[p];
            if (d == 0) continue;
            const int bin = (d >> 8) & (TID_BINS - 1), low = d & (TID_BINS - 1);
            const int w = bin == rec.x ? 0 : (bin == rec.z ? 1 : -1);   // rec.z == rec.x: one histogram serves both ranks
            if (w >= 0) atomicAdd(&s_lo[w][low], 1);   // the low bytes inside a bin are spread: every pixel adds for itself
        }
    __syncthreads();
    for (int w = 0; w < 2; w++) {
        const int c = s_lo[w][tid];
        if (c) atomicAdd(hist_lo + ((size_t)b * 2 + w) * TID_BINS + tid, c);
    }
}

__global__ __launch_bounds__(64) void k_tid_pick(int32_t* table, const int32_t* __restrict__ sel, const int32_t* __restrict__ hist_lo)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (table[TID_COLS * (size_t)b + 5] <= 0) return;   // lo = hi = 0 (k_tid_init)
    const int4 rec = reinterpret_cast<const int4*>(sel)[b];
    int b_lo, b_hi, unused;
    ids_find(hist_lo + ((size_t)b * 2) * TID_BINS, rec.y, lane, &b_lo, &unused);
    ids_find(hist_lo + ((size_t)b * 2 + (rec.z != rec.x ? 1 : 0)) * TID_BINS, rec.w, lane, &b_hi, &unused);
    if (lane == 0) {
        table[TID_COLS * (size_t)b + 6] = (rec.x << 8) | b_lo;
        table[TID_COLS * (size_t)b + 7] = (rec.z << 8) | b_hi;
    }
}

// ---- the crops -----------------------------------------------------------------------------------------------------------------
struct MixParams {
    const TrainWin* objs;
    const MixItem* items;
    const int32_t* bounds;
    const int32_t* kk8;
    const uint8_t* nearer;     // [total, 3]
    unsigned long long* lsum;  // [B] sum of L over the window (items with contrast)
    int B, Si, Sm;
    float *images, *masks, *ignores;
};

__device__ __forceinline__ TrainItem mx_jitter_of(const MixItem& it)
{
    TrainItem j;
    j.frame = 0; j.code = 0; j.near_off = 0; j.near_cnt = 0;
    j.nops = it.nops; j.order = it.order;
    j.fb = it.fb; j.fc = it.fc; j.fs = it.fs;
    j.hue = it.hue;
    j.pad0 = j.pad1 = 0;
    return j;
}

// 0: beyond the padded image (PIL's crop gives 0), 1: padding (the fill value), 2: inside the frame, *p its offset in a plane
__device__ __forceinline__ int mx_where(const MixItem& it, const TrainWin& o, int wy, int wx, size_t* p)
{
    const int fy = o.oy + wy, fx = o.ox + wx;
    if (fx >= o.xlim || fy >= o.ylim) return 0;
    if ((unsigned)fy >= (unsigned)it.H || (unsigned)fx >= (unsigned)it.W) return 1;
    *p = (size_t)fy * it.W + fx;
    return 2;
}

__device__ __forceinline__ void mx_raw_rgb(const MixItem& it, const TrainWin& o, int wy, int wx, int& r, int& g, int& b)
{
    size_t p = 0;
    const int w = mx_where(it, o, wy, wx, &p);
    if (w < 2) {
        r = g = b = w ? 127 : 0;
        return;
    }
    const size_t HW = (size_t)it.H * it.W;
    const uint8_t* f = reinterpret_cast<const uint8_t*>(it.frame) + p;
    r = f[0];
    g = f[HW];
    b = f[2 * HW];
}

__device__ __forceinline__ int mx_code_at(const uint8_t* scene, size_t p)
{
    const uint8_t* s = scene + 3 * p;
    return (int)s[0] | ((int)s[1] << 8) | ((int)s[2] << 16);
}

// kind 1: the mask byte, kind 2: the ignore byte; the plane's source kind is not 0 (the caller wrote such a plane as zeros)
__device__ __forceinline__ int mx_map_byte(const MixParams& A, const MixItem& it, const TrainWin& o, int kind, int wy, int wx)
{
    size_t p = 0;
    const int w = mx_where(it, o, wy, wx, &p);
    if (w < 2) return (w == 1 && kind == 2) ? 255 : 0;
    if (kind == 1) {
        const int v = it.mask_kind == MX_MASK_CODE ? mx_code_at(reinterpret_cast<const uint8_t*>(it.mask_src), p)
                                                   : reinterpret_cast<const int32_t*>(it.mask_src)[p];
        return v == it.code ? 255 : 0;
    }
    if (it.ignore_kind == MX_IGNORE_DISPARITY) return reinterpret_cast<const int32_t*>(it.ignore_src)[p] > it.thr ? 255 : 0;
    const int c = mx_code_at(reinterpret_cast<const uint8_t*>(it.ignore_src), p);
    int count = 0;
    const uint8_t* nc = A.nearer + 3 * (size_t)it.near_off;
    for (int k = 0; k < it.near_cnt; k++) count += (c == ((int)nc[3 * k] | ((int)nc[3 * k + 1] << 8) | ((int)nc[3 * k + 2] << 16))) ? 1 : 0;
    return (255 * count) & 255;
}

struct MixSrc {
    const MixParams& A;
    const MixItem& it;
    const TrainWin& o;
    __device__ __forceinline__ void rgb(int wy, int wx, int& r, int& g, int& b) const { mx_raw_rgb(it, o, wy, wx, r, g, b); }
    __device__ __forceinline__ int map_byte(int kind, int wy, int wx) const { return mx_map_byte(A, it, o, kind, wy, wx); }
    __device__ __forceinline__ float mean(int ch) const { return it.mean[ch]; }
    __device__ __forceinline__ float stdev(int ch) const { return it.std[ch]; }
};

__global__ __launch_bounds__(TI_THREADS) void k_train_stats_mixed(const MixParams A)
{
    __shared__ int s_part[TI_WAVES];
    const int n = blockIdx.y;
    const MixItem it = A.items[n];
    const TrainWin o = A.objs[n];
    ti_stats_body(MixSrc{A, it, o}, o, mx_jitter_of(it), A.lsum + n, s_part);
}

// the body of k_train_crops with the frame, the sources, mean and std of the ITEM
__global__ __launch_bounds__(TI_THREADS) void k_train_crops_mixed(const MixParams A)
{
    __shared__ uint8_t s_src[3 * TI_SRC_PIXELS];
    __shared__ uint8_t s_rows[3 * TI_PLANE_BYTES];
    const int n = blockIdx.z, kind = blockIdx.y, tid = threadIdx.x;   // kind 0: image, 1: mask, 2: ignore
    const int S = kind == 0 ? A.Si : A.Sm;
    const int r0 = blockIdx.x * TI_BAND;
    if (r0 >= S) return;
    const TrainWin o = A.objs[n];
    const MixItem it = A.items[n];
    float* out = kind == 0 ? A.images + (size_t)n * 3 * S * S : (kind == 1 ? A.masks : A.ignores) + (size_t)n * S * S;
    if (kind != 0 && (kind == 1 ? it.mask_kind : it.ignore_kind) == 0) {   // no source: the plane is 0.0, with no fill value
        const int r1 = min(r0 + TI_BAND, S);
        for (int i = tid; i < (r1 - r0) * S; i += TI_THREADS) out[(size_t)r0 * S + i] = 0.f;
        return;
    }
    ti_crops_body(MixSrc{A, it, o}, o, mx_jitter_of(it), A.bounds, A.kk8, A.lsum + n, kind, S, r0, out, s_src, s_rows);
}

static bool tid_debug_checks()
{
    const char* e = getenv("SDN_DEBUG_CHECKS");
    return e && !strcmp(e, "1");
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_train_id_stats_workspace_bytes(int B, size_t* out)
{
    if (!out || B < 1 || B > 65535) return fail(SDN_EINVAL, "sdn_train_id_stats_workspace_bytes: bad arguments");
    *out = (size_t)B * TID_WS_PER_ITEM * sizeof(int32_t);
    return SDN_OK;
}

SDN_API int sdn_train_id_stats(const int32_t* items, int B, long max_pixels, int32_t* table, void* workspace, sdnStream stream)
{
    if (!items || !table || !workspace) return fail(SDN_EINVAL, "sdn_train_id_stats: null pointer");
    if (B < 1 || B > 65535 || max_pixels < 1 || max_pixels > INT_MAX - TID_CHUNK) return fail(SDN_EINVAL, "sdn_train_id_stats: bad sizes");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(table) & 3) || (reinterpret_cast<uintptr_t>(items) & 7))
        return fail(SDN_EINVAL, "sdn_train_id_stats: the workspace must be aligned to 16 bytes, the items to 8 and the table to 4");
    hipStream_t st = (hipStream_t)stream;
    const IdItem* rec = reinterpret_cast<const IdItem*>(items);
    int32_t* ws = static_cast<int32_t*>(workspace);
    int32_t* ws_hi = ws;
    int32_t* ws_sel = ws + (size_t)B * TID_BINS;
    int32_t* ws_lo = ws_sel + (size_t)B * 4;
    const dim3 grid(cdiv(max_pixels, TID_CHUNK), (unsigned)B);
    if (tid_debug_checks()) {   // the precondition 0 .. 65535; synchronous
        int* flag = nullptr;
        int bad = 0;
        if (hipMalloc(&flag, sizeof(int)) != hipSuccess || hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess)
            return fail(SDN_ELAUNCH, "sdn_train_id_stats: no memory for the debug check");
        hipLaunchKernelGGL(k_tid_range, grid, dim3(TID_THREADS), 0, st, rec, flag);
        hipError_t e = hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(flag);
        if (e != hipSuccess) return fail(SDN_ELAUNCH, "sdn_train_id_stats: debug check: %s", hipGetErrorString(e));
        if (bad) return fail(SDN_EINVAL, "sdn_train_id_stats: %d disparity values lie outside 0 .. 65535 (16-bit maps only)", bad);
    }
    hipLaunchKernelGGL(k_tid_init, dim3(cdiv((long)B * TID_WS_PER_ITEM, 256)), dim3(256), 0, st, table, ws, B);
    int rc = check_launch("k_tid_init");
    if (rc != SDN_OK) return rc;
    hipLaunchKernelGGL(k_tid_pass_a, grid, dim3(TID_THREADS), 0, st, rec, table, ws_hi);
    if ((rc = check_launch("k_tid_pass_a")) != SDN_OK) return rc;
    hipLaunchKernelGGL(k_tid_select, dim3(B), dim3(64), 0, st, table, ws_hi, ws_sel);
    if ((rc = check_launch("k_tid_select")) != SDN_OK) return rc;
    hipLaunchKernelGGL(k_tid_pass_b, grid, dim3(TID_THREADS), 0, st, rec, ws_sel, ws_lo);
    if ((rc = check_launch("k_tid_pass_b")) != SDN_OK) return rc;
    hipLaunchKernelGGL(k_tid_pick, dim3(B), dim3(64), 0, st, table, ws_sel, ws_lo);
    return check_launch("k_tid_pick");
}

SDN_API int sdn_train_crops_mixed(const int32_t* rois_host, const int32_t* objs_host, const int32_t* objs, const int32_t* items_host,
                                  const int32_t* items, int B, const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8,
                                  const uint8_t* nearer, int n_nearer, int image_size, int mask_size, void* workspace, float* images,
                                  float* masks, float* ignores, sdnStream stream)
{
    if (!rois_host || !objs_host || !objs || !items_host || !items || !bounds || !kk8 || !workspace || !images ||
        (n_nearer > 0 && !nearer) || (!masks) != (!ignores))
        return fail(SDN_EINVAL, "sdn_train_crops_mixed: null pointer");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(items) & 7))
        return fail(SDN_EINVAL, "sdn_train_crops_mixed: the workspace and the item table must be aligned to 8 bytes");
    static_assert(sizeof(TrainWin) == MX_OBJ_INTS * sizeof(int32_t), "object table row");
    MixSizes z;
    z.B = B; z.n_bounds = n_bounds; z.n_kk8 = n_kk8; z.n_nearer = n_nearer; z.image_size = image_size; z.mask_size = mask_size;
    z.maps = masks != nullptr;
    long scon = 0;
    char why[384];
    if (mx_validate(rois_host, objs_host, items_host, z, &scon, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_train_crops_mixed: %s", why);
    MixParams A;
    A.objs = reinterpret_cast<const TrainWin*>(objs);
    A.items = reinterpret_cast<const MixItem*>(items);
    A.bounds = bounds; A.kk8 = kk8; A.nearer = nearer;
    A.lsum = static_cast<unsigned long long*>(workspace);
    A.B = B; A.Si = image_size; A.Sm = mask_size;
    A.images = images; A.masks = masks; A.ignores = ignores;
    hipStream_t st = (hipStream_t)stream;
    if (scon) {
        if (hipMemsetAsync(workspace, 0, (size_t)B * sizeof(unsigned long long), st) != hipSuccess)
            return fail(SDN_ELAUNCH, "sdn_train_crops_mixed: clearing the sums failed");
        hipLaunchKernelGGL(k_train_stats_mixed, dim3(cdiv(scon * scon, TI_STAT_PIXELS), (unsigned)B), dim3(TI_THREADS), 0, st, A);
        if (int rc = check_launch("k_train_stats_mixed")) return rc;
    }
    const int Smax = z.maps ? (image_size > mask_size ? image_size : mask_size) : image_size;
    hipLaunchKernelGGL(k_train_crops_mixed, dim3(cdiv(Smax, TI_BAND), z.maps ? 3 : 1, (unsigned)B), dim3(TI_THREADS), 0, st, A);
    return check_launch("k_train_crops_mixed");
}
