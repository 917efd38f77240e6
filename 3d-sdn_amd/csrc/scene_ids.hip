// From Cityscapes ground truth to the scene inputs of SceneSession (--dataset cityscapes --source gt: geometric/scripts/main.py:
// 763-795, 812-818; the same statements in derender3d/datasets.py:930-971; Transforms.mask_to_roi datasets.py:95-103).
//
// The reference finds the objects with np.unique over the instance-id map (id = category * 1000 + k), keeps the cars, and per
// car gathers the disparities under the mask, drops the zeros, takes np.percentile(., 95) -- a sort of up to 10^5 values -- and
// compares the WHOLE disparity frame with it (the ignore map).  Here:
//   sdn_scene_id_stats   one chain of five launches, nothing copied to the host: per id j = id - 1000 category the area, the
//                        roi, the count n of non-zero disparities and the two order statistics np.percentile interpolates
//                        between, found by an exact two-level radix select on the 16-bit values (no sort, no pixel lists):
//     k_ids_init     clears the table and the histograms
//     k_ids_pass_a   over the pixels: area, roi, n and a 256-bin histogram of the high byte per object.  The lanes of a wave
//                    hold neighbouring pixels, which mostly share (object, bin): they are grouped by ballot on equal keys, a
//                    group adds once into the workgroup's LDS counters, and the workgroup adds each non-zero counter once to
//                    global memory.  Integer atomics only: the result does not depend on scheduling.
//     k_ids_select   one wave per object scans the bins: bin and residual rank of i = 19 (n - 1) / 20 and of min(i + 1, n - 1)
//     k_ids_pass_b   over the pixels again: the low-byte histograms of the one or two target bins (LDS, then global)
//     k_ids_pick     one wave per object: lo and hi
//   sdn_scene_id_planes  one launch: the binary masks of the selected ids and the ignore maps disparity > thr[k], as cover words
//                        (the layout of sdn_scene_cover) and / or as fp32 planes; whole rows by aligned 16-byte stores, one
//                        writer per word, no memset in front.
// The interpolation between lo and hi stays on the host (derender3d.scene.percentile95_threshold): it is float64 arithmetic
// whose rounding decides pixels, and the host reads the table anyway to choose the largest masks.
//
//   sdn_train_id_stats   CityscapesSemantics.__getitem__ (datasets.py:938-955) for B items over several frames: the same table
//                        per ITEM (one id of one frame) instead of per id of one frame.  It is the same select: k_ids_init,
//                        k_ids_select and k_ids_pick, the workspace layout and the launch chain (ids_chain) are the ones above
//                        over B rows.  Only the two pixel passes are its own:
//     k_tid_pass_a   blockIdx.y is the item: its one 256-bin histogram lives in the workgroup's LDS, no slots
//     k_tid_pass_b   the same for the low-byte histograms
//                        The id and disparity maps are 4-byte elements: the lanes of a wave read consecutive pixels, one dword each.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "device_common.h"
#include "rank_select.h"
#include "sdn_common.h"

namespace sdn {

constexpr int ID_OBJS = 1000;                      // ids of one category
constexpr int ID_COLS = 8;                         // area, y0, x0, y1, x1, n, lo, hi
constexpr int ID_BINS = 256;
constexpr int ID_THREADS = 256;
constexpr int ID_ITERS = 8;                        // pixels per thread
constexpr int ID_CHUNK = ID_THREADS * ID_ITERS;    // pixels of one pass of a workgroup, consecutive
constexpr int ID_SLOTS = 16;                       // objects a workgroup of k_ids_pass_a / _b aggregates in LDS; further ones add to global memory
// the workspace of a select over `rows` table rows, in ints: high-byte histograms [rows][256], the select records [rows][4]
// (bin and residual rank of i, of i + 1), low-byte histograms [rows][2][256]
constexpr size_t ID_WS_PER_ROW = ID_BINS + 4 + 2 * ID_BINS;
static_assert(ID_THREADS == ID_BINS, "a workgroup flushes one bin per thread");
static_assert((ID_SLOTS & (ID_SLOTS - 1)) == 0, "slots are probed modulo a power of two");

__global__ __launch_bounds__(256) void k_ids_init(int32_t* table, int32_t* ws, int rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)rows * ID_WS_PER_ROW) ws[i] = 0;
    if (i < (size_t)rows * ID_COLS) {
        const int c = (int)(i & 7);
        table[i] = (c == 1 || c == 2) ? INT_MAX : 0;   // the invalid roi of sdn_scene_gt_masks
    }
}

// bin and low byte of a disparity; the masks keep a value outside 0 .. 65535 (a broken precondition) in bounds
__device__ __forceinline__ int ids_bin(int d) { return (d >> 8) & (ID_BINS - 1); }
__device__ __forceinline__ int ids_low(int d) { return d & (ID_BINS - 1); }
// which of the two low-byte histograms of the select record a bin feeds, -1: neither (rec.z == rec.x: one serves both ranks)
__device__ __forceinline__ int ids_which(int bin, const int4& rec) { return bin == rec.x ? 0 : (bin == rec.z ? 1 : -1); }

__global__ __launch_bounds__(256) void k_ids_range(const int32_t* __restrict__ disparity, long HW, int* bad)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < HW && (disparity[p] < 0 || disparity[p] > 65535)) atomicAdd(bad, 1);
}

// the LDS slot of object j: claimed by compare-and-swap, linear probing; -1 when all are taken
__device__ __forceinline__ int ids_slot(int* s_key, int j)
{
    int s = j & (ID_SLOTS - 1);
    for (int t = 0; t < ID_SLOTS; t++) {
        const int old = atomicCAS(&s_key[s], -1, j);
        if (old == -1 || old == j) return s;
        s = (s + 1) & (ID_SLOTS - 1);
    }
    return -1;
}

__device__ __forceinline__ void ids_note(int32_t* row, int area, int y0, int x0, int y1, int x1, int n)
{
    atomicAdd(row, area);
    atomicMin(row + 1, y0);
    atomicMin(row + 2, x0);
    atomicMax(row + 3, y1);
    atomicMax(row + 4, x1);
    if (n) atomicAdd(row + 5, n);
}

// `first` = 1000 category: an id belongs to the category exactly when id - first, as unsigned, is below 1000 (a bare
// `category` id is not).  Thread t of a workgroup holds the pixels chunk + it 256 + t: the lanes of a wave are 64 neighbours.
__global__ __launch_bounds__(ID_THREADS) void k_ids_pass_a(const int32_t* __restrict__ scene, const int32_t* __restrict__ disparity,
                                                           unsigned first, long HW, int W, int32_t* table, int32_t* hist_hi)
{
    __shared__ int s_key[ID_SLOTS];
    __shared__ int s_stat[ID_SLOTS][6];
    __shared__ int s_hist[ID_SLOTS][ID_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    const long p0 = (long)blockIdx.x * ID_CHUNK + tid;
    int jj[ID_ITERS], dd[ID_ITERS];
    int any = 0;
#pragma unroll
    for (int it = 0; it < ID_ITERS; it++) {
        const long p = p0 + (long)it * ID_THREADS;
        jj[it] = -1;
        dd[it] = 0;
        if (p < HW) {
            const unsigned r = (unsigned)scene[p] - first;
            if (r < (unsigned)ID_OBJS) {
                jj[it] = (int)r;
                dd[it] = disparity[p];
                any = 1;
            }
        }
    }
    if (!__syncthreads_or(any)) return;   // no pixel of the category in this chunk
    if (tid < ID_SLOTS) {
        s_key[tid] = -1;
        s_stat[tid][0] = 0; s_stat[tid][1] = INT_MAX; s_stat[tid][2] = INT_MAX;
        s_stat[tid][3] = 0; s_stat[tid][4] = 0; s_stat[tid][5] = 0;
    }
    for (int s = 0; s < ID_SLOTS; s++) s_hist[s][tid] = 0;
    __syncthreads();

#pragma unroll
    for (int it = 0; it < ID_ITERS; it++) {
        const int j = jj[it], d = dd[it];
        const bool car = j >= 0;
        unsigned long long rem = __ballot(car);
        if (!rem) continue;
        const unsigned p = (unsigned)(p0 + (long)it * ID_THREADS);   // H W fits an int (the launcher checked)
        const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
        // ids_bin(d), written out here and in pass B: through the helpers the compiler allocates this kernel 51 VGPRs for 78, and
        // the chain of the timing frame took 76 to 78 us for 70 to 72 (profiles/loader_bodies.md)
        const int bin = (d >> 8) & (ID_BINS - 1);
        while (rem) {   // one round per distinct object among the wave's 64 pixels
            const int src = __ffsll((long long)rem) - 1;
            const int j0 = __shfl(j, src, 64);
            const bool mine = car && j == j0;
            const unsigned long long m = __ballot(mine);
            rem &= ~m;
            int slot = -1;
            if (lane == src) slot = ids_slot(s_key, j0);
            slot = __shfl(slot, src, 64);
            const int ymin = wave_imin(mine ? y : INT_MAX), xmin = wave_imin(mine ? x : INT_MAX);
            const int ymax = wave_imax(mine ? y : -1), xmax = wave_imax(mine ? x : -1);
            const bool nz = mine && d != 0;
            unsigned long long left = __ballot(nz);
            if (lane == src) {
                if (slot >= 0) ids_note(s_stat[slot], __popcll(m), ymin, xmin, ymax + 1, xmax + 1, __popcll(left));
                else ids_note(table + ID_COLS * j0, __popcll(m), ymin, xmin, ymax + 1, xmax + 1, __popcll(left));
            }
            while (left) {   // one round per distinct high byte
                const int s2 = __ffsll((long long)left) - 1;
                const int b0 = __shfl(bin, s2, 64);
                const unsigned long long mb = __ballot(nz && bin == b0);
                left &= ~mb;
                if (lane == s2) {
                    if (slot >= 0) atomicAdd(&s_hist[slot][b0], __popcll(mb));
                    else atomicAdd(hist_hi + (size_t)j0 * ID_BINS + b0, __popcll(mb));
                }
            }
        }
    }
    __syncthreads();
    for (int s = 0; s < ID_SLOTS; s++) {
        const int j = s_key[s];
        if (j < 0) continue;
        if (tid == 0) ids_note(table + ID_COLS * j, s_stat[s][0], s_stat[s][1], s_stat[s][2], s_stat[s][3], s_stat[s][4], s_stat[s][5]);
        const int c = s_hist[s][tid];
        if (c) atomicAdd(hist_hi + (size_t)j * ID_BINS + tid, c);
    }
}

__global__ __launch_bounds__(64) void k_ids_select(const int32_t* __restrict__ table, const int32_t* __restrict__ hist_hi, int32_t* sel)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    const long n = table[ID_COLS * j + 5];
    int4 out = make_int4(-1, 0, -1, 0);
    if (n > 0) {   // uniform over the wave
        const long i = (19 * (n - 1)) / 20;   // floor((n - 1) 0.95), in integers
        const long i1 = min(i + 1, n - 1);
        ids_find(hist_hi + (size_t)j * ID_BINS, i, lane, &out.x, &out.y);
        ids_find(hist_hi + (size_t)j * ID_BINS, i1, lane, &out.z, &out.w);
    }
    if (lane == 0) reinterpret_cast<int4*>(sel)[j] = out;
}

__global__ __launch_bounds__(ID_THREADS) void k_ids_pass_b(const int32_t* __restrict__ scene, const int32_t* __restrict__ disparity,
                                                           unsigned first, long HW, const int32_t* __restrict__ sel, int32_t* hist_lo)
{
    __shared__ int s_key[ID_SLOTS];
    __shared__ int s_lo[ID_SLOTS][2][ID_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    const long p0 = (long)blockIdx.x * ID_CHUNK + tid;
    int jj[ID_ITERS], dd[ID_ITERS];
    int any = 0;
#pragma unroll
    for (int it = 0; it < ID_ITERS; it++) {
        const long p = p0 + (long)it * ID_THREADS;
        jj[it] = -1;
        dd[it] = 0;
        if (p < HW) {
            const unsigned r = (unsigned)scene[p] - first;
            if (r < (unsigned)ID_OBJS) {
                const int d = disparity[p];
                if (d != 0) {
                    jj[it] = (int)r;
                    dd[it] = d;
                    any = 1;
                }
            }
        }
    }
    if (!__syncthreads_or(any)) return;
    if (tid < ID_SLOTS) s_key[tid] = -1;
    for (int s = 0; s < ID_SLOTS; s++) {
        s_lo[s][0][tid] = 0;
        s_lo[s][1][tid] = 0;
    }
    __syncthreads();

#pragma unroll
    for (int it = 0; it < ID_ITERS; it++) {
        const int j = jj[it], d = dd[it];
        const bool car = j >= 0;
        unsigned long long rem = __ballot(car);
        while (rem) {   // one round per distinct object: its slot and its select record
            const int src = __ffsll((long long)rem) - 1;
            const int j0 = __shfl(j, src, 64);
            const bool mine = car && j == j0;
            rem &= ~__ballot(mine);
            int slot = -1;
            if (lane == src) slot = ids_slot(s_key, j0);
            slot = __shfl(slot, src, 64);
            const int4 rec = reinterpret_cast<const int4*>(sel)[j0];
            if (mine) {   // the low bytes inside a bin are spread: every pixel adds for itself
                const int bin = (d >> 8) & (ID_BINS - 1), low = d & (ID_BINS - 1);   // ids_bin, ids_low, ids_which, written out as in pass A
                const int w = bin == rec.x ? 0 : (bin == rec.z ? 1 : -1);
                if (w >= 0) {
                    if (slot >= 0) atomicAdd(&s_lo[slot][w][low], 1);
                    else atomicAdd(hist_lo + ((size_t)j0 * 2 + w) * ID_BINS + low, 1);
                }
            }
        }
    }
    __syncthreads();
    for (int s = 0; s < ID_SLOTS; s++) {
        const int j = s_key[s];
        if (j < 0) continue;
        for (int w = 0; w < 2; w++) {
            const int c = s_lo[s][w][tid];
            if (c) atomicAdd(hist_lo + ((size_t)j * 2 + w) * ID_BINS + tid, c);
        }
    }
}

__global__ __launch_bounds__(64) void k_ids_pick(int32_t* table, const int32_t* __restrict__ sel, const int32_t* __restrict__ hist_lo)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    if (table[ID_COLS * j + 5] <= 0) return;   // lo = hi = 0 (k_ids_init)
    const int4 rec = reinterpret_cast<const int4*>(sel)[j];
    int b_lo, b_hi, unused;
    ids_find(hist_lo + ((size_t)j * 2) * ID_BINS, rec.y, lane, &b_lo, &unused);
    ids_find(hist_lo + ((size_t)j * 2 + (rec.z != rec.x ? 1 : 0)) * ID_BINS, rec.w, lane, &b_hi, &unused);
    if (lane == 0) {
        table[ID_COLS * j + 6] = (rec.x << 8) | b_lo;
        table[ID_COLS * j + 7] = (rec.z << 8) | b_hi;
    }
}

// ---- the pixel passes of sdn_train_id_stats: B (frame, id) items ----------------------------------------------------------------
constexpr int TID_ITEM_INTS = 8;

struct IdItem {   // one row of the item table, 8 ints
    uint64_t ids;          // address of the int32 [H, W] id map
    uint64_t disparity;    // address of the int32 [H, W] disparity map, or 0
    int H, W;
    int id;
    int pad;
};
static_assert(sizeof(IdItem) == TID_ITEM_INTS * sizeof(int32_t), "id item row");

__global__ __launch_bounds__(ID_THREADS) void k_tid_range(const IdItem* __restrict__ items, int* bad)
{
    const IdItem it = items[blockIdx.y];
    const int32_t* disp = reinterpret_cast<const int32_t*>(it.disparity);
    if (!disp || it.H < 1 || it.W < 1) return;
    const long HW = (long)it.H * it.W;
    for (long p = (long)blockIdx.x * ID_THREADS + threadIdx.x; p < HW; p += (long)gridDim.x * ID_THREADS)
        if (disp[p] < 0 || disp[p] > 65535) atomicAdd(bad, 1);
}

// blockIdx.y is the item; a workgroup walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of its frame.  Thread t holds
// the pixels chunk + k 256 + t: the lanes of a wave are 64 neighbours, which mostly share the high byte of their disparity:
// they are grouped by ballot on equal bins and a group adds once into the LDS histogram.
__global__ __launch_bounds__(ID_THREADS) void k_tid_pass_a(const IdItem* __restrict__ items, int32_t* table, int32_t* hist_hi)
{
    __shared__ int s_hist[ID_BINS];
    __shared__ int s_stat[6];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const IdItem it = items[b];
    const int32_t* ids = reinterpret_cast<const int32_t*>(it.ids);
    const int32_t* disp = reinterpret_cast<const int32_t*>(it.disparity);
    if (!ids || it.H < 1 || it.W < 1) return;   // uniform over the workgroup; the row stays empty
    const long HW = (long)it.H * it.W;
    if ((long)blockIdx.x * ID_CHUNK >= HW) return;
    s_hist[tid] = 0;
    if (tid == 0) {
        s_stat[0] = 0; s_stat[1] = INT_MAX; s_stat[2] = INT_MAX; s_stat[3] = 0; s_stat[4] = 0; s_stat[5] = 0;
    }
    __syncthreads();
    int area = 0, ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1, n = 0;
    for (long c0 = (long)blockIdx.x * ID_CHUNK; c0 < HW; c0 += (long)gridDim.x * ID_CHUNK) {   // uniform over the workgroup
        for (int k = 0; k < ID_ITERS; k++) {
            const long p = c0 + (long)k * ID_THREADS + tid;
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
            const int bin = ids_bin(d);
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
    if (lane == 0 && area) ids_note(s_stat, area, ymin, xmin, ymax + 1, xmax + 1, n);
    __syncthreads();
    if (!s_stat[0]) return;   // uniform: no pixel of the item in this workgroup's chunks
    if (tid == 0) ids_note(table + ID_COLS * (size_t)b, s_stat[0], s_stat[1], s_stat[2], s_stat[3], s_stat[4], s_stat[5]);
    const int c = s_hist[tid];
    if (c) atomicAdd(hist_hi + (size_t)b * ID_BINS + tid, c);
}

__global__ __launch_bounds__(ID_THREADS) void k_tid_pass_b(const IdItem* __restrict__ items, const int32_t* __restrict__ sel,
                                                           int32_t* hist_lo)
{
    __shared__ int s_lo[2][ID_BINS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const IdItem it = items[b];
    const int32_t* ids = reinterpret_cast<const int32_t*>(it.ids);
    const int32_t* disp = reinterpret_cast<const int32_t*>(it.disparity);
    const int4 rec = reinterpret_cast<const int4*>(sel)[b];
    if (!ids || !disp || it.H < 1 || it.W < 1 || rec.x < 0) return;   // uniform; rec.x < 0: n == 0
    const long HW = (long)it.H * it.W;
    if ((long)blockIdx.x * ID_CHUNK >= HW) return;
    s_lo[0][tid] = 0;
    s_lo[1][tid] = 0;
    __syncthreads();
    for (long c0 = (long)blockIdx.x * ID_CHUNK; c0 < HW; c0 += (long)gridDim.x * ID_CHUNK)
        for (int k = 0; k < ID_ITERS; k++) {
            const long p = c0 + (long)k * ID_THREADS + tid;
            if (p >= HW || ids[p] != it.id) continue;
            const int d = disp[p];
            if (d == 0) continue;
            const int w = ids_which(ids_bin(d), rec);
            if (w >= 0) atomicAdd(&s_lo[w][ids_low(d)], 1);   // the low bytes inside a bin are spread: every pixel adds for itself
        }
    __syncthreads();
    for (int w = 0; w < 2; w++) {
        const int c = s_lo[w][tid];
        if (c) atomicAdd(hist_lo + ((size_t)b * 2 + w) * ID_BINS + tid, c);
    }
}

// blockIdx.y names an output row of H W words: mask plane k, ignore plane k or cover chunk c; a thread owns an aligned quad
// of it.  The rows are addressed from the first 16-byte aligned word at or below the array (H W need not be a multiple of 4,
// and the array may start inside a quad): a quad across two rows is written in part by a thread of either.
__global__ __launch_bounds__(256) void k_ids_planes(const int32_t* __restrict__ scene, const int32_t* __restrict__ disparity,
                                                    const int32_t* __restrict__ ids, const int32_t* __restrict__ thr, int n, long HW,
                                                    float* masks, float* ignores, uint32_t* cover)
{
    const int nm = masks ? n : 0, ni = ignores ? n : 0;
    int r = blockIdx.y, kind = 0;
    void* out = masks;
    if (r >= nm + ni) {
        kind = 2;
        r -= nm + ni;
        out = cover;
    } else if (r >= nm) {
        kind = 1;
        r -= nm;
        out = ignores;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(out);
    uint32_t* base = reinterpret_cast<uint32_t*>(a & ~(uintptr_t)15);
    const long lo = (long)((a & 15) >> 2) + (long)r * HW, hi = lo + HW;
    const long e0 = ((lo >> 2) + (long)blockIdx.x * 256 + threadIdx.x) << 2;
    if (e0 >= hi) return;
    const int32_t* src = kind == 0 ? scene : disparity;
    int v[4];
    for (int j = 0; j < 4; j++) {
        const long e = e0 + j;
        v[j] = (e >= lo && e < hi) ? src[e - lo] : 0;
    }
    uint32_t vals[4] = {0u, 0u, 0u, 0u};
    const uint32_t one = 0x3f800000u;   // 1.0f
    if (kind == 0) {
        const int id = ids[r];
        for (int j = 0; j < 4; j++) vals[j] = v[j] == id ? one : 0u;
    } else if (kind == 1) {
        const int t = thr[r];
        for (int j = 0; j < 4; j++) vals[j] = v[j] > t ? one : 0u;
    } else {
        const int k0 = 32 * r, kn = min(32, n - k0);
        for (int k = 0; k < kn; k++) {
            const int t = thr[k0 + k];
            for (int j = 0; j < 4; j++) vals[j] |= (v[j] > t ? 1u : 0u) << k;
        }
    }
    store_quad(base, e0, lo, hi, vals);
}

// The chain of five launches of a select over `rows` table rows.  pass_a(hist_hi) and pass_b(sel, hist_lo) issue the caller's
// pixel passes and return check_launch's answer.
template <class PassA, class PassB>
static int ids_chain(int rows, int32_t* table, int32_t* ws, hipStream_t st, PassA pass_a, PassB pass_b)
{
    int32_t* hi = ws;
    int32_t* sel = hi + (size_t)rows * ID_BINS;
    int32_t* lo = sel + (size_t)rows * 4;
    hipLaunchKernelGGL(k_ids_init, dim3(cdiv((long)(rows * ID_WS_PER_ROW), 256)), dim3(256), 0, st, table, ws, rows);
    int rc = check_launch("k_ids_init");
    if (rc != SDN_OK) return rc;
    if ((rc = pass_a(hi)) != SDN_OK) return rc;
    hipLaunchKernelGGL(k_ids_select, dim3(rows), dim3(64), 0, st, table, hi, sel);
    if ((rc = check_launch("k_ids_select")) != SDN_OK) return rc;
    if ((rc = pass_b(sel, lo)) != SDN_OK) return rc;
    hipLaunchKernelGGL(k_ids_pick, dim3(rows), dim3(64), 0, st, table, sel, lo);
    return check_launch("k_ids_pick");
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_scene_id_workspace_bytes(size_t* out)
{
    if (!out) return fail(SDN_EINVAL, "sdn_scene_id_workspace_bytes: null pointer");
    *out = ID_OBJS * ID_WS_PER_ROW * sizeof(int32_t);
    return SDN_OK;
}

SDN_API int sdn_scene_id_stats(const int32_t* scene, const int32_t* disparity, int category, int H, int W, int32_t* table,
                               void* workspace, sdnStream stream)
{
    if (!scene || !disparity || !table || !workspace) return fail(SDN_EINVAL, "sdn_scene_id_stats: null pointer");
    if (H < 1 || W < 1 || (long)H * W > INT_MAX - ID_CHUNK) return fail(SDN_EINVAL, "sdn_scene_id_stats: bad sizes");
    if (category < 0 || category > INT_MAX / ID_OBJS - 1)
        return fail(SDN_EINVAL, "sdn_scene_id_stats: category %d; ids are category * 1000 + k in an int32", category);
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(table) & 3))
        return fail(SDN_EINVAL, "sdn_scene_id_stats: the workspace must be aligned to 16 bytes and the table to 4");
    const long HW = (long)H * W;
    hipStream_t st = (hipStream_t)stream;
    if (debug_checks()) {   // the precondition 0 .. 65535; synchronous
        int bad = 0;
        if (int rc = debug_count("sdn_scene_id_stats", st, &bad, [&](int* flag) {
                hipLaunchKernelGGL(k_ids_range, dim3(cdiv(HW, 256)), dim3(256), 0, st, disparity, HW, flag);
            }))
            return rc;
        if (bad) return fail(SDN_EINVAL, "sdn_scene_id_stats: %d disparity values lie outside 0 .. 65535 (16-bit maps only)", bad);
    }
    const unsigned first = (unsigned)category * ID_OBJS;
    const unsigned chunks = cdiv(HW, ID_CHUNK);
    return ids_chain(
        ID_OBJS, table, static_cast<int32_t*>(workspace), st,
        [&](int32_t* hi) {
            hipLaunchKernelGGL(k_ids_pass_a, dim3(chunks), dim3(ID_THREADS), 0, st, scene, disparity, first, HW, W, table, hi);
            return check_launch("k_ids_pass_a");
        },
        [&](const int32_t* sel, int32_t* lo) {
            hipLaunchKernelGGL(k_ids_pass_b, dim3(chunks), dim3(ID_THREADS), 0, st, scene, disparity, first, HW, sel, lo);
            return check_launch("k_ids_pass_b");
        });
}

SDN_API int sdn_train_id_stats_workspace_bytes(int B, size_t* out)
{
    if (!out || B < 1 || B > 65535) return fail(SDN_EINVAL, "sdn_train_id_stats_workspace_bytes: bad arguments");
    *out = (size_t)B * ID_WS_PER_ROW * sizeof(int32_t);
    return SDN_OK;
}

SDN_API int sdn_train_id_stats(const int32_t* items, int B, long max_pixels, int32_t* table, void* workspace, sdnStream stream)
{
    if (!items || !table || !workspace) return fail(SDN_EINVAL, "sdn_train_id_stats: null pointer");
    if (B < 1 || B > 65535 || max_pixels < 1 || max_pixels > INT_MAX - ID_CHUNK) return fail(SDN_EINVAL, "sdn_train_id_stats: bad sizes");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(table) & 3) || (reinterpret_cast<uintptr_t>(items) & 7))
        return fail(SDN_EINVAL, "sdn_train_id_stats: the workspace must be aligned to 16 bytes, the items to 8 and the table to 4");
    hipStream_t st = (hipStream_t)stream;
    const IdItem* rec = reinterpret_cast<const IdItem*>(items);
    const dim3 grid(cdiv(max_pixels, ID_CHUNK), (unsigned)B);
    if (debug_checks()) {   // the precondition 0 .. 65535; synchronous
        int bad = 0;
        if (int rc = debug_count("sdn_train_id_stats", st, &bad,
                                 [&](int* flag) { hipLaunchKernelGGL(k_tid_range, grid, dim3(ID_THREADS), 0, st, rec, flag); }))
            return rc;
        if (bad) return fail(SDN_EINVAL, "sdn_train_id_stats: %d disparity values lie outside 0 .. 65535 (16-bit maps only)", bad);
    }
    return ids_chain(
        B, table, static_cast<int32_t*>(workspace), st,
        [&](int32_t* hi) {
            hipLaunchKernelGGL(k_tid_pass_a, grid, dim3(ID_THREADS), 0, st, rec, table, hi);
            return check_launch("k_tid_pass_a");
        },
        [&](const int32_t* sel, int32_t* lo) {
            hipLaunchKernelGGL(k_tid_pass_b, grid, dim3(ID_THREADS), 0, st, rec, sel, lo);
            return check_launch("k_tid_pass_b");
        });
}

SDN_API int sdn_scene_id_planes(const int32_t* scene, const int32_t* disparity, const int32_t* ids, const int32_t* thr, int n, int H,
                                int W, float* masks, uint32_t* ignore_cover, float* ignores, sdnStream stream)
{
    if (!scene || !disparity || !ids || !thr) return fail(SDN_EINVAL, "sdn_scene_id_planes: null pointer");
    if (!masks && !ignore_cover) return fail(SDN_EINVAL, "sdn_scene_id_planes: neither masks nor ignore_cover asked for");
    if (n < 1 || H < 1 || W < 1 || (long)H * W > INT_MAX - 1024) return fail(SDN_EINVAL, "sdn_scene_id_planes: bad sizes");
    const long rows = (masks ? n : 0) + (ignores ? n : 0) + (ignore_cover ? (n + 31) / 32 : 0);
    if (rows > 65535) return fail(SDN_EINVAL, "sdn_scene_id_planes: bad sizes: %d objects make %ld output rows, at most 65535", n, rows);
    if ((reinterpret_cast<uintptr_t>(masks) | reinterpret_cast<uintptr_t>(ignore_cover) | reinterpret_cast<uintptr_t>(ignores)) & 3)
        return fail(SDN_EINVAL, "sdn_scene_id_planes: an output is not aligned to 4 bytes");
    const long HW = (long)H * W;
    const long quads = (HW + 3) / 4 + 1;   // + 1: a row that starts inside a quad
    hipLaunchKernelGGL(k_ids_planes, dim3(cdiv(quads, 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, scene, disparity, ids,
                       thr, n, HW, masks, ignores, ignore_cover);
    return check_launch("k_ids_planes");
}
