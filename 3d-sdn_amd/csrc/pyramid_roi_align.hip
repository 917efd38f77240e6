// Mask R-CNN's pyramid RoIAlign for gfx950: every box sampled from the FPN level its area selects, one launch forward, a zero fill
// and one scatter launch backward.
//
// Reference: geometric/maskrcnn/model.py:414-502 (pyramid_roi_align) with log2 of :95-100, and the crop it calls per level,
// roialign/roi_align/src/crop_and_resize.c:7-251.  The reference finds each level's boxes on the host (ix.any(), torch.nonzero: two
// waits per level), crops level by level, concatenates, sorts and gathers the result back into box order.  None of that needs the
// host: a box's level is a function of its four numbers, and the output row of box r is row r.
//
//   k_pra_fwd   a workgroup owns one box and a chunk of PRA_CHANNELS channels.  It computes the box's level (fp32, operation for
//               operation as model.py:445-457; no fast-math intrinsics) and builds the pool x pool sample table ONCE in LDS: four tap
//               offsets inside a channel plane, the two lerp weights and an inside flag per sample -- the arithmetic of k_crop_fwd
//               (crop_sample.h), so the values are the bits of crop_and_resize.c.  The lanes then run over (channel, sample), sample
//               fastest: the box's C * pool^2 outputs are contiguous, so the stores are coalesced, and the taps of one box fall into
//               a window of a few dozen pixels per channel.
//   k_pra_zero  16-byte stores over the one allocation that holds the four maps' gradients.
//   k_pra_bwd   the same table.  A box's contributions are summed in fp64 in an LDS window of the level's map, a few channels at a time,
//               and every touched pixel then takes one fp32 atomic add per box (a window of more than PRA_BWD_CELLS pixels keeps
//               the direct fp32 atomic adds of k_crop_bwd and the reference's CUDA kernel: few samples fall on each of its pixels).
//               Levels without a box stay all zero.  The order of the adds is not fixed, so the gradients are not bit-reproducible
//               from run to run; with one add per box and pixel they stay within a few ulp of the exact sum.
//   k_pra_box_records, k_pra_bwd_ordered   the second backward, sdn_pyramid_roi_align_bwd_ordered: a record per box (level, touched
//               window), then a workgroup per (level, 8 x 8 tile, channel chunk) that gathers from the boxes whose window meets its
//               tile, in ascending box index, into fp64 sums in registers, and stores every element once.  No float atomics, no
//               zero fill: the same bits every run.  Described where the kernels stand.
//
// A non-finite level value (a box of area <= 0, NaN) gives level 2: pyramid_roi_align_check.h, pra_level_of.
#include "crop_sample.h"
#include "pyramid_roi_align_check.h"
#include "sdn_common.h"

namespace sdn {

struct PraParams {
    const float* boxes;          // [R, 4] (y1, x1, y2, x2), normalised
    const float* map[PRA_LEVELS];   // forward: [C, H_l, W_l]
    float* gmap[PRA_LEVELS];     // backward: the level's range of the gradient buffer
    int H[PRA_LEVELS], W[PRA_LEVELS];
    int C, pool, chunks;
    float image_area, extrapolation;
    float* pooled;               // forward: [R, C, pool, pool]
    int32_t* levels;             // forward: [R]
    const float* grads;          // backward: [R, C, pool, pool]
};

struct PraTable {
    int4* taps;     // top-left, top-right, bottom-left, bottom-right: offsets inside a channel plane
    float2* lerp;   // x_lerp, y_lerp
    int* inside;
};

// the dynamic LDS, carved with the 16-byte entries first; it is declared 16-byte aligned, whatever static LDS a kernel adds
__device__ __forceinline__ PraTable pra_table(unsigned char* lds, int pp)
{
    PraTable t;
    t.taps = reinterpret_cast<int4*>(lds);
    t.lerp = reinterpret_cast<float2*>(lds + (size_t)pp * 16);
    t.inside = reinterpret_cast<int*>(lds + (size_t)pp * 24);
    return t;
}

// The box's level index (0 = P2 .. 3 = P5), the same in every lane and returned as a scalar, and its sample table.  Ends with a barrier.
__device__ __forceinline__ int pra_prepare(const PraParams& P, int r, const PraTable& t)
{
    const float* box = P.boxes + 4 * (size_t)r;
    const float y1 = box[0], x1 = box[1], y2 = box[2], x2 = box[3];
    const int l = __builtin_amdgcn_readfirstlane(pra_level_of(pra_level_value(y1, x1, y2, x2, P.image_area)) - 2);
    const int H = l == 0 ? P.H[0] : l == 1 ? P.H[1] : l == 2 ? P.H[2] : P.H[3];
    const int W = l == 0 ? P.W[0] : l == 1 ? P.W[1] : l == 2 ? P.W[2] : P.W[3];
    const int pp = P.pool * P.pool;
    for (int s = threadIdx.x; s < pp; s += PRA_THREADS) {
        const int y = s / P.pool, x = s - y * P.pool;
        const float in_y = axis_in(y1, y2, H, P.pool, y);
        const float in_x = axis_in(x1, x2, W, P.pool, x);
        int4 taps = make_int4(0, 0, 0, 0);
        float2 lerp = make_float2(0.0f, 0.0f);
        const bool inside = axis_inside(in_y, H) && axis_inside(in_x, W);
        if (inside) {   // 0 <= in <= extent - 1, so floor and ceil are rows and columns of the map
            const int top = (int)floorf(in_y), bottom = (int)ceilf(in_y);
            const int left = (int)floorf(in_x), right = (int)ceilf(in_x);
            taps = make_int4(top * W + left, top * W + right, bottom * W + left, bottom * W + right);
            lerp = make_float2(in_x - (float)left, in_y - (float)top);
        }
        t.taps[s] = taps;
        t.lerp[s] = lerp;
        t.inside[s] = inside ? 1 : 0;
    }
    __syncthreads();
    return l;
}

__global__ __launch_bounds__(PRA_THREADS) void k_pra_fwd(const PraParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pra_lds[];
    const int pp = P.pool * P.pool;
    const PraTable t = pra_table(pra_lds, pp);
    const int r = blockIdx.x / P.chunks, chunk = blockIdx.x - r * P.chunks;
    const int l = pra_prepare(P, r, t);
    if (chunk == 0 && threadIdx.x == 0) P.levels[r] = l + 2;
    const float* map = l == 0 ? P.map[0] : l == 1 ? P.map[1] : l == 2 ? P.map[2] : P.map[3];
    const int HW = l == 0 ? P.H[0] * P.W[0] : l == 1 ? P.H[1] * P.W[1] : l == 2 ? P.H[2] * P.W[2] : P.H[3] * P.W[3];
    const int c0 = chunk * PRA_CHANNELS, nc = min(PRA_CHANNELS, P.C - c0);
    float* out = P.pooled + ((size_t)r * P.C + c0) * pp;
    const int total = nc * pp;
    // element i = c * pp + s of the chunk; c and s advance without a division
    const int dc = PRA_THREADS / pp, ds = PRA_THREADS - dc * pp;
    int c = threadIdx.x / pp, s = threadIdx.x - c * pp;
    for (int i = threadIdx.x; i < total; i += PRA_THREADS) {
        float v = P.extrapolation;
        if (t.inside[s]) {
            const int4 o = t.taps[s];
            const float2 w = t.lerp[s];
            const float* p = map + (size_t)(c0 + c) * HW;
            const float tl = p[o.x], tr = p[o.y], bl = p[o.z], br = p[o.w];
            const float top = tl + (tr - tl) * w.x;
            const float bottom = bl + (br - bl) * w.x;
            v = top + (bottom - top) * w.y;
        }
        out[i] = v;
        c += dc;
        s += ds;
        if (s >= pp) {
            s -= pp;
            c++;
        }
    }
}

__global__ __launch_bounds__(PRA_THREADS) void k_pra_zero(float4* __restrict__ p, size_t n4)
{
    const size_t stride = (size_t)gridDim.x * PRA_THREADS;
    for (size_t i = (size_t)blockIdx.x * PRA_THREADS + threadIdx.x; i < n4; i += stride) p[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

constexpr int PRA_BWD_CELLS = 4096;   // fp64 cells of the backward's LDS window: 32 KiB

// The rows (or columns) of the map that the box's samples can touch along one axis: axis_in is linear in the sample index, so its
// values at the first and the last sample bound all of them; a sample that is inside (axis_inside) has floor and ceil in [0, extent - 1].
// False when no sample can be inside.  fmaxf / fminf drop a NaN end, which only widens the range.
__device__ __forceinline__ bool pra_axis_range(float a1, float a2, int extent, int pool, int* first, int* last)
{
    const float e0 = axis_in(a1, a2, extent, pool, 0), e1 = axis_in(a1, a2, extent, pool, pool - 1);
    const float lo = fmaxf(fminf(e0, e1), 0.0f), hi = fminf(fmaxf(e0, e1), (float)(extent - 1));
    if (!(lo <= hi)) return false;
    *first = (int)floorf(lo);
    *last = (int)ceilf(hi);
    return true;
}

__global__ __launch_bounds__(PRA_THREADS) void k_pra_bwd(const PraParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pra_lds[];
    __shared__ double acc[PRA_BWD_CELLS];
    const int pp = P.pool * P.pool;
    const PraTable t = pra_table(pra_lds, pp);
    const int r = blockIdx.x / P.chunks, chunk = blockIdx.x - r * P.chunks;
    const int l = pra_prepare(P, r, t);
    float* gmap = l == 0 ? P.gmap[0] : l == 1 ? P.gmap[1] : l == 2 ? P.gmap[2] : P.gmap[3];
    const int H = l == 0 ? P.H[0] : l == 1 ? P.H[1] : l == 2 ? P.H[2] : P.H[3];
    const int W = l == 0 ? P.W[0] : l == 1 ? P.W[1] : l == 2 ? P.W[2] : P.W[3];
    const int HW = H * W;
    const int c0 = chunk * PRA_CHANNELS, nc = min(PRA_CHANNELS, P.C - c0);
    const float* g_in = P.grads + ((size_t)r * P.C + c0) * pp;
    // The window of the level's map that this box touches.  Where it is small, many samples fall on each of its pixels, and a sum of
    // that many fp32 atomic adds in whatever order they arrive strays from the exact gradient by more than the reference's own
    // sequential fp32 sum does.  So the box's contributions are first summed in fp64 in LDS, a few channels at a time, and every
    // touched pixel then receives ONE fp32 atomic add per box.  A window too large for the LDS has few samples per pixel and keeps
    // the direct adds.
    const float* box = P.boxes + 4 * (size_t)r;
    int r0 = 0, r1 = 0, q0 = 0, q1 = 0;
    if (!pra_axis_range(box[0], box[2], H, P.pool, &r0, &r1) || !pra_axis_range(box[1], box[3], W, P.pool, &q0, &q1)) return;   // no sample inside
    const int wh = r1 - r0 + 1, ww = q1 - q0 + 1, cells = wh * ww;   // 1 <= wh <= H, 1 <= ww <= W
    if (cells > PRA_BWD_CELLS) {
        const int total = nc * pp;
        const int dc = PRA_THREADS / pp, ds = PRA_THREADS - dc * pp;
        int c = threadIdx.x / pp, s = threadIdx.x - c * pp;
        for (int i = threadIdx.x; i < total; i += PRA_THREADS) {
            if (t.inside[s]) {   // crop_and_resize.c:241-247
                const int4 o = t.taps[s];
                const float2 w = t.lerp[s];
                float* p = gmap + (size_t)(c0 + c) * HW;
                const float g = g_in[i];
                const float dtop = (1.0f - w.y) * g;
                unsafeAtomicAdd(p + o.x, (1.0f - w.x) * dtop);
                unsafeAtomicAdd(p + o.y, w.x * dtop);
                const float dbottom = w.y * g;
                unsafeAtomicAdd(p + o.z, (1.0f - w.x) * dbottom);
                unsafeAtomicAdd(p + o.w, w.x * dbottom);
            }
            c += dc;
            s += ds;
            if (s >= pp) {
                s -= pp;
                c++;
            }
        }
        return;
    }
    const int group = min(nc, PRA_BWD_CELLS / cells);   // channels per pass, at least 1
    const int origin = r0 * W + q0;
    for (int cb = 0; cb < nc; cb += group) {
        const int gc = min(group, nc - cb), used = gc * cells;
        for (int i = threadIdx.x; i < used; i += PRA_THREADS) acc[i] = 0.0;
        __syncthreads();
        for (int i = threadIdx.x; i < gc * pp; i += PRA_THREADS) {
            const int c = i / pp, s = i - c * pp;
            if (!t.inside[s]) continue;
            const int4 o = t.taps[s];
            const float2 w = t.lerp[s];
            // a tap (row, col) of the map is cell (row - r0, col - q0) of the window: inside it, since the sample is inside the map
            const int top = (o.x - origin) / W, left = (o.x - origin) - top * W;
            const int right = left + (o.y - o.x), down = (o.z - o.x) / W;   // 0 or 1 each
            double* a = acc + c * cells + top * ww;
            const float g = g_in[(size_t)(cb + c) * pp + s];
            const float dtop = (1.0f - w.y) * g, dbottom = w.y * g;   // crop_and_resize.c:241-247
            atomicAdd(a + left, (double)((1.0f - w.x) * dtop));
            atomicAdd(a + right, (double)(w.x * dtop));
            atomicAdd(a + down * ww + left, (double)((1.0f - w.x) * dbottom));
            atomicAdd(a + down * ww + right, (double)(w.x * dbottom));
        }
        __syncthreads();
        for (int i = threadIdx.x; i < used; i += PRA_THREADS) {
            const float v = (float)acc[i];
            if (v == 0.0f) continue;   // an untouched pixel receives nothing
            const int c = i / cells, cell = i - c * cells;
            const int row = cell / ww, col = cell - row * ww;
            unsafeAtomicAdd(gmap + (size_t)(c0 + cb + c) * HW + (size_t)(r0 + row) * W + (q0 + col), v);
        }
        __syncthreads();
    }
}

// ---- the ordered backward: a gather per destination, no float atomics, no zero fill ---------------------------------------------------
struct PraOrdParams {
    const float* boxes;          // [R, 4]
    const float* grads;          // [R, C, pool, pool]
    int4* records;               // the workspace: two int4 per box -- (level index or -1, r0, r1, q0), (q1, 0, 0, 0)
    float* gmap[PRA_LEVELS];
    int H[PRA_LEVELS], W[PRA_LEVELS];
    int start[PRA_LEVELS];       // first workgroup of level 3 - k: P5 comes first, its few tiles meet the most boxes each
    int R, C, pool, chunks;
    float image_area;
};

// A lane per box: the level and the window of the level's map that the box's samples can touch (pra_axis_range), for every workgroup of
// k_pra_bwd_ordered to test against its tile.
__global__ __launch_bounds__(PRA_THREADS) void k_pra_box_records(const PraOrdParams P)
{
    const int r = blockIdx.x * PRA_THREADS + threadIdx.x;
    if (r >= P.R) return;
    const float* box = P.boxes + 4 * (size_t)r;
    const float y1 = box[0], x1 = box[1], y2 = box[2], x2 = box[3];
    int l = pra_level_of(pra_level_value(y1, x1, y2, x2, P.image_area)) - 2;
    const int H = l == 0 ? P.H[0] : l == 1 ? P.H[1] : l == 2 ? P.H[2] : P.H[3];
    const int W = l == 0 ? P.W[0] : l == 1 ? P.W[1] : l == 2 ? P.W[2] : P.W[3];
    int r0 = 0, r1 = 0, q0 = 0, q1 = 0;
    if (!pra_axis_range(y1, y2, H, P.pool, &r0, &r1) || !pra_axis_range(x1, x2, W, P.pool, &q0, &q1)) l = -1;   // no sample inside
    P.records[2 * (size_t)r] = make_int4(l, r0, r1, q0);
    P.records[2 * (size_t)r + 1] = make_int4(q1, 0, 0, 0);
}

// A workgroup owns one level, one tile of PRA_TILE x PRA_TILE pixels and one chunk of PRA_CHANNELS channels, and stores every element
// of that block exactly once.  A lane owns one pixel (the wave's 64 lanes are the tile) and the channels c0 + wave + 4 i, i < 16, with
// an fp64 sum each in registers.  The boxes are taken in ascending index: 256 records at a time, ballot-compacted in index order into
// an LDS list of those of this level whose window meets the tile.  Of PRA_ORD_BATCH listed boxes at a time the per-axis tables stand
// in the LDS -- per sample index the low and high pixel index (-1: outside) and the lerp weight, the arithmetic of pra_prepare; the
// weights are separable, so pool entries per axis replace the pool x pool table.  axis_in is monotonic in the sample index, so the
// samples that touch a lane's row (column) are a contiguous range: the lane finds its two ranges in the tables and runs over their
// product only, first to last, adding the terms of crop_and_resize.c:241-247 in the C code's order.  The order of all additions is
// thus (box, sy, sx, tap): a function of the arguments alone.
__global__ __launch_bounds__(PRA_THREADS) void k_pra_bwd_ordered(const PraOrdParams P)
{
    constexpr int WAVES = PRA_THREADS / 64, PER_LANE = PRA_CHANNELS / WAVES;
    static_assert(PRA_TILE * PRA_TILE == 64 && PER_LANE == 16, "a wave is a tile; 16 sums per lane");
    __shared__ int list[PRA_THREADS];
    __shared__ int wave_count[WAVES];
    __shared__ int tab_lo[PRA_ORD_BATCH][2][PRA_MAX_POOL], tab_hi[PRA_ORD_BATCH][2][PRA_MAX_POOL];
    __shared__ float tab_lerp[PRA_ORD_BATCH][2][PRA_MAX_POOL];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = (b >= P.start[1]) + (b >= P.start[2]) + (b >= P.start[3]);   // the same in every lane
    const int l = PRA_LEVELS - 1 - k;
    const int idx = b - (k == 0 ? P.start[0] : k == 1 ? P.start[1] : k == 2 ? P.start[2] : P.start[3]);
    const int H = l == 0 ? P.H[0] : l == 1 ? P.H[1] : l == 2 ? P.H[2] : P.H[3];
    const int W = l == 0 ? P.W[0] : l == 1 ? P.W[1] : l == 2 ? P.W[2] : P.W[3];
    float* gmap = l == 0 ? P.gmap[0] : l == 1 ? P.gmap[1] : l == 2 ? P.gmap[2] : P.gmap[3];
    const int tiles_x = pra_tiles(W), tiles = tiles_x * pra_tiles(H);
    const int chunk = idx / tiles, tile = idx - chunk * tiles;
    const int ty0 = tile / tiles_x * PRA_TILE, tx0 = (tile - tile / tiles_x * tiles_x) * PRA_TILE;
    const int row = ty0 + lane / PRA_TILE, col = tx0 + lane % PRA_TILE;   // a pixel beyond the map's edge matches no sample
    const int c0 = chunk * PRA_CHANNELS, nc = min(PRA_CHANNELS, P.C - c0);
    const int mine = (nc - wave + WAVES - 1) / WAVES;   // channels c0 + wave + 4 i below c0 + nc; 0 for a wave past a short chunk
    const int pool = P.pool, pp = pool * pool;
    double acc[PER_LANE];
#pragma unroll
    for (int i = 0; i < PER_LANE; i++) acc[i] = 0.0;

    for (int base = 0; base < P.R; base += PRA_THREADS) {
        const int r = base + tid;
        bool hit = false;
        if (r < P.R) {
            const int4 a = P.records[2 * (size_t)r], q = P.records[2 * (size_t)r + 1];
            hit = a.x == l && a.y <= ty0 + PRA_TILE - 1 && a.z >= ty0 && a.w <= tx0 + PRA_TILE - 1 && q.x >= tx0;
        }
        const unsigned long long votes = __ballot(hit);
        if (lane == 0) wave_count[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, n = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            before += w < wave ? wave_count[w] : 0;
            n += wave_count[w];
        }
        if (hit) list[before + __popcll(votes & ((1ull << lane) - 1ull))] = r;   // ascending box index
        __syncthreads();
        for (int b0 = 0; b0 < n; b0 += PRA_ORD_BATCH) {
            const int nb = min(PRA_ORD_BATCH, n - b0);
            for (int e = tid; e < nb * 2 * PRA_MAX_POOL; e += PRA_THREADS) {
                const int j = e / (2 * PRA_MAX_POOL), axis = e / PRA_MAX_POOL % 2, s = e % PRA_MAX_POOL;
                if (s >= pool) continue;
                const float* box = P.boxes + 4 * (size_t)list[b0 + j];
                const int extent = axis ? W : H;
                const float in = axis_in(box[axis], box[axis + 2], extent, pool, s);
                int lo = -1, hi = -1;
                float lerp = 0.0f;
                if (axis_inside(in, extent)) {   // 0 <= in <= extent - 1
                    lo = (int)floorf(in);
                    hi = (int)ceilf(in);
                    lerp = in - (float)lo;
                }
                tab_lo[j][axis][s] = lo;
                tab_hi[j][axis][s] = hi;
                tab_lerp[j][axis][s] = lerp;
            }
            __syncthreads();
            for (int j = 0; j < nb; j++) {
                int sy0 = pool, sy1 = -1, sx0 = pool, sx1 = -1;
                for (int s = 0; s < pool; s++) {
                    if (tab_lo[j][0][s] == row || tab_hi[j][0][s] == row) {
                        sy0 = min(sy0, s);
                        sy1 = s;
                    }
                    if (tab_lo[j][1][s] == col || tab_hi[j][1][s] == col) {
                        sx0 = min(sx0, s);
                        sx1 = s;
                    }
                }
                if (sy1 < 0 || sx1 < 0 || mine == 0) continue;
                const float* g_box = P.grads + ((size_t)list[b0 + j] * P.C + c0 + wave) * pp;
                for (int sy = sy0; sy <= sy1; sy++) {
                    const bool on_top = tab_lo[j][0][sy] == row, on_bottom = tab_hi[j][0][sy] == row;
                    if (!on_top && !on_bottom) continue;
                    const float y_lerp = tab_lerp[j][0][sy];
                    for (int sx = sx0; sx <= sx1; sx++) {
                        const bool on_left = tab_lo[j][1][sx] == col, on_right = tab_hi[j][1][sx] == col;
                        if (!on_left && !on_right) continue;
                        const float x_lerp = tab_lerp[j][1][sx];
                        const float* g_in = g_box + sy * pool + sx;
#pragma unroll
                        for (int i = 0; i < PER_LANE; i++) {
                            if (i >= mine) continue;
                            const float g = g_in[(size_t)i * WAVES * pp];
                            const float dtop = (1.0f - y_lerp) * g, dbottom = y_lerp * g;   // crop_and_resize.c:241-247
                            // a sample on a pixel row or column has low == high: both of its terms land here and both are added
                            if (on_top && on_left) acc[i] += (double)((1.0f - x_lerp) * dtop);
                            if (on_top && on_right) acc[i] += (double)(x_lerp * dtop);
                            if (on_bottom && on_left) acc[i] += (double)((1.0f - x_lerp) * dbottom);
                            if (on_bottom && on_right) acc[i] += (double)(x_lerp * dbottom);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (row < H && col < W) {
        float* out = gmap + (size_t)(c0 + wave) * H * W + (size_t)row * W + col;
#pragma unroll
        for (int i = 0; i < PER_LANE; i++)
            if (i < mine) out[(size_t)i * WAVES * H * W] = (float)acc[i];
    }
    // the level's first workgroup also writes the floats that pad its range to 16 bytes
    const size_t used = (size_t)P.C * H * W;
    if (idx == 0 && tid < (int)((PRA_ALIGN_FLOATS - used % PRA_ALIGN_FLOATS) % PRA_ALIGN_FLOATS)) gmap[used + tid] = 0.0f;
}

static PraParams pra_params(const float* boxes, const int* H, const int* W, int C, int pool, float image_area)
{
    PraParams P = {};
    P.boxes = boxes;
    for (int l = 0; l < PRA_LEVELS; l++) {
        P.H[l] = H[l];
        P.W[l] = W[l];
    }
    P.C = C;
    P.pool = pool;
    P.chunks = pra_chunks(C);
    P.image_area = image_area;
    return P;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_pyramid_roi_align_grad_floats(int C, const int* H, const int* W, size_t* offsets, size_t* total)
{
    char why[256];
    if (pra_grad_layout(C, H, W, offsets, total, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_pyramid_roi_align_grad_floats: %s", why);
    return SDN_OK;
}

SDN_API int sdn_pyramid_roi_align_fwd(const float* boxes, int R, const float* const* maps, const int* H, const int* W, int C, int pool,
                                      float image_area, float extrapolation, float* pooled, int32_t* levels, sdnStream stream)
{
    char why[256];
    if (pra_validate_fwd(boxes, reinterpret_cast<const void* const*>(maps), H, W, R, C, pool, image_area, pooled, levels, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_pyramid_roi_align_fwd: %s", why);
    if (R == 0) return SDN_OK;
    PraParams P = pra_params(boxes, H, W, C, pool, image_area);
    for (int l = 0; l < PRA_LEVELS; l++) P.map[l] = maps[l];
    P.extrapolation = extrapolation;
    P.pooled = pooled;
    P.levels = levels;
    hipLaunchKernelGGL(k_pra_fwd, dim3((unsigned)R * (unsigned)P.chunks), dim3(PRA_THREADS), pra_table_bytes(pool), (hipStream_t)stream, P);
    return check_launch("k_pra_fwd");
}

SDN_API int sdn_pyramid_roi_align_bwd(const float* grads, const float* boxes, int R, const int* H, const int* W, int C, int pool,
                                      float image_area, float* grad_maps, sdnStream stream)
{
    char why[256];
    if (pra_validate_bwd(grads, boxes, H, W, R, C, pool, image_area, grad_maps, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_pyramid_roi_align_bwd: %s", why);
    size_t offsets[PRA_LEVELS], total = 0;
    if (pra_grad_layout(C, H, W, offsets, &total, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_pyramid_roi_align_bwd: %s", why);
    hipStream_t st = (hipStream_t)stream;
    const size_t n4 = total / PRA_ALIGN_FLOATS;   // every range is a whole number of 16-byte pieces
    const size_t want = (n4 + PRA_THREADS * 4 - 1) / (PRA_THREADS * 4);   // four stores per lane
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > 4096 ? 4096 : want);
    hipLaunchKernelGGL(k_pra_zero, dim3(blocks), dim3(PRA_THREADS), 0, st, reinterpret_cast<float4*>(grad_maps), n4);
    if (int rc = check_launch("k_pra_zero")) return rc;
    if (R == 0) return SDN_OK;
    PraParams P = pra_params(boxes, H, W, C, pool, image_area);
    for (int l = 0; l < PRA_LEVELS; l++) P.gmap[l] = grad_maps + offsets[l];
    P.grads = grads;
    hipLaunchKernelGGL(k_pra_bwd, dim3((unsigned)R * (unsigned)P.chunks), dim3(PRA_THREADS), pra_table_bytes(pool), st, P);
    return check_launch("k_pra_bwd");
}

SDN_API int sdn_pyramid_roi_align_bwd_ordered_workspace_bytes(int R, size_t* bytes)
{
    char why[256];
    if (pra_ordered_workspace_bytes(R, bytes, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_pyramid_roi_align_bwd_ordered_workspace_bytes: %s", why);
    return SDN_OK;
}

SDN_API int sdn_pyramid_roi_align_bwd_ordered(const float* grads, const float* boxes, int R, const int* H, const int* W, int C, int pool,
                                              float image_area, float* grad_maps, void* workspace, size_t workspace_bytes, sdnStream stream)
{
    char why[256];
    if (pra_validate_bwd_ordered(grads, boxes, H, W, R, C, pool, image_area, grad_maps, workspace, workspace_bytes, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_pyramid_roi_align_bwd_ordered: %s", why);
    size_t offsets[PRA_LEVELS], total = 0;
    if (pra_grad_layout(C, H, W, offsets, &total, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_pyramid_roi_align_bwd_ordered: %s", why);
    hipStream_t st = (hipStream_t)stream;
    PraOrdParams P = {};
    P.boxes = boxes;
    P.grads = grads;
    P.records = static_cast<int4*>(workspace);
    P.R = R;
    P.C = C;
    P.pool = pool;
    P.chunks = pra_chunks(C);
    P.image_area = image_area;
    int blocks = 0;
    for (int k = 0; k < PRA_LEVELS; k++) {   // P5 first
        const int l = PRA_LEVELS - 1 - k;
        P.H[l] = H[l];
        P.W[l] = W[l];
        P.gmap[l] = grad_maps + offsets[l];
        P.start[k] = blocks;
        blocks += pra_tiles(H[l]) * pra_tiles(W[l]) * P.chunks;   // the sum is below 2^31: pra_validate_bwd_ordered
    }
    if (R > 0) {
        hipLaunchKernelGGL(k_pra_box_records, dim3((unsigned)((R + PRA_THREADS - 1) / PRA_THREADS)), dim3(PRA_THREADS), 0, st, P);
        if (int rc = check_launch("k_pra_box_records")) return rc;
    }
    hipLaunchKernelGGL(k_pra_bwd_ordered, dim3((unsigned)blocks), dim3(PRA_THREADS), 0, st, P);
    return check_launch("k_pra_bwd_ordered");
}
