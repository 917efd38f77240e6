// The 2D and 2D+ edit baselines of the geometric branch (geometric/scripts/main.py:215-322, `_test_2d` / `_test_2d_plus`).
//
// The reference, per object and frame: slices the object's detector mask at its roi, fetches it to the host, PIL-resizes it
// (bilinear) to the edited extent, pastes it into a new frame-sized 'L' image at the edited corner, uploads it, rounds and
// blends `(1 - m) * map + m * (1 + index)` in index order (:293-312).  Here:
//   k_scene_paint2d  one launch for F frames.  A thread owns one output pixel and walks the objects from the highest index
//                    down: the first active object whose pasted, resized mask covers the pixel wins (index-order painting
//                    leaves the highest index on top).  For the pixel it evaluates Pillow's ImagingResample of the 0 / 255
//                    window -- horizontal pass rounded and clipped to 8 bits, then the vertical pass, 22-bit fixed point, a
//                    pass skipped when its size does not change -- out of the cover words of sdn_scene_cover (a tap is a bit
//                    test).  The record of (frame, object) is uniform over the workgroup, so an object whose paste box
//                    misses the workgroup's 64 x 4 tile is skipped before any lane evaluates a tap.  No LDS, no atomics;
//                    every output byte has one writer.
//                    Without records ("identity") the value is the highest set cover bit + 1: the unedited masks painted in
//                    index order, the NAME-ref.png map of :236-238.
// The windows and weights (precompute_coeffs / normalize_coeffs_8bpc) come from derender3d/compositing.py, one table per
// axis and distinct (in, out) pair, pooled as for sdn_scene_crops / sdn_unmold_masks.  Integer arithmetic only: bit-identical
// to the PIL path (tests/test_gpu_scene2d.py).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "device_common.h"
#include "sdn_common.h"

namespace sdn {

constexpr int P2_BITS = 22;         // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int P2_TILE_W = 64;       // a wave is one row segment of 64 pixels
constexpr int P2_TILE_H = 4;
constexpr int P2_THREADS = P2_TILE_W * P2_TILE_H;
constexpr int P2_REC_INTS = 16;

struct Paint2dRec {   // one row of the record table: (frame, object)
    int active;                    // 0: the object is not painted in this frame (deleted)
    int r0, c0, h, w;              // the source window (the roi) in frame pixels, inside the frame, not empty
    int oh, ow;                    // the resized extent, both >= 1
    int top, left;                 // the paste corner in frame pixels, may lie outside the frame
    int boff_v, koff_v, ksize_v;   // tables of the resize h -> oh (ksize 0: equal, Pillow skips the pass)
    int boff_h, koff_h, ksize_h;   // tables of the resize w -> ow
    int pad;
};


// the highest set bit + 1 over the cover words of pixel p, 0 when none is set
__device__ __forceinline__ int p2_top_bit(const uint32_t* __restrict__ cover, int chunks, size_t HW, size_t p)
{
    for (int c = chunks - 1; c >= 0; c--) {
        const uint32_t w = cover[(size_t)c * HW + p];
        if (w) return 32 * c + 32 - __clz(w);
    }
    return 0;
}

__global__ __launch_bounds__(P2_THREADS) void k_scene_paint2d(const uint32_t* __restrict__ cover, const Paint2dRec* __restrict__ recs,
                                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk8,
                                                              int N, int H, int W, uint8_t* __restrict__ out)
{
    const int f = blockIdx.z;
    const int tx0 = blockIdx.x * P2_TILE_W, ty0 = blockIdx.y * P2_TILE_H;
    const int x = tx0 + (threadIdx.x & (P2_TILE_W - 1)), y = ty0 + (threadIdx.x >> 6);
    const bool live = x < W && y < H;
    const size_t HW = (size_t)H * W;
    const size_t p = live ? (size_t)y * W + x : 0;
    int value = 0;
    if (!recs) {
        if (live) out[(size_t)f * HW + p] = (uint8_t)p2_top_bit(cover, (N + 31) / 32, HW, p);
        return;
    }
    bool open = live;   // no object found yet
    for (int n = N - 1; n >= 0; n--) {
        if (__ballot(open) == 0ull) break;                      // the whole wave is painted
        const Paint2dRec r = recs[(size_t)f * N + n];           // uniform over the workgroup
        if (!r.active) continue;
        // paste box against the workgroup's tile (PIL's paste clips at the frame; the tile lies inside it)
        if (r.left >= tx0 + P2_TILE_W || r.left + r.ow <= tx0 || r.top >= ty0 + P2_TILE_H || r.top + r.oh <= ty0) continue;
        const int ox = x - r.left, oy = y - r.top;
        if (!open || ox < 0 || ox >= r.ow || oy < 0 || oy >= r.oh) continue;
        const uint32_t* words = cover + (size_t)(n >> 5) * HW;
        const int bit = n & 31;
        // source rows of the vertical pass and source columns of the horizontal pass for this output pixel
        int y0 = oy, yc = 1, x0 = ox, xc = 1;
        const int32_t* kv = nullptr;
        const int32_t* kh = nullptr;
        if (r.ksize_v) {
            y0 = bounds[2 * (r.boff_v + oy)];
            yc = min(bounds[2 * (r.boff_v + oy) + 1], r.ksize_v);
            kv = kk8 + r.koff_v + (size_t)oy * r.ksize_v;
        }
        if (r.ksize_h) {
            x0 = bounds[2 * (r.boff_h + ox)];
            xc = min(bounds[2 * (r.boff_h + ox) + 1], r.ksize_h);
            kh = kk8 + r.koff_h + (size_t)ox * r.ksize_h;
        }
        int acc_v = 1 << (P2_BITS - 1), v = 0;
        for (int t = 0; t < yc; t++) {
            const int sy = r.r0 + min(max(y0 + t, 0), r.h - 1);   // Pillow's windows lie inside the image; the clamp keeps a
            const uint32_t* row = words + (size_t)sy * W;         // table the launcher could not see from reaching outside
            int hv;                                               // the horizontal pass at (source row, ox)
            if (kh) {
                int acc = 1 << (P2_BITS - 1);
                for (int s = 0; s < xc; s++) {
                    const int sx = r.c0 + min(max(x0 + s, 0), r.w - 1);
                    acc += (int)((row[sx] >> bit) & 1u) * 255 * kh[s];
                }
                hv = clip8(acc >> P2_BITS);
            } else {
                hv = (int)((row[r.c0 + min(max(x0, 0), r.w - 1)] >> bit) & 1u) * 255;
            }
            if (kv) acc_v += hv * kv[t];
            else v = hv;
        }
        if (kv) v = clip8(acc_v >> P2_BITS);
        // to_tensor, torch.round (:309-310): round((float32)v / 255) == 1.  127 / 255 = 0.498 and 128 / 255 = 0.50196, both far
        // from the tie at 0.5, so the test is v >= 128.
        if (v >= 128) {
            value = n + 1;
            open = false;
        }
    }
    if (live) out[(size_t)f * HW + p] = (uint8_t)value;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_scene_paint2d(const uint32_t* cover, const int32_t* recs_host, const int32_t* recs, int F, int N,
                              const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8, int H, int W, uint8_t* out,
                              sdnStream stream)
{
    if (!cover || !out) return fail(SDN_EINVAL, "sdn_scene_paint2d: null pointer");
    if (F < 1 || F > 65535 || N < 1 || N > 255 || H < 1 || W < 1 || (long)H * W > INT_MAX)
        return fail(SDN_EINVAL, "sdn_scene_paint2d: bad sizes (F %d, N %d of at most 255, %d x %d)", F, N, H, W);
    if ((recs == nullptr) != (recs_host == nullptr)) return fail(SDN_EINVAL, "sdn_scene_paint2d: records on one side only");
    if (recs) {
        if (!bounds || !kk8 || n_bounds < 1 || n_kk8 < 1) return fail(SDN_EINVAL, "sdn_scene_paint2d: null pointer (tables)");
        static_assert(sizeof(Paint2dRec) == P2_REC_INTS * sizeof(int32_t), "record table row");
        for (long i = 0; i < (long)F * N; i++) {
            const int32_t* r = recs_host + (size_t)P2_REC_INTS * i;
            const int f = (int)(i / N), n = (int)(i % N);
            if (!r[0]) continue;
            if (r[1] < 0 || r[2] < 0 || r[3] < 1 || r[4] < 1 || (long)r[1] + r[3] > H || (long)r[2] + r[4] > W)
                return fail(SDN_EINVAL, "sdn_scene_paint2d: frame %d object %d: window (%d, %d) + %d x %d is empty or leaves the %d x %d "
                            "frame", f, n, r[1], r[2], r[3], r[4], H, W);
            if (r[5] < 1 || r[6] < 1)
                return fail(SDN_EINVAL, "sdn_scene_paint2d: frame %d object %d: output size %d x %d", f, n, r[5], r[6]);
            if ((long)r[7] + r[5] > INT_MAX || (long)r[8] + r[6] > INT_MAX)
                return fail(SDN_EINVAL, "sdn_scene_paint2d: frame %d object %d: paste box overflows", f, n);
            // the tables of an axis: `out` rows of bounds, out x ksize weights; ksize 0 exactly when the sizes are equal
            for (int axis = 0; axis < 2; axis++) {
                const int32_t* t = r + 9 + 3 * axis;
                const long in = r[3 + axis], o = r[5 + axis];
                if ((t[2] == 0) != (o == in) || t[2] < 0 || t[0] < 0 || t[1] < 0 ||
                    (t[2] && (t[0] + o > n_bounds || t[1] + o * t[2] > n_kk8)))
                    return fail(SDN_EINVAL, "sdn_scene_paint2d: frame %d object %d: resampling table (%d, %d, %d) of %ld -> %ld does not "
                                "fit", f, n, t[0], t[1], t[2], in, o);
            }
        }
    }
    hipLaunchKernelGGL(k_scene_paint2d, dim3(cdiv(W, P2_TILE_W), cdiv(H, P2_TILE_H), (unsigned)F), dim3(P2_THREADS), 0,
                       (hipStream_t)stream, cover, reinterpret_cast<const Paint2dRec*>(recs), bounds, kk8, N, H, W, out);
    return check_launch("k_scene_paint2d");
}
