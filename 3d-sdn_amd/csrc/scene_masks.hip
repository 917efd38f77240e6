// From the detector's output to the binary full-frame masks of SceneSession (geometric/maskrcnn/model.py:1638-1653, 2084-2143;
// maskrcnn/utils.py:378-395; geometric/scripts/main.py:724-818; derender3d/datasets.py:75-76, 95-103).
//
// The reference fetches mrcnn_mask [D, C, 28, 28] to the host, runs per detection scipy.misc.imresize(.., 'bilinear') to the
// box size (toimage -> bytescale -> PIL resize), thresholds, pastes into a full-frame uint8 plane, sums every plane to pick the
// 16 largest and uploads the survivors as float32.  Here:
//   k_unmold_masks    one launch for all objects.  A workgroup owns a band of rows of one object's plane: it makes the bytes
//                     of the object's class plane (bytescale in fp32 as numpy 1.14 evaluates it, the double quotient formed
//                     once), runs Pillow's horizontal pass for the source rows its band needs into LDS, the vertical pass out
//                     of LDS, thresholds and writes the WHOLE rows, zeros beside the box included (no memset in front).  The
//                     ones are counted per wave and added once per workgroup.  With a null plane pointer only the counts are
//                     made and only the workgroups that meet a box do anything.
//   k_scene_gt_masks  --source gt: the K planes np.all(scene == code, axis=2) of an instance-colour image, with the bounding
//                     box (mask_to_roi) and the pixel count of each, integer atomics once per wave.
// Compiled without FMA contraction; every step is integer or single IEEE fp32 operations (tests/test_gpu_detections.py).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "device_common.h"
#include "sdn_common.h"

namespace sdn {

constexpr int UM_BITS = 22;           // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int UM_THREADS = 256;
constexpr int UM_WAVES = UM_THREADS / 64;
constexpr int UM_BAND = 8;            // frame rows per workgroup
constexpr int UM_SRC_MAX = 4096;      // Mh Mw bytes of the class plane (28 x 28 = 784)
constexpr int UM_SIDE_MAX = 64;       // Mh, Mw
// Horizontally resampled source rows of a band, one byte per pixel.  32 KiB + the 4 KiB plane: four workgroups (16 waves)
// share the 160 KiB of a gfx950 CU.  A band inside an enlarged box needs 2 to 5 source rows; a band of a box flatter than
// the mask needs up to all Mh (28 x 1242 bytes = 34 KiB at the widest VKITTI box): the box is then walked in column chunks
// of 32 KiB / rows columns.
constexpr int UM_TILE_BYTES = 32768;
constexpr int UM_OBJ_INTS = 12;

struct UnmoldObj {   // one row of the object table
    int det, cls;                  // row of mrcnn_mask, class plane
    int y1, x1, y2, x2;            // the box in image pixels, inside the frame, not empty
    int boff_v, koff_v, ksize_v;   // tables of the resize Mh -> y2 - y1 (ksize 0: equal, Pillow skips the pass)
    int boff_h, koff_h, ksize_h;   // tables of the resize Mw -> x2 - x1
};

struct UnmoldParams {
    const float* soft;             // [D, C, Mh, Mw]
    const UnmoldObj* objs;
    const int32_t* bounds;
    const int32_t* kk8;
    int C, Mh, Mw, H, W;
    float* masks;                  // [n, 1, H, W] or null
    int32_t* areas;                // [n] or null (zeroed by the launcher)
};

// zeros into the elements [lo, hi) of `base` (element 0 is 16-byte aligned), a quad per thread
__device__ __forceinline__ void zero_range(float* base, long lo, long hi, int tid)
{
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    const long q0 = lo >> 2, q1 = (hi + 3) >> 2;
    for (long q = q0 + tid; q < q1; q += UM_THREADS) store_quad(base, 4 * q, lo, hi, z);
}

__global__ __launch_bounds__(UM_THREADS) void k_unmold_masks(const UnmoldParams A)
{
    __shared__ uint8_t s_src[UM_SRC_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[UM_TILE_BYTES];
    __shared__ float s_lo[UM_WAVES], s_hi[UM_WAVES];
    __shared__ float s_scale;
    __shared__ int s_cnt[UM_WAVES];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * UM_BAND;
    if (r0 >= A.H) return;
    const int r1 = min(r0 + UM_BAND, A.H);
    const UnmoldObj o = A.objs[n];
    const int ya = max(r0, o.y1), yb = min(r1, o.y2);   // the band's rows inside the box
    // The planes are addressed in quads of floats aligned to 16 bytes: `base` is the first aligned float at or below the
    // tensor, `shift` the tensor's offset in it (0 for a tensor torch allocated; H W need not be a multiple of 4).
    float* base = nullptr;
    long plane = 0;
    if (A.masks) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(A.masks);
        base = reinterpret_cast<float*>(a & ~(uintptr_t)15);
        plane = (long)((a & 15) >> 2) + (long)n * A.H * A.W;
    }
    if (ya >= yb) {   // the band lies beside the box
        if (base) zero_range(base, plane + (long)r0 * A.W, plane + (long)r1 * A.W, tid);
        return;
    }
    if (base) {
        zero_range(base, plane + (long)r0 * A.W, plane + (long)ya * A.W, tid);
        zero_range(base, plane + (long)yb * A.W, plane + (long)r1 * A.W, tid);
    }

    // ---- 1. bytescale of the class plane (scipy 1.0.1 misc/pilutil.py, under numpy 1.14: float32 array arithmetic, the
    // float64 scalar 255.0 / cscale is rounded to float32 before it multiplies)
    const int M = A.Mh * A.Mw;
    const float* soft = A.soft + ((size_t)o.det * A.C + o.cls) * M;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = tid; i < M; i += UM_THREADS) {
        const float v = soft[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = wave_fminf(lo);
    hi = wave_fmaxf(hi);
    if (lane == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    float cmin = s_lo[0], cmax = s_hi[0];
    for (int w = 1; w < UM_WAVES; w++) {
        cmin = fminf(cmin, s_lo[w]);
        cmax = fmaxf(cmax, s_hi[w]);
    }
    if (tid == 0) {   // the double division, once per workgroup
        float cscale = cmax - cmin;
        if (cscale == 0.f) cscale = 1.f;
        s_scale = (float)(255.0 / (double)cscale);
    }
    __syncthreads();
    const float scale = s_scale;
    for (int i = tid; i < M; i += UM_THREADS) {
        float t = (soft[i] - cmin) * scale + 0.f;
        t = fminf(fmaxf(t, 0.f), 255.f);
        s_src[i] = (uint8_t)(int)(t + 0.5f);
    }
    __syncthreads();

    // ---- 2. Pillow's two passes for the rows ya .. yb, 3. threshold, 4. paste
    const int w = o.x2 - o.x1;
    const int* bv = A.bounds + 2 * o.boff_v;
    const int* kv = A.kk8 + o.koff_v;
    const int* bh = A.bounds + 2 * o.boff_h;
    const int* kh = A.kk8 + o.koff_h;
    // source rows of the band: the windows of Pillow's bounds move monotonically
    int srow0, srow1;
    if (o.ksize_v) {
        srow0 = bv[2 * (ya - o.y1)];
        srow1 = bv[2 * (yb - 1 - o.y1)] + bv[2 * (yb - 1 - o.y1) + 1];
    } else {
        srow0 = ya - o.y1;
        srow1 = yb - o.y1;
    }
    srow0 = max(0, min(srow0, A.Mh - 1));
    srow1 = max(srow0 + 1, min(srow1, A.Mh));
    const int rows = srow1 - srow0;
    const int cw = min(w, (UM_TILE_BYTES / rows) & ~3);   // columns per chunk (rows <= 64: at least 512)
    int ones = 0;
    for (int c0 = 0; c0 < w; c0 += cw) {
        const int cn = min(cw, w - c0);
        // horizontal pass, rounded to uint8 as Pillow stores the intermediate image
        for (int i = tid; i < rows * cn; i += UM_THREADS) {
            const int ry = i / cn, c = c0 + i % cn;
            const uint8_t* src = s_src + (srow0 + ry) * A.Mw;
            int v;
            if (o.ksize_h) {
                const int x0 = bh[2 * c], xc = bh[2 * c + 1];
                int acc = 1 << (UM_BITS - 1);
                for (int t = 0; t < xc; t++) acc += (int)src[min(x0 + t, A.Mw - 1)] * kh[c * o.ksize_h + t];
                v = clip8(acc >> UM_BITS);
            } else {
                v = src[c];
            }
            s_rows[ry * cn + (c - c0)] = (uint8_t)v;
        }
        __syncthreads();
        // vertical pass over the frame columns of this chunk; the first chunk reaches the frame's left edge and the last
        // its right edge when planes are written
        const int fa = (base && c0 == 0) ? 0 : o.x1 + c0;
        const int fb = (base && c0 + cn >= w) ? A.W : o.x1 + c0 + cn;
        const int nq = (fb - fa + 3) / 4 + 1;   // aligned quads that can meet a row segment
        for (int i = tid; i < (yb - ya) * nq; i += UM_THREADS) {
            const int y = ya + i / nq, q = i % nq;
            const long lo_e = plane + (long)y * A.W + fa, hi_e = lo_e + (fb - fa);
            const long e0 = ((lo_e >> 2) + q) << 2;
            const int yo = y - o.y1;
            int y0 = yo - srow0, yc = 1;
            if (o.ksize_v) {
                y0 = bv[2 * yo] - srow0;
                yc = bv[2 * yo + 1];
            }
            float vals[4];
            for (int j = 0; j < 4; j++) {
                const long e = e0 + j;
                const int c = (int)(e - lo_e) + fa - o.x1 - c0;   // column of the chunk
                int one = 0;
                if (e >= lo_e && e < hi_e && c >= 0 && c < cn) {
                    int v;
                    if (o.ksize_v) {
                        int acc = 1 << (UM_BITS - 1);
                        for (int t = 0; t < yc; t++) acc += (int)s_rows[min(max(y0 + t, 0), rows - 1) * cn + c] * kv[yo * o.ksize_v + t];
                        v = clip8(acc >> UM_BITS);
                    } else {
                        v = s_rows[min(max(y0, 0), rows - 1) * cn + c];
                    }
                    // utils.py:389-390: (float32)v / 255.0f >= 0.5f.  127 / 255 = 0.498 and 128 / 255 = 0.50196, both far from
                    // a rounding boundary, so the test is v >= 128.
                    one = v >= 128 ? 1 : 0;
                }
                ones += one;
                vals[j] = one ? 1.f : 0.f;
            }
            if (base) store_quad(base, e0, lo_e, hi_e, vals);
        }
        __syncthreads();
    }
    if (A.areas) {   // integer addition: the order of the adds does not matter
        ones = wave_sum(ones);
        if (lane == 0) s_cnt[wave] = ones;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
            for (int k = 0; k < UM_WAVES; k++) total += s_cnt[k];
            if (total) atomicAdd(A.areas + n, total);
        }
    }
}

// ---- --source gt --------------------------------------------------------------------------------------------------------
__global__ void k_scene_gt_init(int32_t* rois, int32_t* areas, int K)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    rois[4 * k] = INT_MAX;
    rois[4 * k + 1] = INT_MAX;
    rois[4 * k + 2] = 0;
    rois[4 * k + 3] = 0;
    areas[k] = 0;
}

__device__ __forceinline__ void gt_note(int32_t* rois, int32_t* areas, int k, int ymin, int xmin, int ymax, int xmax, int cnt)
{
    atomicMin(rois + 4 * k, ymin);
    atomicMin(rois + 4 * k + 1, xmin);
    atomicMax(rois + 4 * k + 2, ymax + 1);
    atomicMax(rois + 4 * k + 3, xmax + 1);
    atomicAdd(areas + k, cnt);
}

// A thread owns an aligned quad of the K H W output floats.  The 256 elements of a wave nearly always belong to one plane:
// its matches are reduced over the wave and noted with five atomics; a match of another plane (a wave across a plane
// boundary) is noted by its own thread.
__global__ __launch_bounds__(256) void k_scene_gt_masks(const uint8_t* __restrict__ scene, const uint8_t* __restrict__ codes, int K,
                                                        int H, int W, float* masks, int32_t* rois, int32_t* areas)
{
    const long HW = (long)H * W, total = (long)K * HW;
    const uintptr_t a = reinterpret_cast<uintptr_t>(masks);
    float* base = reinterpret_cast<float*>(a & ~(uintptr_t)15);
    const long shift = (long)((a & 15) >> 2);
    const long lo = shift, hi = shift + total;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const long e0 = 4 * q;
    const long wave_e = 4 * (q - (threadIdx.x & 63));                     // the wave's first element
    const int kw = (int)(min(max(wave_e - shift, 0L), total - 1) / HW);    // the wave's plane
    int ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1, cnt = 0;
    float vals[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; j++) {
        const long e = e0 + j;
        if (e < lo || e >= hi) continue;
        const unsigned g = (unsigned)(e - shift);   // K H W fits an int (the launcher checked)
        const int k = (int)(g / (unsigned)HW);
        const unsigned p = g - (unsigned)k * (unsigned)HW;
        const uint8_t* s = scene + 3 * (size_t)p;
        const uint8_t* c = codes + 3 * k;
        if (s[0] != c[0] || s[1] != c[1] || s[2] != c[2]) continue;
        vals[j] = 1.f;
        const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
        if (k == kw) {
            ymin = min(ymin, y); xmin = min(xmin, x); ymax = max(ymax, y); xmax = max(xmax, x);
            cnt++;
        } else {
            gt_note(rois, areas, k, y, x, y, x, 1);
        }
    }
    if (e0 < hi && e0 + 4 > lo) store_quad(base, e0, lo, hi, vals);
    cnt = wave_sum(cnt);
    if (cnt) {   // uniform over the wave
        ymin = wave_imin(ymin); xmin = wave_imin(xmin); ymax = wave_imax(ymax); xmax = wave_imax(xmax);
        if ((threadIdx.x & 63) == 0) gt_note(rois, areas, kw, ymin, xmin, ymax, xmax, cnt);
    }
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_unmold_masks(const float* mrcnn_mask, int D, int C, int Mh, int Mw, const int32_t* objs_host, const int32_t* objs,
                             int n, const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8, int H, int W, float* masks,
                             int32_t* areas, sdnStream stream)
{
    if (!mrcnn_mask || !objs_host || !objs || !bounds || !kk8) return fail(SDN_EINVAL, "sdn_unmold_masks: null pointer");
    if (!masks && !areas) return fail(SDN_EINVAL, "sdn_unmold_masks: neither planes nor areas asked for");
    if (D < 1 || C < 1 || n < 1 || n > 65535 || H < 1 || W < 1 || (long)H * W > INT_MAX || n_bounds < 1 || n_kk8 < 1)
        return fail(SDN_EINVAL, "sdn_unmold_masks: bad sizes");
    if (Mh < 1 || Mw < 1 || Mh > UM_SIDE_MAX || Mw > UM_SIDE_MAX || Mh * Mw > UM_SRC_MAX)
        return fail(SDN_EINVAL, "sdn_unmold_masks: a %d x %d mask; the sides may be 1 to %d", Mh, Mw, UM_SIDE_MAX);
    if (masks && (reinterpret_cast<uintptr_t>(masks) & 3)) return fail(SDN_EINVAL, "sdn_unmold_masks: masks is not aligned to 4 bytes");
    static_assert(sizeof(UnmoldObj) == UM_OBJ_INTS * sizeof(int32_t), "object table row");
    for (int i = 0; i < n; i++) {
        const int32_t* r = objs_host + (size_t)UM_OBJ_INTS * i;
        if (r[0] < 0 || r[0] >= D || r[1] < 0 || r[1] >= C)
            return fail(SDN_EINVAL, "sdn_unmold_masks: object %d: detection %d, class %d outside [%d, %d]", i, r[0], r[1], D, C);
        if (r[2] < 0 || r[3] < 0 || r[4] > H || r[5] > W || r[4] <= r[2] || r[5] <= r[3])
            return fail(SDN_EINVAL, "sdn_unmold_masks: object %d: box (%d, %d, %d, %d) is empty or leaves the %d x %d frame", i, r[2],
                        r[3], r[4], r[5], H, W);
        // the tables of an axis: `out` rows of bounds, out x ksize weights; ksize 0 exactly when the sizes are equal
        for (int axis = 0; axis < 2; axis++) {
            const int32_t* t = r + 6 + 3 * axis;
            const long out = axis ? r[5] - r[3] : r[4] - r[2];
            const int in = axis ? Mw : Mh;
            if ((t[2] == 0) != (out == in) || t[2] < 0 || t[0] < 0 || t[1] < 0 ||
                (t[2] && (t[0] + out > n_bounds || t[1] + out * t[2] > n_kk8)))
                return fail(SDN_EINVAL, "sdn_unmold_masks: object %d: resampling table (%d, %d, %d) of %d -> %ld does not fit", i, t[0],
                            t[1], t[2], in, out);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (areas && hipMemsetAsync(areas, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess)
        return fail(SDN_ELAUNCH, "sdn_unmold_masks: clearing the areas failed");
    UnmoldParams A;
    A.soft = mrcnn_mask; A.objs = reinterpret_cast<const UnmoldObj*>(objs); A.bounds = bounds; A.kk8 = kk8;
    A.C = C; A.Mh = Mh; A.Mw = Mw; A.H = H; A.W = W; A.masks = masks; A.areas = areas;
    // written: the planes; read: the class planes and tables (small)
    TimedLaunch timed(TIME_SCENE_MASKS, st, masks ? (double)n * H * W * 4.0 : 0.0);
    hipLaunchKernelGGL(k_unmold_masks, dim3(cdiv(H, UM_BAND), (unsigned)n), dim3(UM_THREADS), 0, st, A);
    return check_launch("k_unmold_masks");
}

SDN_API int sdn_scene_gt_masks(const uint8_t* scene, const uint8_t* codes, int K, int H, int W, float* masks, int32_t* rois,
                               int32_t* areas, sdnStream stream)
{
    if (!scene || !codes || !masks || !rois || !areas) return fail(SDN_EINVAL, "sdn_scene_gt_masks: null pointer");
    if (K < 1 || H < 1 || W < 1 || (long)K * H * W > INT_MAX - 8) return fail(SDN_EINVAL, "sdn_scene_gt_masks: bad sizes");
    if (reinterpret_cast<uintptr_t>(masks) & 3) return fail(SDN_EINVAL, "sdn_scene_gt_masks: masks is not aligned to 4 bytes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_scene_gt_init, dim3(cdiv(K, 256)), dim3(256), 0, st, rois, areas, K);
    int rc = check_launch("k_scene_gt_init");
    if (rc != SDN_OK) return rc;
    const long quads = ((long)K * H * W + 3) / 4 + 1;   // + 1: a tensor that starts inside a quad
    TimedLaunch timed(TIME_SCENE_MASKS, st, (double)K * H * W * 4.0 + (double)K * H * W * 3.0);
    hipLaunchKernelGGL(k_scene_gt_masks, dim3(cdiv(quads, 256)), dim3(256), 0, st, scene, codes, K, H, W, masks, rois, areas);
    return check_launch("k_scene_gt_masks");
}
