// The inputs of the geometric branch from a frame and the detector's output, and the edit of a de-rendered scene
// (geometric/scripts/main.py:365-373, 405-421, 461-514; derender3d/datasets.py:49-71, 141-172).
//
// The reference makes, per object, three PIL round trips on the host -- Transforms.crop_square (pad + crop), a bilinear
// PIL resize and to_tensor for the image, the object's mask and its occlusion ("ignore") map -- and fetches every mask from
// the device for it.  Here:
//   k_scene_cover   folds the N binary masks of a frame into cover words (bit n of word n / 32 = object n covers the
//                   pixel): N H W floats read once, H W words per 32 objects written.  A mask tap is then a bit test and an
//                   ignore tap `(cover & nearer[slot]) != 0`, whatever N is.
//   k_scene_crops   one launch for all objects and planes (3 image channels, mask, ignore).  A workgroup owns a band of
//                   output rows of one (object, plane): it runs Pillow's horizontal pass (ImagingResample, 22-bit fixed
//                   point, rounded to uint8 as Pillow stores it) for the source rows the band needs into LDS and the
//                   vertical pass out of LDS, then to_tensor (/ 255) and, for the image, Normalize.
//   k_scene_edit    main.py:481-514 for F edit lists in one launch over [F, N].
// The windows and weights (precompute_coeffs / normalize_coeffs_8bpc) come from derender3d/compositing.py, as for
// sdn_composite_frame.  Compiled without FMA contraction: bit-identical to the PIL / torch path (tests/test_gpu_scene.py).
//
// crop_square's padding quirk is reproduced: it pads the right / bottom by max(0, roi end + d - size) but the window ends
// one pixel further when (s - w) is odd, and PIL's crop fills what lies beyond the padded image with 0, not with `fill`.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "device_common.h"
#include "sdn_common.h"

namespace sdn {

constexpr int CROP_BITS = 22;        // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int CROP_THREADS = 256;
constexpr int CROP_BAND = 8;         // output rows per workgroup
// Horizontally resampled source rows of a band, one byte per pixel.  32 KiB: five workgroups (20 waves) per CU beside
// each other in the 160 KiB of a gfx950 CU; a band of 8 rows at the largest VKITTI window (1242 -> 224: 11 taps, 5.5
// source rows per output row) needs 55 rows of 224 bytes.  Wider windows are walked in sub-bands of fewer output rows.
constexpr int CROP_LDS_BYTES = 32768;
constexpr int CROP_OBJ_INTS = 12;

struct CropObj {   // one row of the host's object table
    int oy, ox;                // frame coordinates of the window's first pixel
    int s;                     // side of the square window
    int xlim, ylim;            // frame coordinates where crop_square's padded image ends (beyond: 0)
    int boff_i, koff_i, ksize_i;   // tables of the resize s -> image_size (ksize 0: s == image_size, no resampling)
    int boff_m, koff_m, ksize_m;   // tables of the resize s -> mask_size
    int pad;
};

struct CropParams {
    const uint8_t* frame;      // [3, H, W]
    const uint32_t* cover;     // [chunks, H W]  mask cover words
    const uint32_t* icover;    // [chunks, H W]  cover words the ignore taps test (the masks' or the caller's ignore maps')
    const int64_t* nearer;     // [N, chunks]    low 32 bits: the objects whose union is slot j's ignore map
    const CropObj* objs;
    const int32_t* bounds;
    const int32_t* kk8;
    int N, H, W, chunks, Si, Sm, kinds;
    float mean[3], std[3];
    float *rgbs, *masks, *ignores;
};

enum { KIND_RGB = 1, KIND_MASK = 2, KIND_IGNORE = 4 };


// pixel (wy, wx) of object n's square window, as the uint8 image crop_square returns holds it.  plane 0..2: image channel,
// 3: mask, 4: ignore.  Every global read is behind the frame test.
__device__ __forceinline__ int crop_source(const CropParams& A, const CropObj& o, int n, int plane, int wy, int wx)
{
    const int fy = o.oy + wy, fx = o.ox + wx;
    if (fx >= o.xlim || fy >= o.ylim) return 0;                     // beyond the padded image: PIL's crop gives 0
    const bool in = (unsigned)fy < (unsigned)A.H && (unsigned)fx < (unsigned)A.W;
    const size_t HW = (size_t)A.H * A.W;
    const size_t p = in ? (size_t)fy * A.W + fx : 0;
    if (plane < 3) return in ? (int)A.frame[plane * HW + p] : 127;
    if (plane == 3) return in ? (int)((A.cover[(size_t)(n >> 5) * HW + p] >> (n & 31)) & 1u) * 255 : 0;
    if (!in) return 255;
    uint32_t hit = 0;
    for (int c = 0; c < A.chunks; c++) hit |= A.icover[(size_t)c * HW + p] & (uint32_t)A.nearer[(size_t)n * A.chunks + c];
    return hit ? 255 : 0;
}

__global__ __launch_bounds__(CROP_THREADS) void k_scene_crops(const CropParams A)
{
    __shared__ uint8_t s_rows[CROP_LDS_BYTES];
    const int n = blockIdx.z;
    int plane = blockIdx.y;   // index among the planes asked for -> 0..4
    {
        int seen = 0, found = -1;
        for (int p = 0; p < 5; p++) {
            const int bit = p < 3 ? KIND_RGB : (p == 3 ? KIND_MASK : KIND_IGNORE);
            if (A.kinds & bit) {
                if (seen == plane) found = p;
                seen++;
            }
        }
        plane = found;
    }
    if (plane < 0) return;
    const bool img = plane < 3;
    const int S = img ? A.Si : A.Sm;
    const int r0 = blockIdx.x * CROP_BAND;
    if (r0 >= S) return;
    const int r1 = min(r0 + CROP_BAND, S);
    const CropObj o = A.objs[n];
    const int ksize = img ? o.ksize_i : o.ksize_m;
    float* out = img ? A.rgbs + ((size_t)n * 3 + plane) * S * S : (plane == 3 ? A.masks : A.ignores) + (size_t)n * S * S;
    const float mean = img ? A.mean[plane] : 0.f, sd = img ? A.std[plane] : 1.f;
    const int tid = threadIdx.x;

    if (ksize == 0) {   // s == S: Pillow skips both passes
        for (int i = tid; i < (r1 - r0) * S; i += CROP_THREADS) {
            const int y = r0 + i / S, x = i % S;
            float v = (float)crop_source(A, o, n, plane, y, x) / 255.f;
            if (img) v = (v - mean) / sd;
            out[(size_t)y * S + x] = v;
        }
        return;
    }
    const int* b = A.bounds + 2 * (img ? o.boff_i : o.boff_m);
    const int* k = A.kk8 + (img ? o.koff_i : o.koff_m);
    const int cap = CROP_LDS_BYTES / S;   // source rows the LDS tile holds (the launcher checked ksize <= cap)
    int ra = r0;
    while (ra < r1) {
        // the longest run of output rows from ra whose source rows fit the tile (uniform over the workgroup)
        const int ybase = b[2 * ra];
        int rb = ra + 1, yend = ybase + b[2 * ra + 1];
        while (rb < r1 && b[2 * rb] + b[2 * rb + 1] - ybase <= cap) {
            yend = max(yend, b[2 * rb] + b[2 * rb + 1]);
            rb++;
        }
        const int rows = min(yend - ybase, cap);
        // horizontal pass: source rows ybase .. ybase + rows, rounded to uint8 as Pillow stores them
        for (int i = tid; i < rows * S; i += CROP_THREADS) {
            const int ry = i / S, x = i % S;
            const int x0 = b[2 * x], xc = b[2 * x + 1];
            int acc = 1 << (CROP_BITS - 1);
            for (int t = 0; t < xc; t++) acc += crop_source(A, o, n, plane, ybase + ry, x0 + t) * k[x * ksize + t];
            s_rows[i] = (uint8_t)clip8(acc >> CROP_BITS);
        }
        __syncthreads();
        // vertical pass, to_tensor, Normalize
        for (int i = tid; i < (rb - ra) * S; i += CROP_THREADS) {
            const int y = ra + i / S, x = i % S;
            const int y0 = b[2 * y] - ybase, yc = b[2 * y + 1];
            int acc = 1 << (CROP_BITS - 1);
            for (int t = 0; t < yc; t++) {
                const int row = min(y0 + t, cap - 1);
                acc += (int)s_rows[row * S + x] * k[y * ksize + t];
            }
            float v = (float)clip8(acc >> CROP_BITS) / 255.f;
            if (img) v = (v - mean) / sd;
            out[(size_t)y * S + x] = v;
        }
        __syncthreads();
        ra = rb;
    }
}

// cover[c][p] bit (n & 31) of chunk n / 32 = masks[n][p] != 0.  *nonbinary (optional) counts values other than 0 and 1.
__global__ __launch_bounds__(256) void k_scene_cover(const float* __restrict__ masks, int N, long HW, uint32_t* __restrict__ cover,
                                                     int* nonbinary)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (p >= HW) return;
    uint32_t w = 0;
    int bad = 0;
    const int n1 = min(N, 32 * c + 32);
    for (int n = 32 * c; n < n1; n++) {
        const float v = masks[(size_t)n * HW + p];
        w |= (v != 0.f ? 1u : 0u) << (n & 31);
        bad += (v != 0.f && v != 1.f) ? 1 : 0;
    }
    cover[(size_t)c * HW + p] = w;
    if (nonbinary && bad) atomicAdd(nonbinary, bad);
}

struct EditRec {   // one matched (object, operation) pair
    int obj;       // -1: unused slot
    int type;      // 0 delete, 1 modify
    float cy, cx;  // the new normalised centre (row, column)
    float lz2;     // 2 log(zoom)
    float c, s;    // cos(-ry), sin(-ry)
    int pad;
};

// main.py:481-514 on [F, N]: every thread copies its object's rows and applies its records in the reference's order, each
// reading what the one before left (yaw and depth compose, the position is overwritten).
__global__ __launch_bounds__(256) void k_scene_edit(const float* __restrict__ theta, const float* __restrict__ trans,
                                                    const float* __restrict__ logd, const float* __restrict__ mroi,
                                                    const float* __restrict__ droi, const uint8_t* __restrict__ interests,
                                                    const EditRec* __restrict__ recs, int F, int N, int P, float* o_theta,
                                                    float* o_trans, float* o_logd, uint8_t* o_int)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F * N) return;
    const int f = i / N, n = i % N;
    float tc = theta[2 * n], ts = theta[2 * n + 1], ty = trans[2 * n], tx = trans[2 * n + 1], ld = logd[n];
    uint8_t keep = interests[n];
    for (int p = 0; p < P; p++) {
        const EditRec r = recs[(size_t)f * P + p];
        if (r.obj != n) continue;
        if (r.type == 0) {
            keep = 0;
        } else {
            ty = (r.cy - mroi[2 * n]) / droi[2 * n];
            tx = (r.cx - mroi[2 * n + 1]) / droi[2 * n + 1];
            ld = ld - r.lz2;
            const float a = tc * r.c - ts * r.s;
            const float bb = ts * r.c + tc * r.s;
            tc = a;
            ts = bb;
        }
    }
    o_theta[2 * i] = tc;
    o_theta[2 * i + 1] = ts;
    o_trans[2 * i] = ty;
    o_trans[2 * i + 1] = tx;
    o_logd[i] = ld;
    o_int[i] = keep;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_scene_cover(const float* masks, int N, int H, int W, uint32_t* cover, sdnStream stream)
{
    if (!masks || !cover) return fail(SDN_EINVAL, "sdn_scene_cover: null pointer");
    if (N < 1 || H < 1 || W < 1 || (long)H * W > INT_MAX) return fail(SDN_EINVAL, "sdn_scene_cover: bad sizes");
    const long HW = (long)H * W;
    const int chunks = (N + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    const auto launch = [&](int* flag) {   // flag: where the kernel counts the values that are neither 0 nor 1, or NULL
        hipLaunchKernelGGL(k_scene_cover, dim3(cdiv(HW, 256), (unsigned)chunks), dim3(256), 0, st, masks, N, HW, cover, flag);
        return check_launch("k_scene_cover");
    };
    if (!debug_checks()) return launch(nullptr);
    int bad = 0, rc = SDN_OK;
    if (int e = debug_count("sdn_scene_cover", st, &bad, [&](int* flag) { rc = launch(flag); })) return e;
    if (rc == SDN_OK && bad) return fail(SDN_EINVAL, "sdn_scene_cover: %d mask values are neither 0 nor 1 (binary masks only)", bad);
    return rc;
}

SDN_API int sdn_scene_crops(const uint8_t* frame, const uint32_t* cover, const uint32_t* ignore_cover, const int64_t* nearer,
                            const int32_t* rois_host, const int32_t* objs, const int32_t* bounds, const int32_t* kk8, int N, int H,
                            int W, int image_size, int mask_size, int kinds, float mean0, float mean1, float mean2, float std0,
                            float std1, float std2, float* rgbs, float* masks, float* ignores, sdnStream stream)
{
    if (!rois_host || !objs || !bounds || !kk8) return fail(SDN_EINVAL, "sdn_scene_crops: null pointer");
    if (N < 1 || N > 65535 || H < 1 || W < 1 || (long)H * W > INT_MAX) return fail(SDN_EINVAL, "sdn_scene_crops: bad sizes");
    if (image_size < 1 || mask_size < 1 || image_size > CROP_LDS_BYTES || mask_size > CROP_LDS_BYTES)
        return fail(SDN_EINVAL, "sdn_scene_crops: bad crop sizes %d, %d", image_size, mask_size);
    if (kinds < 1 || kinds > 7) return fail(SDN_EINVAL, "sdn_scene_crops: kinds must be a mask of 1 (image), 2 (mask), 4 (ignore)");
    if ((kinds & KIND_RGB) && (!frame || !rgbs)) return fail(SDN_EINVAL, "sdn_scene_crops: null pointer (image crops)");
    if ((kinds & KIND_MASK) && (!cover || !masks)) return fail(SDN_EINVAL, "sdn_scene_crops: null pointer (mask crops)");
    if ((kinds & KIND_IGNORE) && (!ignore_cover || !nearer || !ignores))
        return fail(SDN_EINVAL, "sdn_scene_crops: null pointer (ignore crops)");
    if ((kinds & KIND_RGB) && (std0 == 0.f || std1 == 0.f || std2 == 0.f)) return fail(SDN_EINVAL, "sdn_scene_crops: std is 0");
    int planes = 0, smax = 0;
    if (kinds & KIND_RGB) { planes += 3; smax = image_size; }
    if (kinds & KIND_MASK) { planes += 1; smax = mask_size > smax ? mask_size : smax; }
    if (kinds & KIND_IGNORE) { planes += 1; smax = mask_size > smax ? mask_size : smax; }
    for (int n = 0; n < N; n++) {
        const int32_t* r = rois_host + 4 * n;
        if (r[2] <= r[0] || r[3] <= r[1])
            return fail(SDN_EINVAL, "sdn_scene_crops: roi %d (%d, %d, %d, %d) is empty", n, r[0], r[1], r[2], r[3]);
        const long s = (long)(r[2] - r[0]) > (long)(r[3] - r[1]) ? (long)(r[2] - r[0]) : (long)(r[3] - r[1]);
        // Pillow's filter width for s -> S: 2 ceil(max(s / S, 1)) + 1 source rows per output row; they must fit the LDS tile
        for (int which = 0; which < 2; which++) {
            const int S = which ? mask_size : image_size;
            if (!(kinds & (which ? (KIND_MASK | KIND_IGNORE) : KIND_RGB)) || s == S) continue;
            const long taps = 2 * ((s > S ? (s + S - 1) / S : 1)) + 1;
            if (taps + 1 > CROP_LDS_BYTES / S)
                return fail(SDN_EINVAL, "sdn_scene_crops: roi %d: a %ld pixel window resized to %d needs %ld source rows per output "
                            "row, the LDS tile holds %d", n, s, S, taps + 1, CROP_LDS_BYTES / S);
        }
    }
    static_assert(sizeof(CropObj) == CROP_OBJ_INTS * sizeof(int32_t), "object table row");
    CropParams A;
    A.frame = frame; A.cover = cover; A.icover = ignore_cover; A.nearer = nearer;
    A.objs = reinterpret_cast<const CropObj*>(objs); A.bounds = bounds; A.kk8 = kk8;
    A.N = N; A.H = H; A.W = W; A.chunks = (N + 31) / 32; A.Si = image_size; A.Sm = mask_size; A.kinds = kinds;
    A.mean[0] = mean0; A.mean[1] = mean1; A.mean[2] = mean2; A.std[0] = std0; A.std[1] = std1; A.std[2] = std2;
    A.rgbs = rgbs; A.masks = masks; A.ignores = ignores;
    hipLaunchKernelGGL(k_scene_crops, dim3(cdiv(smax, CROP_BAND), (unsigned)planes, (unsigned)N), dim3(CROP_THREADS), 0,
                       (hipStream_t)stream, A);
    return check_launch("k_scene_crops");
}

SDN_API int sdn_scene_edit(const float* theta_deltas, const float* translation2ds, const float* log_depths, const float* mroi_norms,
                           const float* droi_norms, const uint8_t* interests, const int32_t* records, int F, int N, int P,
                           float* theta_out, float* translation_out, float* log_depth_out, uint8_t* interests_out, sdnStream stream)
{
    if (!theta_deltas || !translation2ds || !log_depths || !mroi_norms || !droi_norms || !interests || !theta_out ||
        !translation_out || !log_depth_out || !interests_out || (P > 0 && !records))
        return fail(SDN_EINVAL, "sdn_scene_edit: null pointer");
    if (F < 1 || N < 1 || P < 0 || (long)F * N > INT_MAX / 2) return fail(SDN_EINVAL, "sdn_scene_edit: bad sizes");
    static_assert(sizeof(EditRec) == 8 * sizeof(int32_t), "edit record");
    hipLaunchKernelGGL(k_scene_edit, dim3(cdiv((long)F * N, 256)), dim3(256), 0, (hipStream_t)stream, theta_deltas, translation2ds,
                       log_depths, mroi_norms, droi_norms, interests, reinterpret_cast<const EditRec*>(records), F, N, P, theta_out,
                       translation_out, log_depth_out, interests_out);
    return check_launch("k_scene_edit");
}
