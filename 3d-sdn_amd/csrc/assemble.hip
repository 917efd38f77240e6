// The textural loader's per-item arithmetic, batched over items and computed for the crop window only
// (textural/data/base_dataset.py:41-104 get_transform; vkitti_dataset.py:44-129 and cityscapes_dataset.py:32-111 __getitem__).
//
// The reference makes, per item on the host, five PIL round trips -- resize (or scale_width / make_power_2), crop, flip,
// ToTensor, Normalize for the label map, the image, the instance map, the pose-id map and the normal map -- and then walks
// np.unique of the pose-id map.  All items of a call share the source size [H, W], the options and therefore the scaled
// size [sh, sw] and the output size [h, w]; each item has its own crop position and flip.  Here:
//   k_assemble_planes  one launch for B items x C uint8 planes (image, normal map).  A workgroup owns a band of output rows
//                      of one (item, plane): it runs Pillow's horizontal pass (ImagingResample, 22-bit fixed point, rounded
//                      to uint8 as Pillow stores it) for the source rows the band needs and ONLY for the columns of the crop
//                      window into LDS, and the vertical pass out of LDS; then ToTensor as a look-up in the host's table
//                      (float32(k) / 255, correctly rounded on the host), Normalize, the normal branch's + 1/255.
//   k_assemble_gather  NEAREST geometry (ImagingScaleAffine's source indices, host tables) for the label, instance and pose-id
//                      maps: writes label and inst by the dataset's rule and counts the transformed pixels of each pose id
//                      per item (256 bins, integer atomics, aggregated per workgroup in LDS).
//   k_assemble_paint   paints the pose plane from the host's per-item table by raw id where the id's count reaches min_area
//                      (cityscapes_dataset.py:82: 256; vkitti: 1) and counts the pixels of such ids that have no record.
// A size that does not change means no resampling pass on that axis, as in Pillow.  Compiled without FMA contraction:
// bit-identical to the PIL / torch path (tests/test_gpu_assemble_batch.py).
#include <hip/hip_runtime.h>

#include <climits>

#include "device_common.h"
#include "sdn_common.h"

namespace sdn {

constexpr int ASM_BITS = 22;         // Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
constexpr int ASM_THREADS = 256;
constexpr int ASM_BAND = 8;          // output rows per workgroup
// Horizontally resampled source rows of a band, one byte per window pixel.  32 KiB: five workgroups per CU beside each other
// in the 160 KiB of a gfx950 CU.  A band of 8 rows of the Cityscapes item (2048 -> 1024: 9 taps, 2 source rows per output
// row, a 1024-wide window) needs 25 rows of 1024 bytes; wider windows are walked in sub-bands of fewer output rows.
constexpr int ASM_LDS_BYTES = 32768;
constexpr int ASM_MAP_PIXELS = 2048; // output pixels per workgroup of the map kernels (8 per thread)
constexpr int ASM_IDS = 256;

struct AsmPlanes {
    const int64_t* src;        // [B] device addresses of uint8 [C, H, W]; 0: the map is absent, the item's planes are 0.0
    const int32_t* items;      // [B, 4] crop x1, y1, flip, unused
    const int32_t* xmin;       // [sw] first source column of each scaled column's window
    const int32_t* xk;         // [sw, xks] fixed-point weights, 0 beyond the window
    const int32_t* ymin;       // [sh]
    const int32_t* yk;         // [sh, yks]
    const float* lut;          // [256] ToTensor
    float* out;                // [B, C, h, w]
    int B, C, H, W, sh, sw, h, w;
    int xks, yks;              // taps per output pixel; 0: the size does not change on that axis, no pass
    int normalize, bias;
    float mean, std, add;
};


// pixel (source row sy, scaled column xs) of the horizontally resampled plane, as the uint8 image Pillow's first pass stores
__device__ __forceinline__ int asm_hpix(const AsmPlanes& A, const uint8_t* __restrict__ plane, int sy, int xs)
{
    const uint8_t* row = plane + (size_t)sy * A.W;
    if (A.xks == 0) return row[xs];
    const int x0 = A.xmin[xs];
    const int* k = A.xk + (size_t)xs * A.xks;
    int acc = 1 << (ASM_BITS - 1);
    for (int t = 0; t < A.xks; t++) acc += (int)row[min(x0 + t, A.W - 1)] * k[t];
    return clip8(acc >> ASM_BITS);
}

__device__ __forceinline__ float asm_finish(const AsmPlanes& A, int v)
{
    float f = A.lut[v];
    if (A.normalize) f = (f - A.mean) / A.std;
    if (A.bias) f = f + A.add;
    return f;
}

__global__ __launch_bounds__(ASM_THREADS) void k_assemble_planes(const AsmPlanes A)
{
    __shared__ uint8_t s_rows[ASM_LDS_BYTES];
    const int b = blockIdx.z, c = blockIdx.y;
    const int r0 = blockIdx.x * ASM_BAND;
    if (r0 >= A.h) return;
    const int r1 = min(r0 + ASM_BAND, A.h);
    const int w = A.w, tid = threadIdx.x;
    float* out = A.out + ((size_t)b * A.C + c) * A.h * w;
    const uint8_t* plane = reinterpret_cast<const uint8_t*>(A.src[b]);
    if (!plane) {
        for (int i = tid; i < (r1 - r0) * w; i += ASM_THREADS) out[(size_t)r0 * w + i] = 0.f;
        return;
    }
    plane += (size_t)c * A.H * A.W;
    const int x1 = A.items[4 * b], y1 = A.items[4 * b + 1], flip = A.items[4 * b + 2];
    const float zero = asm_finish(A, 0);   // PIL's crop fills what lies beyond the scaled image with 0

    if (A.yks == 0) {   // sh == H: no vertical pass, nothing to stage
        for (int i = tid; i < (r1 - r0) * w; i += ASM_THREADS) {
            const int y = r0 + i / w, x = i % w;
            const int xs = x1 + (flip ? w - 1 - x : x), ys = y1 + y;
            out[(size_t)y * w + x] = (xs < A.sw && ys < A.sh) ? asm_finish(A, asm_hpix(A, plane, ys, xs)) : zero;
        }
        return;
    }
    const int rv = max(r0, min(r1, A.sh - y1));   // rows from rv on lie below the scaled image
    const int cap = ASM_LDS_BYTES / w;            // source rows the LDS tile holds (the launcher checked yks <= cap)
    int ra = r0;
    while (ra < rv) {
        // the longest run of output rows from ra whose source rows fit the tile (uniform over the workgroup)
        const int ybase = A.ymin[y1 + ra];
        int rb = ra + 1;
        while (rb < rv && A.ymin[y1 + rb] + A.yks - ybase <= cap) rb++;
        const int rows = min(A.ymin[y1 + rb - 1] + A.yks, A.H) - ybase;
        // horizontal pass over the window's columns: source rows ybase .. ybase + rows
        for (int i = tid; i < rows * w; i += ASM_THREADS) {
            const int ry = i / w, xs = x1 + i % w;
            s_rows[i] = xs < A.sw ? (uint8_t)asm_hpix(A, plane, ybase + ry, xs) : (uint8_t)0;
        }
        __syncthreads();
        // vertical pass, flip, ToTensor, Normalize
        for (int i = tid; i < (rb - ra) * w; i += ASM_THREADS) {
            const int y = ra + i / w, x = i % w;
            const int wc = flip ? w - 1 - x : x;
            float v = zero;
            if (x1 + wc < A.sw) {
                const int y0 = A.ymin[y1 + y] - ybase;
                const int* k = A.yk + (size_t)(y1 + y) * A.yks;
                int acc = 1 << (ASM_BITS - 1);
                for (int t = 0; t < A.yks; t++) acc += (int)s_rows[min(y0 + t, rows - 1) * w + wc] * k[t];
                v = asm_finish(A, clip8(acc >> ASM_BITS));
            }
            out[(size_t)y * w + x] = v;
        }
        __syncthreads();
        ra = rb;
    }
    for (int i = tid; i < (r1 - rv) * w; i += ASM_THREADS) out[(size_t)rv * w + i] = zero;
}

enum { ASM_INST_NONE = 0, ASM_INST_TABLE = 1, ASM_INST_FILL = 2, ASM_INST_INT = 3 };

struct AsmMaps {
    const int64_t* segm;       // [B] device addresses of uint8 [H, W]
    const int64_t* inst;       // [B] uint8 [H, W]; 0: no instance map, inst = label.  ASM_INST_INT: int32 [H, W]; 0: inst = 0
    const int64_t* pose;       // [B] uint8 [H, W] pose ids; 0: no pose map.  NULL: no pose feature at all
    const int32_t* items;      // [B, 4] crop x1, y1, flip, unused
    const int32_t* nx;         // [sw] source column of each scaled column (NULL: sw == W)
    const int32_t* ny;         // [sh]
    const int32_t* inst_nx;    // the same for the instance map of ASM_INST_INT where its image mode resizes differently,
    const int32_t* inst_ny;    // each axis on its own (NULL: nx / ny)
    const float* tabs;         // [4, 256]: label, label where the instance value is 0, fill of such an instance, instance
    int inst_mode, wrap16;
    int B, H, W, sh, sw, h, w;
    float* label;              // [B, 1, h, w]
    void* inst_out;            // [B, 1, h, w] fp32 (ASM_INST_INT: int32, int16 with wrap16)
    int32_t* counts;           // [B, 256]
    // the paint launch
    const int32_t* has;        // [B, 256] 1: the raw id has a record
    const uint32_t* val;       // [B, 256, ch] the painted words: int32 bin, or the bits of fp32 (cos, sin)
    int ch, min_area;
    uint32_t* pose_out;        // [B, ch, h, w]
    int32_t* missing;          // [B]
};

// source offset of output pixel i of item b under resize (NEAREST), crop and flip; false: beyond the scaled image (PIL: 0)
__device__ __forceinline__ bool asm_map_source(const AsmMaps& A, const int32_t* nx, const int32_t* ny, int b, int i, size_t& p)
{
    const int y = i / A.w, x = i % A.w;
    const int x1 = A.items[4 * b], y1 = A.items[4 * b + 1], flip = A.items[4 * b + 2];
    const int xs = x1 + (flip ? A.w - 1 - x : x), ys = y1 + y;
    if (xs >= A.sw || ys >= A.sh) return false;
    const int sx = nx ? min(nx[xs], A.W - 1) : xs, sy = ny ? min(ny[ys], A.H - 1) : ys;
    p = (size_t)sy * A.W + sx;
    return true;
}

__global__ __launch_bounds__(ASM_THREADS) void k_assemble_gather(const AsmMaps A)
{
    __shared__ int s_cnt[ASM_IDS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int hw = A.h * A.w;
    const int i0 = blockIdx.x * ASM_MAP_PIXELS, i1 = min(i0 + ASM_MAP_PIXELS, hw);
    const uint8_t* segm = reinterpret_cast<const uint8_t*>(A.segm[b]);
    const void* inst = A.inst_mode != ASM_INST_NONE ? reinterpret_cast<const void*>(A.inst[b]) : nullptr;
    const uint8_t* pose = A.pose ? reinterpret_cast<const uint8_t*>(A.pose[b]) : nullptr;
    const float *t_label = A.tabs, *t_label0 = A.tabs + 256, *t_fill = A.tabs + 512, *t_inst = A.tabs + 768;
    if (pose) {
        for (int k = tid; k < ASM_IDS; k += ASM_THREADS) s_cnt[k] = 0;
        __syncthreads();
    }
    for (int i = i0 + tid; i < i1; i += ASM_THREADS) {
        size_t p = 0;
        const bool in = asm_map_source(A, A.nx, A.ny, b, i, p);
        const int s = in ? (int)segm[p] : 0;
        float lab = t_label[s];
        const size_t o = (size_t)b * hw + i;
        if (A.inst_mode != ASM_INST_NONE) {
            if (A.inst_mode == ASM_INST_INT) {             // an integer map: ToTensor hands it through unscaled
                size_t q = p;
                if (in && (A.inst_nx || A.inst_ny))
                    asm_map_source(A, A.inst_nx ? A.inst_nx : A.nx, A.inst_ny ? A.inst_ny : A.ny, b, i, q);
                // an absent map has no integer form of the fp32 label: 0 of the output's type, never a float store into it
                const int v = (in && inst) ? static_cast<const int32_t*>(inst)[q] : 0;
                if (A.wrap16) static_cast<int16_t*>(A.inst_out)[o] = (int16_t)v;   // ToTensor reads 'I;16' through np.int16
                else static_cast<int32_t*>(A.inst_out)[o] = v;
            } else if (!inst) {                            // FileNotFoundError: inst_tensor IS the label tensor
                static_cast<float*>(A.inst_out)[o] = lab;
            } else {
                float v = t_inst[in ? (int)static_cast<const uint8_t*>(inst)[p] : 0];
                if (A.inst_mode == ASM_INST_FILL && v == 0.f) {
                    lab = t_label0[s];
                    v = t_fill[s];
                }
                static_cast<float*>(A.inst_out)[o] = v;
            }
        }
        A.label[o] = lab;
        if (pose) atomicAdd(&s_cnt[in ? (int)pose[p] : 0], 1);
    }
    if (pose) {
        __syncthreads();
        for (int k = tid; k < ASM_IDS; k += ASM_THREADS)
            if (s_cnt[k]) atomicAdd(&A.counts[b * ASM_IDS + k], s_cnt[k]);
    }
}

__global__ __launch_bounds__(ASM_THREADS) void k_assemble_paint(const AsmMaps A)
{
    __shared__ int s_miss;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int hw = A.h * A.w;
    const int i0 = blockIdx.x * ASM_MAP_PIXELS, i1 = min(i0 + ASM_MAP_PIXELS, hw);
    const uint8_t* pose = reinterpret_cast<const uint8_t*>(A.pose[b]);
    uint32_t* out = A.pose_out + (size_t)b * A.ch * hw;
    if (tid == 0) s_miss = 0;
    __syncthreads();
    int miss = 0;
    for (int i = i0 + tid; i < i1; i += ASM_THREADS) {
        uint32_t v0 = 0, v1 = 0;
        size_t p = 0;
        if (pose && asm_map_source(A, A.nx, A.ny, b, i, p)) {
            const int id = pose[p];
            if (id != 0 && A.counts[b * ASM_IDS + id] >= A.min_area) {
                if (A.has[b * ASM_IDS + id]) {
                    const uint32_t* v = A.val + ((size_t)b * ASM_IDS + id) * A.ch;
                    v0 = v[0];
                    if (A.ch == 2) v1 = v[1];
                } else {
                    miss++;
                }
            }
        }
        out[i] = v0;
        if (A.ch == 2) out[(size_t)hw + i] = v1;
    }
    if (miss) atomicAdd(&s_miss, miss);
    __syncthreads();
    if (tid == 0 && s_miss) atomicAdd(&A.missing[b], s_miss);
}

// the per-item rows (x1, y1, flip, unused) on the host: the crop position is what keeps every read inside the tables
static int check_items(const char* who, const int32_t* items_host, int B, int h, int w)
{
    for (int b = 0; b < B; b++) {
        const int32_t* r = items_host + 4 * b;
        if (r[0] < 0 || r[1] < 0 || r[0] > INT_MAX - w || r[1] > INT_MAX - h || (r[2] != 0 && r[2] != 1))
            return fail(SDN_EINVAL, "%s: item %d: bad crop position (%d, %d) or flip %d", who, b, r[0], r[1], r[2]);
    }
    return SDN_OK;
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_assemble_planes(const int64_t* src, const int32_t* items_host, const int32_t* items, const int32_t* xmin,
                                const int32_t* xk, int xks, const int32_t* ymin, const int32_t* yk, int yks, const float* lut, int B,
                                int C, int H, int W, int sh, int sw, int h, int w, int normalize, float mean, float std, int bias,
                                float add, float* out, sdnStream stream)
{
    if (!src || !items_host || !items || !lut || !out) return fail(SDN_EINVAL, "sdn_assemble_planes: null pointer");
    if (B < 1 || B > 65535 || C < 1 || C > 65535 || H < 1 || W < 1 || (long)C * H * W > INT_MAX || sh < 1 || sw < 1 || h < 1 ||
        w < 1 || (long)h * w > INT_MAX)
        return fail(SDN_EINVAL, "sdn_assemble_planes: bad sizes");
    if (xks < 0 || yks < 0 || (xks == 0) != (sw == W) || (yks == 0) != (sh == H))
        return fail(SDN_EINVAL, "sdn_assemble_planes: %d x %d -> %d x %d with %d and %d taps (0 taps: the size does not change)", H, W,
                    sh, sw, yks, xks);
    if ((xks && (!xmin || !xk)) || (yks && (!ymin || !yk))) return fail(SDN_EINVAL, "sdn_assemble_planes: null table");
    if (normalize && std == 0.f) return fail(SDN_EINVAL, "sdn_assemble_planes: std is 0");
    if (yks && (w > ASM_LDS_BYTES || yks > ASM_LDS_BYTES / w))
        return fail(SDN_EINVAL, "sdn_assemble_planes: one output row of a %d pixel wide window needs %d source rows, the LDS tile "
                    "holds %d", w, yks, w > ASM_LDS_BYTES ? 0 : ASM_LDS_BYTES / w);
    if (int rc = check_items("sdn_assemble_planes", items_host, B, h, w)) return rc;
    AsmPlanes A;
    A.src = src; A.items = items; A.xmin = xmin; A.xk = xk; A.ymin = ymin; A.yk = yk; A.lut = lut; A.out = out;
    A.B = B; A.C = C; A.H = H; A.W = W; A.sh = sh; A.sw = sw; A.h = h; A.w = w; A.xks = xks; A.yks = yks;
    A.normalize = normalize; A.bias = bias; A.mean = mean; A.std = std; A.add = add;
    hipLaunchKernelGGL(k_assemble_planes, dim3(cdiv(h, ASM_BAND), (unsigned)C, (unsigned)B), dim3(ASM_THREADS), 0,
                       (hipStream_t)stream, A);
    return check_launch("k_assemble_planes");
}

SDN_API int sdn_assemble_maps(const int64_t* segm, const int64_t* inst, const int64_t* pose, const int32_t* items_host,
                              const int32_t* items, const int32_t* nx, const int32_t* ny, const int32_t* inst_nx,
                              const int32_t* inst_ny, const float* tabs, int inst_mode, int wrap16, int B, int H, int W, int sh,
                              int sw, int h, int w, float* label, void* inst_out, const int32_t* pose_has, const void* pose_val,
                              int pose_channels, int min_area, void* pose_out, int32_t* counts, int32_t* missing,
                              sdnStream stream)
{
    if (!segm || !items_host || !items || !tabs || !label || !missing) return fail(SDN_EINVAL, "sdn_assemble_maps: null pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > INT_MAX || sh < 1 || sw < 1 || h < 1 || w < 1 ||
        (long)h * w > INT_MAX / 2)
        return fail(SDN_EINVAL, "sdn_assemble_maps: bad sizes");
    if ((nx == nullptr) != (sw == W) || (ny == nullptr) != (sh == H))
        return fail(SDN_EINVAL, "sdn_assemble_maps: %d x %d -> %d x %d: an index table exactly where the size changes", H, W, sh, sw);
    if ((inst_nx && !nx) || (inst_ny && !ny) || ((inst_nx || inst_ny) && inst_mode != ASM_INST_INT))
        return fail(SDN_EINVAL, "sdn_assemble_maps: inst_nx / inst_ny only where that size changes, and only for inst_mode 3");
    if (inst_mode < ASM_INST_NONE || inst_mode > ASM_INST_INT) return fail(SDN_EINVAL, "sdn_assemble_maps: inst_mode %d", inst_mode);
    if (inst_mode != ASM_INST_NONE && (!inst || !inst_out))
        return fail(SDN_EINVAL, "sdn_assemble_maps: null pointer (instance map)");
    if (pose_out && (!pose || !pose_has || !pose_val || !counts || (pose_channels != 1 && pose_channels != 2) || min_area < 1))
        return fail(SDN_EINVAL, "sdn_assemble_maps: the pose plane needs pose, pose_has, pose_val, counts, 1 or 2 channels, "
                    "min_area >= 1");
    if (int rc = check_items("sdn_assemble_maps", items_host, B, h, w)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(missing, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess ||
        (pose_out && hipMemsetAsync(counts, 0, (size_t)B * ASM_IDS * sizeof(int32_t), st) != hipSuccess))
        return fail(SDN_ELAUNCH, "sdn_assemble_maps: clearing the counters failed");
    AsmMaps A;
    A.segm = segm; A.inst = inst; A.pose = pose_out ? pose : nullptr; A.items = items; A.nx = nx; A.ny = ny;
    A.inst_nx = inst_nx; A.inst_ny = inst_ny; A.tabs = tabs;
    A.inst_mode = inst_mode; A.wrap16 = wrap16; A.B = B; A.H = H; A.W = W; A.sh = sh; A.sw = sw; A.h = h; A.w = w;
    A.label = label; A.inst_out = inst_out; A.counts = counts; A.has = pose_has;
    A.val = static_cast<const uint32_t*>(pose_val); A.ch = pose_channels; A.min_area = min_area;
    A.pose_out = static_cast<uint32_t*>(pose_out); A.missing = missing;
    const dim3 grid(cdiv((long)h * w, ASM_MAP_PIXELS), (unsigned)B);
    hipLaunchKernelGGL(k_assemble_gather, grid, dim3(ASM_THREADS), 0, st, A);
    if (int rc = check_launch("k_assemble_gather")) return rc;
    if (!pose_out) return SDN_OK;
    hipLaunchKernelGGL(k_assemble_paint, grid, dim3(ASM_THREADS), 0, st, A);
    return check_launch("k_assemble_paint");
}
