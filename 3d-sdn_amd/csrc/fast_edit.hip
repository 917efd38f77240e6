// Textural inputs of a batch of EDITED frames (textural/edit_vkitti.py:62-103, edit_benchmark.py:87-126): the label map with
// the source's cars removed and the edited frame's cars added, the instance map, the pose-bin map and -- the point of the
// edit -- the source frame's per-instance appearance code painted at each instance's NEW pixels.  The reference does it
// on the host: per JSON object three masked in-place writes, then np.unique + nonzero + feat_num indexed writes per
// instance.  Raw object ids are at most 255 and 1000 k >= 1000, so those sequential rewrites never alias and the whole
// block is a per-pixel function of (source label, raw id) through two 256-entry tables per frame:
//   s = source label, 2 / 12 (car / van) -> 5 (misc);  k = raw object id of the edited frame
//   k in the JSON:  segm = obj_label[k], inst = 1000 k, pose = obj_pose[k]
//   otherwise:      segm = s, inst = (k == 0 ? s : k), pose = 0
//   feat[c] = codes[c, row of inst in code_ids], or 0 (and one more in missing[f]) when the source has no such instance
// One launch for F frames.  Pure streaming, HBM-bound: 5 B read and 4 (2 + P + C) B written per pixel, no reuse.  Four
// pixels per thread, one 128-bit store per output plane; the tables (2 x 256 ints, the sorted ids padded to a power of two
// for a branch-free binary search, the codes) sit in LDS, loaded once per workgroup; the grid is sized per CU and strides.
#include <hip/hip_runtime.h>

#include <climits>

#include "sdn_common.h"

namespace sdn {

constexpr int EDIT_THREADS = 256;
constexpr int EDIT_PIX = 4;                     // pixels per thread and step: one float4 per plane
constexpr int EDIT_LDS_WORDS = 12288;           // ids (padded) + codes kept in LDS: 48 KiB beside the 2 KiB of object tables
constexpr int EDIT_BLOCKS = 2048;               // 256 CUs x 8 workgroups: the rest of the pixels is reached by striding

struct EditParams {
    const float* base_segm;      // [1 | F, HW]
    long base_stride;            // 0 or HW
    const uint8_t* edit_inst;    // [F, HW]
    const int32_t* obj_label;    // [F, 256]
    const int32_t* obj_pose;     // [F, 256]
    const int32_t* code_ids;     // [K] ascending
    const float* codes;          // [C, K]
    int K, Kpad, C, HW, P;
    float *segm, *inst, *pose, *feat;   // [F, 1 | 1 | P | C, HW]
    int32_t* missing;            // [F]
};

// VEC: HW is a multiple of 4 and every plane is 16-byte aligned, so a thread's four pixels move as one 128-bit access
template <bool VEC>
__global__ __launch_bounds__(EDIT_THREADS) void k_edit_assemble(const EditParams A)
{
    __shared__ int s_label[256];
    __shared__ int s_pose[256];
    __shared__ int s_missing;
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];
    int* s_ids = s_dyn;                                      // [Kpad], INT_MAX beyond K
    float* s_codes = reinterpret_cast<float*>(s_dyn + A.Kpad);   // [C, K]
    const int f = blockIdx.y;
    const int tid = threadIdx.x;
    s_label[tid] = A.obj_label[f * 256 + tid];               // EDIT_THREADS == 256
    s_pose[tid] = A.obj_pose[f * 256 + tid];
    for (int i = tid; i < A.Kpad; i += EDIT_THREADS) s_ids[i] = i < A.K ? A.code_ids[i] : INT_MAX;
    for (int i = tid; i < A.C * A.K; i += EDIT_THREADS) s_codes[i] = A.codes[i];
    if (tid == 0) s_missing = 0;
    __syncthreads();

    const int HW = A.HW;
    const float* bs = A.base_segm + (size_t)f * A.base_stride;
    const uint8_t* ei = A.edit_inst + (size_t)f * HW;
    float* o_segm = A.segm + (size_t)f * HW;
    float* o_inst = A.inst + (size_t)f * HW;
    float* o_pose = A.pose + (size_t)f * A.P * HW;
    float* o_feat = A.feat + (size_t)f * A.C * HW;
    const int groups = (HW + EDIT_PIX - 1) / EDIT_PIX;
    int lost = 0;
    for (int g = blockIdx.x * EDIT_THREADS + tid; g < groups; g += gridDim.x * EDIT_THREADS) {
        const int p0 = g * EDIT_PIX;
        float sv[EDIT_PIX];
        int kv[EDIT_PIX];
        if (VEC) {
            const float4 s4 = *reinterpret_cast<const float4*>(bs + p0);
            const uchar4 k4 = *reinterpret_cast<const uchar4*>(ei + p0);
            sv[0] = s4.x; sv[1] = s4.y; sv[2] = s4.z; sv[3] = s4.w;
            kv[0] = k4.x; kv[1] = k4.y; kv[2] = k4.z; kv[3] = k4.w;
        } else {
#pragma unroll
            for (int j = 0; j < EDIT_PIX; j++) {
                const bool in = p0 + j < HW;
                sv[j] = in ? bs[p0 + j] : 0.f;
                kv[j] = in ? ei[p0 + j] : 0;
            }
        }
        float segm[EDIT_PIX], inst[EDIT_PIX], pose[EDIT_PIX];
        int row[EDIT_PIX];
#pragma unroll
        for (int j = 0; j < EDIT_PIX; j++) {
            int s = (int)sv[j];
            s = (s == 2 || s == 12) ? 5 : s;
            const int k = kv[j];
            const int ol = s_label[k];
            const bool listed = ol != 0;
            const int sg = listed ? ol : s;
            const int id = listed ? 1000 * k : (k == 0 ? sg : k);
            segm[j] = (float)sg;
            inst[j] = (float)id;
            pose[j] = (float)s_pose[k];
            // lower bound over the padded, ascending ids: log2(Kpad) steps, no branch
            int pos = 0;
            for (int half = A.Kpad >> 1; half > 0; half >>= 1) pos += s_ids[pos + half - 1] < id ? half : 0;
            const bool found = s_ids[pos] == id;
            row[j] = found ? pos : -1;
            if (!found && (VEC || p0 + j < HW)) lost++;
        }
        if (VEC) {
            *reinterpret_cast<float4*>(o_segm + p0) = make_float4(segm[0], segm[1], segm[2], segm[3]);
            *reinterpret_cast<float4*>(o_inst + p0) = make_float4(inst[0], inst[1], inst[2], inst[3]);
            if (A.P == 1) {
                *reinterpret_cast<float4*>(o_pose + p0) = make_float4(pose[0], pose[1], pose[2], pose[3]);
            } else {   // feat_pose_num_bins == 0: the reference allocates two channels and never writes them
                for (int c = 0; c < A.P; c++) *reinterpret_cast<float4*>(o_pose + (size_t)c * HW + p0) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            for (int c = 0; c < A.C; c++) {
                const float* cc = s_codes + c * A.K;
                float4 v;
                v.x = row[0] >= 0 ? cc[row[0]] : 0.f;
                v.y = row[1] >= 0 ? cc[row[1]] : 0.f;
                v.z = row[2] >= 0 ? cc[row[2]] : 0.f;
                v.w = row[3] >= 0 ? cc[row[3]] : 0.f;
                *reinterpret_cast<float4*>(o_feat + (size_t)c * HW + p0) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < EDIT_PIX; j++) {
                const int p = p0 + j;
                if (p >= HW) break;
                o_segm[p] = segm[j];
                o_inst[p] = inst[j];
                for (int c = 0; c < A.P; c++) o_pose[(size_t)c * HW + p] = A.P == 1 ? pose[j] : 0.f;
                for (int c = 0; c < A.C; c++) o_feat[(size_t)c * HW + p] = row[j] >= 0 ? s_codes[c * A.K + row[j]] : 0.f;
            }
        }
    }
    // pixels without a code: summed over the wave, one LDS add per wave, one global add per workgroup that lost any
    for (int off = 32; off > 0; off >>= 1) lost += __shfl_down(lost, off, 64);
    if ((tid & 63) == 0 && lost) atomicAdd(&s_missing, lost);
    __syncthreads();
    if (tid == 0 && s_missing) atomicAdd(A.missing + f, s_missing);
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_edit_assemble(const float* base_segm, long base_stride, const uint8_t* edit_inst, const int32_t* obj_label,
                              const int32_t* obj_pose, const int32_t* code_ids, const float* codes, int K, int C, int F, int HW,
                              int pose_channels, float* segm_out, float* inst_out, float* pose_out, float* feat_out,
                              int32_t* missing, sdnStream stream)
{
    if (!base_segm || !edit_inst || !obj_label || !obj_pose || !code_ids || !codes || !segm_out || !inst_out || !pose_out ||
        !feat_out || !missing)
        return fail(SDN_EINVAL, "sdn_edit_assemble: null pointer");
    if (K < 1 || C < 1 || F < 1 || F > 65535 || HW < 1 || HW > INT_MAX - EDIT_PIX) return fail(SDN_EINVAL, "sdn_edit_assemble: bad sizes");
    if (pose_channels != 1 && pose_channels != 2) return fail(SDN_EINVAL, "sdn_edit_assemble: pose_channels must be 1 or 2");
    if (base_stride != 0 && base_stride != HW) return fail(SDN_EINVAL, "sdn_edit_assemble: base_stride must be 0 or HW");
    int Kpad = 1;
    while (Kpad < K) Kpad <<= 1;
    if ((long)Kpad + (long)C * K > EDIT_LDS_WORDS)
        return fail(SDN_EINVAL, "sdn_edit_assemble: %d codes of %d channels do not fit the LDS tables (%d words)", K, C,
                    EDIT_LDS_WORDS);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(missing, 0, (size_t)F * sizeof(int32_t), st);
    if (e != hipSuccess) return fail(SDN_ELAUNCH, "sdn_edit_assemble: memset: %s", hipGetErrorString(e));
    EditParams A;
    A.base_segm = base_segm; A.base_stride = base_stride; A.edit_inst = edit_inst; A.obj_label = obj_label; A.obj_pose = obj_pose;
    A.code_ids = code_ids; A.codes = codes; A.K = K; A.Kpad = Kpad; A.C = C; A.HW = HW; A.P = pose_channels;
    A.segm = segm_out; A.inst = inst_out; A.pose = pose_out; A.feat = feat_out; A.missing = missing;
    const int groups = (HW + EDIT_PIX - 1) / EDIT_PIX;
    int bx = (groups + EDIT_THREADS - 1) / EDIT_THREADS;
    const int cap = EDIT_BLOCKS / F > 1 ? EDIT_BLOCKS / F : 1;
    if (bx > cap) bx = cap;
    const size_t lds = ((size_t)Kpad + (size_t)C * K) * sizeof(int);
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const bool vec = HW % EDIT_PIX == 0 && a16(base_segm) && a16(segm_out) && a16(inst_out) && a16(pose_out) && a16(feat_out) &&
                     ((uintptr_t)edit_inst & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(k_edit_assemble<true>, dim3((unsigned)bx, (unsigned)F), dim3(EDIT_THREADS), lds, st, A);
    else
        hipLaunchKernelGGL(k_edit_assemble<false>, dim3((unsigned)bx, (unsigned)F), dim3(EDIT_THREADS), lds, st, A);
    return check_launch("k_edit_assemble");
}
