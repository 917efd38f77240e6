// The input side of the textural networks: Pix2PixHDModel.encode_input's label planes, edge plane and pose planes
// (textural/models/pix2pixHD_model.py:124-166 with get_edges :343-349) and the instance numbering of Encoder.forward
// (networks.py:310-325).  The reference builds the planes with zeros + long + scatter_ twice, about ten slice / compare / or
// launches and a cat, and numbers the instances by sorting every pixel (np.unique / torch.unique).  Here:
//   k_encode_maps   one launch: a lane owns four adjacent pixels of a row (16-byte plane stores) when W % 4 == 0 and the bases are
//                   16-byte aligned, one pixel otherwise; it reads the label, the pose and the instance value with its four
//                   neighbours from global memory and writes every plane of both outputs.  An index outside [0, channels) or a
//                   NaN sets no plane and is counted in bad[0] (label) / bad[1] (pose).
//   k_inst_mark     inst[i] = inst[i] * bs + i in place, and the presence bit of every key in a 2^21-bit window (atomicOr, skipped
//                   while a lane's key repeats or the workgroup has set it); keys outside the window are counted in `overflow`
//   k_inst_scan     one workgroup: the exclusive popcount prefix of the bitmap's words, K, and the ids in ascending order
//   k_inst_rank     seg = prefix[word] + popc(bits below); with counts, the pixels per id through integer atomics, summed per
//                   lane run and per workgroup (in LDS) first
// The element types are wave-uniform runtime switches.  The only atomics are integer ones: the same bits every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "encode_input_check.h"
#include "sdn_common.h"

namespace sdn {

// NP adjacent values of a map as floats' bits or ints: raw[e] holds the value converted to int32 (integer maps) or the float's
// bits (fp32 maps)
template <int NP>
__device__ __forceinline__ void enc_load(const void* __restrict__ base, int dt, long at, int (&raw)[NP])
{
    if (dt == ENC_U8) {
        const uint8_t* p = static_cast<const uint8_t*>(base) + at;
        if constexpr (NP == 4) {
            const uchar4 q = *reinterpret_cast<const uchar4*>(p);
            raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
        } else {
            raw[0] = p[0];
        }
    } else if (dt == ENC_I16) {
        const int16_t* p = static_cast<const int16_t*>(base) + at;
        if constexpr (NP == 4) {
            const short4 q = *reinterpret_cast<const short4*>(p);
            raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
        } else {
            raw[0] = p[0];
        }
    } else {   // 4-byte elements: the bits
        const int32_t* p = static_cast<const int32_t*>(base) + at;
        if constexpr (NP == 4) {
            const int4 q = *reinterpret_cast<const int4*>(p);
            raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
        } else {
            raw[0] = p[0];
        }
    }
}

__device__ __forceinline__ int enc_load1(const void* __restrict__ base, int dt, long at)
{
    int r[1];
    enc_load<1>(base, dt, at, r);
    return r[0];
}

// `!=` in the map's own dtype: NaN differs from everything, -0 equals 0
__device__ __forceinline__ bool enc_differs(int a, int b, bool is_float)
{
    return is_float ? (__int_as_float(a) != __int_as_float(b)) : (a != b);
}

__device__ __forceinline__ int enc_channel(int raw, int dt, int channels)
{
    return dt == ENC_F32 ? enc_channel_f32(__int_as_float(raw), channels) : enc_channel_i32(raw, channels);
}

// the planes of NP pixels: 1.0f in the plane of each pixel's channel, 0.0f elsewhere; every element is written
template <int NP>
__device__ __forceinline__ void enc_store_planes(float* __restrict__ out, long HW, int channels, const int (&ch)[NP])
{
    for (int c = 0; c < channels; c++) {
        if constexpr (NP == 4)
            *reinterpret_cast<float4*>(out + (long)c * HW) =
                make_float4(ch[0] == c ? 1.f : 0.f, ch[1] == c ? 1.f : 0.f, ch[2] == c ? 1.f : 0.f, ch[3] == c ? 1.f : 0.f);
        else
            out[(long)c * HW] = ch[0] == c ? 1.f : 0.f;
    }
}

// groups: N * H * (W / NP) groups of NP adjacent pixels of a row
template <int NP>
__global__ __launch_bounds__(ENC_THREADS) void k_encode_maps(const void* __restrict__ label, int label_dt, const void* __restrict__ inst,
                                                            int inst_dt, const void* __restrict__ pose, int pose_dt, int H, int W,
                                                            long groups, int label_nc, int pose_ch, float* __restrict__ input_label,
                                                            float* __restrict__ pose_onehot, int* __restrict__ bad)
{
    const long HW = (long)H * W;
    const int gw = W / NP;               // groups of a row
    const int planes = label_nc + (inst ? 1 : 0);
    const bool inst_float = inst_dt == ENC_F32;
    int bad_label = 0, bad_pose = 0;
    for (long g0 = (long)blockIdx.x * ENC_THREADS; g0 < groups; g0 += (long)gridDim.x * ENC_THREADS) {
        const long g = g0 + threadIdx.x;
        if (g >= groups) continue;
        const long row = g / gw;                       // n * H + y
        const int x = (int)(g - row * gw) * NP;
        const int n = (int)(row / H), y = (int)(row - (long)n * H);
        const long at = row * W + x;                   // element of a [N, 1, H, W] map
        const long p = (long)y * W + x;                // pixel of the plane

        int raw[NP], ch[NP];
        enc_load<NP>(label, label_dt, at, raw);
#pragma unroll
        for (int e = 0; e < NP; e++) {
            ch[e] = enc_channel(raw[e], label_dt, label_nc);
            bad_label += ch[e] < 0 ? 1 : 0;
        }
        float* out = input_label + (long)n * planes * HW + p;
        enc_store_planes<NP>(out, HW, label_nc, ch);

        if (inst) {
            // get_edges: a pixel is an edge when it differs from its left, right, upper or lower neighbour (inside the map)
            int v[NP], up[NP], dn[NP];
            enc_load<NP>(inst, inst_dt, at, v);
            const bool has_up = y > 0, has_dn = y < H - 1, has_l = x > 0, has_r = x + NP < W;
            if (has_up) enc_load<NP>(inst, inst_dt, at - W, up);
            if (has_dn) enc_load<NP>(inst, inst_dt, at + W, dn);
            const int left = has_l ? enc_load1(inst, inst_dt, at - 1) : 0;
            const int right = has_r ? enc_load1(inst, inst_dt, at + NP) : 0;
            float edge[NP];
#pragma unroll
            for (int e = 0; e < NP; e++) {
                bool d = e > 0 ? enc_differs(v[e], v[e - 1], inst_float) : (has_l && enc_differs(v[e], left, inst_float));
                d = d || (e < NP - 1 ? enc_differs(v[e], v[e + 1 < NP ? e + 1 : e], inst_float) : (has_r && enc_differs(v[e], right, inst_float)));
                d = d || (has_up && enc_differs(v[e], up[e], inst_float));
                d = d || (has_dn && enc_differs(v[e], dn[e], inst_float));
                edge[e] = d ? 1.f : 0.f;
            }
            float* eo = out + (long)label_nc * HW;
            if constexpr (NP == 4) *reinterpret_cast<float4*>(eo) = make_float4(edge[0], edge[1], edge[2], edge[3]);
            else eo[0] = edge[0];
        }

        if (pose_ch > 0) {
            enc_load<NP>(pose, pose_dt, at, raw);
#pragma unroll
            for (int e = 0; e < NP; e++) {
                ch[e] = enc_channel(raw[e], pose_dt, pose_ch);
                bad_pose += ch[e] < 0 ? 1 : 0;
            }
            enc_store_planes<NP>(pose_onehot + (long)n * pose_ch * HW + p, HW, pose_ch, ch);
        }
    }
    // every lane of the wave is here again: one atomic per wave, and only for a wave that met a bad index
    bad_label = wave_sum(bad_label);
    bad_pose = wave_sum(bad_pose);
    if ((threadIdx.x & 63) == 0) {
        if (bad_label) atomicAdd(&bad[0], bad_label);
        if (bad_pose) atomicAdd(&bad[1], bad_pose);
    }
}

// ---- instance numbering ------------------------------------------------------------------------------------------------------------
// NP adjacent values of image i: disambiguated in place; bit[e] = the key's bit or -1
template <int NP>
__device__ __forceinline__ void idx_mark_group(void* __restrict__ inst, int dt, long at, int bs, int i, int (&bit)[NP])
{
    if (dt == ENC_F32) {
        float* p = static_cast<float*>(inst) + at;
        float v[NP];
        if constexpr (NP == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = p[0];
        }
#pragma unroll
        for (int e = 0; e < NP; e++) {
            v[e] = idx_disambiguate_f32(v[e], bs, i);
            bit[e] = idx_bit_f32(v[e]);
        }
        if constexpr (NP == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        else p[0] = v[0];
    } else if (dt == ENC_I32) {
        int32_t* p = static_cast<int32_t*>(inst) + at;
        int32_t v[NP];
        if constexpr (NP == 4) {
            const int4 q = *reinterpret_cast<const int4*>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = p[0];
        }
#pragma unroll
        for (int e = 0; e < NP; e++) {
            v[e] = idx_disambiguate_i32(v[e], bs, i);
            bit[e] = idx_bit_i32(v[e]);
        }
        if constexpr (NP == 4) *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
        else p[0] = v[0];
    } else {
        int16_t* p = static_cast<int16_t*>(inst) + at;
        int16_t v[NP];
        if constexpr (NP == 4) {
            const short4 q = *reinterpret_cast<const short4*>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = p[0];
        }
#pragma unroll
        for (int e = 0; e < NP; e++) {
            v[e] = idx_disambiguate_i16(v[e], bs, i);
            bit[e] = idx_bit_i32((int32_t)v[e]);
        }
        if constexpr (NP == 4) *reinterpret_cast<short4*>(p) = make_short4(v[0], v[1], v[2], v[3]);
        else p[0] = v[0];
    }
}

// the bits of NP adjacent, already disambiguated values
template <int NP>
__device__ __forceinline__ void idx_bits_group(const void* __restrict__ inst, int dt, long at, int (&bit)[NP])
{
    int raw[NP];
    enc_load<NP>(inst, dt, at, raw);
#pragma unroll
    for (int e = 0; e < NP; e++) bit[e] = dt == ENC_F32 ? idx_bit_f32(__int_as_float(raw[e])) : idx_bit_i32(raw[e]);
}

// groups of NP adjacent pixels of one image: HW % NP == 0.  An instance map repeats a few dozen keys over millions of pixels, and
// atomics on one word run one after the other: a lane skips the key it set last, and a workgroup gathers its bits in LDS first
// (a direct-mapped table, slot = word mod IDX_LDS_SLOTS, read plainly before anything atomic) and sets each word it used with one
// global atomicOr at the end.  A word that finds its slot taken by another goes straight to the global bitmap.
template <int NP>
__global__ __launch_bounds__(ENC_THREADS) void k_inst_mark(void* __restrict__ inst, int dt, int bs, long HW, long groups,
                                                          uint32_t* __restrict__ bitmap, int* __restrict__ head)
{
    __shared__ int word_of[IDX_LDS_SLOTS];
    __shared__ unsigned bits_of[IDX_LDS_SLOTS];
    for (int h = threadIdx.x; h < IDX_LDS_SLOTS; h += ENC_THREADS) {
        word_of[h] = -1;
        bits_of[h] = 0u;
    }
    __syncthreads();
    int last = -1, over = 0;
    for (long g0 = (long)blockIdx.x * ENC_THREADS; g0 < groups; g0 += (long)gridDim.x * ENC_THREADS) {
        const long g = g0 + threadIdx.x;
        if (g >= groups) continue;
        const long at = g * NP;
        const int i = (int)(at / HW);
        int bit[NP];
        idx_mark_group<NP>(inst, dt, at, bs, i, bit);
#pragma unroll
        for (int e = 0; e < NP; e++) {
            if (bit[e] < 0) {
                over++;
            } else if (bit[e] != last) {
                last = bit[e];
                const int w = bit[e] >> 5, h = w & (IDX_LDS_SLOTS - 1);
                const unsigned m = 1u << (bit[e] & 31);
                const int owner = *static_cast<volatile int*>(&word_of[h]);
                if (owner == w && (*static_cast<volatile unsigned*>(&bits_of[h]) & m)) continue;   // set already: the common case
                const int was = owner == w ? w : atomicCAS(&word_of[h], -1, w);
                if (was == -1 || was == w) atomicOr(&bits_of[h], m);
                else atomicOr(&bitmap[w], m);
            }
        }
    }
    __syncthreads();
    for (int h = threadIdx.x; h < IDX_LDS_SLOTS; h += ENC_THREADS)
        if (bits_of[h]) atomicOr(&bitmap[word_of[h]], bits_of[h]);
    over = wave_sum(over);
    if ((threadIdx.x & 63) == 0 && over) atomicAdd(&head[1], over);
}

// one workgroup.  Wave v owns the words [4096 v, 4096 v + 4096); in step j its lanes read 64 x 4 consecutive words (one 16-byte
// load each, 1 KiB per wave), scan their set bits across the wave and carry the total to the next step; the waves' totals meet in
// LDS.  Then the ids, word w by thread w % 1024, eight words in flight per thread, so that neighbouring ids are written by
// neighbouring lanes.
__global__ __launch_bounds__(IDX_SCAN_THREADS) void k_inst_scan(const uint32_t* __restrict__ bitmap, int* __restrict__ prefix,
                                                               int* __restrict__ head, int64_t* __restrict__ ids,
                                                               int64_t* __restrict__ counts, long id_capacity)
{
    __shared__ int wave_total[IDX_SCAN_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint4* mine = reinterpret_cast<const uint4*>(bitmap + (long)wave * IDX_WAVE_WORDS) + lane;
    int pc[IDX_SCAN_STEPS];     // the set bits of a lane's four words of step j, a byte each (at most 32)
    int excl[IDX_SCAN_STEPS];   // the set bits of the wave's words before them
    int run = 0;                // the set bits of the wave's words before step j: the same in every lane
#pragma unroll
    for (int j = 0; j < IDX_SCAN_STEPS; j++) {
        const uint4 q = mine[j * 64];
        const int a = __popc(q.x), b = __popc(q.y), c = __popc(q.z), d = __popc(q.w);
        pc[j] = a | (b << 8) | (c << 16) | (d << 24);
        const int sum = a + b + c + d;
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        excl[j] = run + incl - sum;
        run += __shfl(incl, 63, 64);
    }
    if (lane == 0) wave_total[wave] = run;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < IDX_SCAN_WAVES; w++) {
        const int s = wave_total[w];
        before += w < wave ? s : 0;
        total += s;
    }
    int4* pout = reinterpret_cast<int4*>(prefix + (long)wave * IDX_WAVE_WORDS) + lane;
#pragma unroll
    for (int j = 0; j < IDX_SCAN_STEPS; j++) {
        const int a = pc[j] & 255, b = (pc[j] >> 8) & 255, c = (pc[j] >> 16) & 255;
        const int r = before + excl[j];
        pout[j * 64] = make_int4(r, r + a, r + a + b, r + a + b + c);
    }
    if (t == 0) head[0] = total;
    __syncthreads();   // the prefixes of the whole workgroup are visible to it
    constexpr int FLIGHT = 8;
    for (int w0 = t; w0 < IDX_WORDS; w0 += FLIGHT * IDX_SCAN_THREADS) {
        uint32_t bits[FLIGHT];
#pragma unroll
        for (int f = 0; f < FLIGHT; f++) bits[f] = bitmap[w0 + f * IDX_SCAN_THREADS];
#pragma unroll
        for (int f = 0; f < FLIGHT; f++) {
            if (!bits[f]) continue;
            const int w = w0 + f * IDX_SCAN_THREADS;
            long k = prefix[w];
            while (bits[f]) {
                const int b = __ffs(bits[f]) - 1;
                bits[f] &= bits[f] - 1;
                if (k < id_capacity) {
                    ids[k] = idx_key_of_bit(w * 32 + b);
                    if (counts) counts[k] = 0;
                }
                k++;
            }
        }
    }
}

// counts: the pixels of a lane's run go to a direct-mapped LDS table of the workgroup (slot = id mod IDX_LDS_SLOTS: no two ids
// share a slot while K <= IDX_LDS_SLOTS), an id that finds its slot taken goes straight to the global count; at the end one
// global atomic per used slot.  Integer sums: the same counts whatever the order.
template <int NP>
__global__ __launch_bounds__(ENC_THREADS) void k_inst_rank(const void* __restrict__ inst, int dt, long groups,
                                                          const uint32_t* __restrict__ bitmap, const int* __restrict__ prefix,
                                                          int32_t* __restrict__ seg, unsigned long long* __restrict__ counts)
{
    __shared__ int owner[IDX_LDS_SLOTS];
    __shared__ unsigned pixels[IDX_LDS_SLOTS];
    if (counts) {
        for (int h = threadIdx.x; h < IDX_LDS_SLOTS; h += ENC_THREADS) {
            owner[h] = -1;
            pixels[h] = 0u;
        }
        __syncthreads();
    }
    for (long g0 = (long)blockIdx.x * ENC_THREADS; g0 < groups; g0 += (long)gridDim.x * ENC_THREADS) {
        const long g = g0 + threadIdx.x;
        if (g >= groups) continue;
        int bit[NP], s[NP];
        idx_bits_group<NP>(inst, dt, g * NP, bit);
#pragma unroll
        for (int e = 0; e < NP; e++) {
            if (e > 0 && bit[e] == bit[e - 1]) s[e] = s[e - 1];
            else s[e] = bit[e] >= 0 ? idx_rank(prefix[bit[e] >> 5], bitmap[bit[e] >> 5], bit[e]) : -1;
        }
        if constexpr (NP == 4) *reinterpret_cast<int4*>(seg + g * NP) = make_int4(s[0], s[1], s[2], s[3]);
        else seg[g] = s[0];
        if (!counts) continue;
        // a lane's runs of equal ids: one addition per run
        int run = 0;
#pragma unroll
        for (int e = 0; e < NP; e++) {
            run++;
            if (e == NP - 1 || s[e + 1 < NP ? e + 1 : e] != s[e]) {
                if (s[e] >= 0) {
                    const int h = s[e] & (IDX_LDS_SLOTS - 1);
                    const int held = *static_cast<volatile int*>(&owner[h]);
                    const int was = held == s[e] ? held : atomicCAS(&owner[h], -1, s[e]);
                    if (was == -1 || was == s[e]) atomicAdd(&pixels[h], (unsigned)run);
                    else atomicAdd(&counts[s[e]], (unsigned long long)run);
                }
                run = 0;
            }
        }
    }
    if (counts) {
        __syncthreads();
        for (int h = threadIdx.x; h < IDX_LDS_SLOTS; h += ENC_THREADS)
            if (pixels[h]) atomicAdd(&counts[owner[h]], (unsigned long long)pixels[h]);
    }
}

static bool enc_aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
static unsigned enc_grid(long groups, int cap)
{
    const long b = (groups + ENC_THREADS - 1) / ENC_THREADS;
    return (unsigned)(b < cap ? b : cap);
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_encode_maps(const void* label, int label_dtype, const void* inst, int inst_dtype, const void* pose, int pose_dtype, int N,
                            int H, int W, int label_nc, int pose_ch, float* input_label, float* pose_onehot, int32_t* bad,
                            sdnStream stream)
{
    char why[256];
    if (enc_validate_maps(label, label_dtype, inst, inst_dtype, pose, pose_dtype, N, H, W, label_nc, pose_ch, input_label, pose_onehot,
                          bad, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_encode_maps: %s", why);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, 2 * sizeof(int32_t), st) != hipSuccess) return check_launch("sdn_encode_maps: clearing bad");
    if (pose_ch == 0) pose = nullptr;
    const bool vec = (W & 3) == 0 && enc_aligned16(label) && enc_aligned16(inst) && enc_aligned16(pose) && enc_aligned16(input_label) &&
                     enc_aligned16(pose_onehot);
    if (vec) {
        const long groups = (long)N * H * (W / 4);
        hipLaunchKernelGGL(k_encode_maps<4>, dim3(enc_grid(groups, ENC_MAX_BLOCKS)), dim3(ENC_THREADS), 0, st, label, label_dtype, inst,
                           inst_dtype, pose, pose_dtype, H, W, groups, label_nc, pose_ch, input_label, pose_onehot, bad);
    } else {
        const long groups = (long)N * H * W;
        hipLaunchKernelGGL(k_encode_maps<1>, dim3(enc_grid(groups, ENC_MAX_BLOCKS)), dim3(ENC_THREADS), 0, st, label, label_dtype, inst,
                           inst_dtype, pose, pose_dtype, H, W, groups, label_nc, pose_ch, input_label, pose_onehot, bad);
    }
    return check_launch("k_encode_maps");
}

SDN_API int sdn_inst_index_workspace_bytes(size_t* bytes)
{
    if (!bytes) return fail(SDN_EINVAL, "sdn_inst_index_workspace_bytes: bytes is NULL");
    *bytes = IDX_WORKSPACE_BYTES;
    return SDN_OK;
}

SDN_API int sdn_inst_index_build(void* inst, int inst_dtype, int N, int H, int W, void* workspace, size_t workspace_bytes, int64_t* ids,
                                 int64_t* counts, long id_capacity, sdnStream stream)
{
    char why[256];
    if (idx_validate_build(inst, inst_dtype, N, H, W, workspace, workspace_bytes, ids, counts, id_capacity, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_inst_index_build: %s", why);
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + IDX_BITMAP_AT);
    int* prefix = reinterpret_cast<int*>(ws + IDX_PREFIX_AT);
    int* head = reinterpret_cast<int*>(ws + IDX_HEAD_AT);
    // the bitmap and the head behind it in one go; the prefixes are all written by k_inst_scan
    static_assert(IDX_BITMAP_AT == 0 && IDX_HEAD_AT == (size_t)IDX_WORDS * 4, "one memset clears the bitmap and the head");
    if (hipMemsetAsync(ws, 0, IDX_HEAD_AT + 16, st) != hipSuccess) return check_launch("sdn_inst_index_build: clearing the workspace");
    const long HW = (long)H * W, total = (long)N * HW;
    if ((HW & 3) == 0 && enc_aligned16(inst)) {
        const long groups = total / 4;
        hipLaunchKernelGGL(k_inst_mark<4>, dim3(enc_grid(groups, IDX_MAX_BLOCKS)), dim3(ENC_THREADS), 0, st, inst, inst_dtype, N, HW,
                           groups, bitmap, head);
    } else {
        hipLaunchKernelGGL(k_inst_mark<1>, dim3(enc_grid(total, IDX_MAX_BLOCKS)), dim3(ENC_THREADS), 0, st, inst, inst_dtype, N, HW, total,
                           bitmap, head);
    }
    if (int rc = check_launch("k_inst_mark")) return rc;
    hipLaunchKernelGGL(k_inst_scan, dim3(1), dim3(IDX_SCAN_THREADS), 0, st, bitmap, prefix, head, ids, counts, id_capacity);
    return check_launch("k_inst_scan");
}

SDN_API int sdn_inst_index_rank(const void* inst, int inst_dtype, int N, int H, int W, const void* workspace, size_t workspace_bytes,
                                int32_t* seg, int64_t* counts, sdnStream stream)
{
    char why[256];
    if (idx_validate_rank(inst, inst_dtype, N, H, W, workspace, workspace_bytes, seg, counts, why, sizeof(why)))
        return fail(SDN_EINVAL, "sdn_inst_index_rank: %s", why);
    hipStream_t st = (hipStream_t)stream;
    const char* ws = static_cast<const char*>(workspace);
    const uint32_t* bitmap = reinterpret_cast<const uint32_t*>(ws + IDX_BITMAP_AT);
    const int* prefix = reinterpret_cast<const int*>(ws + IDX_PREFIX_AT);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    const long total = (long)N * H * W;
    if ((total & 3) == 0 && enc_aligned16(inst) && enc_aligned16(seg)) {
        const long groups = total / 4;
        hipLaunchKernelGGL(k_inst_rank<4>, dim3(enc_grid(groups, IDX_MAX_BLOCKS)), dim3(ENC_THREADS), 0, st, inst, inst_dtype, groups,
                           bitmap, prefix, seg, cnt);
    } else {
        hipLaunchKernelGGL(k_inst_rank<1>, dim3(enc_grid(total, IDX_MAX_BLOCKS)), dim3(ENC_THREADS), 0, st, inst, inst_dtype, total, bitmap,
                           prefix, seg, cnt);
    }
    return check_launch("k_inst_rank");
}
