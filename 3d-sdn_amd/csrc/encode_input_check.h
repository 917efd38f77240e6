// Index, key, bitmap and prefix arithmetic and HOST argument validation of the textural input encoding (encode_input.hip).  Plain
// C++ so that a host program can walk the validators, the key rule, the window's edges and the rank arithmetic without the HIP
// runtime (tools/encode_input_check.cpp).
#pragma once

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"

namespace sdn {

// element types of the maps (include/sdn_hip.h: SDN_MAP_*)
constexpr int ENC_U8 = 0, ENC_I16 = 1, ENC_I32 = 2, ENC_F32 = 3;
constexpr int ENC_THREADS = 256;
constexpr int ENC_MAX_BLOCKS = 2048;        // grid cap of k_encode_maps; the rest is a grid stride
constexpr int ENC_MAX_CHANNELS = 256;       // label_nc and pose_ch

SDN_HD int enc_elem_bytes(int dt) { return dt == ENC_U8 ? 1 : dt == ENC_I16 ? 2 : 4; }

// the channel of a one-hot index map's value: the value truncated toward zero (.long()) when that lies in [0, channels), else -1
// (counted in `bad`).  trunc(v) in [0, channels)  <=>  -1 < v < channels; NaN fails both comparisons.
SDN_HD int enc_channel_f32(float v, int channels) { return (v > -1.0f && v < (float)channels) ? (int)v : -1; }
SDN_HD int enc_channel_i32(int v, int channels) { return (v >= 0 && v < channels) ? v : -1; }

// ---- instance numbering ------------------------------------------------------------------------------------------------------------
constexpr int IDX_KEY_MIN = -32768;                      // every int16 value lies inside the window
constexpr int IDX_BITS = 1 << 21;                        // keys [IDX_KEY_MIN, IDX_KEY_MIN + IDX_BITS)
constexpr int IDX_WORDS = IDX_BITS / 32;                 // 65536 words of presence bits: 256 KiB
constexpr int IDX_SCAN_THREADS = 1024;                   // the one workgroup of k_inst_scan
constexpr int IDX_SCAN_WAVES = IDX_SCAN_THREADS / 64;
constexpr int IDX_WAVE_WORDS = IDX_WORDS / IDX_SCAN_WAVES;            // 4096 consecutive words per wave
constexpr int IDX_SCAN_STEPS = IDX_WAVE_WORDS / (64 * 4);             // 16 steps of 64 lanes x 4 words
constexpr int IDX_MAX_BLOCKS = 512;                      // grid cap of k_inst_mark / k_inst_rank; the rest is a grid stride
constexpr int IDX_LDS_SLOTS = 1024;                      // a workgroup's table of the keys it has set / the ids it is counting
static_assert((IDX_LDS_SLOTS & (IDX_LDS_SLOTS - 1)) == 0, "slot = key mod a power of two");
static_assert(IDX_SCAN_WAVES * IDX_SCAN_STEPS * 64 * 4 == IDX_WORDS && IDX_WORDS % (8 * IDX_SCAN_THREADS) == 0, "the scan covers every word once");

// workspace: bitmap u32 [IDX_WORDS]; the head, 16 bytes: K and overflow (the 8 bytes the caller copies to the host); prefix i32
// [IDX_WORDS].  The bitmap and the head are cleared together.
constexpr size_t IDX_BITMAP_AT = 0;
constexpr size_t IDX_HEAD_AT = (size_t)IDX_WORDS * 4;
constexpr size_t IDX_PREFIX_AT = IDX_HEAD_AT + 16;
constexpr size_t IDX_WORKSPACE_BYTES = IDX_PREFIX_AT + (size_t)IDX_WORDS * 4;

// `inst[i] = inst[i] * bs + i` in the tensor's own dtype (networks.py:313-316).  fp32: a product and a sum, each rounded (the
// kernels are built without contraction); int32 / int16: wraparound, as torch's integer kernels give.
SDN_HD float idx_disambiguate_f32(float v, int bs, int i) { const float m = v * (float)bs; return m + (float)i; }
SDN_HD int32_t idx_disambiguate_i32(int32_t v, int bs, int i) { return (int32_t)((uint32_t)v * (uint32_t)bs + (uint32_t)i); }
SDN_HD int16_t idx_disambiguate_i16(int16_t v, int bs, int i)
{
    return (int16_t)(uint16_t)((uint32_t)(uint16_t)v * (uint32_t)bs + (uint32_t)i);
}

// the bit of a disambiguated value, or -1 outside the window (NaN and Inf too): trunc(v) in [MIN, MIN + BITS)
SDN_HD int idx_bit_f32(float v)
{
    return (v > (float)(IDX_KEY_MIN - 1) && v < (float)(IDX_KEY_MIN + IDX_BITS)) ? (int)v - IDX_KEY_MIN : -1;
}
SDN_HD int idx_bit_i32(int32_t v) { return (v >= IDX_KEY_MIN && v < IDX_KEY_MIN + IDX_BITS) ? v - IDX_KEY_MIN : -1; }
SDN_HD long idx_key_of_bit(int bit) { return (long)bit + IDX_KEY_MIN; }

SDN_HD int idx_popc(uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(w);
#else
    return __builtin_popcount(w);
#endif
}
// the rank of bit b of a word among the set bits of the whole bitmap: the word's exclusive prefix + the set bits below b
SDN_HD int idx_rank(int prefix_of_word, uint32_t word, int b) { return prefix_of_word + idx_popc(word & ((1u << (b & 31)) - 1u)); }

SDN_HD long idx_id_capacity(long pixels) { return pixels < IDX_BITS ? pixels : (long)IDX_BITS; }

// ---- validators: 0 when valid, otherwise 1 with the reason in msg ------------------------------------------------------------------
inline int enc_validate_sizes(int N, int H, int W, long planes, char* msg, size_t cap)
{
    if (N < 1 || H < 1 || W < 1) SDN_FAIL("bad sizes: N %d, H %d, W %d", N, H, W);
    const long hw = (long)H * (long)W;
    if (hw > INT_MAX || hw * N > INT_MAX || hw * N * planes > INT_MAX)
        SDN_FAIL("N * channels * H * W = %d * %ld * %d * %d must stay below 2^31", N, planes, H, W);
    return 0;
}

inline int enc_validate_maps(const void* label, int label_dt, const void* inst, int inst_dt, const void* pose, int pose_dt, int N, int H,
                             int W, int label_nc, int pose_ch, const void* input_label, const void* pose_onehot, const void* bad,
                             char* msg, size_t cap)
{
    if (!label) SDN_FAIL("label is NULL");
    if (!input_label || !bad) SDN_FAIL("input_label or bad is NULL");
    if (label_dt != ENC_U8 && label_dt != ENC_I32 && label_dt != ENC_F32) SDN_FAIL("label dtype %d; uint8, int32 or float32 are supported", label_dt);
    if (inst && inst_dt != ENC_I16 && inst_dt != ENC_I32 && inst_dt != ENC_F32)
        SDN_FAIL("inst dtype %d; int16, int32 or float32 are supported", inst_dt);
    if (label_nc < 1 || label_nc > ENC_MAX_CHANNELS) SDN_FAIL("label_nc is %d; 1 to %d are supported", label_nc, ENC_MAX_CHANNELS);
    if (pose_ch < 0 || pose_ch > ENC_MAX_CHANNELS) SDN_FAIL("pose_ch is %d; 0 (none) to %d are supported", pose_ch, ENC_MAX_CHANNELS);
    if (pose_ch > 0) {
        if (!pose || !pose_onehot) SDN_FAIL("pose or pose_onehot is NULL with %d pose channels", pose_ch);
        if (pose_dt != ENC_I32 && pose_dt != ENC_F32) SDN_FAIL("pose dtype %d; int32 or float32 are supported", pose_dt);
        if (misaligned(pose, 4) || misaligned(pose_onehot, 4)) SDN_FAIL("pose and pose_onehot must be aligned to 4 bytes");
    }
    if (misaligned(label, enc_elem_bytes(label_dt))) SDN_FAIL("label is not aligned to its element size");
    if (inst && misaligned(inst, enc_elem_bytes(inst_dt))) SDN_FAIL("inst is not aligned to its element size");
    if (misaligned(input_label, 4) || misaligned(bad, 4)) SDN_FAIL("input_label and bad must be aligned to 4 bytes");
    const long planes = (long)label_nc + (inst ? 1 : 0) > (long)pose_ch ? (long)label_nc + (inst ? 1 : 0) : (long)pose_ch;
    return enc_validate_sizes(N, H, W, planes, msg, cap);
}

inline int idx_validate_common(const void* inst, int inst_dt, int N, int H, int W, const void* workspace, size_t workspace_bytes,
                               char* msg, size_t cap)
{
    if (!inst) SDN_FAIL("inst is NULL");
    if (inst_dt != ENC_I16 && inst_dt != ENC_I32 && inst_dt != ENC_F32) SDN_FAIL("inst dtype %d; int16, int32 or float32 are supported", inst_dt);
    if (misaligned(inst, enc_elem_bytes(inst_dt))) SDN_FAIL("inst is not aligned to its element size");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (misaligned(workspace, 16)) SDN_FAIL("workspace must be aligned to 16 bytes");
    if (workspace_bytes < IDX_WORKSPACE_BYTES) SDN_FAIL("workspace holds %zu bytes, %zu are needed", workspace_bytes, IDX_WORKSPACE_BYTES);
    return enc_validate_sizes(N, H, W, 1, msg, cap);
}

inline int idx_validate_build(const void* inst, int inst_dt, int N, int H, int W, const void* workspace, size_t workspace_bytes,
                              const void* ids, const void* counts, long id_capacity, char* msg, size_t cap)
{
    if (idx_validate_common(inst, inst_dt, N, H, W, workspace, workspace_bytes, msg, cap)) return 1;
    if (!ids) SDN_FAIL("ids is NULL");
    if (misaligned(ids, 8) || (counts && misaligned(counts, 8))) SDN_FAIL("ids and counts must be aligned to 8 bytes");
    const long need = idx_id_capacity((long)N * H * W);
    if (id_capacity < need) SDN_FAIL("ids holds %ld entries, %ld are needed", id_capacity, need);
    return 0;
}

inline int idx_validate_rank(const void* inst, int inst_dt, int N, int H, int W, const void* workspace, size_t workspace_bytes,
                             const void* seg, const void* counts, char* msg, size_t cap)
{
    if (idx_validate_common(inst, inst_dt, N, H, W, workspace, workspace_bytes, msg, cap)) return 1;
    if (!seg) SDN_FAIL("seg is NULL");
    if (misaligned(seg, 4)) SDN_FAIL("seg must be aligned to 4 bytes");
    if (counts && misaligned(counts, 8)) SDN_FAIL("counts must be aligned to 8 bytes");
    return 0;
}

}  // namespace sdn
