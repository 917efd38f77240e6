// Constants, the score's integer image, the workspace layout and HOST argument validation of the proposal layer (proposal_layer.hip).
// Plain C++ so that a host program can walk the image's order, the layout and the validators without the HIP runtime
// (tools/proposal_layer_check.cpp).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "check_common.h"

namespace sdn {

constexpr int PROP_MAX_PRE_NMS = 8192;       // K: one workgroup sorts the selected 64-bit keys in 64 KiB of LDS
constexpr int PROP_MAX_ANCHORS = 1 << 24;    // A must stay below: the index fills the low 24 bits of a key with room to spare
constexpr int PROP_THREADS = 256;
constexpr int PROP_CHUNK = 1024;             // anchors of one workgroup of the selection kernels: four per thread
constexpr int PROP_SORT_THREADS = 1024;
constexpr int PROP_HEAD_INTS = 4 * 256 + 8;  // four 256-bin histograms, the compaction's cursor, padding: zeroed by every call
constexpr int PROP_ALIGN = 16;               // every range of the workspace starts on 16 bytes

// Order-preserving integer image of a score: a < b as floats <=> image(a) < image(b) as unsigned, with torch's sort order at the
// ends: -0.0 and +0.0 are one value, every NaN is one value above +inf (torch.sort(descending=True) puts NaN first).
SDN_HD uint32_t prop_image(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;   // NaN, whatever its sign and payload
    if ((bits & 0x7fffffffu) == 0u) return 0x80000000u;           // both zeros
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// The 64-bit key of anchor `index`: descending keys are descending scores, equal scores lower index first.  Never 0.
SDN_HD uint64_t prop_key(uint32_t image, uint32_t index) { return ((uint64_t)image << 32) | (uint64_t)(0xffffffffu - index); }
SDN_HD uint32_t prop_key_index(uint64_t key) { return 0xffffffffu - (uint32_t)(key & 0xffffffffull); }

SDN_HD int prop_chunks(int A) { return (A + PROP_CHUNK - 1) / PROP_CHUNK; }
SDN_HD int prop_words(int K) { return (K + 63) / 64; }
SDN_HD int prop_sort_size(int K)   // the bitonic network's size: the power of two at or above K
{
    int n = 1;
    while (n < K) n <<= 1;
    return n;
}

// Step (k, j) of the bitonic network over N = 2^m keys: compare-exchange t (0 .. N/2 - 1) touches the elements i < l = i + j, and
// leaves the larger one first where `descending`.  The last merge (k = N) is descending throughout: best key first.
SDN_HD void prop_bitonic_pair(int t, int j, int k, int* i, int* l, bool* descending)
{
    *i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    *l = *i | j;
    *descending = (*i & k) == 0;
}

struct PropLayout {
    size_t head;    // int32 [PROP_HEAD_INTS]: histograms of the four radix passes, then the cursor
    size_t ties;    // int32 [chunks]: scores equal to the threshold per chunk of PROP_CHUNK anchors
    size_t keys;    // uint64 [K]: the selected keys, unsorted
    size_t areas;   // float [K]
    size_t mask;    // uint64 [K, words]
    size_t total;
};

// 0 when (A, K, P) is a valid problem; otherwise 1 with the reason in msg
inline int prop_validate_sizes(int A, int K, int P, char* msg, size_t cap)
{
    if (A < 1) SDN_FAIL("bad sizes: A %d (no anchors)", A);
    if (A >= PROP_MAX_ANCHORS) SDN_FAIL("A %d; fewer than 2^24 = %d anchors are supported", A, PROP_MAX_ANCHORS);
    if (K < 1 || K > PROP_MAX_PRE_NMS) SDN_FAIL("K %d; 1 to %d are supported (the selected keys are sorted in the LDS)", K, PROP_MAX_PRE_NMS);
    if (K > A) SDN_FAIL("K %d exceeds A %d: K = min(pre_nms_limit, A)", K, A);
    if (P < 1 || P > PROP_MAX_PRE_NMS) SDN_FAIL("P %d; 1 to %d are supported", P, PROP_MAX_PRE_NMS);
    return 0;
}

inline int prop_layout(int A, int K, int P, PropLayout* L, char* msg, size_t cap)
{
    if (prop_validate_sizes(A, K, P, msg, cap)) return 1;
    if (!L) SDN_FAIL("the layout is NULL");
    size_t at = 0;   // A < 2^24, K <= 2^13: the largest range, the mask, is 2^13 * 2^7 * 8 = 8 MiB
    L->head = at;
    at += round_up(sizeof(int32_t) * (size_t)PROP_HEAD_INTS, PROP_ALIGN);
    L->ties = at;
    at += round_up(sizeof(int32_t) * (size_t)prop_chunks(A), PROP_ALIGN);
    L->keys = at;
    at += round_up(sizeof(uint64_t) * (size_t)K, PROP_ALIGN);
    L->areas = at;
    at += round_up(sizeof(float) * (size_t)K, PROP_ALIGN);
    L->mask = at;
    at += round_up(sizeof(uint64_t) * (size_t)K * (size_t)prop_words(K), PROP_ALIGN);
    L->total = at;
    return 0;
}

inline int prop_validate(const void* rpn_probs, const void* rpn_bbox, const void* anchors, int A, const float* std_dev, int height, int width,
                         int K, int P, const void* order, const void* boxes_px, const void* keep, const void* count,
                         const void* rois, const void* workspace, size_t workspace_bytes, char* msg, size_t cap)
{
    PropLayout L;
    if (prop_layout(A, K, P, &L, msg, cap)) return 1;
    if (height < 1 || width < 1) SDN_FAIL("bad sizes: image %d x %d", height, width);
    if (!std_dev) SDN_FAIL("std_dev is NULL (four floats in host memory)");
    if (!rpn_probs || !rpn_bbox || !anchors) SDN_FAIL("rpn_probs, rpn_bbox or anchors is NULL");
    if (!order || !boxes_px || !keep || !count || !rois) SDN_FAIL("order, boxes_px, keep, count or rois is NULL");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (workspace_bytes < L.total) SDN_FAIL("workspace %zu < %zu bytes", workspace_bytes, L.total);
    if (misaligned(rpn_probs, 4) || misaligned(rpn_bbox, 4) || misaligned(anchors, 4))
        SDN_FAIL("rpn_probs, rpn_bbox and anchors must be aligned to 4 bytes");
    if (misaligned(order, 4) || misaligned(keep, 4) || misaligned(count, 4)) SDN_FAIL("order, keep and count must be aligned to 4 bytes");
    if (misaligned(boxes_px, 16) || misaligned(rois, 16) || misaligned(workspace, 16))
        SDN_FAIL("boxes_px, rois and workspace must be aligned to 16 bytes");
    return 0;
}

}  // namespace sdn
