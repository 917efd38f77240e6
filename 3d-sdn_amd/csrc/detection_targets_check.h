// Constants, the sort key, the negative count, the workspace layout and HOST argument validation of the detection targets
// (detection_targets.hip).  Plain C++ so that a host program can walk them without the HIP runtime (tools/detection_targets_check.cpp).
// The sorting network, the arg-max rule and the workspace's alignment are the proposal and the detection layer's.
#pragma once

#include "detection_layer_check.h"

namespace sdn {

constexpr int DT_MAX_ROIS = PROP_MAX_PRE_NMS;      // N: one workgroup sorts the rows' 64-bit keys in 64 KiB of LDS
constexpr int DT_MAX_TARGETS = PROP_MAX_PRE_NMS;   // R: TRAIN_ROIS_PER_IMAGE
constexpr int DT_MAX_BOXES = 128;                  // G: boxes, ids and kinds lie in the LDS; the matched box fills 7 bits of a key
constexpr int DT_MAX_MASK_SIDE = 64;               // MASK_SHAPE: the per-row sample table has H + W entries
constexpr int DT_THREADS = PROP_SORT_THREADS;      // the sampling kernel's one workgroup
constexpr int DT_MASK_THREADS = 256;               // the mask kernel's workgroup: one output row each

// A row's class in its key.  Keys sort best first: the positives, then the negatives, then the rows that are neither (key 0).
constexpr uint64_t DT_NEITHER = 0, DT_NEGATIVE = 1, DT_POSITIVE = 2;

// The usual order-preserving image of a float's bits: a < b as floats <=> image(a) < image(b) as unsigned (-0.0 below +0.0, NaNs at
// the ends by their bits).
SDN_HD uint32_t dt_image(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }

// The 64-bit key of a row: class, then the INVERTED image of its sampling key (descending keys are ascending sampling keys), then the
// inverted row (lower row first), then the matched box, which no comparison ever reaches because rows are unique.
SDN_HD uint64_t dt_key(uint64_t cls, uint32_t key_bits, uint32_t row, uint32_t assign)
{
    return (cls << 52) | ((uint64_t)(0xffffffffu - dt_image(key_bits)) << 20) | ((uint64_t)(8191u - row) << 7) | (uint64_t)assign;
}
SDN_HD uint64_t dt_key_class(uint64_t key) { return key >> 52; }
SDN_HD uint32_t dt_key_row(uint64_t key) { return 8191u - (uint32_t)((key >> 7) & 8191u); }
SDN_HD uint32_t dt_key_assign(uint64_t key) { return (uint32_t)(key & 127u); }

// model.py:611-612: int(TRAIN_ROIS_PER_IMAGE * ROI_POSITIVE_RATIO), Python's double product truncated
SDN_HD int dt_positive_cap(int R, double ratio) { return (int)((double)R * ratio); }

// model.py:669-670: r = 1.0 / ratio; int(r * P - P) as Python computes it: fp64, a multiplication, THEN a subtraction -- a fused
// multiply-add or fp32 lands one off for some P (the files that include this are built without contraction).
SDN_HD int dt_negative_count(double ratio, int P)
{
    const double r = 1.0 / ratio;
    const double product = r * (double)P;
    return (int)(product - (double)P);
}

// the rows taken: P positives of n_pos candidates, then the negatives, never more than R in all
SDN_HD int dt_positives_taken(int cap, int n_pos) { return n_pos < cap ? n_pos : cap; }
SDN_HD int dt_negatives_taken(double ratio, int R, int P, int n_neg)
{
    if (P <= 0) return 0;   // :667: no negatives without a positive
    int n = dt_negative_count(ratio, P);
    if (n > R - P) n = R - P;
    if (n > n_neg) n = n_neg;
    return n < 0 ? 0 : n;
}

struct DtLayout {
    size_t crop;    // float4 [R]: the box each positive's mask is cropped with, in the frame of the mask
    size_t total;
};

// 0 when the sizes are a valid problem; otherwise 1 with the reason in msg
inline int dt_validate_sizes(int N, int G, int mask_h, int mask_w, int R, int H, int W, double ratio, char* msg, size_t cap)
{
    if (N < 1 || N > DT_MAX_ROIS) SDN_FAIL("N %d; 1 to %d proposals are supported (their keys are sorted in the LDS)", N, DT_MAX_ROIS);
    if (G < 1 || G > DT_MAX_BOXES) SDN_FAIL("G %d; 1 to %d boxes are supported", G, DT_MAX_BOXES);
    if (mask_h < 1 || mask_w < 1 || (long long)mask_h * mask_w > (1ll << 24)) SDN_FAIL("bad sizes: masks %d x %d", mask_h, mask_w);
    if (R < 1 || R > DT_MAX_TARGETS) SDN_FAIL("R %d; 1 to %d rois per image are supported", R, DT_MAX_TARGETS);
    if (H < 1 || H > DT_MAX_MASK_SIDE || W < 1 || W > DT_MAX_MASK_SIDE)
        SDN_FAIL("mask shape %d x %d; each side 1 to %d is supported", H, W, DT_MAX_MASK_SIDE);
    if (!(ratio > 0.0 && ratio <= 1.0)) SDN_FAIL("positive ratio %g; it must lie in (0, 1]", ratio);
    return 0;
}

inline int dt_layout(int N, int G, int mask_h, int mask_w, int R, int H, int W, DtLayout* L, char* msg, size_t cap)
{
    if (dt_validate_sizes(N, G, mask_h, mask_w, R, H, W, 0.5, msg, cap)) return 1;
    if (!L) SDN_FAIL("the layout is NULL");
    L->crop = 0;
    L->total = round_up(4 * sizeof(float) * (size_t)R, PROP_ALIGN);
    return 0;
}

inline int dt_validate(const void* proposals, const void* gt_class_ids, const void* gt_boxes, const void* gt_masks, const void* keys, int N,
                       int G, int mask_h, int mask_w, int ids_int64, const void* roi_count, int R, double ratio, const float* std_dev, int H,
                       int W, const void* rois, const void* target_class_ids, const void* target_deltas, const void* target_mask,
                       const void* rows, const void* assign, const void* count, const void* n_pos, const void* workspace,
                       size_t workspace_bytes, char* msg, size_t cap)
{
    DtLayout L;
    if (dt_validate_sizes(N, G, mask_h, mask_w, R, H, W, ratio, msg, cap)) return 1;
    if (dt_layout(N, G, mask_h, mask_w, R, H, W, &L, msg, cap)) return 1;
    if (!std_dev) SDN_FAIL("std_dev is NULL (four floats in host memory)");
    for (int k = 0; k < 4; k++)
        if (!(std_dev[k] > 0.0f)) SDN_FAIL("std_dev[%d] is %g; it must be positive", k, (double)std_dev[k]);
    if (!proposals || !gt_class_ids || !gt_boxes || !gt_masks || !keys) SDN_FAIL("proposals, gt_class_ids, gt_boxes, gt_masks or keys is NULL");
    if (!rois || !target_class_ids || !target_deltas || !target_mask) SDN_FAIL("rois, target_class_ids, target_deltas or target_mask is NULL");
    if (!rows || !assign || !count || !n_pos) SDN_FAIL("rows, assign, count or n_pos is NULL");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (workspace_bytes < L.total) SDN_FAIL("workspace %zu < %zu bytes", workspace_bytes, L.total);
    if (misaligned(proposals, 4) || misaligned(gt_boxes, 4) || misaligned(gt_masks, 4) || misaligned(keys, 4))
        SDN_FAIL("proposals, gt_boxes, gt_masks and keys must be aligned to 4 bytes");
    if (misaligned(gt_class_ids, ids_int64 ? 8 : 4)) SDN_FAIL("gt_class_ids must be aligned to %d bytes", ids_int64 ? 8 : 4);
    if (roi_count && misaligned(roi_count, 4)) SDN_FAIL("roi_count must be aligned to 4 bytes");
    if (misaligned(target_class_ids, 4) || misaligned(target_mask, 4) || misaligned(rows, 4) || misaligned(assign, 4) ||
        misaligned(count, 4) || misaligned(n_pos, 4))
        SDN_FAIL("target_class_ids, target_mask, rows, assign, count and n_pos must be aligned to 4 bytes");
    if (misaligned(rois, 16) || misaligned(target_deltas, 16) || misaligned(workspace, 16))
        SDN_FAIL("rois, target_deltas and workspace must be aligned to 16 bytes");
    return 0;
}

}  // namespace sdn
