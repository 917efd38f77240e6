// Constants, the workspace layout and HOST argument validation of the detection layer (detection_layer.hip).  Plain C++ so that a host
// program can walk the layout and the validators without the HIP runtime (tools/detection_layer_check.cpp).  The score's integer
// image, the keys, the sorting network and the workspace's alignment are the proposal layer's (proposal_layer_check.h).
#pragma once

#include "proposal_layer_check.h"

namespace sdn {

constexpr int DET_MAX_ROIS = PROP_MAX_PRE_NMS;         // N: one workgroup sorts the rows' 64-bit keys in 64 KiB of LDS
constexpr int DET_MAX_INSTANCES = PROP_MAX_PRE_NMS;    // D: the scan's list of kept rows lies in the LDS
constexpr int DET_MAX_WORDS = DET_MAX_ROIS / 64;
constexpr int DET_ROW_THREADS = 64;                    // the row kernel's workgroup: one wave
constexpr int DET_ROW_LANES = 8;                       // lanes that share a row's arg-max: a power of two that divides 64
constexpr int DET_ROWS_PER_WAVE = DET_ROW_THREADS / DET_ROW_LANES;
constexpr int DET_SORT_THREADS = PROP_SORT_THREADS;
constexpr int DET_HEAD_INTS = 4;                       // the valid count M, padding

// The arg-max of a row as torch.max(dim=1) gives it on the CPU: the first index of the maximum, a NaN counting as the maximum and the
// first NaN winning.  True when the candidate (v, c) replaces (score, cls): a NaN before a number, the lower index of two NaNs, the
// greater of two numbers, the lower index of two equal ones.  A walk in index order that starts from (-inf, INT_MAX) and the merge of
// the candidates of several such walks over disjoint classes both use it, and both give the walk over all classes.
SDN_HD bool det_argmax_takes(float score, int cls, float v, int c)
{
    const bool mine_nan = score != score, other_nan = v != v;
    return other_nan ? (!mine_nan || c < cls) : (!mine_nan && (v > score || (v == score && c < cls)));
}

struct DetLayout {
    size_t head;      // int32 [DET_HEAD_INTS]: M, the rows that enter the NMS, written by the sorting workgroup
    size_t keys;      // uint64 [N]: one key per row, 0 for a row that is no detection
    size_t boxes;     // float4 [N]: the first M in score order
    size_t areas;     // float [N]
    size_t classes;   // int32 [N]
    size_t rows;      // int32 [N]: the row of every place of the score order
    size_t mask;      // uint64 [N, words]
    size_t total;
};

// 0 when (N, C, D) is a valid problem; otherwise 1 with the reason in msg
inline int det_validate_sizes(int N, int C, int D, char* msg, size_t cap)
{
    if (N < 1 || N > DET_MAX_ROIS) SDN_FAIL("N %d; 1 to %d rois are supported (their keys are sorted in the LDS)", N, DET_MAX_ROIS);
    if (C < 1) SDN_FAIL("bad sizes: C %d (no classes)", C);
    if (D < 1 || D > DET_MAX_INSTANCES) SDN_FAIL("D %d; 1 to %d detections are supported", D, DET_MAX_INSTANCES);
    return 0;
}

inline int det_layout(int N, int C, int D, DetLayout* L, char* msg, size_t cap)
{
    if (det_validate_sizes(N, C, D, msg, cap)) return 1;
    if (!L) SDN_FAIL("the layout is NULL");
    size_t at = 0;   // N <= 2^13: the largest range, the mask, is 2^13 * 2^7 * 8 = 8 MiB
    L->head = at;
    at += round_up(sizeof(int32_t) * (size_t)DET_HEAD_INTS, PROP_ALIGN);
    L->keys = at;
    at += round_up(sizeof(uint64_t) * (size_t)N, PROP_ALIGN);
    L->boxes = at;
    at += round_up(4 * sizeof(float) * (size_t)N, PROP_ALIGN);
    L->areas = at;
    at += round_up(sizeof(float) * (size_t)N, PROP_ALIGN);
    L->classes = at;
    at += round_up(sizeof(int32_t) * (size_t)N, PROP_ALIGN);
    L->rows = at;
    at += round_up(sizeof(int32_t) * (size_t)N, PROP_ALIGN);
    L->mask = at;
    at += round_up(sizeof(uint64_t) * (size_t)N * (size_t)prop_words(N), PROP_ALIGN);
    L->total = at;
    return 0;
}

inline int det_validate(const void* rois, const void* probs, const void* deltas, int N, int C, const float* window, const float* std_dev,
                        int height, int width, int D, const void* roi_count, const void* class_ids, const void* scores, const void* boxes_px,
                        const void* keep, const void* count, const void* detections, const void* boxes_norm, const void* workspace,
                        size_t workspace_bytes, char* msg, size_t cap)
{
    DetLayout L;
    if (det_layout(N, C, D, &L, msg, cap)) return 1;
    if (height < 1 || width < 1) SDN_FAIL("bad sizes: image %d x %d", height, width);
    if (!window) SDN_FAIL("window is NULL (four floats in host memory)");
    if (!std_dev) SDN_FAIL("std_dev is NULL (four floats in host memory)");
    if (!rois || !probs || !deltas) SDN_FAIL("rois, probs or deltas is NULL");
    if (!class_ids || !scores || !boxes_px) SDN_FAIL("class_ids, scores or boxes_px is NULL");
    if (!keep || !count || !detections || !boxes_norm) SDN_FAIL("keep, count, detections or boxes_norm is NULL");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (workspace_bytes < L.total) SDN_FAIL("workspace %zu < %zu bytes", workspace_bytes, L.total);
    if (misaligned(rois, 4) || misaligned(probs, 4) || misaligned(deltas, 4))
        SDN_FAIL("rois, probs and deltas must be aligned to 4 bytes");
    if (roi_count && misaligned(roi_count, 4)) SDN_FAIL("roi_count must be aligned to 4 bytes");
    if (misaligned(class_ids, 4) || misaligned(scores, 4) || misaligned(keep, 4) || misaligned(count, 4) ||
        misaligned(detections, 4))
        SDN_FAIL("class_ids, scores, keep, count and detections must be aligned to 4 bytes");
    if (misaligned(boxes_px, 16) || misaligned(boxes_norm, 16) || misaligned(workspace, 16))
        SDN_FAIL("boxes_px, boxes_norm and workspace must be aligned to 16 bytes");
    return 0;
}

}  // namespace sdn
