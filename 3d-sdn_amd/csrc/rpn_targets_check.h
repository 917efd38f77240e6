// Constants, the key images, the caps, the workspace layout and HOST argument validation of the RPN targets (rpn_targets.hip).  Plain
// C++ so that a host program can walk them without the HIP runtime (tools/rpn_targets_check.cpp).  The float image and
// the box cap are the detection targets', the workspace's alignment is the proposal layer's.
#pragma once

#include <cstring>

#include "detection_targets_check.h"

namespace sdn {

constexpr int RT_MAX_ANCHORS = (1 << 24) - 1;   // A: an anchor fills 24 bits
constexpr int RT_MAX_BOXES = DT_MAX_BOXES;      // G: the boxes lie in the LDS; the matched box is one byte per anchor
constexpr int RT_MAX_TARGETS = 8192;            // T: RPN_TRAIN_ANCHORS_PER_IMAGE
constexpr int RT_THREADS = 256;                 // the other kernels' workgroup: four waves
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_PER_LANE = 4;                  // anchors of one of their lanes
constexpr int RT_CHUNK = RT_THREADS * RT_PER_LANE;   // anchors of one workgroup
constexpr int RT_MATCH_THREADS = RT_CHUNK;     // the matching kernel's workgroup: one anchor per lane, sixteen waves to hide the fp64 division
constexpr int RT_MATCH_WAVES = RT_MATCH_THREADS / 64;
constexpr int RT_PASSES = 4;                    // 256-bin radix passes over the 32-bit key image
constexpr int RT_BINS = 256;
constexpr int RT_HIST_INTS = RT_PASSES * 2 * RT_BINS;   // [pass][class][bin]

// the classes of the two selects: the positives are sampled by row 0 of the keys, the negatives by row 1
constexpr int RT_POS = 0, RT_NEG = 1;

SDN_HD int rt_chunks(int A) { return (A + RT_CHUNK - 1) / RT_CHUNK; }

// The order-preserving image of a DOUBLE for np.argmax: a < b <=> image(a) < image(b); -0.0 is +0.0 (argmax compares with >, to
// which they are equal); every NaN is the one largest image, because to argmax the FIRST NaN is the maximum whatever its bits.  No
// double has the image 0: that is "no anchor yet".
constexpr uint64_t RT_IMAGE_NAN = ~0ull;
constexpr uint64_t RT_IMAGE_ZERO = 0x8000000000000000ull;   // the image of 0.0
SDN_HD uint64_t rt_image(double v)
{
    if (v != v) return RT_IMAGE_NAN;
    if (v == 0.0) return RT_IMAGE_ZERO;
    uint64_t bits;
    memcpy(&bits, &v, sizeof(bits));
    return (bits >> 63) ? ~bits : (bits | RT_IMAGE_ZERO);
}
SDN_HD double rt_image_value(uint64_t image)   // the inverse, for every image but the NaN's
{
    const uint64_t bits = (image >> 63) ? (image & ~RT_IMAGE_ZERO) : ~image;
    double v;
    memcpy(&v, &bits, sizeof(v));
    return v;
}

// np.argmax over a row or a column: the first maximum, the first NaN being a maximum.  `have` is false before the first element.
SDN_HD bool rt_argmax_takes(bool have, double best, double v) { return !have || (best == best && (v > best || v != v)); }

// model.py:1276 and :1283-1284: the positives kept, then the negatives kept
SDN_HD int rt_positive_cap(int T) { return T / 2; }
SDN_HD int rt_positives_kept(int T, int n_pos) { return n_pos < rt_positive_cap(T) ? n_pos : rt_positive_cap(T); }
SDN_HD int rt_negative_cap(int T, int n_pos_kept) { return T - n_pos_kept; }
SDN_HD int rt_negatives_kept(int T, int n_pos_kept, int n_neg) { return n_neg < rt_negative_cap(T, n_pos_kept) ? n_neg : rt_negative_cap(T, n_pos_kept); }

// A sampling key and its anchor as one number: the anchors kept are those with the `cap` smallest.  The image is dt_image.
SDN_HD uint64_t rt_sample_key(uint32_t key_bits, uint32_t anchor) { return ((uint64_t)dt_image(key_bits) << 24) | (uint64_t)anchor; }
SDN_HD uint32_t rt_sample_key_image(uint64_t key) { return (uint32_t)(key >> 24); }
SDN_HD uint32_t rt_sample_key_anchor(uint64_t key) { return (uint32_t)(key & 0xffffffu); }
// the digit of radix pass p (0: the highest byte) and the digits before it
SDN_HD uint32_t rt_digit(uint32_t image, int p) { return (image >> (24 - 8 * p)) & 255u; }
SDN_HD uint32_t rt_prefix(uint32_t image, int p) { return p == 0 ? 0u : image >> (32 - 8 * p); }

struct RtLayout {
    size_t hist;       // int32 [RT_PASSES][2][RT_BINS]: the histograms of the radix passes, zeroed by the second launch
    size_t best;       // int32 [G]: every kept box's best anchor (gt_iou_argmax), -1 for a box that is dropped
    size_t counts;     // int32 [3][chunks]: per chunk the positives below the cut key, the positives at it, the negatives at it
    size_t tab_image;  // uint64 [chunks][G]: per chunk and box the largest IoU image ...
    size_t tab_anchor; // int32 [chunks][G]: ... and the lowest anchor that has it
    size_t argmax;     // uint8 [A]: anchor_iou_argmax
    size_t total;
};

// 0 when the sizes are a valid problem; otherwise 1 with the reason in msg
inline int rt_validate_sizes(int A, int G, int T, char* msg, size_t cap)
{
    if (A < 1 || A > RT_MAX_ANCHORS) SDN_FAIL("A %d; 1 to %d anchors are supported (an anchor fills 24 bits)", A, RT_MAX_ANCHORS);
    if (G < 1 || G > RT_MAX_BOXES) SDN_FAIL("G %d; 1 to %d boxes are supported", G, RT_MAX_BOXES);
    if (T < 2 || T > RT_MAX_TARGETS) SDN_FAIL("T %d; 2 to %d anchors per image are supported", T, RT_MAX_TARGETS);
    return 0;
}

inline int rt_layout(int A, int G, int T, RtLayout* L, char* msg, size_t cap)
{
    if (rt_validate_sizes(A, G, T, msg, cap)) return 1;
    if (!L) SDN_FAIL("the layout is NULL");
    const size_t chunks = (size_t)rt_chunks(A);
    size_t at = 0;
    L->hist = at;
    at += round_up(sizeof(int32_t) * (size_t)RT_HIST_INTS, PROP_ALIGN);
    L->best = at;
    at += round_up(sizeof(int32_t) * (size_t)G, PROP_ALIGN);
    L->counts = at;
    at += round_up(sizeof(int32_t) * 3 * chunks, PROP_ALIGN);
    L->tab_image = at;
    at += round_up(sizeof(uint64_t) * chunks * (size_t)G, PROP_ALIGN);
    L->tab_anchor = at;
    at += round_up(sizeof(int32_t) * chunks * (size_t)G, PROP_ALIGN);
    L->argmax = at;
    at += round_up((size_t)A, PROP_ALIGN);
    L->total = at;
    return 0;
}

inline int rt_validate(const void* anchors, const void* gt_class_ids, const void* gt_boxes, const void* keys, int A, int G, int ids_int64,
                       const void* gt_count, int T, const double* std_dev, const void* rpn_match, const void* rpn_bbox,
                       const void* rows, const void* counts, const void* workspace, size_t workspace_bytes, char* msg, size_t cap)
{
    RtLayout L;
    if (rt_layout(A, G, T, &L, msg, cap)) return 1;
    if (!std_dev) SDN_FAIL("std_dev is NULL (four doubles in host memory)");
    for (int k = 0; k < 4; k++)
        if (!(std_dev[k] > 0.0)) SDN_FAIL("std_dev[%d] is %g; it must be positive", k, std_dev[k]);
    if (!anchors || !gt_class_ids || !gt_boxes || !keys) SDN_FAIL("anchors, gt_class_ids, gt_boxes or keys is NULL");
    if (!rpn_match || !rpn_bbox || !rows || !counts) SDN_FAIL("rpn_match, rpn_bbox, rows or counts is NULL");
    if (!workspace) SDN_FAIL("workspace is NULL");
    if (workspace_bytes < L.total) SDN_FAIL("workspace %zu < %zu bytes", workspace_bytes, L.total);
    if (misaligned(anchors, 16)) SDN_FAIL("anchors must be aligned to 16 bytes");
    if (misaligned(gt_boxes, 4) || misaligned(keys, 4)) SDN_FAIL("gt_boxes and keys must be aligned to 4 bytes");
    if (misaligned(gt_class_ids, ids_int64 ? 8 : 4)) SDN_FAIL("gt_class_ids must be aligned to %d bytes", ids_int64 ? 8 : 4);
    if (gt_count && misaligned(gt_count, 4)) SDN_FAIL("gt_count must be aligned to 4 bytes");
    if (misaligned(rpn_match, 4) || misaligned(rows, 4) || misaligned(counts, 4))
        SDN_FAIL("rpn_match, rows and counts must be aligned to 4 bytes");
    if (misaligned(rpn_bbox, 16) || misaligned(workspace, 16)) SDN_FAIL("rpn_bbox and workspace must be aligned to 16 bytes");
    return 0;
}

}  // namespace sdn
