// Sizes, buffer layouts, index arithmetic and HOST argument validation of the Mask R-CNN training losses (mrcnn_loss.hip).  Plain
// C++ so that a host program can walk the chunk arithmetic, the ordered rank of the positive anchors and the validators without
// the HIP runtime (tools/mrcnn_loss_check.cpp).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "check_common.h"

namespace sdn {

constexpr int MRL_THREADS = 64;      // a workgroup is one wave: sums and the prefix count need shuffles only, no LDS and no barrier
constexpr int MRL_QUAD = 4;          // adjacent anchors (or mask pixels) of one lane: one 16-byte load of an [A, 4] row each
constexpr int MRL_STEP = MRL_THREADS * MRL_QUAD;   // anchors a wave takes at once, in anchor order across its lanes
constexpr int MRL_STEPS = 4;
constexpr int MRL_CHUNK = MRL_STEP * MRL_STEPS;    // anchors of one workgroup (ops.py mirrors it)
constexpr int MRL_MAX_CLASSES = 128; // a RoI's logits: at most two per lane
constexpr int MRL_MAX_ANCHORS = 1 << 24;           // every chunk re-adds the counts of the chunks before it: 16384 chunks at most
constexpr int MRL_PART_BYTES = 40;   // workspace per workgroup: three doubles (RPN: class, box, unused; RoI: class, box, mask), then
                                     // four ints (RPN: valid, positives in the box loss, bad, pad; RoI: valid id, positive, bad, pad)
constexpr int MRL_SAVED_HEAD = 16;   // int32 [4] in front of `saved`: n_rpn_valid, n_rpn_pos, n_roi_valid, n_roi_pos

// what an rpn_match value means: 1 positive, -1 negative, 0 neutral, 2 anything else (counted in bad, left out)
SDN_HD int mrl_match_kind(long long v) { return v == 1 ? 1 : v == -1 ? -1 : v == 0 ? 0 : 2; }
// 1 positive RoI, 0 background, -1 an id outside [0, C) (counted in bad, left out of the three head losses)
SDN_HD int mrl_roi_kind(long long id, int C) { return id < 0 || id >= (long long)C ? -1 : id > 0 ? 1 : 0; }

SDN_HD int mrl_chunks(long A) { return (int)((A + MRL_CHUNK - 1) / MRL_CHUNK); }
// the first of the four adjacent anchors that `lane` takes in step `step` of chunk `chunk`: within a step the lanes, and within
// a chunk the steps, follow the anchor order, so (chunk, step, lane, element) in lexicographic order IS the anchor order
SDN_HD long mrl_quad_first(int chunk, int step, int lane) { return (long)chunk * MRL_CHUNK + (long)step * MRL_STEP + (long)lane * MRL_QUAD; }
// workgroups of the forward partial kernel: one per chunk of anchors, then one per RoI
SDN_HD long mrl_blocks(long A, int R) { return (long)mrl_chunks(A) + R; }

// `workspace`: the doubles of all workgroups, then their ints, then the positives of every chunk (the table of the first pass)
SDN_HD size_t mrl_sum_at(long g) { return (size_t)g * 24; }
SDN_HD size_t mrl_cnt_at(long nblk, long g) { return (size_t)nblk * 24 + (size_t)g * 16; }
SDN_HD size_t mrl_table_at(long nblk) { return (size_t)nblk * MRL_PART_BYTES; }
SDN_HD size_t mrl_workspace_bytes(long A, int R)
{
    const size_t n = mrl_table_at(mrl_blocks(A, R)) + (size_t)mrl_chunks(A) * 4;
    return (n + 7) & ~(size_t)7;
}
// `saved`, what backward needs from forward: the head, the RoIs' log-sum-exps (fp64), the positives before every chunk
SDN_HD size_t mrl_lse_at(int r) { return (size_t)MRL_SAVED_HEAD + (size_t)r * 8; }
SDN_HD size_t mrl_prefix_at(int R, int chunk) { return (size_t)MRL_SAVED_HEAD + (size_t)R * 8 + (size_t)chunk * 4; }
SDN_HD size_t mrl_saved_bytes(long A, int R)
{
    const size_t n = mrl_prefix_at(R, mrl_chunks(A));
    return (n + 15) & ~(size_t)15;
}

// 0 when the sizes of sdn_mrcnn_loss_fwd / _bwd are valid; otherwise 1 with the reason in msg
inline int mrl_validate_sizes(int batch, int A, int T, int R, int C, int h, int w, char* msg, size_t cap)
{
    if (batch != 1)
        SDN_FAIL("the RPN tensors have batch %d; only 1 is supported: target_bbox[0, :n] (model.py:1053) has no meaning for more images", batch);
    if (A < 1 || T < 1) SDN_FAIL("bad sizes: A %d, T %d", A, T);
    if (A > MRL_MAX_ANCHORS) SDN_FAIL("%d anchors; at most %d are supported", A, MRL_MAX_ANCHORS);
    if (T > INT_MAX / 4) SDN_FAIL("T * 4 = %d * 4 must stay below 2^31", T);
    if (R < 0) SDN_FAIL("bad sizes: R %d", R);
    if (R == 0) return 0;   // the head tensors are not read
    if (C < 2 || C > MRL_MAX_CLASSES) SDN_FAIL("%d classes; 2 to %d are supported", C, MRL_MAX_CLASSES);
    if (h < 1 || w < 1) SDN_FAIL("bad sizes: h %d, w %d", h, w);
    // no product overflows: every factor is below 2^31 and the running product is checked before the next factor
    const long hw = (long)h * (long)w;
    if (hw > INT_MAX || hw * C > INT_MAX || hw * C * R > INT_MAX)
        SDN_FAIL("R * C * h * w = %d * %d * %d * %d must stay below 2^31", R, C, h, w);
    return 0;
}

struct MrlInputs {
    const void* rpn_match;
    int match_i64;
    const void *rpn_bbox, *rpn_class_logits, *rpn_pred_bbox;
    const void* target_class_ids;
    int ids_i64;
    const void *mrcnn_class_logits, *target_deltas, *mrcnn_bbox, *target_mask, *mrcnn_mask;
};

inline int mrl_validate_inputs(const MrlInputs& in, int R, char* msg, size_t cap)
{
    if (!in.rpn_match) SDN_FAIL("rpn_match is NULL");
    if (!in.rpn_bbox || !in.rpn_class_logits || !in.rpn_pred_bbox) SDN_FAIL("rpn_bbox, rpn_class_logits or rpn_pred_bbox is NULL");
    if ((in.match_i64 != 0 && in.match_i64 != 1) || (in.ids_i64 != 0 && in.ids_i64 != 1)) SDN_FAIL("an integer type flag must be 0 (int32) or 1 (int64)");
    if (misaligned(in.rpn_match, in.match_i64 ? 8 : 4)) SDN_FAIL("rpn_match must be aligned to its element size");
    if (misaligned(in.rpn_bbox, 4) || misaligned(in.rpn_class_logits, 4) || misaligned(in.rpn_pred_bbox, 4))
        SDN_FAIL("the RPN float tensors must be aligned to 4 bytes");
    if (R == 0) return 0;
    if (!in.target_class_ids) SDN_FAIL("target_class_ids is NULL");
    if (!in.mrcnn_class_logits || !in.target_deltas || !in.mrcnn_bbox || !in.target_mask || !in.mrcnn_mask)
        SDN_FAIL("a head tensor is NULL with R > 0");
    if (misaligned(in.target_class_ids, in.ids_i64 ? 8 : 4)) SDN_FAIL("target_class_ids must be aligned to its element size");
    if (misaligned(in.mrcnn_class_logits, 4) || misaligned(in.target_deltas, 4) || misaligned(in.mrcnn_bbox, 4) ||
        misaligned(in.target_mask, 4) || misaligned(in.mrcnn_mask, 4))
        SDN_FAIL("the head float tensors must be aligned to 4 bytes");
    return 0;
}

// the forward call
inline int mrl_validate_fwd(const MrlInputs& in, int batch, int A, int T, int R, int C, int h, int w, const void* workspace,
                            size_t workspace_bytes, const void* saved, size_t saved_bytes, const void* out, const void* counts, char* msg,
                            size_t cap)
{
    if (mrl_validate_sizes(batch, A, T, R, C, h, w, msg, cap)) return 1;
    if (mrl_validate_inputs(in, R, msg, cap)) return 1;
    if (!workspace || !saved || !out || !counts) SDN_FAIL("workspace, saved, out or counts is NULL");
    if (misaligned(workspace, 8) || misaligned(saved, 8) || misaligned(counts, 8) || misaligned(out, 4))
        SDN_FAIL("workspace, saved and counts must be aligned to 8 bytes, out to 4");
    const size_t need = mrl_workspace_bytes(A, R);
    if (workspace_bytes < need) SDN_FAIL("workspace of %zu bytes; %zu are needed (sdn_mrcnn_loss_workspace_bytes)", workspace_bytes, need);
    const size_t keep = mrl_saved_bytes(A, R);
    if (saved_bytes < keep) SDN_FAIL("saved of %zu bytes; %zu are needed (sdn_mrcnn_loss_workspace_bytes)", saved_bytes, keep);
    return 0;
}

// the backward call; g: the five gradients in the order of the inputs they belong to
inline int mrl_validate_bwd(const MrlInputs& in, int batch, int A, int T, int R, int C, int h, int w, const void* saved, size_t saved_bytes,
                            const void* grad_out, const void* const (&g)[5], char* msg, size_t cap)
{
    if (mrl_validate_sizes(batch, A, T, R, C, h, w, msg, cap)) return 1;
    if (mrl_validate_inputs(in, R, msg, cap)) return 1;
    if (!saved || !grad_out) SDN_FAIL("saved or grad_out is NULL");
    if (misaligned(saved, 8) || misaligned(grad_out, 4)) SDN_FAIL("saved must be aligned to 8 bytes, grad_out to 4");
    const size_t keep = mrl_saved_bytes(A, R);
    if (saved_bytes < keep) SDN_FAIL("saved of %zu bytes; %zu are needed (sdn_mrcnn_loss_workspace_bytes)", saved_bytes, keep);
    if (!g[0] && !g[1] && !g[2] && !g[3] && !g[4]) SDN_FAIL("no gradient asked for");
    if (R == 0 && (g[2] || g[3] || g[4])) SDN_FAIL("a head gradient with R = 0");
    for (int i = 0; i < 5; i++)
        if (misaligned(g[i], 4)) SDN_FAIL("the gradients must be aligned to 4 bytes");
    return 0;
}

}  // namespace sdn
