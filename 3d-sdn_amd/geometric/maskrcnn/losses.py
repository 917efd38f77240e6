"""The losses of a Mask R-CNN training step on the device: compute_losses and the five functions it calls (reference:
geometric/maskrcnn/model.py:1004-1147) and their sum in MaskRCNN.train_epoch / valid_epoch (:1955, 2027).

    from maskrcnn.losses import compute_losses        # instead of the one in maskrcnn.model
    losses = compute_losses(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits,
                            target_deltas, mrcnn_bbox, target_mask, mrcnn_mask)
    sum(losses).backward()

or `mrcnn_losses(...)['loss'].backward()` with the sum taken on the device.  The reference finds the contributing anchors and RoIs
with four torch.nonzero calls, each of which waits for the device, and gathers through index tensors; here nothing crosses to the
host.  The kernels are csrc/mrcnn_loss.hip behind sdn_hip.ops.mrcnn_loss; CPU tensors raise NotImplementedError and there is no
torch form.  detection_target_layer, the step that makes the head targets, is maskrcnn.detection_targets; its padded form marks the
rows behind its count with class id -1, which the head losses here leave out.  build_rpn_targets, the step that makes rpn_match and
rpn_bbox, is maskrcnn.rpn_targets; its rpn_targets_padded returns them in the shapes taken here, so no argument comes from the host any
more.  The network and the inputs of build_rpn_targets stay the caller's.
"""
import torch

from sdn_hip import ops

LOSS_KEYS = ('rpn_class_loss', 'rpn_bbox_loss', 'mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss', 'loss')
COUNT_KEYS = ('n_rpn_valid', 'n_rpn_pos', 'n_roi_pos', 'bad')


def _contiguous(t):
    # an autograd op: the gradient flows back through the strides
    return t.contiguous() if isinstance(t, torch.Tensor) and t.is_cuda else t


def mrcnn_losses(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas, mrcnn_bbox,
                 target_mask, mrcnn_mask):
    """The arguments of the reference's compute_losses, CUDA tensors: rpn_match int32 / int64 [1, A, 1] (1 positive, -1 negative,
    0 neutral), rpn_bbox fp32 [1, T, 4], rpn_class_logits fp32 [1, A, 2], rpn_pred_bbox fp32 [1, A, 4], target_class_ids int32 /
    int64 [R], mrcnn_class_logits fp32 [R, C], target_deltas fp32 [R, 4], mrcnn_bbox fp32 [R, C, 4], target_mask fp32 [R, h, w],
    mrcnn_mask fp32 [R, C, h, w] (probabilities); 2 <= C <= 128.  Returns a dict of 0-dim tensors:
        rpn_class_loss    mean over the anchors with match != 0 of the cross entropy against [match == 1] (model.py:1004-1029)
        rpn_bbox_loss     smooth L1 of the k-th positive anchor, in anchor order, against target row k (:1032-1058)
        mrcnn_class_loss  mean cross entropy over the RoIs (:1061-1077)
        mrcnn_bbox_loss   smooth L1 of the positive RoIs' own class deltas (:1080-1106)
        mrcnn_mask_loss   binary cross entropy of the positive RoIs' own class plane (:1109-1136)
        loss              their sum (:1955), taken in fp64 on the device and rounded once
        n_rpn_valid, n_rpn_pos, n_roi_pos, bad   int64: the anchors with match 1 or -1, the positive anchors in the box loss, the
                          RoIs with a class id > 0, and what was left out (below)
    The six fp32 values are views of one [6] tensor, the four integers of one [4] tensor; nothing is copied to the host.  The mean
    over an empty selection is NaN, as torch's mean of nothing.  The five predictions get gradients, the targets none.

    The RPN tensors must have batch 1: the reference's loop feeds one image per step and its target_bbox[0, :n] (:1053) has no
    meaning for more; another batch raises ValueError.

    R = 0 -- an empty target_class_ids, as predict(..., mode='training') returns it with empty head tensors when no RoI was
    sampled (:1803-1812) -- gives 0 for the three head losses, with no gradient, and the head tensors are not read.  That is the
    reference's intent under its own torch, where an empty tensor's .size() is falsy (:1070, 1088, 1118); under a current torch
    the same lines take the other branch and give NaN.

    Deviations, only where the reference has no defined answer (it raises or trips a device assert): an rpn_match value outside
    {-1, 0, 1}, a positive anchor with T or more positives before it (it stays in the class loss) and a target_class_ids value
    outside [0, C) (the RoI leaves all three head losses and their divisors) are each left out and counted in `bad`.  A mask
    probability outside [0, 1] makes mrcnn_mask_loss NaN."""
    args = [rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas, mrcnn_bbox,
            target_mask, mrcnn_mask]
    out, counts = ops.mrcnn_loss(*[_contiguous(t) for t in args])
    res = {k: out[i] for i, k in enumerate(LOSS_KEYS)}
    res.update({k: counts[i] for i, k in enumerate(COUNT_KEYS)})
    return res


def compute_losses(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas, mrcnn_bbox,
                   target_mask, mrcnn_mask):
    """The reference's compute_losses (model.py:1139-1147), name, signature and return value: the list [rpn_class_loss,
    rpn_bbox_loss, mrcnn_class_loss, mrcnn_bbox_loss, mrcnn_mask_loss] of 0-dim fp32 CUDA tensors.  A caller changes one import;
    the sum of :1955 and .backward() work as before.  See mrcnn_losses for the arguments and the two places it departs from the
    reference."""
    res = mrcnn_losses(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas,
                       mrcnn_bbox, target_mask, mrcnn_mask)
    return [res[k] for k in LOSS_KEYS[:5]]
