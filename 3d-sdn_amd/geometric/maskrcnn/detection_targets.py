"""The detection targets on the device: detection_target_layer (reference: geometric/maskrcnn/model.py:545-724, with bbox_overlaps of
:508-542 and utils.box_refinement of utils.py:92-113), the step between the proposal layer and the two heads of
MaskRCNN.predict(mode='training') (:1800), once per image.

    from maskrcnn.detection_targets import detection_target_layer        # instead of the one in maskrcnn.model
    rois, target_class_ids, target_deltas, target_mask = detection_target_layer(rpn_rois, gt_class_ids, gt_boxes, gt_masks, config)

The reference builds an N x G IoU matrix from repeated copies, waits for the device in three or four .any() and three nonzero calls,
shuffles twice with a host randperm, gathers a dozen times, refines the boxes in about fifteen element-wise launches, crops the masks
and concatenates up to four times.  Here one workgroup classes every proposal, sorts the candidates by their sampling keys and writes
the sampled rows with their targets, and one kernel crops the masks: csrc/detection_targets.hip behind sdn_hip.ops.detection_targets,
two launches.  CPU tensors raise NotImplementedError and there is no torch form.

The randomness comes in as data: keys fp32 [2, N], row 0 for the positives and row 1 for the negatives.  The rows taken are the
candidates with the smallest keys, in key order (equal keys: lower row first) -- for uniform keys that is randperm(n)[:k] in
distribution, and exactly so when randperm is the stable argsort of the keys at the candidate rows.  With keys=None they are drawn with
torch.rand on the device, which is no host wait.

detection_targets_padded keeps every result in buffers of the fixed size TRAIN_ROIS_PER_IMAGE with the count beside them and nothing
crosses to the host: rows behind the count carry class id -1, which losses.mrcnn_losses leaves out of all three head losses, so the
padded proposals, the padded targets and the losses join into one training step without a host wait.  The arithmetic is the
reference's fp32, operation by operation; logf is the only operation whose last bit may differ from a CPU run.  No result carries a
gradient.
"""
import torch

from sdn_hip import ops


def _config_values(config):
    if config is None:
        raise ValueError('config is needed: TRAIN_ROIS_PER_IMAGE, ROI_POSITIVE_RATIO, BBOX_STD_DEV, USE_MINI_MASK and MASK_SHAPE are '
                         'read from it (model.py:611-654)')
    return (config.TRAIN_ROIS_PER_IMAGE, config.ROI_POSITIVE_RATIO, config.BBOX_STD_DEV, config.USE_MINI_MASK, config.MASK_SHAPE)


def _one_image(t, name, dims):
    """the reference's squeeze(0) (:571-574): a leading batch axis of 1 is dropped, a view"""
    if hasattr(t, 'dim') and t.dim() == dims + 1:
        if t.shape[0] != 1:
            raise ValueError('%s has batch %d; only 1 is supported, as in the reference ("Currently only supports batchsize 1", '
                             'geometric/maskrcnn/model.py:570)' % (name, t.shape[0]))
        return t[0]
    return t


def detection_targets_padded(proposals, gt_class_ids, gt_boxes, gt_masks, config, keys=None, roi_count=None):
    """(rois fp32 [1, R, 4], target_class_ids int32 [R], target_deltas fp32 [R, 4], target_mask fp32 [R, H, W], count int32 [1], n_pos
    int32 [1]) with R = config.TRAIN_ROIS_PER_IMAGE and (H, W) = config.MASK_SHAPE: the targets of detection_target_layer below in
    buffers of fixed size, with nothing crossing to the host -- the form for a caller that keeps the step on the device.  Positives
    first, then negatives; behind count rois, target_deltas and target_mask are +0.0 and target_class_ids is -1, the id that
    losses.mrcnn_losses leaves out.  proposals fp32 [N, 4] or [1, N, 4] normalised; gt_class_ids int32 or int64 [G] or [1, G];
    gt_boxes fp32 [G, 4] or [1, G, 4] normalised (the caller divides by (h, w, h, w), :1794); gt_masks fp32 [G, mh, mw] or [1, G, mh,
    mw].  keys: fp32 [2, N] on the device, or None to draw torch.rand(2, N) there.  roi_count: the count of proposals_padded (int32
    [1] on the device), so that its zero padding is never sampled, or None for all N rows."""
    proposals = _one_image(proposals, 'proposals', 2)
    gt_class_ids = _one_image(gt_class_ids, 'gt_class_ids', 1)
    gt_boxes = _one_image(gt_boxes, 'gt_boxes', 2)
    gt_masks = _one_image(gt_masks, 'gt_masks', 3)
    rois_per_image, ratio, std_dev, mini_mask, mask_shape = _config_values(config)
    if keys is None and isinstance(proposals, torch.Tensor) and proposals.is_cuda and proposals.dim() == 2:
        keys = torch.rand(2, proposals.shape[0], dtype=torch.float32, device=proposals.device)
    out = ops.detection_targets(proposals, gt_class_ids, gt_boxes, gt_masks, keys, rois_per_image, ratio, std_dev, mask_shape,
                                use_mini_mask=mini_mask, roi_count=roi_count)
    rois, target_class_ids, target_deltas, target_mask, _rows, _assign, count, n_pos = out
    return rois.unsqueeze(0), target_class_ids, target_deltas, target_mask, count, n_pos


def detection_target_layer(proposals, gt_class_ids, gt_boxes, gt_masks, config, keys=None):
    """The reference's detection_target_layer (model.py:545-724), name, first five parameters and its four return values: (rois fp32
    [n, 4], target_class_ids int32 [n], target_deltas fp32 [n, 4], target_mask fp32 [n, H, W]) with n <= config.TRAIN_ROIS_PER_IMAGE,
    positives first.

    The size of the result depends on the data, so the count is read once: the call's only host wait (detection_targets_padded has
    none).  Where there is no positive the results are empty, which is what predict tests (:1803); where the crowd filter leaves no
    box the reference raises and this returns empty results too.  target_class_ids is always int32 (the reference returns int64 when
    there is no negative)."""
    rois, target_class_ids, target_deltas, target_mask, count, _n_pos = detection_targets_padded(proposals, gt_class_ids, gt_boxes,
                                                                                                  gt_masks, config, keys=keys)
    n = int(count.item())
    return rois[0, :n], target_class_ids[:n], target_deltas[:n], target_mask[:n]
