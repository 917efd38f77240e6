"""The RPN targets on the device: build_rpn_targets (reference: geometric/maskrcnn/model.py:1214-1322, with compute_overlaps and
compute_iou of utils.py:52-89), which Dataset.__getitem__ (:1385) calls once per item, and the anchors it works on
(utils.generate_pyramid_anchors, utils.py:402-458).

    from maskrcnn.rpn_targets import build_rpn_targets        # instead of the one in maskrcnn.model
    rpn_match, rpn_bbox = build_rpn_targets(image.shape, anchors, gt_class_ids, gt_boxes, config)

The reference is numpy in float64 on the host: an [A, G] IoU matrix column by column (210 MB at A = 261 888, G = 100), two arg-maxes,
three masked writes, np.random.choice twice and a Python loop over the positive anchors.  Here no matrix exists: a lane owns an
anchor, walks the boxes and keeps the maximum, a table per chunk of anchors gives every box its best anchor, and an exact radix select
finds the sampling cut: csrc/rpn_targets.hip behind sdn_hip.ops.rpn_targets, eight launches.  CPU tensors raise NotImplementedError and
there is no torch form.

All arithmetic is float64, operation for operation the reference's; gt_boxes (fp32 or int32, pixels) are widened exactly to float64
first, which is what the reference computes when its boxes are integers, as extract_bboxes makes them.  Only rpn_bbox is rounded to
fp32 at the end, as Dataset.__getitem__ does (:1404).  log is the only operation whose last bit may differ from a CPU run.

The randomness comes in as data: keys fp32 [2, A], row 0 for the positives and row 1 for the negatives.  Of more than T // 2
positives the T // 2 with the smallest keys stay, then of more than T - n_pos negatives the T - n_pos with the smallest keys (key
order is the monotone image of the float's bits; equal keys keep the lower anchor) -- for uniform keys that is
np.random.choice(ids, extra, replace=False) in distribution.  With keys=None they are drawn with torch.rand on the device, which is no
host wait.

The reference's quirks are kept: the crowd filter runs only when some id is negative, and only then are ids of 0 dropped; a crowd bars
the negative label only; every box's best anchor becomes positive, anchor 0 for a box that overlaps nothing; a positive anchor's
deltas are taken against the box of its own arg-max.  One deviation, where the reference raises: if the filter leaves no box, every
anchor's maximum counts as 0 and there is no positive.

rpn_targets_padded returns the shapes losses.mrcnn_losses takes, so the RPN targets, the padded proposals, the padded detection
targets and the losses join into one training step without a host wait.  No result carries a gradient.
"""
import numpy as np
import torch

from sdn_hip import ops


def _config_values(config):
    if config is None:
        raise ValueError('config is needed: RPN_TRAIN_ANCHORS_PER_IMAGE and RPN_BBOX_STD_DEV are read from it (model.py:1230, 1319)')
    return int(config.RPN_TRAIN_ANCHORS_PER_IMAGE), [float(v) for v in config.RPN_BBOX_STD_DEV]


def rpn_targets_padded(anchors, gt_class_ids, gt_boxes, config, keys=None, gt_count=None):
    """(rpn_match int32 [1, A, 1], rpn_bbox fp32 [1, T, 4], rows int32 [T], counts int32 [2]) with T =
    config.RPN_TRAIN_ANCHORS_PER_IMAGE: the first two are the rpn_match and rpn_bbox arguments of losses.mrcnn_losses, rows holds the
    anchor of every row of rpn_bbox (-1 behind n_pos) and counts (n_pos, n_neg) after sampling.  Nothing crosses to the host.
    anchors fp64 [A, 4] in pixels, on the device; gt_class_ids int32 or int64 [G]; gt_boxes fp32 or int32 [G, 4] in pixels.  keys:
    fp32 [2, A] on the device, or None to draw torch.rand(2, A) there.  gt_count: None, or int32 [1] on the device: boxes at or
    behind it are not read, so a padded box buffer needs no host wait either."""
    T, std_dev = _config_values(config)
    if keys is None and isinstance(anchors, torch.Tensor) and anchors.is_cuda and anchors.dim() == 2:
        keys = torch.rand(2, anchors.shape[0], dtype=torch.float32, device=anchors.device)
    rpn_match, rpn_bbox, rows, counts = ops.rpn_targets(anchors, gt_class_ids, gt_boxes, keys, T, std_dev, gt_count=gt_count)
    return rpn_match.view(1, -1, 1), rpn_bbox.unsqueeze(0), rows, counts


def build_rpn_targets(image_shape, anchors, gt_class_ids, gt_boxes, config, keys=None):
    """The reference's build_rpn_targets (model.py:1214-1322), name and first five parameters: (rpn_match int32 [A], rpn_bbox fp32
    [T, 4]) as device tensors.  The shapes are fixed, so there is no host wait.  image_shape is not used, as in the reference.
    rpn_bbox is fp32, which is what Dataset.__getitem__ makes of it (:1404)."""
    rpn_match, rpn_bbox, _rows, _counts = rpn_targets_padded(anchors, gt_class_ids, gt_boxes, config, keys=keys)
    return rpn_match[0, :, 0], rpn_bbox[0]


def _level_anchors(scale, ratios, shape, feature_stride, anchor_stride):
    """the anchors of one pyramid level (utils.py:402-438), float64 [cells * ratios, 4]: cell-major, the ratios inside a cell"""
    root = np.sqrt(np.asarray(ratios, np.float64))
    heights, widths = np.float64(scale) / root, np.float64(scale) * root
    ys = np.arange(0, shape[0], anchor_stride) * feature_stride
    xs = np.arange(0, shape[1], anchor_stride) * feature_stride
    cy, cx = np.repeat(ys, len(xs)).astype(np.float64), np.tile(xs, len(ys)).astype(np.float64)
    centers = np.stack([np.repeat(cy, len(root)), np.repeat(cx, len(root))], axis=1)
    sizes = np.stack([np.tile(heights, len(cy)), np.tile(widths, len(cy))], axis=1)
    return np.concatenate([centers - 0.5 * sizes, centers + 0.5 * sizes], axis=1)


def generate_pyramid_anchors(scales, ratios, feature_shapes, feature_strides, anchor_stride):
    """The reference's utils.generate_pyramid_anchors (utils.py:441-458): numpy float64 [A, 4] = (y1, x1, y2, x2) in pixels, the
    levels in the order of the scales, one scale per level and every ratio at every level; bit for bit the reference's.  It runs on
    the host, once per configuration: torch.from_numpy(anchors).to(device) is the `anchors` of the functions above."""
    return np.concatenate([_level_anchors(scales[i], ratios, feature_shapes[i], feature_strides[i], anchor_stride)
                           for i in range(len(scales))], axis=0)
