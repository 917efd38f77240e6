#!/usr/bin/env python3
"""Times the detection targets at the reference's size (geometric/maskrcnn/config.py): N = 2000 proposals (POST_NMS_ROIS_TRAINING),
R = 200 (TRAIN_ROIS_PER_IMAGE), ratio 0.33, 56 x 56 mini-masks, a 28 x 28 target, with G = 24 and G = 100 boxes.  Prints one JSON line;
per G
  device_ms      maskrcnn.detection_targets.detection_targets_padded (sdn_detection_targets: nothing crosses to the host)
  sequence_ms    the reference's sequence (model.py:570-724) written in torch ops on the same GPU under a current torch: the .any() and
                 nonzero calls with their waits, the repeated IoU matrix, the gathers, box_refinement, this project's
                 CropAndResizeFunction, the cats.  Its two host randperm calls with their uploads are replaced by one stable device
                 argsort of the sampling keys each, so that both forms choose the same rows; that is no host wait more or fewer.
  *_launches     kernels per call as torch.profiler counts them (null where the profiler is unavailable)
  count, positives   rows in use and positives among them
The inputs are the draws `real` and `real_g100` of tests/detection_targets_util.py.  Each figure: --inner calls inside one
synchronised region of the host clock, divided by --inner; the median of --reps such regions, the forms alternating inside every
repetition, after --warmup calls of each; *_spread is (min, max) over the repetitions.  Checks first that both forms return the same
rois, class ids and masks; deltas_difference is the largest difference of the deltas."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

CASES = ('real', 'real_g100')


class Config(object):
    def __init__(self, c):
        self.BBOX_STD_DEV = np.array(c['std_dev'])
        self.TRAIN_ROIS_PER_IMAGE, self.ROI_POSITIVE_RATIO = c['R'], c['ratio']
        self.USE_MINI_MASK, self.MASK_SHAPE = c['mini'], list(c['shape'])


def bbox_overlaps(boxes1, boxes2):
    """model.py:508-542"""
    n1, n2 = boxes1.size()[0], boxes2.size()[0]
    boxes1 = boxes1.repeat(1, n2).view(-1, 4)
    boxes2 = boxes2.repeat(n1, 1)
    b1_y1, b1_x1, b1_y2, b1_x2 = boxes1.chunk(4, dim=1)
    b2_y1, b2_x1, b2_y2, b2_x2 = boxes2.chunk(4, dim=1)
    y1 = torch.max(b1_y1, b2_y1)[:, 0]
    x1 = torch.max(b1_x1, b2_x1)[:, 0]
    y2 = torch.min(b1_y2, b2_y2)[:, 0]
    x2 = torch.min(b1_x2, b2_x2)[:, 0]
    zeros = torch.zeros(y1.size()[0], device=y1.device)
    intersection = torch.max(x2 - x1, zeros) * torch.max(y2 - y1, zeros)
    b1_area = (b1_y2 - b1_y1) * (b1_x2 - b1_x1)
    b2_area = (b2_y2 - b2_y1) * (b2_x2 - b2_x1)
    union = b1_area[:, 0] + b2_area[:, 0] - intersection
    return (intersection / union).view(n1, n2)


def box_refinement(box, gt_box):
    """utils.py:92-113"""
    height = box[:, 2] - box[:, 0]
    width = box[:, 3] - box[:, 1]
    center_y = box[:, 0] + 0.5 * height
    center_x = box[:, 1] + 0.5 * width
    gt_height = gt_box[:, 2] - gt_box[:, 0]
    gt_width = gt_box[:, 3] - gt_box[:, 1]
    gt_center_y = gt_box[:, 0] + 0.5 * gt_height
    gt_center_x = gt_box[:, 1] + 0.5 * gt_width
    dy = (gt_center_y - center_y) / height
    dx = (gt_center_x - center_x) / width
    dh = torch.log(gt_height / height)
    dw = torch.log(gt_width / width)
    return torch.stack([dy, dx, dh, dw], dim=1)


def sequence_form(proposals, gt_class_ids, gt_boxes, gt_masks, config, keys, crop):
    """detection_target_layer of the reference under a current torch (model.py:570-724)"""
    dev = proposals.device
    if (gt_class_ids < 0).any():
        crowd_ix = torch.nonzero(gt_class_ids < 0)[:, 0]
        non_crowd_ix = torch.nonzero(gt_class_ids > 0)[:, 0]
        crowd_boxes = gt_boxes[crowd_ix, :]
        gt_class_ids = gt_class_ids[non_crowd_ix]
        gt_boxes = gt_boxes[non_crowd_ix, :]
        gt_masks = gt_masks[non_crowd_ix, :]
        crowd_overlaps = bbox_overlaps(proposals, crowd_boxes)
        crowd_iou_max = torch.max(crowd_overlaps, dim=1)[0]
        no_crowd_bool = crowd_iou_max < 0.001
    else:
        no_crowd_bool = torch.ones(proposals.size()[0], dtype=torch.bool, device=dev)
    overlaps = bbox_overlaps(proposals, gt_boxes)
    roi_iou_max = torch.max(overlaps, dim=1)[0]
    positive_roi_bool = roi_iou_max >= 0.5
    if positive_roi_bool.any():
        positive_indices = torch.nonzero(positive_roi_bool)[:, 0]
        positive_count = int(config.TRAIN_ROIS_PER_IMAGE * config.ROI_POSITIVE_RATIO)
        rand_idx = torch.argsort(keys[0][positive_indices], stable=True)[:positive_count]      # in place of randperm
        positive_indices = positive_indices[rand_idx]
        positive_count = positive_indices.size()[0]
        positive_rois = proposals[positive_indices, :]
        positive_overlaps = overlaps[positive_indices, :]
        roi_gt_box_assignment = torch.max(positive_overlaps, dim=1)[1]
        roi_gt_boxes = gt_boxes[roi_gt_box_assignment, :]
        roi_gt_class_ids = gt_class_ids[roi_gt_box_assignment]
        deltas = box_refinement(positive_rois, roi_gt_boxes)
        std_dev = torch.from_numpy(config.BBOX_STD_DEV).float().to(dev)
        deltas /= std_dev
        roi_masks = gt_masks[roi_gt_box_assignment, :, :]
        boxes = positive_rois
        if config.USE_MINI_MASK:
            y1, x1, y2, x2 = positive_rois.chunk(4, dim=1)
            gt_y1, gt_x1, gt_y2, gt_x2 = roi_gt_boxes.chunk(4, dim=1)
            gt_h = gt_y2 - gt_y1
            gt_w = gt_x2 - gt_x1
            y1 = (y1 - gt_y1) / gt_h
            x1 = (x1 - gt_x1) / gt_w
            y2 = (y2 - gt_y1) / gt_h
            x2 = (x2 - gt_x1) / gt_w
            boxes = torch.cat([y1, x1, y2, x2], dim=1)
        box_ids = torch.arange(roi_masks.size()[0], device=dev).int()
        masks = crop(config.MASK_SHAPE[0], config.MASK_SHAPE[1], 0)(roi_masks.unsqueeze(1), boxes, box_ids)
        masks = torch.round(masks.squeeze(1))
    else:
        positive_count = 0
    negative_roi_bool = (roi_iou_max < 0.5) & no_crowd_bool
    if negative_roi_bool.any() and positive_count > 0:
        negative_indices = torch.nonzero(negative_roi_bool)[:, 0]
        r = 1.0 / config.ROI_POSITIVE_RATIO
        negative_count = int(r * positive_count - positive_count)
        rand_idx = torch.argsort(keys[1][negative_indices], stable=True)[:negative_count]       # in place of randperm
        negative_indices = negative_indices[rand_idx]
        negative_count = negative_indices.size()[0]
        negative_rois = proposals[negative_indices, :]
    else:
        negative_count = 0
    assert positive_count > 0 and negative_count > 0, 'the timed cases have both'
    rois = torch.cat((positive_rois, negative_rois), dim=0)
    roi_gt_class_ids = torch.cat([roi_gt_class_ids.int(), torch.zeros(negative_count, device=dev).int()], dim=0)
    deltas = torch.cat([deltas, torch.zeros(negative_count, 4, device=dev)], dim=0)
    masks = torch.cat([masks, torch.zeros(negative_count, config.MASK_SHAPE[0], config.MASK_SHAPE[1], device=dev)], dim=0)
    return rois, roi_gt_class_ids, deltas, masks


def region(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n or None
    except Exception:   # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import detection_targets_util as u
    from maskrcnn import detection_targets
    from maskrcnn.roialign.roi_align.crop_and_resize import CropAndResizeFunction
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    res = {'reps': a.reps, 'inner': a.inner, 'calls': {}}
    for name in CASES:
        c = u.draw_case(name)
        cfg = Config(c)
        proposals, ids, boxes, masks, keys = (torch.from_numpy(c[k].copy()).cuda() for k in u.INPUTS)

        def device():
            return detection_targets.detection_targets_padded(proposals, ids, boxes, masks, cfg, keys=keys)

        def sequence():
            return sequence_form(proposals, ids, boxes, masks, cfg, keys, CropAndResizeFunction)

        forms = {'device': device, 'sequence': sequence}
        # the same result first
        rois, cls, deltas, mask, count, n_pos = device()
        n, P = int(count.item()), int(n_pos.item())
        want = sequence()
        assert want[0].shape == (n, 4) and torch.equal(want[0], rois[0, :n]) and torch.equal(want[1], cls[:n]), 'the two forms differ'
        assert torch.equal(want[3], mask[:n]), 'the two forms differ'
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        samples = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
                samples[k].append(region(fn, a.inner))
        r = {'N': c['N'], 'G': c['G'], 'R': c['R'], 'ratio': c['ratio'], 'mask': c['mask'], 'shape': c['shape'], 'count': n, 'positives': P,
             'deltas_difference': float((want[2] - deltas[:n]).abs().max())}
        for k, v in samples.items():
            r[k + '_ms'] = round(statistics.median(v), 5)
            r[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
        for k, fn in forms.items():
            r[k + '_launches'] = count_launches(fn)
        res['calls'][name] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
