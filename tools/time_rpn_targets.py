#!/usr/bin/env python3
"""Times the RPN targets at the reference's size (geometric/maskrcnn/config.py): the A = 261 888 anchors of a 1024 x 1024 image,
T = 256 (RPN_TRAIN_ANCHORS_PER_IMAGE), with G = 24 and G = 100 boxes.  Prints one JSON line; per G
  device_ms      maskrcnn.rpn_targets.rpn_targets_padded (sdn_rpn_targets: nothing crosses to the host, no [A, G] matrix)
  sequence_ms    the reference's sequence (model.py:1228-1322, utils.py:52-89) written in float64 torch ops on the same GPU: the
                 [A, G] IoU matrix (one broadcast instead of the reference's G column passes, which favours this form), the two
                 arg-maxes, the three masked writes, the two nonzero calls with their waits, the deltas of all positives at once
                 instead of a Python loop.  np.random.choice is replaced by one stable device argsort of the sampling keys each, so
                 that both forms choose the same anchors.
  host_ms        the contract's numpy on the host (tests/rpn_targets_util.py: contract), what Dataset.__getitem__ pays per item;
                 the median of --host-reps calls
  *_launches     kernels per call as torch.profiler counts them (null where the profiler is unavailable)
Neither baseline runs the code under test.  The inputs are the draws `full_g24` and `full` of tests/rpn_targets_util.py.  Each device
figure: --inner calls inside one synchronised region of the host clock, divided by --inner; the median of --reps such regions, the
forms alternating inside every repetition, after --warmup calls of each; *_spread is (min, max) over the repetitions.  Checks first
that all three forms return the same rpn_match, rows and counts; bbox_adjacent counts the float32 values of dh, dw one step apart."""
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

CASES = ('full_g24', 'full')


class Config(object):
    def __init__(self, c):
        self.RPN_TRAIN_ANCHORS_PER_IMAGE, self.RPN_BBOX_STD_DEV = c['T'], np.array(c['std_dev'])


def compute_overlaps(boxes1, boxes2):
    """utils.py:73-89 with compute_iou (:52-70), all columns in one broadcast: float64 [A, G]"""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    y1 = torch.maximum(boxes2[None, :, 0], boxes1[:, None, 0])
    y2 = torch.minimum(boxes2[None, :, 2], boxes1[:, None, 2])
    x1 = torch.maximum(boxes2[None, :, 1], boxes1[:, None, 1])
    x2 = torch.minimum(boxes2[None, :, 3], boxes1[:, None, 3])
    intersection = torch.clamp(x2 - x1, min=0) * torch.clamp(y2 - y1, min=0)
    union = area2[None, :] + area1[:, None] - intersection
    return intersection / union


def sequence_form(anchors, gt_class_ids, gt_boxes, config, keys):
    """build_rpn_targets of the reference in float64 torch ops (model.py:1228-1322)"""
    dev = anchors.device
    T = config.RPN_TRAIN_ANCHORS_PER_IMAGE
    gt_boxes = gt_boxes.double()
    rpn_match = torch.zeros(anchors.shape[0], dtype=torch.int32, device=dev)
    rpn_bbox = torch.zeros(T, 4, dtype=torch.float64, device=dev)
    crowd_ix = torch.nonzero(gt_class_ids < 0)[:, 0]
    if crowd_ix.shape[0] > 0:
        non_crowd_ix = torch.nonzero(gt_class_ids > 0)[:, 0]
        crowd_boxes = gt_boxes[crowd_ix]
        gt_class_ids = gt_class_ids[non_crowd_ix]
        gt_boxes = gt_boxes[non_crowd_ix]
        no_crowd_bool = compute_overlaps(anchors, crowd_boxes).amax(dim=1) < 0.001
    else:
        no_crowd_bool = torch.ones(anchors.shape[0], dtype=torch.bool, device=dev)
    overlaps = compute_overlaps(anchors, gt_boxes)
    anchor_iou_max, anchor_iou_argmax = overlaps.max(dim=1)
    rpn_match[(anchor_iou_max < 0.3) & no_crowd_bool] = -1
    gt_iou_argmax = torch.argmax(overlaps, dim=0)
    rpn_match[gt_iou_argmax] = 1
    rpn_match[anchor_iou_max >= 0.7] = 1
    ids = torch.nonzero(rpn_match == 1)[:, 0]
    extra = len(ids) - T // 2
    if extra > 0:
        order = torch.argsort(keys[0][ids], stable=True)      # in place of np.random.choice
        rpn_match[ids[order[T // 2:]]] = 0
    ids = torch.nonzero(rpn_match == -1)[:, 0]
    keep = T - int((rpn_match == 1).sum())
    if len(ids) - keep > 0:
        order = torch.argsort(keys[1][ids], stable=True)
        rpn_match[ids[order[keep:]]] = 0
    ids = torch.nonzero(rpn_match == 1)[:, 0]
    a, gt = anchors[ids], gt_boxes[anchor_iou_argmax[ids]]
    gt_h, gt_w = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    gt_center_y, gt_center_x = gt[:, 0] + 0.5 * gt_h, gt[:, 1] + 0.5 * gt_w
    a_h, a_w = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    a_center_y, a_center_x = a[:, 0] + 0.5 * a_h, a[:, 1] + 0.5 * a_w
    rpn_bbox[:len(ids)] = torch.stack([(gt_center_y - a_center_y) / a_h, (gt_center_x - a_center_x) / a_w, torch.log(gt_h / a_h),
                                       torch.log(gt_w / a_w)], dim=1) / torch.from_numpy(config.RPN_BBOX_STD_DEV).to(dev)
    return rpn_match, rpn_bbox.float()


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
    ap.add_argument('--host-reps', type=int, default=3)
    a = ap.parse_args()
    import rpn_targets_util as u
    from maskrcnn import rpn_targets
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    res = {'reps': a.reps, 'inner': a.inner, 'calls': {}}
    for name in CASES:
        c = u.draw_case(name)
        cfg = Config(c)
        anchors, ids, boxes, keys = (torch.from_numpy(np.ascontiguousarray(c[k]).copy()).cuda() for k in ('anchors', 'gt_class_ids', 'gt_boxes', 'keys'))

        def device():
            return rpn_targets.rpn_targets_padded(anchors, ids, boxes, cfg, keys=keys)

        def sequence():
            return sequence_form(anchors, ids, boxes, cfg, keys)

        forms = {'device': device, 'sequence': sequence}
        # the same result first
        match, bbox, rows, counts = device()
        host = u.contract(c)
        want = sequence()
        got_match = match[0, :, 0].cpu().numpy()
        assert np.array_equal(got_match, host['rpn_match']) and np.array_equal(want[0].cpu().numpy(), host['rpn_match']), 'the forms differ'
        assert np.array_equal(rows.cpu().numpy(), host['rows']) and np.array_equal(counts.cpu().numpy(), host['counts']), 'the forms differ'
        ok, adjacent = u.adjacent_or_equal(bbox[0].cpu().numpy(), host['rpn_bbox'])
        ok2, adjacent2 = u.adjacent_or_equal(want[1].cpu().numpy(), host['rpn_bbox'])
        assert ok and ok2, 'the deltas differ'
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        samples = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
                samples[k].append(region(fn, a.inner))
        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            u.contract(c)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        r = {'A': c['A'], 'G': c['G'], 'T': c['T'], 'positives': int(host['counts'][0]), 'negatives': int(host['counts'][1]),
             'positives_before_sampling': int((host['before'] == 1).sum()), 'negatives_before_sampling': int((host['before'] == -1).sum()),
             'bbox_adjacent': adjacent, 'sequence_bbox_adjacent': adjacent2, 'host_ms': round(statistics.median(host_ms), 2),
             'host_spread': [round(min(host_ms), 2), round(max(host_ms), 2)]}
        for k, v in samples.items():
            r[k + '_ms'] = round(statistics.median(v), 5)
            r[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
        for k, fn in forms.items():
            r[k + '_launches'] = count_launches(fn)
        res['calls'][name] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
