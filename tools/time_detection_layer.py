#!/usr/bin/env python3
"""Times the detection layer at the reference's size (geometric/maskrcnn/config.py): a 1024 x 1024 image, N = 1000 classified
proposals (POST_NMS_ROIS_INFERENCE), D = 100 (DETECTION_MAX_INSTANCES), confidence 0.7, threshold 0.3, with C = 3 (VKitti) and C = 81
classes.  Prints one JSON line; per C
  device_ms      maskrcnn.detection_layer.detections_padded (sdn_detection_layer: nothing crosses to the host)
  sequence_ms    the reference's sequence (model.py:760-835) written in torch ops on the same GPU, with this project's pth_nms for
                 its nms: the arg-max and two gathers, the element-wise decode, scale, clip and round, a nonzero, then per class
                 present a nonzero, a sort, the gathers, a cat, the NMS and the union, then the intersect and the final sort
  *_launches     kernels per call as torch.profiler counts them (null where the profiler is unavailable)
  valid, kept    rows that enter the NMS and rows it keeps before the cut to D; early_stop: whether kept reached D
The inputs are the object-like draws `real_c3` and `real_c81` of tests/detection_layer_util.py.  Each figure: --inner calls inside one
synchronised region of the host clock, divided by --inner; the median of --reps such regions, the forms alternating inside every
repetition, after --warmup calls of each; *_spread is (min, max) over the repetitions.  Checks first that both forms return the same
detections bit for bit (the boxes are whole pixels)."""
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

CASES = ('real_c3', 'real_c81')


class Config(object):
    def __init__(self, c):
        self.RPN_BBOX_STD_DEV = np.array(c['std_dev'])
        self.IMAGE_SHAPE = np.array([c['image'][0], c['image'][1], 3])
        self.DETECTION_MIN_CONFIDENCE = c['conf']
        self.DETECTION_NMS_THRESHOLD = c['thr']
        self.DETECTION_MAX_INSTANCES = c['D']


def unique1d(t):
    if t.size()[0] < 2:
        return t
    t = t.sort()[0]
    first = torch.ones(1, dtype=torch.bool, device=t.device)
    return t[torch.cat((first, t[1:] != t[:-1]), dim=0)]


def intersect1d(a, b):
    aux = torch.cat((a, b), dim=0).sort()[0]
    return aux[:-1][aux[1:] == aux[:-1]]


def sequence_form(rois, probs, deltas, window, config, nms, cut=True):
    """refine_detections of the reference under a current torch"""
    dev = rois.device
    _, class_ids = torch.max(probs, dim=1)
    idx = torch.arange(class_ids.size()[0], device=dev)
    class_scores = probs[idx, class_ids]
    deltas_specific = deltas[idx, class_ids]
    std_dev = torch.from_numpy(np.reshape(config.RPN_BBOX_STD_DEV, [1, 4])).float().to(dev)
    d = deltas_specific * std_dev
    height = rois[:, 2] - rois[:, 0]
    width = rois[:, 3] - rois[:, 1]
    center_y = rois[:, 0] + 0.5 * height
    center_x = rois[:, 1] + 0.5 * width
    center_y = center_y + d[:, 0] * height
    center_x = center_x + d[:, 1] * width
    height = height * torch.exp(d[:, 2])
    width = width * torch.exp(d[:, 3])
    y1 = center_y - 0.5 * height
    x1 = center_x - 0.5 * width
    refined = torch.stack([y1, x1, y1 + height, x1 + width], dim=1)
    h, w = (int(v) for v in config.IMAGE_SHAPE[:2])
    refined = refined * torch.from_numpy(np.array([h, w, h, w])).float().to(dev)
    refined = torch.stack([refined[:, 0].clamp(float(window[0]), float(window[2])), refined[:, 1].clamp(float(window[1]), float(window[3])),
                           refined[:, 2].clamp(float(window[0]), float(window[2])), refined[:, 3].clamp(float(window[1]), float(window[3]))], 1)
    refined = torch.round(refined)
    keep_bool = class_ids > 0
    if config.DETECTION_MIN_CONFIDENCE:
        keep_bool = keep_bool & (class_scores >= config.DETECTION_MIN_CONFIDENCE)
    keep = torch.nonzero(keep_bool)[:, 0]
    pre_ids, pre_scores, pre_rois = class_ids[keep], class_scores[keep], refined[keep]
    nms_keep = None
    for class_id in unique1d(pre_ids):
        ixs = torch.nonzero(pre_ids == class_id)[:, 0]
        ix_scores, order = pre_scores[ixs].sort(descending=True)
        ix_rois = pre_rois[ixs][order, :]
        class_keep = nms(torch.cat((ix_rois, ix_scores.unsqueeze(1)), dim=1), config.DETECTION_NMS_THRESHOLD)
        class_keep = keep[ixs[order[class_keep]]]
        nms_keep = class_keep if nms_keep is None else unique1d(torch.cat((nms_keep, class_keep)))
    keep = intersect1d(keep, nms_keep)
    top = class_scores[keep].sort(descending=True)[1]
    if cut:
        top = top[:config.DETECTION_MAX_INSTANCES]
    keep = keep[top]
    return torch.cat((refined[keep], class_ids[keep].unsqueeze(1).float(), class_scores[keep].unsqueeze(1)), dim=1)


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
    import detection_layer_util as u
    from maskrcnn import detection_layer
    from maskrcnn.nms.pth_nms import pth_nms
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    res = {'reps': a.reps, 'inner': a.inner, 'calls': {}}
    for name in CASES:
        c = u.draw_case(name)
        cfg = Config(c)
        rois, probs, deltas = (torch.from_numpy(c[k].copy()).cuda() for k in ('rois', 'probs', 'deltas'))

        def device():
            return detection_layer.detections_padded(rois, probs, deltas, c['window'], cfg)

        def sequence():
            return sequence_form(rois, probs, deltas, c['window'], cfg, pth_nms)

        forms = {'device': device, 'sequence': sequence}
        # the same result first
        det, _norm, count = device()
        n = int(count.item())
        want = sequence()
        assert want.shape == (n, 6) and torch.equal(want, det[:n]), 'the two forms differ'
        kept = sequence_form(rois, probs, deltas, c['window'], cfg, pth_nms, cut=False).shape[0]
        valid = int(((probs.argmax(1) > 0) & (probs.max(1)[0] >= c['conf'])).sum())
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        samples = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
                samples[k].append(region(fn, a.inner))
        r = {'N': c['N'], 'C': c['C'], 'D': c['D'], 'image': c['image'], 'valid': valid, 'kept': kept, 'detections': n, 'early_stop': kept >= c['D']}
        for k, v in samples.items():
            r[k + '_ms'] = round(statistics.median(v), 5)
            r[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
        for k, fn in forms.items():
            r[k + '_launches'] = count_launches(fn)
        res['calls'][name] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
