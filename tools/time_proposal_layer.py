#!/usr/bin/env python3
"""Times the proposal layer at the reference's size (geometric/maskrcnn/config.py): a 1024 x 1024 image, A = 261 888 anchors, the best
K = 6000 of them into the NMS at threshold 0.7, P = 1000 (POST_NMS_ROIS_INFERENCE) and 2000 (POST_NMS_ROIS_TRAINING) proposals.
Prints one JSON line; per P
  device_ms      maskrcnn.proposals.proposals_padded (sdn_proposal_layer: nothing crosses to the host)
  sequence_ms    the reference's sequence (model.py:359-405) written in torch ops on the same GPU, with this project's pth_nms for
                 its nms: a full sort of the scores, three gathers, the element-wise decode and clip, a cat, the NMS (one host read
                 of the kept count), the slice, the gather and the division
  *_launches     kernels per call as torch.profiler counts them (null where the profiler is unavailable)
The inputs are the object-like draw of tests/proposal_layer_util.py's `full` case.  Each figure: --inner calls inside one synchronised
region of the host clock, divided by --inner; the median of --reps such regions, the forms alternating inside every repetition, after
--warmup calls of each; *_spread is (min, max) over the repetitions.  Checks first that both forms keep the same anchors and that
their normalised boxes agree to 2^-20 (exp may differ in its last bit)."""
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

COUNTS = (1000, 2000)


class Config(object):
    def __init__(self, std_dev, image):
        self.RPN_BBOX_STD_DEV = np.array(std_dev)
        self.IMAGE_SHAPE = np.array([image[0], image[1], 3])


def sequence_form(inputs, proposal_count, nms_threshold, anchors, config, nms):
    """proposal_layer of the reference under a current torch, without changing `inputs`"""
    probs, deltas = inputs[0].squeeze(0), inputs[1].squeeze(0)
    scores = probs[:, 1]
    std_dev = torch.from_numpy(np.reshape(config.RPN_BBOX_STD_DEV, [1, 4])).float().to(probs.device)
    deltas = deltas * std_dev
    pre_nms_limit = min(6000, anchors.size()[0])
    scores, order = scores.sort(descending=True)
    order = order[:pre_nms_limit]
    scores = scores[:pre_nms_limit]
    deltas = deltas[order, :]
    boxes = anchors[order, :]
    height = boxes[:, 2] - boxes[:, 0]
    width = boxes[:, 3] - boxes[:, 1]
    center_y = boxes[:, 0] + 0.5 * height
    center_x = boxes[:, 1] + 0.5 * width
    center_y = center_y + deltas[:, 0] * height
    center_x = center_x + deltas[:, 1] * width
    height = height * torch.exp(deltas[:, 2])
    width = width * torch.exp(deltas[:, 3])
    y1 = center_y - 0.5 * height
    x1 = center_x - 0.5 * width
    boxes = torch.stack([y1, x1, y1 + height, x1 + width], dim=1)
    h, w = (float(v) for v in config.IMAGE_SHAPE[:2])
    boxes = torch.stack([boxes[:, 0].clamp(0.0, h), boxes[:, 1].clamp(0.0, w), boxes[:, 2].clamp(0.0, h), boxes[:, 3].clamp(0.0, w)], 1)
    keep = nms(torch.cat((boxes, scores.unsqueeze(1)), 1), nms_threshold)
    keep = keep[:proposal_count]
    boxes = boxes[keep, :]
    norm = torch.tensor([h, w, h, w], device=boxes.device)
    return (boxes / norm).unsqueeze(0), order[keep]


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
    import proposal_layer_util as u
    from maskrcnn import proposals
    from maskrcnn.nms.pth_nms import pth_nms
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    c = u.draw_case('full')
    cfg = Config(c['std_dev'], c['image'])
    inputs = [torch.from_numpy(c['probs'].copy())[None].cuda(), torch.from_numpy(c['deltas'].copy())[None].cuda()]
    anchors = torch.from_numpy(c['anchors'].copy()).cuda()
    res = {'image': c['image'], 'A': c['A'], 'K': c['K'], 'nms_threshold': c['thr'], 'reps': a.reps, 'inner': a.inner, 'calls': {}}
    for P in COUNTS:
        def device():
            return proposals.proposals_padded(inputs, P, c['thr'], anchors, cfg)

        def sequence():
            return sequence_form(inputs, P, c['thr'], anchors, cfg, pth_nms)

        forms = {'device': device, 'sequence': sequence}
        # the same result first
        from sdn_hip import ops
        order, _boxes, keep, count, rois = ops.proposal_layer(inputs[0], inputs[1], anchors, c['std_dev'], c['image'][0], c['image'][1], P, c['thr'])
        n = int(count.item())
        want, kept = sequence()
        assert want.shape == (1, n, 4) and torch.equal(order[keep[:n].long()].long(), kept), 'the two forms keep different anchors'
        assert float((want[0] - rois[:n]).abs().max()) <= 2.0 ** -20, 'the two forms differ'
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        samples = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
                samples[k].append(region(fn, a.inner))
        r = {'P': P, 'kept': n}
        for k, v in samples.items():
            r[k + '_ms'] = round(statistics.median(v), 5)
            r[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
        for k, fn in forms.items():
            r[k + '_launches'] = count_launches(fn)
        res['calls']['P%d' % P] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
