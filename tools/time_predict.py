#!/usr/bin/env python3
"""Times two things on the same GPU and prints one JSON line.

  rpn_outputs    sdn_hip.ops.rpn_outputs against the torch expressions of the RPN's tail (tests/predict_util.py: rpn_tail -- per level
                 two permute(0, 2, 3, 1).contiguous().view and a softmax, then three cats) at the reference's size: a 1024 x 1024
                 image, levels 256 .. 16 squared, k = 3, A = 261 888 (geometric/maskrcnn/config.py); forward alone, and forward +
                 backward with gradients into rpn_class_logits and rpn_bbox, as a training step sends them
  predict        maskrcnn.predict.predict_padded(mode='inference') against the same chain with the torch RPN tail in place of the
                 kernel, on the stand-in network of tests/predict_util.py (128 x 128, A = 4092): the chain's other launches are the
                 same in both forms
  *_launches     kernels per call as torch.profiler counts them (null where the profiler is unavailable)
Each figure: --inner calls inside one synchronised region of the host clock, divided by --inner; the median of --reps such regions,
the two forms alternating inside every repetition, after --warmup calls of each; *_spread is (min, max) over the repetitions.  Checks
first that both forms of a pair return the same logits and boxes, bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

LEVELS = [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]


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


def measure(forms, a):
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    samples = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
            samples[k].append(region(fn, a.inner))
    r = {}
    for k, v in samples.items():
        r[k + '_ms'] = round(statistics.median(v), 5)
        r[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
    for k, fn in forms.items():
        r[k + '_launches'] = count_launches(fn)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import predict_util as u
    from maskrcnn import predict as pr
    from sdn_hip import ops
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    res = {'reps': a.reps, 'inner': a.inner}

    cls, box = u.draw_maps(LEVELS, 3, 1, seed=41, device='cuda')
    for t in cls + box:
        t.requires_grad_(True)
    got, want = ops.rpn_outputs(cls, box), u.rpn_tail(cls, box)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), 'the forms differ'
    g_logits, g_bbox = torch.randn_like(got[0]), torch.randn_like(got[2])

    def both_ways(form):
        def run():
            out = form(cls, box)
            torch.autograd.backward([out[0], out[2]], [g_logits, g_bbox])
            for t in cls + box:
                t.grad = None
        return run

    def forward_only(form):
        def run():
            with torch.no_grad():
                form(cls, box)
        return run

    r = {'A': int(got[0].shape[1]), 'bytes_moved_forward': 4 * (sum(t.numel() for t in cls + box) + sum(t.numel() for t in got)),
         'probs_distance_from_torch': float((got[1] - want[1]).abs().max())}
    r.update({'forward_' + k: v for k, v in measure({'kernel': forward_only(ops.rpn_outputs), 'torch': forward_only(u.rpn_tail)}, a).items()})
    r.update({'both_ways_' + k: v for k, v in measure({'kernel': both_ways(ops.rpn_outputs), 'torch': both_ways(u.rpn_tail)}, a).items()})
    res['rpn_outputs'] = r

    model = u.StandIn().to_device('cuda')
    inp = [u.molded(u.painted_frame()).cuda(), u.image_metas()]

    def chain(tail):
        def run():
            saved = pr.rpn_outputs
            pr.rpn_outputs = tail                     # rpn_forward looks the name up at call time
            try:
                with torch.no_grad():
                    return pr.predict_padded(model, inp, 'inference')
            finally:
                pr.rpn_outputs = saved
        return run

    forms = {'kernel': chain(pr.rpn_outputs), 'torch': chain(u.rpn_tail)}
    x, y = forms['kernel'](), forms['torch']()
    assert torch.equal(x[2], y[2]), 'the forms differ'
    r = {'A': int(model.anchors.shape[0]), 'detections': int(x[2])}
    r.update(measure(forms, a))
    res['predict'] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
