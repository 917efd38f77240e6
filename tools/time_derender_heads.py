#!/usr/bin/env python3
"""Times sdn_hip.ops.derender_heads against the module's torch statements on the same GPU and prints one JSON line.

  kernel         ops.derender_heads(pooled, roi_norms, fc, fc1, fc2, fc3, 8): the roi arithmetic, the four layers, the slices, the
                 normalisation and the softmax
  torch          the statements of Derenderer3d.forward and Derenderer.forward behind the ResNet's pooling (tests/derender_heads_util.py:
                 heads, the same expressions on the device): nn.Linear through torch's BLAS, ReLU, cat, slices, norm, softmax
at the real widths (512 -> 256 -> 256 -> 1552, 8 classes) for n = 16 (a frame) and n = 64 (a training step); forward alone, and
forward + backward with a gradient into every output group, into pooled and the eight parameters.
  *_launches     kernels per call as torch.profiler counts them (null where the profiler is unavailable)
Each figure: --inner calls inside one synchronised region of the host clock, divided by --inner; the median of --reps such regions,
the two forms alternating inside every repetition, after --warmup calls of each; *_spread is (min, max) over the repetitions.  One
run, no threshold: it checks first that the two forms agree to 1e-5 of each group's largest magnitude."""
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
    import derender_heads_util as u
    from sdn_hip import ops
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    res = {'reps': a.reps, 'inner': a.inner}
    _pooled, _roi, params = u.draw('real_16')
    params = [p.cuda().requires_grad_(True) for p in params]
    for n in (16, 64):
        g = torch.Generator().manual_seed(n)
        pooled = torch.rand(n, 512, generator=g).cuda().requires_grad_(True)
        top_left = -torch.rand(n, 2, generator=g) * 0.5
        roi = torch.cat((top_left, top_left + 0.1 + torch.rand(n, 2, generator=g) * 0.5), dim=1).cuda()
        grads = [torch.rand(s, generator=g).cuda() * 2 - 1 for s in ((n, 2), (n, 2), (n, 3), (n, 1), (n, 8), (n, 8, 192))]

        def kernel():
            return ops.derender_heads(pooled, roi, params[0:2], params[2:4], params[4:6], params[6:8], 8)

        def torch_form():
            return u.heads(pooled, roi, params, 8)

        got, want = kernel(), torch_form()
        for k in u.KEYS:
            assert float((got[k] - want[k]).abs().max()) <= 1e-5 * float(want[k].abs().max()), k

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        def both_ways(fn):
            def run():
                blob = fn()
                torch.autograd.grad([blob[k] for k in u.KEYS], [pooled] + params, grads)
            return run
        r = {}
        r.update({'forward_' + k: v for k, v in measure({'kernel': forward_only(kernel), 'torch': forward_only(torch_form)}, a).items()})
        r.update({'both_ways_' + k: v for k, v in measure({'kernel': both_ways(kernel), 'torch': both_ways(torch_form)}, a).items()})
        res['n_%d' % n] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
