#!/usr/bin/env python3
"""Times the semantic training loss at the reference's default size (B = 2, C = 14, 48 x 156: the 384 x 1248 crop at 1 / 8), with
and without the deepsup head.  Prints one JSON line; per variant:
  device_fwd_ms, device_fwdbwd_ms   semantic.train_loss.segm_losses (two launches), and with loss.backward() (one more)
  torch_fwd_ms, torch_fwdbwd_ms     the reference's expressions on the same device (semantic/models.py:15-21, 39-44: log_softmax
                                    per head, nn.NLLLoss(ignore_index=-1) per head, the scaled sum, pixel_acc), and with
                                    loss.backward()
  *_launches                        kernels per call as torch.profiler counts them (null where the profiler is unavailable)
Each figure: --inner calls inside one synchronised region of the host clock, divided by --inner; the median of --reps such
regions, the two forms alternating inside every repetition, after --warmup calls of each; *_spread is (min, max) over the
repetitions.  Both forms keep everything on the device; the time is launch-bound at this size (0.8 MB of scores per head), so
it is the host's enqueue rate as much as the kernels.  Checks that both forms give the same loss and gradient (1e-6) and the
same acc (to three pixels: a tie made by rounding)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd')):
    sys.path.insert(0, p)

SHAPE = (2, 14, 48, 156)
SCALE = 0.4


def torch_form(s0, s1, label):
    crit = nn.NLLLoss(ignore_index=-1)
    pred = F.log_softmax(s0, dim=1)
    loss = crit(pred, label)
    if s1 is not None:
        loss = loss + crit(F.log_softmax(s1, dim=1), label) * SCALE
    _, preds = torch.max(pred, dim=1)
    valid = (label >= 0).long()
    acc_sum = torch.sum(valid * (preds == label).long())
    pixel_sum = torch.sum(valid)
    acc = acc_sum.float() / (pixel_sum.float() + 1e-10)
    return loss, acc


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
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    from semantic import train_loss
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    B, C, h, w = SHAPE
    g = torch.Generator(device='cuda').manual_seed(5)
    base0 = 4 * torch.randn(B, C, h, w, device='cuda', generator=g)
    base1 = 4 * torch.randn(B, C, h, w, device='cuda', generator=g)
    label = torch.randint(-1, C, (B, h, w), device='cuda', generator=g)
    label[1, 40:] = -1
    res = {'shape': list(SHAPE), 'reps': a.reps, 'inner': a.inner, 'score_bytes_per_head': B * C * h * w * 4}
    for variant in ('deepsup', 'main_only'):
        s0 = base0.clone().requires_grad_()
        s1 = base1.clone().requires_grad_() if variant == 'deepsup' else None

        def clear():
            s0.grad = None
            if s1 is not None:
                s1.grad = None

        def device_fwd():
            return train_loss.segm_losses(s0, label, s1, SCALE if s1 is not None else None)

        def device_fwdbwd():
            clear()
            device_fwd()['loss'].backward()

        def torch_fwd():
            return torch_form(s0, s1, label)

        def torch_fwdbwd():
            clear()
            torch_form(s0, s1, label)[0].backward()

        forms = {'device_fwd': device_fwd, 'torch_fwd': torch_fwd, 'device_fwdbwd': device_fwdbwd, 'torch_fwdbwd': torch_fwdbwd}
        # the same result first
        d = device_fwd()
        t_loss, t_acc = torch_fwd()
        dl, tl = float(d['loss'].detach()), float(t_loss.detach())
        assert abs(dl - tl) <= 1e-6 * abs(tl), (dl, tl)
        # the two arg-max rules may part on a pixel whose two best log-probabilities round together
        assert abs(float(d['acc'].detach()) - float(t_acc)) <= 3.0 / float(d['pixel_sum']), (float(d['acc'].detach()), float(t_acc))
        device_fwdbwd()
        gd = s0.grad.clone()
        torch_fwdbwd()
        rel = float((gd - s0.grad).norm() / s0.grad.norm())
        assert rel <= 1e-6, rel
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        samples = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
                samples[k].append(region(fn, a.inner))
        out = {}
        for k, v in samples.items():
            out[k + '_ms'] = round(statistics.median(v), 5)
            out[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
        for k, fn in forms.items():
            out[k + '_launches'] = count_launches(fn)
        out['gradient_rel_2norm_between_forms'] = rel
        res[variant] = out
    print(json.dumps(res))


if __name__ == '__main__':
    main()
