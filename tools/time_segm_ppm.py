#!/usr/bin/env python3
"""Times the pyramid pooling module at the decoder's size (conv5 [2, 2048, 47, 156], four branches of 512 channels at scales
1, 2, 3, 6: the 384 x 1248 crop at 1 / 8).  Prints one JSON line:
  device_fwd_ms, device_fwdbwd_ms   semantic.ppm.ppm_concat (two launches of the library around the branch modules), and with
                                    the backward pass for a fixed upstream gradient on the concatenated tensor (two more)
  torch_fwd_ms, torch_fwdbwd_ms     the reference's loop on the same device and the same branch modules (semantic/models.py:339-346:
                                    AdaptiveAvgPool2d, the branch, upsample per scale, torch.cat), and with its backward pass
  *_launches                        kernels per call as torch.profiler counts them, the branch modules' included (null where
                                    the profiler is unavailable)
There is no parent-commit form of this path; the comparison is against the torch expressions.  Each figure: --inner calls inside
one synchronised region of the host clock, divided by --inner; the median of --reps such regions, the forms alternating inside
every repetition, after --warmup calls of each; *_spread is (min, max) over the repetitions.  The branch modules run in eval()
(BatchNorm with running statistics) in both forms.  Checks first that both forms give the same tensor and gradients (1e-5)."""
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

SHAPE = (2, 2048, 47, 156)
SCALES = (1, 2, 3, 6)
K = 512


class Branches(nn.Module):
    """the part of the decoders that semantic.ppm reads: ppm and a conv_last to stand for the rest"""

    def __init__(self, fc_dim):
        super().__init__()
        self.ppm = nn.ModuleList([nn.Sequential(nn.AdaptiveAvgPool2d(s), nn.Conv2d(fc_dim, K, kernel_size=1, bias=False),
                                                nn.BatchNorm2d(K), nn.ReLU(inplace=True)) for s in SCALES])
        self.conv_last = nn.Identity()


def torch_form(dec, conv5):
    h, w = conv5.shape[2:]
    outs = [conv5]
    for branch in dec.ppm:
        outs.append(F.interpolate(branch(conv5), size=(h, w), mode='bilinear', align_corners=False))
    return torch.cat(outs, 1)


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
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    from semantic import ppm
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    B, C, h, w = SHAPE
    torch.manual_seed(5)
    dec = Branches(C).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(5)
    conv5 = torch.randn(B, C, h, w, device='cuda', generator=g).requires_grad_()
    go = torch.randn(B, C + len(SCALES) * K, h, w, device='cuda', generator=g)
    params = [conv5] + list(dec.parameters())

    def clear():
        for p in params:
            p.grad = None

    def device_fwd():
        with torch.no_grad():
            return ppm.ppm_concat(dec, conv5)

    def torch_fwd():
        with torch.no_grad():
            return torch_form(dec, conv5)

    def device_fwdbwd():
        clear()
        ppm.ppm_concat(dec, conv5).backward(go)

    def torch_fwdbwd():
        clear()
        torch_form(dec, conv5).backward(go)

    forms = {'device_fwd': device_fwd, 'torch_fwd': torch_fwd, 'device_fwdbwd': device_fwdbwd, 'torch_fwdbwd': torch_fwdbwd}
    rel = lambda x, y: float((x - y).norm() / y.norm())
    same = {'cat': rel(device_fwd(), torch_fwd())}
    device_fwdbwd()
    gd = [p.grad.clone() for p in params]
    torch_fwdbwd()
    same['grad_conv5'] = rel(gd[0], params[0].grad)
    same['grad_branch_weights'] = max(rel(x, p.grad) for x, p in zip(gd[1:], params[1:]) if p.dim() == 4)
    assert all(v <= 1e-5 for v in same.values()), same
    del gd
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    samples = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
            samples[k].append(region(fn, a.inner))
    res = {'shape': list(SHAPE), 'scales': list(SCALES), 'branch_channels': K, 'reps': a.reps, 'inner': a.inner,
           'conv5_bytes': B * C * h * w * 4, 'cat_bytes': B * (C + len(SCALES) * K) * h * w * 4}
    for k, v in samples.items():
        res[k + '_ms'] = round(statistics.median(v), 4)
        res[k + '_spread'] = [round(min(v), 4), round(max(v), 4)]
    for k, fn in forms.items():
        res[k + '_launches'] = count_launches(fn)
    res['rel_2norm_between_forms'] = same
    print(json.dumps(res))


if __name__ == '__main__':
    main()
