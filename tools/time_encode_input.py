#!/usr/bin/env python3
"""Times the textural input encoding on the device against the torch expressions it replaces, on the same GPU in the same
process, at the sizes a user runs: batch 4 at 384 x 1248 (a train step) and batch 1 at 192 x 624 (an edited frame), label_nc 14,
24 pose bins, a VKITTI-like instance map (rectangular instances with ids x 1000 over a background of class ids, as
tests/test_gpu_textural_fullsize.py draws them), all maps fp32 as textural.data.assemble hands them over.

Without --case the tool runs each size as a child process of its own under `timeout -k 10`, one after the other, and stops at the
first that fails; with --case it measures that size and prints one JSON line:
  encode_device_ms, encode_torch_ms   the planes of Pix2PixHDModel.encode_input (_encode_maps_fused's call against _one_hot +
                                      get_edges + cat + _one_hot)
  index_device_ms, index_torch_ms     the numbering of Encoder._pooled with counts (input_maps.instance_index against
                                      _disambiguate + torch.unique), each call on a fresh copy of the map (the copy is in both)
  *_launches                          kernels per call as torch.profiler counts them, memsets and copies apart (null where the
                                      profiler is unavailable)
Each figure: --inner calls inside one synchronised region of the host clock, divided by --inner; the median of --reps such
regions, the two forms alternating inside every repetition, after --warmup calls of each; *_spread is (min, max) over the
repetitions.  Both forms include the one host synchronisation of the numbering.  Checks first that both forms give equal
tensors."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'textural')):
    sys.path.insert(0, p)

CASES = {'batch4_384x1248': (4, 384, 1248), 'batch1_192x624': (1, 192, 624)}
LABEL_NC, POSE_CH = 14, 25
CHILD_SECONDS = 240


def region(fn, inner, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def count_launches(fn, torch):
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


def maps(torch, n, h, w):
    g = torch.Generator().manual_seed(16)
    label = torch.randint(0, LABEL_NC, (n, 1, h, w), generator=g).float()
    pose = torch.randint(0, POSE_CH, (n, 1, h, w), generator=g).float()
    inst = label.clone()                                       # the background carries the class ids
    for i in range(n):
        for k in range(10):
            y0, x0 = int(torch.randint(0, h - h // 6, (1,), generator=g)), int(torch.randint(0, w - w // 6, (1,), generator=g))
            inst[i, 0, y0:y0 + int(torch.randint(h // 20, h // 6, (1,), generator=g)),
                 x0:x0 + int(torch.randint(w // 30, w // 6, (1,), generator=g))] = 1000 * (k + 1)
    return label.cuda(), inst.cuda(), pose.cuda()


def measure(name, a):
    import torch
    from models import input_maps, networks
    from models.pix2pixHD_model import Pix2PixHDModel
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    n, h, w = CASES[name]
    label, inst, pose = maps(torch, n, h, w)
    m = Pix2PixHDModel.__new__(Pix2PixHDModel)

    def encode_device():
        return input_maps.encode_maps(label, inst, pose, LABEL_NC, POSE_CH)[:2]

    def encode_torch():
        return torch.cat((m._one_hot(label, LABEL_NC), m.get_edges(inst)), dim=1), m._one_hot(pose, POSE_CH)

    def index_device():
        return input_maps.instance_index(inst.clone(), True)[:3]

    def index_torch():
        d = networks.Encoder._disambiguate(inst.clone())
        ids, inverse, counts = torch.unique(d.reshape(-1).long(), return_inverse=True, return_counts=True)
        return ids, inverse.to(torch.int32).reshape(n, h, w), counts

    forms = {'encode_device': encode_device, 'encode_torch': encode_torch, 'index_device': index_device, 'index_torch': index_torch}
    assert all(torch.equal(x, y) for x, y in zip(encode_device(), encode_torch())), 'the planes differ'
    assert all(torch.equal(x, y) for x, y in zip(index_device(), index_torch())), 'the numbering differs'
    assert input_maps.instance_index(inst.clone(), True)[3]['path'] == 'device'
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    samples = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():   # alternating: what disturbs one form disturbs the other
            samples[k].append(region(fn, a.inner, torch))
    res = {'case': name, 'shape': [n, 1, h, w], 'label_nc': LABEL_NC, 'pose_ch': POSE_CH, 'reps': a.reps, 'inner': a.inner,
           'ids': int(index_device()[0].numel()), 'plane_bytes': n * (LABEL_NC + 1 + POSE_CH) * h * w * 4}
    for k, v in samples.items():
        res[k + '_ms'] = round(statistics.median(v), 4)
        res[k + '_spread'] = [round(min(v), 4), round(max(v), 4)]
    for k, fn in forms.items():
        res[k + '_launches'] = count_launches(fn, torch)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=sorted(CASES))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    if a.case:
        measure(a.case, a)
        return 0
    for name in CASES:   # every GPU step under its own time limit; the first failure ends the run
        rc = subprocess.call(['timeout', '-k', '10', str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), '--case', name,
                              '--reps', str(a.reps), '--inner', str(a.inner), '--warmup', str(a.warmup)])
        if rc != 0:
            print('%s ended with status %d; nothing further was started' % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
