#!/usr/bin/env python3
"""Times the semantic tail on one seeded VKITTI-sized frame (C = 14, 375 x 1242, the five test scales' maps 13 x 42 .. 47 x 156;
tests/segm_tail_util.FULL).  Prints one JSON line:
  fuse_device_ms    semantic.segm_tail.fuse_predictions (one sdn_segm_fuse launch; the label map stays on the device)
  fuse_torch_ms     the reference's form on the same device (semantic/vkitti_test.py:58-72): per scale upsample, softmax and
                    add at full resolution, then .cpu() of the [1, 14, 375, 1242] sum and torch.max on the host
  update_device_ms  SegmEvaluator.update (one sdn_segm_confusion launch, nothing fetched)
  update_numpy_ms   accuracy() and intersectionAndUnion() of semantic/utils.py restated in numpy on maps already on the host
host clock around a synchronised region, median of --reps after --warmup; the two kernels alone between events on the stream;
the bytes each form moves by its algorithm.  Checks that the two forms give the same labels outside the 8 e_ref band and the
same counts.  Needs the repository's tests/ directory (tests/segm_tail_util.py)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def events(fn, reps):
    """median microseconds of fn's launches between two events on the current stream"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def numpy_counts(preds, label, C):
    """utils.py:101-129"""
    valid = label >= 0
    acc_sum, valid_sum = (valid * (preds == label)).sum(), valid.sum()
    imPred, imLab = preds + 1, label + 1
    imPred = imPred * (imLab > 0)
    intersection = imPred * (imPred == imLab)
    area_intersection, _ = np.histogram(intersection, bins=C, range=(1, C))
    area_pred, _ = np.histogram(imPred, bins=C, range=(1, C))
    area_lab, _ = np.histogram(imLab, bins=C, range=(1, C))
    return np.concatenate((area_intersection, area_pred, area_lab, [acc_sum, valid_sum, 0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import segm_tail_util as u
    from sdn_hip import ops
    from semantic import segm_tail as st
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    seed, B, C, (H, W), sizes = u.FULL
    scores = [torch.from_numpy(t).cuda() for t in u.draw_scores(seed, B, C, sizes)]
    state = {}

    def fuse_device():
        state['labels'] = st.fuse_predictions(scores, (H, W))

    def fuse_torch():
        pred = torch.zeros(B, C, H, W, device='cuda')
        for t in scores:
            x = torch.nn.functional.interpolate(t, size=(H, W), mode='bilinear', align_corners=False)
            pred = pred + torch.nn.functional.softmax(x, dim=1) / len(scores)
        _, preds = torch.max(pred.cpu(), dim=1)
        state['preds'] = preds

    gt = torch.randint(-1, C + 1, (B, H, W), device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)).to(torch.int16)
    ev = st.SegmEvaluator(C)

    def update_device():
        del ev._rows[:]
        ev.update(state['labels'], gt)

    for _ in range(a.warmup):
        fuse_device()
        fuse_torch()
        update_device()
    preds_h, gt_h = state['preds'][0].numpy().astype(np.int64), gt[0].cpu().numpy().astype(np.int64)
    res = {'frame': [H, W], 'classes': C, 'scales': len(scores), 'reps': a.reps,
           'fuse_device_ms': wall(fuse_device, a.reps), 'fuse_torch_ms': wall(fuse_torch, a.reps),
           'update_device_ms': wall(update_device, a.reps),
           'update_numpy_ms': wall(lambda: numpy_counts(preds_h, gt_h, C), max(3, a.reps // 3))}
    table = ops.segm_scale_table(scores)
    import sdn_hip
    lab = state['labels']
    res['fuse_kernel_us'] = events(lambda: sdn_hip.check(sdn_hip.lib().sdn_segm_fuse(
        table.ctypes.data, len(scores), B, C, H, W, lab.data_ptr(), None, sdn_hip.stream())), a.reps)
    res['confusion_chain_us'] = events(lambda: ops.segm_confusion(lab, gt, C), a.reps)
    in_bytes = sum(t.numel() * 4 for t in scores)
    res['fuse_bytes'] = in_bytes + B * H * W
    # per scale: read the map, write and re-read the upsampled tensor, write the softmax, re-read it with the running sum, write the sum
    full = B * C * H * W * 4
    res['torch_bytes'] = in_bytes + len(scores) * 6 * full + full
    res['torch_device_to_host_bytes'] = full
    res['fuse_device_to_host_bytes'] = 0
    # the same result: labels outside the band of the float64 pipeline, counts equal to numpy's on the device labels
    pred64 = u.pipeline(scores, (H, W), torch.float64, 'cuda')
    e_ref = float((u.pipeline(scores, (H, W), torch.float32, 'cuda').double() - pred64).abs().max())
    arg, margin = u.margins(pred64)
    clear = margin > 8 * e_ref
    assert bool((lab[:, 0].long()[clear] == arg[clear]).all()) and bool((state['preds'].cuda()[clear] == arg[clear]).all())
    assert np.array_equal(ev.counts()[0], numpy_counts(lab[0, 0].cpu().numpy().astype(np.int64), gt_h, C))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
