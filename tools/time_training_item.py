#!/usr/bin/env python3
"""Times the Mask R-CNN training item at the reference's size: a 375 x 1242 VKITTI frame into 1024 x 1024 (IMAGE_MIN_DIM 800,
IMAGE_MAX_DIM 1024), MINI_MASK_SHAPE (56, 56), G = 24 instances, with the colour jitter (all four ops) and the mirror.  Prints one
JSON line:
  device_ms        maskrcnn.training_item.training_item (sdn_training_item: one upload of the parameter block, nothing crosses back)
  device_full_ms   the same with use_mini_mask=False (fp32 [G, 1024, 1024] masks)
  mold_ms          maskrcnn.training_item.mold_inputs on the one frame (the image kernel alone)
  host_ms          tests/training_item_util.py: training_item on the host over Pillow and scipy.ndimage.zoom, which is what
                   Dataset.__getitem__ pays per item before its upload; the median of --host-reps calls
  *_launches       kernels per call as torch.profiler counts them (null where the profiler is unavailable)
The host form does not run the code under test.  Each device figure: --inner calls inside one synchronised region of the host clock,
divided by --inner; the median of --reps such regions, the forms alternating inside every repetition, after --warmup calls of each;
*_spread is (min, max) over the repetitions.  Checks first that the device and the host give the same bits."""
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

H, W, G = 375, 1242, 24


def draw(seed=7):
    """a noisy frame and a scene map with G ellipses of their own colours, small and large, some cut by the frame's edge"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    frame = np.clip((xx * 255 // (W - 1))[..., None] + rng.integers(-80, 81, (H, W, 3)), 0, 255).astype(np.uint8)
    codes = rng.permutation(200)[:G, None].astype(np.uint8) + np.array([[1, 20, 40]], np.uint8)
    scene = np.zeros((H, W, 3), np.uint8)
    for g in range(G):
        cy, cx = rng.integers(60, H), rng.integers(0, W)
        ry, rx = rng.integers(8, 150), rng.integers(10, 200)
        scene[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = codes[g]
    return frame, scene, codes


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
    import training_item_util as u
    from maskrcnn import training_item as ti
    from sdn_hip import pillow
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    cfg = u.Config(800, 1024, 56)
    frame, scene, codes = draw()
    ids = ti.color_keys(codes)
    jitter = ([pillow.SATURATION, pillow.CONTRAST, pillow.HUE, pillow.BRIGHTNESS], (1.2, 0.8, 1.3), 21)
    d_frame, d_scene, d_ids = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (frame, scene, ids))
    d_class = torch.ones(G, dtype=torch.int32, device='cuda')

    def device():
        return ti.training_item(d_frame, d_scene, d_ids, d_class, cfg, flip=1, jitter=jitter, use_mini_mask=True)

    def device_full():
        return ti.training_item(d_frame, d_scene, d_ids, d_class, cfg, flip=1, jitter=jitter, use_mini_mask=False)

    def mold():
        return ti.mold_inputs([d_frame], cfg)

    def host(use_mini=True):
        return u.training_item(frame, scene, ids, cfg, flip=True, jitter=jitter, use_mini_mask=use_mini)

    for fn, use_mini in ((device, True), (device_full, False)):   # the same bits first
        item, want = fn(), host(use_mini)
        for k in ('image', 'gt_boxes_int', 'gt_boxes', 'gt_boxes_norm', 'gt_masks', 'areas', 'bad'):
            assert getattr(item, k).cpu().numpy().tobytes() == want[k].tobytes(), 'the forms differ in %s' % k
    forms = {'device': device, 'device_full': device_full, 'mold': mold}
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
        host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    want = host()
    res = {'reps': a.reps, 'inner': a.inner, 'H': H, 'W': W, 'G': G, 'M': cfg.IMAGE_MAX_DIM, 'mini': list(cfg.MINI_MASK_SHAPE),
           'block_bytes': int(ti.plan_block(frame.shape, cfg)[0].nbytes), 'instance_pixels': int(want['areas'].sum()),
           'tallest_box': int((want['gt_boxes_int'][:, 2] - want['gt_boxes_int'][:, 0]).max()),
           'host_ms': round(statistics.median(host_ms), 2), 'host_spread': [round(min(host_ms), 2), round(max(host_ms), 2)]}
    for k, v in samples.items():
        res[k + '_ms'] = round(statistics.median(v), 5)
        res[k + '_spread'] = [round(min(v), 5), round(max(v), 5)]
    for k, fn in forms.items():
        res[k + '_launches'] = count_launches(fn)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
