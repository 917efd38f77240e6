#!/usr/bin/env python3
"""Times the scene-input stage (derender3d/scene.py) on a VKITTI-shaped frame: 375 x 1242, 16 objects, rois drawn as
bench.edit_pipeline draws them (centre within +-0.12 / +-0.7 of the principal point in normalised units, 40-150 x 60-300
pixels).  Prints one JSON line:
  device   wall time (host clock around a synchronised region, median of --reps warm runs) of CropPlan + image_mask_crops
           (tables, one upload, cover pre-pass, crop launch), of ignore_crops, and of the construction up to the encoder
  host     the same crops through tests/scene_util.py's PIL loop -- the reference's host path: each mask fetched from the
           device per object, crop_square + resize + to_tensor, results stacked and uploaded
Kernel times come from running this script under `rocprofv3 --kernel-trace --stats -- python tools/time_scene_inputs.py`."""
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

H, W, N, FOCAL, U0, V0 = 375, 1242, 16, 725.0, 620.5, 187.0


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import scene_util as su
    from derender3d import scene
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    c = np.stack([rng.uniform(-0.12, 0.12, N), rng.uniform(-0.7, 0.7, N)], 1)
    h, w = rng.uniform(40, 150, N) / FOCAL, rng.uniform(60, 300, N) / FOCAL
    rn = np.stack([c[:, 0] - h / 2, c[:, 1] - w / 2, c[:, 0] + h / 2, c[:, 1] + w / 2], 1)
    rois = np.round(rn * FOCAL + np.asarray([V0, U0, V0, U0])).astype(np.int32)
    rois[:, 2:] = np.maximum(rois[:, 2:], rois[:, :2] + 2)
    image_np = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks_np = np.zeros((N, 1, H, W), np.float32)
    for n, (y0, x0, y1, x1) in enumerate(rois):
        masks_np[n, 0, max(0, y0):min(H, y1), max(0, x0):min(W, x1)] = 1.0
    image = torch.from_numpy(image_np.transpose(2, 0, 1).copy()).to(dev)
    masks = torch.from_numpy(masks_np).to(dev)
    logd = torch.from_numpy(rng.permutation(N).astype(np.float32).reshape(N, 1)).to(dev)
    cam = su.Camera(FOCAL, U0, V0)
    _, _, droi = scene.roi_norms_host(rois, cam)
    droi_d = droi.to(dev)
    mean, std = (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)
    state = {}

    def device_crops():
        plan = scene.CropPlan(rois, H, W, 224, 256, dev)
        state['plan'] = plan
        state['out'] = scene.image_mask_crops(plan, image, masks, mean, std)

    def device_ignores():
        state['ign'] = scene.ignore_crops(state['plan'], state['out'][2], logd, droi_d)

    def host_loop():
        # main.py:365-373, 418-421: masks come from the device one by one
        rgbs = torch.stack([su.transform_rgb(image_np, r, mean, std) for r in rois]).to(dev)
        ms = torch.stack([su.transform_plane(masks[n].cpu().numpy()[0], rois[n], 0) for n in range(N)]).to(dev)
        state['host'] = (rgbs, ms)

    ignores_np = su.ignore_maps(masks_np, list(range(N)))
    ignores_d = torch.from_numpy(ignores_np).to(dev)

    def host_ignores():
        state['host_ign'] = torch.stack([su.transform_plane(ignores_d[n].cpu().numpy()[0], rois[n], 255) for n in range(N)]).to(dev)

    for _ in range(a.warmup):
        device_crops(), device_ignores(), host_loop(), host_ignores()
    res = {'frame': [H, W], 'objects': N, 'reps': a.reps,
           'device_image_mask_crops_ms': timed(device_crops, a.reps), 'device_ignore_crops_ms': timed(device_ignores, a.reps),
           'host_image_mask_crops_ms': timed(host_loop, a.reps), 'host_ignore_crops_ms': timed(host_ignores, a.reps)}
    assert torch.equal(state['out'][0], state['host'][0]) and torch.equal(state['out'][1], state['host'][1])
    sides = np.maximum(rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1])
    res['window_sides'] = [int(sides.min()), int(np.median(sides)), int(sides.max())]
    # bytes: cover reads N H W floats and writes H W words; the crops write N (3 S_i^2 + S_m^2) floats and read each window
    res['cover_bytes'] = N * H * W * 4 + H * W * 4
    res['crop_bytes_written'] = N * (3 * 224 * 224 + 256 * 256) * 4
    res['crop_window_bytes'] = int((sides.astype(np.int64) ** 2).sum() * (3 + 4))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
