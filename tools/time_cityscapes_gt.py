#!/usr/bin/env python3
"""Times the Cityscapes ground-truth source on one seeded 1024 x 2048 frame with 20 cars (tests/cityscapes_util.big_frame; the
largest car 86 450 pixels), 16 selected.  Prints one JSON line:
  device   derender3d.scene.cityscapes_gt_inputs: the sdn_scene_id_stats chain, the table to the host, selection and thresholds,
           one upload, the sdn_scene_id_planes launch (host clock around a synchronised region, median of --reps); the chain
           and the planes launch alone between hipEvents on the stream; the bytes each moves by the algorithm and its rate
  host     a restatement of the reference's flow (geometric/scripts/main.py:763-795, 812-818) in numpy on the maps already on
           the host, then what SceneSession(image_ignores=...) needs of it: the float32 upload of the selected masks and ignore
           planes and ops.scene_cover of the ignores (its stages are reported one by one)
and checks that the two give the same masks and cover words.  With --profile N it only runs the device flow N times, for a
`rocprofv3 --kernel-trace --stats` run.  Needs the repository's tests/ directory (tests/cityscapes_util.py)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--profile', type=int, default=0)
    a = ap.parse_args()
    import cityscapes_util as cu
    from derender3d import scene as sc
    from sdn_hip import ops
    dev = torch.device('cuda:0')
    scene_h, disparity_h = cu.big_frame()
    H, W = scene_h.shape
    scene, disparity = torch.from_numpy(scene_h).to(dev), torch.from_numpy(disparity_h).to(dev)
    state = {}

    def device_flow():
        state['dev'] = sc.cityscapes_gt_inputs(scene, disparity)

    if a.profile:
        for _ in range(a.profile):
            device_flow()
        torch.cuda.synchronize()
        return

    stages = {}

    def host_flow():
        t = [time.perf_counter()]

        def lap(name):
            t.append(time.perf_counter())
            stages.setdefault(name, []).append((t[-1] - t[-2]) * 1e3)
        image_scene, image_disparity = scene_h[..., None], disparity_h[..., None]
        masks, ignores = [], []
        for obj_index in np.unique(image_scene):
            if obj_index // 1000 != 26:
                continue
            image_mask = np.all(image_scene == [obj_index], axis=2, keepdims=True).astype(np.float32)
            d = image_disparity[image_mask.astype(bool)]
            d = d[d != 0]
            d = np.percentile(d, 95) if d.size else 0
            image_ignore = np.all((image_disparity > d) == 1.0, axis=2, keepdims=True).astype(np.float32)
            masks.append(np.transpose(image_mask, (2, 0, 1)))
            ignores.append(np.transpose(image_ignore, (2, 0, 1)))
        lap('host_loop_ms')
        masks, ignores = np.stack(masks, axis=0), np.stack(ignores, axis=0)
        sels = np.flipud(np.argsort(np.sum(masks, axis=(1, 2, 3))))[:min(len(masks), 16)]
        masks, ignores = masks[sels], ignores[sels]
        lap('host_stack_select_ms')
        masks_d, ignores_d = torch.from_numpy(masks).to(dev), torch.from_numpy(ignores).to(dev)
        torch.cuda.synchronize()
        lap('host_float32_upload_ms')
        state['host'] = (masks_d, ops.scene_cover(ignores_d))
        torch.cuda.synchronize()
        lap('host_scene_cover_ms')

    for _ in range(a.warmup):
        device_flow()
    host_flow()
    stages.clear()
    res = {'frame': [H, W], 'cars': int(len(np.unique(scene_h[scene_h // 1000 == 26]))), 'selected': int(state['dev'][0].shape[0]),
           'largest_car_pixels': int(state['dev'][3].max()), 'reps': a.reps, 'device_flow_ms': wall(device_flow, a.reps),
           'host_flow_ms': wall(host_flow, max(2, a.reps // 5))}
    assert torch.equal(state['dev'][0], state['host'][0]) and torch.equal(state['dev'][1], state['host'][1])
    res.update({k: statistics.median(v) for k, v in stages.items()})
    n = res['selected']
    ids_d, thr_d = sc.upload_int32([state['dev'][4], state['dev'][5]], dev)
    res['stats_chain_us'] = events(lambda: ops.scene_id_stats(scene, disparity), a.reps)
    res['planes_launch_us'] = events(lambda: ops.scene_id_planes(scene, disparity, ids_d, thr_d), a.reps)
    res['masks_only_us'] = events(lambda: ops.scene_id_planes(scene, disparity, ids_d, thr_d, cover=False), a.reps)
    res['cover_only_us'] = events(lambda: ops.scene_id_planes(scene, disparity, ids_d, thr_d, planes=False), a.reps)
    # the algorithm's traffic: two reads of the two maps and the cleared workspace; one read of the scene per plane row is what
    # the kernel issues, one read of each map plus the outputs is what the algorithm needs
    res['stats_bytes'] = 2 * 2 * H * W * 4 + 4 * (1000 * 256 + 1000 * 4 + 1000 * 2 * 256)
    res['planes_bytes'] = 2 * H * W * 4 + n * H * W * 4 + ((n + 31) // 32) * H * W * 4
    res['stats_chain_TBps'] = res['stats_bytes'] / (res['stats_chain_us'] * 1e-6) / 1e12
    res['planes_launch_TBps'] = res['planes_bytes'] / (res['planes_launch_us'] * 1e-6) / 1e12
    res['host_upload_bytes'] = 2 * n * H * W * 4
    res['device_download_bytes'] = 1000 * 8 * 4
    print(json.dumps(res))


if __name__ == '__main__':
    main()
