#!/usr/bin/env python3
"""Time the hybrid training items on the GPU (profiles/train_hybrid.md):
  (a) 16 items, 12 VKITTI (375 x 1242) + 4 Cityscapes (1024 x 2048), through derender3d.train_items.hybrid_batch;
  (b) the crops of 16 VKITTI items through sdn_train_crops_mixed and through sdn_train_crops (the same items, rois and jitter).
Synthetic frames; every figure is the median of --repeats runs after --warmup, with the spread (min .. max) beside it; (b) is
device time between two events around the one entry point, (a) wall time of the whole call including its host half.
Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric')):
    sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def vkitti_frame(rng, H=375, W=1242, n=6):
    rgb = torch.from_numpy(rng.integers(0, 256, (3, H, W), dtype=np.uint8)).cuda()
    scene = np.full((H, W, 3), 90, np.uint8)
    codes = np.stack([np.uint8([10 + 30 * k, 200 - 20 * k, 5 * k]) for k in range(n)])
    for k in range(n):
        x0 = 40 + k * 190
        scene[120 + 10 * k:300, x0:x0 + 170] = codes[k]
    rows = {'ry': rng.uniform(-3, 3, n), 'l3d': np.full(n, 4.0), 'h3d': np.full(n, 1.5), 'w3d': np.full(n, 1.7),
            'x3d': rng.uniform(-8, 8, n), 'y3d': np.full(n, 1.6), 'z3d': rng.uniform(6, 40, n)}
    return rgb, torch.from_numpy(scene).cuda(), rows, codes


def cityscapes_frame(rng, H=1024, W=2048, n=4):
    rgb = torch.from_numpy(rng.integers(0, 256, (3, H, W), dtype=np.uint8)).cuda()
    ids = np.full((H, W), 7, np.int32)
    for k in range(n):
        ids[300 + 40 * k:700, 100 + 450 * k:500 + 450 * k] = 26001 + k
    disp = rng.integers(0, 20000, (H, W)).astype(np.int32)
    return rgb, torch.from_numpy(ids).cuda(), torch.from_numpy(disp).cuda()


def spread(values):
    return {'median_ms': statistics.median(values), 'min_ms': min(values), 'max_ms': max(values), 'runs': len(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    from derender3d import scene as sc
    from derender3d import train_items as ti
    from sdn_hip import ops
    rng = np.random.default_rng(1)
    frames, items = [], []
    for f in range(4):
        rgb, scene, rows, codes = vkitti_frame(rng)
        frames.append(ti.SourceFrame(rgb, scene_u8=scene))
        items += [ti.Item(f, k, rows, codes) for k in range(4)]
    vk_items = list(items)
    rgb, ids, disp = cityscapes_frame(rng)
    frames.append(ti.SourceFrame(rgb, ids=ids, disparity=disp))
    mixed = vk_items[:12] + [ti.CityscapesItem(4, 26001 + k) for k in range(4)]

    def wall(fn):
        out = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                out.append(1e3 * (time.perf_counter() - t0))
        return out

    def device(fn):
        out = []
        for i in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                out.append(e0.elapsed_time(e1))
        return out

    result = {'hybrid_batch_12_vkitti_4_cityscapes': spread(wall(lambda: ti.hybrid_batch(frames, mixed, True, rng=random.Random(3))))}
    # (b): the same 16 VKITTI items, rois and jitter through both entry points
    fd = torch.stack([f.rgb_u8 for f in frames[:4]])
    sd = torch.stack([f.scene_u8 for f in frames[:4]])
    first = torch.tensor([[it.frame] + it.code.tolist() for it in vk_items], dtype=torch.int32).cuda()
    rois = ops.train_rois(sd, first).cpu().numpy()[:, :4]
    r = random.Random(5)
    jit = [ti.jitter_params(rng=r) for _ in vk_items]
    near = [it.codes[ti.nearer_objects(it.rows, it.index)] for it in vk_items]
    counts = [c.shape[0] for c in near]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    nearer = torch.from_numpy(np.concatenate(near)).cuda() if sum(counts) else torch.zeros(0, 3, dtype=torch.uint8).cuda()
    H, W = int(fd.shape[2]), int(fd.shape[3])
    objs, bounds, kk8 = sc.crop_tables(rois, H, W, 224, 256)
    tab = ti.item_table([it.frame for it in vk_items], [it.code for it in vk_items], offs, counts, jit)
    d = sc.upload_int32([objs, bounds, kk8, tab], fd.device)
    plain = lambda: ops.train_crops(fd, sd, rois, objs, tab, d[:3], d[3], nearer, 224, 256, ti.VKITTI_MEAN, ti.VKITTI_STD)
    recs = [{'frame': fd[it.frame], 'mask': (ti.MASK_CODE, sd[it.frame], ti._pack_code(it.code)),
             'ignore': (ti.IGNORE_NEARER, sd[it.frame], 0, int(offs[i]), counts[i]), 'jitter': jit[i], 'mean': ti.VKITTI_MEAN,
             'std': ti.VKITTI_STD} for i, it in enumerate(vk_items)]
    mtab = ti.mixed_item_table(recs)
    md = sc.upload_int32([mtab, objs, bounds, kk8], fd.device)
    mix = lambda: ops.train_crops_mixed(rois, objs, mtab, md[1:4], md[0], nearer, 224, 256)
    assert all(torch.equal(a, b) for a, b in zip(plain(), mix()))
    result['train_crops_16_vkitti'] = spread(device(plain))
    result['train_crops_mixed_16_vkitti'] = spread(device(mix))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
