#!/usr/bin/env python3
"""Times the textural loader's item on seeded frames, B = 1, 4 and 16 items per call, at the VKITTI size (375 x 1242 scaled to
192 x 624) and at the Cityscapes size (1024 x 2048 scaled to width 1024, a 512 x 1024 crop).  Prints one JSON line per size:
  batch   data.assemble.assemble_batch: table upload and the four launches (host clock around a synchronised region, median
          of --reps); the sdn_assemble_planes launch of the image alone between hipEvents on the stream, the bytes it moves by
          the algorithm (the source rows and columns the windows need, read once, plus the fp32 planes written) and its rate
  item    data.assemble.assemble_item, the tensor-op form, called per item on the same device tensors
  host    the PIL flow of the reference's loader on the host (oracle/loader_oracle.get_item for VKITTI,
          tests/cityscapes_loader_util.cityscapes_item for Cityscapes) from PIL images already decoded, per item
and checks that batch and item (VKITTI) / batch and host (Cityscapes) give the same tensors.  With --profile N it only runs
assemble_batch N times at --size / --batch, for a `rocprofv3 --kernel-trace --stats` run.  The Cityscapes host flow is the
restatement the tests use (tests/cityscapes_loader_util.py, as tools/time_cityscapes_gt.py takes tests/cityscapes_util.py)."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'textural'), os.path.join(ROOT, 'tests')):
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


def options(**kw):
    """the loader options of the reference's training default (scale_width_and_crop, flips, instance, pose and normal features)"""
    o = dict(resize_or_crop='scale_width_and_crop', loadSize=624, fineWidth=624, fineHeight=192, isTrain=True, no_flip=False,
             n_downsample_global=4, netG='global', n_local_enhancers=1, label_nc=14, no_instance=False,
             segm_precomputed_path='', inst_precomputed_path='', feat_pose='x', feat_pose_num_bins=24, feat_normal='x')
    o.update(kw)
    return SimpleNamespace(**o)


def frame(seed, H, W, cityscapes):
    rng = np.random.default_rng(seed)
    segm = rng.integers(0, 34 if cityscapes else 14, (H, W), dtype=np.uint8)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    normal = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pose = np.zeros((H, W), dtype=np.uint8)
    js = {}
    for k in range(1, 13):
        y0, x0 = int(rng.integers(0, H - H // 5)), int(rng.integers(0, W - W // 5))
        pose[y0:y0 + int(rng.integers(H // 30, H // 5)), x0:x0 + int(rng.integers(W // 30, W // 5))] = k
        js[str(k)] = {'class_id': 1, 'alpha': float(rng.uniform(-np.pi, np.pi))}
    inst = pose
    if cityscapes:
        inst = segm.astype(np.uint16)
        inst[pose > 0] = 26000 + pose[pose > 0].astype(np.uint16)
    return {'segm': segm, 'image': image, 'inst': inst, 'pose_inst': pose, 'pose_json': js, 'normal': normal}


def to_device(src):
    def t(a):
        if not isinstance(a, np.ndarray):
            return a
        if a.dtype == np.uint16:
            a = a.astype(np.int32)
        return torch.from_numpy(a if a.ndim == 3 else a[:, :, None]).permute(2, 0, 1).contiguous().cuda()
    return {k: t(v) for k, v in src.items()}


def plane_bytes(asm, opt, params, H, W):
    """bytes sdn_assemble_planes moves by the algorithm for 3 planes of every item: the source rectangle the window needs, once,
    and the fp32 window"""
    sh, sw, h, w, crops = asm.batch_geometry(opt, H, W)
    total = 0
    for p in params:
        x1, y1 = p['crop_pos'] if crops else (0, 0)
        xs = np.arange(x1, min(x1 + w, sw))
        ys = np.arange(y1, min(y1 + h, sh))
        cols = len(np.unique(asm._resample_table(W, sw, 'bicubic')[0].numpy()[xs])) if sw != W else len(xs)
        rows = len(np.unique(asm._resample_table(H, sh, 'bicubic')[0].numpy()[ys])) if sh != H else len(ys)
        total += 3 * (rows * cols + 4 * h * w)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--profile', type=int, default=0)
    ap.add_argument('--size', default='cityscapes')
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_assemble_batch.py needs a GPU'
    import cityscapes_loader_util as cu
    from data import assemble as asm
    from oracle import loader_oracle as lo
    from sdn_hip import ops
    sizes = {'vkitti': ((375, 1242), options(), 'vkitti'),
             'cityscapes': ((1024, 2048), options(loadSize=1024, fineWidth=1024, fineHeight=512, label_nc=20), 'cityscapes')}
    for name, ((H, W), opt, dataset) in sizes.items():
        if args.profile and name != args.size:
            continue
        city = dataset == 'cityscapes'
        srcs = [frame(s, H, W, city) for s in range(4)]
        devs = [to_device(s) for s in srcs]
        sh, sw, h, w, crops = asm.batch_geometry(opt, H, W)
        rng = np.random.default_rng(1)
        for B in ((args.batch,) if args.profile else (1, 4, 16)):
            params = [{'crop_pos': (int(rng.integers(0, sw - w + 1)), int(rng.integers(0, sh - h + 1))), 'flip': bool(b & 1)}
                      for b in range(B)]
            frames = [devs[b % 4] for b in range(B)]

            def batch():
                return asm.assemble_batch(opt, params, frames, dataset=dataset, inst_wrap_int16=city)
            if args.profile:
                for _ in range(args.profile):
                    batch()
                torch.cuda.synchronize()
                continue

            def item():
                return [asm.assemble_item(opt, p, f['segm'], f['image'], f['inst'] if not city else None, f['pose_inst'],
                                          f['pose_json'], f['normal']) for p, f in zip(params, frames)]
            pils = [{k: (cu.pil(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in srcs]

            def host():
                out = []
                for b, p in enumerate(params):
                    f = pils[b % 4]
                    if city:
                        out.append(cu.cityscapes_item(opt, p, f['segm'], f['image'], f['inst'], f['pose_inst'], f['pose_json'],
                                                      f['normal'], label_table=asm.CITYSCAPES_LABEL_TABLE))
                    else:
                        out.append(lo.get_item(opt, p, f['segm'], f['image'], f['inst'], f['pose_inst'], f['pose_json'], f['normal']))
                return out
            got = batch()
            ref = host() if city else item()
            for b in range(B):
                for k in ('label', 'inst', 'image', 'pose', 'normal'):
                    assert torch.equal(got[k][b].cpu(), ref[b][k].cpu()), (name, B, b, k)
            for _ in range(3):
                batch()
                item()
            # the image planes' launch alone, on tables uploaded once
            d = asm._upload(frames[0]['image'].device, {
                'items': np.array([[p['crop_pos'][0] if crops else 0, p['crop_pos'][1] if crops else 0, int(p['flip']), 0] for p in params],
                                  np.int32),
                'lut': asm._to_tensor_lut().numpy(), 'src': np.array([f['image'].data_ptr() for f in frames], np.int64),
                'xmin': asm._resample_table(W, sw, 'bicubic')[0][:, 0].numpy().astype(np.int32),
                'xk': asm._resample_table(W, sw, 'bicubic')[1].numpy().astype(np.int32),
                'ymin': asm._resample_table(H, sh, 'bicubic')[0][:, 0].numpy().astype(np.int32),
                'yk': asm._resample_table(H, sh, 'bicubic')[1].numpy().astype(np.int32)})
            items_host = d['items'].cpu().numpy()

            def planes():
                return ops.assemble_planes(d['src'], items_host, d['items'], (d['xmin'], d['xk']), (d['ymin'], d['yk']), d['lut'], 3,
                                           H, W, sh, sw, h, w)
            assert torch.equal(planes(), got['image'])
            us = events(planes, args.reps)
            nbytes = plane_bytes(asm, opt, params, H, W)
            print(json.dumps({'size': name, 'source': [H, W], 'scaled': [sh, sw], 'window': [h, w], 'B': B,
                              'batch_ms': round(wall(batch, args.reps), 4), 'item_ms': round(wall(item, args.reps), 4),
                              'host_ms': round(wall(host, args.host_reps), 3), 'planes_us': round(us, 2),
                              'planes_bytes': nbytes, 'planes_GBps': round(nbytes / us / 1e3, 1)}), flush=True)


if __name__ == '__main__':
    main()
