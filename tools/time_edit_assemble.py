#!/usr/bin/env python3
"""Time the edit assembly on the GPU: data.assemble.assemble_edit (one sdn_edit_assemble launch for F frames) against the
host-loop composition a user had to write before it (per object masked writes, then np.unique + one masked write per
instance and channel: textural/edit_vkitti.py:62-103), on the same seeded inputs, F = 4 frames of 375 x 1242 -> 368 x 1248.

Device events around warmed-up repetitions; the kernel's bytes come from its contract (5 B read and 4 (2 + P + C) B written
per pixel).  `--kernel-only` runs just the launches (for a kernel trace in a run of its own).  Prints markdown.
"""
import argparse
import os
import sys
from math import pi
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'textural')):
    sys.path.insert(0, p)

H, W, F, C, BINS, OBJECTS = 375, 1242, 4, 5, 24, 10


def frames(dev):
    rng = np.random.default_rng(1)
    segm = np.zeros((H, W), np.uint8)
    for y in range(0, H, 25):
        for x in range(0, W, 54):
            segm[y:y + 25, x:x + 54] = rng.choice([0, 3, 4, 5, 6, 8, 9])
    inst0 = np.zeros((H, W), np.uint8)
    boxes = []
    for k in range(1, OBJECTS + 1):
        y, x, h, w = 150 + 40 * (k % 3), 20 + 120 * (k - 1), int(rng.integers(30, 90)), int(rng.integers(60, 100))   # disjoint
        boxes.append((y, x, h, w))
        inst0[y:y + h, x:x + w] = k
        segm[y:y + h, x:x + w] = 1 if k % 3 else 11
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    edits = []
    for f in range(F):
        e = np.zeros((H, W), np.uint8)
        js = {}
        for k, (y, x, h, w) in enumerate(boxes, 1):
            dx = 7 * (f + 1)
            e[y:y + h, x + dx:x + dx + w] = k
            js[str(k)] = {'class_id': 1 if k % 3 else 2, 'alpha': float(rng.uniform(-pi, pi))}
        edits.append((e, js, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[:, :, None])).permute(2, 0, 1).contiguous().to(dev)  # noqa: E731
    return t(segm), t(image), t(inst0), [(t(e), js, t(n)) for e, js, n in edits]


def host_loop(asm, opt, params, base_item, feat_dict, edit_u8, js, normal_u8):
    inst = asm._geometry(edit_u8, opt, params, 'nearest').int()
    segm = base_item['label'].int().clone()
    feat = torch.zeros(opt.feat_num, segm.shape[1], segm.shape[2], device=segm.device)
    pose = torch.zeros(1, segm.shape[1], segm.shape[2], device=segm.device)
    segm[(segm == 2) | (segm == 12)] = 5
    bins = asm.pose_bins(opt.feat_pose_num_bins)
    for key, rec in js.items():
        m = inst == int(key)
        inst[m] = 1000 * int(key)
        segm[m] = {1: 2, 2: 12}[rec['class_id']]
        pose[m] = int(np.digitize(rec['alpha'] / pi, bins))
    inst = torch.where(inst == 0, segm, inst)
    normal = asm.transform(normal_u8, opt, params) + 1 / 255
    for i in np.unique(inst.cpu().numpy()):
        m = inst[0] == int(i)
        for j in range(opt.feat_num):
            feat[j][m] = feat_dict[int(i)][j]
    return segm.float(), inst.float(), pose, feat, normal


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--kernel-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_edit_assemble needs a GPU: timings taken anywhere else say nothing')
    from data import assemble as asm
    from sdn_hip import ops
    dev = torch.device('cuda:0')
    opt = SimpleNamespace(resize_or_crop='none', loadSize=1248, fineWidth=1248, fineHeight=368, isTrain=False, no_flip=True,
                          n_downsample_global=4, netG='global', n_local_enhancers=0, feat_num=C, feat_pose='1',
                          feat_pose_num_bins=BINS, feat_normal='1', feat_depth='', label_nc=14, no_instance=False,
                          segm_precomputed_path='geometric', inst_precomputed_path='geometric')
    params = {'crop_pos': (0, 0), 'flip': False}
    segm, image, inst0, edits = frames(dev)
    base = asm.assemble_item(opt, params, segm, image, inst=inst0)
    ids = torch.unique(base['inst'].long())
    g = torch.Generator().manual_seed(2)
    means = (torch.rand(ids.numel(), C, generator=g) * 2 - 1).to(dev)
    codes = (ids, means)
    feat_dict = {int(i): [float(v) for v in row] for i, row in zip(ids.cpu().tolist(), means.cpu().tolist())}
    lists = ([e[0] for e in edits], [e[1] for e in edits], codes, [e[2] for e in edits])
    x = asm.assemble_edit(opt, params, base, *lists)
    h, w = x['label'].shape[2:]
    assert (h, w) == (368, 1248) and x['missing'].cpu().tolist() == [0] * F
    # the launch alone, on prepared device tensors
    edit = torch.stack([asm._geometry(e[0], opt, params, 'nearest') for e in edits])
    ol, op = torch.from_numpy(x['obj_label']).to(dev), torch.from_numpy(x['obj_pose']).to(dev)
    ids32, codes_ck = ids.to(torch.int32), means.t().contiguous()
    launch = lambda: ops.edit_assemble(base['label'][None], edit, ol, op, ids32, codes_ck)   # noqa: E731
    if args.kernel_only:
        for _ in range(args.reps):
            launch()
        torch.cuda.synchronize()
        return
    for f, (e, js, n) in enumerate(edits):      # same values before any clock is read
        want = host_loop(asm, opt, params, base, feat_dict, e, js, n)
        for k, t in zip(('label', 'inst', 'pose', 'feat', 'normal'), want):
            assert torch.equal(x[k][f], t), (f, k)
    t_launch = timed(launch, args.reps)
    t_asm = timed(lambda: asm.assemble_edit(opt, params, base, *lists), max(args.reps // 4, 5))
    t_host = timed(lambda: [host_loop(asm, opt, params, base, feat_dict, e, js, n) for e, js, n in edits], 5, warm=1)
    nbytes = F * h * w * (5 + 4 * (2 + 1 + C))
    print('| what (F = %d frames, %d x %d, %d codes of %d channels) | ms per call |' % (F, h, w, ids.numel(), C))
    print('|---|---|')
    print('| `ops.edit_assemble`: allocation of the outputs, clearing of `missing`, one kernel (device events over %d back-to-back calls) | %.4f |'
          % (args.reps, t_launch))
    print('| `assemble_edit`: + NEAREST geometry of the id maps, table upload, BICUBIC normals | %.3f |' % t_asm)
    print('| host-loop composition of the same tensors (per object / per instance masked writes, np.unique) | %.2f |' % t_host)
    print()
    print('bytes moved by the kernel per call (contract): %.1f MB; over the back-to-back call time that is %.0f GB/s '
          '(a lower bound on the kernel: the figure includes the launch gaps)' % (nbytes / 1e6, nbytes / t_launch / 1e6))


if __name__ == '__main__':
    main()
