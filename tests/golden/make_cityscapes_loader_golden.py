#!/usr/bin/env python3
"""Generate tests/golden/cityscapes_loader_golden.npz: the reference's OWN Cityscapes loader, executed.

/root/reference/textural/data/cityscapes_dataset.py (CustomDataset.__getitem__, :32-111) on top of data/base_dataset.py is
imported as it lies -- with `torchvision.transforms` stubbed exactly as make_loader_golden.py does (torchvision is absent) --
and pointed at a temporary Cityscapes-shaped tree (annotations/instancesonly_gtFine_{train,val}.json, gtFine/, images/, the
precomputed label / instance directories and the geometric branch's pose / normal directory) holding three synthetic 64 x 128
frames.  Every option set the fixture covers is asked for its items; the fixture stores the frames' source arrays, the crop and
flip the loader drew, and every tensor of the returned `input_dict`, plus the trainId table of data/cityscapes_labels.py as a
list of integers.  tests/test_cityscapes_loader_golden.py holds the restatement and the kernels' emulation
(tests/cityscapes_loader_util.py) against it, tests/test_gpu_assemble_batch.py the kernels.  Runs only where the reference is.

Planted: pose ids 1 and 2 cover exactly 256 and 255 pixels of the val cases' transformed map (the `< 256` test of :82), id 4 is
small and has NO record (the test comes before the look-up), the label map holds every id 0..33 and 40, the 16-bit instance
map holds ids above 32 767, and case 4's crop box reaches below the scaled image.  A large instance without a record makes the
reference raise KeyError; that is kept out (tests/test_gpu_assemble_batch.py tests `missing` for it).
"""
import contextlib
import io
import json
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_loader_golden import REF, _textured, torchvision_stub  # noqa: E402

H, W = 64, 128
BASE = dict(resize_or_crop='scale_width_and_crop', loadSize=96, fineWidth=64, fineHeight=32, isTrain=False, no_flip=False,
            n_downsample_global=4, netG='global', n_local_enhancers=1, label_nc=20, no_instance=False,
            segm_precomputed=False, inst_precomputed=False, feat_pose_num_bins=24, files=('inst', 'pose', 'normal'), items=1)
CASES = [
    dict(isTrain=True, segm_precomputed=True, inst_precomputed=True, items=3),   # the geometric branch's outputs as inputs
    dict(isTrain=True, items=3),                                                 # ground truth: 16-bit instance ids
    dict(feat_pose_num_bins=0, files=('pose', 'normal')),                        # no instance file: inst IS the label tensor
    dict(segm_precomputed=True, inst_precomputed=True, files=('inst',)),         # no pose, no normal file
    dict(fineHeight=56),                                                         # the crop box reaches below the 48-row image
    dict(segm_precomputed=True, inst_precomputed=True, feat_pose_num_bins=0),
]
NAMES = ['aachen_%06d_000019' % k for k in range(3)]


def val_window_sources():
    """flat source index of every pixel of the val cases' transformed map (scale width 128 -> 96, central 32 x 64 crop), found by
    sending an index image through PIL"""
    idx = PIL.Image.fromarray(np.arange(H * W, dtype=np.int32).reshape(H, W), 'I')
    idx = idx.resize((96, 48), PIL.Image.NEAREST).crop((16, 8, 16 + 64, 8 + 32))
    return np.asarray(idx)


def frame(seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ids = np.array(list(range(34)) + [40], dtype=np.uint8)
    segm = ids[((y // 3) * 7 + (x // 3) + seed) % len(ids)]           # every id of the table and 40, in every crop
    image = _textured(rng, H, W, 3, 255).astype(np.uint8)
    normal = _textured(rng, H, W, 3, 255).astype(np.uint8)
    win = val_window_sources()
    pose = np.zeros(H * W, dtype=np.uint8)
    pose.reshape(H, W)[2:30, 90:126] = 3                              # large, partly inside the val window
    pose.reshape(H, W)[50:62, 4:9] = 4                                # 60 pixels: never reaches 256, has no record
    pose[win[2:18, 4:20].reshape(-1)] = 1                             # exactly 256 transformed pixels
    pose[win[12:28, 30:46].reshape(-1)[:255]] = 2                     # exactly 255
    pose = pose.reshape(H, W)
    js = {str(k): {'class_id': 1, 'depth': 10.0, 'alpha': float(rng.uniform(-np.pi, np.pi))} for k in (1, 2, 3, 9)}
    inst8 = np.where(rng.random((H, W)) < 0.02, 0, pose).astype(np.uint8)   # precomputed: small ids, 0 = filled from the label
    inst16 = segm.astype(np.uint16)
    for k, v in ((1, 26001), (2, 26002), (3, 33005), (4, 33999)):
        inst16[pose == k] = v
    return dict(segm=segm, rgb=image, normalmap=normal, posemap=pose, inst8=inst8, inst16=inst16), js


def main():
    tv, tr = torchvision_stub()
    sys.modules['torchvision'] = tv
    sys.modules['torchvision.transforms'] = tr
    sys.path.insert(0, os.path.join(REF, 'textural'))
    from data import cityscapes_dataset as cd          # the reference module, as it lies
    from data import cityscapes_labels
    table = [0] * 34
    for lab in cityscapes_labels.labels:
        if 0 <= lab.id < 34:
            table[lab.id] = lab.trainId + 1 if lab.trainId != 255 else 0
    out = {'ncases': np.int64(len(CASES)), 'label_table': np.asarray(table, np.int64)}
    frames = [frame(100 + f) for f in range(len(NAMES))]
    for f, (src, js) in enumerate(frames):
        for k, a in src.items():
            out['f%d/%s' % (f, k)] = a
        out['f%d/json' % f] = np.asarray(json.dumps(js, sort_keys=True))
    for ci, over in enumerate(CASES):
        cfg = dict(BASE)
        cfg.update(over)
        tmp = tempfile.mkdtemp(prefix='cityscapes_loader_golden_')
        try:
            o = types.SimpleNamespace(**{k: v for k, v in cfg.items() if k not in ('segm_precomputed', 'inst_precomputed', 'files',
                                                                                    'items')})
            subset = 'train' if cfg['isTrain'] else 'val'
            o.dataroot = os.path.join(tmp, 'root')
            o.segm_precomputed_path = os.path.join(tmp, 'segm') if cfg['segm_precomputed'] else ''
            o.inst_precomputed_path = os.path.join(tmp, 'inst') if cfg['inst_precomputed'] else ''
            o.feat_pose = os.path.join(tmp, 'geo')
            o.feat_normal = os.path.join(tmp, 'geo')
            os.makedirs(os.path.join(o.dataroot, 'annotations'))
            with open(os.path.join(o.dataroot, 'annotations', 'instancesonly_gtFine_%s.json' % subset), 'w') as fh:
                json.dump({'images': [{'file_name': n + '_leftImg8bit.png', 'seg_file_name': n + '_gtFine_instanceIds.png'}
                                      for n in NAMES]}, fh)
            ds = cd.CustomDataset()
            with contextlib.redirect_stdout(io.StringIO()):
                ds.initialize(o)

            def put(path, arr, mode=None):
                os.makedirs(os.path.dirname(path), exist_ok=True)
                PIL.Image.fromarray(arr, mode).save(path)
            inst_mode = ''
            for i in range(len(NAMES)):
                f = NAMES.index(os.path.basename(ds.B_paths[i]).replace('_leftImg8bit.png', ''))
                src, js = frames[f]
                put(ds.A_paths[i], src['segm'], 'L')
                put(ds.B_paths[i], src['rgb'], 'RGB')
                if 'inst' in cfg['files']:
                    if cfg['inst_precomputed']:
                        put(ds.inst_paths[i], src['inst8'], 'L')
                    else:
                        put(ds.inst_paths[i], src['inst16'])
                        inst_mode = PIL.Image.open(ds.inst_paths[i]).mode
                if 'pose' in cfg['files']:
                    put(ds.pose_paths[i].replace('.json', '.png'), src['posemap'], 'L')
                    with open(ds.pose_paths[i], 'w') as fh:
                        json.dump(js, fh)
                if 'normal' in cfg['files']:
                    put(ds.normal_paths[i], src['normalmap'], 'RGB')
            p = 'c%d/' % ci
            out[p + 'cfg'] = np.asarray(json.dumps(cfg, sort_keys=True))
            out[p + 'inst_mode'] = np.asarray(inst_mode)
            random.seed(2000 + ci)
            real = cd.get_params
            for i in range(cfg['items']):
                drawn = {}

                def spy(opt, size):
                    q = real(opt, size)
                    drawn.update(q)
                    return q
                cd.get_params = spy
                try:
                    item = ds[i]
                finally:
                    cd.get_params = real
                q = p + 'i%d/' % i
                out[q + 'frame'] = np.int64(NAMES.index(os.path.basename(ds.B_paths[i]).replace('_leftImg8bit.png', '')))
                out[q + 'crop_pos'] = np.asarray([int(drawn['crop_pos'][0]), int(drawn['crop_pos'][1])], np.int64)
                out[q + 'flip'] = np.asarray(bool(drawn['flip']))
                for k in ('label', 'inst', 'image', 'pose', 'normal'):
                    v = item[k]
                    out[q + k] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
                print(ci, i, over, {k: (tuple(item[k].shape), str(item[k].dtype)) for k in ('label', 'inst', 'image', 'pose', 'normal')},
                      drawn, 'alias' if item['inst'] is item['label'] else '')
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, 'cityscapes_loader_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path))


if __name__ == '__main__':
    main()
