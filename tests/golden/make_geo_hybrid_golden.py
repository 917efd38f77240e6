#!/usr/bin/env python3
"""Generate tests/golden/geo_hybrid_golden.npz: the reference's geometric training items of every training set (VKitti,
KittiObject, KittiSemantics, CityscapesSemantics, CityscapesMaskRCNN) and its collate_fn over batches that mix them, EXECUTED
from their own source.

Made the way make_geo_train_golden.py is made (its torchvision stub, ColorJitter, hooks, spies and noting numpy are imported):
the classes are taken with `ast` from geometric/derender3d/datasets.py and collate_fn from data_loader.py, and run on small
synthetic PNG trees in a temporary directory (the *_ROOT_DIR variables point there; instance and disparity maps are 16-bit).
The class-level data frames (motgt_df, camera_df, scenegt_df) are set directly with the synthetic rows: parsing label files is
not what the fixture pins.  Name shims only: `collections.Mapping` (gone from Python) and, for CityscapesMaskRCNN, a read_rgb
whose array also has the `.width` / `.height` the class reads from it (np.asarray's result has neither).

Only data goes into the fixture: the frames, the item descriptions, the rois and parameters used, the collated dict of every
batch, the libm values.  Every case the tests rely on is asserted here.  Runs only where the reference exists."""
import ast
import collections.abc
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np
import pandas as pd
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_geo_train_golden as base      # noqa: E402  (also puts the product packages on sys.path)

REF = base.REF
DATASETS = base.DATASETS
LOADER = os.path.join(REF, 'geometric', 'derender3d', 'data_loader.py')
OUT = os.path.join(HERE, 'geo_hybrid_golden.npz')
Hooks = base.Hooks

VK, KO, KS, CS, MR = range(5)             # item kinds
KEYS = ('images', 'masks', 'ignores', 'rois', 'roi_norms', 'thetas', 'rotations', 'translations', 'translation2ds', 'scales',
        'log_scales', 'log_depths', 'widths', 'heights', 'focals', 'u0s', 'v0s', 'targets')
CITY, SEQ = 'aachen', '000000'


def reference_code(npx):
    names = ('Transforms', 'BaseDataset', 'VKitti', 'KittiBaseDataset', 'KittiObject', 'KittiSemantics', 'CityscapesBaseDataset',
             'CityscapesSemantics', 'CityscapesMaskRCNN')
    tree = ast.parse(open(DATASETS).read())
    classes = [st for st in tree.body if isinstance(st, ast.ClassDef) and st.name in names]
    assert [c.name for c in classes] == list(names)
    from derender3d import TargetType
    ns = {'torchvision': base.torchvision_stub(), 'torch': torch, 'np': npx, 'PIL': PIL, 'F': torch.nn.functional, 'os': os, 'pd': pd,
          'random': random, 'json': None, 'TargetType': TargetType, 'print': lambda *a, **k: None}
    exec(compile(ast.Module(body=classes, type_ignores=[]), DATASETS, 'exec'), ns)
    ltree = ast.parse(open(LOADER).read())
    (fn,) = [st for st in ltree.body if isinstance(st, ast.FunctionDef) and st.name == 'collate_fn']
    lns = {'torch': torch, 'np': np, 'collections': types.SimpleNamespace(Mapping=collections.abc.Mapping)}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), LOADER, 'exec'), lns)
    return ns, lns['collate_fn']


# ---------------------------------------------------------------------------------------------------- the synthetic frames
def smooth_rgb(H, W, seed):
    """ramps along x that change every twelve rows, and one flat patch: rows repeat, so the PNG and the npz stay small"""
    y, x = np.mgrid[0:H, 0:W]
    band = y // 12
    r = (8 * (x // 4) + 40 * band + 9 * seed) % 256
    g = (20 * (x // 8) + 17 * band + 5 * seed) % 256
    b = (30 * band + x // 16 * 8) % 256
    rgb = np.stack([r, g, b], axis=2).astype(np.uint8)
    rgb[H // 3:H // 2, W // 4:W // 2] = (250, 10 * seed % 256, 20)
    return np.ascontiguousarray(rgb)


def save16(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    PIL.Image.fromarray(arr.astype(np.uint16)).save(path)


def save_rgb(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    PIL.Image.fromarray(arr, 'RGB').save(path)


def cityscapes_frame(seed):
    """96 x 200: ids 26001 .. 26006 (cars) and a 24001 (not a car), the disparity cases of the issue"""
    H, W = 96, 200
    ids = np.full((H, W), 7, np.int32)
    disp = np.zeros((H, W), np.int32)
    y, x = np.mgrid[0:H, 0:W]
    disp[:] = (40 + x + 2 * y) * (((x // 8) + (y // 8)) % 3 != 0)          # background: small values with holes of 0
    ids[10:50, 20:70] = 26001                                              # smooth, above 255: lo != hi, fractional
    disp[10:50, 20:70] = (300 + x + 60 * y)[10:50, 20:70]
    ids[60:90, 5:45] = 26002                                               # no non-zero disparity under the mask
    disp[60:90, 5:45] = 0
    ids[5:40, 100:140] = 26003                                             # n == 1
    disp[5:40, 100:140] = 0
    disp[20, 120] = 4321
    ids[50:56, 90:94] = 26004                                              # 24 pixels, 22 non-zero: ranks 19 / 20 straddle a high byte
    vals = np.concatenate([np.arange(1, 20) * 12, [255, 700, 900], [0, 0]])
    disp[50:56, 90:94] = vals.reshape(6, 4)
    ids[60:96, 120:200] = 26005                                            # ties at the rank
    disp[60:96, 120:200] = np.where((x + y) % 4 == 0, 130, 500)[60:96, 120:200]
    ids[0:30, 160:200] = 26006                                             # touches the top and the right edge
    disp[0:30, 160:200] = (1000 + 50 * x - 3 * y)[0:30, 160:200]
    ids[70:80, 60:80] = 24001
    return smooth_rgb(H, W, seed), ids, disp


def kitti_ids(H, W):
    ids = np.zeros((H, W), np.int32)
    ids[4:44, 10:60] = 6601
    ids[8:44, 70:150] = 6602
    ids[0:10, 0:8] = 2600
    return ids


class Sized(np.ndarray):
    """np.asarray's result with the two attributes CityscapesMaskRCNN.__getitem__ reads from it (datasets.py:1104-1105)"""
    width = property(lambda self: self.shape[1])
    height = property(lambda self: self.shape[0])


# ---------------------------------------------------------------------------------------------------- the trees
def write_trees(tmp, ns):
    F = {}
    # VKITTI: the tree of make_geo_train_golden.py (64 x 320)
    vk = base.write_tree(os.path.join(tmp, 'vkitti'))
    for n in base.TRAIN_FRAMES + base.EVAL_FRAMES:
        F['vk%d' % n] = dict(rgb=vk[n][0], scene=vk[n][1])
    # KITTI object: two frames of different sizes
    for frame, (H, W) in ((0, (48, 160)), (1, (50, 156)), (6733, (48, 160))):
        rgb = smooth_rgb(H, W, 3 + frame % 7)
        save_rgb(os.path.join(tmp, 'kobj', 'training', 'image_2', '%06d.png' % frame), rgb)
        F['ko%d' % frame] = dict(rgb=rgb)
    # KITTI semantics
    for frame, (H, W) in ((0, (50, 156)), (1, (48, 160)), (180, (50, 156))):
        rgb, ids = smooth_rgb(H, W, 11 + frame % 5), kitti_ids(H, W)
        save_rgb(os.path.join(tmp, 'ksem', 'training', 'image_2', '%06d_10.png' % frame), rgb)
        save16(os.path.join(tmp, 'ksem', 'training', 'instance', '%06d_10.png' % frame), ids)
        F['ks%d' % frame] = dict(rgb=rgb, ids=ids)
    # Cityscapes
    for split, frame, seed in (('train', '000019', 1), ('val', '000020', 2), ('test', '000021', 3)):
        rgb, ids, disp = cityscapes_frame(seed)
        stem = '%s_%s_%s' % (CITY, SEQ, frame)
        save_rgb(os.path.join(tmp, 'city', 'images', 'leftImg8bit', split, CITY, stem + '_leftImg8bit.png'), rgb)
        save16(os.path.join(tmp, 'city', 'gtFine', split, CITY, stem + '_gtFine_instanceIds.png'), ids)
        save16(os.path.join(tmp, 'city', 'disparity', split, CITY, stem + '_disparity.png'), disp)
        det = (ids % 1000) * (ids >= 26000)                                # the detector's index image: 0 background, 1 .. 6
        save16(os.path.join(tmp, 'mrcnn', split, CITY, stem + '_leftImg8bit.png'), det)
        F['cs' + frame] = dict(rgb=rgb, ids=ids, disp=disp)
        F['mr' + frame] = dict(rgb=rgb, ids=det.astype(np.int32))
    return F


KO_ROWS = [   # region, frame, type, top, left, bottom, right, h, w, l, x, y, z, ry
    ('training', 0, 'Car', 10.37, 20.81, 44.62, 90.15, 1.5, 1.7, 4.1, -3.0, 1.6, 12.0, 0.3),
    ('training', 0, 'Van', 2.5, 100.49, 47.99, 159.2, 2.1, 1.9, 5.2, 2.5, 1.8, 6.0, 1.57),
    ('training', 1, 'Truck', 0.0, 0.75, 30.25, 60.5, 3.0, 2.4, 7.5, -9.0, 2.0, 30.0, -2.9),
    ('training', 1, 'Pedestrian', 5.0, 5.0, 30.0, 20.0, 1.8, 0.6, 0.8, 1.0, 1.6, 9.0, 0.0),
    ('validation', 6733, 'Car', 12.9, 33.3, 40.1, 95.7, 1.4, 1.6, 4.0, 1.0, 1.5, 15.0, -0.7),
]
KO_CAMERAS = {('training', 0): (721.5377, 609.5593, 172.854), ('training', 1): (707.0493, 604.0814, 180.5066),
              ('validation', 6733): (718.856, 607.1928, 185.2157)}
MR_CAMERAS = {'000019': (2262.52, 1096.98, 513.137), '000021': (2268.36, 1048.64, 519.277)}


def set_frames(ns, tmp):
    KittiObject, KittiSemantics = ns['KittiObject'], ns['KittiSemantics']
    rows = []
    for region, frame, typ, top, left, bottom, right, h, w, l, x, y, z, ry in KO_ROWS:
        rows.append(dict(type=typ, truncated=0.0, occluded=0, alpha=0.0, left=left, top=top, right=right, bottom=bottom, h=h, w=w,
                         l=l, x=x, y=y, z=z, ry=ry, score=1.0, region=region, frame=frame))
    KittiObject.motgt_df = pd.DataFrame(rows).set_index(['region', 'frame'])
    KittiObject.camera_df = pd.DataFrame([dict(focal=f, u0=u, v0=v, region=r, frame=n) for (r, n), (f, u, v) in KO_CAMERAS.items()]
                                         ).set_index(['region', 'frame'])
    KittiSemantics.scenegt_df = pd.DataFrame(
        [dict(region='training', frame=0, obj_index=6601, roi=[4, 10, 44, 60]), dict(region='training', frame=0, obj_index=6602, roi=[8, 70, 44, 150]),
         dict(region='training', frame=1, obj_index=6602, roi=[8, 70, 44, 150]), dict(region='validation', frame=180, obj_index=6601, roi=[4, 10, 44, 60]),
         dict(region='validation', frame=180, obj_index=6602, roi=[8, 70, 44, 150])]).set_index(['region', 'frame'])
    CB, CSem, MRC = ns['CityscapesBaseDataset'], ns['CityscapesSemantics'], ns['CityscapesMaskRCNN']
    CB.camera_df = pd.DataFrame([dict(split=s, city=CITY, seq=SEQ, frame=fr, f=MR_CAMERAS[fr][0], u0=MR_CAMERAS[fr][1], v0=MR_CAMERAS[fr][2])
                                 for s, fr in (('train', '000019'), ('test', '000021'))]).set_index(['split', 'city', 'seq', 'frame'])
    CSem.scenegt_df = pd.DataFrame([dict(split=s, city=CITY, seq=SEQ, frame=fr, obj_index=26000 + k)
                                    for s, fr in (('train', '000019'), ('val', '000020')) for k in range(1, 7)]
                                   ).set_index(['split', 'city', 'seq', 'frame'])
    boxes = {1: [10, 20, 50, 70], 3: [5, 100, 40, 140], 5: [60, 120, 96, 200], 6: [0, 160, 30, 200]}
    MRC.scenegt_df = pd.DataFrame([dict(split=s, city=CITY, seq=SEQ, frame=fr, obj_index=k, roi=roi)
                                   for s, fr in (('train', '000019'), ('test', '000021')) for k, roi in boxes.items()]
                                  ).set_index(['split', 'city', 'seq', 'frame'])
    real_read = CB.__dict__['read_rgb'].__func__
    MRC.read_rgb = staticmethod(lambda *a: np.ascontiguousarray(real_read(*a)).view(Sized))


# ---------------------------------------------------------------------------------------------------- the batches
# an item: (kind, frame key, selector, prescribed roi or None, prescribed jitter or None)
J = base.FACTORS
BATCHES = [
    ('vk', True, [(VK, 'vk0', 'Car:1', None, None), (VK, 'vk1', 'Van:3', (30, 30, 64, 286), ([1, 3, 0, 2], J[1], 37))]),
    ('ko', True, [(KO, 'ko0', 0, None, None), (KO, 'ko0', 1, None, ([2, 1], J[2], 0))]),
    ('ks', True, [(KS, 'ks0', 0, (-90, -40, 134, 150), ([3], J[3], 128)),        # s == 224, past the top, left and bottom edge
                  (KS, 'ks0', 1, (-100, -40, 156, 216), None),                   # s == 256, past all four edges
                  (KS, 'ks1', 2, (0, 10, 48, 310), ([0, 1, 2, 3], J[5], 200))]),  # s == 300, well past the right edge
    ('cs', True, [(CS, 'cs000019', 26001, None, None), (CS, 'cs000019', 26002, (58, 3, 93, 44), None),
                  (CS, 'cs000019', 26003, (5, 100, 40, 141), ([1], J[0], 0)), (CS, 'cs000019', 26004, None, ([3, 2], J[1], 255)),
                  (CS, 'cs000019', 26005, (60, 121, 96, 200), None),             # s - h = 43 odd against the bottom edge
                  (CS, 'cs000019', 26006, (0, 165, 30, 200), None),              # s - h = 5 odd ... the window leaves at the top
                  (CS, 'cs000019', 26005, (40, 151, 96, 200), None)]),           # s - w = 7 odd against the right edge
    ('ce', False, [(CS, 'cs000020', 26001, None, None), (CS, 'cs000020', 26004, None, None), (CS, 'cs000020', 26002, None, None)]),
    ('mr', False, [(MR, 'mr000021', 0, None, None), (MR, 'mr000021', 2, None, None)]),
    ('mt', True, [(MR, 'mr000019', 1, (-60, 20, 196, 200), None), (MR, 'mr000019', 3, None, None)]),
    ('vc', True, [(VK, 'vk0', 'Car:2', None, None), (CS, 'cs000019', 26001, None, None), (VK, 'vk2', 'Car:7', None, None)]),
    ('kk', True, [(KO, 'ko0', 0, None, None), (KS, 'ks1', 2, None, None), (KS, 'ks0', 0, (0, 0, 50, 41), None)]),
]


def datasets_for(ns, is_train):
    ds = {VK: ns['VKitti'](is_train=is_train), KO: ns['KittiObject'](is_train=is_train), KS: ns['KittiSemantics'](is_train=is_train),
          CS: ns['CityscapesSemantics'](is_train=is_train), MR: ns['CityscapesMaskRCNN'](is_train=is_train)}
    return ds


def index_of(ds, kind, key, sel):
    df = ds[kind].df
    if kind == VK:
        frame = int(key[2:])
        for i in range(len(df)):
            r = df.iloc[i]
            if int(r.name[2]) == frame and '%s:%d' % (r.orig_label, int(r.tid)) == sel:
                return i
    elif kind == KO:
        frame = int(key[2:])
        hits = [i for i in range(len(df)) if int(df.iloc[i].name[1]) == frame]
        return hits[sel if frame != 1 else 0] if frame != 6733 else hits[0]
    elif kind == KS:
        frame = int(key[2:])
        want = [6601, 6602, 6602][sel] if sel < 3 else None
        for i in range(len(df)):
            r = df.iloc[i]
            if int(r.name[1]) == frame and int(r.obj_index) == want:
                return i
    elif kind == CS:
        for i in range(len(df)):
            r = df.iloc[i]
            if r.name[3] == key[2:] and int(r.obj_index) == sel:
                return i
    else:
        hits = [i for i in range(len(df)) if df.iloc[i].name[3] == key[2:]]
        return hits[sel]
    raise KeyError((kind, key, sel))


def run_batch(tag, is_train, items, ns, collate, npx, F, out):
    ds = datasets_for(ns, is_train)
    B = len(items)
    kind = np.asarray([it[0] for it in items], np.int32)
    frame_keys = sorted({it[1] for it in items})
    data = np.zeros((B, 16), np.float64)     # KO: the 11 row values and (focal, u0, v0); KS / MR: the cached roi and the camera
    obj = np.zeros(B, np.int32)
    order = np.full((B, 4), -1, np.int32)
    nops, shifts = np.zeros(B, np.int32), np.zeros(B, np.int32)
    factors = np.ones((B, 3), np.float64)
    used, mask_rois = np.zeros((B, 4), np.int32), np.zeros((B, 4), np.int32)
    seeds = np.zeros(B, np.int64)
    drawn_roi, drawn_jitter = np.zeros(B, bool), np.zeros(B, bool)
    libm = np.full((B, 8), np.nan, np.float64)
    results = []
    for b, (k, key, sel, roi, jit) in enumerate(items):
        seeds[b] = 9000 + 17 * b + 1000 * len(out) % 7919
        random.seed(int(seeds[b]))
        Hooks.roi, Hooks.jitter = roi, jit
        Hooks.used_roi = Hooks.used_jitter = Hooks.mask_roi = None
        npx.noted = []
        i = index_of(ds, k, key, sel)
        res = ds[k][i]
        row = ds[k].df.iloc[i]
        if k == VK:
            names = list(out['%s_names' % key]) if '%s_names' % key in out else None
            if names is None:
                df = ns['VKitti'].motgt_df.loc[(base.WORLD, base.TOPIC, int(key[2:]))]
                names = [a + ':' + str(t) for a, t in zip(df.orig_label.values, df.tid.values)]
                out['%s_rows' % key] = np.stack([df[c].values.astype(np.float64) for c in base.ROW_KEYS], axis=1)
                out['%s_codes' % key] = np.asarray([base.COLOURS[x] for x in names], np.uint8)
                out['%s_names' % key] = np.asarray(names)
            obj[b] = names.index(sel)
            used[b] = Hooks.used_roi if is_train else Hooks.mask_roi
            mask_rois[b] = Hooks.mask_roi
            drawn_roi[b] = is_train and roi is None
        elif k == KO:
            cam = ns['KittiObject'].camera_df.loc[row.name]
            data[b, :14] = [row.top, row.left, row.bottom, row['right'], row.ry, row.l, row.h, row.w, row.x, row.y, row.z, cam.focal, cam.u0, cam.v0]
            used[b] = [int(row.top), int(row.left), int(row.bottom), int(row['right'])]
            assert Hooks.used_roi is None
        else:
            obj[b] = int(row.obj_index)
            if k in (KS, MR):
                data[b, :4] = row.roi
                mask_rois[b] = row.roi
                used[b] = Hooks.used_roi if is_train else row.roi
                if k == MR:
                    cam = ns['CityscapesBaseDataset'].camera_df.loc[row.name]
                    data[b, 4:7] = [cam.f, cam.u0, cam.v0]
            else:
                mask_rois[b] = Hooks.mask_roi
                used[b] = Hooks.used_roi if is_train else Hooks.mask_roi
            drawn_roi[b] = is_train and roi is None
        drawn_jitter[b] = is_train and jit is None
        if is_train:
            o, f, s = Hooks.used_jitter
            order[b, :len(o)], nops[b], factors[b], shifts[b] = o, len(o), f, s
        else:
            assert Hooks.used_jitter is None
        noted = [n for n, _ in npx.noted]
        if k == VK:
            assert noted == ['cos', 'sin', 'log', 'log', 'log', 'log'], noted
            libm[b] = np.concatenate([v for _, v in npx.noted])
        elif k == KO:
            assert noted == ['log', 'log', 'log', 'log'], noted
            libm[b, 2:] = np.concatenate([v for _, v in npx.noted])
        else:
            assert not noted
        res = {kk: (v if isinstance(v, torch.Tensor) else (np.asarray(v) if not isinstance(v, int) else v)) for kk, v in res.items()
               if kk not in ('image_masks', 'image_ignores')}
        results.append(res)
    keysets = [sorted(r.keys()) for r in results]
    col = collate([dict(r) for r in results])
    p = tag + '_'
    for kk, v in col.items():
        assert kk in KEYS, kk
        out[p + kk] = v.numpy()
        assert v.shape[0] == B
    out[p + 'keys'] = np.asarray(sorted(col.keys()))
    for b, ks in enumerate(keysets):
        out['%sitem%d_keys' % (p, b)] = np.asarray(ks)
    out[p + 'frame_keys'] = np.asarray(frame_keys)
    out[p + 'item_frame'] = np.asarray([frame_keys.index(it[1]) for it in items], np.int32)
    for kk, v in (('kind', kind), ('obj', obj), ('data', data), ('order', order), ('nops', nops), ('factors', factors), ('hue_shift', shifts),
                  ('rois_used', used), ('mask_rois', mask_rois), ('seeds', seeds), ('drawn_roi', drawn_roi), ('drawn_jitter', drawn_jitter),
                  ('libm', libm), ('is_train', np.asarray(is_train))):
        out[p + kk] = v
    return col


def main():
    tmp = tempfile.mkdtemp(prefix='geo_hybrid_golden_')
    out = {}
    try:
        for var, sub in (('VKITTI_ROOT_DIR', 'vkitti'), ('KITTI_OBJECT_ROOT_DIR', 'kobj'), ('KITTI_SEMANTICS_ROOT_DIR', 'ksem'),
                         ('KITTI_SEMANTICS_CACHE_DIR', 'ksem_cache'), ('CITYSCAPES_ROOT_DIR', 'city'), ('CITYSCAPES_SEMANTICS_CACHE_DIR', 'c'),
                         ('CITYSCAPES_MASKRCNN_ROOT_DIR', 'mrcnn'), ('CITYSCAPES_MASKRCNN_CACHE_DIR', 'mc')):
            os.environ[var] = os.path.join(tmp, sub)
        npx = base.NumpyNoting()
        ns, collate = reference_code(npx)
        base.install_spies(ns['Transforms'])
        F = write_trees(tmp, ns)
        set_frames(ns, tmp)
        VKitti = ns['VKitti']
        VKitti.worlds, VKitti.topics = [base.WORLD], [base.TOPIC]
        VKitti.train_frames, VKitti.test_frames = VKitti.train_frames[:1], VKitti.test_frames[:1]
        cols = {}
        for tag, is_train, items in BATCHES:
            cols[tag] = run_batch(tag, is_train, items, ns, collate, npx, F, out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    used_frames = sorted({str(k) for tag, _, _ in BATCHES for k in out[tag + '_frame_keys']})
    for key in used_frames:
        for part, arr in F[key].items():
            out['F_%s_%s' % (key, part)] = arr
    out['batches'] = np.asarray([t for t, _, _ in BATCHES])

    # ---- the cases the tests rely on
    from derender3d import scene as sc
    assert {tuple(F[k]['rgb'].shape[:2]) for k in used_frames} == {(96, 200), (48, 160), (50, 156), (64, 320)}
    assert len({tuple(F[str(k)]['rgb'].shape[:2]) for k in out['kk_frame_keys']}) >= 2 and len({tuple(F[str(k)]['rgb'].shape[:2]) for k in out['vc_frame_keys']}) == 2
    assert out['kk_kind'][0] == KO and 'masks' in out['kk_keys'] and not out['kk_masks'][0].any() and out['kk_masks'][1].any()
    assert 'masks' not in out['ko_keys'] and 'rois' not in out['ks_keys'] and 'rotations' in out['vc_keys'] and not out['vc_rotations'][1].any()
    assert sorted(set(out['vc_targets'].tolist())) == [2, 3] and sorted(set(out['kk_targets'].tolist())) == [1, 2]
    assert max(np.bincount(out['cs_item_frame'])) >= 2
    sides = []
    for tag, _, _ in BATCHES:
        r = out[tag + '_rois_used'].astype(np.int64)
        sides += np.maximum(r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]).tolist()
    assert 224 in sides and 256 in sides and min(sides) < 224 and max(sides) >= 290
    r = out['cs_rois_used'].astype(np.int64)
    h, w = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    s = np.maximum(h, w)
    y0, x0 = r[:, 0] - (s - h) // 2, r[:, 1] - (s - w) // 2
    quirk_row = np.flatnonzero(((s - h) % 2 == 1) & (y0 + s > 96))
    quirk_col = np.flatnonzero(((s - w) % 2 == 1) & (x0 + s > 200))
    assert quirk_row.size and quirk_col.size
    ig = out['cs_ignores']
    assert ig[quirk_row[0], 0, -1].max() == 0 and ig[quirk_col[0], 0, :, -1].max() == 0      # PIL's 0 row / column beside the 255 fill
    assert ig[quirk_row[0], 0, -4].min() == 1.0 or ig[quirk_row[0], 0, -6].min() == 1.0
    past = np.zeros(4, bool)                                     # rois past each edge of their OWN frame
    for t, _, _ in BATCHES:
        fk = [str(k) for k in out[t + '_frame_keys']]
        for b_, roi in enumerate(out[t + '_rois_used'].astype(np.int64)):
            Hf, Wf = F[fk[out[t + '_item_frame'][b_]]]['rgb'].shape[:2]
            past |= [roi[0] < 0, roi[1] < 0, roi[2] > Hf, roi[3] > Wf]
    assert past.all(), past
    d = out['ko_data']
    assert (d[:, :4] != np.floor(d[:, :4])).any()
    # disparity cases, from the frame itself
    ids, disp = F['cs000019']['ids'], F['cs000019']['disp']
    stats = {}
    for k in range(1, 7):
        v = np.sort(disp[(ids == 26000 + k) & (disp != 0)])
        n = v.size
        i = int(np.floor(0.95 * (n - 1))) if n else 0
        stats[k] = (n, int(v[i]) if n else 0, int(v[min(i + 1, n - 1)]) if n else 0)
        want = int(np.floor(np.percentile(v, 95))) if n else 0
        assert int(sc.percentile95_threshold([stats[k][0]], [stats[k][1]], [stats[k][2]])[0]) == want
    assert stats[2][0] == 0 and stats[3][0] == 1
    n1, lo1, hi1 = stats[1]
    assert lo1 != hi1 and ((n1 - 1) * 0.95) % 1 != 0 and lo1 > 255
    assert stats[4][1] >> 8 != stats[4][2] >> 8 and stats[4][0] == 22
    assert stats[5][1] == stats[5][2] == 500
    for t in ('vk', 'cs', 'vc', 'kk'):
        assert (out[t + '_drawn_roi'] | out[t + '_drawn_jitter']).any()
    assert (out['cs_rois_used'][out['cs_drawn_roi']] != out['cs_mask_rois'][out['cs_drawn_roi']]).any()
    assert not out['ce_nops'].any() and np.array_equal(out['ce_rois_used'], out['ce_mask_rois'])

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s: %d arrays, %.1f KiB' % (OUT, len(out), size / 1024))
    assert size <= os.path.getsize(os.path.join(HERE, 'geo_train_golden.npz')), 'the fixture must not outgrow geo_train_golden.npz'


if __name__ == '__main__':
    main()
