#!/usr/bin/env python3
"""Generate tests/golden/scene_golden.npz: the reference's geometric edit path up to the render, EXECUTED from its own source.

geometric/scripts/main.py and geometric/derender3d/datasets.py cannot be imported here (absl, chainer, bulb, pandas,
matplotlib, scipy, torchvision).  This script takes with `ast`, from where they lie,
  * datasets.py   class Transforms (:18-137; crop_square is :49-71) and class BaseDataset (:140-172: transform_ignore /
                  transform_mask / transform_rgb)
  * main.py `_test`  :342-355 (interests), :365-403 (crops, normalised rois, the encoder call), the body of
                  `if FLAGS.num_opts:` up to :421 (ignore maps and their crops), :461-514 (the edit)
and executes them on seeded scenes: `torchvision.transforms.functional` is the stub of make_loader_golden.py (torchvision
0.2.1's published behaviour on the real Pillow) extended by pad (ImageOps.expand), crop, resize, normalize, to_tensor and
to_pil_image; `.cuda()` is the identity; `model.module.derenderer` is a seeded stand-in for the encoder's outputs.
Only data goes into the fixture: frames, masks, rois, the crops, the ignore maps, the matched pairs, the edited blob rows,
interests and the values the host's float32 log / cos / sin returned for the operations.  Every case the tests rely on is asserted here.  Runs only where the reference exists.
"""
import ast
import copy
import json
import os
import sys
import types

import numpy as np
import PIL.Image
import PIL.ImageOps
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
DATASETS = os.path.join(REF, 'geometric', 'derender3d', 'datasets.py')
MAIN = os.path.join(REF, 'geometric', 'scripts', 'main.py')
OUT = os.path.join(HERE, 'scene_golden.npz')


def functional_stub():
    from make_loader_golden import torchvision_stub
    tv, tr = torchvision_stub()
    fn = types.ModuleType('torchvision.transforms.functional')
    to_tensor_cls, normalize_cls = tr.ToTensor, tr.Normalize

    def pad(img, padding, fill=0, padding_mode='constant'):
        return PIL.ImageOps.expand(img, border=padding, fill=fill)

    def crop(img, i, j, h, w):
        return img.crop((j, i, j + w, i + h))

    def resize(img, size, interpolation=PIL.Image.BILINEAR):
        return img.resize(tuple(size[::-1]), interpolation)

    def normalize(tensor, mean, std):
        return normalize_cls(mean, std)(tensor)

    def to_tensor(pic):
        return to_tensor_cls()(pic)

    def to_pil_image(pic, mode=None):
        assert isinstance(pic, np.ndarray) and pic.dtype == np.uint8 and pic.ndim == 3, 'only the forms the crop path uses'
        if pic.shape[2] == 1:
            return PIL.Image.fromarray(pic[:, :, 0], 'L')
        assert pic.shape[2] == 3
        return PIL.Image.fromarray(pic, 'RGB')

    fn.pad, fn.crop, fn.resize, fn.normalize, fn.to_tensor, fn.to_pil_image = pad, crop, resize, normalize, to_tensor, to_pil_image
    tr.functional = fn
    return tv


def reference_classes():
    """class Transforms and class BaseDataset of datasets.py, executed on the stub"""
    src = open(DATASETS).read()
    tree = ast.parse(src)
    classes = [st for st in tree.body if isinstance(st, ast.ClassDef) and st.name in ('Transforms', 'BaseDataset')]
    assert [c.name for c in classes] == ['Transforms', 'BaseDataset']
    ns = {'torchvision': functional_stub(), 'torch': torch, 'np': np, 'PIL': PIL, 'F': torch.nn.functional}
    exec(compile(ast.Module(body=classes, type_ignores=[]), DATASETS, 'exec'), ns)
    return ns['Transforms'], ns['BaseDataset']


def test_blocks():
    """the statements of main.py's `_test` by line range"""
    src = open(MAIN).read()
    tree = ast.parse(src)
    (fn,) = [st for st in tree.body if isinstance(st, ast.FunctionDef) and st.name == '_test']

    def take(body, first, last, opens):
        sts = [st for st in body if first <= st.lineno and st.end_lineno <= last]
        assert sts and sts[0].lineno == first and sts[-1].end_lineno == last, (first, last, sts[0].lineno, sts[-1].end_lineno)
        assert ast.get_source_segment(src, sts[0]).startswith(opens), ast.get_source_segment(src, sts[0])
        return compile(ast.Module(body=sts, type_ignores=[]), MAIN, 'exec')

    (opt_if,) = [st for st in fn.body if isinstance(st, ast.If) and st.lineno == 405]
    assert ast.get_source_segment(src, opt_if.test) == 'FLAGS.num_opts'
    return {
        'interests': take(fn.body, 342, 355, 'num_objs = len(class_ids)'),
        'crops': take(fn.body, 365, 403, 'rgbs = []'),
        'ignores': take(opt_if.body, 406, 421, 'if image_ignores is None:'),
        'edit': take(fn.body, 461, 514, 'if operations is not None and operations:'),
    }


def blocky(rng, H, W, cell=8):
    a = rng.integers(0, 256, ((H + cell - 1) // cell, (W + cell - 1) // cell, 3), dtype=np.uint8)
    return np.ascontiguousarray(a.repeat(cell, 0).repeat(cell, 1)[:H, :W])


def box_masks(H, W, rois, shrink):
    """one binary mask per roi: the roi clipped to the frame, shrunk by `shrink[n]` pixels per side (overlaps stay)"""
    m = np.zeros((len(rois), 1, H, W), np.float32)
    for n, (y0, x0, y1, x1) in enumerate(rois):
        k = shrink[n]
        m[n, 0, max(0, y0 + k):min(H, y1 - k), max(0, x0 + k):min(W, x1 - k)] = 1.0
    return m


SCENE_A = dict(
    H=150, W=1000, camera=(725.0, 499.5, 74.5), seed=11, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225],
    rois=[
        [40, 100, 80, 400],     # 0 wider than tall, s = 300 (above both sizes); the window leaves the frame at the top and bottom
        [50, 600, 87, 630],     # 1 s = 37 (below both sizes), s - w odd inside the frame
        [5, 500, 135, 560],     # 2 taller than wide, s = 130
        [60, 975, 90, 1000],    # 3 s - w = 5 odd, reaches past the right edge: the 0 column
        [120, 300, 150, 341],   # 4 s - h = 11 odd, reaches past the bottom edge: the 0 row
        [30, 0, 130, 10],       # 5 the window leaves the frame on the left (fill)
        [0, 700, 150, 924],     # 6 s = 224 = the image size; leaves the frame at the top (fill)
        [10, 650, 140, 906],    # 7 s = 256 = the mask size
        [20, 30, 130, 980],     # 8 s = 950 > 4 x 224
    ],
    class_ids=[1, 2, 1, 1, 3, 1, 2, 1, 1], shrink=[2, 3, 4, 1, 2, 0, 20, 30, 40],
    log_depths=[2.0, 0.5, 3.1, -0.4, 1.2, 4.0, 0.9, 2.6, 1.7],
    operations=[
        [],
        [{'type': 'delete', 'from': {'u': 250, 'v': 60}}],
        [{'type': 'modify', 'from': {'u': 530, 'v': 70}, 'to': {'u': 560.5, 'v': 64}, 'zoom': 1.3, 'ry': 0.4}],
        [{'type': 'modify', 'from': {'u': 615, 'v': 68}, 'to': {}, 'zoom': 0.8, 'ry': -1.1}],
        [{'type': 'modify', 'from': {'u': 810, 'v': 75}, 'to': {'u': 700}, 'zoom': 1.5, 'ry': 0.25},
         {'type': 'modify', 'from': {'u': 814, 'v': 76}, 'to': {'v': 90}, 'zoom': 0.9, 'ry': 0.6},
         {'type': 'delete', 'from': {'u': 987, 'v': 75}}],
    ])
SCENE_B = dict(
    H=60, W=90, camera=(90.0, 44.5, 29.5), seed=12, mean=[0.5, 0.5, 0.5], std=[0.25, 0.25, 0.25],
    rois=[[10, 5, 50, 45], [20, 40, 45, 85]], class_ids=[1, 1], shrink=[3, 2], log_depths=[1.0, 0.2],
    supplied_ignores=True,
    operations=[
        # more operations than objects: every OBJECT takes its nearest operation (main.py:474-476)
        [{'type': 'modify', 'from': {'u': 24, 'v': 31}, 'to': {'u': 30, 'v': 28}, 'zoom': 1.1, 'ry': 0.3},
         {'type': 'delete', 'from': {'u': 80, 'v': 50}},
         {'type': 'modify', 'from': {'u': 63, 'v': 33}, 'to': {'u': 60}, 'zoom': 1.2, 'ry': -0.2}],
        [],
    ])


class Recorder:
    """`torch` for the edit block: every attribute is torch's; log / cos / sin also note what they returned"""

    def __init__(self):
        self.values = []

    def __getattr__(self, name):
        fn = getattr(torch, name)
        if name not in ('log', 'cos', 'sin'):
            return fn

        def noted(x):
            y = fn(x)
            self.values.append((name, float(y)))
            return y
        return noted


def run_scene(tag, cfg, blocks, dataset, out):
    rng = np.random.default_rng(cfg['seed'])
    H, W, N = cfg['H'], cfg['W'], len(cfg['rois'])
    image_rgb = blocky(rng, H, W)
    rois = np.asarray(cfg['rois'], np.int32)
    image_masks = box_masks(H, W, cfg['rois'], cfg['shrink'])
    dataset.mean, dataset.std = cfg['mean'], cfg['std']
    dataset.Camera = types.SimpleNamespace(focal=cfg['camera'][0], u0=cfg['camera'][1], v0=cfg['camera'][2])
    # the seeded stand-in of the encoder (derender3d/models/derenderer.py:39-54: six keys)
    g = torch.Generator().manual_seed(cfg['seed'])
    delta = torch.randn(N, 2, generator=g)
    encoded = {'_theta_deltas': delta / torch.norm(delta, p=2, dim=1, keepdim=True),
               '_translation2ds': 0.1 * torch.randn(N, 2, generator=g),
               '_log_scales': 0.1 * torch.randn(N, 3, generator=g),
               '_log_depths': torch.tensor(cfg['log_depths'], dtype=torch.float32).reshape(N, 1)}
    seen = {}

    def derenderer(rgbs, mroi, droi):
        seen['rgbs'] = rgbs
        return {k: v.clone() for k, v in encoded.items()}

    supplied = None
    if cfg.get('supplied_ignores'):
        supplied = (rng.random((N, 1, H // 6 + 1, W // 6 + 1)) < 0.4).astype(np.float32).repeat(6, 2).repeat(6, 3)[:, :, :H, :W]
        supplied = np.ascontiguousarray(supplied)
    ns = {'torch': torch, 'np': np, 'PIL': PIL, 'os': os, 'to_numpy': lambda v: v.detach().cpu().numpy(), 'dataset': dataset,
          'FLAGS': types.SimpleNamespace(render_size=384, num_opts=1), 'print': lambda *a, **k: None,
          'model': types.SimpleNamespace(module=types.SimpleNamespace(derenderer=derenderer)),
          'image_rgb': image_rgb, 'class_ids': list(cfg['class_ids']), 'image_masks': image_masks, 'rois': rois,
          'image_ignores': supplied, 'all_interested': False, 'height': H, 'width': W}
    exec(blocks['interests'], ns)
    exec(blocks['crops'], ns)
    exec(blocks['ignores'], ns)
    p = tag + '_'
    out[p + 'image'] = image_rgb
    out[p + 'image_masks'] = image_masks.astype(np.uint8)
    out[p + 'rois'] = rois
    out[p + 'class_ids'] = np.asarray(cfg['class_ids'], np.int32)
    out[p + 'camera'] = np.asarray(cfg['camera'], np.float64)
    out[p + 'mean'], out[p + 'std'] = np.asarray(cfg['mean'], np.float64), np.asarray(cfg['std'], np.float64)
    out[p + 'interests'] = ns['interests'].numpy().astype(np.uint8)
    out[p + 'rgbs'] = ns['rgbs'].numpy()
    out[p + 'masks'] = ns['masks'].numpy()
    out[p + 'ignores'] = ns['ignores'].numpy()
    out[p + 'image_ignores'] = ns['image_ignores'].numpy().astype(np.uint8)
    out[p + 'supplied_ignores'] = np.asarray(supplied is not None)
    for k in ('_roi_norms', '_mroi_norms', '_droi_norms'):
        out[p + 'blob' + k] = ns['_blob'][k].numpy()
    for k, v in encoded.items():
        out[p + 'blob' + k] = v.numpy()
    assert set(np.unique(ns['image_ignores'].numpy())) <= {0.0, 1.0}
    if supplied is None:
        out[p + 'order'] = ns['index'].numpy().astype(np.int32)
    # ---- the edit, per operation list, each on a fresh copy of the blob (the block edits `.detach()` views in place)
    out[p + 'operations'] = np.asarray(json.dumps(cfg['operations']))
    blob0 = {k: v.clone() for k, v in ns['_blob'].items()}
    for f, operations in enumerate(cfg['operations']):
        e = dict(ns)
        e['_blob'] = {k: v.clone() for k, v in blob0.items()}
        e['interests'] = ns['interests'].clone()
        e['operations'] = copy.deepcopy(operations)
        e.pop('indices', None)
        rec = Recorder()
        e['torch'] = rec
        exec(blocks['edit'], e)
        pairs = [(int(a), int(b)) for a, b in e.get('indices', [])]
        q = '%sedit%d_' % (p, f)
        out[q + 'pairs'] = np.asarray(pairs, np.int32).reshape(-1, 2)
        out[q + 'theta_deltas'] = e['_blob']['_theta_deltas'].numpy()
        out[q + 'translation2ds'] = e['_blob']['_translation2ds'].numpy()
        out[q + 'log_depths'] = e['_blob']['_log_depths'].numpy()
        out[q + 'interests'] = e['interests'].numpy().astype(np.uint8)
        # what torch.log(tensor(zoom)), torch.cos(tensor(-ry)), torch.sin(tensor(-ry)) returned HERE, per `modify` pair in
        # iteration order: float32 transcendental functions differ in the last place between hosts (vector math libraries)
        assert len(rec.values) % 3 == 0 and [n for n, _ in rec.values] == ['log', 'cos', 'sin'] * (len(rec.values) // 3)
        out[q + 'transcendentals'] = np.asarray([v for _, v in rec.values], np.float32).reshape(-1, 3)
    return ns, seen


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # the identity: everything below is host arithmetic
    Transforms, BaseDataset = reference_classes()
    blocks = test_blocks()
    dataset = BaseDataset()
    dataset.is_train = False
    out = {}

    # ---- the padding quirk on the issue's own example (frame 20 x 30 of value 200, fill 77 -> 200 x 9, 77, 0)
    row = np.asarray(Transforms.crop_square(PIL.Image.new('L', (30, 20), 200), [2, 22, 13, 30], fill=77))[0]
    assert row.tolist() == [200] * 9 + [77, 0], row

    nsa, _ = run_scene('a', SCENE_A, blocks, dataset, out)
    nsb, _ = run_scene('b', SCENE_B, blocks, dataset, out)

    # ---- the cases the tests rely on
    ra = np.asarray(SCENE_A['rois'])
    h, w = ra[:, 2] - ra[:, 0], ra[:, 3] - ra[:, 1]
    s = np.maximum(h, w)
    assert (w > h).any() and (h > w).any()
    assert (ra[:, 1] - (s - w) // 2 < 0).any() and (ra[:, 0] - (s - h) // 2 < 0).any()
    assert (((s - w) % 2 == 1) & (ra[:, 1] - (s - w) // 2 + s > SCENE_A['W'])).any()
    assert (((s - h) % 2 == 1) & (ra[:, 0] - (s - h) // 2 + s > SCENE_A['H'])).any()
    assert (s < 224).any() and (s == 224).any() and (s == 256).any() and (s > 256).any() and (s > 4 * 224).any()
    ig = out['a_ignores']
    assert ig[3, 0, :, -1].max() == 0 and ig[3, 0, :, 238].min() == 1.0    # object 3: PIL's 0 column beside the 255 fill
    assert ig[4, 0, -1].max() == 0 and ig[4, 0, 230].min() == 1.0          # object 4: the 0 row under the 255 fill
    order = out['a_order']
    assert sorted(order.tolist()) == list(range(len(ra))) and order.tolist() != list(range(len(ra)))
    assert len(set(SCENE_A['log_depths'])) == len(ra)
    assert (out['a_image_masks'].sum(0) > 1).any()                   # overlapping masks
    assert out['a_image_ignores'][1:].any() and not out['a_image_ignores'][0].any()
    ints = out['a_interests']
    assert ints.any() and not ints.all()                             # a class outside {1, 2} and a small mask
    assert bool(out['b_supplied_ignores']) and 0.0 < out['b_ignores'].mean() < 1.0
    pa = [out['a_edit%d_pairs' % f] for f in range(5)]
    assert pa[0].shape == (0, 2) and pa[1].shape == (1, 2) and out['a_edit1_interests'].sum() == ints.sum() - 1
    assert len(set(pa[4][:, 0].tolist())) < len(pa[4])               # two operations on one object
    assert not np.array_equal(out['a_edit3_translation2ds'], out['a_blob_translation2ds'])
    pb = out['b_edit0_pairs']
    assert len(pb) == 2 and len(SCENE_B['operations'][0]) == 3       # the other matching branch

    np.savez_compressed(OUT, **out)
    print('wrote %s: %d arrays, %.1f KiB' % (OUT, len(out), os.path.getsize(OUT) / 1024))


if __name__ == '__main__':
    main()
