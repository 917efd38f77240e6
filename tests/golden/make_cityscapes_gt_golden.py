#!/usr/bin/env python3
"""Generate tests/golden/cityscapes_gt_golden.npz: the reference's `--dataset cityscapes --source gt` path from the instance-id
map and the disparity map to (class_ids, image_masks, image_ignores, rois), EXECUTED from its own source.

geometric/scripts/main.py and geometric/derender3d/datasets.py cannot be imported here (absl, chainer, pandas ...).  This script
takes with `ast`, from where they lie,
  * datasets.py  Transforms.scene_to_mask (:75-76), Transforms.mask_to_roi (:95-103), CityscapesSemantics.Category and
                 CityscapesSemantics.index2cat (:844-849)
  * main.py      :764-795 (the reads, the loop over np.unique(image_scene), the stacks) and :812-818 (the 16 largest)
and executes them on synthetic frames (no Cityscapes data exists here): `dataset.read_scene` / `read_disparity` hand out the
frame as the reference's readers do, [H, W, 1]; `np` is numpy with the alias `np.bool` the reference's numpy 1.14 still had,
and its `percentile` also notes what it returned.

Only data goes into the fixture: the maps as uint16, the ids, rois, areas, the binary planes through np.packbits, the
selection, the percentiles and, per object, the row sdn_scene_id_stats must produce (lo and hi read from np.sort of the values).
Every case the tests rely on is asserted here.  Runs only where the reference exists."""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_detections_golden import DATASETS, MAIN, function_of, statements_of  # noqa: E402

OUT = os.path.join(HERE, 'cityscapes_gt_golden.npz')
CAR = 26


class Numpy114:
    """numpy with `np.bool` (removed since) and a percentile that records its results"""

    def __init__(self):
        self.bool = bool
        self.percentiles = []

    def __getattr__(self, name):
        return getattr(np, name)

    def percentile(self, a, q, *args, **kwargs):
        assert q == 95 and not args and not kwargs
        v = np.percentile(a, q)
        self.percentiles.append(float(v))
        return v


def reference():
    ns_tr = {'np': np}
    exec(function_of(DATASETS, 'scene_to_mask', cls='Transforms'), ns_tr)
    exec(function_of(DATASETS, 'mask_to_roi', cls='Transforms'), ns_tr)
    src = open(DATASETS).read()
    (cls,) = [st for st in ast.parse(src).body if isinstance(st, ast.ClassDef) and st.name == 'CityscapesSemantics']
    (cat,) = [st for st in cls.body if isinstance(st, ast.ClassDef) and st.name == 'Category']
    ns_ds = {}
    exec(compile(ast.Module(body=[cat], type_ignores=[]), DATASETS, 'exec'), ns_ds)
    exec(function_of(DATASETS, 'index2cat', cls='CityscapesSemantics'), ns_ds)
    assert ns_ds['Category'].car == CAR and ns_ds['index2cat'](26999) == 26 and ns_ds['index2cat'](26) == 0
    transforms = types.SimpleNamespace(scene_to_mask=ns_tr['scene_to_mask'], mask_to_roi=ns_tr['mask_to_roi'])
    loop = statements_of(MAIN, 764, 795, 'image_scene = dataset.read_scene(split, city, seq, frame)')
    select = statements_of(MAIN, 812, 818, 'sels = np.flipud(np.argsort(')
    return transforms, ns_ds, loop, select


def run_case(tag, scene, disparity, ref, out):
    transforms, ns_ds, loop, select = ref
    assert scene.dtype == np.uint16 and disparity.dtype == np.uint16 and scene.shape == disparity.shape
    np114 = Numpy114()
    dataset = types.SimpleNamespace(read_scene=lambda *a: scene[..., None], read_disparity=lambda *a: disparity[..., None],
                                    index2cat=ns_ds['index2cat'], Category=ns_ds['Category'])
    ns = {'np': np114, 'Transforms': transforms, 'dataset': dataset, 'split': 'val', 'city': 'x', 'seq': '0', 'frame': '0',
          'class_ids': [], 'image_masks': [], 'image_ignores': [], 'rois': []}
    exec(loop, ns)
    masks, ignores, rois = ns['image_masks'], ns['image_ignores'], ns['rois']
    H, W = scene.shape
    K = masks.shape[0]
    assert masks.shape == ignores.shape == (K, 1, H, W) and masks.dtype == ignores.dtype == np.float32 and rois.shape == (K, 4)
    assert ns['class_ids'].tolist() == [1] * K
    assert set(np.unique(masks)) <= {0.0, 1.0} and set(np.unique(ignores)) <= {0.0, 1.0}
    ids = np.asarray([i for i in np.unique(scene) if i // 1000 == CAR], np.int32)
    assert len(ids) == K
    # the row of sdn_scene_id_stats per object, lo and hi from a sort; the percentiles in loop order (none where n == 0)
    stats = np.zeros((K, 8), np.int32)
    pcs = np.zeros(K, np.float64)
    noted = iter(np114.percentiles)
    for k in range(K):
        m = masks[k, 0] > 0
        assert np.array_equal(m, scene == ids[k])
        d = np.sort(disparity[m][disparity[m] != 0].astype(np.int64))
        n = d.size
        stats[k, 0], stats[k, 1:5], stats[k, 5] = m.sum(), rois[k], n
        if n:
            i = int(np.floor((n - 1) * 0.95))
            stats[k, 6], stats[k, 7] = d[i], d[min(i + 1, n - 1)]
            pcs[k] = next(noted)
        assert np.array_equal(ignores[k, 0] > 0, disparity > pcs[k])
    assert next(noted, None) is None
    p = tag + '_'
    out[p + 'scene'], out[p + 'disparity'] = scene, disparity
    out[p + 'ids'], out[p + 'rois'], out[p + 'areas'] = ids, rois.astype(np.int32), masks.sum(axis=(1, 2, 3)).astype(np.int32)
    out[p + 'stats'], out[p + 'percentiles'] = stats, pcs
    out[p + 'masks_bits'] = np.packbits(masks.astype(np.uint8))
    out[p + 'ignores_bits'] = np.packbits(ignores.astype(np.uint8))
    exec(select, ns)
    sels = np.asarray(ns['sels'], np.int32)
    out[p + 'sels'] = sels
    assert np.array_equal(ns['image_masks'], masks[sels]) and np.array_equal(ns['image_ignores'], ignores[sels])
    assert np.array_equal(ns['rois'], rois[sels]) and len(sels) == min(K, 16)
    return dict(ids=ids, stats=stats, pcs=pcs, sels=sels, masks=masks, ignores=ignores)


def plant(scene, disparity, rng, car_id, region, values=None):
    """paint `car_id` over the boolean region; its disparities are `values` in a seeded order (None: leave what is there)"""
    scene[region] = car_id
    if values is not None:
        values = np.asarray(values)
        assert values.size == int(region.sum()), (car_id, values.size, int(region.sum()))
        disparity[region] = rng.permutation(values).astype(np.uint16)


def rect(shape, y0, x0, h, w):
    m = np.zeros(shape, bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def others(scene):
    """ids that are not cars, on both sides of the range, and a car without an instance number"""
    H, W = scene.shape
    scene[H - 1, 0:3] = (26, 25999, 27000)
    scene[H - 1, 3:6] = (24001, 27999, 26)
    scene[H - 2, 0] = 0


def frame_a(rng):
    """37 x 70, one car: a cross that touches all four borders"""
    H, W = 37, 70
    scene = np.full((H, W), 7, np.uint16)
    disparity = rng.integers(0, 4000, (H, W)).astype(np.uint16)
    others(scene)
    region = rect((H, W), 17, 0, 3, W) | rect((H, W), 0, 33, H, 4) | rect((H, W), 10, 20, 15, 30)
    plant(scene, disparity, rng, 26000, region)
    disparity[region & (rng.random((H, W)) < 0.1)] = 0
    return scene, disparity


def frame_b(rng):
    """37 x 70, three cars: 26000, 26500 and 26999; ranks i and i + 1 in different high-byte bins"""
    H, W = 37, 70
    scene = np.zeros((H, W), np.uint16)
    disparity = rng.integers(0, 700, (H, W)).astype(np.uint16)
    others(scene)
    # n = 40: i = 37, i + 1 = 38 -> sorted[37] = 255, sorted[38] = 256
    plant(scene, disparity, rng, 26000, rect((H, W), 2, 3, 5, 8), list(rng.integers(1, 256, 37)) + [255, 256, 300])
    # n = 60: i = 56 -> 0x01FF, 0x0200
    plant(scene, disparity, rng, 26999, rect((H, W), 10, 41, 6, 10), list(rng.integers(1, 0x200, 56)) + [0x1FF, 0x200, 0x200, 0x7000])
    # 65535 at both ranks, and zeros that do not count: 90 pixels, 20 of them 0 -> n = 70, i = 65
    plant(scene, disparity, rng, 26500, rect((H, W), 20, 1, 9, 10), [0] * 20 + list(rng.integers(60000, 65535, 60)) + [65535] * 10)
    return scene, disparity


def frame_c(rng):
    """64 x 128, 33 cars in cells of 12 x 16 pixels (five rows of eight), the planted objects first"""
    H, W = 64, 128
    scene = np.full((H, W), 11, np.uint16)
    disparity = rng.integers(0, 20000, (H, W)).astype(np.uint16)
    others(scene)
    scene[H - 3, :] = 24017

    def cell(c, h=12, w=16, dy=0, dx=0):
        return rect((H, W), 12 * (c // 8) + dy, 16 * (c % 8) + dx, h, w)

    def around(level, n):
        return np.clip(level + rng.normal(0, 40, n), 1, 65535).astype(np.int64)

    plant(scene, disparity, rng, 26000, cell(0, 5, 6), [0] * 30)                               # n = 0: ignore = disparity > 0
    plant(scene, disparity, rng, 26001, cell(1, 4, 5), [0] * 19 + [777])                       # n = 1
    plant(scene, disparity, rng, 26002, cell(2, 3, 4), [0] * 10 + [500, 900])                  # n = 2: t = 900 - 400 * 0.05
    plant(scene, disparity, rng, 26003, cell(3, 3, 7), around(3000, 21))                       # n = 21: (n - 1) 0.95 = 19
    plant(scene, disparity, rng, 26004, cell(4, 1, 41 - 25, dy=11) | cell(4, 5, 5), around(9000, 41))   # n = 41
    plant(scene, disparity, rng, 26005, cell(5, 6, 9), [4242] * 54)                            # all values equal
    # lo != hi with an integral percentile: n = 11, g = 0.5, hi - lo = 2 -> lo + 1 exactly
    plant(scene, disparity, rng, 26006, cell(6, 1, 11), list(rng.integers(100, 1000, 9)) + [1000, 1002])
    # ... and one whose g = frac(21 * 0.95) is not exact in binary: n = 22, hi - lo = 20 -> lo + 19 in exact arithmetic
    plant(scene, disparity, rng, 26007, cell(7, 2, 11), list(rng.integers(100, 2000, 19)) + [2000, 2020, 2500])
    plant(scene, disparity, rng, 26008, cell(8), around(12000, 192))                           # two cars of equal area
    plant(scene, disparity, rng, 26009, cell(9), around(15000, 192))
    plant(scene, disparity, rng, 26010, cell(10) | cell(33) | cell(34), around(700, 576))      # above 16 x 16 pixels: interesting
    plant(scene, disparity, rng, 26011, cell(11) | cell(35) | cell(36, 12, 9), around(40000, 492))
    used = {(5, 6), (4, 5), (3, 4), (3, 7), (1, 41), (6, 9), (1, 11), (2, 11), (12, 16)}
    for c in range(12, 33):
        while True:
            h, w = int(rng.integers(2, 13)), int(rng.integers(2, 17))
            if (h, w) not in used and all(h * w != a * b for a, b in used):
                break
        used.add((h, w))
        region = cell(c, h, w)
        plant(scene, disparity, rng, 26000 + (999 if c == 32 else c * 7), region, around(int(rng.integers(300, 30000)), h * w))
        disparity[region & (rng.random((H, W)) < 0.15)] = 0
    return scene, disparity


def main():
    ref = reference()
    out = {}
    rng = np.random.default_rng(2026)
    a = run_case('a', *frame_a(rng), ref, out)
    b = run_case('b', *frame_b(rng), ref, out)
    c = run_case('c', *frame_c(rng), ref, out)

    # ---- the cases the tests rely on
    for tag in 'abc':
        present = set(np.unique(out[tag + '_scene']).tolist())
        assert {26, 25999, 27000, 24001, 27999, 0} <= present, tag
    assert len(a['ids']) == 1 and out['a_rois'].tolist() == [[0, 0, 37, 70]]                   # touches all four borders
    assert b['ids'].tolist() == [26000, 26500, 26999]
    assert b['stats'][0, 5:].tolist() == [40, 255, 256] and b['stats'][2, 5:].tolist() == [60, 0x1FF, 0x200]
    assert b['stats'][1, 5:].tolist() == [70, 65535, 65535] and out['b_areas'][1] == 90
    K = len(c['ids'])
    assert K == 33 and len(c['sels']) == 16 and c['ids'][-1] == 26999 and c['ids'][0] == 26000
    s = c['stats']
    assert s[0, 5:].tolist() == [0, 0, 0] and c['pcs'][0] == 0 and np.array_equal(c['ignores'][0, 0] > 0, out['c_disparity'] > 0)
    assert s[1, 5:].tolist() == [1, 777, 777] and s[2, 5:].tolist() == [2, 500, 900]
    assert s[3, 5] == 21 and s[4, 5] == 41 and s[5, 5:].tolist() == [54, 4242, 4242]
    assert s[6, 5:].tolist() == [11, 1000, 1002] and c['pcs'][6] == 1001.0
    assert s[7, 5:].tolist() == [22, 2000, 2020] and abs(c['pcs'][7] - 2019.0) < 1e-9
    integral = [k for k in range(K) if s[k, 6] != s[k, 7] and c['pcs'][k] == np.floor(c['pcs'][k])]
    assert 6 in integral
    areas = out['c_areas']
    assert areas[8] == areas[9] == 192 and 8 in c['sels'] and 9 in c['sels']                   # the tie is inside the selection
    assert sorted(areas.tolist()).count(192) == 2 and len(set(areas.tolist())) == K - 1
    assert (areas > 256).sum() == 2 and (areas[c['sels']] <= 256).any()
    assert (s[:, 5] < s[:, 0]).sum() > 5                                                       # zeros under many masks

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 400000, size
    print('wrote %s: %d arrays, %.1f KiB; integral percentiles with lo != hi: objects %s of case c' % (OUT, len(out), size / 1024,
                                                                                                    integral))


if __name__ == '__main__':
    sys.exit(main())
