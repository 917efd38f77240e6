#!/usr/bin/env python3
"""Generate tests/golden/detections_golden.npz: the reference's way from the detector's heads to (class_ids, masks, rois),
EXECUTED from its own source.

geometric/maskrcnn/model.py, maskrcnn/utils.py, derender3d/datasets.py and scripts/main.py cannot be imported here (old torch
idioms, scipy.misc, absl, pandas ...).  This script takes with `ast`, from where they lie,
  * model.py    MaskRCNN.unmold_detections (:2084-2143)
  * utils.py    unmold_mask (:378-395) and resize_image (:272-320; only its window / scale arithmetic is used: the image
                resize inside it is replaced by a function that returns zeros of the requested shape)
  * datasets.py Transforms.scene_to_mask (:75-76) and Transforms.mask_to_roi (:95-103)
  * main.py     :805-807 (layout of the masks) and :812-818 (the 16 largest)
and executes them on seeded inputs.

scipy.misc.imresize no longer exists in the installed scipy.  `imresize` below restates scipy 1.0.1's published semantics
(misc/pilutil.py): imresize -> toimage -> bytescale -> Image.frombytes('L') -> Image.resize((w, h), BILINEAR) -> fromimage;
the resize is the real Pillow.  bytescale is evaluated AS NUMPY 1.14 DOES (the reference's environment.yml): there a float32
array times a float64 scalar stays float32 (the scalar `scale = 255.0 / cscale` is cast to float32 first), so the subtract,
multiply, clip and + 0.5 are float32 operations.  The numpy installed here (2.x) would promote the same expression to
float64 and can round to another byte; `bytescale_f64` is that evaluation, kept only to assert that the two differ on this
fixture, i.e. that the distinction is exercised.

Only data goes into the fixture (binary planes through np.packbits).  Every case the tests rely on is asserted here.  Runs
only where the reference exists."""
import ast
import os
import sys
import types

import numpy as np
import PIL.Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
UTILS = os.path.join(REF, 'geometric', 'maskrcnn', 'utils.py')
DATASETS = os.path.join(REF, 'geometric', 'derender3d', 'datasets.py')
MAIN = os.path.join(REF, 'geometric', 'scripts', 'main.py')
OUT = os.path.join(HERE, 'detections_golden.npz')


# ---------------------------------------------------------------------------------------------------- scipy 1.0.1's imresize
def bytescale(data):
    """pilutil.bytescale(data) with cmin = cmax = None, high = 255, low = 0, in numpy 1.14's arithmetic (see above)"""
    assert data.dtype == np.float32
    cmin, cmax = data.min(), data.max()
    cscale = cmax - cmin                                    # float32
    if cscale == 0:
        cscale = 1
    scale = np.float32(255.0 / float(cscale))               # the float64 quotient, cast to float32 by the multiplication
    bytedata = (data - cmin) * scale + np.float32(0)
    assert bytedata.dtype == np.float32
    out = bytedata.clip(np.float32(0), np.float32(255)) + np.float32(0.5)
    assert out.dtype == np.float32
    return out.astype(np.uint8)


def bytescale_f64(data):
    """the same expression as numpy 2.x promotes it -- NOT the reference's bytes; for the assertion in main() only"""
    cmin, cmax = data.min(), data.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    bytedata = (data - cmin).astype(np.float64) * (255.0 / float(cscale)) + 0
    return (bytedata.clip(0, 255) + 0.5).astype(np.uint8)


BYTES_SEEN = []


def imresize(arr, size, interp='bilinear', mode=None):
    assert interp == 'bilinear' and mode is None and arr.ndim == 2
    data = bytescale(np.asarray(arr))
    BYTES_SEEN.append((data, bytescale_f64(np.asarray(arr))))
    im = PIL.Image.frombytes('L', (data.shape[1], data.shape[0]), data.tobytes())
    imnew = im.resize((int(size[1]), int(size[0])), resample=PIL.Image.BILINEAR)
    return np.array(imnew)


# ---------------------------------------------------------------------------------------------------- the reference's code
def function_of(path, name, cls=None, first=None, last=None):
    src = open(path).read()
    body = ast.parse(src).body
    if cls is not None:
        (c,) = [st for st in body if isinstance(st, ast.ClassDef) and st.name == cls]
        body = c.body
    (fn,) = [st for st in body if isinstance(st, ast.FunctionDef) and st.name == name]
    if first is not None:
        assert (fn.lineno, fn.end_lineno) == (first, last), (name, fn.lineno, fn.end_lineno)
    fn.decorator_list = []
    return compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec')


def statements_of(path, first, last, opens):
    """the innermost statements of `path` that lie wholly in the lines first .. last"""
    src = open(path).read()
    sts = [st for st in ast.walk(ast.parse(src)) if isinstance(st, ast.stmt) and first <= st.lineno and st.end_lineno <= last]
    inner = set()
    for st in sts:
        for ch in ast.walk(st):
            if ch is not st and isinstance(ch, ast.stmt):
                inner.add(id(ch))
    sts = sorted([st for st in sts if id(st) not in inner], key=lambda st: st.lineno)
    assert sts and sts[0].lineno == first and sts[-1].end_lineno == last, (first, last)
    assert ast.get_source_segment(src, sts[0]).startswith(opens), ast.get_source_segment(src, sts[0])
    return compile(ast.Module(body=sts, type_ignores=[]), path, 'exec')


def reference():
    scipy_stub = types.SimpleNamespace(misc=types.SimpleNamespace(imresize=imresize))
    ns_utils = {'np': np, 'scipy': scipy_stub}
    exec(function_of(UTILS, 'unmold_mask', first=378, last=395), ns_utils)
    shape_only = types.SimpleNamespace(misc=types.SimpleNamespace(
        imresize=lambda image, size: np.zeros(tuple(size) + image.shape[2:], image.dtype)))
    ns_resize = {'np': np, 'scipy': shape_only}
    exec(function_of(UTILS, 'resize_image', first=272, last=320), ns_resize)
    ns_model = {'np': np, 'utils': types.SimpleNamespace(unmold_mask=ns_utils['unmold_mask'])}
    exec(function_of(MODEL, 'unmold_detections', cls='MaskRCNN', first=2084, last=2143), ns_model)
    ns_tr = {'np': np}
    exec(function_of(DATASETS, 'scene_to_mask', cls='Transforms'), ns_tr)
    exec(function_of(DATASETS, 'mask_to_roi', cls='Transforms'), ns_tr)
    layout = statements_of(MAIN, 805, 807, 'image_masks = np.transpose(image_masks, (2, 0, 1))')
    select = statements_of(MAIN, 812, 818, 'sels = np.flipud(np.argsort(')
    return ns_model['unmold_detections'], ns_resize['resize_image'], ns_tr['scene_to_mask'], ns_tr['mask_to_roi'], layout, select


# ---------------------------------------------------------------------------------------------------- seeded inputs
def soft_masks(rng, D, C, M=28):
    """sigmoid blobs with noise, as a mask head's outputs look: float32 [D, C, M, M]"""
    yy, xx = np.mgrid[0:M, 0:M].astype(np.float64)
    out = np.zeros((D, C, M, M), np.float32)
    for d in range(D):
        for c in range(C):
            cy, cx = rng.uniform(9, 18, 2)
            ry, rx = rng.uniform(5, 16, 2)
            logit = 5.0 * (1.0 - np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)) + rng.normal(0, 0.7, (M, M))
            out[d, c] = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    return out


def boundary_values(plane, limit=12):
    """float32 values whose byte differs between the two evaluations of bytescale (the float32 rounding of `scale`, of the
    product and of the sum each move a value by about one unit in the last place), those at the threshold (127 against 128)
    first; planted into a plane they do not change its minimum or maximum"""
    cmin, cmax = plane.min(), plane.max()
    scale = 255.0 / float(cmax - cmin)
    found = []
    for k in [127] + list(range(100, 127)) + list(range(128, 156)):
        x = np.float32((k + 0.5) / scale + float(cmin))
        cands = [x]
        for toward in (0, 1):
            c = x
            for _ in range(100):
                c = np.nextafter(c, np.float32(toward), dtype=np.float32)
                cands.append(c)
        probe = np.repeat(plane[None], len(cands), axis=0)
        probe[:, 14, 14] = cands
        for c, q in zip(cands, probe):
            if bytescale(q)[14, 14] != bytescale_f64(q)[14, 14]:
                found.append(float(c))
        if k == 127 and not found:
            return np.zeros(0, np.float32)
        if len(found) >= limit:
            break
    return np.asarray(found[:limit], np.float32)


def molded(boxes, window, image_shape):
    """detections coordinates whose unmolding gives `boxes` (+ 0.5: the truncation does not rest on a rounding)"""
    scale = min(image_shape[0] / (window[2] - window[0]), image_shape[1] / (window[3] - window[1]))
    shift = np.asarray([window[0], window[1], window[0], window[1]], np.float64)
    return ((np.asarray(boxes, np.float64) + 0.5) / scale + shift).astype(np.float32)


BOXES_A = [
    (180, 100, 260, 300), (150, 400, 250, 520),
    (200, 600, 220, 615),        # 2  both sides < 28: Pillow reduces (more taps)
    (20, 700, 350, 1000),        # 3  a side > 300
    (170, 50, 170, 120),         # 4  zero area: excluded
    (300, 1100, 375, 1242),      # 5  touches the frame's right and bottom edges
    (100, 0, 128, 60),           # 6  h = 28: Pillow skips the vertical pass; touches the left edge
    (0, 300, 40, 328),           # 7  w = 28: Pillow skips the horizontal pass; touches the top edge
    (180, 0, 190, 1242),         # 8  flatter than the mask and as wide as the frame: a band needs all 28 source rows
    (120, 800, 200, 900),        # 9  constant soft mask: cscale == 0, all zero
    (60, 150, 130, 260), (210, 320, 300, 470), (140, 530, 200, 640), (90, 900, 160, 1080), (250, 20, 330, 140),
    (30, 420, 75, 505), (160, 1010, 233, 1121), (270, 560, 340, 700), (10, 20, 95, 118), (225, 730, 262, 790),
    (305, 300, 372, 398), (135, 1130, 188, 1241), (50, 560, 117, 677), (262, 875, 349, 1003), (195, 215, 231, 297),
    (335, 600, 363, 628),        # 25 the mask's own size: no resampling, the thresholded bytes themselves; boundary values planted
]
ZERO_AREA, CONSTANT, PLANTED = 4, 9, 25


def case_detections(tag, image_shape, window, boxes, class_ids, D, C, seed, unmold_detections, layout, select, out, constant=None,
                    planted=None):
    rng = np.random.default_rng(seed)
    n = len(boxes)
    detections = np.zeros((D, 6), np.float32)
    if n:
        detections[:n, :4] = molded(boxes, window, image_shape)
        detections[:n, 4] = class_ids
        detections[:n, 5] = np.sort(rng.uniform(0.7, 0.999, n))[::-1]
    mrcnn_mask = np.zeros((D, C, 28, 28), np.float32)       # the network's layout
    mrcnn_mask[:max(n, 1)] = soft_masks(rng, max(n, 1), C)
    if constant is not None:
        mrcnn_mask[constant, class_ids[constant]] = np.float32(0.3)
    if planted is not None:
        values = boundary_values(mrcnn_mask[planted, class_ids[planted]])
        for _ in range(200):       # not every range has such a value at the threshold: draw the plane again
            if len(values):
                break
            mrcnn_mask[planted, class_ids[planted]] = soft_masks(rng, 1, 1)[0, 0]
            values = boundary_values(mrcnn_mask[planted, class_ids[planted]])
        assert len(values), 'no plane found that tells the float32 from the float64 evaluation at the threshold'
        mrcnn_mask[planted, class_ids[planted], 14, 8:8 + len(values)] = values
    # model.py:1640: the reference permutes to [D, Mh, Mw, C] for its numpy indexing
    b, ids, scores, full = unmold_detections(None, detections, np.ascontiguousarray(mrcnn_mask.transpose(0, 2, 3, 1)),
                                             image_shape, np.asarray(window))
    p = tag + '_'
    out[p + 'image_shape'] = np.asarray(image_shape, np.int32)
    out[p + 'window'] = np.asarray(window, np.int32)
    out[p + 'detections'] = detections
    out[p + 'mrcnn_mask'] = mrcnn_mask
    out[p + 'boxes'], out[p + 'class_ids'], out[p + 'scores'] = b, ids, scores
    out[p + 'masks_shape'] = np.asarray(full.shape, np.int32)
    res = {'boxes': b, 'class_ids': ids, 'scores': scores, 'full': full}
    if b.shape[0] == 0:
        return res
    assert full.dtype == np.uint8 and full.shape == (image_shape[0], image_shape[1], b.shape[0]) and full.max() <= 1
    ns = {'np': np, 'image_masks': full, 'class_ids': ids, 'rois': b}
    exec(layout, ns)
    image_masks = ns['image_masks']                          # [N, 1, H, W]
    assert image_masks.shape == (b.shape[0], 1, image_shape[0], image_shape[1])
    out[p + 'masks_bits'] = np.packbits(image_masks)
    out[p + 'areas'] = np.sum(image_masks, axis=(1, 2, 3)).astype(np.int32)
    exec(select, ns)
    out[p + 'sels'] = np.asarray(ns['sels'], np.int32)
    out[p + 'sel_class_ids'], out[p + 'sel_rois'] = ns['class_ids'], ns['rois']
    assert np.array_equal(ns['image_masks'], image_masks[ns['sels']])
    res.update(image_masks=image_masks, sels=ns['sels'])
    return res


def case_gt(tag, H, W, codes, painted, seed, out):
    """an instance-colour image with ellipses of the painted codes"""
    rng = np.random.default_rng(seed)
    scene = np.zeros((H, W, 3), np.uint8)
    scene[:] = (90, 90, 90)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in painted:
        cy, cx = rng.integers(8, H - 8), rng.integers(8, W - 8)
        ry, rx = rng.integers(3, H // 3), rng.integers(3, W // 4)
        scene[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = codes[k]
    p = tag + '_'
    out[p + 'scene'] = scene
    out[p + 'codes'] = np.asarray(codes, np.uint8)
    return scene


def main():
    unmold_detections, resize_image, scene_to_mask, mask_to_roi, layout, select = reference()
    out = {}

    # ---- a: the VKITTI frame, D = 100, C = 3
    shape_a = (375, 1242, 3)
    _, window_a, scale_a, _ = resize_image(np.zeros(shape_a, np.uint8), 300, 1024, padding=True)
    assert tuple(window_a) == (357, 0, 666, 1024), window_a
    out['a_mold'] = np.asarray([300, 1024], np.int32)
    out['a_scale'] = np.asarray(scale_a, np.float64)
    ids_a = [1 + (i * 7 + i // 3) % 2 for i in range(len(BOXES_A))]
    a = case_detections('a', shape_a, window_a, BOXES_A, ids_a, 100, 3, 41, unmold_detections, layout, select, out, constant=CONSTANT,
                        planted=PLANTED)
    keep = np.asarray([i for i in range(len(BOXES_A)) if i != ZERO_AREA])
    out['a_keep'] = keep.astype(np.int32)
    assert np.array_equal(a['boxes'], np.asarray(BOXES_A, np.int32)[keep])          # the zero-area row is gone
    assert np.array_equal(a['class_ids'], np.asarray(ids_a, np.int32)[keep]) and set(ids_a) == {1, 2}
    hh, ww = a['boxes'][:, 2] - a['boxes'][:, 0], a['boxes'][:, 3] - a['boxes'][:, 1]
    assert (np.maximum(hh, ww) < 28).any() and (np.maximum(hh, ww) > 300).any() and (hh == 28).any() and (ww == 28).any()
    assert ((a['boxes'][:, 2] == 375) & (a['boxes'][:, 3] == 1242)).any()
    assert ((hh < 28) & (ww * 28 > 32768)).any()                                    # the column chunks of the kernel
    areas = out['a_areas']
    assert len(set(areas.tolist())) == len(areas), 'areas must be distinct: the selection must not rest on tie order'
    assert areas[list(keep).index(CONSTANT)] == 0 and (areas > 0).sum() == len(areas) - 1
    assert len(areas) == 25 and len(a['sels']) == 16
    assert (areas[a['sels']] > 256).any() and (areas <= 256).any()
    differ = sum(int((f32 != f64).sum()) for f32, f64 in BYTES_SEEN)
    assert differ > 0, 'no byte differs between the float32 and the float64 evaluation of bytescale'
    out['a_bytes_f32_vs_f64'] = np.asarray(differ, np.int32)
    # the bytes themselves, for the emulation's first step
    out['a_bytes'] = np.stack([b for b, _ in BYTES_SEEN])
    assert out['a_bytes'].shape == (25, 28, 28)
    # ... and a difference reaches a mask: the planted box is not resampled, a byte of 127 against 128 is a pixel
    f32, f64 = BYTES_SEEN[24]
    assert ((f32 >= 128) != (f64 >= 128)).any() and (hh[24], ww[24]) == (28, 28)

    # ---- b: a small frame with one detection; c: none
    shape_b = (60, 90, 3)
    _, window_b, _, _ = resize_image(np.zeros(shape_b, np.uint8), 32, 64, padding=True)
    out['b_mold'] = np.asarray([32, 64], np.int32)
    b = case_detections('b', shape_b, window_b, [(12, 20, 47, 71)], [2], 4, 3, 42, unmold_detections, layout, select, out)
    assert b['boxes'].tolist() == [[12, 20, 47, 71]] and b['sels'].tolist() == [0]
    out['c_mold'] = np.asarray([32, 64], np.int32)
    c = case_detections('c', shape_b, window_b, [], [], 4, 3, 43, unmold_detections, layout, select, out)
    assert c['boxes'].shape == (0, 4) and c['class_ids'].shape == (0,) and c['scores'].shape == (0,) and c['full'].shape == (0, 28, 28)

    # ---- g: a ground-truth scene with 5 codes, one of them a single pixel; h: a code that matches nothing
    codes = [(255, 0, 0), (0, 255, 0), (17, 99, 203), (17, 99, 204), (250, 250, 1), (3, 2, 1)]
    scene = case_gt('g', 70, 110, codes[:5], [0, 1, 2, 3], 45, out)
    scene[5, 7] = codes[4]                                                           # the single pixel
    scene[69, 109] = codes[0]                                                        # the frame's last pixel
    out['g_scene'] = scene
    masks, rois = [], []
    for code in codes[:5]:
        m = scene_to_mask(scene, np.asarray(code, np.uint8))
        rois.append(mask_to_roi(m))
        masks.append(np.transpose(m, (2, 0, 1)))
    masks, rois = np.stack(masks, axis=0), np.stack(rois, axis=0)
    assert masks.shape == (5, 1, 70, 110) and masks.dtype == np.float32 and rois.shape == (5, 4)
    assert masks[4].sum() == 1 and rois[4].tolist() == [5, 7, 6, 8] and (masks.sum(axis=(1, 2, 3)) > 0).all()
    out['g_masks_bits'] = np.packbits(masks.astype(np.uint8))
    out['g_rois'] = rois.astype(np.int32)
    out['g_areas'] = masks.sum(axis=(1, 2, 3)).astype(np.int32)
    ns = {'np': np, 'image_masks': masks, 'class_ids': np.asarray([1, 2, 1, 1, 2]), 'rois': rois, 'image_ignores': None}
    exec(select, ns)
    out['g_sels'] = np.asarray(ns['sels'], np.int32)
    assert len(set(out['g_areas'].tolist())) == 5
    out['h_codes'] = np.asarray(codes[:2] + [codes[5]], np.uint8)
    try:
        mask_to_roi(scene_to_mask(scene, np.asarray(codes[5], np.uint8)))
        raise AssertionError('the reference accepted a code that matches nothing')
    except IndexError as e:
        out['h_error'] = np.asarray(type(e).__name__)

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1000000, size
    print('wrote %s: %d arrays, %.1f KiB; %d bytes differ between float32 and float64 bytescale' % (OUT, len(out), size / 1024, differ))


if __name__ == '__main__':
    sys.exit(main())
