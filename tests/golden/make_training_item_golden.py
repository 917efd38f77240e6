#!/usr/bin/env python3
"""Generate tests/golden/training_item_golden.npz: the reference's training item -- load_image_gt with resize_image, resize_mask,
extract_bboxes, minimize_mask, compose_image_meta, mold_image and MaskRCNN.mold_inputs -- EXECUTED from its own source.

geometric/maskrcnn/model.py and utils.py cannot be imported here (old torch idioms, scipy.misc ...).  This script takes the functions
with `ast` from where they lie (the way make_detections_golden.py does) and gives them the real Pillow, the real scipy.ndimage.zoom
and the imresize restatement that make_detections_golden.py documents (tests/training_item_util.py: imresize; the crops here are
0 / 1 in float64, where bytescale is exact in any numpy).  They run on seeded inputs through a stub dataset object; the flip's
random.randint is a stub that returns what the case asks for.

Where the reference raises (minimize_mask on an instance that vanished in the zoom) the script asserts that it does, and takes the
other instances' mini-masks from minimize_mask on the instances that are left.

Only data goes into the fixture: packed bits for the masks, uint8 for the padded images (a mirrored image or mask stack is asserted
to be np.fliplr of the plain one and is not stored).  Every property the tests rely on is asserted here, and so is that
tests/training_item_util.py gives the same bits.  Runs only where the reference exists."""
import ast
import os
import sys
import types

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), '3d-sdn_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), '3d-sdn_amd', 'geometric'))
import training_item_util as u   # noqa: E402

REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
UTILS = os.path.join(REF, 'geometric', 'maskrcnn', 'utils.py')
OUT = os.path.join(HERE, 'training_item_golden.npz')


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


class Coin(object):
    """random.randint(0, 1) with a set outcome"""

    def __init__(self):
        self.outcome = 0

    def randint(self, a, b):
        assert (a, b) == (0, 1)
        return self.outcome


COIN = Coin()


def reference():
    scipy_stub = types.SimpleNamespace(misc=types.SimpleNamespace(imresize=u.imresize), ndimage=scipy.ndimage)
    ns_utils = {'np': np, 'scipy': scipy_stub}
    for name, first, last in (('extract_bboxes', 26, 49), ('resize_image', 272, 320), ('resize_mask', 323, 335), ('minimize_mask', 338, 353)):
        exec(function_of(UTILS, name, first=first, last=last), ns_utils)
    ns_model = {'np': np, 'random': COIN, 'utils': types.SimpleNamespace(**{k: ns_utils[k] for k in ('extract_bboxes', 'resize_image', 'resize_mask', 'minimize_mask')})}
    exec(function_of(MODEL, 'compose_image_meta', first=2150, last=2168), ns_model)
    exec(function_of(MODEL, 'mold_image', first=2196, last=2201), ns_model)
    exec(function_of(MODEL, 'load_image_gt', first=1154, last=1211), ns_model)
    exec(function_of(MODEL, 'mold_inputs', cls='MaskRCNN', first=2046, last=2082), ns_model)
    return ns_utils, ns_model


class Dataset(object):
    """what load_image_gt asks of a dataset: one image, one source with every class"""

    def __init__(self, frame, inst_map, ids, class_ids, num_classes):
        self.frame, self.stack, self.class_ids, self.num_classes = frame, u.instance_stack(inst_map, ids), class_ids, num_classes
        self.image_info = [{'source': 'seeded'}]
        self.source_class_ids = {'seeded': list(range(num_classes))}

    def load_image(self, image_id):
        return self.frame

    def load_mask(self, image_id):
        return self.stack, self.class_ids


# ---------------------------------------------------------------------------------------------------- seeded inputs
def noise_frame(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), ((xx + yy) * 3) % 256], axis=-1)
    return np.clip(base + rng.integers(-60, 61, (H, W, 3)), 0, 255).astype(np.uint8)


def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def ell_shape(H, W, r0, r1, c0, c1):
    """the rows r0 .. r1 and columns c0 .. c1 without their top left quarter: the extents of a rectangle, but not solid"""
    m = np.zeros((H, W), bool)
    m[r0:r1 + 1, c0:c1 + 1] = True
    m[r0:(r0 + r1) // 2, c0:(c0 + c1) // 2] = False
    return m


def tables(H, W, cfg):
    from maskrcnn.training_item import resize_plan, zoom_table
    oh, ow, window, scale, padding = resize_plan((H, W, 3), cfg)
    return oh, ow, zoom_table(H, oh), zoom_table(W, ow)


def run_span(tab, want, lo):
    """source indices (a, b), a >= lo, such that exactly `want` outputs read a .. b"""
    for a in range(lo, int(tab.max()) + 1):
        for b in range(a, int(tab.max()) + 1):
            n = int(((tab >= a) & (tab <= b)).sum())
            if n == want and (tab == a).any() and (tab == b).any():
                return a, b
            if n > want:
                break
    raise AssertionError('no span of %d outputs' % want)


def paint(shapes, H, W, rgb, first_id):
    """shapes painted in order (a later one covers an earlier one) -> (inst_map, ids)"""
    ids = np.asarray([first_id + 7 * k for k in range(len(shapes))], np.int32)
    flat = np.zeros((H, W), np.int32)
    for k, m in enumerate(shapes):
        flat[m] = ids[k]
    if rgb:
        return np.stack([(flat >> 16) & 255, (flat >> 8) & 255, flat & 255], axis=-1).astype(np.uint8), ids
    return flat, ids


def case_down(rng):
    H, W, cfg = 75, 248, u.Config(64, 192, 56)
    oh, ow, yt, xt = tables(H, W, cfg)
    assert (oh, ow) == (58, 192) and xt[-1] == -1 and (yt >= 0).all() and (xt[:-1] >= 0).all(), 'the last column is the constant'
    skipped = [c for c in range(50, 58) if c not in set(xt.tolist())][0]
    kept = [c for c in range(44, 49) if c in set(xt.tolist())][0]
    c0, c1 = run_span(xt, 56, 125)
    row = [r for r in range(3, 9) if r in set(yt.tolist())][0]
    line = np.zeros((H, W), bool)
    line[5:31, kept] = line[40:61, kept] = True
    pixel = np.zeros((H, W), bool)
    pixel[row, skipped] = True
    solid = np.zeros((H, W), bool)
    solid[50:71, 10:41] = True
    shapes = [ellipse(H, W, 20, 20, 12, 10), ellipse(H, W, 25, 247, 20, 15), solid, pixel, line, ellipse(H, W, 20, 110, 15, 50),
              ell_shape(H, W, 45, 72, c0, c1)]
    inst_map, ids = paint(shapes, H, W, True, 0x0a1b2c)
    return noise_frame(rng, H, W), inst_map, ids, cfg, dict(narrow=0, edge=1, solid=2, gone=3, line=4, wide=5, exact_w=6)


def case_up(rng):
    H, W, cfg = 40, 60, u.Config(96, 192, 28)
    oh, ow, yt, xt = tables(H, W, cfg)
    assert (oh, ow) == (96, 144)
    shapes = [ellipse(H, W, 10, 15, 8, 12), ell_shape(H, W, 4, 30, 30, 55), ellipse(H, W, 30, 12, 8, 9)]
    inst_map, ids = paint(shapes, H, W, False, 26001)
    return noise_frame(rng, H, W), inst_map, ids, cfg, {}


def case_same(rng):
    H, W, cfg = 99, 121, u.Config(64, 128, 28)
    shapes = [ellipse(H, W, 30, 0, 20, 25), ellipse(H, W, 70, 80, 25, 30), ell_shape(H, W, 3, 30, 60, 110)]
    inst_map, ids = paint(shapes, H, W, False, 24000)
    return noise_frame(rng, H, W), inst_map, ids, cfg, dict(left=0, exact_h=2)


def case_exact(rng):
    H, W, cfg = 128, 128, u.Config(128, 128, 28)
    inst_map, ids = paint([ellipse(H, W, 60, 70, 40, 30)], H, W, True, 0xc81e64)
    return noise_frame(rng, H, W), inst_map, ids, cfg, {}


def case_many(rng):
    H, W, cfg = 48, 80, u.Config(64, 128, 28)
    shapes = []
    for g in range(128):
        r, c = 6 * (g // 16), 5 * (g % 16)
        m = np.zeros((H, W), bool)
        m[r:r + 5, c:c + 4] = True
        m[r + (g % 5), c + (g % 4)] = g % 3 == 0     # two of three lose a pixel: not solid
        shapes.append(m)
    inst_map, ids = paint(shapes, H, W, False, 1000)
    return noise_frame(rng, H, W), inst_map, ids, cfg, {}


def run_reference(ns_utils, ns_model, frame, inst_map, ids, class_ids, cfg, flip, use_mini):
    """load_image_gt; with mini-masks and a vanished instance: asserts that it raises, then minimize_mask on the others"""
    data = Dataset(frame, inst_map, ids, class_ids, cfg.NUM_CLASSES)
    COIN.outcome = int(flip)
    image, meta, cls, bbox, full = ns_model['load_image_gt'](data, cfg, 0, augment=True, use_mini_mask=False)
    assert full.dtype == bool and bbox.dtype == np.int32 and image.dtype == np.uint8 and np.array_equal(cls, class_ids)
    if not use_mini:
        return image, meta, bbox, full
    gone = np.where((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1]) == 0)[0]
    try:
        image2, meta2, _, bbox2, mini = ns_model['load_image_gt'](data, cfg, 0, augment=True, use_mini_mask=True)
        assert len(gone) == 0 and np.array_equal(image2, image) and np.array_equal(meta2, meta) and np.array_equal(bbox2, bbox)
    except Exception as e:
        assert len(gone) and 'Invalid bounding box with area of zero' in str(e), e
        left = np.asarray([g for g in range(len(ids)) if g not in set(gone.tolist())])
        mini = np.zeros(tuple(cfg.MINI_MASK_SHAPE) + (len(ids),), bool)
        mini[:, :, left] = ns_utils['minimize_mask'](bbox[left], full[:, :, left], cfg.MINI_MASK_SHAPE)
    assert mini.dtype == bool and mini.shape == tuple(cfg.MINI_MASK_SHAPE) + (len(ids),)
    return image, meta, bbox, mini


def main():
    from maskrcnn.training_item import resize_plan
    ns_utils, ns_model = reference()
    rng = np.random.default_rng(20)
    out, images = {}, {}
    makers = dict(down=case_down, up=case_up, same=case_same, exact=case_exact, many=case_many)
    assert tuple(makers) == u.CASES
    for name in u.CASES:
        frame, inst_map, ids, cfg, tags = makers[name](rng)
        G, M, mini_shape = len(ids), cfg.IMAGE_MAX_DIM, tuple(cfg.MINI_MASK_SHAPE)
        class_ids = (1 + np.arange(G) % (cfg.NUM_CLASSES - 1)).astype(np.int32)
        p = name + '_'
        out[p + 'frame'], out[p + 'inst_map'], out[p + 'ids'], out[p + 'class_ids'] = frame, inst_map, ids, class_ids
        out[p + 'dims'] = np.asarray([cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, mini_shape[0]], np.int32)
        # the plan: resize_image's own returns
        _, window, scale, padding = ns_utils['resize_image'](frame, min_dim=cfg.IMAGE_MIN_DIM, max_dim=cfg.IMAGE_MAX_DIM, padding=True)
        oh, ow = window[2] - window[0], window[3] - window[1]
        out[p + 'plan'] = np.asarray([oh, ow] + list(window) + [padding[0][0], padding[0][1], padding[1][0], padding[1][1]], np.int32)
        out[p + 'scale'] = np.asarray(scale, np.float64)
        assert resize_plan(frame.shape, cfg) == (oh, ow, window, scale, padding)
        plain = {}
        for flip in (0, 1):
            image, meta, bbox, full = run_reference(ns_utils, ns_model, frame, inst_map, ids, class_ids, cfg, flip, False)
            image_m, meta_m, bbox_m, mini = run_reference(ns_utils, ns_model, frame, inst_map, ids, class_ids, cfg, flip, True)
            assert np.array_equal(image, image_m) and np.array_equal(meta, meta_m) and np.array_equal(bbox, bbox_m)
            assert image.shape == (M, M, 3) and full.shape == (M, M, G)
            if flip == 0:
                plain = dict(image=image, full=full, meta=meta)
                out[p + 'image_u8'] = image
                out[p + 'full_bits'] = np.packbits(full)
                out[p + 'meta'] = meta.astype(np.int64)
                out[p + 'areas'] = full.reshape(-1, G).sum(axis=0).astype(np.int32)
                images[name] = image
            else:   # the mirror of the PADDED image; the window in the meta stays
                assert np.array_equal(image, np.fliplr(plain['image'])) and np.array_equal(full, np.fliplr(plain['full']))
                assert np.array_equal(meta, plain['meta'])
            out[p + 'boxes%d' % flip] = bbox
            out[p + 'mini_bits%d' % flip] = np.packbits(mini)
            # what Dataset.__getitem__ makes of the image (:1398, :1401)
            molded = ns_model['mold_image'](image.astype(np.float32), cfg)
            assert molded.dtype == np.float64
            # tests/training_item_util.py gives the same bits
            for use_mini, masks in ((False, full), (True, mini)):
                r = u.training_item(frame, inst_map, ids, cfg, flip=bool(flip), use_mini_mask=use_mini)
                assert np.array_equal(r['image_u8'], image) and np.array_equal(r['gt_boxes_int'], bbox) and r['window'] == window
                assert np.array_equal(r['image'], molded.transpose(2, 0, 1).astype(np.float32))
                assert np.array_equal(r['gt_masks'], masks.astype(int).transpose(2, 0, 1).astype(np.float32))
                assert np.array_equal(r['areas'], out[p + 'areas'])
            # ---- the properties the tests rely on
            areas, hh, ww = out[p + 'areas'], bbox[:, 2] - bbox[:, 0], bbox[:, 3] - bbox[:, 1]
            mini_area = mini.reshape(-1, G).sum(axis=0)
            if name == 'down':
                assert padding[0] == (67, 67) and padding[1] == (0, 0)
                e = tags['edge']    # the constant column takes the instance's last column: it ends one short of the frame
                assert (bbox[e, 3] == 191 if flip == 0 else bbox[e, 1] == 1), bbox[e]
                s = tags['solid']
                assert areas[s] == hh[s] * ww[s] > 0 and mini_area[s] == 0, 'a solid rectangle has an all-zero mini-mask'
                z = tags['gone']
                assert areas[z] == 0 and bbox[z].tolist() == [0, 0, 0, 0] and mini_area[z] == 0 and (areas == 0).sum() == 1
                l = tags['line']
                assert ww[l] == 1 and hh[l] > 30 and 0 < areas[l] < hh[l] and mini_area[l] > 0, 'one pixel wide, and it survives'
                assert ww[tags['wide']] > 56 and ww[tags['narrow']] < 56 and ww[tags['exact_w']] == 56 and hh[tags['exact_w']] != 56
                assert mini_area[tags['exact_w']] > 0 and mini_area[tags['wide']] > 0
                out[p + 'bad'] = np.asarray([1], np.int32)
            else:
                assert (areas > 0).all()
                out[p + 'bad'] = np.asarray([0], np.int32)
            if name == 'up':
                assert scale == 2.4 and (hh > 28).any() and (ww > 28).any()
            if name == 'same':
                assert scale == 1 and padding[0] == (14, 15) and padding[1] == (3, 4), 'odd pads: the mirror shows'
                assert (bbox[tags['left'], 1] == 3 if flip == 0 else bbox[tags['left'], 3] == 128 - 3)
                assert hh[tags['exact_h']] == 28 and ww[tags['exact_h']] != 28 and mini_area[tags['exact_h']] > 0, 'the vertical pass is skipped'
            if name == 'exact':
                assert scale == 1 and window == (0, 0, 128, 128) and G == 1
            if name == 'many':
                assert G == 128 and padding[1] == (10, 11) and scale == 64 / 48
                assert (mini_area == 0).any() and (mini_area > 0).any()
    # ---- mold_inputs on a list with three frame sizes, one of them twice
    cfg = u.Config(64, 128, 28)
    names = ['same', 'exact', 'many', 'same']
    model = types.SimpleNamespace(config=cfg)
    molded, metas, windows = ns_model['mold_inputs'](model, [out[n + '_frame'] for n in names])
    assert molded.dtype == np.float64 and molded.shape == (4, 128, 128, 3)
    for k, n in enumerate(names):
        assert np.array_equal(molded[k], images[n].astype(np.float32) - cfg.MEAN_PIXEL), n
    out['mold_names'] = np.asarray(names)
    out['mold_metas'] = metas.astype(np.int64)
    out['mold_windows'] = windows.astype(np.int64)

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 600000, size
    print('wrote %s: %d arrays, %.1f KiB' % (OUT, len(out), size / 1024))


if __name__ == '__main__':
    sys.exit(main())
