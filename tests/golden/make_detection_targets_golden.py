#!/usr/bin/env python3
"""Generate tests/golden/detection_targets_golden.npz: the reference's detection targets, EXECUTED from its own source.

geometric/maskrcnn/model.py cannot be imported here (old torch idioms, its compiled nms / roialign extensions).  This script takes
with `ast`, from where they lie, bbox_overlaps (model.py:508-542), detection_target_layer (:545-724) and box_refinement
(utils.py:92-113) and runs them unmodified under the installed torch on the CPU in float32, on the seeded inputs of
tests/detection_targets_util.py.  Old idioms are met by binding names, never by editing the text:

  CropAndResizeFunction  oracle.maskrcnn_np.crop_forward(..., impl='ref'): the reference's own crop_and_resize.c, compiled
                         unmodified by oracle/build_ref.py into oracle/_ref
  utils                  a namespace that holds the box_refinement taken from utils.py
  torch                  a shim that hands every name on to torch but two: nonzero remembers its last result, and randperm(n)
                         returns the stable argsort of the call's key row (the first call keys[0], the second keys[1]) at those
                         rows -- the contract's sampling order, so that the reference's randperm(n)[:k] IS the contract's choice

Before anything is stored the restatement (`contract`) is asserted equal to the reference on every case that has a reference run:
rois, class ids, masks, dy and dx, the row order and the shapes bit for bit.  dh and dw pass through logf: they are measured against
the reference's own box_refinement run in float64 on the same rows, and the gate stored per case is four times the largest
|fp32 - fp64| of the reference (the tests let an element also pass within 2^-22 of its value).  Measured, printed, stored, never
widened by hand.  For the masks the smallest distance of a float64 sample before rounding from 0.5 is recorded and asserted to exceed
four times the float32 run's error; the draw (tests/detection_targets_util.py) moves a proposal one of whose samples lies within
DRAW_GATE = 0.01 of 0.5.  With roi_count the reference gets the rows before it.  Where the crowd filter leaves no box the reference
raises (asserted).  Only data goes into the fixture: the masks bit-packed, the inputs as checksums.  Runs only where the reference
exists."""
import ast
import os
import sys
import types
import warnings

import numpy as np
import torch
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detection_targets_util as u   # noqa: E402
from oracle import maskrcnn_np as mnp   # noqa: E402

REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
UTILS = os.path.join(REF, 'geometric', 'maskrcnn', 'utils.py')


def take(path, functions, ns):
    """the named functions, compiled from where they lie"""
    body = ast.parse(open(path).read()).body
    for name, first, last in functions:
        (fn,) = [st for st in body if isinstance(st, ast.FunctionDef) and st.name == name]
        assert (fn.lineno, fn.end_lineno) == (first, last), (name, fn.lineno, fn.end_lineno)
        exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), ns)
    return ns


class TorchShim(object):
    """torch, but nonzero remembers its last result and randperm is the order of the keys at those rows"""

    def __init__(self, keys):
        self.keys, self.last, self.calls = keys, None, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def nonzero(self, t):
        self.last = torch.nonzero(t)
        return self.last

    def randperm(self, n):
        rows = self.last[:, 0].numpy()
        assert n == len(rows) and self.calls < 2
        order = np.argsort(u.key_image(self.keys[self.calls][rows]), kind='stable')
        self.calls += 1
        return torch.from_numpy(order.astype(np.int64))


class CropAndResizeFunction(object):
    def __init__(self, crop_height, crop_width, extrapolation_value=0):
        self.size, self.extrapolation = (crop_height, crop_width), extrapolation_value

    def __call__(self, image, boxes, box_ind):
        out = mnp.crop_forward(image.numpy(), boxes.numpy(), box_ind.numpy(), self.size[0], self.size[1], self.extrapolation, impl='ref')
        return torch.from_numpy(out)


class Config(object):
    GPU_COUNT = 0
    BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, c):
        self.TRAIN_ROIS_PER_IMAGE, self.ROI_POSITIVE_RATIO = c['R'], c['ratio']
        self.USE_MINI_MASK, self.MASK_SHAPE = c['mini'], list(c['shape'])


def run_reference(c):
    """(rois, class ids, deltas, masks) of the reference's own code as numpy arrays, and its box_refinement"""
    n = c['N'] if c['roi_count'] is None else c['roi_count']
    refine = take(UTILS, (('box_refinement', 92, 113),), {'torch': torch})['box_refinement']
    ns = {'torch': TorchShim(c['keys'][:, :n]), 'np': np, 'Variable': Variable, 'CropAndResizeFunction': CropAndResizeFunction,
          'utils': types.SimpleNamespace(box_refinement=refine)}
    take(MODEL, (('bbox_overlaps', 508, 542), ('detection_target_layer', 545, 724)), ns)
    args = [torch.from_numpy(c['proposals'][:n].copy())[None], torch.from_numpy(c['gt_class_ids'].copy())[None],
            torch.from_numpy(c['gt_boxes'].copy())[None], torch.from_numpy(c['gt_masks'].copy())[None]]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = ns['detection_target_layer'](*args, Config(c))
    return [t.numpy() for t in out], refine


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main():
    assert mnp.have('ref'), 'oracle/_ref/libmaskrcnn_ref.so is missing: run `python __graft_entry__.py build` where the reference exists'
    out = {}
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        mine, exact = u.contract(c, np.float32), u.contract(c, np.float64)
        n, P = int(mine['count'][0]), int(mine['n_pos'][0])
        H, W = c['shape']
        log_err = 0.0
        if name in u.REFERENCE_RAISES:
            try:
                run_reference(c)
            except Exception:
                pass
            else:
                raise AssertionError('%s: the reference was expected to raise' % name)
            assert n == 0, name
        else:
            (rois, ids, deltas, masks), refine = run_reference(c)
            if n == 0:
                assert rois.size == ids.size == deltas.size == masks.size == 0, name
            else:
                assert rois.shape == (n, 4) and ids.shape == (n,) and deltas.shape == (n, 4) and masks.shape == (n, H, W), name
                assert rois.dtype == deltas.dtype == masks.dtype == np.float32 and ids.dtype in (np.int32, np.int64), name
                assert same(rois, mine['rois'][:n]), name                         # the rows and their order
                assert np.array_equal(ids, mine['target_class_ids'][:n]), name
                assert same(masks, mine['target_mask'][:n]), name
                assert same(deltas[:, :2], mine['target_deltas'][:n, :2]), name    # dy, dx: IEEE operations only
                assert same(deltas[P:], np.zeros((n - P, 4), np.float32)), name
                # dh, dw: the reference's float32 run against its own float64 run of the same function on the same rows
                b, g = torch.from_numpy(mine['rois'][:P].astype(np.float64)), torch.from_numpy(c['gt_boxes'][mine['assign'][:P]].astype(np.float64))
                d64 = (refine(b, g) / torch.from_numpy(np.asarray(u.STD_DEV, np.float32).astype(np.float64))).numpy()
                log_err = float(np.abs(deltas[:P, 2:].astype(np.float64) - d64[:, 2:]).max())
                assert np.abs(mine['target_deltas'][:P, 2:].astype(np.float64) - deltas[:P, 2:]).max() <= 4 * log_err, name
                assert np.allclose(d64, exact['target_deltas'][:P], rtol=1e-12, atol=0), name
        gate = 4 * log_err
        mask_err = float(np.abs(mine['pre_round'].astype(np.float64) - exact['pre_round']).max()) if P else 0.0
        dist = u.half_distance(exact['pre_round'])
        print('%-19s N %4d G %3d R %4d count %4d positives %3d; dh, dw of the float32 run within %.2e of float64, gate %.2e; '
              'mask samples within %.2e, nearest to 0.5 at %.2e' % (name, c['N'], c['G'], c['R'], n, P, log_err, gate, mask_err, dist))
        assert dist > 4 * mask_err and (name in u.EXPLICIT or dist >= u.DRAW_GATE), (name, dist, mask_err)
        for k in u.INPUTS:
            out[p + 'crc_' + k] = np.uint32(u.checksum(c[k]))
        for k in u.OUTPUTS:
            if k != 'target_mask':
                out[p + k] = mine[k]
        out[p + 'target_mask_bits'] = u.pack_masks(mine['target_mask'])
        out[p + 'log_error'] = np.float64(log_err)
        out[p + 'gate'] = np.float64(gate)
        out[p + 'mask_error'] = np.float64(mask_err)
        out[p + 'half_distance'] = np.float64(dist)

    # what the cases are there for
    cnt = {k: int(out[k + '/count'][0]) for k in u.CASES}
    pos = {k: int(out[k + '/n_pos'][0]) for k in u.CASES}
    assert cnt['n1'] == pos['n1'] == 1
    for k in ('n63', 'n64', 'n65'):
        assert pos[k] == 4 and cnt[k] == 8, (k, pos[k], cnt[k])                                 # R = 8, ratio 0.5: both caps bind
    for k in ('n1025', 'n8192', 'g100', 'real'):
        assert pos[k] == 66 and cnt[k] == 200, (k, pos[k], cnt[k])                             # int(200 * 0.33) and int((1 / 0.33) * 66 - 66) = 134
    assert out['n1025/rows'][0] == 1024 and out['n8192/assign'].max() > 100 and out['g100/assign'].max() > 64
    assert pos['r1100'] == 550 and cnt['r1100'] == 1100
    assert pos['ratio_one'] == cnt['ratio_one'] == 32
    assert cnt['none_positive'] == 0 and cnt['only_crowd'] == 0
    assert cnt['no_negative'] == pos['no_negative'] == 21
    assert 0 < pos['few_positive'] < 21 and cnt['few_positive'] == pos['few_positive'] + u.negative_count(0.33, pos['few_positive']) < 64
    assert pos['few_negative'] == 21 and 21 < cnt['few_negative'] < 21 + u.negative_count(0.33, 21)
    for k in ('crowd', 'crowd_with_zero_id'):
        c = u.draw_case(k)
        positive, negative, assign, gt = u.classes_of(c)
        assert (c['gt_class_ids'] < 0).any() and not gt.all() and (~positive & ~negative).sum() > 10, k    # the crowd keeps rows out
        assert (c['gt_class_ids'][out[k + '/assign'][:pos[k]]] > 0).all() and pos[k] > 0
    assert (u.draw_case('crowd_with_zero_id')['gt_class_ids'] == 0).any()
    z = out['zero_id_no_crowd/target_class_ids'][:pos['zero_id_no_crowd']]
    assert (z == 0).any() and (z > 0).any()                                                    # a positive with class id 0
    assert pos['iou_half'] == 2 and sorted(out['iou_half/rows'][:2]) == [0, 1] and 2 in out['iou_half/rows'][2:cnt['iou_half']]
    t = out['tie_argmax/assign'][:pos['tie_argmax']]
    assert (t == 0).any() and not (t == 1).any()
    tk = u.draw_case('tie_keys')['keys']
    assert len(np.unique(tk)) <= 4 and len(np.unique(tk[0][out['tie_keys/rows'][:pos['tie_keys']]])) < pos['tie_keys']
    nan = u.draw_case('nan_iou')
    ov = u.overlaps(nan['proposals'], nan['gt_boxes'])
    assert np.isnan(ov).any(axis=1).sum() == 8 and not np.isin(np.nonzero(np.isnan(ov).any(axis=1))[0], out['nan_iou/rows']).any() and pos['nan_iou'] > 0
    assert out['roi_count/rows'].max() < 100 and cnt['roi_count'] == 63
    assert out['full_mask/target_mask_bits'].any() and out['mask_7x9/target_mask_bits'].any()

    path = u.GOLD
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print('wrote %s: %d arrays, %.1f KiB' % (path, len(out), size / 1024))


if __name__ == '__main__':
    sys.exit(main())
