#!/usr/bin/env python3
"""Generate tests/golden/proposal_layer_golden.npz: the reference's proposal layer, EXECUTED from its own source.

geometric/maskrcnn/model.py cannot be imported here (old torch idioms, its compiled nms / roialign extensions).  This script takes
with `ast`, from where they lie, apply_box_deltas (model.py:307-328), clip_boxes (:331-341) and proposal_layer (:344-407) and runs them
under the installed torch on the CPU in float32, on the seeded inputs of tests/proposal_layer_util.py; the literal 6000 of :374 is
replaced by the case's pre_nms_limit.  The one name they need from the
compiled extension, nms, is bound to oracle.maskrcnn_np.pth_nms(..., impl='ref'): the reference's own nms.c, compiled unmodified by
oracle/build_ref.py into oracle/_ref.  The binding also records what the reference hands to its NMS (the K decoded boxes with their
scores) and what comes back.  generate_anchors / generate_pyramid_anchors (utils.py:402-458) are taken the same way and compared with
the restated anchors.

Before anything is stored the restatement is asserted equal to the reference on every case that has a reference run: order and keep
exactly, boxes and normalised boxes bit for bit; and the margin condition is asserted: no pair of a case's K boxes has an fp32 IoU
within 1e-5 of the threshold (so `>` and `>=` keep the same boxes, and the last bit of exp cannot change them).  The `ties*` cases and
`tie_iou` hang on exact ties, which the reference's unstable sort and its two comparison rules do not pin down: they are stored from
the restatement.  Only data goes into the fixture.  Runs only where the reference exists."""
import ast
import os
import sys

import numpy as np
import torch
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import proposal_layer_util as u   # noqa: E402
from oracle import maskrcnn_np as mnp   # noqa: E402

REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
UTILS = os.path.join(REF, 'geometric', 'maskrcnn', 'utils.py')
FUNCTIONS = (('apply_box_deltas', 307, 328), ('clip_boxes', 331, 341), ('proposal_layer', 344, 407))
ANCHOR_FUNCTIONS = (('generate_anchors', 402, 438), ('generate_pyramid_anchors', 441, 458))


def take(path, functions, ns, limit=None):
    """the named functions, compiled from where they lie; limit: the one literal 6000 of proposal_layer (model.py:374, the reference's
    fixed pre-NMS limit) is replaced by this value, so that the small cases exercise K < A"""
    body = ast.parse(open(path).read()).body
    for name, first, last in functions:
        (fn,) = [st for st in body if isinstance(st, ast.FunctionDef) and st.name == name]
        assert (fn.lineno, fn.end_lineno) == (first, last), (name, fn.lineno, fn.end_lineno)
        if limit is not None and name == 'proposal_layer':
            literals = [n for n in ast.walk(fn) if isinstance(n, ast.Constant) and n.value == 6000]
            assert len(literals) == 1 and literals[0].lineno == 374, [n.lineno for n in literals]
            literals[0].value = int(limit)
        exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), ns)
    return ns


def reference_functions(calls, limit):
    def nms(dets, thresh):
        keep = mnp.pth_nms(dets.numpy(), thresh, impl='ref')
        calls.append((dets.numpy().copy(), keep.copy()))
        return torch.from_numpy(keep)
    return take(MODEL, FUNCTIONS, {'torch': torch, 'np': np, 'Variable': Variable, 'nms': nms}, limit)


class Config(object):
    GPU_COUNT = 0
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, image):
        self.IMAGE_SHAPE = np.array([image[0], image[1], 3])


def run_reference(c):
    """(order [K], boxes float32 [K, 4], keep [<= P], normalised boxes float32 [n, 4]) of the reference's own code"""
    calls = []
    ns = reference_functions(calls, c['limit'])
    inputs = [torch.from_numpy(c['probs'].copy())[None], torch.from_numpy(c['deltas'].copy())[None]]
    out = ns['proposal_layer'](inputs, c['P'], c['thr'], torch.from_numpy(c['anchors'].copy()), config=Config(c['image']))
    ((dets, keep),) = calls
    assert dets.shape == (c['K'], 5) and dets.dtype == np.float32 and out.dim() == 3 and out.shape[0] == 1
    # the anchor of every row, from its score: the scores of the best K + 1 are distinct
    scores = c['probs'][:, 1]
    where = {}
    for i in np.argsort(-scores, kind='stable')[:c['K'] + 1]:
        assert float(scores[i]) not in where, 'two equal scores'
        where[float(scores[i])] = int(i)
    order = np.asarray([where[float(s)] for s in dets[:, 4]], np.int32)
    return order, dets[:, :4].copy(), keep[:c['P']].astype(np.int32), out[0].numpy()


def same(a, b):
    """equal bits, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def main():
    assert mnp.have('ref'), 'oracle/_ref/libmaskrcnn_ref.so is missing: run `python __graft_entry__.py build` where the reference exists'
    gen = take(UTILS, ANCHOR_FUNCTIONS, {'np': np})
    for side in (256, 1024):
        shapes = [[int(np.ceil(side / s))] * 2 for s in u.STRIDES]
        ref = gen['generate_pyramid_anchors'](u.SCALES, u.RATIOS, shapes, u.STRIDES, 1).astype(np.float32)
        assert same(ref, u.pyramid_anchors(side)), side
    out = {}
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        mine = u.contract(c, np.float32, strict=True)
        loose = u.contract(c, np.float32, strict=False)
        b64 = u.contract(c, np.float64)['boxes']
        if name not in u.NO_REFERENCE:
            order, boxes32, keep, rois = run_reference(c)
            assert np.array_equal(order, mine['order']), name
            assert same(boxes32, mine['boxes']), name
            if name not in u.DECODE_ONLY:
                assert np.array_equal(keep, mine['keep']) and np.array_equal(keep, loose['keep']), name
                assert same(rois, mine['rois']), name
        if name != 'tie_iou' and name not in u.DECODE_ONLY:
            assert not u.near_pairs(mine['boxes'], c['thr']), name
            assert np.array_equal(mine['keep'], loose['keep']), name
        if name not in u.TIES:
            s = c['probs'][:, 1][u.select(c['probs'][:, 1], min(c['K'] + 1, c['A']))]
            assert len(set(s.tolist())) == len(s), name
        boxes32 = mine['boxes']
        finite = np.isfinite(boxes32) & np.isfinite(b64)
        err = float(np.abs(boxes32.astype(np.float64) - b64)[finite].max())
        gate = max(4 * err, 2.0 ** -23 * max(c['image']))
        assert np.array_equal(np.isnan(boxes32), np.isnan(b64)), name
        print('%-14s A %6d K %4d P %4d kept %4d; float32 run within %.2e px of float64, gate %.2e; smallest |IoU - thr| %.2e'
              % (name, c['A'], c['K'], c['P'], len(mine['keep']), err, gate, u.min_margin(boxes32, c['thr'])))
        out[p + 'crc_probs'] = np.uint32(u.checksum(c['probs']))
        out[p + 'crc_deltas'] = np.uint32(u.checksum(c['deltas']))
        out[p + 'crc_anchors'] = np.uint32(u.checksum(c['anchors']))
        out[p + 'order'] = mine['order']
        out[p + 'keep'] = mine['keep']
        out[p + 'keep_loose'] = loose['keep']
        out[p + 'count'] = np.int32(len(mine['keep']))
        out[p + 'crc_boxes32'] = np.uint32(u.checksum(boxes32))
        out[p + 'crc_rois32'] = np.uint32(u.checksum(mine['rois']))
        if name in u.STORED_WHOLE:
            out[p + 'boxes_px32'] = boxes32
            out[p + 'rois32'] = mine['rois']
            out[p + 'boxes_px64'] = b64
        out[p + 'fp32_error'] = np.float64(err)
        out[p + 'gate'] = np.float64(gate)

    # what the cases are there for
    assert out['onebox/count'] == 1
    assert out['disjoint/count'] == u.CASES['disjoint']['P'] and len(u.nms(out['disjoint/boxes_px32'], 0.7, True)) == 128     # nothing suppressed
    assert out['padded/count'] < u.CASES['padded']['P'] and out['full/count'] < u.CASES['full']['P'] and out['objects/count'] < out['objects/order'].size / 3
    assert np.isnan(out['overflow/boxes_px32']).any() and not np.isinf(out['overflow/boxes_px32']).any()
    assert len(out['tie_iou/keep']) == len(out['tie_iou/keep_loose']) + 1
    assert out['noexp/fp32_error'] < 1e-4 and np.array_equal(out['ties_all/order'], np.arange(1000))
    b = out['clip/boxes_px32']
    assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == 200).any() and (b[:, 3] == 200).any()

    path = u.GOLD
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print('wrote %s: %d arrays, %.1f KiB' % (path, len(out), size / 1024))


if __name__ == '__main__':
    sys.exit(main())
