#!/usr/bin/env python3
"""Generate tests/golden/detection_layer_golden.npz: the reference's detection layer, EXECUTED from its own source.

geometric/maskrcnn/model.py cannot be imported here (old torch idioms, its compiled nms / roialign extensions).  This script takes
with `ast`, from where they lie, unique1d (model.py:77-86), intersect1d (:89-92), apply_box_deltas (:307-328), clip_to_window
(:731-741) and refine_detections (:744-837) and runs them unmodified under the installed torch on the CPU in float32, on the seeded
inputs of tests/detection_layer_util.py.  The one name they need from the compiled extension, nms, is bound to
oracle.maskrcnn_np.pth_nms(..., impl='ref'): the reference's own nms.c, compiled unmodified by oracle/build_ref.py into oracle/_ref.
The binding also records what the reference hands to its NMS: per class the rounded boxes and scores of the valid rows.

Before anything is stored the restatement is asserted equal to the reference, bit for bit, on every case that has a reference run:
the detections, and per class the boxes and scores that entered the NMS.  nms.c suppresses on IoU >= threshold, so the reference is
compared with the restatement's strict=False form; no case but `tie_iou` has a same-class pair of valid rows whose fp32 IoU equals
the threshold, so strict and loose keep the same rows there (asserted), and both are stored.  Where no row is a detection the
reference raises (asserted); `ties_score` hangs on the reference's unstable sorts.  Those cases are stored from the restatement.

The margin that makes the device's result exact: scores are gathered, never computed, and boxes are whole pixels after rounding, so
the last bit of expf can only show by moving a coordinate across k + 0.5.  For every case not built on exact halves, every finite
coordinate of the float64 run before rounding (a clipped one is the window's edge, a whole number) must lie further from k + 0.5 than
gate_px = 4 x the largest distance between the reference's own float32 coordinates and the float64 ones, at least 2^-23 x the image's
longer side.  Measured, printed, asserted and stored per case; nothing is widened by hand.  The inputs are not selected by seed
alone: draw_case (tests/detection_layer_util.py) redraws the deltas of a row while the float64 RESTATEMENT puts one of its coordinates
within DRAW_GATE = 0.01 px of a half -- with 4000 coordinates and gates near 1e-3 px no seed of N = 1000 passes untouched.  The
restatement only shapes the draw; the condition asserted here is on the reference's own float32 run against float64, after the
restatement has been shown equal to the reference bit for bit.  Only data goes into the fixture.  Runs
only where the reference exists."""
import ast
import os
import sys
import warnings

import numpy as np
import torch
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detection_layer_util as u   # noqa: E402
from oracle import maskrcnn_np as mnp   # noqa: E402

REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
FUNCTIONS = (('unique1d', 77, 86), ('intersect1d', 89, 92), ('apply_box_deltas', 307, 328), ('clip_to_window', 731, 741),
             ('refine_detections', 744, 837))


def take(path, functions, ns):
    """the named functions, compiled from where they lie"""
    body = ast.parse(open(path).read()).body
    for name, first, last in functions:
        (fn,) = [st for st in body if isinstance(st, ast.FunctionDef) and st.name == name]
        assert (fn.lineno, fn.end_lineno) == (first, last), (name, fn.lineno, fn.end_lineno)
        exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), ns)
    return ns


def reference_functions(calls):
    def nms(dets, thresh):
        keep = mnp.pth_nms(dets.numpy(), thresh, impl='ref')
        calls.append((dets.numpy().copy(), keep.copy()))
        return torch.from_numpy(keep)
    return take(MODEL, FUNCTIONS, {'torch': torch, 'np': np, 'Variable': Variable, 'nms': nms})


class Config(object):
    GPU_COUNT = 0
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, c):
        self.IMAGE_SHAPE = np.array([c['image'][0], c['image'][1], 3])
        self.DETECTION_MIN_CONFIDENCE = c['conf']
        self.DETECTION_NMS_THRESHOLD = c['thr']
        self.DETECTION_MAX_INSTANCES = c['D']


def run_reference(c):
    """(detections float32 [n, 6], [(boxes and scores [m, 5], kept) per class present]) of the reference's own code; with roi_count, on
    the rows before it"""
    calls = []
    ns = reference_functions(calls)
    n = c['N'] if c['roi_count'] is None else c['roi_count']
    args = [torch.from_numpy(c[k][:n].copy()) for k in ('rois', 'probs', 'deltas')]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')            # indexing with uint8 is deprecated
        out = ns['refine_detections'](args[0], args[1], args[2], np.asarray(c['window']), Config(c))
    return out.numpy(), calls


def same(a, b):
    """equal bits, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def main():
    assert mnp.have('ref'), 'oracle/_ref/libmaskrcnn_ref.so is missing: run `python __graft_entry__.py build` where the reference exists'
    out = {}
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        mine = u.contract(c, np.float32, strict=True)
        loose = u.contract(c, np.float32, strict=False)
        pre64 = u.contract(c, np.float64)['pre_round']
        class_ids, scores, pre32, valid = u.rows_of(c, np.float32)
        n_loose = int(loose['count'][0])
        if name in u.REFERENCE_RAISES:
            try:
                run_reference(c)
            except UnboundLocalError:
                pass
            else:
                raise AssertionError('%s: the reference was expected to raise' % name)
            assert int(mine['count'][0]) == 0 and not valid.any(), name
        elif name not in u.NO_REFERENCE:
            ref, calls = run_reference(c)
            # per class present, ascending: what entered the NMS
            present = np.unique(class_ids[valid])
            assert len(calls) == len(present), name
            for class_id, (dets, _kept) in zip(present, calls):
                rows = np.nonzero(valid & (class_ids == class_id))[0]
                rows = rows[u._descending(scores[rows])]
                assert same(dets[:, :4], mine['boxes_px'][rows]) and same(dets[:, 4], scores[rows]), (name, class_id)
            if name not in u.ROWS_ONLY:
                assert ref.dtype == np.float32 and same(ref, loose['detections'][:n_loose]), name
        if name not in u.ROWS_ONLY:
            on_thr = u.pairs_on_threshold(class_ids, mine['boxes_px'], valid, c['thr'])
            if name == 'tie_iou':
                assert on_thr == 1, on_thr
            else:
                assert on_thr == 0, (name, on_thr)
                assert all(same(mine[k], loose[k]) for k in u.OUTPUTS), name
            if name != 'ties_score':
                s = scores[valid]
                assert len(set(s.tolist())) == len(s), '%s: two equal scores among the valid rows' % name
        # the margin
        assert np.array_equal(np.isnan(pre32), np.isnan(pre64)) and np.array_equal(np.isinf(pre32), np.isinf(pre64)), name
        finite = np.isfinite(pre64)
        err = float(np.abs(pre32.astype(np.float64) - pre64)[finite].max())
        gate = max(4 * err, 2.0 ** -23 * max(c['image']))
        dist = u.half_distance(pre64)
        print('%-14s N %4d C %2d D %3d valid %4d kept %3d; float32 run within %.2e px of float64 before rounding, gate %.2e, nearest half %.2e'
              % (name, c['N'], c['C'], c['D'], int(valid.sum()), int(mine['count'][0]), err, gate, dist))
        if name in u.ON_HALVES:
            assert err == 0.0 and dist == 0.0, (name, err, dist)
        else:
            assert dist > gate, (name, dist, gate)
        for k in ('rois', 'probs', 'deltas'):
            out[p + 'crc_' + k] = np.uint32(u.checksum(c[k]))
        for k in u.OUTPUTS:
            out[p + k] = mine[k]
        out[p + 'keep_loose'] = loose['keep']
        out[p + 'count_loose'] = loose['count']
        out[p + 'valid'] = np.int32(valid.sum())
        out[p + 'fp32_error'] = np.float64(err)
        out[p + 'gate'] = np.float64(gate)
        out[p + 'half_distance'] = np.float64(dist)

    # what the cases are there for
    count = {name: int(out[name + '/count'][0]) for name in u.CASES}
    assert count['one'] == 1
    for n in (63, 64, 65):
        assert out['words%d/valid' % n] == n and 1 < count['words%d' % n] < n
    for name in ('real_c3', 'real_c81'):
        assert 250 <= out[name + '/valid'] <= 450 and count[name] > 20, (name, out[name + '/valid'], count[name])     # about a third
        b = out[name + '/boxes_px']
        assert (b[:, 0] == 128).any() and (b[:, 2] == 896).any()                                                        # the window clips
    assert out['real_c81/class_ids'].max() > 60
    assert count['cross_class'] == 6 and count['same_class'] == 1
    assert out['cross_class/boxes_px'].tobytes() == out['same_class/boxes_px'].tobytes()
    assert count['all_background'] == 0 and count['C1'] == 0 and count['below_conf'] == 0
    assert (out['below_conf/class_ids'] > 0).any() and count['no_min_conf'] > 0
    assert out['top_d/valid'] > 100 and count['top_d'] == 5 and np.array_equal(out['top_d/keep'], u._descending(out['top_d/scores'])[:5])
    assert 0 < count['few'] < u.CASES['few']['D'] and count['D1'] == 1 and out['D1/keep'][0] == out['few/keep'][0]
    rc = u.draw_case('roi_count')
    assert (out['roi_count/class_ids'][100:] > 0).all() and (out['roi_count/scores'][100:] >= 0.7).all()
    assert 0 < count['roi_count'] and out['roi_count/keep'].max() < rc['roi_count']
    b, w = out['window/boxes_px'], u.CASES['window']['window']
    assert all((b[:, k] == w[k]).any() and (b[:, k] == w[(k + 2) % 4]).any() for k in range(4))         # each coordinate on both of its edges
    pre = u.rows_of(u.draw_case('halves'), np.float32)[2]
    assert (np.rint(pre) != np.floor(pre + 0.5)).any() and (np.rint(pre) == np.floor(pre + 0.5)).any()   # half to even differs from half up
    t = out['ties_score/scores'][out['ties_score/keep'][:count['ties_score']]]
    assert len(set(t.tolist())) < len(t) and (np.diff(t) <= 0).all()
    assert count['tie_iou'] == int(out['tie_iou/count_loose'][0]) + 1 and 1 in out['tie_iou/keep'] and 1 not in out['tie_iou/keep_loose']
    a = u.draw_case('argmax_tie')
    assert ((a['probs'] == a['probs'].max(1, keepdims=True)).sum(1) >= 2).all() and (out['argmax_tie/class_ids'] == 0).any()
    assert np.isnan(out['nan_row/scores']).sum() == 20 and not np.isnan(out['nan_row/detections']).any() and count['nan_row'] > 0
    assert np.isnan(out['overflow/boxes_px']).any() and not np.isinf(out['overflow/boxes_px']).any()

    path = u.GOLD
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print('wrote %s: %d arrays, %.1f KiB' % (path, len(out), size / 1024))


if __name__ == '__main__':
    sys.exit(main())
