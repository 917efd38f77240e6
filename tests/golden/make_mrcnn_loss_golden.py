#!/usr/bin/env python3
"""Generate tests/golden/mrcnn_loss_golden.npz: the reference's Mask R-CNN training losses, EXECUTED from its own source.

geometric/maskrcnn/model.py cannot be imported here (old torch idioms, its compiled nms / roialign extensions).  This script
takes with `ast`, from where they lie, the six functions compute_rpn_class_loss, compute_rpn_bbox_loss, compute_mrcnn_class_loss,
compute_mrcnn_bbox_loss, compute_mrcnn_mask_loss and compute_losses (model.py:1004-1147) and runs them under the installed torch
on the CPU, on the seeded inputs of tests/mrcnn_loss_util.py, once in float64 and once in float32, with autograd for the gradients
of sum(WEIGHTS[k] * loss_k) + WEIGHTS[5] * (the sum of model.py:1955).

Per case the fixture holds: the checksums of the ten inputs (and the inputs themselves for the small cases), the float64 losses,
the counts, the float64 gradients as (indices, values) of their non-zero elements, the float32 run's distance from the float64
one in the measure of the GPU test's gate, and that gate: 1e-6, or 4 x the float32 run's distance where torch's own float32
arithmetic does not stay within 1e-6.  The restatement of tests/mrcnn_loss_util.py is asserted against the reference on every
case before anything is stored.  Only data goes into the fixture.  Runs only where the reference exists.

With R = 0 the reference's head functions are not run: under the installed torch an empty tensor's .size() is truthy, so they
would return NaN instead of the 0 their `else` branches (model.py:1073, 1102, 1132) were written for; the fixture holds that 0."""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mrcnn_loss_util as u   # noqa: E402

REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
FUNCTIONS = (('compute_rpn_class_loss', 1004, 1029), ('compute_rpn_bbox_loss', 1032, 1058), ('compute_mrcnn_class_loss', 1061, 1077),
             ('compute_mrcnn_bbox_loss', 1080, 1106), ('compute_mrcnn_mask_loss', 1109, 1136), ('compute_losses', 1139, 1147))


def reference_functions():
    body = ast.parse(open(MODEL).read()).body
    ns = {'torch': torch, 'F': F, 'Variable': Variable}
    for name, first, last in FUNCTIONS:
        (fn,) = [st for st in body if isinstance(st, ast.FunctionDef) and st.name == name]
        assert (fn.lineno, fn.end_lineno) == (first, last), (name, fn.lineno, fn.end_lineno)
        exec(compile(ast.Module(body=[fn], type_ignores=[]), MODEL, 'exec'), ns)
    return ns


def run_reference(ns, c, dtype):
    """(the six losses, {prediction: gradient}) of the reference's own code in `dtype`"""
    t = {}
    for k in u.INPUTS:
        a = torch.as_tensor(c[k])
        if a.dtype == torch.float32:
            a = a.to(dtype)
            if k in u.PREDICTIONS:
                a.requires_grad_()
        t[k] = a
    R = c['target_class_ids'].shape[0]
    if R:
        losses = ns['compute_losses'](*[t[k] for k in u.INPUTS])
        assert isinstance(losses, list) and len(losses) == 5
    else:
        zero = torch.zeros((), dtype=dtype)
        losses = [ns['compute_rpn_class_loss'](t['rpn_match'], t['rpn_class_logits']),
                  ns['compute_rpn_bbox_loss'](t['rpn_bbox'], t['rpn_match'], t['rpn_pred_bbox']), zero, zero, zero]
    loss = losses[0] + losses[1] + losses[2] + losses[3] + losses[4]          # model.py:1955
    w = [float(np.float32(v)) for v in u.WEIGHTS]
    total = sum(w[i] * losses[i] for i in range(5)) + w[5] * loss
    total.backward()
    grads = {k: (t[k].grad.numpy() if t[k].grad is not None else (np.zeros(c[k].shape) if R or k.startswith('rpn') else None))
             for k in u.PREDICTIONS}
    return [float(v) for v in losses] + [float(loss)], grads


def same(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol * max(abs(b), 1.0)


def main():
    ns = reference_functions()
    out = {'weights': np.asarray(u.WEIGHTS, np.float64)}
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        mine = u.reference(c)
        losses64, grads64 = run_reference(ns, c, torch.float64)
        losses32, grads32 = run_reference(ns, c, torch.float32)
        # the restatement is the reference, to float64's rounding
        for k, v in zip(u.LOSSES, losses64):
            assert same(mine[k], v, 1e-13), (name, k, mine[k], v)
        for k in u.PREDICTIONS:
            if grads64[k] is None:
                assert mine['grad'][k] is None
                continue
            assert np.allclose(mine['grad'][k], grads64[k], rtol=1e-11, atol=1e-300), (name, k)
            assert not grads64[k][~mine['selected'][k]].any(), (name, k)
        assert mine['bad'] == 0
        # the float32 run in the measure of the gate
        err = 0.0
        for k, v64, v32 in zip(u.LOSSES, losses64, losses32):
            assert np.isnan(v64) == np.isnan(v32), (name, k)
            if not np.isnan(v64):
                err = max(err, abs(v32 - v64))
        for k in u.PREDICTIONS:
            if grads64[k] is not None:
                err = max(err, u.grad_error(grads32[k], grads64[k], mine['n'][k]))
        gate = u.GATE if err <= u.GATE else 4.0 * err
        print('%-8s float32 run within %.3g of the float64 one; gate %.3g; losses %s' % (name, err, gate, ' '.join('%.6g' % v for v in losses64)))
        out[p + 'fp32_error'], out[p + 'gate'] = np.float64(err), np.float64(gate)
        for k in u.INPUTS:
            out[p + 'crc_' + k] = np.uint32(u.checksum(c[k]))
            if name in u.STORED_WHOLE:
                out[p + k] = c[k]
        for k, v in zip(u.LOSSES, losses64):
            out[p + k] = np.float64(v)
        for k in u.COUNTS:
            out[p + k] = np.int64(mine[k])
        for k in u.PREDICTIONS:
            if grads64[k] is not None:
                out[p + 'grad_idx_' + k], out[p + 'grad_val_' + k] = u.sparse(grads64[k])

    # what the cases are there for
    ch = u.draw_case('chunks')
    m = ch['rpn_match'].reshape(-1)
    A = m.shape[0]
    assert A % 4 and A > 4 * u.CHUNK and m[0] == 1 and m[A - 1] == 1
    for edge in (u.QUAD, u.STEP, u.CHUNK, 2 * u.CHUNK, 4 * u.CHUNK):
        assert m[edge - 1] == 1 and m[edge] == 1, edge
    assert 0 < int(out['chunks/n_rpn_pos']) < ch['rpn_bbox'].shape[1]
    ids = ch['target_class_ids']
    assert (ids == 0).any() and (ids > 0).any() and ch['mrcnn_mask'].shape[2:] == (28, 28)
    plane, target = ch['mrcnn_mask'][0, ids[0], 0, :4], ch['target_mask'][0, 0, :4]
    assert ids[0] > 0 and plane.tolist() == [0.0, 1.0, 0.0, 1.0] and target.tolist() == [0.0, 0.0, 1.0, 1.0]
    g = u.dense(out['chunks/grad_idx_mrcnn_mask'], out['chunks/grad_val_mrcnn_mask'], ch['mrcnn_mask'].shape)[0, ids[0], 0, :4]
    assert g[0] == 0.0 and g[3] == 0.0 and g[1] > 1e6 and g[2] < -1e6              # the 1e-12 floor
    used = np.nonzero(m == 1)[0]
    d = ch['rpn_pred_bbox'][0, used] - ch['rpn_bbox'][0, :len(used)]
    assert (d[0] == 1.0).all() and (d[-1] == -1.0).all()
    d = ch['mrcnn_bbox'][0, ids[0]] - ch['target_deltas'][0]
    assert d.tolist() == [1.0, 1.0, -1.0, -1.0]
    ex = u.draw_case('exact')
    assert int(out['exact/n_rpn_pos']) == ex['rpn_bbox'].shape[1] == int((ex['rpn_match'] == 1).sum()) and ex['rpn_match'].dtype == np.int64
    assert ex['rpn_match'].shape[1] == 2 * u.CHUNK and ex['mrcnn_mask'].shape == (1, 81, 28, 28)
    assert int(out['nopos/n_rpn_pos']) == 0 and np.isnan(out['nopos/rpn_bbox_loss']) and not np.isnan(out['nopos/rpn_class_loss'])
    assert u.draw_case('nopos')['mrcnn_mask'].shape == (200, 2, 5, 7)
    assert int(out['novalid/n_rpn_valid']) == 0 and np.isnan(out['novalid/rpn_class_loss']) and int(out['novalid/n_roi_pos']) == 0
    assert np.isnan(out['novalid/mrcnn_bbox_loss']) and np.isnan(out['novalid/mrcnn_mask_loss']) and not np.isnan(out['novalid/mrcnn_class_loss'])
    assert all(float(out['empty/' + k]) == 0.0 for k in u.LOSSES[2:5]) and 'empty/grad_idx_mrcnn_mask' not in out

    path = u.GOLD
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print('wrote %s: %d arrays, %.1f KiB' % (path, len(out), size / 1024))


if __name__ == '__main__':
    sys.exit(main())
