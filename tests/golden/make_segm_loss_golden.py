#!/usr/bin/env python3
"""Generate tests/golden/segm_loss_golden.npz: the reference's semantic training loss, executed on the CPU in float64.

Imported from the reference as it lies: SegmentationModuleBase.pixel_acc of semantic/models.py (:15-21), where that module
imports under this torch; tests/segm_loss_util.py restates it statement for statement and `reference` asserts that both give
the same bits.  Where models.py does not import, the restatement is used alone; the fixture's key `pixel_acc` says which
happened.  The loss is torch's own nn.NLLLoss(ignore_index=-1) (vkitti_train.py:133) over F.log_softmax(dim=1)
(models.py:279-280, 412-413), combined as models.py:39-44 does, in float64 with autograd for the gradients of
0.7 loss + 1.3 loss_main + 0.45 loss_deepsup.

One thing the reference cannot be asked: a label outside [-1, C) makes NLLLoss raise.  The device treats such a pixel as
ignored and counts it in `bad`, so the reference functions are handed the labels with those turned into -1 (the raise itself
is asserted here); the fixture stores the labels as drawn.

Per case the generator asserts what the tie rule rests on: the drawing contains exact ties of the two best scores (cases with
C >= 2 and a valid pixel count worth the name; C = 1 has no second class), torch's fp32 CPU prediction equals the float64 one,
and both equal the lowest-index arg-max of the scores.  Only the main head predicts (models.py:44), so only its scores are asked.

Stored per case: the inputs (scores as int16 eighths: they are multiples of 1 / 8; labels), loss, loss_main, loss_deepsup, acc,
acc_sum, pixel_sum, bad and both float64 gradients -- in full for the small cases, for `maxc` and `blocks*` (101 904 float64
elements do not fit the 300 KB the fixture may take) as every 8th element plus the 2-norm; the tests rerun the float64
expressions of segm_loss_util.reference, compare with these and then hold the device against the full arrays.  Runs only where
the reference exists.
"""
import os
import sys
import warnings

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
sys.path.insert(0, os.path.join(REF, 'semantic'))

import segm_loss_util as u   # noqa: E402

warnings.filterwarnings('ignore')
try:
    import models as ref_models   # the reference's semantic/models.py
    _base = ref_models.SegmentationModuleBase()
    ACC_FN = _base.pixel_acc
    PIXEL_ACC = 'semantic/models.py SegmentationModuleBase.pixel_acc, :15-21'
except Exception as e:   # noqa: BLE001
    ACC_FN = None
    PIXEL_ACC = 'restated in tests/segm_loss_util.py (models.py did not import: %r)' % (e,)


def check_ties(name, scores, label):
    """the three properties the strict-> rule rests on"""
    C = scores.shape[1]
    first = scores.argmax(axis=1)                                  # numpy: the first of equal maxima
    p32 = torch.max(F.log_softmax(torch.as_tensor(scores), dim=1), dim=1)[1].numpy()
    p64 = torch.max(F.log_softmax(torch.as_tensor(scores).double(), dim=1), dim=1)[1].numpy()
    assert np.array_equal(p32, p64), 'case %s: the fp32 prediction differs from the float64 one' % name
    assert np.array_equal(p64, first), 'case %s: the prediction is not the lowest-index arg-max of the scores' % name
    ties = 0
    if C >= 2:
        gap = u.top_two_gap(scores)
        assert bool(((gap == 0) | (gap >= 0.125)).all())
        ties = int((gap == 0).sum())
        assert ties > 0, 'case %s: the drawing holds no exact tie: change the seed' % name
    return ties


def main():
    out = {'pixel_acc': PIXEL_ACC, 'weights': np.asarray([u.WEIGHTS[k] for k in ('loss', 'acc', 'loss_main', 'loss_deepsup')]),
           'scale': np.float64(u.SCALE)}
    for name, (seed, (B, C, h, w), deepsup, recipe) in u.CASES.items():
        scores, deep, label = u.draw_case(name)
        ties = check_ties(name, scores, label)
        r = u.reference(scores, deep, label, acc_fn=ACC_FN)
        r32 = u.reference(scores, deep, label, dtype=torch.float32, acc_fn=ACC_FN)
        assert np.array_equal(r['preds'], r32['preds']) and r['acc_sum'] == r32['acc_sum']
        p = name + '/'
        for key, a in (('scores8', scores), ('deepsup8', deep)):
            if a is not None:
                q = np.round(a.astype(np.float64) * 8)
                assert np.array_equal(q / 8, a) and np.abs(q).max() < 32767
                out[p + key] = q.astype(np.int16)
        out[p + 'seg_label'] = label
        for key in ('loss', 'loss_main', 'loss_deepsup'):
            out[p + key] = np.float64(r[key])
        out[p + 'acc'] = np.float32(r['acc'])
        assert np.float32(r['acc']) == u.acc_fp32(r['acc_sum'], r['pixel_sum'])
        for key in ('acc_sum', 'pixel_sum', 'bad'):
            out[p + key] = np.int64(r[key])
        for key in ('grad', 'grad_deepsup'):
            g = r[key]
            if g is None:
                continue
            assert g.dtype == np.float64
            if name in u.STORED_WHOLE:
                out[p + key] = g
            else:
                out[p + key + '_sample'] = g.reshape(-1)[::u.SAMPLE_STRIDE].copy()
                out[p + key + '_norm'] = np.float64(np.linalg.norm(g))
        # what the case is there for
        if recipe == 'mixed':
            assert r['bad'] > 0 and (label == C).any() and (label == -2).any() and (label[1] == -1).all()
            try:
                nn.NLLLoss(ignore_index=-1)(F.log_softmax(torch.as_tensor(scores), dim=1), torch.as_tensor(label))
                raise AssertionError('the reference did not raise on a label outside [-1, C)')
            except (IndexError, RuntimeError):
                pass
        else:
            assert r['bad'] == 0
        if recipe == 'ignored':
            assert np.isnan(r['loss']) and np.isnan(r['loss_main']) and r['acc'] == 0 and r['pixel_sum'] == 0
            assert not r['grad'].any() and not r['grad_deepsup'].any(), 'torch gives a non-zero gradient on an all-ignored batch'
        else:
            rel = lambda a, b: abs(a - b) / abs(b) if b else abs(a)
            g32 = np.linalg.norm(r32['grad'] - r['grad']) / max(np.linalg.norm(r['grad']), 1e-300)
            print('case %s: loss %.12g, acc %.6f (%d / %d), bad %d, %d ties; torch fp32 against float64: loss rel %.1e, gradient rel '
                  '2-norm %.1e' % (name, r['loss'], float(r['acc']), r['acc_sum'], r['pixel_sum'], r['bad'], ties,
                                   rel(r32['loss'], r['loss']), g32))
        if C == 1:
            assert r['loss'] == 0 and not r['grad'].any() and not r['grad_deepsup'].any()
    path = os.path.join(HERE, 'segm_loss_golden.npz')
    np.savez_compressed(path, **out)
    print('pixel_acc:', PIXEL_ACC)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == '__main__':
    main()
