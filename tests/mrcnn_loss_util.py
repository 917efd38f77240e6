"""Shared pieces of the Mask R-CNN loss tests (tests/test_mrcnn_loss_host.py, tests/test_gpu_mrcnn_loss.py) and of the fixture's
generator (tests/golden/make_mrcnn_loss_golden.py): the cases, their seeded inputs and a numpy / float64 restatement of the
reference's compute_losses (geometric/maskrcnn/model.py:1004-1147), of the sum of :1955 and of their gradients.  The generator
runs the reference's own functions beside the restatement and asserts that they agree before it stores anything; the GPU machine
has the restatement and the fixture only."""
import os
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mrcnn_loss_golden.npz')

CHUNK, STEP, QUAD = 1024, 256, 4     # csrc/mrcnn_loss_check.h: MRL_CHUNK, MRL_STEP, MRL_QUAD
GATE = 1e-6                          # tests/test_gpu_segm_loss.py's, of the float64 run
INPUTS = ('rpn_match', 'rpn_bbox', 'rpn_class_logits', 'rpn_pred_bbox', 'target_class_ids', 'mrcnn_class_logits', 'target_deltas',
          'mrcnn_bbox', 'target_mask', 'mrcnn_mask')
PREDICTIONS = ('rpn_class_logits', 'rpn_pred_bbox', 'mrcnn_class_logits', 'mrcnn_bbox', 'mrcnn_mask')   # the inputs with a gradient
LOSSES = ('rpn_class_loss', 'rpn_bbox_loss', 'mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss', 'loss')
COUNTS = ('n_rpn_valid', 'n_rpn_pos', 'n_roi_pos', 'bad')
# weights of the backward pass, d(total) / d(each of LOSSES): distinct, so that a swapped grad_out slot shows, and exact in fp32
WEIGHTS = (0.75, 1.25, 0.5, 1.5, 2.0, 0.25)
BCE_FLOOR = np.float64(np.float32(1e-12))   # torch keeps its 1e-12 as a float constant, in float64 runs too

# positives on both sides of every lane quad, step and chunk boundary of the kernel, the first anchor and the last
_BOUNDARY = (0, 3, 4, 7, 252, 255, 256, 259, 1020, 1023, 1024, 1027, 1279, 1280, 2047, 2048, 2049, 3071, 3072, 4095, 4096, 4999, 5000, 5002)

# name: seed, A, T, positives ('boundary', a number drawn at random, or 0), valid share, R, C, h, w, ids ('mixed', 'negative'), dtype
CASES = {
    # five chunks, A % 4 == 3; every kind of RoI; saturated mask probabilities; smooth-L1 differences of exactly +-1
    'chunks': dict(seed=5101, A=5003, T=64, pos='boundary', valid=0.3, R=13, C=3, h=28, w=28, ids='mixed', dtype=np.int32),
    # exactly two chunks, as many positives as target rows; one RoI of 81 classes; int64
    'exact': dict(seed=5102, A=2048, T=7, pos=7, valid=0.2, R=1, C=81, h=28, w=28, ids='mixed', dtype=np.int64),
    # less than one chunk, no positive anchor: rpn_bbox_loss is NaN; 200 RoIs, two classes, an odd plane
    'nopos': dict(seed=5103, A=1000, T=4, pos=0, valid=0.5, R=200, C=2, h=5, w=7, ids='mixed', dtype=np.int32),
    # no valid anchor at all: rpn_class_loss is NaN too; every RoI negative: the box and mask losses are NaN
    'novalid': dict(seed=5104, A=300, T=4, pos=0, valid=0.0, R=13, C=3, h=5, w=7, ids='negative', dtype=np.int64),
    # no RoI was sampled: the head losses are 0
    'empty': dict(seed=5105, A=777, T=8, pos=5, valid=0.4, R=0, C=0, h=0, w=0, ids='mixed', dtype=np.int32),
}
STORED_WHOLE = ('nopos', 'novalid', 'empty')   # cases whose inputs the fixture holds in full; the others by checksum


def draw(seed, A, T, pos, valid, R, C, h, w, ids, dtype, scale=2.0):
    """the ten arguments of compute_losses as numpy arrays, from numpy's frozen RandomState stream"""
    rs = np.random.RandomState(seed)
    match = np.where(rs.rand(A) < valid, -1, 0)
    if pos == 'boundary':
        where = np.unique(np.concatenate([[a for a in _BOUNDARY if a < A] + [A - 1], rs.choice(A, 12, replace=False)]))
    else:
        where = np.sort(rs.choice(A, pos, replace=False)) if pos else np.zeros(0, np.int64)
    match[where] = 1
    c = {'rpn_match': match.astype(dtype).reshape(1, A, 1)}
    # targets on a grid of 1 / 8: a prediction can sit exactly 1 away
    c['rpn_bbox'] = (np.round(rs.randn(1, T, 4) * 8.0) / 8.0).astype(np.float32)
    c['rpn_class_logits'] = (rs.randn(1, A, 2) * scale).astype(np.float32)
    pred = (rs.randn(1, A, 4) * 1.5).astype(np.float32)
    n = min(len(where), T)
    if n >= 2:   # the first positive exactly +1 from its target, the last used one exactly -1
        pred[0, where[0]] = c['rpn_bbox'][0, 0] + np.float32(1.0)
        pred[0, where[n - 1]] = c['rpn_bbox'][0, n - 1] - np.float32(1.0)
    c['rpn_pred_bbox'] = pred
    if R == 0:   # what predict(..., mode='training') returns when no RoI was sampled (model.py:1803-1812)
        c['target_class_ids'] = np.zeros(0, dtype)
        for k in INPUTS[5:]:
            c[k] = np.zeros(0, np.float32)
        return c
    cls = rs.randint(0, C, R) if ids == 'mixed' else np.zeros(R, np.int64)
    if ids == 'mixed':
        cls[0] = C - 1       # at least one positive RoI, of the last class
        if R > 2:
            cls[1], cls[R - 1] = 0, 1
    c['target_class_ids'] = cls.astype(dtype)
    c['mrcnn_class_logits'] = (rs.randn(R, C) * scale).astype(np.float32)
    c['target_deltas'] = (np.round(rs.randn(R, 4) * 8.0) / 8.0).astype(np.float32)
    bbox = (rs.randn(R, C, 4) * 1.5).astype(np.float32)
    bbox[0, cls[0], :2] = c['target_deltas'][0, :2] + np.float32(1.0)
    bbox[0, cls[0], 2:] = c['target_deltas'][0, 2:] - np.float32(1.0)
    c['mrcnn_bbox'] = bbox
    c['target_mask'] = (rs.rand(R, h, w) < 0.4).astype(np.float32)
    mask = (1.0 / (1.0 + np.exp(-rs.randn(R, C, h, w) * 2.0))).astype(np.float32)
    # probabilities of exactly 0 and 1 against both targets in the first positive RoI's plane: the clamp at -100 and the 1e-12 floor
    mask[0, cls[0], 0, :4] = (0.0, 1.0, 0.0, 1.0)
    c['target_mask'][0, 0, :4] = (0.0, 0.0, 1.0, 1.0)
    c['mrcnn_mask'] = mask
    return c


def draw_case(name):
    return draw(**CASES[name])


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def _mean(total, n):
    """torch's mean: NaN over nothing"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64(total) / np.float64(n)


def _cross_entropy(x, label):
    """(the sum of lse - x[label] over the rows, d sum / d x)"""
    m = x.max(axis=1, keepdims=True) if x.shape[0] else x[:, :1]
    lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
    rows = np.arange(x.shape[0])
    grad = np.exp(x - lse[:, None])
    grad[rows, label] -= 1.0
    return (lse - x[rows, label]).sum(), grad, lse


def _smooth_l1(d):
    z = np.abs(d)
    return np.where(z < 1.0, 0.5 * z * z, z - 0.5).sum(), np.clip(d, -1.0, 1.0)


def _bce(p, y):
    with np.errstate(invalid='ignore', divide='ignore'):
        l1, l0 = np.log(p), np.log1p(-p)
        l1 = np.where(l1 < -100.0, -100.0, l1)          # a NaN stays
        l0 = np.where(l0 < -100.0, -100.0, l0)
        return ((y - 1.0) * l0 - y * l1).sum(), (p - y) / np.maximum((1.0 - p) * p, BCE_FLOOR)


def reference(c, weights=WEIGHTS):
    """compute_losses in float64 with the device's rules for what the reference leaves undefined (counted in `bad`).  Returns a
    dict: the six LOSSES (Python floats), the four COUNTS, 'grad': {prediction: float64 array, or None for R = 0} of
    sum(weights[k] * LOSSES[k]), 'n': the element count each loss is a mean over, and 'selected': {prediction: bool mask}."""
    w = [np.float64(np.float32(v)) for v in weights]
    match = c['rpn_match'].reshape(-1).astype(np.int64)
    A, T = match.shape[0], c['rpn_bbox'].shape[1]
    bad = int((~np.isin(match, (-1, 0, 1))).sum())
    valid = (match == 1) | (match == -1)
    positives = np.nonzero(match == 1)[0]
    used = positives[:T]
    bad += len(positives) - len(used)
    grad, sel, n, loss = {}, {}, {}, {}

    x = c['rpn_class_logits'].reshape(A, 2).astype(np.float64)
    s, g, _ = _cross_entropy(x[valid], (match[valid] == 1).astype(np.int64))
    n[0] = int(valid.sum())
    loss[0] = _mean(s, n[0])
    grad[0] = np.zeros((A, 2))
    if n[0]:
        grad[0][valid] = g * ((w[0] + w[5]) / n[0])
    sel[0] = np.repeat(valid[:, None], 2, axis=1)

    d = c['rpn_pred_bbox'].reshape(A, 4).astype(np.float64)[used] - c['rpn_bbox'].reshape(T, 4).astype(np.float64)[:len(used)]
    s, g = _smooth_l1(d)
    n[1] = 4 * len(used)
    loss[1] = _mean(s, n[1])
    grad[1] = np.zeros((A, 4))
    if n[1]:
        grad[1][used] = g * ((w[1] + w[5]) / n[1])
    sel[1] = np.zeros((A, 4), bool)
    sel[1][used] = True

    R = c['target_class_ids'].shape[0]
    if R == 0:
        for k in (2, 3, 4):
            loss[k], n[k], grad[k], sel[k] = 0.0, 0, None, None
        n_roi_pos = 0
    else:
        ids = c['target_class_ids'].astype(np.int64)
        C = c['mrcnn_class_logits'].shape[1]
        ok = (ids >= 0) & (ids < C)
        bad += int((~ok).sum())
        pos = np.nonzero(ok & (ids > 0))[0]
        n_roi_pos = len(pos)
        x = c['mrcnn_class_logits'].astype(np.float64)
        s, g, _ = _cross_entropy(x[ok], ids[ok])
        n[2] = int(ok.sum())
        loss[2] = _mean(s, n[2])
        grad[2] = np.zeros(x.shape)
        if n[2]:
            grad[2][ok] = g * ((w[2] + w[5]) / n[2])
        sel[2] = np.repeat(ok[:, None], C, axis=1)

        bb = c['mrcnn_bbox'].astype(np.float64)
        s, g = _smooth_l1(bb[pos, ids[pos]] - c['target_deltas'].astype(np.float64)[pos])
        n[3] = 4 * n_roi_pos
        loss[3] = _mean(s, n[3])
        grad[3] = np.zeros(bb.shape)
        sel[3] = np.zeros(bb.shape, bool)
        if n[3]:
            grad[3][pos, ids[pos]] = g * ((w[3] + w[5]) / n[3])
        sel[3][pos, ids[pos]] = True

        pm = c['mrcnn_mask'].astype(np.float64)
        s, g = _bce(pm[pos, ids[pos]], c['target_mask'].astype(np.float64)[pos])
        n[4] = n_roi_pos * pm.shape[2] * pm.shape[3]
        loss[4] = _mean(s, n[4])
        grad[4] = np.zeros(pm.shape)
        sel[4] = np.zeros(pm.shape, bool)
        if n[4]:
            grad[4][pos, ids[pos]] = g * ((w[4] + w[5]) / n[4])
        sel[4][pos, ids[pos]] = True

    res = {k: float(loss[i]) for i, k in enumerate(LOSSES[:5])}
    res['loss'] = float(loss[0] + loss[1] + loss[2] + loss[3] + loss[4])
    res.update(n_rpn_valid=n[0], n_rpn_pos=len(used), n_roi_pos=n_roi_pos, bad=bad)
    res['grad'] = {k: (grad[i].reshape(c[k].shape) if grad[i] is not None else None) for i, k in enumerate(PREDICTIONS)}
    res['selected'] = {k: (sel[i].reshape(c[k].shape) if sel[i] is not None else None) for i, k in enumerate(PREDICTIONS)}
    res['n'] = {k: n[i] for i, k in enumerate(PREDICTIONS)}
    return res


def grad_error(got, want, n):
    """the largest |got - want| / max(|want|, 1 / n) over the elements: the gate's measure (0 for an empty selection)"""
    if want.size == 0:
        return 0.0
    scale = np.maximum(np.abs(want), 1.0 / max(n, 1))
    return float((np.abs(np.asarray(got, np.float64) - want) / scale).max())


def sparse(a):
    """(flat indices of the non-zero elements int32, their values): how the fixture holds a gradient"""
    flat = a.reshape(-1)
    idx = np.nonzero(flat)[0]
    return idx.astype(np.int32), flat[idx]


def dense(idx, values, shape):
    out = np.zeros(int(np.prod(shape)), np.float64)
    out[idx] = values
    return out.reshape(shape)
