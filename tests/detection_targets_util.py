"""Shared pieces of the detection targets' tests (tests/test_detection_targets_host.py, tests/test_gpu_detection_targets.py) and of the
fixture's generator (tests/golden/make_detection_targets_golden.py): the cases and their seeded inputs (not stored, only their
checksums) and a numpy restatement of the contract -- the reference's detection_target_layer (geometric/maskrcnn/model.py:545-724)
with bbox_overlaps (:508-542), utils.box_refinement (utils.py:92-113) and crop_and_resize.c, the two randperm calls replaced by the
order of the sampling keys (keys fp32 [2, N]: the candidates with the smallest keys, equal keys lower row first).

The generator runs the reference's own functions beside `contract` and asserts that they agree before it stores anything; the GPU
machine has the restatement and the fixture only.

What is float64 in the float64 form: box_refinement / std_dev, the crop boxes and the bilinear samples BEFORE rounding (all from the
float32 inputs), to measure how far the float32 run lies from exact values.  Everything that decides (IoU, arg-max, classes, order,
counts) is float32 in both forms.  In the float32 form every operation is a float32 numpy operation in the reference's order; log is
torch's, as in the reference's CPU run; the rounding is np.rint, half to even as torch.round."""
import functools
import os

import numpy as np
import torch

import proposal_layer_util as pu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'detection_targets_golden.npz')

MAX_ROIS, MAX_TARGETS, MAX_BOXES, MAX_MASK_SIDE = 8192, 8192, 128, 64   # csrc/detection_targets_check.h
STD_DEV = (0.1, 0.1, 0.2, 0.2)                                          # config.py: BBOX_STD_DEV
DRAW_GATE = 0.01      # the draw moves a positive proposal one of whose exact mask samples lies this close to 0.5; the generator then
                      # MEASURES the float32 run's error and asserts the smallest distance left against four times that
REPAIR_ROUNDS = 400
f32 = np.float32
OUTPUTS = ('rois', 'target_class_ids', 'target_deltas', 'target_mask', 'rows', 'assign', 'count', 'n_pos')
INPUTS = ('proposals', 'gt_class_ids', 'gt_boxes', 'gt_masks', 'keys')
checksum = pu.checksum


def _case(seed, N, G, R, ratio, mask=(28, 28), shape=(14, 14), mini=True, kind='objects', pos=0.4, jitter=0.12, ids='plain', roi_count=None):
    return dict(seed=seed, N=N, G=G, R=R, ratio=ratio, mask=mask, shape=shape, mini=mini, kind=kind, pos=pos, jitter=jitter, ids=ids,
                roi_count=roi_count)


CASES = {
    'n1': _case(9101, 1, 1, 8, 0.5, pos=1.0, jitter=0.05),
    'n63': _case(9102, 63, 7, 8, 0.5),                       # the sorting network's sizes round 64
    'n64': _case(9102, 64, 7, 8, 0.5),
    'n65': _case(9102, 65, 7, 8, 0.5),
    'n1025': _case(9105, 1025, 7, 200, 0.33),                # one lane with a second row
    'n8192': _case(9106, 8192, 128, 200, 0.33, pos=0.3),     # the limits of N and G
    'g100': _case(9107, 600, 100, 200, 0.33, pos=0.5),
    'r1100': _case(9108, 1500, 7, 1100, 0.5, mask=(8, 8), shape=(3, 2), pos=0.5),   # more output rows than lanes
    'ratio_one': _case(9109, 200, 7, 32, 1.0),
    'none_positive': _case(9110, 90, 7, 8, 0.5, kind='none_positive'),
    'no_negative': _case(9111, 40, 7, 64, 0.33, pos=1.0, jitter=0.04),
    'few_positive': _case(9112, 200, 7, 64, 0.33, pos=0.03),
    'few_negative': _case(9113, 100, 7, 64, 0.33, pos=0.92, jitter=0.06),
    'crowd': _case(9114, 200, 12, 64, 0.33, ids='crowd'),
    'crowd_with_zero_id': _case(9115, 200, 12, 64, 0.33, ids='crowd_zero'),
    'zero_id_no_crowd': _case(9116, 200, 6, 64, 0.33, ids='zero'),
    'only_crowd': _case(9117, 100, 5, 64, 0.33, ids='only_crowd'),
    'iou_half': _case(9118, 4, 1, 8, 0.5, mask=(9, 9), shape=(5, 5), kind='iou_half'),
    'tie_argmax': _case(9119, 6, 3, 8, 0.5, mask=(9, 9), shape=(5, 5), kind='tie_argmax'),
    'tie_keys': _case(9120, 200, 7, 64, 0.33, kind='tie_keys'),
    'nan_iou': _case(9121, 40, 4, 16, 0.5, mask=(9, 9), shape=(5, 5), kind='nan_iou'),
    'roi_count': _case(9122, 256, 7, 64, 0.33, roi_count=100, kind='roi_count'),
    'full_mask': _case(9123, 120, 5, 32, 0.33, mask=(40, 48), mini=False),
    'mask_7x9': _case(9124, 120, 5, 32, 0.33, shape=(7, 9)),
    'real': _case(9125, 2000, 24, 200, 0.33, mask=(56, 56), shape=(28, 28), pos=0.3),   # the reference's training sizes
}
TIMING = {'real_g100': _case(9126, 2000, 100, 200, 0.33, mask=(56, 56), shape=(28, 28), pos=0.3)}   # tools/time_detection_targets.py; not in the fixture
REFERENCE_RAISES = ('only_crowd',)   # the crowd filter leaves no box: the reference's bbox_overlaps fails on the empty tensor
EXPLICIT = ('iou_half', 'tie_argmax', 'nan_iou')   # dyadic boxes, masks of ones, 8 / 4 steps per sample: every fp32 operation but log is exact


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
def key_image(keys):
    """the usual order-preserving image of a float's bits (csrc/detection_targets_check.h: dt_image)"""
    bits = np.ascontiguousarray(keys, f32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def key_order(keys_row, rows):
    """the candidate rows in sampling order: ascending key image, equal keys lower row first (rows ascending; the sort is stable)"""
    return rows[np.argsort(key_image(keys_row[rows]), kind='stable')]


def negative_count(ratio, P):
    """model.py:669-670 as Python computes it"""
    r = 1.0 / ratio
    return int(r * P - P)


def overlaps(boxes1, boxes2):
    """bbox_overlaps (:508-542) in float32, operation by operation: [len(boxes1), len(boxes2)]"""
    a, b = boxes1.astype(f32)[:, None, :], boxes2.astype(f32)[None, :, :]
    with np.errstate(all='ignore'):
        y1, x1 = np.maximum(a[..., 0], b[..., 0]), np.maximum(a[..., 1], b[..., 1])     # np.maximum hands a NaN on, as torch.max
        y2, x2 = np.minimum(a[..., 2], b[..., 2]), np.minimum(a[..., 3], b[..., 3])
        inter = np.maximum(x2 - x1, f32(0)) * np.maximum(y2 - y1, f32(0))
        area1 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area2 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        union = area1 + area2 - inter
        return (inter / union).astype(f32)


def classes_of(c):
    """per proposal: (positive bool [N], negative bool [N], matched box among the G int [N], kept boxes bool [G])"""
    ids = c['gt_class_ids'].astype(np.int64)
    N, G = c['N'], c['G']
    crowd = bool((ids < 0).any())
    gt = (ids > 0) if crowd else np.ones(G, bool)
    idx = np.arange(N)
    limit = N if c['roi_count'] is None else min(max(int(c['roi_count']), 0), N)
    positive, negative, assign = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, np.int64)
    if not gt.any():
        return positive, negative, assign, gt
    ov = overlaps(c['proposals'], c['gt_boxes'][gt])
    kept = np.nonzero(gt)[0]
    assign = kept[np.argmax(ov, axis=1)]                      # the first maximum; a NaN is the maximum, the first NaN wins: torch.max
    with np.errstate(invalid='ignore'):
        best = np.max(ov, axis=1)                             # NaN where the row holds one
        positive = (best >= f32(0.5)) & (idx < limit)
        negative = (best < f32(0.5)) & (idx < limit)
        if crowd:
            negative &= np.max(overlaps(c['proposals'], c['gt_boxes'][ids < 0]), axis=1) < f32(0.001)
    return positive, negative, assign, gt


def select(c):
    """(rows of the positives taken, rows of the negatives taken, matched boxes of the positives), in output order"""
    positive, negative, assign, _gt = classes_of(c)
    cap = int(c['R'] * c['ratio'])
    pos = key_order(c['keys'][0], np.nonzero(positive)[0])[:cap]
    P = len(pos)
    want = min(negative_count(c['ratio'], P), c['R'] - P) if P > 0 else 0
    neg = key_order(c['keys'][1], np.nonzero(negative)[0])[:max(want, 0)]
    return pos, neg, assign[pos]


def refinement(rois, gt, std_dev, dtype):
    """utils.box_refinement / std_dev (:628-632) in dtype, operation by operation"""
    b, g = rois.astype(dtype), gt.astype(dtype)
    with np.errstate(all='ignore'):
        h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cy, cx = b[:, 0] + dtype(0.5) * h, b[:, 1] + dtype(0.5) * w
        gh, gw = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        gcy, gcx = g[:, 0] + dtype(0.5) * gh, g[:, 1] + dtype(0.5) * gw
        dy, dx = (gcy - cy) / h, (gcx - cx) / w
        rh, rw = np.ascontiguousarray(gh / h), np.ascontiguousarray(gw / w)
        if dtype is np.float32:
            dh, dw = torch.log(torch.from_numpy(rh)).numpy(), torch.log(torch.from_numpy(rw)).numpy()   # the reference's log on the CPU
        else:
            dh, dw = np.log(rh), np.log(rw)
        return (np.stack([dy, dx, dh, dw], 1) / np.asarray(std_dev, f32).astype(dtype)).astype(dtype)


def crop_boxes(rois, gt, mini, dtype):
    """:642-650: the roi in the frame of its box's mini-mask; without mini-masks the roi itself"""
    b, g = rois.astype(dtype), gt.astype(dtype)
    if not mini:
        return b
    with np.errstate(all='ignore'):
        gh, gw = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        return np.stack([(b[:, 0] - g[:, 0]) / gh, (b[:, 1] - g[:, 1]) / gw, (b[:, 2] - g[:, 0]) / gh, (b[:, 3] - g[:, 1]) / gw], 1).astype(dtype)


def _axis(a1, a2, extent, crop, dtype):
    """crop_and_resize.c:44-56: source coordinates [n, crop] along one axis (float / double mixing as written there)"""
    with np.errstate(all='ignore'):
        if crop > 1:
            scale = (a2 - a1) * dtype(extent - 1) / dtype(crop - 1)
            return (a1[:, None] * dtype(extent - 1) + np.arange(crop).astype(dtype)[None, :] * scale[:, None]).astype(dtype)
        return (0.5 * (a1 + a2).astype(np.float64) * (extent - 1)).astype(dtype)[:, None]


def crop_samples(masks, assign, boxes, H, W, dtype):
    """crop_and_resize.c:52-106 with extrapolation 0: the bilinear samples [n, H, W] of masks[assign] BEFORE rounding, in dtype"""
    boxes = boxes.astype(dtype)
    mh, mw = masks.shape[1:]
    n = len(assign)
    in_y, in_x = _axis(boxes[:, 0], boxes[:, 2], mh, H, dtype), _axis(boxes[:, 1], boxes[:, 3], mw, W, dtype)
    with np.errstate(invalid='ignore'):
        ok_y, ok_x = (in_y >= 0) & (in_y <= mh - 1), (in_x >= 0) & (in_x <= mw - 1)
    sy, sx = np.where(ok_y, in_y, 0), np.where(ok_x, in_x, 0)
    top, bottom, left, right = np.floor(sy).astype(int), np.ceil(sy).astype(int), np.floor(sx).astype(int), np.ceil(sx).astype(int)
    ly, lx = (sy - top).astype(dtype)[:, :, None], (sx - left).astype(dtype)[:, None, :]
    m = masks.astype(dtype)
    a = np.asarray(assign)[:, None, None]
    tl, tr = m[a, top[:, :, None], left[:, None, :]], m[a, top[:, :, None], right[:, None, :]]
    bl, br = m[a, bottom[:, :, None], left[:, None, :]], m[a, bottom[:, :, None], right[:, None, :]]
    t = tl + (tr - tl) * lx
    b = bl + (br - bl) * lx
    v = t + (b - t) * ly
    return np.where(ok_y[:, :, None] & ok_x[:, None, :], v, dtype(0)).astype(dtype).reshape(n, H, W)


def contract(c, dtype=np.float32):
    """the outputs of sdn_detection_targets (include/sdn_hip.h) for case c, plus 'pre_round': the positives' mask samples before
    rounding.  dtype float64: deltas and samples in float64 on the float32 run's selection."""
    R, (H, W) = c['R'], c['shape']
    pos, neg, assign = select(c)
    P, Q = len(pos), len(neg)
    out = dict(rois=np.zeros((R, 4), f32), target_class_ids=np.full(R, -1, np.int32), target_deltas=np.zeros((R, 4), dtype),
               target_mask=np.zeros((R, H, W), f32), rows=np.full(R, -1, np.int32), assign=np.full(R, -1, np.int32),
               count=np.array([P + Q], np.int32), n_pos=np.array([P], np.int32))
    taken = np.concatenate([pos, neg]).astype(int)
    out['rois'][:P + Q] = c['proposals'][taken]
    out['rows'][:P + Q] = taken
    out['target_class_ids'][:P] = c['gt_class_ids'][assign]
    out['target_class_ids'][P:P + Q] = 0
    out['assign'][:P] = assign
    rois, gt = c['proposals'][pos], c['gt_boxes'][assign]
    out['target_deltas'][:P] = refinement(rois, gt, c['std_dev'], dtype)
    pre = crop_samples(c['gt_masks'], assign, crop_boxes(rois, gt, c['mini'], dtype), H, W, dtype)
    out['pre_round'] = pre
    out['target_mask'][:P] = np.rint(pre).astype(f32)
    return out


def half_distance(pre):
    """the smallest distance of a sample from 0.5 (inf without samples)"""
    return float(np.abs(np.asarray(pre, np.float64) - 0.5).min()) if np.size(pre) else float('inf')


def pack_masks(masks):
    assert np.isin(masks, (0.0, 1.0)).all()
    return np.packbits(masks.astype(bool))


def unpack_masks(packed, shape):
    return np.unpackbits(packed)[:int(np.prod(shape))].reshape(shape).astype(f32)


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def _boxes(rs, n, lo=0.08, hi=0.4):
    h, w = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n)
    y1, x1 = rs.uniform(0, 1 - h), rs.uniform(0, 1 - w)
    return np.stack([y1, x1, y1 + h, x1 + w], 1).astype(f32)


def _jittered(rs, boxes, jitter):
    h, w = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    d = rs.uniform(-jitter, jitter, (len(boxes), 4)) * np.stack([h, w, h, w], 1)
    return (boxes + d).astype(f32)


def _mini_masks(rs, G, mh, mw):
    """binary masks of objects cropped to their boxes: an ellipse with a few flipped pixels"""
    yy, xx = (np.arange(mh) + 0.5) / mh - 0.5, (np.arange(mw) + 0.5) / mw - 0.5
    a, b = rs.uniform(0.3, 0.55, G), rs.uniform(0.3, 0.55, G)
    m = (yy[None, :, None] / a[:, None, None]) ** 2 + (xx[None, None, :] / b[:, None, None]) ** 2 < 1
    return (m ^ (rs.uniform(0, 1, m.shape) < 0.02)).astype(f32)


def _full_masks(rs, boxes, mh, mw):
    """binary masks over the whole image: an ellipse inside every box"""
    yy, xx = (np.arange(mh) + 0.5) / mh, (np.arange(mw) + 0.5) / mw
    cy, cx = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
    ry, rx = (boxes[:, 2] - boxes[:, 0]) / 2, (boxes[:, 3] - boxes[:, 1]) / 2
    m = ((yy[None, :, None] - cy[:, None, None]) / ry[:, None, None]) ** 2 + ((xx[None, None, :] - cx[:, None, None]) / rx[:, None, None]) ** 2 < 1
    return m.astype(f32)


def _ids(rs, G, how):
    ids = rs.randint(1, 6, G)
    if how in ('crowd', 'crowd_zero'):
        ids[rs.permutation(G)[:max(G // 4, 1)]] *= -1
    if how in ('zero', 'crowd_zero'):
        free = np.nonzero(ids > 0)[0]
        ids[free[:max(len(free) // 3, 1)]] = 0
    if how == 'only_crowd':
        ids = -ids
    return ids.astype(np.int32)


@functools.lru_cache(maxsize=None)
def draw_case(name):
    """the case's inputs; shared between tests, so read-only"""
    p = CASES[name] if name in CASES else TIMING[name]
    rs = np.random.RandomState(p['seed'])
    N, G, (mh, mw) = p['N'], p['G'], p['mask']
    c = dict(p, name=name, std_dev=STD_DEV)
    ones = np.ones((G, mh, mw), f32)
    if p['kind'] == 'iou_half':       # IoU exactly 0.5 is positive; just under is negative
        c['gt_boxes'] = np.array([[0, 0, 0.5, 0.5]], f32)
        c['proposals'] = np.array([[0, 0, 0.5, 0.25], [0, 0, 0.25, 0.5], [0, 0, 0.5, 0.249], [0.5, 0.5, 1, 1]], f32)
        c['gt_class_ids'], c['gt_masks'] = np.array([3], np.int32), ones
    elif p['kind'] == 'tie_argmax':   # boxes 0 and 1 are one box: the first wins
        c['gt_boxes'] = np.array([[0.25, 0.25, 0.75, 0.75], [0.25, 0.25, 0.75, 0.75], [0, 0, 0.125, 0.125]], f32)
        c['proposals'] = np.array([[0.25, 0.25, 0.75, 0.75], [0.25, 0.25, 0.75, 0.625], [0, 0, 0.125, 0.125], [0.875, 0.875, 1, 1],
                                   [0.25, 0.375, 0.75, 0.75], [0.5, 0, 0.625, 0.125]], f32)
        c['gt_class_ids'], c['gt_masks'] = np.array([2, 4, 5], np.int32), ones
    elif p['kind'] == 'nan_iou':      # a box and proposals of no area at one point: 0 / 0
        c['gt_boxes'] = np.array([[0.5, 0.5, 0.5, 0.5], [0, 0, 0.25, 0.25], [0.5, 0.5, 1, 1], [0.25, 0.5, 0.5, 0.75]], f32)
        pr = _boxes(rs, N)
        pr[::5] = (0.5, 0.5, 0.5, 0.5)
        pr[1::5] = np.array([0, 0, 0.25, 0.25], f32)
        pr[2::5] = np.array([0.5, 0.5, 1, 0.875], f32)
        c['proposals'], c['gt_class_ids'], c['gt_masks'] = pr, np.array([1, 2, 3, 4], np.int32), ones
    else:
        gt = _boxes(rs, G)
        if p['kind'] == 'none_positive':
            gt = (gt * f32(0.4)).astype(f32)                                  # boxes in one corner, proposals in the other
            pr = (_boxes(rs, N) * f32(0.4) + f32(0.55)).astype(f32)
            source = np.full(N, -1)
        else:
            source = np.where(rs.uniform(0, 1, N) < p['pos'], rs.randint(0, G, N), -1)
            pr = _boxes(rs, N, 0.04, 0.5)
            pr[source >= 0] = _jittered(rs, gt[source[source >= 0]], p['jitter'])
        if p['kind'] == 'roi_count':
            pr[p['roi_count']:] = gt[rs.randint(0, G, N - p['roi_count'])]   # the best rows there are lie behind the count
        c['gt_boxes'], c['proposals'], c['gt_class_ids'] = gt, pr, _ids(rs, G, p['ids'])
        c['gt_masks'] = _mini_masks(rs, G, mh, mw) if p['mini'] else _full_masks(rs, gt, mh, mw)
    keys = rs.uniform(0, 1, (2, N)).astype(f32)
    if p['kind'] == 'tie_keys':
        keys = (np.floor(keys * 4) / 4).astype(f32)
    if name == 'n1025':               # the one row of a lane's second pass is a positive and comes first
        c['proposals'][N - 1] = _jittered(rs, c['gt_boxes'][:1], 0.05)[0]
        keys[:, N - 1] = 0
    c['keys'] = keys
    if name not in EXPLICIT:
        _repair(c, rs)
    for k in INPUTS:
        c[k].setflags(write=False)
    return c


def _near_half(c):
    """positive candidates one of whose exact mask samples lies within DRAW_GATE of 0.5"""
    positive, _negative, assign, _gt = classes_of(c)
    rows = np.nonzero(positive)[0]
    if not len(rows):
        return rows
    pre = crop_samples(c['gt_masks'], assign[rows], crop_boxes(c['proposals'][rows], c['gt_boxes'][assign[rows]], c['mini'], np.float64),
                       c['shape'][0], c['shape'][1], np.float64)
    return rows[(np.abs(pre - 0.5).reshape(len(rows), -1).min(1) < DRAW_GATE)]


def _repair(c, rs):
    """move every positive candidate whose mask has a sample near 0.5: a new jitter of its matched box"""
    limit = c['N'] if c['roi_count'] is None else c['roi_count']
    for _ in range(REPAIR_ROUNDS):
        rows = _near_half(c)
        rows = rows[rows < limit]
        if not len(rows):
            return
        assign = classes_of(c)[2][rows]
        c['proposals'][rows] = _jittered(rs, c['gt_boxes'][assign], max(c['jitter'], 0.05))
    raise AssertionError('%s: the draw still has samples near 0.5 after %d rounds' % (c['name'], REPAIR_ROUNDS))
