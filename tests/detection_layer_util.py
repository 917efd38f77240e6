"""Shared pieces of the detection layer's tests (tests/test_detection_layer_host.py, tests/test_gpu_detection_layer.py) and of the
fixture's generator (tests/golden/make_detection_layer_golden.py): the cases and their seeded inputs (not stored, only their
checksums) and two numpy restatements of the contract -- the reference's refine_detections (geometric/maskrcnn/model.py:744-837,
apply_box_deltas :307-328, clip_to_window :731-741) with the NMS of nms/pth_nms.py on nms/src/nms.c.

  contract         the reference's way: validity, a loop over the classes present, per class a stable sort and an NMS, the union, the
                   intersect, a final stable sort cut to D.
  contract_global  the kernel's way (csrc/detection_layer.hip): ONE order of the valid rows by (score descending, row ascending), a
                   greedy scan whose pair test also requires equal class ids, stopped at D.
tests/test_detection_layer_host.py asserts the two equal on every case: a row's fate in a per-class NMS depends only on the kept
rows of its class before it, the global order holds every class's rows in their per-class order, and the best D of the kept rows by
score are the first D the scan keeps.

The generator runs the reference's own functions beside `contract` and asserts that they agree before it stores anything; the GPU
machine has the restatements and the fixture only.

What is float64 in the float64 form: the decode, the scale and the clip (from the float32 inputs), to measure how far the float32
run's coordinates lie from exact ones BEFORE rounding.  Everything that decides (arg-max, validity, order, NMS) is float32 on the
float32 run's rounded boxes.  In the float32 form every operation is a float32 numpy operation in the reference's order; exp is torch's,
as in the reference's CPU run; the rounding is np.rint, half to even as torch.round."""
import functools
import os

import numpy as np
import torch

import proposal_layer_util as pu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'detection_layer_golden.npz')

MAX_ROIS, MAX_INSTANCES = 8192, 8192                       # csrc/detection_layer_check.h: DET_MAX_ROIS, DET_MAX_INSTANCES
STD_DEV = (0.1, 0.1, 0.2, 0.2)                             # config.py: RPN_BBOX_STD_DEV
DRAW_GATE = 0.01           # px: the draw moves a row whose exact coordinate lies this close to k + 0.5; the generator then MEASURES the
                           # float32 run's error and asserts the smallest distance left against four times that (about 1e-3 px at 1024)
REPAIR_ROUNDS = 12
f32 = np.float32
OUTPUTS = ('class_ids', 'scores', 'boxes_px', 'keep', 'count', 'detections', 'boxes_norm')
checksum = pu.checksum

# name: seed, rows N, classes C, image (height, width), window, min_confidence, threshold, max_instances D, how it is drawn
_W128, _W256 = (0, 0, 128, 128), (0, 0, 256, 256)
CASES = {
    'one': dict(seed=8101, N=1, C=2, image=(128, 128), window=_W128, conf=0.7, thr=0.3, D=3, kind='allfg'),
    'words63': dict(seed=8102, N=63, C=3, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=30, kind='allfg'),   # the mask's word edges
    'words64': dict(seed=8102, N=64, C=3, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=30, kind='allfg'),
    'words65': dict(seed=8102, N=65, C=3, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=30, kind='allfg'),
    'real_c3': dict(seed=8105, N=1000, C=3, image=(1024, 1024), window=(128, 0, 896, 1024), conf=0.7, thr=0.3, D=100, kind='objects'),
    'real_c81': dict(seed=8106, N=1000, C=81, image=(1024, 1024), window=(128, 0, 896, 1024), conf=0.7, thr=0.3, D=100, kind='objects'),
    'cross_class': dict(seed=8107, N=6, C=7, image=(64, 64), window=(0, 0, 64, 64), conf=0.7, thr=0.3, D=10, kind='cross_class'),
    'same_class': dict(seed=8107, N=6, C=2, image=(64, 64), window=(0, 0, 64, 64), conf=0.7, thr=0.3, D=10, kind='same_class'),
    'all_background': dict(seed=8109, N=70, C=3, image=(128, 128), window=_W128, conf=0.7, thr=0.3, D=10, kind='all_background'),
    'C1': dict(seed=8110, N=40, C=1, image=(128, 128), window=_W128, conf=0.7, thr=0.3, D=10, kind='random'),
    'below_conf': dict(seed=8111, N=90, C=4, image=(128, 128), window=_W128, conf=0.7, thr=0.3, D=10, kind='below_conf'),
    'no_min_conf': dict(seed=8112, N=90, C=4, image=(128, 128), window=_W128, conf=0.0, thr=0.3, D=80, kind='below_conf'),
    'top_d': dict(seed=8113, N=200, C=3, image=(512, 512), window=(0, 0, 512, 512), conf=0.7, thr=0.3, D=5, kind='disjoint'),
    'few': dict(seed=8114, N=150, C=4, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=100, kind='random'),
    'D1': dict(seed=8114, N=150, C=4, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=1, kind='random'),
    'roi_count': dict(seed=8116, N=256, C=4, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=100, kind='allfg', roi_count=100),
    'window': dict(seed=8117, N=300, C=3, image=(320, 480), window=(40, 60, 280, 420), conf=0.5, thr=0.5, D=100, kind='random'),
    'halves': dict(seed=8118, N=128, C=3, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=100, kind='halves'),
    'ties_score': dict(seed=8119, N=160, C=4, image=(256, 256), window=_W256, conf=0.7, thr=0.3, D=100, kind='ties_score'),
    'tie_iou': dict(seed=8120, N=6, C=2, image=(64, 64), window=(0, 0, 64, 64), conf=0.3, thr=0.5, D=6, kind='tie_iou'),
    'argmax_tie': dict(seed=8121, N=80, C=5, image=(128, 128), window=_W128, conf=0.3, thr=0.3, D=50, kind='argmax_tie'),
    'nan_row': dict(seed=8122, N=80, C=5, image=(128, 128), window=_W128, conf=0.7, thr=0.3, D=50, kind='nan_row'),
    'overflow': dict(seed=8123, N=64, C=3, image=(128, 128), window=_W128, conf=0.7, thr=0.3, D=10, kind='overflow'),
}
REFERENCE_RAISES = ('all_background', 'C1', 'below_conf')   # no row is a detection: the reference never binds nms_keep (:824)
NO_REFERENCE = REFERENCE_RAISES + ('ties_score',)            # ties_score: the reference's sorts are unstable; stored from the restatement
ROWS_ONLY = ('overflow',)                                    # NaN boxes: only class_ids, scores and boxes_px are compared
EXACT = ('halves', 'tie_iou', 'cross_class', 'same_class')   # zero deltas on dyadic coordinates: every fp32 operation is exact
ON_HALVES = ('halves',)                                      # built ON k + 0.5: exempt from the margin, float32 == float64 instead


def decode(rois, deltas, std_dev, height, width, window, dtype=np.float64):
    """model.py:775 (:313-326), :782, :736-739 on the given rows, operation by operation in `dtype`: the coordinates BEFORE rounding"""
    a, d = rois.astype(dtype), deltas.astype(dtype) * np.asarray(std_dev, f32).astype(dtype)
    with np.errstate(all='ignore'):
        h, w = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cy, cx = a[:, 0] + dtype(0.5) * h, a[:, 1] + dtype(0.5) * w
        cy, cx = cy + d[:, 0] * h, cx + d[:, 1] * w
        if dtype is np.float32:
            e = torch.exp(torch.from_numpy(np.ascontiguousarray(d[:, 2:4]))).numpy()       # the reference's exp on the CPU
        else:
            e = np.exp(d[:, 2:4])
        h, w = h * e[:, 0], w * e[:, 1]
        y1, x1 = cy - dtype(0.5) * h, cx - dtype(0.5) * w
        y2, x2 = y1 + h, x1 + w
        scale = (dtype(height), dtype(width), dtype(height), dtype(width))
        cols = [v * s for v, s in zip((y1, x1, y2, x2), scale)]
        win = [dtype(f32(v)) for v in window]
        lims = ((win[0], win[2]), (win[1], win[3]), (win[0], win[2]), (win[1], win[3]))
        cols = [np.where(v < lo, lo, np.where(v > hi, hi, v)) for v, (lo, hi) in zip(cols, lims)]      # torch.clamp: NaN stays
    return np.stack(cols, 1).astype(dtype)


def rows_of(c, dtype=np.float32):
    """the per-row half of the contract: (class_ids int32 [N], scores float32 [N], coordinates before rounding [N, 4] in dtype,
    valid bool [N])"""
    probs = c['probs']
    class_ids = np.argmax(probs, axis=1).astype(np.int32)          # first maximum; a NaN is the maximum, the first NaN wins: torch.max
    idx = np.arange(c['N'])
    scores = probs[idx, class_ids]
    pre = decode(c['rois'], c['deltas'][idx, class_ids], c['std_dev'], c['image'][0], c['image'][1], c['window'], dtype)
    limit = c['N'] if c['roi_count'] is None else min(max(int(c['roi_count']), 0), c['N'])
    valid = (idx < limit) & (class_ids > 0)                        # :793
    if c['conf']:                                                  # :796: a falsy value switches the filter off
        with np.errstate(invalid='ignore'):
            valid = valid & (scores >= f32(c['conf']))
    return class_ids, scores, pre, valid


def suppress_row(b, areas, i, thr, strict):
    """which of the boxes behind place i box i suppresses: nms.c:51-59, strict: the CUDA kernel's `>`"""
    ovr = pu.iou_rows(b, areas, i, i + 1)
    with np.errstate(invalid='ignore'):
        return (ovr > f32(thr)) if strict else (ovr >= f32(thr))


def _descending(scores):
    """stable order by descending score, NaN above +inf: torch.sort(descending=True, stable=True)"""
    return np.argsort(-(pu.score_image(scores).astype(np.int64)), kind='stable')


def keep_per_class(class_ids, scores, boxes32, valid, thr, D, strict):
    """:798-829, the reference's way"""
    keep = np.nonzero(valid)[0]
    if not len(keep):
        return np.zeros(0, np.int32)
    pre_cls, pre_scores, pre_rois = class_ids[keep], scores[keep], boxes32[keep]
    nms_keep = None
    for class_id in np.unique(pre_cls):
        ixs = np.nonzero(pre_cls == class_id)[0]
        order = _descending(pre_scores[ixs])
        class_keep = pu.nms(pre_rois[ixs][order], thr, strict)
        class_keep = keep[ixs[order[class_keep]]]
        nms_keep = class_keep if nms_keep is None else np.union1d(nms_keep, class_keep)
    keep = np.intersect1d(keep, nms_keep)
    top = _descending(scores[keep])[:D]
    return keep[top].astype(np.int32)


def keep_global(class_ids, scores, boxes32, valid, thr, D, strict):
    """the kernel's way: one order, the class test in the pair mask, stop at D"""
    rows = np.nonzero(valid)[0]
    rows = rows[_descending(scores[rows])]               # rows ascending among equal scores: the sort is stable
    b = np.ascontiguousarray(boxes32[rows], f32)
    cls = class_ids[rows]
    areas = pu.areas_of(b)
    dead = np.zeros(len(rows), bool)
    keep = []
    for i in range(len(rows)):
        if dead[i]:
            continue
        keep.append(rows[i])
        if len(keep) == D:
            break
        dead[i + 1:] |= suppress_row(b, areas, i, thr, strict) & (cls[i + 1:] == cls[i])
    return np.asarray(keep, np.int32)


def _assemble(c, class_ids, scores, boxes, keep):
    D = c['D']
    H, W = c['image']
    n = len(keep)
    detections, boxes_norm = np.zeros((D, 6), f32), np.zeros((D, 4), f32)
    keep_padded = np.full(D, -1, np.int32)
    keep_padded[:n] = keep
    b32 = boxes.astype(f32)
    detections[:n, :4] = b32[keep]
    detections[:n, 4] = class_ids[keep].astype(f32)            # :834
    detections[:n, 5] = scores[keep]
    with np.errstate(all='ignore'):
        boxes_norm[:n] = b32[keep] / np.asarray([H, W, H, W], f32)      # :1769
    return dict(class_ids=class_ids, scores=scores.astype(f32), boxes_px=boxes, keep=keep_padded, count=np.asarray([n], np.int32),
                detections=detections, boxes_norm=boxes_norm)


def _contract(c, dtype, strict, keeper):
    class_ids, scores, pre32, valid = rows_of(c, np.float32)
    boxes32 = np.rint(pre32)                                       # :788 torch.round: half to even
    keep = keeper(class_ids, scores, boxes32, valid, c['thr'], c['D'], strict)
    out = _assemble(c, class_ids, scores, boxes32, keep)
    out['pre_round'] = pre32 if dtype is np.float32 else rows_of(c, dtype)[2]
    return out


def contract(c, dtype=np.float32, strict=True):
    """The contract on a drawn case, the reference's way: the seven outputs (padded as the device pads them) and `pre_round`, the
    coordinates before rounding in `dtype`.  Everything but pre_round always comes from the float32 run."""
    return _contract(c, dtype, strict, keep_per_class)


def contract_global(c, dtype=np.float32, strict=True):
    """the same, the kernel's way"""
    return _contract(c, dtype, strict, keep_global)


def half_distance(pre):
    """the smallest distance of a finite coordinate from k + 0.5 (inf when there is none)"""
    v = np.asarray(pre, np.float64)
    v = v[np.isfinite(v)]
    return float(np.abs(v - np.floor(v) - 0.5).min()) if v.size else np.inf


def pairs_on_threshold(class_ids, boxes32, valid, thr):
    """same-class pairs of valid rows whose fp32 IoU equals the threshold"""
    rows = np.nonzero(valid)[0]
    b, cls = np.ascontiguousarray(boxes32[rows], f32), class_ids[rows]
    areas = pu.areas_of(b)
    n = 0
    for i in range(len(rows) - 1):
        ovr = pu.iou_rows(b, areas, i, i + 1)
        n += int(((ovr == f32(thr)) & (cls[i + 1:] == cls[i])).sum())
    return n


def _boxes(rs, N, H, W, lo=10.0):
    h, w = np.exp(rs.uniform(np.log(lo), np.log(0.5 * H), N)), np.exp(rs.uniform(np.log(lo), np.log(0.5 * W), N))
    cy, cx = rs.uniform(0.05 * H, 0.95 * H, N), rs.uniform(0.05 * W, 0.95 * W, N)
    return np.stack([(cy - h / 2) / H, (cx - w / 2) / W, (cy + h / 2) / H, (cx + w / 2) / W], 1)


def _probs(rs, N, C, winner, top):
    """rows whose class `winner` holds `top` and whose other classes share the rest at random"""
    p = np.zeros((N, C))
    if C > 1:
        rest = rs.dirichlet(np.ones(C - 1), N) * (1.0 - top)[:, None]
        for i in range(N):
            p[i, np.arange(C) != winner[i]] = rest[i]
    p[np.arange(N), winner] = top
    return p


def _px(boxes, H, W):
    return np.asarray(boxes, np.float64) / np.asarray([H, W, H, W], np.float64)


def _draw(rs, k):
    """(rois [N, 4], probs [N, C], deltas [N, C, 4]) float32, before any repair"""
    N, C, (H, W), kind = k['N'], k['C'], k['image'], k['kind']
    rois = _boxes(rs, N, H, W)
    deltas = rs.normal(0, 1.0, (N, C, 4))
    winner = rs.randint(0, C, N) if C > 1 else np.zeros(N, np.int64)
    top = rs.uniform(0.45, 0.999, N)
    if kind == 'random':
        pass
    elif kind == 'allfg':          # every row a confident foreground row: M = N
        winner = rs.randint(1, C, N)
        top = rs.uniform(0.75, 0.999, N)
    elif kind == 'objects':        # rows scattered round a few objects, as a classifier head sees proposals: two in five of them background
        n_obj = 24
        ob = _boxes(rs, n_obj, H, W, lo=40.0)
        ob_cls = rs.randint(1, C, n_obj)
        which = rs.randint(0, n_obj, N)
        size = np.stack([ob[which, 2] - ob[which, 0], ob[which, 3] - ob[which, 1]], 1)
        rois = ob[which] + rs.normal(0, 0.12, (N, 4)) * np.tile(size, 2)
        rois = np.stack([np.minimum(rois[:, 0], rois[:, 2] - 4.0 / H), np.minimum(rois[:, 1], rois[:, 3] - 4.0 / W), rois[:, 2], rois[:, 3]], 1)
        fg = rs.uniform(0, 1, N) < 0.62
        stray = rs.uniform(0, 1, N) < 0.15                         # a neighbouring class now and then
        winner = np.where(fg, np.where(stray, rs.randint(1, C, N), ob_cls[which]), 0)
        top = rs.uniform(0.45, 0.999, N)
    elif kind in ('cross_class', 'same_class'):                   # identical boxes on whole pixels, zero deltas
        rois = np.tile(_px([[10, 12, 40, 50]], H, W), (N, 1))
        deltas[:] = 0
        winner = 1 + np.arange(N) if kind == 'cross_class' else np.ones(N, np.int64)
        top = 0.95 - 0.03 * np.arange(N)
    elif kind == 'all_background':
        winner[:] = 0
    elif kind == 'below_conf':     # foreground rows under 0.7, background rows above it
        top = np.where(winner > 0, rs.uniform(0.45, 0.69, N), rs.uniform(0.7, 0.99, N))
    elif kind == 'disjoint':       # a grid of 24 px boxes 36 px apart, moved by about a pixel: nothing suppressed
        gy, gx = np.divmod(np.arange(N), 14)
        rois = _px(np.stack([gy * 36 + 4, gx * 36 + 4, gy * 36 + 28, gx * 36 + 28], 1), H, W)
        deltas = rs.normal(0, 0.3, (N, C, 4))
        winner = rs.randint(1, C, N)
        top = rs.uniform(0.75, 0.999, N)
    elif kind == 'halves':         # corners on k + 0.5 pixels of a 256 px image, k even and odd; zero deltas
        y1, x1 = rs.randint(0, 100, N), rs.randint(0, 100, N)
        y2, x2 = y1 + rs.randint(8, 120, N), x1 + rs.randint(8, 120, N)
        rois = _px(np.stack([y1, x1, y2, x2], 1) + 0.5, H, W)
        deltas[:] = 0
        winner = rs.randint(1, C, N)
        top = rs.uniform(0.75, 0.999, N)
    elif kind == 'ties_score':     # five score values shared by all rows, within and across classes
        winner = rs.randint(1, C, N)
        top = np.asarray([0.75, 0.8125, 0.875, 0.9375, 0.96875])[rs.randint(0, 5, N)]
    elif kind == 'tie_iou':        # areas 100 and 50 under the +1 convention, intersection 50: IoU = 0.5 exactly
        rois = _px([[0, 0, 9, 9], [0, 0, 9, 4], [30, 30, 50, 50], [31, 31, 50, 50], [5, 40, 25, 60], [40, 5, 60, 25]], H, W)
        deltas[:] = 0
        winner = np.ones(N, np.int64)
        top = np.asarray([0.9, 0.85, 0.8, 0.75, 0.7, 0.65])
    elif kind in ('argmax_tie', 'nan_row', 'overflow'):
        winner = rs.randint(1, C, N)
        top = rs.uniform(0.75, 0.999, N)
    else:
        raise KeyError(kind)
    probs = _probs(rs, N, C, winner, top).astype(f32)
    rois, deltas = rois.astype(f32), deltas.astype(f32)
    if kind == 'argmax_tie':       # the maximum twice or three times in a row: the first index wins, which is class 0 in every third
        for i in range(N):
            m = probs[i].max()
            probs[i] = rs.uniform(0.0, 0.1, C).astype(f32)
            first = 0 if i % 3 == 0 else int(rs.randint(1, C - 1))
            probs[i, first] = m
            probs[i, rs.randint(first + 1, C)] = m
            if i % 5 == 0:
                probs[i, C - 1] = m
    elif kind == 'nan_row':        # every fourth row: one NaN, or two, before or behind the largest number
        for i in range(0, N, 4):
            probs[i, rs.randint(0, C)] = np.nan
            if i % 8 == 0:
                probs[i, rs.randint(0, C)] = -np.nan
    elif kind == 'overflow':
        idx = np.arange(N)
        cls = np.argmax(probs, 1)
        deltas[idx[0::4], cls[0::4], 2] = 5000.0      # exp = inf, in float64 too: h = inf, y1 = -inf, y2 = -inf + inf = NaN
        deltas[idx[1::4], cls[1::4], 3] = 4000.0
        deltas[idx[2::8], cls[2::8], 2] = -2000.0     # exp = 0: h = 0
        rois[5] = (0.25, 0.25, 0.25, 0.5)             # h = 0 and exp = inf: 0 * inf = NaN
        deltas[5, cls[5], 2] = 5000.0
    return rois, probs, deltas


@functools.lru_cache(maxsize=None)
def draw_case(name):
    """The inputs of a case, float32: rois [N, 4], probs [N, C], deltas [N, C, 4], and its parameters.  The draw repairs itself, the same
    way every time: while a row's exact (float64) coordinate lies within DRAW_GATE px of k + 0.5 before rounding, the deltas of its
    class are moved by a fresh draw (not in the EXACT cases, whose coordinates are exact by construction, and not in `overflow`)."""
    k = CASES[name]
    rs = np.random.RandomState(k['seed'])
    rois, probs, deltas = _draw(rs, k)
    c = dict(name=name, rois=rois, probs=probs, deltas=deltas, std_dev=STD_DEV, image=k['image'], window=k['window'], N=k['N'], C=k['C'],
             D=k['D'], conf=k['conf'], thr=k['thr'], roi_count=k.get('roi_count'))
    if name not in EXACT and name not in ROWS_ONLY:
        idx = np.arange(k['N'])
        cls = np.argmax(probs, 1)
        for _ in range(REPAIR_ROUNDS):
            pre = rows_of(c, np.float64)[2]
            near = np.abs(pre - np.floor(pre) - 0.5) < DRAW_GATE
            bad = idx[near.any(1)]
            if not len(bad):
                break
            deltas[bad, cls[bad]] = (deltas[bad, cls[bad]].astype(np.float64) + rs.normal(0, 0.25, (len(bad), 4))).astype(f32)
        else:
            raise AssertionError('%s: a coordinate within %g px of a half after %d rounds' % (name, DRAW_GATE, REPAIR_ROUNDS))
    for a in (rois, probs, deltas):
        a.setflags(write=False)
    return c
