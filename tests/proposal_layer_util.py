"""Shared pieces of the proposal layer's tests (tests/test_proposal_layer_host.py, tests/test_gpu_proposal_layer.py) and of the
fixture's generator (tests/golden/make_proposal_layer_golden.py): the cases and their seeded inputs (not stored, only their
checksums), the pyramid anchors restated in numpy, a numpy restatement of the contract -- the reference's proposal_layer
(geometric/maskrcnn/model.py:344-407, apply_box_deltas :307-328, clip_boxes :331-341) with the NMS of nms/pth_nms.py:10-26 on
nms/src/nms.c:4-69 -- in float32 and float64, and the IoU margin that keeps the stored cases away from the suppression threshold.

The generator runs the reference's own functions beside the restatement and asserts that they agree before it stores anything; the
GPU machine has the restatement and the fixture only.

What is float64 in the float64 form: the decode and the clip (from the float32 inputs).  Selection is on the float32 scores and the NMS
always runs on the float32 boxes: they decide WHICH boxes come out, and the margin below makes that decision safe against the last
bit of exp.  In the float32 form every operation is a float32 numpy operation in the reference's order; exp is torch's, as in the
reference's CPU run."""
import functools
import os
import zlib

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'proposal_layer_golden.npz')

MAX_PRE_NMS, MAX_ANCHORS, CHUNK = 8192, 1 << 24, 1024      # csrc/proposal_layer_check.h: PROP_MAX_PRE_NMS, PROP_MAX_ANCHORS, PROP_CHUNK
MARGIN = 1e-5              # no pair j > i of a stored case's K boxes has an fp32 IoU this close to the threshold: about 100 x what one ulp
                           # of exp moves the IoU of a box of 20 px or more
STD_DEV = (0.1, 0.1, 0.2, 0.2)                             # config.py: RPN_BBOX_STD_DEV
SCALES, RATIOS, STRIDES = (32, 64, 128, 256, 512), (0.5, 1, 2), (4, 8, 16, 32, 64)   # config.py: RPN_ANCHOR_SCALES, _RATIOS, BACKBONE_STRIDES
REPAIR_ROUNDS = 12
f32 = np.float32

# name: seed, anchors A (or the side of a pyramid), image (height, width), pre_nms_limit, proposal_count P, threshold, how it is drawn
CASES = {
    'single': dict(seed=7101, A=1, image=(128, 128), limit=6000, P=3, thr=0.7, kind='random'),
    'short': dict(seed=7102, A=37, image=(128, 128), limit=6000, P=10, thr=0.7, kind='random'),                # A < pre_nms_limit
    'exactK': dict(seed=7103, A=100, image=(256, 256), limit=100, P=20, thr=0.7, kind='random'),
    'K+1': dict(seed=7104, A=101, image=(256, 256), limit=100, P=20, thr=0.7, kind='random'),
    'chunks1025': dict(seed=7105, A=1025, image=(256, 256), limit=300, P=50, thr=0.4, kind='random'),         # one anchor in the second chunk
    'chunks2049': dict(seed=7106, A=2049, image=(256, 256), limit=300, P=50, thr=0.4, kind='random'),
    'k63': dict(seed=7107, A=200, image=(256, 256), limit=63, P=30, thr=0.3, kind='random'),                    # K either side of a mask word
    'k64': dict(seed=7107, A=200, image=(256, 256), limit=64, P=30, thr=0.3, kind='random'),
    'k65': dict(seed=7107, A=200, image=(256, 256), limit=65, P=30, thr=0.3, kind='random'),
    'onebox': dict(seed=7110, A=150, image=(128, 128), limit=100, P=10, thr=0.7, kind='onebox'),                # all boxes identical: one is kept
    'disjoint': dict(seed=7111, A=400, image=(512, 512), limit=128, P=50, thr=0.7, kind='disjoint'),            # nothing suppressed, P cuts
    'padded': dict(seed=7112, A=300, image=(64, 64), limit=200, P=150, thr=0.3, kind='random'),                 # kept < P
    'noexp': dict(seed=7113, A=500, image=(256, 256), limit=200, P=60, thr=0.7, kind='noexp'),                  # d2 = d3 = 0: exp is exact
    'rect': dict(seed=7114, A=777, image=(320, 480), limit=300, P=100, thr=0.7, kind='random'),                 # not square, no power of two
    'clip': dict(seed=7115, A=600, image=(200, 200), limit=256, P=80, thr=0.7, kind='clip'),                    # boxes leave all four sides
    'overflow': dict(seed=7116, A=64, image=(128, 128), limit=64, P=10, thr=0.7, kind='overflow'),              # exp gives inf, y2 NaN
    'ties_all': dict(seed=7117, A=2500, image=(256, 256), limit=1000, P=40, thr=0.7, kind='ties_all'),          # all scores equal
    'ties_straddle': dict(seed=7118, A=3333, image=(256, 256), limit=500, P=40, thr=0.7, kind='ties_straddle'),  # a tie run across place K
    'ties_special': dict(seed=7119, A=1500, image=(256, 256), limit=200, P=40, thr=0.7, kind='ties_special'),   # NaN, +inf, -inf, both zeros
    'tie_iou': dict(seed=7120, A=6, image=(64, 64), limit=6000, P=6, thr=0.5, kind='tie_iou'),                   # one pair at IoU == threshold
    'objects': dict(seed=7121, side=256, image=(256, 256), limit=2048, P=1000, thr=0.7, kind='objects'),        # A = 16 368, heavy suppression
    'full': dict(seed=7122, side=1024, image=(1024, 1024), limit=6000, P=2000, thr=0.7, kind='objects'),        # A = 261 888: the reference's size
}
TIES = tuple(n for n in CASES if n.startswith('ties'))
NO_REFERENCE = TIES + ('tie_iou',)               # checked against the restatement only: their order or their keep hangs on an exact tie
DECODE_ONLY = ('overflow',)                      # NaN boxes: only selection and decode are compared
STORED_WHOLE = tuple(n for n in CASES if n != 'full' and n not in TIES)    # boxes in full; the others by checksum, their float64 boxes recomputed


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def pyramid_anchors(side_h, side_w=None):
    """The anchors of an image of side_h x side_w pixels (utils.py:402-458 with config.py's scales, ratios and strides, anchor stride
    1), float32 [A, 4] = (y1, x1, y2, x2): per level every feature-map cell in row-major order, per cell the three ratios."""
    side_w = side_h if side_w is None else side_w
    out = []
    for scale, stride in zip(SCALES, STRIDES):
        rows, cols = int(np.ceil(side_h / stride)), int(np.ceil(side_w / stride))
        root = np.sqrt(np.asarray(RATIOS, np.float64))
        h, w = scale / root, scale * root                                        # [3]
        cy = (np.arange(rows) * stride)[:, None, None] + np.zeros((1, cols, 3))
        cx = (np.arange(cols) * stride)[None, :, None] + np.zeros((rows, 1, 3))
        boxes = np.stack([cy - 0.5 * h, cx - 0.5 * w, cy + 0.5 * h, cx + 0.5 * w], axis=3)
        out.append(boxes.reshape(-1, 4))
    return np.concatenate(out, 0).astype(f32)


def score_image(scores):
    """csrc/proposal_layer_check.h: prop_image -- the order-preserving integer image of float32 scores: both zeros one value, every NaN
    one value above +inf"""
    bits = np.ascontiguousarray(scores, f32).view(np.uint32)
    mag = bits & np.uint32(0x7fffffff)
    img = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    img = np.where(mag == 0, np.uint32(0x80000000), img)
    return np.where(mag > np.uint32(0x7f800000), np.uint32(0xffffffff), img).astype(np.uint32)


def select(scores, K):
    """the K best anchors, best first, equal scores lower index first: torch.sort(descending=True, stable=True), NaN above +inf"""
    return np.argsort(-(score_image(scores).astype(np.int64)), kind='stable')[:K].astype(np.int32)


def decode(anchors, deltas, std_dev, height, width, dtype=np.float64):
    """model.py:370, :313-326, :336-340 on the given rows, operation by operation in `dtype`"""
    a, d = anchors.astype(dtype), deltas.astype(dtype) * np.asarray(std_dev, f32).astype(dtype)
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
        lim = (dtype(height), dtype(width), dtype(height), dtype(width))
        cols = [np.where(v < 0, dtype(0), np.where(v > hi, hi, v)) for v, hi in zip((y1, x1, y2, x2), lim)]    # torch.clamp: NaN stays
    return np.stack(cols, 1).astype(dtype)


def areas_of(b):
    return (b[:, 3] - b[:, 1] + f32(1)) * (b[:, 2] - b[:, 0] + f32(1))           # pth_nms.py:18, float32


def iou_rows(b, areas, i, lo):
    """nms.c:51-58 in float32: the IoU of box i with the boxes lo .. (the +1 pixel convention)"""
    with np.errstate(all='ignore'):
        yy1, xx1 = np.maximum(b[i, 0], b[lo:, 0]), np.maximum(b[i, 1], b[lo:, 1])
        yy2, xx2 = np.minimum(b[i, 2], b[lo:, 2]), np.minimum(b[i, 3], b[lo:, 3])
        w, h = np.maximum(f32(0), xx2 - xx1 + f32(1)), np.maximum(f32(0), yy2 - yy1 + f32(1))
        inter = w * h
        return inter / (areas[i] + areas[lo:] - inter)


def nms(boxes32, thr, strict, limit=None):
    """greedy NMS over boxes already in score order: the kept positions (int32), at most `limit`"""
    b = np.ascontiguousarray(boxes32, f32)
    areas, thr = areas_of(b), f32(thr)
    dead = np.zeros(len(b), bool)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(i)
        if limit is not None and len(keep) == limit:
            break
        ovr = iou_rows(b, areas, i, i + 1)
        dead[i + 1:] |= (ovr > thr) if strict else (ovr >= thr)
    return np.asarray(keep, np.int32)


def near_pairs(boxes32, thr, rows=None):
    """the boxes j that form, with a box i < j, a pair whose fp32 IoU lies within MARGIN of thr (float64 comparison of the fp32 IoU);
    rows: only pairs with i or j among them"""
    b = np.ascontiguousarray(boxes32, f32)
    areas = areas_of(b)
    bad = set()
    if rows is None:
        for i in range(len(b) - 1):
            ovr = iou_rows(b, areas, i, i + 1).astype(np.float64)
            bad.update((i + 1 + np.nonzero(np.abs(ovr - thr) < MARGIN)[0]).tolist())
    else:
        for r in rows:
            ovr = iou_rows(b, areas, r, 0).astype(np.float64)
            hit = np.nonzero(np.abs(ovr - thr) < MARGIN)[0]
            bad.update(max(int(j), r) for j in hit if j != r)
    return sorted(bad)


def min_margin(boxes32, thr):
    """the smallest |IoU - thr| over all pairs of finite boxes (inf when there is no pair)"""
    b = np.ascontiguousarray(boxes32, f32)
    areas = areas_of(b)
    best = np.inf
    for i in range(len(b) - 1):
        ovr = iou_rows(b, areas, i, i + 1).astype(np.float64)
        ovr = ovr[np.isfinite(ovr)]
        if len(ovr):
            best = min(best, float(np.abs(ovr - thr).min()))
    return best


def contract(c, dtype=np.float32, strict=True):
    """The contract on a drawn case: dict(order [K], boxes [K, 4] in `dtype`, keep [<= P], rois float32 [len(keep), 4]).  keep and rois
    always come from the float32 boxes."""
    order = select(c['probs'][:, 1], c['K'])
    H, W = c['image']
    boxes32 = decode(c['anchors'][order], c['deltas'][order], c['std_dev'], H, W, np.float32)
    boxes = boxes32 if dtype is np.float32 else decode(c['anchors'][order], c['deltas'][order], c['std_dev'], H, W, dtype)
    keep = nms(boxes32, c['thr'], strict, c['P'])
    with np.errstate(all='ignore'):
        rois = boxes32[keep] / np.asarray([H, W, H, W], f32)          # :402
    return dict(order=order, boxes=boxes, keep=keep, rois=rois.astype(f32))


def _random_anchors(rs, A, H, W):
    h, w = np.exp(rs.uniform(np.log(8.0), np.log(0.6 * H), A)), np.exp(rs.uniform(np.log(8.0), np.log(0.6 * W), A))
    cy, cx = rs.uniform(0, H, A), rs.uniform(0, W, A)
    return np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(f32)


def _object_scores(rs, anchors, H, W, n_obj):
    """scores and deltas as an RPN gives them: anchors that overlap one of n_obj objects score high and regress towards it"""
    a = anchors.astype(np.float64)
    oh, ow = np.exp(rs.uniform(np.log(0.06 * H), np.log(0.5 * H), n_obj)), np.exp(rs.uniform(np.log(0.06 * W), np.log(0.5 * W), n_obj))
    oy, ox = rs.uniform(0.1 * H, 0.9 * H, n_obj), rs.uniform(0.1 * W, 0.9 * W, n_obj)
    ob = np.stack([oy - oh / 2, ox - ow / 2, oy + oh / 2, ox + ow / 2], 1)
    best, which = np.zeros(len(a)), np.zeros(len(a), np.int64)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    for k in range(n_obj):
        ih = np.clip(np.minimum(a[:, 2], ob[k, 2]) - np.maximum(a[:, 0], ob[k, 0]), 0, None)
        iw = np.clip(np.minimum(a[:, 3], ob[k, 3]) - np.maximum(a[:, 1], ob[k, 1]), 0, None)
        iou = ih * iw / (area_a + oh[k] * ow[k] - ih * iw)
        better = iou > best
        best, which = np.where(better, iou, best), np.where(better, k, which)
    scores = np.clip(0.02 + 0.9 * best + rs.normal(0, 0.03, len(a)), 1e-4, 0.999)
    ah, aw = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    ay, ax = a[:, 0] + ah / 2, a[:, 1] + aw / 2
    target = np.stack([(oy[which] - ay) / ah, (ox[which] - ax) / aw, np.log(oh[which] / ah), np.log(ow[which] / aw)], 1) / np.asarray(STD_DEV)
    pull = np.clip(best / 0.5, 0, 1)[:, None]
    deltas = pull * np.clip(target, -12, 12) + rs.normal(0, 0.6, (len(a), 4))
    return scores.astype(f32), deltas.astype(f32)


def _draw(rs, k):
    """(scores [A], deltas [A, 4], anchors [A, 4]) before any repair"""
    H, W = k['image']
    kind = k['kind']
    if kind == 'objects':
        anchors = pyramid_anchors(k['side'])
        scores, deltas = _object_scores(rs, anchors, H, W, 40 if k['side'] >= 1024 else 12)
        return scores, deltas, anchors
    A = k['A']
    anchors = _random_anchors(rs, A, H, W)
    scores = rs.uniform(0.0, 1.0, A).astype(f32)
    deltas = rs.normal(0, 1.0, (A, 4)).astype(f32)
    if kind == 'onebox':
        anchors[:] = np.asarray([20, 30, 70, 90], f32)
        deltas[:] = np.asarray([0.5, -0.25, 1.0, -1.0], f32)
    elif kind == 'disjoint':      # a 20 x 20 grid of 12 px boxes 25 px apart, moved by less than a pixel
        gy, gx = np.divmod(np.arange(A), 20)
        anchors = np.stack([gy * 25 + 2, gx * 25 + 2, gy * 25 + 14, gx * 25 + 14], 1).astype(f32)
        deltas = rs.normal(0, 0.3, (A, 4)).astype(f32)
    elif kind == 'noexp':
        deltas[:, 2:] = 0
    elif kind == 'clip':          # anchors centred on the border, pushed outwards
        side = np.arange(A) % 4
        cy = np.where(side == 0, 0, np.where(side == 1, H, rs.uniform(0, H, A)))
        cx = np.where(side == 2, 0, np.where(side == 3, W, rs.uniform(0, W, A)))
        h, w = rs.uniform(20, 120, (2, A))
        anchors = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(f32)
        deltas = (rs.normal(0, 1.0, (A, 4)) * (1, 1, 3, 3)).astype(f32)
    elif kind == 'overflow':
        deltas[0::4, 2] = 5000.0      # exp = inf, in float64 too: h = inf, y1 = -inf -> 0, y2 = -inf + inf = NaN
        deltas[1::4, 3] = 4000.0
        deltas[2::8, 2] = -2000.0     # exp = 0: h = 0
        anchors[5] = (40, 40, 40, 80)  # h = 0 and exp = inf: 0 * inf = NaN
        deltas[5, 2] = 5000.0
    elif kind == 'ties_all':
        scores[:] = f32(0.625)
    elif kind == 'ties_straddle':   # 300 equal scores scattered over the chunks, about a third of them above place K
        order = np.argsort(-scores, kind='stable')
        run = order[k['limit'] - 100:k['limit'] + 200]
        scores[run] = scores[order[k['limit']]]
    elif kind == 'ties_special':
        scores[700:1300:7] = f32(-0.0)
        scores[701:1300:7] = f32(0.0)
        scores[702:1300:7] = -scores[702:1300:7]
        scores[rs.permutation(A)[:12]] = np.asarray([np.nan, -np.nan, np.inf, np.inf, -np.inf, 0.0, -0.0, 0.0, 1.0, 1.0, -1.0, np.nan], f32)
    elif kind == 'tie_iou':          # areas 100 and 50 under the +1 convention, intersection 50: IoU = 0.5 exactly
        anchors = np.asarray([[0, 0, 9, 9], [0, 0, 9, 4], [30, 30, 50, 50], [31, 31, 50, 50], [5, 40, 25, 60], [40, 5, 60, 25]], f32)
        scores = np.asarray([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], f32)
        deltas = np.zeros((A, 4), f32)
    elif kind != 'random':
        raise KeyError(kind)
    return scores, deltas, anchors


@functools.lru_cache(maxsize=None)
def draw_case(name):
    """The inputs of a case, float32: probs [A, 2], deltas [A, 4], anchors [A, 4], and its parameters.  The draw repairs itself, the same
    way every time: equal scores among the best K + 1 are drawn again (not in the `ties*` cases), and while a pair j > i of the K
    selected boxes has an fp32 IoU within MARGIN of the threshold, the deltas of box j are drawn again from the case's generator."""
    k = CASES[name]
    rs = np.random.RandomState(k['seed'])
    scores, deltas, anchors = _draw(rs, k)
    A = len(anchors)
    K = min(k['limit'], A)
    H, W = k['image']
    if name not in TIES:
        for _ in range(REPAIR_ROUNDS):
            top = select(scores, min(K + 1, A))
            s = scores[top]
            dup = top[1:][s[1:] == s[:-1]]
            if not len(dup):
                break
            scores[dup] = rs.uniform(0.0, 1.0, len(dup)).astype(f32)
        else:
            raise AssertionError('%s: equal scores among the best K + 1 after %d rounds' % (name, REPAIR_ROUNDS))
    order = select(scores, K)
    if name != 'tie_iou' and name not in DECODE_ONLY:
        rows = None
        for _ in range(REPAIR_ROUNDS):
            boxes = decode(anchors[order], deltas[order], STD_DEV, H, W, np.float32)
            bad = near_pairs(boxes, k['thr'], rows)
            if not bad:
                break
            noise = 0.6 if k['kind'] == 'objects' else 1.0
            deltas[order[bad]] = _redraw(rs, k, deltas[order[bad]], noise)
            rows = bad
        else:
            raise AssertionError('%s: a pair within %g of the threshold after %d rounds' % (name, MARGIN, REPAIR_ROUNDS))
    probs = np.stack([f32(1) - scores, scores], 1).astype(f32)
    for a in (probs, deltas, anchors):
        a.setflags(write=False)
    return dict(name=name, probs=probs, deltas=deltas, anchors=anchors, std_dev=STD_DEV, image=(H, W), A=A, K=K, P=k['P'], thr=k['thr'],
                limit=k['limit'])


def _redraw(rs, k, old, noise):
    """new deltas for the boxes of a pair too close to the threshold: the old ones moved by a fresh draw (an object's box stays near
    its object); the `noexp` case keeps d2 = d3 = 0"""
    new = old.astype(np.float64) + rs.normal(0, 0.25 * noise, old.shape)
    if k['kind'] == 'noexp':
        new[:, 2:] = 0
    return new.astype(f32)
