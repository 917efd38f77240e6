"""Shared pieces of the pyramid RoIAlign tests (tests/test_pyramid_roi_align_host.py, tests/test_gpu_pyramid_roi_align.py) and of the
fixture's generator (tests/golden/make_pyramid_roi_align_golden.py): the cases, their seeded inputs and a numpy restatement of the
reference's pyramid_roi_align (geometric/maskrcnn/model.py:414-502, log2 of :95-100) with the crop it calls per level
(roialign/roi_align/src/crop_and_resize.c:7-251): levels, forward and the gradients of the four maps.  The generator runs the
reference's own code beside the restatement and asserts that they agree before it stores anything; the GPU machine has the
restatement and the fixture only.

What is float64 here: the level value, and the products and sums of forward and backward.  The sample coordinates, the tap indices
and the two lerp weights are always formed in float32, operation for operation as crop_and_resize.c forms them: they decide WHICH
pixels a sample reads, and a float64 coordinate would pick other taps wherever a sample lands on a pixel row.  With dtype=np.float32
the interpolation is done in float32 too, in the C code's order, and gives its bits."""
import functools
import os
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pyramid_roi_align_golden.npz')

LEVELS = 4                           # P2 .. P5
CHANNELS, MAX_POOL = 64, 32          # csrc/pyramid_roi_align_check.h: PRA_CHANNELS, PRA_MAX_POOL
GATE = 1e-6                          # per level map, of that map's largest float64 gradient magnitude
MARGIN = 1e-3                        # no stored box has a float64 level value this close to a half-integer
IMAGE_SHAPE = (1024, 1024, 3)        # normalised boxes of side 0.03 .. 0.9 reach all four levels; the maps need not match it
IMAGE_AREA = float(IMAGE_SHAPE[0] * IMAGE_SHAPE[1])
PYRAMID = ((24, 20), (12, 10), (6, 5), (3, 3))
f32 = np.float32

# name: seed, R, C, the four maps' (H, W), pool, how the boxes are drawn
CASES = {
    'mixed7': dict(seed=6101, R=37, C=5, maps=PYRAMID, pool=7, boxes='mixed'),       # all four levels
    'mixed14': dict(seed=6101, R=37, C=5, maps=PYRAMID, pool=14, boxes='mixed'),     # the same boxes and maps, the mask head's pool
    'onelevel': dict(seed=6103, R=11, C=3, maps=PYRAMID, pool=7, boxes='level3'),    # three levels take the reference's `continue`
    'single': dict(seed=6104, R=1, C=4, maps=PYRAMID, pool=7, boxes='mixed'),
    'outside': dict(seed=6105, R=23, C=3, maps=PYRAMID, pool=7, boxes='outside'),    # samples off the map: value 0, no gradient
    'clamp': dict(seed=6106, R=16, C=2, maps=PYRAMID, pool=5, boxes='clamp'),        # level values below 2 and above 5
    'degenerate': dict(seed=6107, R=6, C=2, maps=PYRAMID, pool=3, boxes='degenerate'),   # area 0 and below: -inf and NaN go to level 2
    'thin': dict(seed=6108, R=19, C=3, maps=((1, 20), (12, 1), (6, 5), (1, 1)), pool=7, boxes='mixed'),   # H = 1, W = 1, both
    'pool1': dict(seed=6109, R=9, C=2, maps=PYRAMID, pool=1, boxes='mixed'),         # the crop's other coordinate formula (:56, 79)
    'c67': dict(seed=6110, R=9, C=67, maps=((6, 5), (5, 4), (3, 3), (2, 2)), pool=7, boxes='mixed'),   # one full channel chunk and three channels
    'big': dict(seed=6111, R=1000, C=8, maps=PYRAMID, pool=7, boxes='mixed'),        # the grid's upper end
}
STORED_WHOLE = ('mixed7', 'onelevel', 'single', 'outside', 'clamp', 'degenerate', 'thin', 'pool1')   # pooled in full; the others by checksum


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def level_values(boxes):
    """model.py:445-455 in float64 on the float32 boxes"""
    b = boxes.astype(np.float64)
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    with np.errstate(all='ignore'):
        return 4.0 + np.log(np.sqrt(h * w) / (224.0 / np.sqrt(IMAGE_AREA))) / np.log(2.0)


def levels_of(values):
    """model.py:456-457: round half to even, clamp to [2, 5]; a non-finite value gives 2 (x86's float-to-int conversion gives
    INT_MIN for NaN and for both infinities, which the clamp lifts to 2)"""
    v = np.asarray(values, np.float64)
    ok = np.isfinite(v)
    return np.where(ok, np.clip(np.rint(np.where(ok, v, 0.0)), 2, 5), 2).astype(np.int32)


def margin(values):
    """distance of every finite level value from the nearest half-integer (inf where the value is not finite)"""
    v = np.asarray(values, np.float64)
    with np.errstate(all='ignore'):
        d = np.abs(v - np.floor(v) - 0.5)
    return np.where(np.isfinite(v), d, np.inf)


def _draw_boxes(rs, kind, n):
    if kind == 'degenerate':
        b = np.array([[0.2, 0.3, 0.2, 0.7],       # h = 0: log(0) = -inf
                      [0.1, 0.6, 0.5, 0.6],       # w = 0
                      [0.4, 0.4, 0.4, 0.4],       # a point
                      [0.7, 0.2, 0.3, 0.8],       # h < 0: sqrt(< 0) = NaN
                      [0.2, 0.9, 0.6, 0.1],       # w < 0
                      [0.8, 0.7, 0.3, 0.2]])      # both: a positive area again, walked backwards
        return b[:n].astype(f32)
    if kind == 'mixed':       # side lengths log-uniform over 0.02 .. 0.95, placed inside the image
        h, w = np.exp(rs.uniform(np.log(0.02), np.log(0.95), (2, n)))
        y1, x1 = rs.uniform(0, 1 - h), rs.uniform(0, 1 - w)
    elif kind == 'level3':    # sqrt(h * w) inside (0.0773, 0.1547), away from both ends
        s = rs.uniform(0.085, 0.14, n)
        a = np.exp(rs.uniform(-0.4, 0.4, n))
        h, w = s * a, s / a
        y1, x1 = rs.uniform(0, 1 - h), rs.uniform(0, 1 - w)
    elif kind == 'outside':   # every box crosses at least one border of [0, 1]
        h, w = np.exp(rs.uniform(np.log(0.05), np.log(0.9), (2, n)))
        y1, x1 = rs.uniform(-0.4, 1.1, n), rs.uniform(-0.4, 1.1, n)
        flip = rs.rand(n) < 0.5
        y1 = np.where(flip, np.where(rs.rand(n) < 0.5, -h * rs.uniform(0.1, 0.9, n), 1 - h * rs.uniform(0.1, 0.9, n)), y1)
        x1 = np.where(~flip, np.where(rs.rand(n) < 0.5, -w * rs.uniform(0.1, 0.9, n), 1 - w * rs.uniform(0.1, 0.9, n)), x1)
    elif kind == 'clamp':     # half tiny (value below 1.5), half huge (value above 5.5)
        tiny = np.arange(n) % 2 == 0
        s = np.where(tiny, np.exp(rs.uniform(np.log(1e-4), np.log(0.03), n)), rs.uniform(0.7, 3.0, n))
        a = np.exp(rs.uniform(-0.2, 0.2, n))
        h, w = s * a, s / a
        y1, x1 = rs.uniform(0, 0.9, n) - np.where(tiny, 0, h / 2), rs.uniform(0, 0.9, n) - np.where(tiny, 0, w / 2)
    else:
        raise KeyError(kind)
    return np.stack([y1, x1, y1 + h, x1 + w], 1).astype(f32)


def draw_boxes(rs, kind, R):
    """R boxes; any whose float64 level value lies within MARGIN of a half-integer is drawn again, so that no case is left out and
    the device's logf cannot flip a level"""
    boxes = _draw_boxes(rs, kind, R)
    for _ in range(100):
        bad = np.nonzero(margin(level_values(boxes)) <= MARGIN)[0]
        if not len(bad):
            return boxes
        boxes[bad] = _draw_boxes(rs, kind, len(bad))
    raise AssertionError('could not draw the boxes of %r' % kind)


@functools.lru_cache(maxsize=None)
def draw_case(name):
    """boxes [R, 4], the four maps [C, H, W] and grads [R, C, pool, pool], float32, from numpy's frozen RandomState stream"""
    k = CASES[name]
    rs = np.random.RandomState(k['seed'])
    boxes = draw_boxes(rs, k['boxes'], k['R'])
    maps = [rs.randn(k['C'], h, w).astype(f32) for h, w in k['maps']]
    grads = np.random.RandomState(k['seed'] + 50000).randn(k['R'], k['C'], k['pool'], k['pool']).astype(f32)
    c = dict(boxes=boxes, maps=maps, grads=grads, pool=k['pool'], C=k['C'], R=k['R'])
    for a in [boxes, grads] + maps:
        a.setflags(write=False)
    return c


def _axis(a1, a2, extent, crop):
    """crop_and_resize.c:44-56 along one axis, in float32 as written there: (coordinate, inside, low index, high index, lerp)"""
    k = np.arange(crop)
    if crop > 1:
        scale = f32(f32(a2 - a1) * f32(extent - 1)) / f32(crop - 1)
        pos = f32(a1 * f32(extent - 1)) + k.astype(f32) * f32(scale)
    else:
        pos = np.full(1, f32(0.5 * float(f32(a1 + a2)) * float(extent - 1)), f32)
    pos = pos.astype(f32)
    with np.errstate(invalid='ignore'):
        inside = (pos >= 0) & (pos <= f32(extent - 1))     # :58 turned round; a NaN counts as outside, as in the kernel
    safe = np.where(inside, pos, f32(0))
    lo, hi = np.floor(safe).astype(np.int64), np.ceil(safe).astype(np.int64)
    return inside, lo, hi, (safe - lo.astype(f32)).astype(f32)


def sample_table(box, H, W, pool):
    """per sample (y fastest outside, x inside): inside flag, the four tap offsets in a channel plane, x_lerp, y_lerp"""
    y1, x1, y2, x2 = [f32(v) for v in box]
    iy, top, bottom, yl = _axis(y1, y2, H, pool)
    ix, left, right, xl = _axis(x1, x2, W, pool)
    inside = (iy[:, None] & ix[None, :]).reshape(-1)
    taps = [(a[:, None] * W + b[None, :]).reshape(-1) for a, b in ((top, left), (top, right), (bottom, left), (bottom, right))]
    xl = np.broadcast_to(xl[None, :], (pool, pool)).reshape(-1)
    yl = np.broadcast_to(yl[:, None], (pool, pool)).reshape(-1)
    return inside, taps, xl, yl


def levels(c):
    return levels_of(level_values(c['boxes']))


def forward(c, dtype=np.float64):
    """pooled [R, C, pool, pool] in `dtype`, in box order; np.float32 follows crop_and_resize.c:102-106 operation for operation"""
    lv = levels(c)
    pool, C = c['pool'], c['C']
    out = np.zeros((c['R'], C, pool * pool), dtype)
    for r in range(c['R']):
        m = c['maps'][lv[r] - 2]
        flat = m.reshape(C, -1).astype(dtype)
        inside, (tl, tr, bl, br), xl, yl = sample_table(c['boxes'][r], m.shape[1], m.shape[2], pool)
        xl, yl = xl.astype(dtype), yl.astype(dtype)
        top = flat[:, tl] + (flat[:, tr] - flat[:, tl]) * xl
        bottom = flat[:, bl] + (flat[:, br] - flat[:, bl]) * xl
        out[r] = np.where(inside, top + (bottom - top) * yl, dtype(0))
    return out.reshape(c['R'], C, pool, pool)


def backward(c, dtype=np.float64):
    """the gradients of the four maps for c['grads'], crop_and_resize.c:241-247; levels without a box stay zero"""
    lv = levels(c)
    pool, C = c['pool'], c['C']
    gm = [np.zeros(m.shape, dtype) for m in c['maps']]
    one = dtype(1)
    for r in range(c['R']):
        m = gm[lv[r] - 2]
        flat = m.reshape(C, -1)
        inside, (tl, tr, bl, br), xl, yl = sample_table(c['boxes'][r], m.shape[1], m.shape[2], pool)
        g = c['grads'][r].reshape(C, -1).astype(dtype)[:, inside]
        xl, yl = xl.astype(dtype)[inside], yl.astype(dtype)[inside]
        dtop, dbottom = (one - yl) * g, yl * g
        for idx, val in ((tl, (one - xl) * dtop), (tr, xl * dtop), (bl, (one - xl) * dbottom), (br, xl * dbottom)):
            np.add.at(flat, (slice(None), idx[inside]), val)
    return gm


def grad_error(got, want):
    """per level: the largest difference, relative to the largest float64 gradient magnitude of that map (0 for an all-zero map that
    is matched exactly, inf for one that is not)"""
    out = []
    for g, w in zip(got, want):
        top = float(np.abs(w).max())
        diff = float(np.abs(np.asarray(g, np.float64) - w).max())
        out.append(diff / top if top > 0 else (0.0 if diff == 0 else np.inf))
    return np.asarray(out)


def gate_of(err):
    """the fixture's gate per level: GATE, or four times the distance of the reference's own float32 run where that is more"""
    err = np.asarray(err, np.float64)
    return np.where(err <= GATE, GATE, 4.0 * err)


def grad_offsets(C, maps):
    """sdn_pyramid_roi_align_grad_floats, restated: every level's range starts on 16 bytes"""
    offsets, at = [], 0
    for h, w in maps:
        offsets.append(at)
        at += (C * h * w + 3) // 4 * 4
    return offsets, at
