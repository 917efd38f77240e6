"""Shared pieces of the ordered pyramid RoIAlign backward's tests (tests/test_pyramid_ordered_host.py, tests/test_gpu_pyramid_ordered.py):
the contract of sdn_pyramid_roi_align_bwd_ordered (include/sdn_hip.h) restated in numpy, and the cases beyond the fixture's.

The contract: for every element of the four maps, the four float32 terms of every inside sample that lands on it, formed operation for
operation as crop_and_resize.c:241-247 forms them, widened to float64, added to +0.0, the sum rounded to float32 once.  The kernel is
free to choose the order of the additions as long as it is fixed; the GPU test may still demand equal bits because the float64 sum of
these float32 terms does not depend on the order on any case used here, which tests/test_pyramid_ordered_host.py shows for four orders.

The sample coordinates, taps and lerp weights come from pyramid_roi_align_util.sample_table, the levels from its `levels`."""
import functools

import numpy as np

import pyramid_roi_align_util as u
import test_gpu_pyramid_bwd_window as window   # its make_case: the 'passes' shape and the 'fallback' / 'pool1' boxes

f32 = np.float32
NEW_CASES = ('tiles', 'chunks', 'special', 'special_pool1', 'long', 'pool32', 'nonfinite', 'zero_inf')
ALL_CASES = tuple(u.CASES) + NEW_CASES
LIST_BATCH = 256          # csrc/pyramid_roi_align.hip: k_pra_bwd_ordered compacts PRA_THREADS records at a time into its LDS list
TILE = 8                  # csrc/pyramid_roi_align_check.h: PRA_TILE


def _drawn(seed, R, C, pool, maps, extra=None):
    rs = np.random.RandomState(seed)
    boxes = u.draw_boxes(rs, 'mixed', R)
    if extra is not None:
        boxes = np.concatenate([np.asarray(extra, f32), boxes])[:R]
    return dict(boxes=np.ascontiguousarray(boxes, f32), maps=[rs.randn(C, h, w).astype(f32) for h, w in maps], pool=pool, C=C, R=R,
                grads=rs.randn(R, C, pool, pool).astype(f32))


def _first_inside_sample(c, r):
    m = c['maps'][u.levels(c)[r] - 2]
    inside = u.sample_table(c['boxes'][r], m.shape[1], m.shape[2], c['pool'])[0]
    return int(np.nonzero(inside)[0][0])


@functools.lru_cache(maxsize=None)
def make_case(name):
    """a fixture case (pyramid_roi_align_util.CASES) or one of NEW_CASES; seeded, read-only"""
    if name in u.CASES:
        return u.draw_case(name)
    if name == 'tiles':        # map sides that are no multiple of the 8 x 8 tile; boxes across tile borders, two of them on the map's corners
        c = _drawn(7303, 60, 3, 7, ((37, 41), (19, 21), (9, 11), (5, 5)), extra=[[0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 1.0, 1.0]])
    elif name == 'chunks':     # C = 130: channel chunks 64, 64, 2; maps up to 128 x 120: many tiles
        c = window.make_case('passes')
    elif name == 'special':    # reversed, zero-height, NaN and infinite boxes; a window over most of the 80 x 70 map beside small ones
        c = window.make_case('fallback')
    elif name == 'special_pool1':   # the same boxes, the one-sample coordinate formula
        c = window.make_case('pool1')
    elif name == 'long':       # more boxes than one batch of the kernel's list: the 3 x 3 map is one tile that every P5 box meets
        c = _drawn(7301, 2500, 2, 7, u.PYRAMID)
    elif name == 'pool32':     # the largest per-axis tables
        c = _drawn(7302, 12, 3, 32, u.PYRAMID)
    elif name == 'nonfinite':  # mixed7 with one +inf and one NaN among the gradients of inside samples
        c = dict(u.draw_case('mixed7'))
        g = c['grads'].copy()
        g[3, 1].reshape(-1)[_first_inside_sample(c, 3)] = np.inf
        g[20, 4].reshape(-1)[_first_inside_sample(c, 20)] = np.nan
        c['grads'] = g
    elif name == 'zero_inf':   # samples ON pixel rows and columns (lerp 0) with infinite gradients: the 0 * inf terms, and inf - inf
        c = _drawn(7304, 6, 2, 7, u.PYRAMID, extra=[[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.25, 0.25]])
        c['grads'][0, 0, 0, 0] = np.inf        # sample (0, 0) of the whole-image box: coordinate (0, 0), both lerps 0
        c['grads'][0, 1, 6, 6] = -np.inf       # its last sample: coordinate (H - 1, W - 1)
        c['grads'][1, 1, 6, 6] = np.inf        # the same pixel from the second box: inf - inf
        c['grads'][2, 0, 0, 3] = np.inf        # y on row 0 (y_lerp 0), x between columns
    else:
        raise KeyError(name)
    for a in [c['boxes'], c['grads']] + list(c['maps']):
        a.setflags(write=False)
    return c


def level_terms(c):
    """per level (flat pixel index int64 [n], float32 terms [C, n]): every term of every inside sample routed to that level, in the
    order (box, tap: top-left, top-right, bottom-left, bottom-right, sample).  crop_and_resize.c:241-247 in float32."""
    lv = u.levels(c)
    pool, C = c['pool'], c['C']
    one = f32(1)
    idx, val = [[] for _ in range(u.LEVELS)], [[] for _ in range(u.LEVELS)]
    with np.errstate(invalid='ignore', over='ignore'):
        for r in range(c['R']):
            m = c['maps'][lv[r] - 2]
            inside, (tl, tr, bl, br), xl, yl = u.sample_table(c['boxes'][r], m.shape[1], m.shape[2], pool)
            g = c['grads'][r].reshape(C, -1)[:, inside]
            xl, yl = xl[inside].astype(f32), yl[inside].astype(f32)
            dtop, dbottom = (one - yl) * g, yl * g
            for tap, t in ((tl, (one - xl) * dtop), (tr, xl * dtop), (bl, (one - xl) * dbottom), (br, xl * dbottom)):
                assert t.dtype == np.float32
                idx[lv[r] - 2].append(tap[inside])
                val[lv[r] - 2].append(t)
    return [(np.concatenate(i) if i else np.zeros(0, np.int64), np.concatenate(v, 1) if v else np.zeros((C, 0), f32)) for i, v in zip(idx, val)]


def accumulate(c, terms, order=None, dtype=np.float64):
    """the terms added to +0.0 of `dtype` per destination, in the given order of the terms (None: as listed), rounded to float32"""
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for m, (idx, val) in zip(c['maps'], terms):
            acc = np.zeros((c['C'], m.shape[1] * m.shape[2]), dtype)
            o = np.arange(len(idx)) if order is None else order(len(idx))
            np.add.at(acc, (slice(None), idx[o]), val[:, o].astype(dtype))
            out.append(acc.astype(f32).reshape(m.shape))
    return out


_done = {}


def ordered_backward(c_or_name):
    """the contract: the four maps' gradients, float32; computed once per named case and shared (read-only)"""
    if isinstance(c_or_name, str):
        if c_or_name not in _done:
            c = make_case(c_or_name)
            _done[c_or_name] = accumulate(c, level_terms(c))
            for a in _done[c_or_name]:
                a.setflags(write=False)
        return _done[c_or_name]
    return accumulate(c_or_name, level_terms(c_or_name))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def reached(c):
    """per level a bool map: the pixels some inside sample lands on"""
    return [np.isin(np.arange(m.shape[1] * m.shape[2]), idx).reshape(m.shape[1:]) for m, (idx, _) in zip(c['maps'], level_terms(c))]
