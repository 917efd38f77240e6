"""The paths of k_pra_bwd (csrc/pyramid_roi_align.hip) that the fixture cases of tests/pyramid_roi_align_util.py do not reach: their
maps have at most 480 pixels and 67 channels, so a box's fp64 LDS window always holds a whole channel chunk in one pass.  Here:

  passes     windows of up to a few hundred pixels with 64-channel chunks (C = 130: chunks of 64, 64 and 2): fewer than 64 channels per
             pass, so several passes per workgroup, the last one short -- the shape of the real sizes (C = 256);
  fallback   windows above PRA_BWD_CELLS = 4096 pixels: reversed and degenerate boxes, which go to level 2, over most of an 80 x 70
             map, beside small ones and NaN and infinite boxes in the same call: the direct atomic adds;
  pool1      the same boxes with one sample each (axis_in's other branch): windows of at most four pixels.

Reference: the float64 restatement u.backward.  Gate: u.gate_of of the distance of the restatement's own serial float32 sum, the rule
of the fixture (1e-6 of the map's largest float64 gradient magnitude, or four times the serial float32 run's distance where that is
more).  Each case runs the backward several times, since the order of the atomic adds differs from run to run."""
import numpy as np
import pytest
import torch

import pyramid_roi_align_util as u
from sdn_hip import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CELLS = 4096          # csrc/pyramid_roi_align.hip: PRA_BWD_CELLS
RUNS = 5


def make_case(kind):
    rs = np.random.RandomState(9100 + len(kind))
    if kind == 'passes':
        sizes, C, pool = ((128, 120), (64, 60), (32, 30), (16, 15)), 130, 7
        boxes = u.draw_boxes(rs, 'mixed', 40)
    else:
        sizes, C, pool = ((80, 70), (40, 35), (20, 18), (10, 9)), 5, {'fallback': 14, 'pool1': 1}[kind]
        nan, inf = np.nan, np.inf
        special = np.asarray([[0.97, 0.02, 0.03, 0.98],        # reversed in y: area < 0, level 2, nearly the whole 80 x 70 map
                              [0.02, 0.96, 0.99, 0.03],        # reversed in x
                              [0.01, 0.01, 0.01, 0.99],        # no height: one row of the map, 70 pixels
                              [nan, 0.1, 0.5, 0.6], [0.1, 0.2, inf, 0.6], [-inf, 0.2, 0.4, inf], [0.2, nan, nan, 0.4]], np.float32)
        boxes = np.concatenate([special, u.draw_boxes(rs, 'mixed', 9)])
    maps = [rs.randn(C, h, w).astype(np.float32) for h, w in sizes]
    R = len(boxes)
    return dict(boxes=np.ascontiguousarray(boxes, np.float32), maps=maps, pool=pool, C=C, R=R,
                grads=rs.randn(R, C, pool, pool).astype(np.float32))


def windows(c):
    """pixels of the window of every box that has a sample inside its level's map"""
    lv, out = u.levels(c), []
    for r in range(c['R']):
        m = c['maps'][lv[r] - 2]
        inside, (tl, tr, bl, br), _xl, _yl = u.sample_table(c['boxes'][r], m.shape[1], m.shape[2], c['pool'])
        if inside.any():
            rows = np.concatenate([tl[inside], bl[inside]]) // m.shape[2]
            cols = np.concatenate([tl[inside], tr[inside]]) % m.shape[2]
            out.append(int((rows.max() - rows.min() + 1) * (cols.max() - cols.min() + 1)))
    return out


@pytest.mark.parametrize('kind', ['passes', 'fallback', 'pool1'])
def test_the_backward_is_within_the_gate_of_float64_on_every_path(kind):
    c = make_case(kind)
    w = windows(c)
    if kind == 'passes':
        assert max(w) <= CELLS and sum(1 for n in w if 64 * n > CELLS) >= 10            # several passes per 64-channel chunk
    elif kind == 'fallback':
        assert max(w) > CELLS and min(w) < CELLS                                         # both paths in one call
    else:
        assert max(w) <= 4                                                               # one sample per box: at most its four taps
    want = u.backward(c, np.float64)
    gate = u.gate_of(u.grad_error(u.backward(c, np.float32), want))
    boxes = torch.from_numpy(c['boxes']).to(DEV)
    g = torch.from_numpy(c['grads']).to(DEV)
    worst = np.zeros(u.LEVELS)
    for _ in range(RUNS):
        maps = [torch.from_numpy(m).to(DEV).requires_grad_(True) for m in c['maps']]
        pooled, levels = ops.pyramid_roi_align(boxes, maps, c['pool'], u.IMAGE_AREA)
        assert np.array_equal(levels.cpu().numpy(), u.levels(c))
        pooled.backward(g)
        got = [m.grad.cpu().numpy() for m in maps]
        worst = np.maximum(worst, u.grad_error(got, want))
        for a, b in zip(got, want):
            assert not a[b == 0].any()                                                  # where no sample reads, no gradient arrives
    print('%s: windows %d .. %d pixels; worst of %d runs %s, gate %s' % (kind, min(w), max(w), RUNS, worst, gate))
    assert (worst <= gate).all(), (worst, gate)
