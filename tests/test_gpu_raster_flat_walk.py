"""The candidate walk of k_raster_tiles on scenes whose candidate boxes have prescribed sizes.

A wave of the tile kernel fetches up to 64 faces per batch and walks the pixels of their clipped candidate boxes: boxes of up
to FLAT_MAX = 256 pixels as one stream of (face, pixel) candidates, 64 consecutive ones per pass whichever faces they belong
to, larger ones shared by the wave and walked by row spans.  The scenes here pin what the walk must keep whichever class a box
falls into -- they hold for the walks the stream replaced as well (one lane per box of up to SMALL = 32 pixels, one broadcast
per box of 33 .. 256): every (face, pixel) pair of a clipped box is tested exactly once and the maps are the oracle's, bit
for bit.

Faces are right triangles whose vertices lie a quarter pixel outside the first and last pixel centre of a w x h box; their
margin (face_margin_px) is about 0.004 px, so k_face_setup's candidate box is exactly that box.  The order of a tile's list is
whatever the binning kernels produce, so scenes that need an exact total per batch use faces of one area throughout.
"""
import numpy as np
import pytest
import torch

from oracle import nr_oracle as no
from util import biteq

pytestmark = pytest.mark.gpu

TS = 32            # tile side of k_raster_tiles
FLAT_MAX = 256     # boxes up to this many pixels join the candidate stream; larger ones are walked by row spans (fewer tests than pixels)
SMALL = 32         # the largest box the lane-private walk took before the stream


def box_faces(rng, boxes, S):
    """boxes: rows (x0, y0, w, h) in internal pixels -> [1, n, 3, 3] float32 NDC faces, front-facing, random vertex depths."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    x0, y0, x1, y1 = b[:, 0] - 0.25, b[:, 1] - 0.25, b[:, 0] + b[:, 2] - 0.75, b[:, 1] + b[:, 3] - 0.75
    pix = np.stack([np.stack([x0, y0], -1), np.stack([x1, y0], -1), np.stack([x0, y1], -1)], 1)      # [n, 3, 2]
    ndc = (2.0 * pix + 1.0 - S) / S
    z = rng.uniform(0.5, 5.0, (len(b), 3, 1))
    return np.concatenate([ndc, z], -1).astype(np.float32)[None]


def random_boxes(rng, n, S, amax=FLAT_MAX, amin=1):
    """n boxes with areas in amin .. amax, anywhere in the S x S image."""
    out = []
    while len(out) < n:
        w, h = int(rng.integers(1, TS + 1)), int(rng.integers(1, TS + 1))
        if not amin <= w * h <= amax:
            continue
        out.append((int(rng.integers(0, S - w + 1)), int(rng.integers(0, S - h + 1)), w, h))
    return out


def same_boxes(rng, n, w, h, S=TS):
    return [(int(rng.integers(0, S - w + 1)), int(rng.integers(0, S - h + 1)), w, h) for _ in range(n)]


def candidate_tests(faces, S):
    """Sum over faces and tiles of the clipped candidate box areas, the boxes computed as k_face_setup computes them (float32)."""
    f = faces[0].astype(np.float32)
    fS = np.float32(S)
    px = np.float32(0.5) * ((f[:, :, 0] * fS + fS) - np.float32(1))
    py = np.float32(0.5) * ((f[:, :, 1] * fS + fS) - np.float32(1))
    e = [(f[:, 1] - f[:, 0])[:, :2], (f[:, 2] - f[:, 0])[:, :2], (f[:, 2] - f[:, 1])[:, :2]]
    ln = [np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) for d in e]
    lmax = np.maximum(ln[0], np.maximum(ln[1], ln[2]))
    perim = ln[0] + ln[1] + ln[2]
    cmax = np.abs(f[:, :, :2]).max((1, 2))
    u = np.float32(9.5367432e-7)
    area2 = np.abs(e[0][:, 0] * e[1][:, 1] - e[1][:, 0] * e[0][:, 1]) - u * lmax * lmax
    assert (area2 > 0).all()
    delta = u * (np.float32(1) + cmax)
    base = np.float32(0.004) * max(np.float32(1), fS / np.float32(1024)) + np.float32(0.5) * fS * delta
    m = base + np.float32(0.5) * fS * (delta * perim * lmax / area2)
    assert (m > 0).all() and (m < 0.05).all(), 'the construction keeps every face far from the thin-face band path'
    x0 = np.maximum(np.ceil(px.min(1) - m), 0).astype(int)
    x1 = np.minimum(np.floor(px.max(1) + m), S - 1).astype(int)
    y0 = np.maximum(np.ceil(py.min(1) - m), 0).astype(int)
    y1 = np.minimum(np.floor(py.max(1) + m), S - 1).astype(int)
    total, largest, per_tile = 0, 0, 0
    for Y0 in range(0, S, TS):
        for X0 in range(0, S, TS):
            w = np.minimum(x1, X0 + TS - 1) - np.maximum(x0, X0) + 1
            h = np.minimum(y1, Y0 + TS - 1) - np.maximum(y0, Y0) + 1
            a = np.where((w > 0) & (h > 0), w * h, 0)
            total += int(a.sum())
            largest = max(largest, int(a.max()))
            per_tile = max(per_tile, int((a > 0).sum()))
    return total, largest, per_tile, np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], 1)


def class_border_boxes(rng):
    """The class borders old and new: 32 and 33 pixels, FLAT_MAX = 16 x 16, 16 x 17 (257 is prime: the next box above) and the
    full tile, small faces listed before, between and after them (the `behind` test, hits carried over in the queue)."""
    big = [(3, 5, 8, 4), (12, 20, 11, 3), (8, 2, 16, 16), (10, 12, 16, 17), (0, 0, 32, 32)]
    small = random_boxes(rng, 19, TS, amax=12)
    out = []
    for i, s in enumerate(small):
        out.append(s)
        if i % 4 == 1:
            out.append(big[i // 4])
    return out


def start_boxes(rng):
    """Twelve faces, three per wave in list order: an 8 x 8 box first in its batch, after one pixel, and after 31 + 32 = 63."""
    A = lambda w, h: same_boxes(rng, 1, w, h)[0]
    return [A(8, 8), A(3, 2), A(5, 1),
            A(1, 1), A(8, 8), A(2, 2),
            A(31, 1), A(8, 4), A(8, 8),
            A(4, 4), A(1, 7), A(6, 5)]


def _scene(name):
    """name -> (faces, S, image_size, anti_aliasing); seeded by the name's position in SCENES."""
    rng = np.random.default_rng(1000 + list(SCENES).index(name))
    kind, arg = SCENES[name]
    if kind == 'tile':           # one 32 x 32 tile, no anti-aliasing
        return box_faces(rng, arg(rng), TS), TS, TS, False
    return box_faces(rng, arg(rng), 2 * TS), 2 * TS, TS, True    # 2 x 2 tiles: image size 32 with anti-aliasing


SCENES = {}
for _n in (1, 2, 31, 32, 33, 63, 64, 65, 128, 256):   # the batch size and the old walk's lanes-per-face threshold; areas 1 .. FLAT_MAX
    SCENES['n%d' % _n] = ('tile', lambda rng, n=_n: random_boxes(rng, n, TS))
SCENES['area1'] = ('tile', lambda rng: same_boxes(rng, 200, 1, 1))
SCENES['area_small'] = ('tile', lambda rng: same_boxes(rng, 200, 8, 4))
SCENES['area_flat_max'] = ('tile', lambda rng: same_boxes(rng, 100, 16, 16))
# totals per batch (a short list is cut into four equal runs, one per wave; every face of a scene has the same area)
SCENES['total64'] = ('tile', lambda rng: same_boxes(rng, 4 * 8, 4, 2))
SCENES['total128'] = ('tile', lambda rng: same_boxes(rng, 4 * 16, 4, 2))
SCENES['total63'] = ('tile', lambda rng: same_boxes(rng, 4 * 9, 7, 1))
SCENES['total255'] = ('tile', lambda rng: same_boxes(rng, 4 * 15, 17, 1))
SCENES['total65'] = ('tile', lambda rng: same_boxes(rng, 4 * 5, 1, 13))
SCENES['total129'] = ('tile', lambda rng: same_boxes(rng, 4 * 43, 3, 1))
SCENES['area64_starts'] = ('tile', start_boxes)
SCENES['class_borders'] = ('tile', class_border_boxes)
SCENES['tiles_small'] = ('image', lambda rng: random_boxes(rng, 500, 2 * TS, amax=SMALL))
SCENES['tiles_medium'] = ('image', lambda rng: random_boxes(rng, 120, 2 * TS, amin=SMALL + 1)
                          + random_boxes(rng, 200, 2 * TS, amax=SMALL))
SCENES['tiles_borders'] = ('image', lambda rng: [(TS - 3, TS - 2, 8, 4), (TS - 1, 4, 2, 16), (20, TS - 8, 16, 16),
                                                  (TS - 16, TS - 16, 32, 32), (0, 0, 32, 32), (TS, TS, 32, 8)]
                           + random_boxes(rng, 300, 2 * TS, amax=SMALL))
# the long-list path (batches of 64 handed out as the waves become free, hierarchical depth cull on): maps only
SCENES['long300'] = ('tile', lambda rng: random_boxes(rng, 300, TS, amax=SMALL))
SCENES['long1000'] = ('tile', lambda rng: random_boxes(rng, 1000, TS, amax=SMALL))

_cache = {}


def scene_and_reference(name):
    """The scene, its face colours and the oracle's maps, computed once per module run and left unchanged."""
    if name not in _cache:
        faces, S, image_size, aa = _scene(name)
        nf = faces.shape[1]
        col = np.random.default_rng(7).uniform(-1, 1, (1, nf, 3)).astype(np.float32)
        tex = np.ascontiguousarray(np.broadcast_to(col[:, :, None, None, None, :], (1, nf, 2, 2, 2, 3)))
        ref = no.rasterize_rgbad(torch.tensor(faces), torch.tensor(tex), image_size, aa, 0.1, 100, 1e-3, (0.1, 0.2, 0.3),
                                 True, True, True)
        maps = tuple(ref[k].detach().numpy() for k in ('rgb', 'alpha', 'depth'))
        _cache[name] = (faces, col, S, image_size, aa, maps)
    return _cache[name]


def hip_maps(faces, col, image_size, aa):
    from sdn_hip import ops
    dev = torch.device('cuda:0')
    out = ops.RasterizeMaps.apply(torch.tensor(faces, device=dev), torch.tensor(col, device=dev), image_size, aa, 0.1, 100,
                                  1e-3, (0.1, 0.2, 0.3), True, True, True, None, True)
    return tuple(o.detach().cpu().numpy() for o in out)


@pytest.mark.parametrize('name', list(SCENES))
def test_maps_and_candidate_count(name):
    from sdn_hip import ops
    faces, col, S, image_size, aa, ref = scene_and_reference(name)
    total, largest, per_tile, boxes = candidate_tests(faces, S)
    with ops.verification(count_work=True):
        got = hip_maps(faces, col, image_size, aa)
        work = ops.last_work()
    for g, r, what in zip(got, ref, ('face colour', 'alpha', 'depth')):
        assert biteq(g, r), '%s map of scene %s differs from the oracle' % (what, name)
    assert ref[1].max() == 1.0, 'the scene covers some pixel'
    print('scene %s: %d faces, %d candidate tests expected, %d counted, largest clipped box %d, longest list %d'
          % (name, faces.shape[1], total, int(work[0]), largest, per_tile))
    if largest <= FLAT_MAX and per_tile <= 256:   # (row spans test fewer pixels than the box holds; long lists run the depth cull)
        assert int(work[0]) == total
    got2 = hip_maps(faces, col, image_size, aa)    # the timed build
    for g, r in zip(got2, ref):
        assert biteq(g, r)


def test_scene_construction_gives_the_prescribed_boxes():
    """(needs no GPU work of its own beyond the import: the boxes k_face_setup would compute are the prescribed ones)"""
    rng = np.random.default_rng(5)
    want = random_boxes(rng, 300, 2 * TS) + [(0, 0, 32, 32), (63, 63, 1, 1), (0, 63, 1, 1)]
    _, _, _, boxes = candidate_tests(box_faces(rng, want, 2 * TS), 2 * TS)
    assert np.array_equal(boxes, np.asarray(want))


@pytest.mark.parametrize('name', ['n65', 'tiles_medium'])
def test_list_overflow_path_walks_the_same_stream(name):
    from sdn_hip import ops
    faces, col, S, image_size, aa, ref = scene_and_reference(name)
    with ops.verification(stream_faces=True):
        got = hip_maps(faces, col, image_size, aa)
    for g, r in zip(got, ref):
        assert biteq(g, r)
