"""The candidate stream of k_raster_tiles when a stream position is a RUN of G horizontally adjacent pixels (STREAM_G = 1, 2, 4).

A face with a clipped box of w x h <= FLAT_MAX pixels contributes ceil(w / G) * h positions; a lane computes what the run's
pixels share (owner look-up, operands, the row half of the edge tests) once and tests up to G pixels, masking those past the
box's last column.  The scenes below are the smallest at which that can go wrong -- short last runs, runs that would leave the
tile, pass boundaries in run units for G = 2 and G = 4, a hit queue that fills within one pass -- and they pin RESULTS, not the
implementation: they hold for one pixel per position as well.  Every scene asserts
  * rgb / alpha / depth and the face-index map bit-equal to oracle.nr_oracle (the face-index map from the same oracle kernel,
    oracle.raster_np.forward, that nr_oracle.Rasterize runs),
  * the counting build's candidate tests == the sum of the clipped box areas, wherever every box of the scene is in the stream
    and no depth cull runs (the rule of test_gpu_raster_flat_walk: row spans test fewer pixels than their box holds, a list of
    more than 256 entries runs the hierarchical depth cull).  `mixed_spans` holds row-span boxes and still gets an equality:
    a face's row-span tests depend on the face and the tile alone, so the scene's count less the count of its row-span faces
    rendered alone must be the summed area of its stream boxes.  `mixed` (258 entries: depth cull on) asserts only that no
    more tests are counted than the boxes hold,
  * every margin below 0.05 (candidate_tests' own assertions).

Pass boundaries: a short list is cut into four equal runs, one per wave, in whatever order the binning produced, so a scene that
needs an exact run count per wave uses faces of one size.  8 x 1 and 4 x 1 boxes give 64 and 128 runs per wave; their run counts
are even at G = 2, so 63 and 65 come from 2 x 1 (one run), 10 x 1 (five runs at G = 2) and 20 x 1 (five runs at G = 4) boxes.
"""
import numpy as np
import pytest
import torch

from oracle import nr_oracle as no
from test_gpu_raster_flat_walk import box_faces, candidate_tests, random_boxes, same_boxes
from util import biteq

pytestmark = pytest.mark.gpu

TS = 32
FLAT_MAX = 256
DEV = 'cuda:0'


def runs(boxes, G):
    """stream positions of (already clipped) boxes at G pixels per run"""
    return sum(-(-w // G) * h for _, _, w, h in boxes)


def grid_boxes(rng, h, widths=range(1, 10)):
    """every width at an even and an odd first column (short last runs, single-pixel rows, at h = 32 a 1 x 32 column)"""
    out = []
    for w in widths:
        for parity in (0, 1):
            x0 = 2 * int(rng.integers(0, (TS - w - parity) // 2 + 1)) + parity
            out.append((x0, int(rng.integers(0, TS - h + 1)), w, h))
    return out


def column31_boxes(rng):
    """boxes whose last column is tile column 31: the last run of a row starts at column 31 (odd widths at G = 2, widths 1 mod 4
    at G = 4) and its masked pixels would be xtab[32..34] and the next row of the depth buffer"""
    out = []
    for w in range(1, 10):
        for h in (1, 2, 5):
            out.append((TS - w, int(rng.integers(0, TS - h + 1)), w, h))
    out += [(TS - 1, 0, 1, TS), (TS - 1, TS - 1, 1, 1), (TS - 1, TS - 2, 1, 2), (TS - 5, TS - 1, 5, 1)]
    return out


def straddling_boxes(rng):
    """S = 64: boxes across the tile border at columns 31 / 32 (clipped widths 1 | 3, 3 | 5, 5 | 1, 1 | 1, 2 | 7: odd from even)
    and the same across the row border"""
    out = []
    for x0, w in ((31, 4), (29, 8), (27, 6), (31, 2), (30, 9)):
        for y0, h in ((3, 1), (30, 4), (40, 7)):
            out.append((x0, y0, w, h))
    return out + random_boxes(rng, 40, 2 * TS, amax=32)


def two_per_wave(w, h):
    """eight faces of ceil(w / G) * h = 63 runs: whichever of a wave's two comes first, the other's runs start at position 63 of
    the first pass and continue into the next"""
    return lambda rng: same_boxes(rng, 8, w, h)


def half_covered_rows(rng):
    """128 disjoint 8 x 1 boxes (4 per row), each covering its first 4 pixels: 512 hits from 512 runs at G = 2 (every pass fills
    the queue exactly), from 256 runs at G = 4 (128 hits per pass of 64 runs)"""
    return [(8 * k, y, 8, 1) for y in range(TS) for k in range(4)]


def mixed_boxes(n):
    def make(rng):
        small = random_boxes(rng, n, TS)
        big = [(3, 9, 16, 17), (14, 2, 16, 17)]
        return small[:n // 3] + big[:1] + small[n // 3:2 * n // 3] + big[1:] + small[2 * n // 3:]
    return make


SCENES = {
    'grid_h1': ('tile', lambda rng: grid_boxes(rng, 1)),
    'grid_h2': ('tile', lambda rng: grid_boxes(rng, 2)),
    'grid_h32': ('tile', lambda rng: grid_boxes(rng, 32, range(1, 9))),
    'grid_h32_w9': ('tile', lambda rng: grid_boxes(rng, 32, [9]) + grid_boxes(rng, 32, [1, 3])),   # 288 pixels: row spans
    'column31': ('tile', column31_boxes),
    'straddle': ('image', straddling_boxes),
    # runs per wave (faces per wave x runs per face); G = 2
    'g2_runs63': ('tile', lambda rng: same_boxes(rng, 4 * 63, 2, 1)),
    'g2_runs64': ('tile', lambda rng: same_boxes(rng, 4 * 16, 8, 1)),
    'g2_runs65': ('tile', lambda rng: same_boxes(rng, 4 * 13, 10, 1)),
    'g2_runs128': ('tile', lambda rng: same_boxes(rng, 4 * 32, 8, 1)),
    'g2_runs128_w4': ('tile', lambda rng: same_boxes(rng, 4 * 64, 4, 1)),
    # G = 4
    'g4_runs63': ('tile', lambda rng: same_boxes(rng, 4 * 63, 4, 1)),
    'g4_runs64': ('tile', lambda rng: same_boxes(rng, 4 * 32, 8, 1)),
    'g4_runs64_w4': ('tile', lambda rng: same_boxes(rng, 4 * 64, 4, 1)),
    'g4_runs65': ('tile', lambda rng: same_boxes(rng, 4 * 13, 20, 1)),
    'g4_runs128': ('tile', lambda rng: same_boxes(rng, 4 * 64, 8, 1)),
    'g2_start63': ('tile', two_per_wave(6, 21)),
    'g4_start63': ('tile', two_per_wave(12, 21)),
    'hits_per_pass': ('tile', half_covered_rows),
    'mixed': ('tile', mixed_boxes(256)),
    'mixed_spans': ('tile', mixed_boxes(120)),
}
RUNS_PER_WAVE = {'g2_runs63': (2, 63), 'g2_runs64': (2, 64), 'g2_runs65': (2, 65), 'g2_runs128': (2, 128),
                 'g2_runs128_w4': (2, 128), 'g4_runs63': (4, 63), 'g4_runs64': (4, 64), 'g4_runs64_w4': (4, 64),
                 'g4_runs65': (4, 65), 'g4_runs128': (4, 128), 'g2_start63': (2, 126), 'g4_start63': (4, 126)}

_cache = {}


def colours(nf):
    return np.random.default_rng(7).uniform(-1, 1, (1, nf, 3)).astype(np.float32)


def oracle_maps(faces, col, S, image_size, aa):
    nf = faces.shape[1]
    tex = np.ascontiguousarray(np.broadcast_to(col[:, :, None, None, None, :], (1, nf, 2, 2, 2, 3)))
    ref = no.rasterize_rgbad(torch.tensor(faces), torch.tensor(tex), image_size, aa, 0.1, 100, 1e-3, (0.1, 0.2, 0.3),
                             True, True, True)
    fim = no.raster_np.forward(faces, None, S, 0.1, 100, 1e-3, None, False, True, True).face_index_map
    return tuple(ref[k].detach().numpy() for k in ('rgb', 'alpha', 'depth')) + (fim,)


def scene_and_reference(name):
    """The scene, its face colours and the oracle's maps, computed once per module run and left unchanged."""
    if name not in _cache:
        rng = np.random.default_rng(2000 + list(SCENES).index(name))
        kind, make = SCENES[name]
        S, aa = (TS, False) if kind == 'tile' else (2 * TS, True)
        boxes = make(rng)
        faces = box_faces(rng, boxes, S)
        col = colours(faces.shape[1])
        _cache[name] = (boxes, faces, col, S, TS, aa, oracle_maps(faces, col, S, TS, aa))
    return _cache[name]


def hip_maps(faces, col, image_size, aa):
    from sdn_hip import ops
    out = ops.RasterizeMaps.apply(torch.tensor(faces, device=DEV), torch.tensor(col, device=DEV), image_size, aa, 0.1, 100,
                                  1e-3, (0.1, 0.2, 0.3), True, True, True, None, True)
    return tuple(o.detach().cpu().numpy() for o in out)


def hip_face_index(faces, S, extra_flags=0):
    from sdn_hip import ALPHA, SAVE_MAPS, check, lib, ptr, raster_workspace, stream
    f = torch.tensor(np.ascontiguousarray(faces, dtype=np.float32), device=DEV)
    bs, nf = f.shape[:2]
    face_inv = torch.empty((bs, nf, 3, 3), device=DEV)
    fim = torch.empty((bs, S, S), dtype=torch.int32, device=DEV)
    wmap = torch.empty((bs, S, S, 3), device=DEV)
    dmap = torch.empty((bs, S, S), device=DEV)
    alpha = torch.empty((bs, S, S), device=DEV)
    ws = raster_workspace(bs, nf, S, f.device)
    check(lib().sdn_rasterize_fwd(ptr(f), None, 0, bs, nf, S, 0.1, 100.0, 1e-3, None, 0, ALPHA | SAVE_MAPS | extra_flags,
                                  ptr(face_inv), ptr(fim), ptr(wmap), ptr(dmap), None, None, ptr(alpha), None, ptr(ws),
                                  ws.numel(), stream()))
    torch.cuda.synchronize()
    return fim.cpu().numpy()


def counted(faces, col, image_size, aa):
    from sdn_hip import ops
    with ops.verification(count_work=True):
        got = hip_maps(faces, col, image_size, aa)
        work = ops.last_work()
    return got, int(work[0])


def assert_maps(got, ref, name, what='timed'):
    for g, r, m in zip(got, ref, ('face colour', 'alpha', 'depth')):
        assert biteq(g, r), '%s map of scene %s (%s build) differs from the oracle' % (m, name, what)


@pytest.mark.parametrize('name', list(SCENES))
def test_maps_face_index_and_candidate_count(name):
    boxes, faces, col, S, image_size, aa, ref = scene_and_reference(name)
    total, largest, per_tile, got_boxes = candidate_tests(faces, S)
    assert np.array_equal(got_boxes, np.asarray(boxes)), 'the candidate boxes are the prescribed ones'
    if name in RUNS_PER_WAVE:   # the scene is what its name says: runs per wave at that G
        G, want = RUNS_PER_WAVE[name]
        assert len(boxes) % 4 == 0 and per_tile <= 256 and runs(boxes, G) == 4 * want
    got, n_cand = counted(faces, col, image_size, aa)
    assert_maps(got, ref, name, 'counting')
    assert ref[1].max() == 1.0, 'the scene covers some pixel'
    print('scene %s: %d faces, %d candidate tests expected, %d counted, largest clipped box %d, longest list %d'
          % (name, faces.shape[1], total, n_cand, largest, per_tile))
    if largest <= FLAT_MAX and per_tile <= 256:
        assert n_cand == total
    elif per_tile <= 256:
        # row-span faces test the same pixels wherever they are listed: what is left is the stream's share
        big = np.asarray([w * h > FLAT_MAX for _, _, w, h in boxes])
        _, n_big = counted(faces[:, big], col[:, big], image_size, aa)
        flat_total = candidate_tests(faces[:, ~big], S)[0]
        print('   row-span faces alone: %d tests; stream boxes hold %d pixels' % (n_big, flat_total))
        assert n_cand - n_big == flat_total
    else:
        assert n_cand <= total   # (depth cull: faces hidden behind what is drawn are never walked)
    assert_maps(hip_maps(faces, col, image_size, aa), ref, name)
    assert np.array_equal(hip_face_index(faces, S), ref[3]), 'face-index map of scene %s differs from the oracle' % name


def test_hits_per_pass_scene_fills_the_queue_within_one_pass():
    """(CPU side) from the oracle's alpha: the scene's covered pixels per 64 runs.  A right triangle covers at most half of its
    box, so at G = 2 a pass of 64 runs yields exactly 64 hits -- the queue drains with nothing left, every pass -- and at
    G = 4 it yields 128: more than push_hits accepts at once and as much as the queue holds."""
    boxes, faces, col, S, image_size, aa, ref = scene_and_reference('hits_per_pass')
    assert len(boxes) >= 64 and all(w == 8 and h == 1 for _, _, w, h in boxes)
    covered = int((ref[1] == 1.0).sum())
    assert covered * 64 > 64 * runs(boxes, 4), 'more than 64 covered pixels per 64 runs of four'
    assert covered * 64 >= 64 * runs(boxes, 2), '64 covered pixels per 64 runs of two'
    assert covered == 4 * len(boxes), 'half of each row passes'


def test_list_overflow_fallback_walks_the_same_runs():
    """the fallback (every tile streams every face's tile box) calls the same raster_batch; forced as in
    test_gpu_raster_thin_faces.py.  It runs no depth cull, so the count is exact here too."""
    from sdn_hip import STREAM_FACES, ops
    name = 'straddle'
    boxes, faces, col, S, image_size, aa, ref = scene_and_reference(name)
    total = candidate_tests(faces, S)[0]
    with ops.verification(stream_faces=True):
        got, n_cand = counted(faces, col, image_size, aa)
        got2 = hip_maps(faces, col, image_size, aa)
    assert_maps(got, ref, name, 'counting, fallback')
    assert_maps(got2, ref, name, 'timed, fallback')
    assert n_cand == total
    assert np.array_equal(hip_face_index(faces, S, STREAM_FACES), ref[3])
