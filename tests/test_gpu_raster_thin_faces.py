"""The band path of k_raster_tiles after k_face_setup learnt two things about thin faces (tests/test_thin_faces_host.py):
faces with a repeated vertex are dropped, and slivers with a finite margin (THIN_MARGIN < m < S) are culled and clipped by
their dilated box as well as by the line through their longest edge; faces with m = -1 keep the whole line.

Scenes: slivers whose long edge runs THROUGH pixel centres (those pixels pass or fail by rounding alone, and the oracle
covers a good part of them), alone and among ordinary faces and repeated-vertex faces.  Maps are compared bit for bit with
the oracle at S = 96 without anti-aliasing (3 x 3 tiles) and at S = 64 with it (image size 32, 2 x 2 tiles).
"""
import numpy as np
import pytest
import torch

from oracle import nr_oracle as no
from test_thin_faces_host import face_margin_px, repeated_vertex_faces
from util import biteq, random_soup

pytestmark = pytest.mark.gpu
F = np.float32
THIN_MARGIN = 4.0

# end points of the long edges in pixels of the 96 x 96 image: horizontal, vertical, both diagonals, three oblique
EDGES = [((3, 5), (90, 5)), ((7, 2), (7, 93)), ((2, 2), (92, 92)), ((4, 80), (84, 0)), ((1, 10), (91, 40)),
         ((10, 1), (40, 91)), ((20, 60), (52, 64))]
# apex distance from the edge midpoint in pixels: (all 28 margins in THIN_MARGIN .. S, 8 of the 28 margins -1) at either size --
# the margin grows with the internal size, so the smaller image takes the smaller offsets
APEX = {96: (1e-3, 3e-4), 64: (4e-4, 2e-4)}


def slivers(rng, S, apex_off):
    """7 edges x apex on either side x both windings = 28 faces [28, 3, 3]; the apex is apex_off pixels off the midpoint."""
    out = []
    for a, b in EDGES:
        a = np.floor(np.asarray(a, np.float64) * S / 96.0)
        b = np.floor(np.asarray(b, np.float64) * S / 96.0)
        d = b - a
        nrm = np.array([-d[1], d[0]]) / np.hypot(d[0], d[1])
        for side in (-1.0, 1.0):
            pix = np.stack([a, b, 0.5 * (a + b) + side * apex_off * nrm])
            v = np.concatenate([(2.0 * pix + 1.0 - S) / S, rng.uniform(0.5, 5.0, (3, 1))], 1).astype(F)
            out.append(v)
            out.append(v[::-1].copy())
    return np.stack(out)


def is_thin(f, S):
    m = face_margin_px(f, S)
    return ~((m > 0) & (m <= F(THIN_MARGIN)))


def mixed(rng, S):
    """[3, 288, 3, 3]: object 0 = 28 bounded slivers, 200 small ordinary faces, 60 repeated-vertex faces; object 1 = 14
    slivers on the whole-line path among 274 ordinary faces; object 2 = ordinary faces only."""
    def soup(n):
        f = random_soup(rng, 1, 2 * n, 0.05)[0]
        f = f[~is_thin(f, S)][:n]
        assert len(f) == n
        return f
    rep = repeated_vertex_faces(rng, 4)                                      # 72 faces built for S = 96 ...
    rep = rep[rng.permutation(len(rep))[:60]]                                # ... a repeated vertex is one at any size
    a = np.concatenate([slivers(rng, S, APEX[S][0]), soup(200), rep])
    b = np.concatenate([soup(274), slivers(rng, S, APEX[S][1])[::2]])
    c = soup(288)
    return np.stack([a[rng.permutation(288)], b[rng.permutation(288)], c])


def _scene(name):
    """name -> (faces [bs, nf, 3, 3], S, image size, anti-aliasing)"""
    kind, size = name.split('_')
    S, image_size, aa = (96, 96, False) if size == '96' else (64, 32, True)
    rng = np.random.default_rng(2000 + list(SCENES).index(name))
    if kind == 'covering':
        return slivers(rng, S, APEX[S][0])[None], S, image_size, aa
    if kind == 'wholeline':
        return slivers(rng, S, APEX[S][1])[None], S, image_size, aa
    return mixed(rng, S), S, image_size, aa


SCENES = ['covering_96', 'covering_64', 'wholeline_96', 'wholeline_64', 'mixed_96', 'mixed_64']
_cache = {}


def scene_and_reference(name):
    """The scene, its face colours and the oracle's maps, computed once per module run and left unchanged.  The oracle draws
    one object per call: its texture sampling restates the reference's, which looks the face's depths up without the batch
    offset (rasterize.py:390), so the colours of a batch are the reference's only for its first object."""
    if name not in _cache:
        faces, S, image_size, aa = _scene(name)
        bs, nf = faces.shape[:2]
        col = np.random.default_rng(7).uniform(-1, 1, (bs, nf, 3)).astype(F)
        tex = np.ascontiguousarray(np.broadcast_to(col[:, :, None, None, None, :], (bs, nf, 2, 2, 2, 3)))
        refs = [no.rasterize_rgbad(torch.tensor(faces[b:b + 1]), torch.tensor(tex[b:b + 1]), image_size, aa, 0.1, 100, 1e-3,
                                   (0.1, 0.2, 0.3), True, True, True) for b in range(bs)]
        maps = tuple(np.concatenate([r[k].detach().numpy() for r in refs]) for k in ('rgb', 'alpha', 'depth'))
        _cache[name] = (faces, col, S, image_size, aa, maps)
    return _cache[name]


def hip_maps(faces, col, image_size, aa):
    from sdn_hip import ops
    dev = torch.device('cuda:0')
    out = ops.RasterizeMaps.apply(torch.tensor(faces, device=dev), torch.tensor(col, device=dev), image_size, aa, 0.1, 100,
                                  1e-3, (0.1, 0.2, 0.3), True, True, True, None, True)
    return tuple(o.detach().cpu().numpy() for o in out)


def covered_internal_pixels(alpha, aa):
    """internal pixels the oracle covers (an anti-aliased alpha is the mean of 2 x 2 internal pixels)"""
    return int(round(float(alpha.astype(np.float64).sum()) * (4 if aa else 1)))


@pytest.mark.parametrize('name', SCENES)
def test_maps_equal_the_oracle(name):
    faces, col, S, image_size, aa, ref = scene_and_reference(name)
    kind = name.split('_')[0]
    m = face_margin_px(faces[0], S)
    n_cov = covered_internal_pixels(ref[1][0], aa)
    print('scene %s: %d faces per object, object 0: margins of the thin faces %s, %d on the whole-line path, oracle covers %d internal pixels'
          % (name, faces.shape[1], np.sort(m[m > THIN_MARGIN])[[0, -1]] if (m > THIN_MARGIN).any() else '-', int((m < 0).sum()), n_cov))
    if kind == 'covering':
        # the construction puts every sliver on the boxed path, and the oracle's coverage gives the comparison something to bite on
        assert ((m > THIN_MARGIN) & (m < S)).all()
        assert n_cov >= (300 if S == 96 else 150)
    if kind == 'wholeline':
        assert (m < 0).sum() >= 4 and ((m > THIN_MARGIN) & (m < S)).sum() >= 4
        assert n_cov >= 100
    if kind == 'mixed':
        thin = [int(is_thin(faces[b], S).sum()) for b in range(3)]
        assert thin[0] > thin[1] > 0 and thin[2] == 0, thin
    got = hip_maps(faces, col, image_size, aa)
    for g, r, what in zip(got, ref, ('face colour', 'alpha', 'depth')):
        assert biteq(g, r), '%s map of scene %s differs from the oracle in %d values' % (what, name, int((g != r).sum()))


@pytest.mark.parametrize('name', ['mixed_96', 'mixed_64'])
def test_list_overflow_path_draws_the_same_maps(name):
    from sdn_hip import ops
    faces, col, S, image_size, aa, ref = scene_and_reference(name)
    with ops.verification(stream_faces=True):
        got = hip_maps(faces, col, image_size, aa)
    for g, r in zip(got, ref):
        assert biteq(g, r)


def rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize('name', ['mixed_96', 'mixed_64'])
def test_alpha_backward_matches_the_oracle(name):
    """Silhouette-only gradient of the mixed scene: 1e-5 relative L2, the gate of tests/test_gpu_raster.py."""
    from sdn_hip import ops
    faces, col, S, image_size, aa, ref = scene_and_reference(name)
    dev = torch.device('cuda:0')
    ft = torch.tensor(faces, device=dev, requires_grad=True)
    alpha = ops.RasterizeMaps.apply(ft, None, image_size, aa, 0.1, 100, 1e-4, None, False, True, False, None, False)[1]
    fo = torch.tensor(faces, requires_grad=True)
    alpha_o = no.rasterize_rgbad(fo, None, image_size, aa, 0.1, 100, 1e-4, None, False, True, False)['alpha']
    assert biteq(alpha.detach().cpu().numpy(), alpha_o.detach().numpy())
    g = np.random.default_rng(3).normal(size=tuple(alpha_o.shape)).astype(F)
    (alpha * torch.tensor(g, device=dev)).sum().backward()
    (alpha_o * torch.tensor(g)).sum().backward()
    gh, go = ft.grad.cpu().numpy(), fo.grad.numpy()
    assert np.isfinite(go).all() and np.abs(go).max() > 0
    err = rel_l2(gh, go)
    print('scene %s: alpha-only gradient relative L2 %.3g' % (name, err))
    assert err < 1e-5
