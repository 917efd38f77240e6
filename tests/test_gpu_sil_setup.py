"""Set-up of the silhouette backward (k_cover_bits + k_compact_rows in raster_bwd.hip): coverage bit maps in both
orientations, the upstream gradient transposed at output resolution, and from them every row's and column's list of
non-zero h = max(-g_alpha, 0) on background pixels.

The lists have no entry point of their own; what they feed is the silhouette gradient, compared here with the CPU oracle
at the yardstick of tests/test_gpu_raster.py for wave-mode gradients (relative L2 below 1e-5).  A wrong bit, count or
list entry moves a whole scan, far above that bound.  Sizes are the smallest at which the structure can go wrong:
32-bit coverage words (S around 32 / 64 / 128, the padded last word), the 64 lanes of a row's wave (R around 64), both
alignments of the 16-bit count rows (S + 1 entries: every other row starts off a word when S is even), and rows longer
than one group of 384 output elements (S = 385 without anti-aliasing, R = 385 with it).  bs = 3, so that row numbers
cross objects.
"""
import numpy as np
import pytest
import torch

from test_gpu_raster import hip_rasterize, oracle_rasterize, rel_l2
from util import biteq, random_soup

pytestmark = pytest.mark.gpu
FLAGS = (False, True, False)   # silhouette only: the fast path
NO_AA = [2, 17, 31, 32, 33, 63, 64, 65, 127, 129]   # internal size S = image size
AA = [16, 17, 33, 65]                               # image size R, S = 2 R


def cover_pair(z):
    """Two triangles (both windings of each, so one of them faces the camera) that cover the whole view."""
    a, b, c, d = (-3., -3., z), (3., -3., z), (3., 3., z), (-3., 3., z)
    return np.array([[a, b, c], [a, c, b], [a, c, d], [a, d, c]], np.float32)


def mixed_scene(rng, nf=48):
    """object 0: a soup with faces across all four image borders; object 1: covered completely (every list is empty);
    object 2: nothing in view (no visible face; every pixel is background)."""
    faces = random_soup(rng, 3, nf, 0.4)
    faces[1:, :, :, 0] += 10.0
    faces[1, :4] = cover_pair(1.0)
    return faces


def upstream(rng, shape, kind):
    g = rng.normal(size=shape).astype(np.float32)
    if kind == 'neg':    # every background pixel is a list entry: the lists reach their maximum length
        g = -np.abs(g) - 0.1
    elif kind == 'pos':  # h = 0 everywhere: every list is empty
        g = np.abs(g) + 0.1
    return g


def check(faces, image_size, aa, kind, seed=0):
    ft, _, (_, a, _) = hip_rasterize(faces, None, image_size, aa, FLAGS, eps=1e-4, bg=None)
    fo, _, (_, r, _) = oracle_rasterize(faces, None, image_size, aa, FLAGS, eps=1e-4, bg=None)
    assert biteq(a.detach().cpu().numpy(), r.detach().numpy())
    g = upstream(np.random.default_rng(seed), tuple(a.shape), kind)
    (a * torch.tensor(g, device=a.device)).sum().backward()
    (r * torch.tensor(g)).sum().backward()
    gh, go = ft.grad.cpu().numpy(), fo.grad.numpy()
    err = rel_l2(gh, go)
    print('S_out %d aa %d %s: |grad| %.4g rel L2 %.3g' % (image_size, aa, kind, np.linalg.norm(go), err))
    assert np.isfinite(gh).all()
    assert err < 1e-5
    return go


@pytest.mark.parametrize('image_size,aa', [(s, False) for s in NO_AA] + [(r, True) for r in AA])
def test_soup_random_sign(image_size, aa):
    rng = np.random.default_rng(100 + image_size)
    go = check(random_soup(rng, 3, 64, 0.3), image_size, aa, 'random', seed=image_size)
    assert np.abs(go).max() > 0


@pytest.mark.parametrize('kind', ['random', 'neg', 'pos'])
@pytest.mark.parametrize('image_size,aa', [(33, False), (65, False), (17, True), (33, True)])
def test_full_cover_empty_object_and_gradient_signs(image_size, aa, kind):
    rng = np.random.default_rng(7 * image_size + aa)
    go = check(mixed_scene(rng), image_size, aa, kind, seed=3)
    assert np.abs(go[0]).max() > 0
    assert not go[1:].any()   # a face that covers the view has no edge in it; object 2 has no face in view


@pytest.mark.parametrize('image_size,aa,kind', [(385, False, 'neg'), (385, True, 'random')])
def test_rows_longer_than_one_group(image_size, aa, kind):
    """One output element more than a group: the running count is carried into a second group of one lane.
    (S = 770 is not run with the all-negative gradient: a scan then adds up to 770 terms of one sign, and the order in
    which k_edge_rows adds them -- not touched by the set-up -- differs from the oracle's serial sum by 2.5e-5 relative
    L2 with bit-identical lists; the yardstick belongs to sums of the sizes above.)"""
    rng = np.random.default_rng(385 + aa)
    check(random_soup(rng, 3, 24, 0.3), image_size, aa, kind, seed=5)


def test_workspace_bytes_are_what_they_were():
    """The set-up structures live inside the slots of the layout that had the dense h map: the size the library asks
    for is part of its ABI (callers cache workspaces by it).  Values returned by the build before this set-up."""
    import ctypes
    import sdn_hip
    for (bs, nf, S), want in (((16, 89800, 768), 1850279680), ((3, 64, 17), 6026240), ((1, 5000, 130), 10023424)):
        n = ctypes.c_size_t(0)
        sdn_hip.check(sdn_hip.lib().sdn_raster_bwd_workspace_bytes(bs, nf, S, ctypes.byref(n)))
        assert n.value == want, (bs, nf, S, n.value, want)
