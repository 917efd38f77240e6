"""The C restatement (oracle/raster_oracle.c) must equal, bit for bit, the reference's own kernel strings
compiled for the CPU (oracle/_ref, built by oracle/build_ref.py where the reference checkout exists).  Where oracle/_ref
is absent the oracle is held to tests/golden/ref_digests.json instead: the digests of what the reference's kernels
returned on the same seeded inputs (tests/golden/make_ref_digests.py)."""
import numpy as np
import pytest

from oracle import raster_np as rn
from util import biteq, digest, random_soup, recorded_digests

MAPS = ['face_index_map', 'weight_map', 'depth_map', 'face_inv_map', 'rgb_map', 'alpha_map', 'sampling_index_map',
        'sampling_weight_map']
FWD_CASES = [(50, 32, 0.3, 2), (300, 48, 0.1, 3), (1500, 96, 0.04, 2)]
NEAR_FAR = ((0.1, 100), (0.5, 2.0), (0.3, 1.7))


def forward_backward_case(nf, is_, scale, ts, unsafe, impl):
    rng = np.random.default_rng(nf + is_)
    faces = random_soup(rng, 1, nf, scale)
    tex = rng.uniform(0, 1, (1, nf, ts, ts, ts, 3)).astype(np.float32)
    s = rn.forward(faces, tex, is_, 0.1, 100, 1e-3, (0.1, 0.2, 0.3), True, True, True, unsafe=unsafe, impl=impl)
    out = {k: getattr(s, k) for k in MAPS}
    g_rgb = rng.normal(size=s.rgb_map.shape).astype(np.float32)
    g_a = rng.normal(size=s.alpha_map.shape).astype(np.float32)
    g_d = rng.normal(size=s.depth_map.shape).astype(np.float32)
    g = rn.backward(s, g_rgb, g_a, g_d)
    out['grad_faces'], out['grad_textures'] = g[0], g[1]
    return out


def multi_batch_case(impl):
    # bs > 1 is only well defined without rgb (rasterize.py:390 drops the batch offset in K4)
    rng = np.random.default_rng(7)
    faces = random_soup(rng, 3, 200, 0.15)
    s = rn.forward(faces, None, 40, 0.1, 100, 1e-4, None, False, True, True, impl=impl)
    out = {k: getattr(s, k) for k in ('face_index_map', 'weight_map', 'depth_map', 'face_inv_map', 'alpha_map')}
    g = rng.normal(size=s.alpha_map.shape).astype(np.float32)
    out['grad_faces'] = rn.backward(s, None, g, g)[0]
    return out


def near_far_case(impl):
    # the reference pastes near/far into the kernel text: comparisons happen in double
    rng = np.random.default_rng(11)
    faces = random_soup(rng, 1, 120, 0.3, zlo=0.05, zhi=3.0)
    out = {}
    for near, far in NEAR_FAR:
        s = rn.forward(faces, None, 32, near, far, 1e-4, None, False, True, True, impl=impl)
        out['%g_%g/depth_map' % (near, far)] = s.depth_map
        out['%g_%g/face_index_map' % (near, far)] = s.face_index_map
    return out


def cases():
    """(key, case, args) of every comparison below: what tests/golden/make_ref_digests.py records."""
    for nf, is_, scale, ts in FWD_CASES:
        for unsafe in (False, True):
            yield 'raster/fwd_bwd/%d_%d_%g_%d_%d' % (nf, is_, scale, ts, unsafe), forward_backward_case, (nf, is_, scale, ts, unsafe)
    yield 'raster/multi_batch', multi_batch_case, ()
    yield 'raster/near_far', near_far_case, ()


def oracle_equals_reference(key):
    """Runs one case on the oracle and demands bit equality with the reference's kernels: live where oracle/_ref is built,
    else through the recorded digests of the reference's outputs.  Returns the oracle's arrays."""
    _, case, args = next(c for c in cases() if c[0] == key)
    a = case(*args, impl='oracle')
    if rn.have_ref():
        b = case(*args, impl='ref')
        assert sorted(a) == sorted(b)
        for k in a:
            assert biteq(a[k], b[k]), k
    else:
        want = recorded_digests()[key]
        assert sorted(a) == sorted(want)
        for k in a:
            assert digest(a[k]) == want[k], k
    return a


@pytest.mark.parametrize('nf,is_,scale,ts', FWD_CASES)
@pytest.mark.parametrize('unsafe', [False, True])
def test_forward_backward_bit_equal(nf, is_, scale, ts, unsafe):
    a = oracle_equals_reference('raster/fwd_bwd/%d_%d_%g_%d_%d' % (nf, is_, scale, ts, unsafe))
    assert (a['face_index_map'] >= 0).sum() > 0


def test_multi_batch_without_textures():
    oracle_equals_reference('raster/multi_batch')


def test_near_far_literals():
    oracle_equals_reference('raster/near_far')
