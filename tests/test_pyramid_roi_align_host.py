"""The pyramid RoIAlign without a GPU: the numpy restatement of tests/pyramid_roi_align_util.py against the fixture
tests/golden/pyramid_roi_align_golden.npz (the reference's own functions on its own C crop, run by
tests/golden/make_pyramid_roi_align_golden.py), the entry points' names in header, binding and library, the build list, the
constants the Python side mirrors, the argument checks of sdn_pyramid_roi_align_fwd / _bwd / _grad_floats and of the wrappers, all
of which run before any launch, and the check header under ASan and UBSan in a stand-alone host program."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import host_checks
import makefile_rules
import pyramid_roi_align_util as u
from maskrcnn import pyramid   # the feature itself: without it this module does not import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_pyramid_roi_align_grad_floats', 'sdn_pyramid_roi_align_fwd', 'sdn_pyramid_roi_align_bwd')


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_gives_the_references_numbers(gold, name):
    c = u.draw_case(name)
    p = name + '/'
    assert int(gold[p + 'crc_boxes']) == u.checksum(c['boxes']) and int(gold[p + 'crc_grads']) == u.checksum(c['grads'])
    assert gold[p + 'crc_maps'].tolist() == [u.checksum(m) for m in c['maps']]
    assert gold[p + 'boxes'].dtype == np.float32 and np.array_equal(gold[p + 'boxes'], c['boxes'])
    assert np.array_equal(u.levels(c), gold[p + 'levels'])
    out = u.forward(c, np.float32)
    assert out.dtype == np.float32 and u.checksum(out) == int(gold[p + 'crc_pooled'])
    if name in u.STORED_WHOLE:
        assert out.tobytes() == gold[p + 'pooled'].tobytes()            # bit for bit
    # the float64 forward is the same function: it differs from the float32 one by float32's rounding of three lerps
    assert np.abs(u.forward(c) - out).max() <= 32 * 2.0 ** -24 * max(np.abs(m).max() for m in c['maps'])
    g64 = u.backward(c)
    ref32 = [gold[p + 'grad32_%d' % l] for l in range(u.LEVELS)]
    for l in range(u.LEVELS):
        want = gold[p + 'grad64_%d' % l]
        assert want.dtype == np.float64 and g64[l].shape == want.shape == ref32[l].shape
        assert np.allclose(g64[l], want, rtol=1e-12, atol=1e-300), l
    # the reference's float32 gradients lie at the stored distance from the float64 ones
    assert np.allclose(u.grad_error(ref32, g64), gold[p + 'fp32_error'], rtol=1e-6, atol=1e-12)


def test_the_fixture_holds_what_the_cases_are_there_for(gold):
    assert os.path.getsize(u.GOLD) < 400 * 1024
    assert tuple(gold['image_shape']) == u.IMAGE_SHAPE and u.IMAGE_AREA == 1024.0 * 1024.0
    lv = {n: gold[n + '/levels'] for n in u.CASES}
    for name in u.CASES:
        k = u.CASES[name]
        # the gate: 1e-6 per level map, or four times what the reference's own float32 run is off where that is more
        err, gate = gold[name + '/fp32_error'], gold[name + '/gate']
        assert err.shape == gate.shape == (4,) and np.array_equal(gate, np.where(err <= u.GATE, u.GATE, 4 * err)), name
        assert len(lv[name]) == k['R'] and lv[name].min() >= 2 and lv[name].max() <= 5
        for l in range(u.LEVELS):
            g32, g64 = gold[name + '/grad32_%d' % l], gold[name + '/grad64_%d' % l]
            assert g32.shape == g64.shape == (k['C'],) + tuple(k['maps'][l])
            if not (lv[name] == l + 2).any():          # the reference's `continue` branch: no gradient at all
                assert not g32.any() and not g64.any() and err[l] == 0.0
    assert all(set(lv[n].tolist()) == {2, 3, 4, 5} for n in ('mixed7', 'mixed14', 'thin', 'big'))
    assert (u.CASES['mixed7']['R'], u.CASES['mixed7']['C'], u.CASES['mixed7']['maps']) == (37, 5, ((24, 20), (12, 10), (6, 5), (3, 3)))
    assert u.CASES['mixed7']['pool'] == 7 and u.CASES['mixed14']['pool'] == 14 and np.array_equal(gold['mixed7/boxes'], gold['mixed14/boxes'])
    assert set(lv['onelevel'].tolist()) == {3} and len(lv['single']) == 1
    b = gold['outside/boxes']
    assert ((b.min(1) < 0) | (b.max(1) > 1)).all()
    o = gold['outside/pooled']
    assert (o == 0).all(axis=1).any() and (o != 0).any()
    v = u.level_values(gold['clamp/boxes'])
    assert (v < 1.5).sum() == 8 and (v > 5.5).sum() == 8 and set(lv['clamp'].tolist()) == {2, 5}
    v = u.level_values(gold['degenerate/boxes'])
    assert np.isneginf(v[:3]).all() and np.isnan(v[3:5]).all() and lv['degenerate'].tolist() == [2, 2, 2, 2, 2, 5]
    assert any(1 in hw for hw in u.CASES['thin']['maps']) and (1, 1) in u.CASES['thin']['maps']
    assert u.CASES['pool1']['pool'] == 1
    assert u.CASES['c67']['C'] == 67 and 67 % u.CHANNELS and (u.CASES['big']['R'], u.CASES['big']['C'], u.CASES['big']['pool']) == (1000, 8, 7)


def test_no_stored_box_sits_near_a_level_boundary(gold):
    for name in u.CASES:
        m = u.margin(u.level_values(gold[name + '/boxes']))
        assert (m > u.MARGIN).all(), (name, float(m.min()))
    # what the generator redraws: a box on a boundary
    side = np.float32(0.21875 * 2 ** 0.5)          # level value 4.5
    assert u.margin(u.level_values(np.array([[0, 0, side, side]], np.float32)))[0] < u.MARGIN
    assert np.isinf(u.margin(np.array([np.nan, np.inf, -np.inf]))).all()
    assert u.levels_of([2.5, 3.5, 4.5, 5.5, -7.0, 9.0, np.nan, np.inf, -np.inf]).tolist() == [2, 4, 4, 5, 2, 5, 2, 2, 2]


def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    assert all(name in history[at - 3000:at] for name in NAMES)
    clause = 'still 20: sdn_pyramid_roi_align_grad_floats, sdn_pyramid_roi_align_fwd, sdn_pyramid_roi_align_bwd added'
    assert clause in history
    assert history.index('sdn_mrcnn_loss_bwd added') < history.index(clause) < at
    assert 'model.py:414-502' in history and ':95-100' in history and 'NOT bit-reproducible' in history and 'gives level 2' in history
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernels_are_built_without_fma_contraction_and_share_the_crops_sample():
    csrc = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
    makefile_rules.assert_built_exactly('pyramid_roi_align.hip')
    shared = open(os.path.join(csrc, 'crop_sample.h')).read()
    assert len(re.findall(r'float axis_in\(', shared)) == 1
    for f in ('raster_boxes.hip', 'pyramid_roi_align.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "crop_sample.h"' in text and 'axis_in(' in text and not re.search(r'float axis_in\(', text), f
    text = open(os.path.join(csrc, 'pyramid_roi_align.hip')).read()
    assert '#include "pyramid_roi_align_check.h"' in text and not re.search(r'__(logf|log2f|fsqrt_r[a-z]|fdividef|expf)\b', text)


def test_the_constants_are_mirrored_and_the_layout_comes_from_the_library():
    from sdn_hip import ops
    const = lambda k: host_checks.constexpr_int('pyramid_roi_align_check.h', k)   # noqa: E731
    assert const('PRA_LEVELS') == ops.PYRAMID_LEVELS == u.LEVELS == 4
    assert const('PRA_MAX_POOL') == ops.PYRAMID_MAX_POOL == u.MAX_POOL and const('PRA_CHANNELS') == ops.PYRAMID_CHANNELS == u.CHANNELS
    assert const('PRA_THREADS') % 64 == 0 and const('PRA_MAX_POOL') ** 2 * const('PRA_SAMPLE_BYTES') <= 64 * 1024
    for C, maps in ((5, u.PYRAMID), (67, u.CASES['c67']['maps']), (3, u.CASES['thin']['maps']), (1, ((1, 1),) * 4), (256, ((256, 256), (128, 128), (64, 64), (32, 32)))):
        offsets, total = ops.pyramid_grad_floats(C, [h for h, _ in maps], [w for _, w in maps])
        assert (offsets, total) == u.grad_offsets(C, maps), (C, maps)
        assert all(o % 4 == 0 for o in offsets) and total % 4 == 0
    assert ops.pyramid_grad_floats(5, (24, 12, 6, 3), (20, 10, 5, 3)) == ([0, 2400, 3000, 3152], 3200)   # 45 floats of P5 rounded up to 48


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _ints(v):
    return None if v is None else (ctypes.c_int * 4)(*v)


def _fwd(boxes=FAKE, R=5, maps=(FAKE,) * 4, H=(24, 12, 6, 3), W=(20, 10, 5, 3), C=3, pool=7, area=1048576.0, pooled=FAKE, levels=FAKE):
    import sdn_hip
    L = sdn_hip.lib()
    m = None if maps is None else (ctypes.c_void_p * 4)(*maps)
    rc = L.sdn_pyramid_roi_align_fwd(boxes, R, m, _ints(H), _ints(W), C, pool, area, 0.0, pooled, levels, None)
    return rc, L.sdn_last_error().decode()


def _bwd(grads=FAKE, boxes=FAKE, R=5, H=(24, 12, 6, 3), W=(20, 10, 5, 3), C=3, pool=7, area=1048576.0, gmaps=FAKE, **_unused):
    import sdn_hip
    L = sdn_hip.lib()
    rc = L.sdn_pyramid_roi_align_bwd(grads, boxes, R, _ints(H), _ints(W), C, pool, area, gmaps, None)
    return rc, L.sdn_last_error().decode()


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_the_entry_points_refuse_bad_arguments_before_any_launch(call):
    prefix = 'sdn_pyramid_roi_align_fwd: ' if call is _fwd else 'sdn_pyramid_roi_align_bwd: '
    for kw, reason in ((dict(R=-1), 'bad sizes: R -1'), (dict(C=0), 'bad sizes: C 0'), (dict(C=-3), 'bad sizes: C -3'),
                       (dict(H=(24, 0, 6, 3)), 'bad sizes: level P3 is 0 x 10'), (dict(W=(20, 10, 5, -1)), 'bad sizes: level P5 is 3 x -1'),
                       (dict(H=None), 'H or W is NULL'), (dict(W=None), 'H or W is NULL'),
                       (dict(pool=0), 'pool 0; 1 to 32'), (dict(pool=33), 'pool 33; 1 to 32'), (dict(pool=-7), 'pool -7; 1 to 32'),
                       (dict(area=0.0), 'must be finite and positive'), (dict(area=-4.0), 'must be finite and positive'),
                       (dict(area=float('inf')), 'must be finite and positive'), (dict(area=float('nan')), 'must be finite and positive'),
                       (dict(boxes=None), 'NULL with R > 0'), (dict(boxes=FAKE + 2), 'aligned to 4'),
                       (dict(H=(65536, 12, 6, 3), W=(32768, 10, 5, 3), C=1), 'level P2 must stay below 2^31'),        # exactly 2^31
                       (dict(H=(24, 12, 6, 1024), W=(20, 10, 5, 1024), C=2048), 'level P5 must stay below 2^31'),
                       (dict(H=(0x7fffffff,) * 4, W=(0x7fffffff,) * 4, C=0x7fffffff), 'below 2^31'),                  # the check itself must not overflow
                       (dict(H=(1,) * 4, W=(1,) * 4, C=3000000, pool=32), 'C * pool * pool'),
                       (dict(H=(1,) * 4, W=(1,) * 4, C=2000000, R=0x7fffffff), 'workgroups must stay below 2^31')):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(prefix) and reason in msg, (kw, msg)


def test_the_forward_entry_point_checks_its_buffers_and_r0_launches_nothing():
    for kw, reason in ((dict(pooled=None), 'NULL with R > 0'), (dict(levels=None), 'NULL with R > 0'), (dict(maps=None), 'maps is NULL'),
                       (dict(maps=(FAKE, FAKE, None, FAKE)), 'the map of level P4 is NULL'), (dict(maps=(FAKE, FAKE + 1, FAKE, FAKE)), 'aligned to 4'),
                       (dict(levels=FAKE + 2), 'aligned to 4')):
        rc, msg = _fwd(**kw)
        assert rc == -1 and reason in msg, (kw, msg)
    # R = 0 is valid and touches nothing: no pointer is needed and no GPU either
    assert _fwd(R=0, boxes=None, maps=None, pooled=None, levels=None)[0] == 0


def test_the_backward_entry_point_checks_its_buffers():
    for kw, reason in ((dict(gmaps=None), 'grad_maps is NULL'), (dict(gmaps=FAKE + 4), 'aligned to 16'), (dict(grads=None), 'grads or boxes is NULL'),
                       (dict(R=0, grads=None, boxes=None, gmaps=None), 'grad_maps is NULL')):       # R = 0 still zero-fills
        rc, msg = _bwd(**kw)
        assert rc == -1 and reason in msg, (kw, msg)


def test_the_layout_query_checks_its_arguments():
    import sdn_hip
    L = sdn_hip.lib()
    off, total = (ctypes.c_size_t * 4)(), ctypes.c_size_t()
    H, W = _ints((24, 12, 6, 3)), _ints((20, 10, 5, 3))
    assert L.sdn_pyramid_roi_align_grad_floats(5, H, W, off, ctypes.byref(total)) == 0 and total.value == 3200
    assert L.sdn_pyramid_roi_align_grad_floats(0, H, W, off, ctypes.byref(total)) == -1
    assert L.sdn_pyramid_roi_align_grad_floats(5, None, W, off, ctypes.byref(total)) == -1
    assert L.sdn_pyramid_roi_align_grad_floats(5, H, W, None, ctypes.byref(total)) == -1
    assert L.sdn_pyramid_roi_align_grad_floats(5, H, W, off, None) == -1
    assert 'sdn_pyramid_roi_align_grad_floats: offsets or total is NULL' in L.sdn_last_error().decode()
    assert L.sdn_pyramid_roi_align_grad_floats(5, H, _ints((20, 10, 0, 3)), off, ctypes.byref(total)) == -1


def _cpu_inputs(name='single', batch=True):
    c = u.draw_case(name)
    lift = (lambda t: t[None]) if batch else (lambda t: t)
    return [lift(torch.from_numpy(c['boxes'].copy()))] + [lift(torch.from_numpy(m.copy())) for m in c['maps']], c['pool']


def test_the_wrappers_refuse_what_the_reference_cannot_mean():
    from sdn_hip import ops
    inputs, pool = _cpu_inputs()
    keep = list(inputs)
    for fn in (pyramid.pyramid_roi_align, pyramid.pyramid_levels):
        with pytest.raises(NotImplementedError, match='boxes is on cpu'):
            fn(inputs, pool, u.IMAGE_SHAPE)                 # well-formed, but not on the GPU: there is no torch form
    assert all(a is b for a, b in zip(inputs, keep)) and inputs[0].dim() == 3 and inputs[1].dim() == 4     # `inputs` is not changed
    with pytest.raises(NotImplementedError):
        pyramid.pyramid_roi_align(_cpu_inputs(batch=False)[0], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match=r'boxes has batch 2; only 1 is supported.*model\.py:433'):
        pyramid.pyramid_roi_align([torch.cat([inputs[0], inputs[0]])] + inputs[1:], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match='P4 has batch 3'):
        pyramid.pyramid_roi_align(inputs[:3] + [torch.cat([inputs[3]] * 3)] + inputs[4:], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match=r'got 4 entries \(3 feature maps\)'):
        pyramid.pyramid_roi_align(inputs[:4], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match=r'got 6 entries \(5 feature maps\)'):
        pyramid.pyramid_roi_align(inputs + inputs[-1:], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match='P3 has 3 channels, P2 4'):
        pyramid.pyramid_roi_align(inputs[:2] + [inputs[2][:, :3]] + inputs[3:], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match=r'boxes must be \[1, R, 4\]'):
        pyramid.pyramid_roi_align([inputs[0][:, :, :3]] + inputs[1:], pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match='P5 must have 3 or 4 dimensions'):
        pyramid.pyramid_roi_align(inputs[:4] + [inputs[4][0, 0]], pool, u.IMAGE_SHAPE)
    with pytest.raises(TypeError, match='P2 must be a torch.Tensor'):
        pyramid.pyramid_roi_align([inputs[0], inputs[1].numpy()] + inputs[2:], pool, u.IMAGE_SHAPE)
    boxes, maps = inputs[0][0], [m[0] for m in inputs[1:]]
    with pytest.raises(ValueError, match='3 feature maps; the four levels'):
        ops.pyramid_roi_align(boxes, maps[:3], pool, u.IMAGE_AREA)
    with pytest.raises(NotImplementedError):
        ops.pyramid_roi_align(boxes, maps, pool, u.IMAGE_AREA)


def test_the_public_names_and_the_docstrings():
    assert list(inspect.signature(pyramid.pyramid_roi_align).parameters) == ['inputs', 'pool_size', 'image_shape']   # model.py:414
    from sdn_hip import ops
    assert list(inspect.signature(ops.pyramid_roi_align).parameters) == ['boxes', 'maps', 'pool', 'image_area']
    doc = pyramid.pyramid_roi_align.__doc__
    assert 'model.py:414-502' in doc and 'R = 0' in doc and 'is not changed' in doc
    assert 'not bit-reproducible' in ops.pyramid_roi_align.__doc__ and 'not bit-reproducible' in pyramid.__doc__


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_layout_level_rule_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/pyramid_roi_align_check.cpp: a stand-alone program with its own main that includes only
    csrc/pyramid_roi_align_check.h; host code on the CPU, never loaded into Python"""
    rc, out = host_checks.run_check_program('pyramid_roi_align_check', ['pyramid_roi_align_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out and b'the validators' in out
