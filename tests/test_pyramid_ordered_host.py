"""The ordered pyramid RoIAlign backward without a GPU (sdn_pyramid_roi_align_bwd_ordered, csrc/pyramid_roi_align.hip): that the numpy
restatement of its contract (tests/pyramid_ordered_util.py) does not depend on the order of the additions on any case the GPU test
uses -- which is what lets that test demand equal bits while the kernel chooses its order --, that it lies within the fixture's gate
of the fixture's float64 gradients, the new names in header, binding and library, the argument checks of the two entry points (they
run before any launch), the switch behind ops.pyramid_backward_path(), and the check header's new validator under ASan and UBSan in a
stand-alone host program."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import host_checks
import pyramid_ordered_util as o
import pyramid_roi_align_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_pyramid_roi_align_bwd_ordered_workspace_bytes', 'sdn_pyramid_roi_align_bwd_ordered')
RECORD_BYTES = 32         # csrc/pyramid_roi_align_check.h: PRA_RECORD_BYTES


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.mark.parametrize('name', o.ALL_CASES)
def test_the_restatement_does_not_depend_on_the_order_of_the_additions(name):
    """the same float32 terms added forward, reversed, in a seeded permutation and in np.longdouble: not one element differs"""
    c = o.make_case(name)
    terms = o.level_terms(c)
    want = o.ordered_backward(name)
    rs = np.random.RandomState(4242)
    others = dict(reversed=o.accumulate(c, terms, lambda n: np.arange(n)[::-1]),
                  permuted=o.accumulate(c, terms, lambda n: rs.permutation(n)),
                  longdouble=o.accumulate(c, terms, None, np.longdouble))
    for how, got in others.items():
        for l in range(u.LEVELS):
            assert got[l].dtype == np.float32 and got[l].shape == c['maps'][l].shape
            nan_a, nan_b = np.isnan(want[l]), np.isnan(got[l])
            # a NaN has no value to compare: where one run has it, every run has it; everything else bit for bit
            assert np.array_equal(nan_a, nan_b), (name, how, l)
            differing = int((o.bits(want[l])[~nan_a] != o.bits(got[l])[~nan_a]).sum())
            assert differing == 0, (name, how, l, differing)


def test_the_new_cases_reach_what_they_are_there_for():
    assert np.longdouble(1) + np.longdouble(2.0 ** -60) != np.longdouble(1), 'np.longdouble is no wider than float64 here'
    c = o.make_case('tiles')
    assert (c['R'], c['C'], c['pool']) == (60, 3, 7) and all(h % o.TILE and w % o.TILE for _, h, w in (m.shape for m in c['maps']))
    assert set(u.levels(c).tolist()) == {2, 3, 4, 5}
    c = o.make_case('chunks')
    assert c['C'] == 130 and c['C'] % u.CHANNELS == 2 and c['maps'][0].shape == (130, 128, 120) and c['R'] == 40
    c = o.make_case('special')
    assert c['pool'] == 14 and o.make_case('special_pool1')['pool'] == 1 and c['maps'][0].shape == (5, 80, 70)
    assert np.isnan(c['boxes']).any() and np.isinf(c['boxes']).any() and (c['boxes'][0, 0] > c['boxes'][0, 2])
    assert np.array_equal(c['boxes'][:7], o.make_case('special_pool1')['boxes'][:7], equal_nan=True)      # the seven hand-made boxes
    c = o.make_case('long')
    # more boxes of one level meet one tile than one batch of the kernel's list holds: P5's 3 x 3 map is a single tile
    lv = u.levels(c)
    assert c['R'] == 2500 and (lv == 5).sum() > o.LIST_BATCH and c['maps'][3].shape[1:] == (3, 3)
    assert o.make_case('pool32')['pool'] == u.MAX_POOL == 32
    c = o.make_case('nonfinite')
    assert np.isinf(c['grads']).sum() == 1 and np.isnan(c['grads']).sum() == 1 and np.array_equal(c['boxes'], u.draw_case('mixed7')['boxes'])
    got = o.ordered_backward('nonfinite')
    assert any(np.isinf(g).any() for g in got) and any(np.isnan(g).any() for g in got)
    c = o.make_case('zero_inf')
    got = o.ordered_backward('zero_inf')
    # 0 * inf: the infinite gradient of a sample ON pixel (0, 0) gives NaN there, as in the reference's C, and inf - inf at (2, 2)
    assert np.isnan(got[3][0, 0, 0]) and np.isnan(got[3][1, 2, 2]) and np.isnan(got[2][0, 0, :2]).all()
    for name in o.NEW_CASES:
        c = o.make_case(name)
        assert c['boxes'].dtype == c['grads'].dtype == np.float32 and c['grads'].shape == (c['R'], c['C'], c['pool'], c['pool'])
        finite = np.isfinite(c['boxes']).all(1)
        assert (u.margin(u.level_values(c['boxes'][finite])) > u.MARGIN).all(), name      # no box near a level boundary


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_is_within_the_fixtures_gate_of_its_float64_gradients(gold, name):
    """u.backward forms the terms in float64, the contract in float32 as the reference's C does: that is the whole distance"""
    got = o.ordered_backward(name)
    want = [gold[name + '/grad64_%d' % l] for l in range(u.LEVELS)]
    err, gate = u.grad_error(got, want), gold[name + '/gate']
    print('%s: %s of the largest float64 magnitude per level, gate %s' % (name, err, gate))
    assert (err <= gate).all(), (err, gate)
    for l in range(u.LEVELS):
        assert not got[l][want[l] == 0].any() and not np.signbit(got[l][want[l] == 0]).any()


def test_header_binding_and_library_hold_the_new_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    clause = 'still 20: sdn_pyramid_roi_align_bwd_ordered_workspace_bytes, sdn_pyramid_roi_align_bwd_ordered added'
    assert clause in history and history.index('sdn_rpn_outputs_bwd added') < history.index(clause) < at
    assert 'NOT bit-reproducible' in history and 'ORDERED backward' in history and 'crop_and_resize.c:241-247' in history
    host_checks.stale_library_is_refused(NAMES)        # added without a revision bump: a library built before them is stale
    text = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'pyramid_roi_align.hip')).read()
    body = text[text.index('void k_pra_box_records'):text.index('static PraParams pra_params')]
    assert 'tomicAdd' not in body and 'hipMemset' not in text        # no atomics in the ordered kernels, no memset anywhere


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _ints(v):
    return None if v is None else (ctypes.c_int * 4)(*v)


def _ordered(grads=FAKE, boxes=FAKE, R=5, H=(24, 12, 6, 3), W=(20, 10, 5, 3), C=3, pool=7, area=1048576.0, gmaps=FAKE, ws=FAKE, ws_bytes=None):
    import sdn_hip
    L = sdn_hip.lib()
    if ws_bytes is None:
        ws_bytes = max(R, 0) * RECORD_BYTES
    rc = L.sdn_pyramid_roi_align_bwd_ordered(grads, boxes, R, _ints(H), _ints(W), C, pool, area, gmaps, ws, ws_bytes, None)
    return rc, L.sdn_last_error().decode()


def test_the_ordered_entry_point_refuses_bad_arguments_before_any_launch():
    prefix = 'sdn_pyramid_roi_align_bwd_ordered: '
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
                       (dict(H=(1,) * 4, W=(1,) * 4, C=2000000, R=0x7fffffff), 'workgroups must stay below 2^31'),
                       # the buffers, as sdn_pyramid_roi_align_bwd
                       (dict(gmaps=None), 'grad_maps is NULL'), (dict(gmaps=FAKE + 4), 'aligned to 16'), (dict(grads=None), 'grads or boxes is NULL'),
                       (dict(grads=FAKE + 1), 'aligned to 4'), (dict(R=0, grads=None, boxes=None, gmaps=None, ws=None), 'grad_maps is NULL'),
                       # the workspace
                       (dict(ws=None), 'workspace is NULL with R > 0'), (dict(ws=FAKE + 8), 'workspace must be aligned to 16'),
                       (dict(ws=FAKE + 4), 'workspace must be aligned to 16'),
                       (dict(ws_bytes=5 * RECORD_BYTES - 1), 'workspace of 159 bytes; 160 are needed for 5 boxes'), (dict(ws_bytes=0), 'workspace of 0 bytes')):
        rc, msg = _ordered(**kw)
        assert rc == -1 and msg.startswith(prefix) and reason in msg, (kw, msg)


def test_the_workspace_query_answers_and_refuses():
    import sdn_hip
    from sdn_hip import ops
    L = sdn_hip.lib()
    n = ctypes.c_size_t(12345)
    for R in (0, 1, 5, 1000, 0x7fffffff):
        assert L.sdn_pyramid_roi_align_bwd_ordered_workspace_bytes(R, ctypes.byref(n)) == 0 and n.value == R * RECORD_BYTES
        assert n.value % 16 == 0 and n.value <= 48 * R                          # whole 16-byte pieces, a few dozen bytes per box
    assert ops.pyramid_ordered_workspace_bytes(0) == 0 and ops.pyramid_ordered_workspace_bytes(200) == 200 * RECORD_BYTES      # R = 0 needs no workspace
    assert L.sdn_pyramid_roi_align_bwd_ordered_workspace_bytes(-1, ctypes.byref(n)) == -1
    assert 'sdn_pyramid_roi_align_bwd_ordered_workspace_bytes: bad sizes: R -1' in L.sdn_last_error().decode()
    assert L.sdn_pyramid_roi_align_bwd_ordered_workspace_bytes(5, None) == -1
    assert 'sdn_pyramid_roi_align_bwd_ordered_workspace_bytes: bytes is NULL' in L.sdn_last_error().decode()
    const = lambda k: host_checks.constexpr_int('pyramid_roi_align_check.h', k)   # noqa: E731
    assert const('PRA_RECORD_BYTES') == RECORD_BYTES and const('PRA_TILE') == o.TILE and const('PRA_THREADS') == o.LIST_BATCH


def test_the_backward_path_follows_the_switches(monkeypatch):
    import sdn_hip
    from sdn_hip import conv, ops
    assert list(inspect.signature(ops.pyramid_roi_align).parameters) == ['boxes', 'maps', 'pool', 'image_area']
    assert list(inspect.signature(ops.pyramid_backward_path).parameters) == []
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        monkeypatch.delenv('SDN_DETERMINISTIC', raising=False)
        assert ops.pyramid_backward_path() == 'atomic' and not sdn_hip.deterministic() and not conv.deterministic()
        monkeypatch.setenv('SDN_DETERMINISTIC', '1')
        assert ops.pyramid_backward_path() == 'ordered' and sdn_hip.deterministic() and conv.deterministic()
        for off in ('0', '', 'true'):
            monkeypatch.setenv('SDN_DETERMINISTIC', off)      # '1' alone turns it on, as for the conv stack
            assert ops.pyramid_backward_path() == 'atomic' and not conv.deterministic()
        monkeypatch.delenv('SDN_DETERMINISTIC')
        torch.use_deterministic_algorithms(True)
        assert ops.pyramid_backward_path() == 'ordered' and sdn_hip.deterministic() and conv.deterministic()
        torch.use_deterministic_algorithms(False)
        assert ops.pyramid_backward_path() == 'atomic'
    finally:
        torch.use_deterministic_algorithms(before)
    # one rule: conv's name is the package's function, and ops.py does not import conv.py for it
    text = open(os.path.join(ROOT, '3d-sdn_amd', 'sdn_hip', 'ops.py')).read()
    assert not re.search(r'^\s*(from \. import conv|from \.conv import|import sdn_hip\.conv)', text, re.M)
    assert 'SDN_DETERMINISTIC' in ops.pyramid_roi_align.__doc__ and 'not bit-reproducible' in ops.pyramid_roi_align.__doc__


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_ordered_validator_and_workspace_size_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/pyramid_roi_align_ordered_check.cpp: a stand-alone program with its own main that includes only
    csrc/pyramid_roi_align_check.h; host code on the CPU in its own process, never loaded into Python, nothing preloaded"""
    rc, out = host_checks.run_check_program('pyramid_roi_align_ordered_check', ['pyramid_roi_align_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out and b'the ordered validator' in out
