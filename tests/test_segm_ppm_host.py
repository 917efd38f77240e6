"""Host side of the pyramid pooling module (semantic.ppm, sdn_hip.ops.segm_ppm_pool / segm_ppm_fill): the fixture
tests/golden/segm_ppm_golden.npz against the float64 restatement of tests/segm_ppm_util.py, the two index rules against torch,
the refusals, and use_device_ppm's install / remove on a CPU module.  No GPU is needed: every refusal happens before the library
is touched, and the C entry points validate on the host."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import host_checks
import makefile_rules
import segm_ppm_util as u


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_drawn_state(gold):
    drawn, kept = u.draw_state(), u.fixture_state(gold)
    assert sorted(drawn) == sorted(kept)
    for k in drawn:
        assert np.array_equal(drawn[k].reshape(-1), kept[k].reshape(-1)), k


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_the_restatement_gives_the_fixtures_float64_results(gold, mode):
    res = u.module_reference(mode, state=u.fixture_state(gold))
    u.check_against_fixture(gold, mode, res)
    conv5, _ = u.draw_module_case(mode)
    assert np.array_equal(res['cat'][:, :u.MOD_FC], conv5.astype(np.float64))


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_torchs_fp32_errors_in_the_fixture_are_reproduced(gold, mode):
    """the yardstick of the training-mode gate: torch's own fp32 CPU run against float64, per quantity"""
    want = u.module_reference(mode)
    got = u.module_reference(mode, dtype=torch.float32)
    for q in u.MOD_QUANTITIES:
        kept = float(gold['err32/%s/%s' % (mode, q)])
        now = u.rel(got[q], want[q])
        print('%s %s: torch fp32 rel 2-norm %.3g (fixture %.3g)' % (mode, q, now, kept))
        assert 0 < kept < 1e-5 and now < 1e-5


def test_the_fixture_is_small():
    import os
    assert os.path.getsize(u.GOLD) < 300 * 1024


# ---- the index rules ----------------------------------------------------------------------------------------------------------------
def test_ppm_bins_are_torchs_adaptive_bins():
    from semantic import ppm
    for n in range(1, 21):
        x = torch.arange(1, n + 1, dtype=torch.float64).reshape(1, 1, n, 1)
        ones = torch.eye(n, dtype=torch.float64).reshape(n, 1, n, 1)          # item y: an indicator of row y
        for s in range(1, 9):
            bins = ppm.ppm_bins(n, s)
            assert len(bins) == s and bins[0][0] == 0 and bins[-1][1] == n and all(a < b for a, b in bins)
            pooled = F.adaptive_avg_pool2d(ones, (s, 1)).reshape(n, s)            # [y, i]: 1 / area where bin i holds row y
            for i, (a, b) in enumerate(bins):
                want = np.zeros(n)
                want[a:b] = 1.0 / (b - a)
                assert np.allclose(pooled[:, i].numpy(), want, rtol=0, atol=1e-15), (n, s, i)
            means = F.adaptive_avg_pool2d(x, (s, 1)).reshape(s).numpy()
            assert np.allclose(means, [(a + 1 + b) / 2.0 for a, b in bins], rtol=1e-14), (n, s)
    with pytest.raises(ValueError):
        ppm.ppm_bins(0, 3)


def test_ppm_lerp_is_torchs_bilinear_rule():
    from semantic import ppm
    for n in range(1, 21):
        for s in range(1, 9):
            i0, i1, lam = ppm.ppm_lerp(n, s)
            assert i0.dtype == np.int32 and i1.dtype == np.int32 and lam.dtype == np.float32 and len(i0) == len(i1) == len(lam) == n
            assert (i0 >= 0).all() and (i1 <= s - 1).all() and ((i1 == i0) | (i1 == i0 + 1)).all() and (lam >= 0).all() and (lam < 1).all()
            # the interpolation matrix torch applies in fp32, column by column
            eye = torch.eye(s, dtype=torch.float32).reshape(s, 1, s, 1)
            up = F.interpolate(eye, size=(n, 1), mode='bilinear', align_corners=False).reshape(s, n).numpy()   # [tap, o]
            mine = np.zeros((s, n), dtype=np.float32)
            for o in range(n):
                mine[i0[o], o] += np.float32(1) - lam[o]
                mine[i1[o], o] += lam[o]
            # the source position is below 8, where an ulp is 2^-21: torch's CPU kernel may round scale * (o + 0.5) - 0.5 once
            # (a fused multiply-add) where the rule rounds twice, and 1 - lambda rounds once more; a wrong tap would show as ~1
            assert np.abs(up - mine).max() <= 2.0 ** -21 + 2.0 ** -23, (n, s, np.abs(up - mine).max())
            if n == s:
                assert np.array_equal(i0, np.arange(n)) and not lam.any()
    with pytest.raises(ValueError):
        ppm.ppm_lerp(4, 0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_pool_refuses_before_the_library_is_touched(monkeypatch):
    import sdn_hip
    from sdn_hip import ops
    from semantic import ppm
    monkeypatch.setattr(ops, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was touched')))
    x = torch.zeros(2, 8, 7, 13)
    with pytest.raises(NotImplementedError):
        ppm.ppm_pool(x, (1, 2, 3, 6), (4, 4, 4, 4))
    with pytest.raises(TypeError):
        ppm.ppm_pool(x.double(), (1, 2, 3, 6), (4, 4, 4, 4))
    with pytest.raises(TypeError):
        ppm.ppm_pool(x.half(), (1, 2, 3, 6), (4, 4, 4, 4))
    with pytest.raises(TypeError):
        ppm.ppm_pool(x.numpy(), (1, 2, 3, 6), (4, 4, 4, 4))
    with pytest.raises(ValueError):
        ppm.ppm_pool(x[0], (1, 2, 3, 6), (4, 4, 4, 4))                  # three axes
    with pytest.raises(ValueError):
        ppm.ppm_pool(x[:, :, :0], (1, 2, 3, 6), (4, 4, 4, 4))           # an empty axis
    for scales, K in (((), ()), ((1, 2, 3, 6, 7), (4,) * 5), ((1, 2, 3), (4, 4)), ((1, 2, 3, 9), (4,) * 4), ((0, 2), (4, 4)),
                      ((1, 2), (4, 0))):
        with pytest.raises(ValueError):
            ppm.ppm_pool(x, scales, K)
    with pytest.raises(ValueError, match='2\\^31'):
        ppm.ppm_pool(torch.zeros(1, 1, 1, 1).expand(4, 2048, 512, 512), (1,), (1,))
    assert sdn_hip is not None


def test_fill_refuses_before_the_library_is_touched(monkeypatch):
    from sdn_hip import ops
    from semantic import ppm
    monkeypatch.setattr(ops, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was touched')))
    cat = torch.zeros(2, 8 + 16, 7, 13)
    ys = [torch.zeros(2, 4, s, s) for s in (1, 2, 3, 6)]
    with pytest.raises(NotImplementedError):
        ppm.ppm_fill(cat, 8, ys)
    with pytest.raises(NotImplementedError):
        ppm.ppm_fill(cat, 8, *ys)                                         # the branch outputs as arguments
    with pytest.raises(TypeError):
        ppm.ppm_fill(cat.double(), 8, ys)
    with pytest.raises(TypeError):
        ppm.ppm_fill(cat, 8, ys[:3] + [ys[3].double()])
    with pytest.raises(TypeError):
        ppm.ppm_fill(cat, 8, ys[:3] + [None])
    with pytest.raises(ValueError):
        ppm.ppm_fill(cat, 9, ys)                                          # the channels do not add up
    with pytest.raises(ValueError):
        ppm.ppm_fill(cat, 8, ys[:3])
    with pytest.raises(ValueError):
        ppm.ppm_fill(cat, 8, [])
    with pytest.raises(ValueError):
        ppm.ppm_fill(cat, 8, ys[:3] + [torch.zeros(2, 4, 6, 5)])          # not square
    with pytest.raises(ValueError):
        ppm.ppm_fill(cat, 8, ys[:3] + [torch.zeros(3, 4, 6, 6)])          # another batch
    with pytest.raises(ValueError):
        ppm.ppm_fill(cat[:, :, 0], 8, ys)


def test_the_c_entry_points_validate_on_the_host():
    import sdn_hip
    L = sdn_hip.lib()
    fake = ctypes.c_void_p(4096)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    sc, K = ints(1, 2, 3, 6), ints(4, 4, 4, 4)
    assert L.sdn_segm_ppm_pool(None, 2, 8, 7, 13, sc, K, 4, fake, fake, None) == -1 and b'conv5 is NULL' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool(fake, 2, 8, 7, 13, sc, K, 5, fake, fake, None) == -1 and b'5 scales' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool(fake, 2, 8, 7, 13, ints(1, 2, 3, 9), K, 4, fake, fake, None) == -1 and b'scale 3 is 9' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool(fake, 4, 2048, 512, 512, sc, K, 4, fake, fake, None) == -1 and b'below 2^31' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool(fake, 2, 8, 7, 13, sc, K, 4, ctypes.c_void_p(4098), fake, None) == -1 and b'aligned to 4' in L.sdn_last_error()
    assert L.sdn_segm_ppm_fill(ptrs(4096, None, 4096, 4096), 2, 8, 7, 13, sc, K, 4, fake, None) == -1 and b'y[1] is NULL' in L.sdn_last_error()
    assert L.sdn_segm_ppm_fill(ptrs(4096, 4096, 4096, 4096), 2, 8, 7, 13, sc, ints(4, 0, 4, 4), 4, fake, None) == -1
    assert b'branch 1 has 0' in L.sdn_last_error()
    assert L.sdn_segm_ppm_fill_bwd(fake, 2, 8, 7, 13, sc, K, 4, ptrs(None, None, None, None), None) == -1 and b'no gradient' in L.sdn_last_error()
    assert L.sdn_segm_ppm_fill_bwd(None, 2, 8, 7, 13, sc, K, 4, ptrs(4096, None, None, None), None) == -1 and b'grad_cat is NULL' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool_bwd(None, ptrs(None, None, None, None), 2, 8, 7, 13, sc, K, 4, fake, None) == -1 and b'neither' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool_bwd(None, None, 2, 8, 7, 13, sc, K, 4, fake, None) == -1 and b'neither' in L.sdn_last_error()
    assert L.sdn_segm_ppm_pool_bwd(fake, None, 2, 8, 7, 13, sc, K, 4, None, None) == -1 and b'grad_conv5 is NULL' in L.sdn_last_error()


def test_header_binding_and_library_hold_the_ppm_entry_points(monkeypatch):
    names = ('sdn_segm_ppm_pool', 'sdn_segm_ppm_fill', 'sdn_segm_ppm_fill_bwd', 'sdn_segm_ppm_pool_bwd')
    history = host_checks.entry_points(names)
    assert all(name in history[history.index('#define SDN_ABI_VERSION') - 3000:history.index('#define SDN_ABI_VERSION')] for name in names)
    assert 'models.py:336-346, 387-397' in history
    # the family came without a revision bump: a library that lacks one of its entry points is refused by name when it is bound
    host_checks.stale_library_is_refused(names)


def test_the_kernels_are_built_without_fma_contraction():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    makefile_rules.assert_built_exactly('segm_ppm.hip')


# ---- use_device_ppm on a CPU module ------------------------------------------------------------------------------------------------
def test_use_device_ppm_installs_and_removes_an_instance_forward():
    from semantic import ppm
    dec = u.Decoder(branch=4, deepsup=True)
    keys = list(dec.state_dict())
    cls_forward = type(dec).forward
    handle = ppm.use_device_ppm(dec)
    assert 'forward' in dec.__dict__ and dec.forward.__func__ is not cls_forward
    assert list(dec.state_dict()) == keys and 'forward' not in dict(dec.named_modules())
    with pytest.raises(ValueError, match='already'):
        ppm.use_device_ppm(dec)
    with pytest.raises(NotImplementedError):                   # the patched forward is the device's: a CPU tensor is refused
        dec([torch.zeros(2, 8, 14, 26), torch.zeros(2, 16, 7, 13)])
    handle.remove()
    handle.remove()                                            # twice is harmless
    assert 'forward' not in dec.__dict__ and dec.forward.__func__ is cls_forward
    out = dec.eval()([torch.zeros(1, 8, 14, 26), torch.zeros(1, 16, 7, 13)])
    assert isinstance(out, tuple) and out[0].shape == (1, u.MOD_CLASSES, 7, 13)
    with ppm.use_device_ppm(dec) as h:
        assert 'forward' in dec.__dict__ and h.decoder is dec
    assert 'forward' not in dec.__dict__


def test_use_device_ppm_reads_the_sizes_and_refuses_other_modules():
    from semantic import ppm
    assert [(s, k) for s, k, _ in ppm._branches(u.Decoder(branch=4))] == [(1, 4), (2, 4), (3, 4), (6, 4)]
    assert [(s, k) for s, k, _ in ppm._branches(u.Decoder(branch=3, pair_sizes=True, pool_scales=(2, 8)))] == [(2, 3), (8, 3)]
    with pytest.raises(ValueError, match='no ppm / conv_last'):
        ppm.use_device_ppm(nn.Sequential(nn.Conv2d(3, 3, 1)))          # a C1 decoder has neither
    with pytest.raises(TypeError):
        ppm.use_device_ppm(object())
    dec = u.Decoder(branch=4)
    dec.ppm[1][0] = nn.AdaptiveAvgPool2d((2, 3))
    with pytest.raises(ValueError, match='square'):
        ppm.use_device_ppm(dec)
    dec.ppm[1][0] = nn.AdaptiveAvgPool2d((None, 2))
    with pytest.raises(ValueError):
        ppm.use_device_ppm(dec)
    dec.ppm[1][0] = nn.AdaptiveAvgPool2d(9)
    with pytest.raises(ValueError, match='1 to 8'):
        ppm.use_device_ppm(dec)
    dec.ppm[1][0] = nn.AvgPool2d(2)
    with pytest.raises(ValueError, match='AdaptiveAvgPool2d'):
        ppm.use_device_ppm(dec)
    dec = u.Decoder(branch=4, pool_scales=(1, 2, 3, 4, 6))
    with pytest.raises(ValueError, match='5 branches'):
        ppm.use_device_ppm(dec)
    dec = u.Decoder(branch=4)
    dec.ppm[0] = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.ReLU())
    with pytest.raises(ValueError, match='no Conv2d'):
        ppm.use_device_ppm(dec)
    dec = u.Decoder(branch=4)
    del dec.use_softmax
    with pytest.raises(ValueError, match='use_softmax'):
        ppm.use_device_ppm(dec)
    assert 'forward' not in dec.__dict__
