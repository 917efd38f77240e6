"""What tests/test_gpu_conv_gemm.py takes for granted, checked without a GPU.  First: under the launch geometry restated in
tests/conv_gemm_util.py every named case reaches the tile family, K order, step and slice counts, channel passes and chunk counts its
row claims (if this fails after a change of a launcher's thresholds, pick new cases).  Second: the launch formula of include/sdn_hip.h,
    out[n, qy os + py, qx os + px, co] = sum_t sum_ci f(in[n, qy is + dy_t, qx is + dx_t, ci]) W_t[co, ci],
evaluated by a plain numpy gather-sum on the very launch arguments the GPU test passes, reproduces torch's float64 convolution for
the hand-built 2- and 3-tap lists, the single-phase launch, the strided and the reflected 7 x 7 case -- the one formula all GPU cases
rely on.  Third, the redraw rule: the float32 CPU evaluation of every sdn_conv_gemm / sdn_conv_wgrad case lies within a quarter of the
gate, so that a GPU miss is the kernel's and not the input's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_gemm_util as u


# ------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize('name', list(u.GEMM_CASES))
def test_gemm_cases_reach_their_named_geometry(name):
    c = u.GEMM_CASES[name]
    assert u.gemm_geometry(c) == c['geo']
    bn, tiles, Kp, steps, ksplit, slices, order, pad = c['geo']
    assert sum(slices) == steps and len(slices) == ksplit and Kp == 32 * steps
    P = u.gemm_problem(name)
    assert P.rows == {32: 32, 64: 64, 128: -(-P.Cop // 128) * 128}[bn] and len(P.taps) <= u.MAX_TAPS
    if name == 'split2':
        assert u.bias_act_stats_passes(c) == (12,)
    if name == 'split4_mid':
        assert slices[0] % (c['kh'] * c['kw']) != 0                 # a slice starts inside a channel block's 16 taps
    if name == 'split3_tapmajor':
        assert P.Cip == 16 and P.QH * P.QW == 128 + 15
    if name == 'split32':
        assert ksplit == 32 and P.w.numel() * 4 < 38e6
    if name == 'split_wide':
        assert u.bias_act_stats_passes(c) == (256, 4) and P.Cop % 128 == 16
    if name == 'nosplit_big':
        assert tiles > 160 and -(-P.QH * P.QW // 128) > u.STAT_SLOTS
    if name in ('gpt3', 'bf16_gpt3'):
        assert P.Cip // 16 == 3 and P.Cop == 160 and P.rows == 256
    if name == 'nosplit_acc_tail':
        assert u.gemm_geometry(dict(c, acc=0))[4] == 2               # only the accumulate keeps it in one slice
    if name == 'phase':
        assert (P.ostride, P.py, P.px, P.QH, P.QW, P.OH, P.OW) == (2, 1, 0, 9, 14, 18, 28) and len(P.taps) == 2
    if name == 's2':
        assert P.istride == 2 and (P.QH, P.QW) == (13, 16)
    if name in ('pad_channels', 'split_pad'):
        assert P.Cop > c['cout']


def test_gemm_cases_cover_the_branches():
    cs = u.GEMM_CASES
    assert {c['geo'][0] for c in cs.values()} == {32, 64, 128}
    assert {c['geo'][3] for c in cs.values()} >= {1, 2, 3, 5}                                     # the pipeline's short paths
    assert {(c['geo'][0], c['geo'][6], c['geo'][4] > 1) for c in cs.values()} >= {(32, 'tapmajor', True), (64, 'cmajor', True),
                                                                                 (64, 'tapmajor', True), (128, 'cmajor', True),
                                                                                 (128, 'tapmajor', False), (32, 'cmajor', False)}
    assert {c['act'] for c in cs.values()} == {0, 1, 2}
    assert {(c['precision'], c['in_relu']) for c in cs.values()} == {(1, 0), (1, 1), (3, 0), (3, 1)}
    assert all(cs[n]['geo'][4] > 1 for n in u.GEMM_SPLIT_CASES) and len(u.GEMM_SPLIT_CASES) >= 8
    split = [cs[n] for n in u.GEMM_SPLIT_CASES]
    assert any(c['acc'] for c in split) and any(c['stats'] and c['bias'] for c in split) and any(c['act'] == 2 for c in split)


@pytest.mark.parametrize('name', list(u.WGRAD_CASES))
def test_wgrad_cases_reach_their_named_geometry(name):
    c = u.WGRAD_CASES[name]
    assert u.wgrad_geometry(c) == c['geo']
    family, row_tiles, col_tiles, steps, slices = c['geo']
    P = u.wgrad_problem(name)
    ncols = len(P.WL.taps) * P.Cc
    if name == 'tiny_images':
        assert c['QH'] * c['QW'] * 8 == 32 and c['QW'] == 2
    if name == 'column':
        assert c['QH'] >= 64 and c['QW'] == 1
    if name == 'tall':
        assert c['QH'] >= 64 and c['QW'] == 3
    if name in ('row32', 'row31'):
        assert (c['QW'] >= 32) == (name == 'row32')
    if name == 'odd_tail':
        assert steps == 1 and c['N'] * c['QH'] * c['QW'] % 2 == 1
    if name == 'rows64':
        assert ncols == 432 and col_tiles * 128 - ncols == 80 and (col_tiles * 8 - 1) // (P.Cc // 16) >= len(P.WL.taps)
    if name == 'rows160':
        assert row_tiles == 2 and P.Cr % 128 == 32
    if name == 'reflect7':
        assert len(P.WL.taps) == 49
    if name == 'splits8_clamped':
        assert slices == (1,) and c['splits'] == 8


def test_wgrad_cases_cover_the_branches():
    cs = u.WGRAD_CASES.values()
    assert {c['geo'][0] for c in cs} == {32, 64, 128}
    assert {(c['relu_rows'], c['relu_gath']) for c in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c['base'] for c in cs} == {0, 1} and {c['precision'] for c in cs} == {1, 3}
    assert {(c['kind'], c['s']) for c in cs} >= {('conv', 2), ('convT', 2)}
    assert sum(len(c['geo'][4]) > 1 for c in cs) == 3
    assert any(c['nr'] % 16 for c in cs) and any(c['nc'] % 16 for c in cs)                        # padding rows and columns exist


@pytest.mark.parametrize('name', list(u.NARROW_CASES))
def test_narrow_cases_reach_their_named_geometry(name):
    c = u.NARROW_CASES[name]
    assert u.narrow_geometry(c) == c['geo']
    P = u.narrow_problem(name)
    assert tuple(u.narrow_reference(name).shape) == (c['N'], c['rows_used'], c['H'], c['W'])
    assert tuple(P.dense.shape) == (c['k'], c['k'], c['cin'], P.RP) and c['geo'][2] * c['geo'][3] >= c['cin']
    assert ((8 + c['k'] - 1) * 40 + 4) * min(c['cin'], c['geo'][2]) * 4 <= 160 * 1024            # the planes of a pass fit in LDS


def test_narrow_cases_cover_every_instance():
    cs = u.NARROW_CASES.values()
    assert {(c['geo'][0], c['k']) for c in cs} == {(r, k) for r in (1, 3, 4, 5, 8) for k in (3, 4, 7)}
    assert {c['rows_used'] for c in cs} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {(c['H'], c['W']) for c in cs} >= {(13, 70), (9, 33), (8, 32), (3, 5)}
    assert {(c['geo'][2], c['geo'][3]) for c in cs} == {(16, 1), (16, 3), (16, 4), (64, 1), (64, 2)}
    assert {c['act'] for c in cs} == {0, 1, 2} and {c['bias'] for c in cs} == {0, 1} and {c['Cop'] for c in cs} == {16, 32}
    assert {c['reflect'] for c in cs} == {0, 1} and {c['in_relu'] for c in cs} == {0, 1}
    assert any(c['geo'][1] >= 256 and c['cin'] == 64 for c in cs)


@pytest.mark.parametrize('name', list(u.SEGMENT_CASES))
def test_segment_cases_reach_their_named_geometry(name):
    c = u.SEGMENT_CASES[name]
    assert u.segment_geometry(c) == c['geo']
    P = u.segment_problem(name)
    r = u.segment_reference(name)
    assert int(P.seg.min()) >= 0 and int(P.seg.max()) < c['K']
    if name == 'k_eq_hw':
        assert bool(r['present'].all()) and c['K'] == c['H'] * c['W']
    else:
        assert not bool(r['present'].all())                          # some ids are absent
    if name == 'groups':
        assert c['geo'][1] > 16 and c['K'] - 64 == 6
    if name == 'images':
        assert c['H'] * c['W'] % 4 and c['H'] * c['W'] % 256
    if name == 'lds_atomics':
        assert c['H'] * c['W'] < c['K'] <= 4096
    assert set(u.SEGMENT_ORDERED) == {n for n, k in u.SEGMENT_CASES.items() if k['geo'][0] == 'ordered' and n != 'k_eq_hw'}


def test_segment_reference_is_the_masked_mean():
    """the index_add reference against the reference model's own wording: per id, the mean over the pixels that carry it"""
    P = u.segment_problem('images')
    r = u.segment_reference('images')
    x = P.x.double()
    for k in (0, 1, 6):
        m = (P.seg == k)[:, None].expand_as(x)
        for ch in range(x.shape[1]):
            sel = m[:, ch]
            mean = x[:, ch][sel].mean()
            assert abs(float(r['means'][ch, k] - mean)) <= 1e-12 * float(x[:, ch][sel].abs().sum())
            assert float((r['out'][:, ch][sel] - r['means'][ch, k]).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ the launch formula
@pytest.mark.parametrize('name', ['steps2', 'steps3', 'phase', 's2', 'reflect7'])
def test_gather_sum_of_the_launch_arguments_is_the_torch_convolution(name):
    P = u.gemm_problem(name)
    got = torch.from_numpy(u.gather_sum(P)).permute(0, 3, 1, 2)
    pre, _ = u.gemm_reference(name)
    owned = torch.zeros(P.OH, P.OW, dtype=torch.bool)
    owned[P.py::P.ostride, P.px::P.ostride] = True
    assert int(owned.sum()) == P.QH * P.QW
    assert bool(torch.isnan(got[:, :, ~owned]).all()) and not bool(torch.isnan(got[:, :, owned]).any())
    err = float((got[:, :, owned] - pre[:, :, owned]).abs().max())
    assert err <= 1e-12 * float(pre.abs().max()), (name, err)


def test_precision_1_reference_uses_round_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20)])      # two ties and one above a tie
    assert torch.equal(x.bfloat16().float(), torch.tensor([1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7)]))
    pre3, pre1 = u.gemm_reference('split2')[0], u.gemm_reference('bf16_split2')[0]
    assert 1e-4 < u.scale_error(pre1, pre3) < 2e-2                                                # bf16 operands, the same inputs


# ------------------------------------------------------------------------------------------ the redraw rule
@pytest.mark.parametrize('name', list(u.GEMM_CASES))
def test_gemm_inputs_are_well_conditioned(name):
    pre64, post64 = u.gemm_reference(name)
    pre32, post32 = u.gemm_reference(name, torch.float32)
    e32 = u.scale_error(post32, post64)
    print('sdn_conv_gemm | %s: e32 %.3e (gate / 4 = %.1e)' % (name, e32, u.GATE / 4))
    assert e32 <= u.GATE / 4, (name, e32)
    c = u.GEMM_CASES[name]
    if c['act'] == 2:   # the tanh must not shrink the output scale under the products' (module docstring of the util)
        assert float(pre64.abs().max()) / float(post64.abs().max()) <= 1.25 and float(pre64.abs().max()) >= 0.3
    if c['stats']:
        r1, r2 = pre64.sum((2, 3)), (pre64 * pre64).sum((2, 3))
        s1, s2 = pre32.double().sum((2, 3)), (pre32.double() ** 2).sum((2, 3))
        assert float((s1 - r1).abs().max()) <= u.GATE / 4 * float(r1.abs().max() + r2.sqrt().max())
        assert float(((s2 - r2).abs() / r2).max()) <= u.GATE / 4


@pytest.mark.parametrize('name', list(u.WGRAD_CASES))
def test_wgrad_inputs_are_well_conditioned(name):
    e32 = u.scale_error(u.wgrad_reference(name, torch.float32), u.wgrad_reference(name))
    print('sdn_conv_wgrad | %s: e32 %.3e (gate / 4 = %.1e)' % (name, e32, u.GATE / 4))
    assert e32 <= u.GATE / 4, (name, e32)


def test_wgrad_reference_layout_is_row_tap_channel():
    """[r][tap][c]: element (r, t, c) is the derivative with respect to w[r, c, ky, kx] of the tap t = ky k + kx, by finite differences
    of the float64 convolution (the layer is linear in w: the difference quotient is exact up to rounding)"""
    name = 's2_conv'
    P = u.wgrad_problem(name)
    c = P.c
    ref = u.wgrad_reference(name)
    for (r, t, ch) in ((0, 0, 0), (5, 7, 3), (c['nr'] - 1, 8, c['nc'] - 1)):
        w = torch.zeros(c['nr'], c['nc'], c['k'], c['k'], dtype=torch.float64)
        w[r, ch, t // c['k'], t % c['k']] = 1.0
        d = float((F.conv2d(P.gath.double(), w, stride=c['s'], padding=c['p']) * P.rows.double()).sum())
        assert abs(d - float(ref[r, t, ch])) <= 1e-10 * float(ref.abs().max())
    assert P.WL.tapidx == list(range(9)) and np.array_equal(np.array(P.WL.taps), [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)])
