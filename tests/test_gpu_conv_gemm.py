"""The r01-r03 conv kernels and the instance pooling at operator level, through the C ABI: sdn_conv_gemm (csrc/conv_gemm.hip),
sdn_conv_wgrad (csrc/conv_wgrad.hip), sdn_conv_narrow_fwd (csrc/conv_narrow.hip) and sdn_segment_mean (csrc/fast_segment.hip) against
torch's float64 operators on the CPU.  These kernels still run every layer their successors refuse (stride 2, transposed
convolutions, 128 channels or fewer, the 48 -> 64 stem, every deterministic-mode launch, the whole ResNet-18 encoder) and were
only reached through whole networks so far.  Cases, inputs, references and gates live in tests/conv_gemm_util.py;
tests/test_conv_gemm_host.py shows on the CPU that every named case reaches the branch its name claims, that the launch formula
evaluated on these very launch arguments is torch's convolution, and that every input is well conditioned.

Setup as tests/test_gpu_conv_phases.py / test_gpu_conv_tile.py: weights packed by the library's own sdn_conv_pack_weights, tap lists
from sdn_hip.convplan, cpad / kpad / weight_rows.

Gates, and the worst value measured over all cases on an MI355X:
  sdn_conv_gemm        output, max |got - ref| / max |ref|      6.1e-6 (steps3)             gate 1e-5
                       statistics: sums / sums of squares       2.8e-6 / 4.8e-6             gates 1e-5 (as test_gpu_conv_tile.py)
                       precision 1 against the bf16 operands    2.1e-7                      gate 1e-5
                       deterministic mode                       bit-identical over two calls, every split case
  sdn_conv_wgrad       dw, of the gradient's scale              8.4e-6 (splits8_clamped)    gate 1e-5
                       precision 1                              2.6e-7                      gate 1e-5
  sdn_conv_narrow_fwd  relative L2                              6.5e-7 (e32 4.6e-7)         gate max(2e-6, 4 e32)
  sdn_segment_mean     relative L2: out / means / gradient      1.4e-7 / 1.4e-7 / 1.3e-7    gate max(1e-6, 4 e32)
The first draw of split3_tapmajor (a tanh case with max |pre| 3.6) measured 1.078e-5 in both split modes: the tanh shrinks the
output scale under the products'; tests/conv_gemm_util.py says how tanh cases are drawn and the host test asserts it.
"""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_gemm_util as u  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_i8 = ctypes.c_int8
NAN = float('nan')


def _i8s(vals):
    return (_i8 * len(vals))(*vals)


def _nchw(t, c):
    """channels-last device tensor -> the first c channels as NCHW float64 on the CPU"""
    return t[..., :c].permute(0, 3, 1, 2).double().cpu()


# ------------------------------------------------------------------------------------------ sdn_conv_gemm
_GEMM_DEVICE = {}


def _gemm_device(name):
    """device copies of the case's inputs and its packed weights (kept: the deterministic test uses the same)"""
    from sdn_hip import check, lib, ptr, stream
    key = name.replace('bf16_', '')
    if key not in _GEMM_DEVICE:
        _GEMM_DEVICE.clear()                                # one case at a time: split32 alone holds 110 MB
        P = u.gemm_problem(name)
        xg = u.channels_last(P.x, P.Cip).to(DEV)
        wg = P.w.to(DEV)
        tix = torch.tensor(list(P.tapidx), dtype=torch.int32, device=DEV)
        packed = torch.empty(2 * P.rows * P.Kp, dtype=torch.bfloat16, device=DEV)
        check(lib().sdn_conv_pack_weights(ptr(wg), P.R, P.C, P.sr, P.sc, ptr(tix), len(P.taps), P.Cip, P.Kp, P.rows, ptr(packed), stream()))
        bg = None
        if P.bias is not None:
            bg = torch.zeros(P.Cop, device=DEV)
            bg[:P.R] = P.bias.to(DEV)
        base = None if P.base is None else P.base.to(DEV)
        torch.cuda.synchronize()
        _GEMM_DEVICE[key] = (xg, packed, bg, base)
    return _GEMM_DEVICE[key]


def _gemm_call(name, workspace=None, workspace_bytes=None, **over):
    """one sdn_conv_gemm call of the case; returns (out [N, OH, OW, Cop] pre-filled with the base or a NaN sentinel, stats or None)"""
    from sdn_hip import check, lib, ptr, stream
    P = u.gemm_problem(name)
    c = P.c
    xg, packed, bg, base = _gemm_device(name)
    out = base.clone() if base is not None else torch.full((c['N'], P.OH, P.OW, P.Cop), NAN, device=DEV)
    st = torch.zeros(c['N'], u.STAT_SLOTS, P.Cop, 2, dtype=torch.float64, device=DEV) if c['stats'] else None
    a = dict(Cip=P.Cip, Cop=P.Cop, QH=P.QH, QW=P.QW, ntaps=len(P.taps), Kp=P.Kp, rows=P.rows, precision=c['precision'])
    a.update(over)
    wb = 0 if workspace is None else (workspace.numel() if workspace_bytes is None else workspace_bytes)
    check(lib().sdn_conv_gemm(ptr(xg), c['N'], c['IH'], c['IW'], a['Cip'], ptr(out), P.OH, P.OW, a['Cop'], a['QH'], a['QW'], P.istride,
                              P.ostride, P.py, P.px, a['ntaps'], _i8s([t[0] for t in P.taps] + [0] * 8), _i8s([t[1] for t in P.taps] + [0] * 8),
                              c['reflect'], c['in_relu'], ptr(packed), a['Kp'], a['rows'], ptr(bg), c['act'], ptr(st), c['acc'],
                              a['precision'], ptr(workspace), wb, stream()))
    torch.cuda.synchronize()
    return out, st


def _gemm_workspace(name):
    from sdn_hip import check, lib
    P = u.gemm_problem(name)
    n = ctypes.c_size_t(0)
    check(lib().sdn_conv_gemm_workspace_bytes(P.c['N'], P.OH, P.OW, P.Cop, ctypes.byref(n)))
    return torch.empty(n.value, dtype=torch.uint8, device=DEV)


def _gemm_check(name, mode, out, st):
    P = u.gemm_problem(name)
    c = P.c
    pre, post = u.gemm_reference(name)
    got = _nchw(out, c['cout'])
    want = post if P.base is None else post + _nchw(P.base, c['cout'])
    if c['kind'] == 'phase':
        owned = torch.zeros(P.OH, P.OW, dtype=torch.bool)
        owned[P.py::P.ostride, P.px::P.ostride] = True
        sentinel = torch.full_like(out, NAN).cpu()
        assert u.same_bits(out.cpu()[:, ~owned], sentinel[:, ~owned]), (name, 'positions of the other phases were written')
        got, want = got[:, :, owned], want[:, :, owned]
    assert bool(torch.isfinite(got).all()), (name, mode, 'not finite')
    err = u.scale_error(got, want)
    print('sdn_conv_gemm | %s | %s: gate %.1e measured %.3e' % (name, mode, u.GATE, err))
    assert err <= u.GATE, (name, mode, err)
    if P.Cop > c['cout'] and P.base is None:
        assert float(out[..., c['cout']:].abs().max()) == 0.0, (name, mode, 'padding channels must come out as zeros')
    if st is not None:
        tot = st.sum(1).cpu()
        s1, s2 = tot[:, :c['cout'], 0], tot[:, :c['cout'], 1]
        r1, r2 = pre.sum((2, 3)), (pre * pre).sum((2, 3))
        e1 = float((s1 - r1).abs().max()) / float(r1.abs().max() + r2.sqrt().max())
        e2 = float(((s2 - r2).abs() / r2).max())
        print('sdn_conv_gemm | %s | %s: statistics, sums %.3e sums of squares %.3e (gates %.1e)' % (name, mode, e1, e2, u.GATE))
        assert e1 <= u.GATE and e2 <= u.GATE, (name, mode, e1, e2)
        if P.Cop > c['cout']:
            assert float(tot[:, c['cout']:].abs().max()) == 0.0, (name, mode, 'statistics of the padding channels')
        if name == 'nosplit_big':
            assert bool((st[:, :, :c['cout'], 1] > 0).all()), 'every statistics slot receives tiles'


@pytest.mark.parametrize('name', list(u.GEMM_CASES))
def test_conv_gemm_matches_float64(name):
    """every case with workspace NULL: split cases meet in `out` through float atomics (held to the gate, not to bit equality)"""
    out, st = _gemm_call(name)
    _gemm_check(name, 'atomics' if name in u.GEMM_SPLIT_CASES else 'one slice', out, st)


@pytest.mark.parametrize('name', u.GEMM_SPLIT_CASES)
def test_conv_gemm_deterministic_mode_is_repeatable(name):
    """with a workspace the slices are stored and added in slice order: within the gate and bit-identical over two calls (with
    accumulate: from the same base)"""
    ws = _gemm_workspace(name)
    out_a, st_a = _gemm_call(name, ws)
    _gemm_check(name, 'workspace', out_a, st_a)
    ws.fill_(0xff)                                          # NaN patterns: nothing of the first call is reused
    out_b, st_b = _gemm_call(name, ws)
    assert u.same_bits(out_a, out_b), (name, 'the deterministic mode gave different bits in %d elements' % int((out_a != out_b).sum()))


def test_conv_gemm_refusals():
    """every refusal leaves the library usable: a valid call still succeeds afterwards"""
    from sdn_hip import SdnHipError
    name = 'split2'
    P = u.gemm_problem(name)
    _gemm_call(name)
    bad = [dict(Cip=P.Cip - 8), dict(Cop=P.Cop + 8),        # channel counts not padded to 16
           dict(Kp=P.Kp + 16),                              # Kp no multiple of 32
           dict(Kp=P.Kp - 32),                              # Kp smaller than taps x Cip
           dict(precision=2),
           dict(QH=P.QH + 1), dict(QW=P.QW + 1),            # the grid leaves the output tensor
           dict(rows=32),                                   # w_rows below the 64-wide family's
           dict(ntaps=65)]
    for over in bad:
        with pytest.raises(SdnHipError):
            _gemm_call(name, **over)
    for wide, rows in (('split_wide', 1024), ('split3_tapmajor', 0)):      # ... below the 128- and the 32-wide family's
        with pytest.raises(SdnHipError):
            _gemm_call(wide, rows=rows)
    ws = _gemm_workspace(name)
    need = 2 * P.c['N'] * P.OH * P.OW * P.Cop * 4           # two slices of the output
    assert ws.numel() >= need
    with pytest.raises(SdnHipError, match='error %d' % u.SDN_ENOMEM):
        _gemm_call(name, ws, workspace_bytes=need - 1)
    out, st = _gemm_call(name, ws, workspace_bytes=need)
    _gemm_check(name, 'workspace of exactly two slices', out, st)


# ------------------------------------------------------------------------------------------ sdn_conv_wgrad
def _wgrad_call(name, workspace=None, workspace_bytes=None):
    from sdn_hip import check, lib, ptr, stream
    P = u.wgrad_problem(name)
    c = P.c
    rows = u.channels_last(P.rows, P.Cr).to(DEV)
    gath = u.channels_last(P.gath, P.Cc).to(DEV)
    nt = len(P.WL.taps)
    dw = P.base.to(DEV) if P.base is not None else torch.zeros(P.Cr, nt * P.Cc, device=DEV)
    wb = 0 if workspace is None else (workspace.numel() * 4 if workspace_bytes is None else workspace_bytes)
    check(lib().sdn_conv_wgrad(ptr(rows), ptr(gath), ptr(dw), c['N'], P.WL.QH, P.WL.QW, P.Cr, P.GH, P.GW, P.Cc, P.WL.istride, nt,
                               _i8s([t[0] for t in P.WL.taps]), _i8s([t[1] for t in P.WL.taps]), c['reflect'], c['relu_rows'],
                               c['relu_gath'], c['splits'], c['precision'], ptr(workspace), wb, stream()))
    torch.cuda.synchronize()
    return dw.cpu()


def _wgrad_check(name, mode, dw):
    P = u.wgrad_problem(name)
    c = P.c
    nt = len(P.WL.taps)
    base = P.base if P.base is not None else torch.zeros(P.Cr, nt * P.Cc)
    ref = u.wgrad_reference(name)
    got3, base3 = dw.reshape(P.Cr, nt, P.Cc), base.reshape(P.Cr, nt, P.Cc)
    assert bool(torch.isfinite(dw).all()), (name, mode, 'not finite')
    want = ref + base3[:c['nr'], :, :c['nc']].double()
    err = float((got3[:c['nr'], :, :c['nc']].double() - want).abs().max()) / float(ref.abs().max())
    print('sdn_conv_wgrad | %s | %s: gate %.1e measured %.3e' % (name, mode, u.GATE, err))
    assert err <= u.GATE, (name, mode, err)
    # rows and channels behind the real ones receive sums of zeros: they stay exactly what they were
    assert torch.equal(got3[c['nr']:], base3[c['nr']:]), (name, mode, 'padding rows changed')
    assert torch.equal(got3[:, :, c['nc']:], base3[:, :, c['nc']:]), (name, mode, 'padding channels changed')


@pytest.mark.parametrize('name', list(u.WGRAD_CASES))
def test_conv_wgrad_matches_float64(name):
    """dw += the float64 autograd weight gradient, from a random base or from zeros; cases of more than one slice also in the
    deterministic mode (within the gate, bit-identical over two calls, SDN_ENOMEM for a workspace one byte too small)"""
    from sdn_hip import SdnHipError
    P = u.wgrad_problem(name)
    slices = len(P.c['geo'][4])
    _wgrad_check(name, 'atomics' if slices > 1 else 'one slice', _wgrad_call(name))
    if P.c['splits'] > 1:
        elems = slices * P.Cr * len(P.WL.taps) * P.Cc
        ws = torch.full((elems,), NAN, device=DEV)
        dw_a = _wgrad_call(name, ws)
        _wgrad_check(name, 'workspace', dw_a)
        if slices > 1:
            ws.fill_(NAN)
            assert u.same_bits(dw_a, _wgrad_call(name, ws)), (name, 'the deterministic mode gave different bits')
            with pytest.raises(SdnHipError, match='error %d' % u.SDN_ENOMEM):
                _wgrad_call(name, ws, workspace_bytes=4 * elems - 1)
            _wgrad_check(name, 'after the refusal', _wgrad_call(name, ws))


# ------------------------------------------------------------------------------------------ sdn_conv_narrow_fwd
def _narrow_call(name, **over):
    from sdn_hip import check, lib, ptr, stream
    P = u.narrow_problem(name)
    c = P.c
    xg = u.channels_last(P.x, c['cin']).to(DEV)
    wd = P.dense.to(DEV)
    bg = None
    if P.bias is not None:
        bg = torch.zeros(8, device=DEV)
        bg[:c['rows_used']] = P.bias.to(DEV)
    a = dict(Cop=c['Cop'], rows_used=c['rows_used'], KH=c['k'], KW=c['k'])
    a.update(over)
    out = torch.full((c['N'], c['H'], c['W'], c['Cop']), NAN, device=DEV)
    check(lib().sdn_conv_narrow_fwd(ptr(xg), c['N'], P.IH, P.IW, c['cin'], ptr(out), c['H'], c['W'], a['Cop'], a['rows_used'], ptr(wd),
                                    a['KH'], a['KW'], -P.pad, -P.pad, c['reflect'], c['in_relu'], ptr(bg), c['act'], stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', list(u.NARROW_CASES))
def test_conv_narrow_fwd_matches_float64(name):
    """all 15 (rows, window) builds, every channel-pass schedule, ragged and single tiles; exact fp32: gate max(2e-6, 4 e32)"""
    c = u.NARROW_CASES[name]
    out = _narrow_call(name)
    u.check_gate('sdn_conv_narrow_fwd', name, 'out', _nchw(out, c['rows_used']), u.narrow_reference(name),
                 u.narrow_reference(name, torch.float32), u.FLOOR_ACT)
    assert float(out[..., c['rows_used']:].abs().max()) == 0.0, (name, 'channels behind rows_used must come out as zeros')


def test_conv_narrow_fwd_refusals():
    from sdn_hip import SdnHipError
    name = 'r3_k4_two_rows_3x5'
    for over in (dict(KH=5, KW=5), dict(KH=3, KW=4), dict(rows_used=0), dict(rows_used=9)):
        with pytest.raises(SdnHipError):
            _narrow_call(name, **over)
    with pytest.raises(SdnHipError):                        # rows_used above Cop (the header also wants Cop padded to 16: 0 is)
        _narrow_call(name, Cop=0, rows_used=2)
    c = u.NARROW_CASES[name]
    u.check_gate('sdn_conv_narrow_fwd', name, 'out after the refusals', _nchw(_narrow_call(name), c['rows_used']),
                 u.narrow_reference(name), u.narrow_reference(name, torch.float32), u.FLOOR_ACT)


# ------------------------------------------------------------------------------------------ sdn_segment_mean
def _segment_abi(x, seg, K):
    """(out, sums, counts) of one sdn_segment_mean call; every buffer pre-filled with NaN"""
    from sdn_hip import check, lib, ptr, stream
    N, C, H, W = x.shape
    sums = torch.full((C, K), NAN, device=DEV)
    counts = torch.full((K,), NAN, device=DEV)
    out = torch.full_like(x, NAN)
    check(lib().sdn_segment_mean(ptr(x), ptr(seg), N, C, H * W, K, ptr(sums), ptr(counts), ptr(out), stream()))
    torch.cuda.synchronize()
    return out, sums, counts


@pytest.mark.parametrize('name', list(u.SEGMENT_CASES))
def test_segment_mean_matches_float64(name):
    """ops.SegmentMeanFn, forward and backward, on all three paths (ordered sums, LDS-table atomics, global atomics)"""
    from sdn_hip import ops
    P = u.segment_problem(name)
    r64, r32 = u.segment_reference(name), u.segment_reference(name, torch.float32)
    xg = P.x.to(DEV).detach().requires_grad_(True)
    out, means = ops.SegmentMeanFn.apply(xg, P.seg.to(torch.int32).to(DEV), P.c['K'])
    u.check_gate('sdn_segment_mean', name, 'out', out, r64['out'], r32['out'], u.FLOOR_FOLD)
    present = r64['present']
    u.check_gate('sdn_segment_mean', name, 'means of the present ids', means.detach().cpu()[:, present], r64['means'][:, present],
                 r32['means'][:, present], u.FLOOR_FOLD)
    (out * P.w.to(DEV)).sum().backward()
    u.check_gate('sdn_segment_mean', name, 'gradient', xg.grad, r64['grad'], r32['grad'], u.FLOOR_FOLD)


@pytest.mark.parametrize('name', u.SEGMENT_ORDERED)
def test_segment_mean_ordered_sums_are_repeatable(name):
    """the kernel's own promise for K <= 4096 and K <= HW: the same input gives the same bits (values over six decades: a different
    order of the float32 additions would show)"""
    P = u.segment_problem(name)
    x, seg = P.x.to(DEV), P.seg.to(torch.int32).to(DEV)
    out_a, sums_a, counts_a = _segment_abi(x, seg, P.c['K'])
    out_b, sums_b, counts_b = _segment_abi(x, seg, P.c['K'])
    assert u.same_bits(out_a, out_b) and u.same_bits(sums_a, sums_b) and u.same_bits(counts_a, counts_b), name
    r64 = u.segment_reference(name)
    assert torch.equal(counts_a.cpu().double(), torch.bincount(P.seg.reshape(-1), minlength=P.c['K']).double())
    assert bool(torch.isfinite(out_a).all()) and u.rel_l2(out_a, r64['out']) <= 1e-5


@pytest.mark.parametrize('name', ['groups', 'images', 'lds_atomics', 'global'])
def test_segment_mean_one_nan_pixel_poisons_exactly_its_instance(name):
    P = u.segment_problem(name)
    N, C, H, W = P.x.shape
    n, ch, y, xx = N - 1, C - 1, H // 2, W // 3
    x = P.x.clone()
    x[n, ch, y, xx] = NAN
    out, _, _ = _segment_abi(x.to(DEV), P.seg.to(torch.int32).to(DEV), P.c['K'])
    want = torch.zeros(N, C, H, W, dtype=torch.bool)
    want[:, ch] = P.seg == P.seg[n, y, xx]                  # the id's pixels in every image, in that channel only
    assert torch.equal(torch.isnan(out).cpu(), want), name
    clean = u.segment_reference(name)['out']
    assert u.rel_l2(out.cpu()[~want], clean[~want]) <= 1e-5
