"""Shared pieces of the operator-level tests of the r01-r03 conv kernels and the instance pooling (tests/test_conv_gemm_host.py,
tests/test_gpu_conv_gemm.py): case tables, seeded inputs, float64 / float32 references and the launch geometry, restated, for
sdn_conv_gemm (csrc/conv_gemm.hip), sdn_conv_wgrad (csrc/conv_wgrad.hip), sdn_conv_narrow_fwd (csrc/conv_narrow.hip) and
sdn_segment_mean (csrc/fast_segment.hip).  Nothing here needs a GPU.

References.  torch on the CPU in float64 from the float32 inputs: F.conv2d / F.conv_transpose2d, F.pad(mode='reflect') for
reflected borders, autograd of those for the weight gradient, clamp(min=0) for ReLU on load; the same call in float32 gives e32.
precision 1 (plain bf16): the same float64 expression on the bf16-rounded operands, f(x).bfloat16() and w.bfloat16() (the kernels
convert with round to nearest even; bf16 products are exact in fp32, so the gate is that of precision 3).

Gates.  sdn_conv_gemm / sdn_conv_wgrad: 1e-5 of the output scale, max |got - ref| / max |ref| -- the gate tests/test_gpu_conv_phases.py
holds for sdn_conv_gemm and tests/test_gpu_conv_tile.py for the kernels of the same arithmetic class; statistics as in the latter (sums
within 1e-5 (max |sum| + max sqrt(sum of squares)), sums of squares 1e-5 relative).  The host test holds the float32 CPU evaluation
of every such case to a quarter of the gate: a case that misses it is ill-conditioned and is redrawn before anything runs on a GPU.
sdn_conv_narrow_fwd (exact fp32) and sdn_segment_mean: conv_companions_util.check_gate, max(floor, 4 e32) on relative L2 with the
floors FLOOR_ACT (2e-6) and FLOOR_FOLD (1e-6).

Tanh and the output scale.  The error of the split products is proportional to the PRE-activation's scale (the sum of |terms|), tanh
passes it on unchanged where its slope is 1, and its output scale is at most 1 whatever the pre-activation's.  A tanh case drawn with
max |pre| = 3.5 therefore holds the products to 1e-5 / 3.5 of their scale, a level the arithmetic class does not have (the same
kernel measures 4e-6 .. 6e-6 of the scale without the tanh; tests/test_gpu_conv_head.py notes the same effect).  The weights of a
tanh case are drawn so that max |pre| / max |tanh(pre)| <= 1.25 and max |pre| >= 0.3 in the float64 reference (asserted by the host
test): the gate then measures the products at the level of every other case, and tanh(0.3) still differs from 0.3 by 3000 gates.
The first draw of split3_tapmajor (weights 0.025, max |pre| 3.6) measured 1.078e-5 in both split modes.

Launch geometry.  gemm_geometry, wgrad_geometry, narrow_geometry and segment_geometry restate launch_conv, sdn_conv_wgrad's slice
arithmetic, the narrow forward's channel-pass rule and sdn_segment_mean's chunking for ONE purpose: the host test asserts that every
named case reaches the tile family, K order, step and slice counts its row claims.  Whoever changes a threshold is told there to
pick new cases; no GPU assertion depends on the restatement.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from conv_companions_util import FLOOR_ACT, FLOOR_FOLD, bits, check_gate, rel_l2, same_bits  # noqa: F401  (re-exported)

GATE = 1e-5            # sdn_conv_gemm, sdn_conv_wgrad: of the output scale
STAT_SLOTS = 8         # SDN_STAT_SLOTS
MAX_TAPS = 64          # CONV_MAX_TAPS
SDN_ENOMEM = -3


def cpad(c):
    return (c + 15) // 16 * 16


def kpad(ntaps, ccp):
    return (ntaps * ccp + 31) // 32 * 32


def weight_rows(cop):
    return (cop + 127) // 128 * 128 if cop > 64 else (64 if cop > 32 else 32)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def scale_error(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------ sdn_conv_gemm
# kind 'conv': Conv2d(kh x kw, stride s, padding p, zero or reflected); 'taps': a 1 x kw window whose taps are listed by hand
# (dx = kx + dx0, zeros outside); 'phase': one phase (py, px) of ConvTranspose2d(k, stride s, padding p, output_padding 1).
# N, IH, IW: the layer's input.  geo = (channel tile, tiles, Kp, steps, ksplit, steps per slice, K order, K padding) as the
# launcher computes them -- asserted by the host test from gemm_geometry.
def _g(kind, N, IH, IW, cin, cout, k, s=1, p=0, reflect=0, in_relu=0, act=0, bias=0, stats=0, acc=0, precision=3, wscale=0.1,
       phase=None, dx0=0, geo=None):
    kh, kw = (k, k) if isinstance(k, int) else k
    return dict(kind=kind, N=N, IH=IH, IW=IW, cin=cin, cout=cout, kh=kh, kw=kw, s=s, p=p, reflect=reflect, in_relu=in_relu, act=act,
                bias=bias, stats=stats, acc=acc, precision=precision, wscale=wscale, phase=phase, dx0=dx0, geo=geo)


GEMM_CASES = {
    # 64-wide tile, channel-block-major K, two slices of 9 steps, k_bias_act_stats with 12 threads per position
    'split2': _g('conv', 1, 9, 9, 64, 48, 3, p=1, bias=1, stats=1, geo=(64, 1, 576, 18, 2, (9, 9), 'cmajor', 0)),
    # slices of 8 steps start in the middle of a channel block's 16 taps
    'split4_mid': _g('conv', 1, 9, 9, 64, 48, 4, p=2, act=1, geo=(64, 1, 1024, 32, 4, (8, 8, 8, 8), 'cmajor', 0)),
    # 32-wide tile (one accumulator per product), tap-major with one group per tap, 16 columns of K padding, two position
    # tiles (128 + 15 positions)
    'split3_tapmajor': _g('conv', 1, 11, 13, 16, 32, 7, p=3, reflect=1, act=2, bias=1, wscale=0.0054,
                          geo=(32, 2, 800, 25, 3, (9, 9, 7), 'tapmajor', 16)),
    'split32': _g('conv', 1, 9, 9, 1024, 1024, 3, p=1, geo=(128, 8, 9216, 288, 32, (9,) * 32, 'cmajor', 0)),
    # ragged ninth channel tile; k_bias_act_stats takes a second channel pass (260 > 256 threads per position)
    'split_wide': _g('conv', 1, 8, 8, 64, 1040, 3, p=1, bias=1, stats=1, geo=(128, 9, 576, 18, 2, (9, 9), 'cmajor', 0)),
    'split_acc': _g('conv', 1, 9, 9, 64, 48, 3, p=1, acc=1, geo=(64, 1, 576, 18, 2, (9, 9), 'cmajor', 0)),
    # accumulate with a fused tail keeps ksplit 1: the fused epilogue with +=
    'nosplit_acc_tail': _g('conv', 1, 9, 9, 64, 48, 3, p=1, bias=1, acc=1, geo=(64, 1, 576, 18, 1, (18,), 'cmajor', 0)),
    # 164 tiles: above the split threshold; statistics slots mtile & 7 wrap (41 position tiles an image)
    'nosplit_big': _g('conv', 4, 72, 72, 64, 48, 3, p=1, stats=1, geo=(64, 164, 576, 18, 1, (18,), 'cmajor', 0)),
    # tap-major with three groups per tap: steps straddle taps; ragged second channel tile
    'gpt3': _g('conv', 2, 20, 30, 48, 160, 3, p=1, reflect=1, in_relu=1, act=1, stats=1,
               geo=(128, 20, 448, 14, 1, (14,), 'tapmajor', 16)),
    'steps1_pad': _g('conv', 1, 5, 5, 16, 16, 1, geo=(32, 1, 32, 1, 1, (1,), 'tapmajor', 16)),
    'steps1': _g('conv', 1, 5, 5, 32, 16, 1, geo=(32, 1, 32, 1, 1, (1,), 'cmajor', 0)),
    'steps2': _g('taps', 1, 5, 5, 32, 64, (1, 2), geo=(64, 1, 64, 2, 1, (2,), 'cmajor', 0)),
    'steps3': _g('taps', 1, 5, 5, 32, 64, (1, 3), dx0=-1, geo=(64, 1, 96, 3, 1, (3,), 'cmajor', 0)),
    'steps5': _g('conv', 1, 5, 5, 16, 16, 3, p=1, geo=(32, 1, 160, 5, 1, (5,), 'tapmajor', 16)),
    # istride 2 on an odd input grid (16 steps and 4 tiles: the launcher splits it in two)
    's2': _g('conv', 2, 25, 31, 32, 64, 4, s=2, p=2, geo=(64, 4, 512, 16, 2, (8, 8), 'cmajor', 0)),
    # the 64-wide tile in tap-major order, split (the shape of the weight-gradient case of the same name)
    'reflect7': _g('conv', 1, 9, 11, 16, 64, 7, p=3, reflect=1, geo=(64, 1, 800, 25, 3, (9, 9, 7), 'tapmajor', 16)),
    # ostride 2: the positions the phase does not own keep their bits
    'phase': _g('phase', 2, 9, 14, 64, 96, 3, s=2, p=1, phase=(1, 0), geo=(128, 2, 128, 4, 1, (4,), 'cmajor', 0)),
    'bf16_split2': _g('conv', 1, 9, 9, 64, 48, 3, p=1, bias=1, stats=1, precision=1, geo=(64, 1, 576, 18, 2, (9, 9), 'cmajor', 0)),
    'bf16_gpt3': _g('conv', 2, 20, 30, 48, 160, 3, p=1, reflect=1, in_relu=1, act=1, stats=1, precision=1,
                    geo=(128, 20, 448, 14, 1, (14,), 'tapmajor', 16)),
    # channel counts that are no multiple of 16: padding channels of the fused and of the split epilogue
    'pad_channels': _g('conv', 1, 5, 5, 16, 20, 3, p=1, act=1, bias=1, geo=(32, 1, 160, 5, 1, (5,), 'tapmajor', 16)),
    'split_pad': _g('conv', 1, 9, 9, 60, 40, 3, p=1, bias=1, stats=1, geo=(64, 1, 576, 18, 2, (9, 9), 'cmajor', 0)),
}
GEMM_SPLIT_CASES = [n for n, c in GEMM_CASES.items() if c['geo'][4] > 1]


def gemm_launch(c):
    """(QH, QW, istride, ostride, py, px, taps [(dy, dx)], tapidx, OH, OW) of the case's one sdn_conv_gemm call"""
    from sdn_hip import convplan as cp
    if c['kind'] == 'conv':
        (L,), (OH, OW) = cp.conv_fwd(c['kh'], c['s'], c['p'], c['IH'], c['IW'])
        return tuple(L) + (OH, OW)
    if c['kind'] == 'taps':
        taps = [(0, kx + c['dx0']) for kx in range(c['kw'])]
        return (c['IH'], c['IW'], 1, 1, 0, 0, taps, list(range(c['kw'])), c['IH'], c['IW'])
    launches, (OH, OW) = cp.convT_fwd(c['kh'], c['s'], c['p'], 1, c['IH'], c['IW'])
    (L,) = [Lh for Lh in launches if (Lh.py, Lh.px) == c['phase']]
    return tuple(L) + (OH, OW)


def gemm_geometry(c):
    """launch_conv of csrc/conv_gemm.hip, restated: (channel tile, tiles, Kp, steps, ksplit, steps per slice, K order, K padding)"""
    QH, QW, ist, ost, py, px, taps, _, OH, OW = gemm_launch(c)
    Cip, Cop = cpad(c['cin']), cpad(c['cout'])
    Kp = kpad(len(taps), Cip)
    bn = 128 if Cop > 64 else (64 if Cop > 32 else 32)
    tiles = -(-QH * QW // 128) * c['N'] * -(-Cop // bn)
    steps = Kp // 32
    dense = ost == 1 and py == 0 and px == 0 and QH == OH and QW == OW
    fused_tail = bool(c['bias'] or c['act'] or c['stats'])
    ksplit = 1
    if dense and tiles <= 160 and steps >= 16 and not (c['acc'] and fused_tail):
        ksplit = min(-(-512 // tiles), steps // 8, 32)
        if ksplit < 2:
            ksplit = 1
    sps = -(-steps // ksplit)
    ksplit = -(-steps // sps)
    slices = tuple(min(sps, steps - z * sps) for z in range(ksplit))
    cmajor = Cip % 32 == 0 and Kp == len(taps) * Cip
    return (bn, tiles, Kp, steps, ksplit, slices, 'cmajor' if cmajor else 'tapmajor', Kp - len(taps) * Cip)


def bias_act_stats_passes(c):
    """(threads per position of each channel pass of k_bias_act_stats)"""
    C4 = cpad(c['cout']) // 4
    return tuple(min(C4 - q, 256) for q in range(0, C4, 256))


@functools.lru_cache(maxsize=None)
def _gemm_problem(name):
    c = GEMM_CASES[name]
    g = torch.Generator().manual_seed(9100 + _seed(name.replace('bf16_', '')))
    QH, QW, ist, ost, py, px, taps, tapidx, OH, OW = gemm_launch(c)
    x = torch.randn(c['N'], c['cin'], c['IH'], c['IW'], generator=g)
    if c['kind'] == 'phase':
        w = torch.randn(c['cin'], c['cout'], c['kh'], c['kw'], generator=g) * c['wscale']
        R, C, sr, sc = c['cout'], c['cin'], c['kh'] * c['kw'], c['cout'] * c['kh'] * c['kw']
    else:
        w = torch.randn(c['cout'], c['cin'], c['kh'], c['kw'], generator=g) * c['wscale']
        R, C, sr, sc = c['cout'], c['cin'], c['cin'] * c['kh'] * c['kw'], c['kh'] * c['kw']
    bias = torch.randn(c['cout'], generator=g) * 5 * c['wscale'] if c['bias'] else None
    Cip, Cop = cpad(c['cin']), cpad(c['cout'])
    base = torch.randn(c['N'], OH, OW, Cop, generator=g) if c['acc'] else None
    return SimpleNamespace(name=name, c=c, x=x, w=w, bias=bias, base=base, QH=QH, QW=QW, istride=ist, ostride=ost, py=py, px=px,
                           taps=taps, tapidx=tapidx, OH=OH, OW=OW, R=R, C=C, sr=sr, sc=sc, Cip=Cip, Cop=Cop,
                           rows=weight_rows(Cop), Kp=kpad(len(taps), Cip))


def gemm_problem(name):
    """the case's seeded inputs (float32, torch layouts; shared, do not modify) and its launch arguments"""
    return _gemm_problem(name)


def _operand(t, precision, dtype):
    return t.bfloat16().to(dtype) if precision == 1 else t.to(dtype)


@functools.lru_cache(maxsize=None)
def gemm_reference(name, dtype=torch.float64):
    """(pre, post) [N, cout, OH, OW] in `dtype`: pre-activation with bias (what the statistics sum) and the activated output (without
    the accumulate base).  For 'phase' the whole transposed convolution: the phase owns [py::s, px::s]."""
    P = gemm_problem(name)
    c = P.c
    x = P.x.clamp(min=0) if c['in_relu'] else P.x
    x, w = _operand(x, c['precision'], dtype), _operand(P.w, c['precision'], dtype)
    b = None if P.bias is None else P.bias.to(dtype)
    if c['kind'] == 'conv':
        p = c['p']
        if c['reflect']:
            pre = F.conv2d(F.pad(x, (p, p, p, p), mode='reflect'), w, b, stride=c['s'])
        else:
            pre = F.conv2d(x, w, b, stride=c['s'], padding=p)
    elif c['kind'] == 'taps':
        lo, hi = -c['dx0'], c['kw'] - 1 + c['dx0']
        pre = F.conv2d(F.pad(x, (lo, hi, 0, 0)), w, b)
    else:
        pre = F.conv_transpose2d(x, w, b, stride=c['s'], padding=c['p'], output_padding=1)
    post = F.leaky_relu(pre, 0.2) if c['act'] == 1 else torch.tanh(pre) if c['act'] == 2 else pre
    return pre, post


def channels_last(t, cp):
    """NCHW -> [N, H, W, cp] float32 with zero pad channels (CPU)"""
    n, ch, h, w = t.shape
    out = torch.zeros(n, h, w, cp, dtype=t.dtype)
    out[..., :ch] = t.permute(0, 2, 3, 1)
    return out.contiguous()


def gather_sum(P, x=None):
    """the launch formula of include/sdn_hip.h, evaluated by a plain numpy gather-sum in float64 on the launch arguments the GPU test
    passes (taps, tapidx, strides of the weight, istride / ostride / phase):
        out[n, qy os + py, qx os + px, co] = bias[co] + sum_t sum_ci f(in[n, qy is + dy_t, qx is + dx_t, ci]) w[co sr + ci sc + tapidx_t]
    Returns [N, OH, OW, cout] with NaN where the launch does not write."""
    c = P.c
    xin = (P.x if x is None else x).double()
    xin = (xin.clamp(min=0) if c['in_relu'] else xin).permute(0, 2, 3, 1).numpy()
    wf = P.w.double().flatten().numpy()
    N, IH, IW, _ = xin.shape
    out = np.full((N, P.OH, P.OW, P.R), np.nan)
    r, ci = np.arange(P.R)[:, None], np.arange(P.C)[None, :]
    Wt = [wf[r * P.sr + ci * P.sc + ti] for ti in P.tapidx]
    for qy in range(P.QH):
        for qx in range(P.QW):
            acc = np.zeros((N, P.R)) + (0.0 if P.bias is None else P.bias.double().numpy())
            for (dy, dx), W in zip(P.taps, Wt):
                iy, ix = qy * P.istride + dy, qx * P.istride + dx
                if c['reflect']:
                    iy, ix = abs(iy), abs(ix)
                    iy, ix = min(iy, 2 * IH - 2 - iy), min(ix, 2 * IW - 2 - ix)
                if 0 <= iy < IH and 0 <= ix < IW:
                    acc += xin[:, iy, ix, :] @ W.T
            out[:, qy * P.ostride + P.py, qx * P.ostride + P.px] = acc
    return out


# ------------------------------------------------------------------------------------------ sdn_conv_wgrad
# kind 'conv': rows = d(out) [N, cout, QH, QW], gathered = the input; 'convT': rows = the input [N, cin, QH, QW], gathered = d(out).
# nr / nc: real rows / gathered channels.  geo = (row-tile family, row tiles, column tiles, steps, slices (steps of each)).
def _w(kind, N, QH, QW, nr, nc, k, s=1, p=1, reflect=0, relu_rows=0, relu_gath=0, splits=1, base=1, precision=3, geo=None):
    return dict(kind=kind, N=N, QH=QH, QW=QW, nr=nr, nc=nc, k=k, s=s, p=p, reflect=reflect, relu_rows=relu_rows, relu_gath=relu_gath,
                splits=splits, base=base, precision=precision, geo=geo)


WGRAD_CASES = {
    # 32-row family (one accumulator per product); a 32-position step crosses eight images; QW = 2 reciprocal
    'tiny_images': _w('conv', 9, 2, 2, 32, 32, 3, geo=(32, 1, 3, 2, (2,))),
    # QH >= 64 compare path with QW = 1
    'column': _w('conv', 2, 64, 1, 24, 20, 3, base=0, geo=(32, 1, 3, 4, (4,))),
    'tall': _w('conv', 3, 70, 3, 48, 16, 3, geo=(64, 1, 2, 20, (20,))),
    'row32': _w('conv', 1, 5, 32, 32, 16, 3, base=0, geo=(32, 1, 2, 5, (5,))),
    'row31': _w('conv', 1, 5, 31, 32, 16, 3, geo=(32, 1, 2, 5, (5,))),
    # a single partial step that ends at an odd position
    'odd_tail': _w('conv', 1, 3, 5, 64, 32, 3, base=0, geo=(64, 1, 3, 1, (1,))),
    # 432 columns: four column tiles, the last 48 of 128 (groups behind the last tap)
    'rows64': _w('conv', 2, 12, 18, 48, 48, 3, geo=(64, 1, 4, 14, (14,))),
    'rows160': _w('conv', 1, 14, 20, 160, 64, 4, p=2, base=0, geo=(128, 2, 8, 9, (9,))),
    's2_conv': _w('conv', 2, 11, 17, 64, 48, 3, s=2, geo=(64, 1, 4, 12, (12,))),
    's2_convT': _w('convT', 2, 9, 13, 40, 24, 3, s=2, base=0, geo=(64, 1, 3, 8, (8,))),
    'reflect7': _w('conv', 1, 9, 11, 64, 16, 7, p=3, reflect=1, geo=(64, 1, 7, 4, (4,))),
    'relu_rows': _w('conv', 2, 12, 18, 48, 48, 3, relu_rows=1, geo=(64, 1, 4, 14, (14,))),
    'relu_gath': _w('conv', 2, 12, 18, 48, 48, 3, relu_gath=1, base=0, geo=(64, 1, 4, 14, (14,))),
    'relu_both': _w('conv', 2, 12, 18, 48, 48, 3, relu_rows=1, relu_gath=1, geo=(64, 1, 4, 14, (14,))),
    'splits3_of_7': _w('conv', 1, 7, 31, 32, 16, 3, splits=3, geo=(32, 1, 2, 7, (3, 3, 1))),
    'splits4_of_10': _w('conv', 1, 17, 17, 64, 32, 3, splits=4, base=0, geo=(64, 1, 3, 10, (3, 3, 3, 1))),
    'splits8_clamped': _w('conv', 1, 3, 5, 64, 32, 3, splits=8, geo=(64, 1, 3, 1, (1,))),
    'splits5_tall': _w('conv', 3, 70, 3, 48, 16, 3, splits=5, geo=(64, 1, 2, 20, (4, 4, 4, 4, 4))),
    'bf16_rows64': _w('conv', 2, 12, 18, 48, 48, 3, precision=1, geo=(64, 1, 4, 14, (14,))),
}


def wgrad_geometry(c):
    """the launcher of csrc/conv_wgrad.hip, restated: (row-tile family, row tiles, column tiles, steps, steps of each slice)"""
    Cr, Cc = cpad(c['nr']), cpad(c['nc'])
    ncols = c['k'] * c['k'] * Cc
    steps = -(-c['N'] * c['QH'] * c['QW'] // 32)
    splits = min(c['splits'], steps)
    sps = -(-steps // splits)
    zs = -(-steps // sps)
    family = 64 if 32 < Cr <= 64 else (128 if Cr > 32 else 32)
    return (family, -(-Cr // 128) if Cr > 64 else 1, -(-ncols // 128), steps, tuple(min(sps, steps - z * sps) for z in range(zs)))


def wgrad_sizes(c):
    """(GH, GW) of the gathered operand"""
    if c['kind'] == 'conv':
        return (c['QH'] - 1) * c['s'] + c['k'] - 2 * c['p'], (c['QW'] - 1) * c['s'] + c['k'] - 2 * c['p']
    return (c['QH'] - 1) * c['s'] - 2 * c['p'] + c['k'] + 1, (c['QW'] - 1) * c['s'] - 2 * c['p'] + c['k'] + 1


@functools.lru_cache(maxsize=None)
def wgrad_problem(name):
    """rows / gath (NCHW float32), base [Cr, ntaps Cc] or None, the WLaunch of the plan; shared, do not modify"""
    from sdn_hip import convplan as cp
    c = WGRAD_CASES[name]
    g = torch.Generator().manual_seed(9200 + _seed(name.replace('bf16_', '')))
    GH, GW = wgrad_sizes(c)
    rows = torch.randn(c['N'], c['nr'], c['QH'], c['QW'], generator=g)
    gath = torch.randn(c['N'], c['nc'], GH, GW, generator=g)
    WL = (cp.conv_wgrad if c['kind'] == 'conv' else cp.convT_wgrad)(c['k'], c['s'], c['p'], c['QH'], c['QW'])
    Cr, Cc = cpad(c['nr']), cpad(c['nc'])
    base = torch.randn(Cr, len(WL.taps) * Cc, generator=g) if c['base'] else None
    return SimpleNamespace(name=name, c=c, rows=rows, gath=gath, base=base, WL=WL, GH=GH, GW=GW, Cr=Cr, Cc=Cc)


@functools.lru_cache(maxsize=None)
def wgrad_reference(name, dtype=torch.float64):
    """autograd weight gradient in `dtype`, laid out [r][tap of the plan][c] (real rows and channels only)"""
    P = wgrad_problem(name)
    c = P.c
    rows = P.rows.clamp(min=0) if c['relu_rows'] else P.rows
    gath = P.gath.clamp(min=0) if c['relu_gath'] else P.gath
    rows, gath = _operand(rows, c['precision'], dtype), _operand(gath, c['precision'], dtype)
    k, s, p = c['k'], c['s'], c['p']
    if c['kind'] == 'conv':
        w = torch.zeros(c['nr'], c['nc'], k, k, dtype=dtype, requires_grad=True)
        y = F.conv2d(F.pad(gath, (p, p, p, p), mode='reflect'), w, stride=s) if c['reflect'] else F.conv2d(gath, w, stride=s, padding=p)
        (y * rows).sum().backward()
    else:
        w = torch.zeros(c['nr'], c['nc'], k, k, dtype=dtype, requires_grad=True)       # ConvTranspose2d weight [cin, cout, k, k]
        y = F.conv_transpose2d(rows, w, stride=s, padding=p, output_padding=1)
        (y * gath).sum().backward()
    return w.grad.permute(0, 2, 3, 1).reshape(c['nr'], k * k, c['nc'])[:, list(P.WL.tapidx), :].contiguous()


# ------------------------------------------------------------------------------------------ sdn_conv_narrow_fwd
# name: N, output grid H x W, cin, rows_used, k (padding k // 2: the 4 x 4 window has dy_min = -2 and an input one smaller than the
# output, the discriminators' padding), borders, ReLU on load, act, bias, Cop; geo = (R build, tiles, channels per pass, passes)
def _n(N, H, W, cin, rows_used, k, reflect=0, in_relu=0, act=0, bias=0, Cop=16, geo=None):
    return dict(N=N, H=H, W=W, cin=cin, rows_used=rows_used, k=k, reflect=reflect, in_relu=in_relu, act=act, bias=bias, Cop=Cop, geo=geo)


NARROW_CASES = {
    'r1_k7_13x70': _n(1, 13, 70, 16, 1, 7, geo=(1, 6, 16, 1)),
    'r3_k7_generator_head': _n(2, 9, 33, 64, 3, 7, reflect=1, in_relu=1, act=2, bias=1, geo=(3, 8, 64, 1)),
    'r4_k7_one_tile_three_passes': _n(1, 8, 32, 48, 4, 7, reflect=1, act=1, bias=1, Cop=32, geo=(4, 1, 16, 3)),
    'r5_k7_encoder_head': _n(1, 13, 70, 16, 5, 7, reflect=1, act=2, bias=1, geo=(5, 6, 16, 1)),
    'r8_k7_six_rows_two_passes_of_64': _n(1, 9, 33, 128, 6, 7, bias=1, geo=(8, 4, 64, 2)),
    'r1_k4_discriminator_head': _n(2, 13, 70, 64, 1, 4, bias=1, geo=(1, 12, 64, 1)),
    'r3_k4_two_rows_3x5': _n(1, 3, 5, 16, 2, 4, act=1, geo=(3, 1, 16, 1)),
    'r4_k4_reflect': _n(1, 9, 33, 48, 4, 4, reflect=1, in_relu=1, act=2, bias=1, Cop=32, geo=(4, 4, 16, 3)),
    'r5_k4_one_tile': _n(1, 8, 32, 16, 5, 4, act=1, geo=(5, 1, 16, 1)),
    'r8_k4_two_passes_of_64': _n(1, 9, 33, 128, 8, 4, in_relu=1, bias=1, geo=(8, 4, 64, 2)),
    # 4 x 16 x 4 tiles: the threshold at which 64 input channels go in four passes of 16 (N 4 at 64 x 128 is only 128 tiles)
    'r1_k3_256_tiles_four_passes': _n(4, 128, 128, 64, 1, 3, reflect=1, bias=1, geo=(1, 256, 16, 4)),
    'r3_k3_3x5': _n(1, 3, 5, 16, 3, 3, reflect=1, act=2, geo=(3, 1, 16, 1)),
    'r4_k3_three_passes': _n(1, 13, 70, 48, 4, 3, in_relu=1, act=1, geo=(4, 6, 16, 3)),
    'r5_k3_reflect': _n(1, 9, 33, 64, 5, 3, reflect=1, act=2, bias=1, geo=(5, 4, 64, 1)),
    'r8_k3_seven_rows': _n(1, 8, 32, 128, 7, 3, bias=1, Cop=32, geo=(8, 1, 64, 2)),
}


def narrow_build(rows_used):
    return 1 if rows_used == 1 else (3 if rows_used <= 3 else (rows_used if rows_used <= 5 else 8))


def narrow_geometry(c):
    """sdn_conv_narrow_fwd's launcher, restated: (R build, tiles, channels per LDS pass, passes)"""
    tiles = c['N'] * -(-c['H'] // 8) * -(-c['W'] // 32)
    ch_pass = 16 if (tiles >= 256 or c['cin'] < 64) else 64
    return (narrow_build(c['rows_used']), tiles, ch_pass, -(-c['cin'] // ch_pass))


def narrow_input_size(c):
    d = 1 if c['k'] == 4 else 0
    return c['H'] - d, c['W'] - d


@functools.lru_cache(maxsize=None)
def narrow_problem(name):
    """x [N, cin, IH, IW], w [rows_used, cin, k, k], bias or None, and the dense window [k][k][cin][RP] the kernel reads"""
    c = NARROW_CASES[name]
    g = torch.Generator().manual_seed(9300 + _seed(name))
    IH, IW = narrow_input_size(c)
    k, ru = c['k'], c['rows_used']
    x = torch.randn(c['N'], c['cin'], IH, IW, generator=g)
    w = torch.randn(ru, c['cin'], k, k, generator=g) * (0.7 / (c['cin'] * k * k) ** 0.5 if c['act'] == 2 else 0.1)
    bias = torch.randn(ru, generator=g) * 0.3 if c['bias'] else None
    RP = 1 if ru == 1 else (4 if ru <= 4 else 8)
    dense = torch.zeros(k, k, c['cin'], RP)
    dense[..., :ru] = w.permute(2, 3, 1, 0)
    return SimpleNamespace(name=name, c=c, x=x, w=w, bias=bias, dense=dense.contiguous(), IH=IH, IW=IW, RP=RP, pad=k // 2)


@functools.lru_cache(maxsize=None)
def narrow_reference(name, dtype=torch.float64):
    P = narrow_problem(name)
    c = P.c
    x = (P.x.clamp(min=0) if c['in_relu'] else P.x).to(dtype)
    b = None if P.bias is None else P.bias.to(dtype)
    p = P.pad
    if c['reflect']:
        y = F.conv2d(F.pad(x, (p, p, p, p), mode='reflect'), P.w.to(dtype), b)
    else:
        y = F.conv2d(x, P.w.to(dtype), b, padding=p)
    return F.leaky_relu(y, 0.2) if c['act'] == 1 else torch.tanh(y) if c['act'] == 2 else y


# ------------------------------------------------------------------------------------------ sdn_segment_mean
# name: N, C, H, W, K, id map ('blocks': spatially coherent, 'random', 'unique': every pixel its own id);
# geo = (path, chunks, k tiles of the combine kernel)
SEGMENT_CASES = {
    'one_chunk': dict(N=1, C=2, H=25, W=40, K=9, ids='blocks', geo=('ordered', 1, 1)),
    'groups': dict(N=1, C=2, H=131, W=140, K=70, ids='blocks', geo=('ordered', 18, 2)),
    'images': dict(N=3, C=4, H=37, W=91, K=7, ids='random', geo=('ordered', 4, 1)),
    'k_eq_hw': dict(N=1, C=1, H=8, W=8, K=64, ids='unique', geo=('ordered', 1, 1)),
    'lds_atomics': dict(N=1, C=2, H=16, W=16, K=300, ids='random', geo=('lds_atomics', 1, 0)),
    'global': dict(N=2, C=3, H=37, W=91, K=5000, ids='random', geo=('global', 1, 0)),
}
SEGMENT_ORDERED = ('one_chunk', 'groups', 'images')


def segment_geometry(c):
    """sdn_segment_mean's path and chunking, restated"""
    N, C, HW, K = c['N'], c['C'], c['H'] * c['W'], c['K']
    if K <= 4096 and K <= HW:
        chunks = max(min(4096 // (N * C), HW // K), 1)
        chunk = max(-(-HW // chunks), 1024)
        return ('ordered', -(-HW // chunk), -(-K // 64))
    chunks = max(2048 // (N * C), 1)
    chunk = max(-(-HW // chunks), 4096)
    return ('lds_atomics' if K <= 4096 else 'global', -(-HW // chunk), 0)


@functools.lru_cache(maxsize=None)
def segment_problem(name):
    """x (values over six decades, so that the order of a float32 sum matters), seg [N, H, W] int64 ids in [0, K) with some ids
    absent, w (the weights of the scalar the backward pass differentiates)"""
    c = SEGMENT_CASES[name]
    N, C, H, W, K = c['N'], c['C'], c['H'], c['W'], c['K']
    g = torch.Generator().manual_seed(9400 + _seed(name))
    if c['ids'] == 'unique':
        seg = torch.randperm(H * W, generator=g).reshape(1, H, W).repeat(N, 1, 1)
    elif c['ids'] == 'random':
        seg = torch.randint(0, K, (N, H, W), generator=g)
        seg[seg == K // 2] = 0                                   # an absent id
        seg[0, :min(H, 10), :min(W, 40)] = 0                     # one large coherent segment, as instances are
    else:
        by, bx = -(-H // 5), -(-W // 7)                          # 5 x 7 blocks with ids from [0, K), then one stray pixel in a hundred
        blk = (torch.arange(H)[:, None] // by) * 7 + torch.arange(W)[None, :] // bx
        seg = torch.randint(0, K, (35,), generator=g)[blk].expand(N, H, W).clone()
        stray = torch.rand(N, H, W, generator=g) < 0.01
        seg = torch.where(stray, torch.randint(0, K, (N, H, W), generator=g), seg)
        seg[seg == K // 2] = 0                                   # an absent id
    x = torch.randn(N, C, H, W, generator=g) * 10.0 ** (torch.rand(N, C, H, W, generator=g) * 6 - 3)
    w = torch.randn(N, C, H, W, generator=g)
    return SimpleNamespace(name=name, c=c, x=x, seg=seg, w=w)


@functools.lru_cache(maxsize=None)
def segment_reference(name, dtype=torch.float64):
    """the index_add reference: dict out [N, C, H, W], means [C, K], present [K] bool, grad (of sum(out w) with respect to x)"""
    P = segment_problem(name)
    N, C, H, W, K = (P.c[k] for k in 'NCHWK')
    x = P.x.to(dtype).clone().requires_grad_(True)
    flat = x.permute(1, 0, 2, 3).reshape(C, -1)
    idx = P.seg.reshape(-1)
    sums = torch.zeros(C, K, dtype=dtype).index_add(1, idx, flat)
    cnt = torch.bincount(idx, minlength=K).to(dtype).clamp(min=1)
    out = (sums / cnt)[:, idx].reshape(C, N, H, W).permute(1, 0, 2, 3)
    (out * P.w.to(dtype)).sum().backward()
    return dict(out=out.detach(), means=(sums / cnt).detach(), present=torch.bincount(idx, minlength=K) > 0, grad=x.grad)
