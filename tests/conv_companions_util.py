"""Shared pieces of the conv-companion kernel tests (tests/test_conv_companions_host.py, tests/test_gpu_conv_companions.py):
case tables, seeded generators, float64 / float32 references and gate helpers for the HBM-bound kernels that sit between the
convolutions -- csrc/conv_norm.hip (InstanceNorm apply / backward, activation backward, reflection fold, weight pack and
gradient unpack), csrc/conv_pack.h, csrc/fast_program.hip (k_weights_multi, k_add, k_colsum) and csrc/conv_bn.hip (BatchNorm,
3x3 stride-2 max pool, global average pool).  Nothing here needs a GPU.

References.  Every reference is written out as formulas and evaluated by torch on the CPU in float64 from the float32 input
values; the same function in float32 gives e32, the relative L2 error of a float32 evaluation of the same expression.
tests/test_conv_companions_host.py checks each formula against torch's own operator (F.instance_norm with running statistics,
F.batch_norm, autograd of F.pad(mode='reflect'), F.max_pool2d, F.leaky_relu / relu / tanh autograd).  torch refuses HW = 1 for
InstanceNorm and one row for BatchNorm in training: those cases are checked against the formula only.

Gates.  gate = max(floor, 4 e32) on relative L2 (the factor 4 covers a different but legitimate summation order).  The floors are
gates the project already holds at operator level, none is taken from the kernels under test: 2e-6 for normalised activations
(the BatchNorm forward of tests/test_gpu_encoder.py), 2e-5 for gradients and per-channel reductions (the same test and
frame_kernels_util.FLOOR_GRAD), 1e-6 for the reflection fold and the pools (tests/test_gpu_segm_ppm.py, test_gpu_encoder.py).
A per-channel sum that ends in fp32 atomics (bias_grad of sdn_act_bwd) is measured relative to sum |terms| of its channel, not
to the possibly cancelling sum: floor 2e-5.

Launch geometry.  ppb_for, zchunks and bn_grid restate the launch code of conv_norm.hip / conv_bn.hip for ONE purpose: the host
test asserts that every named case has the block count, positions per block and last-block fill its name claims.  Whoever changes
the launch geometry is told there to pick new cases; no GPU assertion depends on the restatement.

Exact kinks.  The InstanceNorm-backward inputs are quantised: z = mu_c + q / 256 with integer q in +- pairs, so that every
per-(image, channel) mean is exactly mu_c in float32 and float64 alike, z - mean is exact, and the planted q = 0 positions give
xhat == 0 exactly -- the kink of ReLU (gradient 0) and LeakyReLU (slope 0.2), where kernel and torch follow the same rule.  The
sign of xhat is then the same in both precisions, so no sign flip inflates e32.
"""
import functools

import torch

FLOOR_ACT = 2e-6     # normalised activations
FLOOR_GRAD = 2e-5    # gradients and per-channel reductions
FLOOR_FOLD = 1e-6    # reflection fold, pools
STAT_SLOTS = 8       # SDN_STAT_SLOTS
SUMS_ZEROED = 8      # SDN_IN_BWD_SUMS_ZEROED
EPS = 1e-5
MOMENTUM = 0.1
NAN = float('nan')


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def gate(floor, e32):
    return max(floor, 4.0 * e32)


def check_gate(kernel, case, name, got, ref64, ref32, floor):
    """print (e32, gate, measured) for one tensor and assert measured <= gate"""
    assert bool(torch.isfinite(got).all()), (kernel, case, name, 'not finite')
    e32 = rel_l2(ref32, ref64)
    g = gate(floor, e32)
    err = rel_l2(got, ref64)
    print('%s | %s | %s: e32 %.3e gate %.3e measured %.3e' % (kernel, case, name, e32, g, err))
    assert err <= g, (kernel, case, name, e32, g, err)


def sum_error(got, ref64, terms64):
    """largest error of a per-channel sum in units of its channel's sum |terms|"""
    return float(((got.double() - ref64).abs() / (terms64 + 1e-300)).max())


def check_sum_gate(kernel, case, name, got, ref64, ref32, terms64, floor):
    assert bool(torch.isfinite(got).all()), (kernel, case, name, 'not finite')
    e32 = sum_error(ref32.cpu(), ref64, terms64)
    g = gate(floor, e32)
    err = sum_error(got.cpu(), ref64, terms64)
    print('%s | %s | %s: e32 %.3e gate %.3e measured %.3e' % (kernel, case, name, e32, g, err))
    assert err <= g, (kernel, case, name, e32, g, err)


def bits(t):
    """the tensor's bytes as integers (NaN sentinels compare equal, -0.0 differs from 0.0)"""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def split_planes_reference(x, relu):
    """(hi, lo) bf16 of conv_planes.hip: hi = bf16(x) round-to-nearest-even, lo = bf16(x - hi); relu splits max(x, 0)"""
    v = x.detach().cpu().float().flatten()
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    hi = v.bfloat16()
    return hi, (v - hi.float()).bfloat16()


# ------------------------------------------------------------------------------------------ launch geometry, restated
def ppb_for(npos, Cp, images, target):
    CH = min(Cp, 64)
    per_iter = 1024 // CH
    slices = max(target // (images * (Cp // CH)), 1)
    ppb = max(-(-npos // slices), 4 * per_iter)
    return -(-ppb // per_iter) * per_iter


def zchunks(Cp):
    return 1 if Cp < 64 else Cp // 64


def slice_geometry(npos, Cp, images, target):
    """(positions per block, blocks along the positions, positions of the last block)"""
    ppb = ppb_for(npos, Cp, images, target)
    blocks = -(-npos // ppb)
    return ppb, blocks, npos - (blocks - 1) * ppb


def pstep(Cp):
    return 256 // (min(Cp, 64) // 4)


def bn_grid(rows, C):
    """(row blocks, channel chunks, rows per block)"""
    CH = min(C, 64)
    chunks = C // CH
    rpb = max(-(-rows // max(2048 // chunks, 1)), 256)
    return -(-rows // rpb), chunks, rpb


# ------------------------------------------------------------------------------------------ InstanceNorm
# name: N, C, Cp, HW; the sdn_in_apply arguments of the case (act, res: None | res_relu, planes: None | planes_relu, running
# statistics or NULL); `apply` / `reduce`: (ppb, blocks, last-block positions) at the targets 4096 / 1024, asserted by the host test
IN_CASES = {
    'ppb_floor_16_blocks_last_40': dict(N=2, C=64, Cp=64, HW=1000, act=0, res=None, planes=None, running=True,
                                        apply=(64, 16, 40), reduce=(64, 16, 40)),
    'chunks_16_reduce_80x63_apply_64x79_last_8': dict(N=1, C=1024, Cp=1024, HW=5000, act=1, res=1, planes=0, running=False,
                                                      apply=(64, 79, 8), reduce=(80, 63, 40)),
    'c4n_4_pstep_64_last_188': dict(N=3, C=3, Cp=16, HW=700, act=1, res=None, planes=0, running=True,
                                    apply=(256, 3, 188), reduce=(256, 3, 188)),
    'last_2_below_pstep': dict(N=5, C=20, Cp=32, HW=130, act=0, res=0, planes=None, running=True,
                               apply=(128, 2, 2), reduce=(128, 2, 2)),
    'chunks_4_two_blocks_last_13': dict(N=4, C=136, Cp=256, HW=77, act=0, res=None, planes=1, running=True,
                                        apply=(64, 2, 13), reduce=(64, 2, 13)),
    'hw_2': dict(N=2, C=128, Cp=128, HW=2, act=1, res=0, planes=1, running=True, apply=(64, 1, 2), reduce=(64, 1, 2)),
    'hw_1': dict(N=2, C=128, Cp=128, HW=1, act=0, res=1, planes=0, running=True, apply=(64, 1, 1), reduce=(64, 1, 1)),
}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def _leaky(x):
    return torch.where(x > 0, x, 0.2 * x)


def _relu(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def instance_norm(x):
    """nn.InstanceNorm2d(affine=False) of channels-last x [N, HW, C]: (xhat, mean [N, 1, C], biased var, rstd)"""
    HW = x.shape[1]
    mean = x.sum(dim=1, keepdim=True) / HW
    d = x - mean
    var = (d * d).sum(dim=1, keepdim=True) / HW
    rstd = 1.0 / torch.sqrt(var + EPS)
    return d * rstd, mean, var, rstd


@functools.lru_cache(maxsize=None)
def _in_apply_inputs(name):
    c = IN_CASES[name]
    N, C, Cp, HW = c['N'], c['C'], c['Cp'], c['HW']
    g = torch.Generator().manual_seed(8100 + _seed(name))
    z = torch.zeros(N, HW, Cp)
    z[..., :C] = torch.randn(N, HW, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + (torch.rand(C, generator=g) * 2 - 1)
    res = torch.zeros(N, HW, Cp)
    res[..., :C] = torch.randn(N, HW, C, generator=g)
    # every position goes to one of the SDN_STAT_SLOTS copies; all copies are used once there are that many positions
    slot = torch.stack([(torch.randperm(HW, generator=g) + int(torch.randint(0, 8, (1,), generator=g))) % STAT_SLOTS for _ in range(N)])
    if HW >= 64:
        slot = torch.where(torch.rand(N, HW, generator=g) < 0.5, slot, torch.randint(0, STAT_SLOTS, (N, HW), generator=g))
    rm0 = torch.rand(C, generator=g) - 0.5
    rv0 = torch.rand(C, generator=g) + 0.5
    return z, res, slot, rm0, rv0


def in_apply_inputs(name):
    """(z [N, HW, Cp], res, slot [N, HW], running_mean, running_var): fresh clones; the pad channels of z and res are zero"""
    return tuple(t.clone() for t in _in_apply_inputs(name))


def in_stats(z, slot):
    """stats [N, SDN_STAT_SLOTS, Cp, 2] float64: the sums and sums of squares of z, each position added to its slot's copy"""
    N, HW, Cp = z.shape
    zd = z.double()
    st = torch.zeros(N, STAT_SLOTS, Cp, 2, dtype=torch.float64)
    for n in range(N):
        st[n, :, :, 0].index_add_(0, slot[n], zd[n])
        st[n, :, :, 1].index_add_(0, slot[n], zd[n] * zd[n])
    return st


def in_apply_reference(z, res, C, act, res_relu, rm0, rv0, dtype):
    """dict: y (what the call leaves in z), out2 (y + f(res)), mr [N, Cp, 2], running_mean / running_var [C] after the update.
    For HW == 1 the variance is 0, y is 0 and the unbiased variance is the biased one (the kernel's rule)."""
    x = z.to(dtype)
    N, HW, Cp = x.shape
    xhat, mean, var, rstd = instance_norm(x)
    y = _leaky(xhat) if act == 1 else xhat
    r = res.to(dtype)
    out2 = y + (_relu(r) if res_relu else r)
    unbiased = var * (HW / (HW - 1.0)) if HW > 1 else var
    rm = (1 - MOMENTUM) * rm0.to(dtype) + MOMENTUM * mean[:, 0, :C].sum(dim=0) / N
    rv = (1 - MOMENTUM) * rv0.to(dtype) + MOMENTUM * unbiased[:, 0, :C].sum(dim=0) / N
    return dict(y=y, out2=out2, mr=torch.stack((mean[:, 0], rstd[:, 0]), dim=2), rm=rm, rv=rv)


@functools.lru_cache(maxsize=None)
def _in_bwd_inputs(name):
    c = IN_CASES[name]
    N, C, Cp, HW = c['N'], c['C'], c['Cp'], c['HW']
    g = torch.Generator().manual_seed(8200 + _seed(name))
    half = HW // 2
    q = torch.zeros(N, HW, C)
    a = torch.round(torch.randn(N, half, C, generator=g) * 384.0)
    a = torch.where(torch.rand(N, half, C, generator=g) < 0.03, torch.zeros_like(a), a)     # planted zeros, in pairs
    if half >= 2:
        a[:, 0] = 0                                                                          # at least one per (image, channel)
    q[:, 0:2 * half:2] = a
    q[:, 1:2 * half:2] = -a                                                                  # (an odd HW leaves q = 0 last)
    q = q[:, torch.randperm(HW, generator=g)]
    mu = torch.randint(-4, 5, (C,), generator=g).float() / 4
    z = torch.zeros(N, HW, Cp)
    z[..., :C] = mu + q / 256.0
    xhat = instance_norm(z.double())[0]
    up = torch.zeros(N, HW, Cp)
    up[..., :C] = (0.3 + 0.5 * xhat[..., :C] + torch.randn(N, HW, C, dtype=torch.float64, generator=g)).float()
    return z, up


def in_bwd_inputs(name):
    """(z, g): quantised z (module docstring) and an upstream gradient with a non-zero mean and a non-zero correlation with xhat,
    so that both reductions of the backward matter; pad channels zero"""
    return tuple(t.clone() for t in _in_bwd_inputs(name))


def in_bwd_reference(z, g, mode, dtype):
    """autograd through the written-out InstanceNorm + activation (mode 0 none, 1 ReLU applied by the consumers, 2 LeakyReLU):
    dict dz, sums [N, Cp, 2] = (sum g_eff, sum g_eff xhat), stored (what the forward kept: xhat, or LeakyReLU(xhat) in mode 2),
    mr [N, Cp, 2]"""
    x = z.to(dtype).clone().requires_grad_(True)
    xhat, mean, _, rstd = instance_norm(x)
    y = _relu(xhat) if mode == 1 else _leaky(xhat) if mode == 2 else xhat
    up = g.to(dtype)
    (y * up).sum().backward()
    xh = xhat.detach()
    slope = {0: torch.ones_like(xh), 1: (xh > 0).to(dtype), 2: torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, 0.2))}
    ge = up * slope[mode]
    sums = torch.stack((ge.sum(dim=1), (ge * xh).sum(dim=1)), dim=2)
    stored = _leaky(xh) if mode == 2 else xh
    return dict(dz=x.grad, sums=sums, stored=stored, mr=torch.stack((mean.detach()[:, 0], rstd.detach()[:, 0]), dim=2))


# ------------------------------------------------------------------------------------------ activation backward
# name: npos, Cp and the (ppb, blocks, last) of the launch with / without bias_grad (targets 1024 / 4096)
ACT_SHAPES = {
    'npos_70000_cp_64': dict(npos=70000, Cp=64, with_bias=(80, 875, 80), without=(64, 1094, 48)),
    'npos_3_cp_16': dict(npos=3, Cp=16, with_bias=(256, 1, 3), without=(256, 1, 3)),
    'npos_1000_cp_512': dict(npos=1000, Cp=512, with_bias=(64, 16, 40), without=(64, 16, 40)),
}


@functools.lru_cache(maxsize=None)
def _act_inputs(shape, act):
    c = ACT_SHAPES[shape]
    gen = torch.Generator().manual_seed(8300 + 10 * _seed(shape) + act)
    npos, Cp = c['npos'], c['Cp']
    pre = torch.randn(npos, Cp, generator=gen)
    pre = torch.where(torch.rand(npos, Cp, generator=gen) < 0.03, torch.zeros_like(pre), pre)   # the kink of act 1 and 3
    y = _leaky(pre) if act == 1 else torch.tanh(pre * 1.5) if act == 2 else pre
    g = torch.randn(npos, Cp, generator=gen) + 0.3
    bias0 = torch.randn(Cp, generator=gen)
    return g, y, bias0


def act_inputs(shape, act):
    """(g, y, bias_grad before the call): y = LeakyReLU(pre) (act 1), tanh(pre) (act 2) or the stored pre-activation (act 0, 3),
    with exact zeros planted"""
    return tuple(t.clone() for t in _act_inputs(shape, act))


def act_bwd_reference(g, y, act, dtype):
    """(dz, sum over the positions, sum of |dz| over the positions)"""
    g, y = g.to(dtype), y.to(dtype)
    if act == 1:
        dz = torch.where(y > 0, g, 0.2 * g)
    elif act == 2:
        dz = g * (1 - y * y)
    elif act == 3:
        dz = torch.where(y > 0, g, torch.zeros_like(g))
    else:
        dz = g
    return dz, dz.sum(dim=0), dz.abs().sum(dim=0)


# ------------------------------------------------------------------------------------------ reflection fold
# name: N, H, W, Cp, pad
FOLD_CASES = {
    'pad1_2x2_smallest': (2, 2, 2, 4, 1),
    'pad1_3x3_mirrored_from_both_sides': (1, 3, 3, 64, 1),
    'pad3_4x4_smallest_3x3_terms': (2, 4, 4, 4, 3),
    'pad3_4x9_mixed': (1, 4, 9, 64, 3),
    'pad1_5x7_no_double_mirror': (3, 5, 7, 4, 1),
    'pad3_9x11_no_double_mirror_uneven_blocks': (2, 9, 11, 64, 3),     # 3168 threads = 12.375 blocks
}


def fold_inputs(name):
    N, H, W, Cp, pad = FOLD_CASES[name]
    g = torch.Generator().manual_seed(8400 + _seed(name))
    return torch.randn(N, H + 2 * pad, W + 2 * pad, Cp, generator=g), torch.randn(N, H, W, Cp, generator=g)


def reflect_index(n, pad):
    """source index in [0, n) of every padded index of nn.ReflectionPad2d(pad)"""
    i = (torch.arange(-pad, n + pad)).abs()
    return torch.where(i > n - 1, 2 * (n - 1) - i, i)


def reflect_fold_reference(gp, pad, base, dtype):
    """the adjoint of ReflectionPad2d on channels-last gp [N, H + 2 pad, W + 2 pad, Cp]; `base` is added (accumulate)"""
    N, Hp, Wp, Cp = gp.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    t = torch.zeros(N, H, Wp, Cp, dtype=dtype).index_add_(1, reflect_index(H, pad), gp.to(dtype))
    out = torch.zeros(N, H, W, Cp, dtype=dtype).index_add_(2, reflect_index(W, pad), t)
    return out if base is None else out + base.to(dtype)


def fold_interior(H, W, pad):
    """[H, W] bool: the positions no padded position mirrors onto"""
    one = torch.ones(1, H + 2 * pad, W + 2 * pad, 1, dtype=torch.float64)
    return reflect_fold_reference(one, pad, None, torch.float64)[0, :, :, 0] == 1


# ------------------------------------------------------------------------------------------ weight pack / gradient unpack
# A parameter is Conv2d [O, I, kh, kw] or ConvTranspose2d [I, O, kh, kw]; `rows` names which of O / I indexes the matrix rows.
# name: layer, O, I, kh, kw, rows, taps ('all' or (ky, kx) pairs), Ccp, Kp, matrix rows of the fragment pack
PACK_CASES = {
    'tap_major_ccp16_kp_padded_r24_c13': dict(layer='conv', O=24, I=13, k=(3, 3), rows='O', taps='all', Ccp=16, Kp=160, prows=32),
    'tap_major_ccp48_convT_phase_taps': dict(layer='convT', O=40, I=45, k=(4, 4), rows='O', taps=((1, 1), (1, 3), (3, 1), (3, 3)),
                                             Ccp=48, Kp=224, prows=64),
    'tap_major_ccp32_kp_padded_data_grad': dict(layer='conv', O=20, I=33, k=(3, 3), rows='I', taps='all', Ccp=32, Kp=352, prows=64),
    'block_major_ccp32_r33_c20': dict(layer='conv', O=33, I=20, k=(3, 3), rows='O', taps='all', Ccp=32, Kp=288, prows=64),
    'block_major_ccp64_convT_phase_taps': dict(layer='convT', O=70, I=61, k=(4, 4), rows='O', taps=((0, 0), (0, 2), (2, 0), (2, 2)),
                                               Ccp=64, Kp=256, prows=96),
}
# the K-major pack: Ccp % 32 == 0, rows % 64 == 0
KMAJOR_CASES = {
    'kmajor_ccp32_r33_c20': dict(layer='conv', O=33, I=20, k=(3, 3), rows='O', taps='all', Ccp=32, prows=64),
    'kmajor_ccp64_convT_phase_taps': dict(layer='convT', O=70, I=61, k=(4, 4), rows='O', taps=((0, 0), (0, 2), (2, 0), (2, 2)),
                                          Ccp=64, prows=128),
    'kmajor_ccp32_data_grad': dict(layer='conv', O=20, I=33, k=(3, 3), rows='I', taps='all', Ccp=32, prows=64),
}
# name: ..., accumulate, and the kernel the launcher picks: 'rows' (LDS transpose: sc <= 64, ntaps <= 64, sc < sr) or 'group4'
UNPACK_CASES = {
    'rows_c65_3x3': dict(layer='conv', O=5, I=65, k=(3, 3), rows='O', taps='all', Ccp=80, accumulate=0, kernel='rows'),
    'rows_c130_49_taps_accumulate': dict(layer='conv', O=3, I=130, k=(7, 7), rows='O', taps='all', Ccp=144, accumulate=1, kernel='rows'),
    'rows_convT_partial_taps': dict(layer='convT', O=65, I=4, k=(3, 3), rows='I', taps=((0, 0), (0, 2), (2, 0), (2, 2)), Ccp=80,
                                    accumulate=0, kernel='rows'),
    'rows_partial_taps_accumulate': dict(layer='conv', O=4, I=65, k=(4, 4), rows='O', taps=((1, 1), (1, 3), (3, 1), (3, 3)), Ccp=80,
                                         accumulate=1, kernel='rows'),
    'group4_81_taps_c6': dict(layer='conv', O=2, I=6, k=(9, 9), rows='O', taps='all', Ccp=16, accumulate=0, kernel='group4'),
    'group4_sc_above_sr_accumulate': dict(layer='conv', O=65, I=7, k=(3, 3), rows='I', taps='all', Ccp=80, accumulate=1, kernel='group4'),
    'group4_sc_above_sr_partial_taps': dict(layer='conv', O=130, I=3, k=(3, 3), rows='I', taps=((0, 1), (1, 0), (1, 2), (2, 1)), Ccp=144,
                                            accumulate=0, kernel='group4'),
    # 257 rows x 1 tap x 4 padded columns = 1028 elements: one element group past a 1024-element block
    'group4_1028_elements': dict(layer='conv', O=3, I=257, k=(1, 1), rows='I', taps='all', Ccp=4, accumulate=0, kernel='group4'),
}


def weight_layout(c):
    """(parameter shape, R, C, sr, sc, tapidx list) of a case: element (r, c, tap) of the matrix is w.flatten()[r sr + c sc + tapidx]"""
    O, I, (kh, kw) = c['O'], c['I'], c['k']
    taps = [(ky, kx) for ky in range(kh) for kx in range(kw)] if c['taps'] == 'all' else list(c['taps'])
    tapidx = [ky * kw + kx for ky, kx in taps]
    shape = (O, I, kh, kw) if c['layer'] == 'conv' else (I, O, kh, kw)
    s_first, s_second = shape[1] * kh * kw, kh * kw
    o_stride, i_stride = (s_first, s_second) if c['layer'] == 'conv' else (s_second, s_first)
    if c['rows'] == 'O':
        return shape, O, I, o_stride, i_stride, tapidx
    return shape, I, O, i_stride, o_stride, tapidx


def unpack_kernel(sr, sc, ntaps):
    """which kernel sdn_conv_unpack_grad launches (restated from its launcher)"""
    return 'rows' if (1 <= sc <= 64 and ntaps <= 64 and sc < sr) else 'group4'


def weight_inputs(name, c, extra=0):
    g = torch.Generator().manual_seed(8500 + _seed(name) + extra)
    return torch.randn(weight_layout(c)[0], generator=g)


def logical_matrix(w, R, C, sr, sc, tapidx, Ccp, Kp, rows, block_major):
    """Wm [rows, Kp] of include/sdn_hip.h: Wm[r, k] = w[r sr + c sc + tapidx[t]] with k = t Ccp + c, or, channel-block-major,
    k = ((c / 32) ntaps + t) 32 + c % 32; zero where r >= R, c >= C or k lies in the K padding"""
    ntaps = len(tapidx)
    r = torch.arange(rows)[:, None]
    k = torch.arange(Kp)[None, :]
    if block_major:
        step = k // 32
        cb = step // ntaps
        t, c = step - cb * ntaps, cb * 32 + k % 32
    else:
        t, c = k // Ccp, k % Ccp
    valid = (r < R) & (t < ntaps) & (c < C)
    tap = torch.tensor(tapidx)[t.clamp(max=ntaps - 1)]
    src = (r * sr + c * sc + tap).clamp(0, w.numel() - 1)
    return torch.where(valid, w.flatten()[src], torch.zeros(()))


def fragment_index(rows, Kp):
    """[rows, Kp] index of the hi element of Wm[r, k] in the fragment-ordered buffer; its lo element lies 512 further"""
    r = torch.arange(rows)[:, None]
    k = torch.arange(Kp)[None, :]
    return (((r // 32) * (Kp // 16) + k // 16) * 2) * 512 + (r % 32 + 32 * ((k % 16) // 8)) * 8 + k % 8


def pack_reference(w, R, C, sr, sc, tapidx, Ccp, Kp, rows):
    """the 2 rows Kp bf16 of sdn_conv_pack_weights"""
    Wm = logical_matrix(w, R, C, sr, sc, tapidx, Ccp, Kp, rows, Ccp % 32 == 0 and Kp == len(tapidx) * Ccp)
    hi = Wm.bfloat16()
    lo = (Wm - hi.float()).bfloat16()
    dst = fragment_index(rows, Kp)
    out = torch.full((2 * rows * Kp,), NAN, dtype=torch.bfloat16)
    out[dst.flatten()] = hi.flatten()
    out[(dst + 512).flatten()] = lo.flatten()
    return out, Wm


def kmajor_index(rows, K, ntaps):
    """index of the hi element of Wm[r, k] in packed[r][step][part][32]; lo lies 32 further"""
    r = torch.arange(rows)[:, None]
    k = torch.arange(K)[None, :]
    return (r * (K // 32) + k // 32) * 64 + k % 32


def pack_kmajor_reference(w, R, C, sr, sc, tapidx, Ccp, rows):
    """the 2 rows ntaps Ccp bf16 of sdn_conv_pack_weights_kmajor (always channel-block-major)"""
    K = len(tapidx) * Ccp
    Wm = logical_matrix(w, R, C, sr, sc, tapidx, Ccp, K, rows, True)
    hi = Wm.bfloat16()
    lo = (Wm - hi.float()).bfloat16()
    dst = kmajor_index(rows, K, len(tapidx))
    out = torch.full((2 * rows * K,), NAN, dtype=torch.bfloat16)
    out[dst.flatten()] = hi.flatten()
    out[(dst + 32).flatten()] = lo.flatten()
    return out, Wm


def unpack_index(R, C, sr, sc, tapidx):
    """[R, ntaps, C] flat index into the parameter gradient of dw[r, t Ccp + c]"""
    r = torch.arange(R)[:, None, None]
    t = torch.tensor(tapidx)[None, :, None]
    c = torch.arange(C)[None, None, :]
    return r * sr + c * sc + t


def unpack_reference(dw, R, C, sr, sc, tapidx, Ccp, base, accumulate):
    """grad_w (+)= dw through the inverse map, in float32 (one add at most per element: exact); `base` is what grad_w held"""
    idx = unpack_index(R, C, sr, sc, tapidx).flatten()
    vals = dw.reshape(R, len(tapidx), Ccp)[:, :, :C].flatten()
    out = base.clone().flatten()
    out[idx] = out[idx] + vals if accumulate else vals
    return out.reshape(base.shape)


# ------------------------------------------------------------------------------------------ program records
ADD_N4 = (1, 1023, 8192 * 1024 + 1023)       # float4 counts; the last one enters the grid-stride loop of k_add (134 MB a buffer)
COLSUM_ROWS = (1, 255, 70000)
COLSUM_COLS = ((3, 16), (64, 64))            # (C, pitch)


def ulp32(x):
    """spacing of float32 at |x| (x float32)"""
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float('inf'))) - x).double()


# ------------------------------------------------------------------------------------------ BatchNorm
BN_BIG_ROWS = 2048 * 256 + 777
# name: rows, C, training, res, relu, affine (gamma / beta present), running statistics present; grid = (row blocks, chunks, rpb)
BN_CASES = {
    'c4_rows_2_c4n_1': dict(rows=2, C=4, training=1, res=0, relu=0, affine=1, running=1, grid=(1, 1, 256)),
    'c4_rows_495_c4n_1_res_relu': dict(rows=495, C=4, training=1, res=1, relu=1, affine=1, running=1, grid=(2, 1, 256)),
    'c4_rows_257_eval_c4n_1': dict(rows=257, C=4, training=0, res=1, relu=0, affine=1, running=1, grid=(2, 1, 256)),
    'c8_rows_255_eval': dict(rows=255, C=8, training=0, res=0, relu=1, affine=1, running=1, grid=(1, 1, 256)),
    'c8_rows_1_train_formula_only': dict(rows=1, C=8, training=1, res=0, relu=0, affine=1, running=1, grid=(1, 1, 256)),
    'c32_rows_257_second_block_of_one_row': dict(rows=257, C=32, training=1, res=1, relu=1, affine=1, running=1, grid=(2, 1, 256)),
    'c32_rows_495_eval_res': dict(rows=495, C=32, training=0, res=1, relu=0, affine=0, running=1, grid=(2, 1, 256)),
    'c64_rows_495_no_running': dict(rows=495, C=64, training=1, res=0, relu=1, affine=1, running=0, grid=(2, 1, 256)),
    'c64_rows_2_eval_res_relu': dict(rows=2, C=64, training=0, res=1, relu=1, affine=1, running=1, grid=(1, 1, 256)),
    'c128_rows_257_two_chunks_no_affine': dict(rows=257, C=128, training=1, res=1, relu=0, affine=0, running=1, grid=(2, 2, 256)),
    'c128_rows_255_eval_relu': dict(rows=255, C=128, training=0, res=0, relu=1, affine=1, running=1, grid=(1, 2, 256)),
    'c512_rows_495_eight_chunks': dict(rows=495, C=512, training=1, res=1, relu=1, affine=1, running=1, grid=(2, 8, 256)),
    'c512_rows_2_eval': dict(rows=2, C=512, training=0, res=0, relu=0, affine=1, running=1, grid=(1, 8, 256)),
    'c64_stem_rows_per_block_257': dict(rows=BN_BIG_ROWS, C=64, training=1, res=1, relu=1, affine=1, running=1, grid=(2044, 1, 257)),
}


def bn_inputs(name):
    """dict x [rows, C] (mean 3, standard deviation 0.5: the conditioning the stem sees), res, g, gamma, beta, rm0, rv0"""
    c = BN_CASES[name]
    rows, C = c['rows'], c['C']
    gen = torch.Generator().manual_seed(8600 + _seed(name))
    x = torch.randn(rows, C, generator=gen) * 0.5 + 3.0
    d = dict(x=x, res=torch.randn(rows, C, generator=gen) if c['res'] else None)
    d['g'] = torch.randn(rows, C, generator=gen) + 0.3 + 0.5 * (x - 3.0) / 0.5
    d['gamma'] = torch.rand(C, generator=gen) + 0.5 if c['affine'] else None
    d['beta'] = torch.randn(C, generator=gen) if c['affine'] else None
    d['rm0'] = 3.0 + 0.2 * torch.randn(C, generator=gen)
    d['rv0'] = 0.25 + 0.1 * torch.rand(C, generator=gen)
    return d


def bn_forward_reference(d, training, relu, dtype):
    """nn.BatchNorm2d (+ residual, + ReLU) on [rows, C]: dict out, mr [C, 2], ss [C, 2] = (scale, shift), rm, rv.
    One row in training: variance 0 and the unbiased variance is the biased one (the kernel's rule; torch refuses)."""
    x = d['x'].to(dtype)
    rows, C = x.shape
    one, zero = torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype)
    gamma = d['gamma'].to(dtype) if d['gamma'] is not None else one
    beta = d['beta'].to(dtype) if d['beta'] is not None else zero
    rm, rv = d['rm0'].to(dtype), d['rv0'].to(dtype)
    if training:
        mean = x.sum(dim=0) / rows
        xc = x - mean
        var = (xc * xc).sum(dim=0) / rows
        unbiased = var * (rows / (rows - 1.0)) if rows > 1 else var
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * unbiased
    else:
        mean, var = rm, rv
        xc = x - mean
    rstd = 1.0 / torch.sqrt(var + EPS)
    out = xc * (rstd * gamma) + beta
    if d['res'] is not None:
        out = out + d['res'].to(dtype)
    if relu:
        out = _relu(out)
    scale = gamma * rstd
    return dict(out=out, mr=torch.stack((mean, rstd), dim=1), ss=torch.stack((scale, beta - mean * scale), dim=1), rm=rm, rv=rv)


def bn_backward_reference(d, out32, mr, training, relu, dtype):
    """closed form of the backward: gm = g masked by the float32 `out` the forward stored (the mask is data, the same in every
    precision), sums [C, 2] = (sum gm, sum gm xhat) = (d beta, d gamma), dx.  mr [C, 2] = (mean, rstd) in `dtype`."""
    x, g = d['x'].to(dtype), d['g'].to(dtype)
    rows, C = x.shape
    gamma = d['gamma'].to(dtype) if d['gamma'] is not None else torch.ones(C, dtype=dtype)
    gm = torch.where(out32 > 0, g, torch.zeros_like(g)) if relu else g
    xhat = (x - mr[:, 0]) * mr[:, 1]
    s0, s1 = gm.sum(dim=0), (gm * xhat).sum(dim=0)
    k = gamma * mr[:, 1]
    dx = k * (gm - s0 / rows - xhat * (s1 / rows)) if training else k * gm
    return dict(gm=gm, sums=torch.stack((s0, s1), dim=1), dx=dx)


# ------------------------------------------------------------------------------------------ pools
# name: N, H, W, C
MAXPOOL_SHAPES = {
    'h1_w1_c4': (1, 1, 1, 4),
    'h1_w7_c4': (2, 1, 7, 4),
    'h2_w2_c8': (1, 2, 2, 8),
    'h7_w2_c4': (1, 7, 2, 4),
    'h8_w6_c16': (2, 8, 6, 16),
    'h9_w10_c64_uneven_blocks': (2, 9, 10, 64),      # 800 output threads = 3.125 blocks, 2880 input threads = 11.25
}
MAXPOOL_INPUTS = ('relu_ties', 'neg_inf_window', 'nan')


def maxpool_inputs(shape, kind):
    N, H, W, C = MAXPOOL_SHAPES[shape]
    gen = torch.Generator().manual_seed(8700 + _seed(shape) + len(kind))
    x = torch.randn(N, H, W, C, generator=gen)
    if kind == 'relu_ties':
        x = _relu(x)                                     # half of the values are equal zeros
    elif kind == 'neg_inf_window':
        x[:, :min(H, 3), :min(W, 3)] = float('-inf')     # the first window(s) hold nothing else
        x[0, H // 2, W // 2, 0] = float('-inf')
    else:
        x = torch.where(torch.rand(N, H, W, C, generator=gen) < 0.04, torch.full_like(x, NAN), x)
        x[0, 0, 0, 0] = NAN
    g = torch.randn(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, generator=gen)
    return x, g


def _pool_taps(H, W):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for ky in range(3):
        iy = 2 * torch.arange(OH) - 1 + ky
        for kx in range(3):
            ix = 2 * torch.arange(OW) - 1 + kx
            valid = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            yield ky * 3 + kx, iy.clamp(0, H - 1), ix.clamp(0, W - 1), valid


def maxpool_reference(x):
    """MaxPool2d(3, 2, 1) on channels-last x [N, H, W, C]: (out, idx int8 = ky * 3 + kx, window-holds-a-NaN mask).  Scan order ky,
    kx; a tap replaces the best so far when it is larger, when it is the first inside the image, or when it is NaN (ATen's
    `val > maxval || isnan(val)` with the window's first element as the start)."""
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = torch.full((N, OH, OW, C), float('-inf'), dtype=x.dtype)
    bi = torch.full((N, OH, OW, C), -1, dtype=torch.int8)
    has_nan = torch.zeros(N, OH, OW, C, dtype=torch.bool)
    for tap, iy, ix, valid in _pool_taps(H, W):
        v = x[:, iy][:, :, ix]
        ok = valid[None, :, :, None]
        upd = ok & ((v > best) | (bi < 0) | torch.isnan(v))
        best = torch.where(upd, v, best)
        bi = torch.where(upd, torch.full_like(bi, tap), bi)
        has_nan |= ok & torch.isnan(v)
    return best, bi, has_nan


def maxpool_flat_index(idx, H, W):
    """iy * W + ix of the routed input, the form F.max_pool2d returns"""
    N, OH, OW, C = idx.shape
    ky, kx = (idx // 3).long(), (idx % 3).long()
    iy = 2 * torch.arange(OH)[None, :, None, None] - 1 + ky
    ix = 2 * torch.arange(OW)[None, None, :, None] - 1 + kx
    return iy * W + ix


def maxpool_bwd_reference(g, idx, H, W, dtype):
    """(gin [N, H, W, C], number of windows routed to each input)"""
    N, OH, OW, C = g.shape
    flat = maxpool_flat_index(idx, H, W).reshape(N, OH * OW, C)
    gin = torch.zeros(N, H * W, C, dtype=dtype).scatter_add_(1, flat, g.to(dtype).reshape(N, OH * OW, C))
    cnt = torch.zeros(N, H * W, C, dtype=torch.int64).scatter_add_(1, flat, torch.ones(N, OH * OW, C, dtype=torch.int64))
    return gin.reshape(N, H, W, C), cnt.reshape(N, H, W, C)


# name: N, HW, C
AVGPOOL_CASES = {
    'hw_1_c8': (1, 1, 8),
    'hw_7_c4': (2, 7, 4),
    'hw_468_384_threads': (3, 468, 512),     # N * C / 4 = 384: two blocks, the second half full
}


def avgpool_inputs(name):
    N, HW, C = AVGPOOL_CASES[name]
    gen = torch.Generator().manual_seed(8800 + _seed(name))
    return torch.randn(N, HW, C, generator=gen) + 0.5, torch.randn(N, C, generator=gen)


def avgpool_reference(x, dtype):
    """mean over the positions; in float32 as an explicitly sequential sum, the kernel's order"""
    N, HW, C = x.shape
    if dtype == torch.float64:
        return x.double().sum(dim=1) / HW
    s = torch.zeros(N, C)
    for p in range(HW):
        s = s + x[:, p]
    return s * torch.tensor(1.0 / HW, dtype=torch.float32)


def avgpool_bwd_reference(g, HW, dtype):
    return (g.to(dtype) / HW)[:, None, :].expand(-1, HW, -1)
