"""What tests/test_gpu_conv_companions.py takes for granted, checked without a GPU.  First: the float64 references of
tests/conv_companions_util.py agree with torch's own operators -- F.instance_norm with running statistics, F.batch_norm, autograd of
F.pad(mode='reflect'), F.max_pool2d with indices, autograd of relu / leaky_relu / tanh -- so that a wrong reference cannot pass a
wrong kernel (torch refuses HW = 1 for InstanceNorm and one row for BatchNorm in training: those two are formula only).  Second:
under the launch geometry restated in the util module every named case has the block count, positions per block and last-block
fill its name claims; if this fails after a change of the launch code, pick new cases."""
import pytest
import torch
import torch.nn.functional as F

import conv_companions_util as u

F64 = torch.float64


def close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


# ------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize('name', list(u.IN_CASES))
def test_instance_norm_cases_reach_their_named_geometry(name):
    c = u.IN_CASES[name]
    assert u.slice_geometry(c['HW'], c['Cp'], c['N'], 4096) == c['apply']
    assert u.slice_geometry(c['HW'], c['Cp'], c['N'], 1024) == c['reduce']
    assert c['C'] <= c['Cp'] and c['Cp'] in (16, 32, 64, 128, 256, 512, 1024)
    if name == 'ppb_floor_16_blocks_last_40':
        assert u.pstep(c['Cp']) == 16 and c['apply'][2] / u.pstep(c['Cp']) == 2.5      # 2.5 iterations in the last block
    if name.startswith('chunks_16'):
        assert u.zchunks(c['Cp']) == 16 and c['apply'] != c['reduce'] and c['N'] * c['HW'] * c['Cp'] * 4 == 20480000
    if name.startswith('c4n_4'):
        assert min(c['Cp'], 64) // 4 == 4 and u.pstep(c['Cp']) == 64
    if name == 'last_2_below_pstep':
        assert c['apply'][2] < u.pstep(c['Cp'])
    if name.startswith('chunks_4'):
        assert u.zchunks(c['Cp']) == 4


def test_instance_norm_cases_cover_the_argument_combinations():
    cs = list(u.IN_CASES.values())
    assert {(c['C'], c['Cp']) for c in cs} >= {(3, 16), (20, 32), (136, 256)}
    assert {c['act'] for c in cs} == {0, 1}
    assert {c['res'] for c in cs} == {None, 0, 1}
    assert {c['planes'] for c in cs} == {None, 0, 1}
    assert {(c['res'] is not None, c['planes'] is not None) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c['running'] for c in cs} == {True, False}
    assert {c['HW'] for c in cs} >= {1, 2}


@pytest.mark.parametrize('name', list(u.ACT_SHAPES))
def test_activation_backward_shapes_reach_their_named_geometry(name):
    c = u.ACT_SHAPES[name]
    assert u.slice_geometry(c['npos'], c['Cp'], 1, 1024) == c['with_bias']
    assert u.slice_geometry(c['npos'], c['Cp'], 1, 4096) == c['without']
    if name == 'npos_70000_cp_64':
        assert c['with_bias'][0] != c['without'][0]


@pytest.mark.parametrize('name', list(u.BN_CASES))
def test_batch_norm_cases_reach_their_named_grid(name):
    c = u.BN_CASES[name]
    assert u.bn_grid(c['rows'], c['C']) == c['grid']
    if 'second_block_of_one_row' in name:
        assert c['rows'] - c['grid'][2] == 1
    if name == 'c64_stem_rows_per_block_257':
        assert c['grid'][2] > 256 and 134e6 < c['rows'] * c['C'] * 4 < 135e6


def test_batch_norm_cases_cover_the_argument_combinations():
    cs = list(u.BN_CASES.values())
    assert {c['C'] for c in cs} == {4, 8, 32, 64, 128, 512}
    for C in (4, 8, 32, 64, 128, 512):
        assert {c['training'] for c in cs if c['C'] == C} == {0, 1}, C
    assert {c['rows'] for c in cs} >= {2, 255, 257, 495}
    assert {(c['res'], c['relu']) for c in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(not c['affine'] for c in cs) and any(c['training'] and not c['running'] for c in cs)


# ------------------------------------------------------------------------------------------ InstanceNorm references
@pytest.mark.parametrize('name', list(u.IN_CASES))
def test_instance_norm_forward_reference_matches_torch(name):
    c = u.IN_CASES[name]
    z, res, slot, rm0, rv0 = u.in_apply_inputs(name)
    N, C, Cp, HW = c['N'], c['C'], c['Cp'], c['HW']
    assert float(z[..., C:].abs().max() if C < Cp else 0) == 0 and float(res[..., C:].abs().max() if C < Cp else 0) == 0
    st = u.in_stats(z, slot)
    assert close(st.sum(dim=1)[..., 0], z.double().sum(dim=1)) and close(st.sum(dim=1)[..., 1], (z.double() ** 2).sum(dim=1))
    used = [int((slot[n].bincount(minlength=u.STAT_SLOTS) > 0).sum()) for n in range(N)]
    assert used == [min(HW, u.STAT_SLOTS)] * N          # load_stats must add every copy
    ref = u.in_apply_reference(z, res, C, c['act'], c['res'] or 0, rm0, rv0, F64)
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all()), k
    if C < Cp:
        assert float(ref['y'][..., C:].abs().max()) == 0 and float(ref['out2'][..., C:].abs().max()) == 0
    if HW == 1:      # torch refuses one value per channel in training: the kernel's own rule, variance 0 and output 0
        assert float(ref['y'].abs().max()) == 0 and close(ref['mr'][..., 1], torch.full((N, Cp), 1e-5, dtype=F64) ** -0.5)
        assert close(ref['rv'], 0.9 * rv0.double())
        return
    x = z[..., :C].double().permute(0, 2, 1).contiguous()
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = F.instance_norm(x, rm, rv, use_input_stats=True, momentum=u.MOMENTUM, eps=u.EPS)
    if c['act'] == 1:
        y = F.leaky_relu(y, 0.2)
    y = y.permute(0, 2, 1)
    assert close(ref['y'][..., :C], y, 1e-11)
    r = res[..., :C].double()
    assert close(ref['out2'][..., :C], y + (F.relu(r) if c['res'] else r), 1e-11)
    assert close(ref['rm'], rm) and close(ref['rv'], rv)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', list(u.IN_CASES))
def test_instance_norm_backward_reference_matches_torch(name, mode):
    c = u.IN_CASES[name]
    N, C, Cp, HW = c['N'], c['C'], c['Cp'], c['HW']
    z, g = u.in_bwd_inputs(name)
    # the quantisation: every mean is exact in both precisions, so xhat == 0 exactly at the planted positions
    for dt in (torch.float32, F64):
        xhat, mean, _, _ = u.instance_norm(z.to(dt))
        assert torch.equal(mean[:, 0], mean[:1, 0].expand(N, Cp)) and torch.equal(mean * 4, torch.round(mean * 4)), dt
        zeros = (xhat[..., :C] == 0)
        assert torch.equal(zeros, z[..., :C].to(dt) == mean[..., :C])
    if HW >= 4:
        assert bool(zeros.any(dim=1).all())      # every (image, channel) holds a kink
    s32, s64 = u.instance_norm(z)[0], u.instance_norm(z.double())[0]
    assert torch.equal(torch.sign(s32), torch.sign(s64).float())
    assert float(g[..., :C].mean()) > 0.1 and float((g[..., :C].double() * s64[..., :C]).mean()) > 0.1 or HW == 1
    ref = u.in_bwd_reference(z, g, mode, F64)
    xh, rstd = u.instance_norm(z.double())[0], ref['mr'][..., 1][:, None, :]
    slope = {0: torch.ones_like(xh), 1: (xh > 0).double(), 2: torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, 0.2))}[mode]
    ge = g.double() * slope
    assert close(ref['dz'], rstd * (ge - ref['sums'][:, None, :, 0] / HW - xh * ref['sums'][:, None, :, 1] / HW), 1e-10)
    if HW == 1:
        assert float(ref['dz'].abs().max()) == 0
        return
    assert float(ref['dz'][..., C:].abs().max() if C < Cp else 0) == 0
    # torch's own operator on an input without exact kinks (its mean is not exact, so xhat == 0 does not survive it) ...
    z2 = u.in_apply_inputs(name)[0]
    x = z2[..., :C].double().permute(0, 2, 1).contiguous().requires_grad_(True)
    y = F.instance_norm(x, use_input_stats=True, eps=u.EPS)
    y = F.relu(y) if mode == 1 else F.leaky_relu(y, 0.2) if mode == 2 else y
    (y * g[..., :C].double().permute(0, 2, 1)).sum().backward()
    assert close(u.in_bwd_reference(z2, g, mode, F64)['dz'][..., :C], x.grad.permute(0, 2, 1), 1e-10)
    # ... and torch's rule at the kink itself: gradient 0 for ReLU, slope 0.2 for LeakyReLU
    k = torch.zeros(2, dtype=F64, requires_grad=True)
    (F.relu(k)[0] + F.leaky_relu(k, 0.2)[1]).backward()
    assert k.grad.tolist() == [0.0, 0.2]


@pytest.mark.parametrize('act', [0, 1, 2, 3])
def test_activation_backward_reference_matches_autograd(act):
    gen = torch.Generator().manual_seed(5)
    pre = torch.randn(300, 16, generator=gen).double()
    pre[::7] = 0.0
    pre.requires_grad_(True)
    g = torch.randn(300, 16, generator=gen).double()
    y = F.leaky_relu(pre, 0.2) if act == 1 else torch.tanh(pre) if act == 2 else F.relu(pre) if act == 3 else pre * 1.0
    (y * g).sum().backward()
    stored = pre.detach() if act in (0, 3) else y.detach()       # act 3 keeps the pre-activation
    dz, s, a = u.act_bwd_reference(g, stored, act, F64)
    assert close(dz, pre.grad) and close(s, pre.grad.sum(dim=0)) and close(a, pre.grad.abs().sum(dim=0))
    for shape in u.ACT_SHAPES:
        _, yy, _ = u.act_inputs(shape, act)
        assert act == 2 or bool((yy == 0).any())


# ------------------------------------------------------------------------------------------ reflection fold
@pytest.mark.parametrize('name', list(u.FOLD_CASES))
def test_reflect_fold_reference_is_the_gradient_of_reflection_padding(name):
    N, H, W, Cp, pad = u.FOLD_CASES[name]
    gp, base = u.fold_inputs(name)
    x = torch.zeros(N, Cp, H, W, dtype=F64, requires_grad=True)
    (F.pad(x, (pad, pad, pad, pad), mode='reflect') * gp.double().permute(0, 3, 1, 2)).sum().backward()
    assert close(u.reflect_fold_reference(gp, pad, None, F64), x.grad.permute(0, 2, 3, 1))
    assert close(u.reflect_fold_reference(gp, pad, base, F64), x.grad.permute(0, 2, 3, 1) + base.double())
    cnt = u.reflect_fold_reference(torch.ones(1, H + 2 * pad, W + 2 * pad, 1), pad, None, F64)[0, :, :, 0]
    inner = u.fold_interior(H, W, pad)
    if 'smallest' in name:
        assert H == pad + 1 and W == pad + 1
    if '3x3_terms' in name or 'both_sides' in name:
        assert float(cnt.max()) == 9
    if 'no_double_mirror' in name:
        assert float(cnt.max()) == 4 and bool(inner.any())
    if 'uneven' in name:
        assert (N * H * W * Cp // 4) % 256 != 0
    ref = u.reflect_fold_reference(gp, pad, None, torch.float32)
    assert torch.equal(ref[:, inner], gp[:, pad:pad + H, pad:pad + W][:, inner])


def test_reflect_fold_cases_cover_pads_and_widths():
    cs = list(u.FOLD_CASES.values())
    assert {c[4] for c in cs} == {1, 3} and {c[3] for c in cs} == {4, 64}


# ------------------------------------------------------------------------------------------ weight pack / unpack
def _dense(c, w):
    """the parameter as [rows, columns, taps] through plain tensor indexing"""
    _, R, C, _, _, tapidx = u.weight_layout(c)
    kh, kw = c['k']
    m = w.reshape(w.shape[0], w.shape[1], kh * kw)[:, :, tapidx]
    first_is_rows = (c['layer'] == 'conv') == (c['rows'] == 'O')
    return m if first_is_rows else m.permute(1, 0, 2)


@pytest.mark.parametrize('name', list(u.PACK_CASES) + list(u.KMAJOR_CASES))
def test_pack_reference_holds_the_split_weights_at_the_documented_places(name):
    kmajor = name in u.KMAJOR_CASES
    c = (u.KMAJOR_CASES if kmajor else u.PACK_CASES)[name]
    shape, R, C, sr, sc, tapidx = u.weight_layout(c)
    nt, Ccp, rows = len(tapidx), c['Ccp'], c['prows']
    Kp = nt * Ccp if kmajor else c['Kp']
    w = u.weight_inputs(name, c)
    if kmajor:
        packed, Wm = u.pack_kmajor_reference(w, R, C, sr, sc, tapidx, Ccp, rows)
        dst, lo_off = u.kmajor_index(rows, Kp, nt), 32
        assert Ccp % 32 == 0 and rows % 64 == 0
    else:
        packed, Wm = u.pack_reference(w, R, C, sr, sc, tapidx, Ccp, Kp, rows)
        dst, lo_off = u.fragment_index(rows, Kp), 512
        assert Ccp % 8 == 0 and rows % 32 == 0 and Kp % 32 == 0 and Kp >= nt * Ccp
    block_major = kmajor or (Ccp % 32 == 0 and Kp == nt * Ccp)
    assert block_major == (not name.startswith('tap_major'))
    if 'kp_padded' in name:
        assert Kp > nt * Ccp
    if 'phase_taps' in name:
        assert nt < c['k'][0] * c['k'][1]
    # every element of the buffer is written exactly once
    both = torch.cat((dst.flatten(), (dst + lo_off).flatten()))
    assert torch.equal(both.sort().values, torch.arange(2 * rows * Kp))
    assert not bool(torch.isnan(packed.float()).any())
    # the logical matrix against plain indexing of the parameter
    dense = _dense(c, w)                                          # [R, C, nt]
    full = torch.zeros(rows, (Kp // Ccp if not block_major else nt), Ccp)
    full[:R, :nt, :C] = dense.permute(0, 2, 1)
    if block_major:
        want = full.reshape(rows, nt, Ccp // 32, 32).permute(0, 2, 1, 3).reshape(rows, Kp)
    else:
        want = torch.zeros(rows, Kp)
        want[:, :(Kp // Ccp) * Ccp] = full.reshape(rows, -1)
    assert torch.equal(Wm, want)
    hi, lo = packed[dst].float(), packed[dst + lo_off].float()
    assert torch.equal(hi, Wm.bfloat16().float()) and float((hi + lo - Wm).abs().max()) <= 2.0 ** -16 * float(Wm.abs().max())
    assert bool((lo != 0).any()) and R % 32 != 0 and C % 8 != 0
    if not kmajor:
        assert (rows * Kp) % 4096 != 0 or name.startswith('block_major_ccp64')   # a partly filled last block of k_weights_multi


@pytest.mark.parametrize('name', list(u.UNPACK_CASES))
def test_unpack_reference_is_the_inverse_map_and_picks_the_named_kernel(name):
    c = u.UNPACK_CASES[name]
    shape, R, C, sr, sc, tapidx = u.weight_layout(c)
    nt, Ccp = len(tapidx), c['Ccp']
    assert u.unpack_kernel(sr, sc, nt) == c['kernel'] and Ccp % 4 == 0 and Ccp >= C
    idx = u.unpack_index(R, C, sr, sc, tapidx).flatten()
    assert idx.unique().numel() == idx.numel() and int(idx.max()) < torch.Size(shape).numel()
    gen = torch.Generator().manual_seed(3)
    dw = torch.randn(R, nt * Ccp, generator=gen)
    base = torch.randn(shape, generator=gen)
    out = u.unpack_reference(dw, R, C, sr, sc, tapidx, Ccp, base, c['accumulate'])
    got = _dense(c, out)                                           # [R, C, nt]
    want = dw.reshape(R, nt, Ccp)[:, :, :C].permute(0, 2, 1)
    assert torch.equal(got, _dense(c, base) + want if c['accumulate'] else want)
    untouched = torch.ones(shape, dtype=torch.bool).flatten()
    untouched[idx] = False
    assert torch.equal(out.flatten()[untouched], base.flatten()[untouched])
    assert bool(untouched.any()) == ('partial' in name)
    if 'c65' in name or 'c130' in name:
        assert C % 64 != 0 and C > 64
    if name == 'group4_1028_elements':
        assert R * nt * Ccp == 1024 + 4


# ------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize('name', [n for n in u.BN_CASES if n != 'c64_stem_rows_per_block_257'])
def test_batch_norm_reference_matches_torch(name):
    c = u.BN_CASES[name]
    d = u.bn_inputs(name)
    rows, C, training, relu = c['rows'], c['C'], c['training'], c['relu']
    assert abs(float(d['x'].mean()) - 3.0) < 0.5 and (rows < 100 or abs(float(d['x'].std()) - 0.5) < 0.1)
    fwd = u.bn_forward_reference(d, training, relu, F64)
    out32 = fwd['out'].float()
    bwd = u.bn_backward_reference(d, out32, fwd['mr'], training, relu, F64)
    x = d['x'].double()
    scale, shift = fwd['ss'][:, 0], fwd['ss'][:, 1]
    plain = x * scale + shift + (d['res'].double() if d['res'] is not None else 0)
    assert close(fwd['out'], F.relu(plain) if relu else plain, 1e-10)
    if training and rows == 1:    # torch refuses one value per channel: the kernel's rule, variance 0
        assert close(fwd['mr'][:, 1], torch.full((C,), 1e-5, dtype=F64) ** -0.5) and close(fwd['rv'], 0.9 * d['rv0'].double())
        assert float(bwd['dx'].abs().max()) < 1e-9
        return
    xg = x.clone().requires_grad_(True)
    gamma = (d['gamma'].double() if d['gamma'] is not None else torch.ones(C, dtype=F64)).requires_grad_(True)
    beta = (d['beta'].double() if d['beta'] is not None else torch.zeros(C, dtype=F64)).requires_grad_(True)
    rm, rv = d['rm0'].double().clone(), d['rv0'].double().clone()
    y = F.batch_norm(xg, rm, rv, gamma, beta, training=bool(training), momentum=u.MOMENTUM, eps=u.EPS)
    if d['res'] is not None:
        y = y + d['res'].double()
    if relu:
        y = F.relu(y)
    assert close(fwd['out'], y, 1e-10)
    assert close(fwd['rm'], rm) and close(fwd['rv'], rv)
    if relu:      # the mask is taken from the float32 output: no element may sit where rounding decides it
        assert torch.equal(out32 > 0, y.detach() > 0)
    (y * d['g'].double()).sum().backward()
    assert close(bwd['dx'], xg.grad, 1e-9)
    assert close(bwd['sums'][:, 0], beta.grad, 1e-9) and close(bwd['sums'][:, 1], gamma.grad, 1e-9)
    assert float(bwd['sums'].abs().median()) > 0


# ------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize('kind', u.MAXPOOL_INPUTS)
@pytest.mark.parametrize('shape', list(u.MAXPOOL_SHAPES))
def test_max_pool_reference_matches_torch(shape, kind):
    N, H, W, C = u.MAXPOOL_SHAPES[shape]
    x, g = u.maxpool_inputs(shape, kind)
    out, idx, has_nan = u.maxpool_reference(x)
    xt = x.permute(0, 3, 1, 2).contiguous()
    want, widx = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    want, widx = want.permute(0, 2, 3, 1), widx.permute(0, 2, 3, 1)
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.equal(torch.isnan(out), has_nan)
    assert torch.equal(torch.nan_to_num(out, nan=7.0), torch.nan_to_num(want, nan=7.0))
    flat = u.maxpool_flat_index(idx, H, W)
    assert bool((idx >= 0).all()) and torch.equal(flat[~has_nan], widx[~has_nan])       # routing where no NaN is in the window
    if kind == 'relu_ties':
        ties = (F.unfold(F.pad(xt, (1, 1, 1, 1), value=-1.0), 3, stride=2).reshape(N, C, 9, -1) == want.permute(0, 3, 1, 2).reshape(N, C, 1, -1))
        assert H * W < 40 or bool((ties.sum(dim=2) > 1).any())
        xg = xt.double().requires_grad_(True)
        (F.max_pool2d(xg, 3, 2, 1) * g.double().permute(0, 3, 1, 2)).sum().backward()
        gin, cnt = u.maxpool_bwd_reference(g, idx, H, W, F64)
        assert close(gin, xg.grad.permute(0, 2, 3, 1)) and int(cnt.max()) <= 4
    if kind == 'neg_inf_window':
        assert bool((out == float('-inf')).any())
    if kind == 'nan':
        assert bool(has_nan.any()) and (H * W == 1 or bool((~has_nan).any()))
    if 'uneven' in shape:
        assert (out.numel() // 4) % 256 != 0 and (x.numel() // 4) % 256 != 0


@pytest.mark.parametrize('name', list(u.AVGPOOL_CASES))
def test_average_pool_reference(name):
    N, HW, C = u.AVGPOOL_CASES[name]
    x, g = u.avgpool_inputs(name)
    r64, r32 = u.avgpool_reference(x, F64), u.avgpool_reference(x, torch.float32)
    assert close(r64, x.double().mean(dim=1)) and r32.dtype == torch.float32 and u.rel_l2(r32, r64) < 1e-6
    xg = x.double().requires_grad_(True)
    (xg.mean(dim=1) * g.double()).sum().backward()
    assert close(u.avgpool_bwd_reference(g, HW, F64), xg.grad)
    if '384' in name:
        assert N * C // 4 == 384


def test_helpers():
    assert float(u.ulp32(torch.tensor([1.0, 3.0, 0.75]))[0]) == 2.0 ** -23
    a = torch.tensor([0.0, float('nan'), 1.0])
    assert u.same_bits(a, a.clone()) and not u.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    hi, lo = u.split_planes_reference(torch.tensor([1.00390625, -2.5, 3.1415927]), relu=True)
    assert hi.tolist() == [1.0, 0.0, 3.140625] and lo[0] == 0.00390625 and lo[1] == 0
    assert u.ADD_N4[2] > 8192 * 1024 and 134e6 < u.ADD_N4[2] * 16 < 135e6
