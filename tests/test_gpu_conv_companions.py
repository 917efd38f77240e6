"""The HBM-bound companions of the convolutions through the C ABI -- sdn_in_apply, sdn_in_bwd, sdn_act_bwd, sdn_reflect_fold,
sdn_conv_pack_weights(_kmajor), sdn_conv_unpack_grad (csrc/conv_norm.hip, conv_pack.h), the pack / unpack / copy runs, ADD and
COLSUM records of sdn_program (csrc/fast_program.hip), sdn_bn_forward / sdn_bn_backward, sdn_maxpool3x3s2_* and sdn_avgpool_global
(csrc/conv_bn.hip) -- against float64 references at the shapes where their launch geometry changes: more than one block per image
(the cross-block fp64 atomics), ragged last blocks, positions per block above the floor, reduce and apply kernels with different
geometries, every channel layout, one and two positions per image.  Cases, generators, references and gates:
tests/conv_companions_util.py; tests/test_conv_companions_host.py proves on the CPU that the references agree with torch's own
operators and that every case reaches the path its name claims.

Every output and scratch tensor handed to a kernel holds NaN (or a sentinel) before the call, except where the ABI says the
caller zeroes it (stats, sums with SDN_IN_BWD_SUMS_ZEROED) or the call adds to it (bias_grad, accumulate): anything left
unwritten or read before it is written shows.  What the code defines exactly is compared bit for bit: packed weights, the bf16
planes (equal to sdn_split_planes of the fp32 tensor the same call wrote), unpacked gradients, max-pool values and indices, pad
channels, interior positions of the fold, a program run against per-record calls, k_add, k_colsum between two runs.

Every gated comparison prints (e32, gate, measured); see WORST below for the figures of an MI355X."""
import pytest
import torch
import torch.nn.functional as F

import conv_companions_util as u

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64

# Worst (e32, gate, measured) per entry point -- the comparison nearest its gate -- over all cases of this file on an MI355X:
WORST = """
    sdn_in_apply           hw_2, z                                          3.08e-07   2.00e-06   3.05e-07
    sdn_in_bwd             hw_2, mode 1, dz                                 2.32e-06   2.00e-05   1.25e-06
    sdn_act_bwd            npos_70000_cp_64, act 2, bias_grad               5.38e-08   2.00e-05   5.00e-07
    sdn_reflect_fold       pad3_4x4_smallest_3x3_terms, store               4.87e-08   1.00e-06   6.57e-08
    sdn_bn_forward         c4_rows_2_c4n_1, out                             2.68e-07   2.00e-06   2.71e-07
    sdn_bn_backward        c4_rows_2_c4n_1, d gamma                         4.21e-07   2.00e-05   4.25e-07
    sdn_maxpool3x3s2_bwd   h9_w10_c64_uneven_blocks, nan                    2.53e-08   1.00e-06   2.61e-08
    sdn_avgpool_global     hw_468_384_threads, out                          3.00e-07   1.20e-06   3.00e-07
    OP_COLSUM              rows 70000, C 64                                 0.498 ulp of the float64 sum (bound: 1 ulp)
Packs, unpacks, planes, max-pool forward, program runs and OP_ADD are bit-exact comparisons.  One finding: before k_bn_apply
was centred ((x - mean) * scale + beta instead of x * scale + shift) sdn_bn_forward measured 1.00e-05 on c4_rows_2_c4n_1
(e32 2.68e-07, gate 2.00e-06), where two rows 0.007 apart around 3 give rstd 270; c8_rows_1_train_formula_only (rstd 316) is
the second case of that kind.
Mutation check (each alone, on a scratch copy): 5.0f -> 4.0f in eff(); HW - 1.0 -> HW in k_in_finalize; r = 1 -> r = 2 in
block_reduce_rows; count - 1.0 -> count in k_bn_finalize; >= -> > in k_reflect_fold; lo plane 0 in pack_split8; accumulate
ignored in unpack_grad_rows; > -> >= in k_maxpool_fwd; load_stats one slot short.  Every one fails tests of this file (test_in_bwd
mode 2; test_in_apply; test_in_bwd + test_act_bwd; test_batch_norm; test_reflect_fold; test_pack_weights(_kmajor);
test_unpack_grad accumulate cases; test_max_pool ties and -inf; test_in_apply).  The earlier textural / encoder / conv /
program / trainstep / dropin / pipeline GPU tests catch eight of them; ignoring accumulate in unpack_grad_rows passes all 172.
"""


def api():
    from sdn_hip import check, lib, ptr, stream
    return check, lib(), ptr, stream


def nanf(*shape, dtype=F32):
    return torch.full(shape, u.NAN, dtype=dtype, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def new_planes(elems):
    """a NaN-filled plane pair whose stride leaves 8 guard elements behind each plane"""
    stride = elems + 8
    return torch.full((2 * stride,), u.NAN, dtype=torch.bfloat16, device=DEV), stride


def assert_planes(pl, stride, src, relu, what):
    """the planes are bit-equal to sdn_split_planes of `src` (the fp32 tensor the same call wrote), to the written-out split, and the
    guard elements are untouched"""
    check, L, ptr, stream = api()
    n = src.numel()
    want = torch.full_like(pl, u.NAN)
    check(L.sdn_split_planes(ptr(src), n, int(relu), ptr(want), stride, stream()))
    torch.cuda.synchronize()
    assert u.same_bits(pl, want), what
    hi, lo = u.split_planes_reference(src, relu)
    plc = pl.cpu()
    assert u.same_bits(plc[:n], hi) and u.same_bits(plc[stride:stride + n], lo), what
    assert bool(torch.isnan(plc[n:stride].float()).all()) and bool(torch.isnan(plc[stride + n:].float()).all()), what


def guarded(values, extra=8):
    """`values` followed by sentinels that must survive: (device buffer, the sentinels)"""
    tail = 12345.0 + torch.arange(extra, dtype=F32)
    return dev(torch.cat((values.float(), tail))), tail


# ------------------------------------------------------------------------------------------ sdn_in_apply
@pytest.mark.parametrize('name', list(u.IN_CASES))
def test_in_apply(name):
    """z in place, out2, mr, the running statistics (unbiased factor HW / (HW - 1), batch-averaged; exactly C floats, the floats
    behind them survive) and the planes, with stats spread at random over all SDN_STAT_SLOTS copies.  HW = 1: variance 0, output 0,
    everything finite."""
    check, L, ptr, stream = api()
    c = u.IN_CASES[name]
    N, C, Cp, HW = c['N'], c['C'], c['Cp'], c['HW']
    z, res, slot, rm0, rv0 = u.in_apply_inputs(name)
    has_res, res_relu = c['res'] is not None, int(c['res'] or 0)
    ref64 = u.in_apply_reference(z, res, C, c['act'], res_relu, rm0, rv0, F64)
    ref32 = u.in_apply_reference(z, res, C, c['act'], res_relu, rm0, rv0, F32)
    stats = dev(u.in_stats(z, slot))
    stats_before = stats.clone()
    zg, mr = dev(z), nanf(N, Cp, 2)
    resg = dev(res) if has_res else None
    out2 = nanf(N, HW, Cp) if has_res else None
    rm = rv = tail = None
    if c['running']:
        (rm, tail), (rv, _) = guarded(rm0), guarded(rv0)
    pl, stride = new_planes(N * HW * Cp) if c['planes'] is not None else (None, 0)
    check(L.sdn_in_apply(ptr(zg), ptr(stats), ptr(mr), ptr(resg), ptr(out2), N, HW, C, Cp, u.EPS, c['act'], res_relu, u.MOMENTUM,
                         ptr(rm), ptr(rv), ptr(pl), stride, int(c['planes'] or 0), stream()))
    torch.cuda.synchronize()
    assert u.same_bits(stats, stats_before)
    u.check_gate('sdn_in_apply', name, 'z', zg, ref64['y'], ref32['y'], u.FLOOR_ACT)
    if has_res:
        u.check_gate('sdn_in_apply', name, 'out2', out2, ref64['out2'], ref32['out2'], u.FLOOR_ACT)
    u.check_gate('sdn_in_apply', name, 'mean', mr[..., 0], ref64['mr'][..., 0], ref32['mr'][..., 0], u.FLOOR_GRAD)
    u.check_gate('sdn_in_apply', name, 'rstd', mr[..., 1], ref64['mr'][..., 1], ref32['mr'][..., 1], u.FLOOR_GRAD)
    if c['running']:
        u.check_gate('sdn_in_apply', name, 'running_mean', rm[:C], ref64['rm'], ref32['rm'], u.FLOOR_GRAD)
        u.check_gate('sdn_in_apply', name, 'running_var', rv[:C], ref64['rv'], ref32['rv'], u.FLOOR_GRAD)
        assert u.same_bits(rm[C:], tail) and u.same_bits(rv[C:], tail)
    if C < Cp:      # pad channels: exact zeros (the planes follow from their equality with the split of these tensors)
        assert u.same_bits(zg[..., C:], torch.zeros(N, HW, Cp - C))
        assert not has_res or u.same_bits(out2[..., C:], torch.zeros(N, HW, Cp - C))
    if HW == 1:
        assert u.same_bits(zg, torch.zeros(N, HW, Cp)) and bool(torch.isfinite(mr).all())
    if pl is not None:
        assert_planes(pl, stride, out2 if has_res else zg, c['planes'], name)


# ------------------------------------------------------------------------------------------ sdn_in_bwd
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', list(u.IN_CASES))
def test_in_bwd(name, mode):
    """dz in place, sums and the planes against autograd through the float64 InstanceNorm + activation, with exact zeros planted in
    `stored` (ReLU: gradient 0; LeakyReLU: slope 0.2).  Each mode runs with SDN_IN_BWD_SUMS_ZEROED (zeroed sums handed in) and
    without it (NaN-filled sums the call must clear), with and without planes."""
    check, L, ptr, stream = api()
    c = u.IN_CASES[name]
    N, C, Cp, HW = c['N'], c['C'], c['Cp'], c['HW']
    z, g = u.in_bwd_inputs(name)
    ref64, ref32 = u.in_bwd_reference(z, g, mode, F64), u.in_bwd_reference(z, g, mode, F32)
    stored, mr = dev(ref64['stored'].float()), dev(ref64['mr'].float())
    if mode and HW > 2:
        assert bool((stored[..., :C] == 0).any())
    for zeroed in (1, 0):
        for with_planes in (1, 0):
            tag = '%s/mode%d/%s/%s' % (name, mode, 'zeroed' if zeroed else 'cleared', 'planes' if with_planes else 'no planes')
            gg = dev(g)
            sums = torch.zeros(N, Cp, 2, dtype=F64, device=DEV) if zeroed else nanf(N, Cp, 2, dtype=F64)
            pl, stride = new_planes(N * HW * Cp) if with_planes else (None, 0)
            check(L.sdn_in_bwd(ptr(gg), ptr(stored), ptr(mr), ptr(sums), N, HW, Cp, mode | (u.SUMS_ZEROED if zeroed else 0), ptr(pl),
                               stride, stream()))
            torch.cuda.synchronize()
            u.check_gate('sdn_in_bwd', tag, 'dz', gg, ref64['dz'], ref32['dz'], u.FLOOR_GRAD)
            u.check_gate('sdn_in_bwd', tag, 'sum g', sums[..., 0], ref64['sums'][..., 0], ref32['sums'][..., 0], u.FLOOR_GRAD)
            u.check_gate('sdn_in_bwd', tag, 'sum g xhat', sums[..., 1], ref64['sums'][..., 1], ref32['sums'][..., 1], u.FLOOR_GRAD)
            if C < Cp:
                assert u.same_bits(gg[..., C:], torch.zeros(N, HW, Cp - C)), tag
            if pl is not None:
                assert_planes(pl, stride, gg, 0, tag)


# ------------------------------------------------------------------------------------------ sdn_act_bwd
@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('shape', list(u.ACT_SHAPES))
def test_act_bwd(shape, act):
    """g * act'(y) in place, bias_grad (which arrives holding non-zero values: the call adds to it; its error is measured against
    sum |terms| per channel) and the planes, with and without bias_grad (different positions per block) and planes.  act 0 with
    neither is the early return: g stays untouched, y may be NULL."""
    check, L, ptr, stream = api()
    c = u.ACT_SHAPES[shape]
    npos, Cp = c['npos'], c['Cp']
    g, y, b0 = u.act_inputs(shape, act)
    dz64, s64, a64 = u.act_bwd_reference(g, y, act, F64)
    dz32, s32, _ = u.act_bwd_reference(g, y, act, F32)
    yg = dev(y) if act else None
    for with_bias in (1, 0):
        for with_planes in (1, 0):
            tag = '%s/act%d/%s/%s' % (shape, act, 'bias' if with_bias else 'no bias', 'planes' if with_planes else 'no planes')
            gg = dev(g)
            bg = dev(b0) if with_bias else None
            pl, stride = new_planes(npos * Cp) if with_planes else (None, 0)
            check(L.sdn_act_bwd(ptr(gg), ptr(yg), ptr(bg), npos, Cp, act, ptr(pl), stride, stream()))
            torch.cuda.synchronize()
            if act == 0:
                assert u.same_bits(gg, g), tag
            else:
                u.check_gate('sdn_act_bwd', tag, 'dz', gg, dz64, dz32, u.FLOOR_GRAD)
            if with_bias:
                u.check_sum_gate('sdn_act_bwd', tag, 'bias_grad', bg, b0.double() + s64, b0 + s32, a64, u.FLOOR_GRAD)
            if pl is not None:
                assert_planes(pl, stride, gg, 0, tag)


# ------------------------------------------------------------------------------------------ sdn_reflect_fold
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('name', list(u.FOLD_CASES))
def test_reflect_fold(name, accumulate):
    """the gradient of F.pad(mode='reflect'); positions nothing mirrors onto equal gp (or out + gp) exactly"""
    check, L, ptr, stream = api()
    N, H, W, Cp, pad = u.FOLD_CASES[name]
    gp, base = u.fold_inputs(name)
    b = base if accumulate else None
    out = dev(base) if accumulate else nanf(N, H, W, Cp)
    gpg = dev(gp)
    check(L.sdn_reflect_fold(ptr(gpg), ptr(out), N, H, W, Cp, pad, accumulate, stream()))
    torch.cuda.synchronize()
    tag = '%s/%s' % (name, 'accumulate' if accumulate else 'store')
    u.check_gate('sdn_reflect_fold', tag, 'out', out, u.reflect_fold_reference(gp, pad, b, F64), u.reflect_fold_reference(gp, pad, b, F32),
                 u.FLOOR_FOLD)
    inner = u.fold_interior(H, W, pad)
    centre = gp[:, pad:pad + H, pad:pad + W]
    assert u.same_bits(out.cpu()[:, inner], (base + centre if accumulate else centre)[:, inner])


# ------------------------------------------------------------------------------------------ weight pack / gradient unpack
def _tapidx(tapidx):
    return torch.tensor(tapidx, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('name', list(u.PACK_CASES))
def test_pack_weights(name):
    """both planes bit for bit: hi == bf16(v), lo == bf16(v - hi) at the places include/sdn_hip.h documents, zero padding"""
    check, L, ptr, stream = api()
    c = u.PACK_CASES[name]
    _, R, C, sr, sc, tapidx = u.weight_layout(c)
    w = u.weight_inputs(name, c)
    want, _ = u.pack_reference(w, R, C, sr, sc, tapidx, c['Ccp'], c['Kp'], c['prows'])
    packed = nanf(2 * c['prows'] * c['Kp'], dtype=torch.bfloat16)
    wg, tap = dev(w), _tapidx(tapidx)        # (named: a temporary's memory would be handed to the next allocation before the launch)
    check(L.sdn_conv_pack_weights(ptr(wg), R, C, sr, sc, ptr(tap), len(tapidx), c['Ccp'], c['Kp'], c['prows'], ptr(packed),
                                  stream()))
    torch.cuda.synchronize()
    assert u.same_bits(packed, want)


@pytest.mark.parametrize('name', list(u.KMAJOR_CASES))
def test_pack_weights_kmajor(name):
    check, L, ptr, stream = api()
    c = u.KMAJOR_CASES[name]
    _, R, C, sr, sc, tapidx = u.weight_layout(c)
    w = u.weight_inputs(name, c)
    want, _ = u.pack_kmajor_reference(w, R, C, sr, sc, tapidx, c['Ccp'], c['prows'])
    packed = nanf(2 * c['prows'] * len(tapidx) * c['Ccp'], dtype=torch.bfloat16)
    wg, tap = dev(w), _tapidx(tapidx)
    check(L.sdn_conv_pack_weights_kmajor(ptr(wg), R, C, sr, sc, ptr(tap), len(tapidx), c['Ccp'], c['prows'], ptr(packed),
                                         stream()))
    torch.cuda.synchronize()
    assert u.same_bits(packed, want)


def _unpack_inputs(name, extra=0):
    c = u.UNPACK_CASES[name]
    shape, R, C, sr, sc, tapidx = u.weight_layout(c)
    gen = torch.Generator().manual_seed(8550 + u._seed(name) + extra)
    dw = torch.randn(R, len(tapidx) * c['Ccp'], generator=gen)          # the pad columns hold values too: nothing may take them
    base = torch.randn(shape, generator=gen) if c['accumulate'] else torch.full(shape, u.NAN)
    return c, (R, C, sr, sc, tapidx), dw, base


@pytest.mark.parametrize('name', list(u.UNPACK_CASES))
def test_unpack_grad(name):
    """both kernels (the LDS transpose and the group-of-4 scatter), store and accumulate, bit for bit; positions a partial tap list
    does not name keep their NaN"""
    check, L, ptr, stream = api()
    c, (R, C, sr, sc, tapidx), dw, base = _unpack_inputs(name)
    grad, dwg, tap = dev(base), dev(dw), _tapidx(tapidx)
    check(L.sdn_conv_unpack_grad(ptr(dwg), R, C, sr, sc, ptr(tap), len(tapidx), c['Ccp'], ptr(grad), c['accumulate'],
                                 stream()))
    torch.cuda.synchronize()
    want = u.unpack_reference(dw, R, C, sr, sc, tapidx, c['Ccp'], base, c['accumulate'])
    assert u.same_bits(grad, want)
    assert bool(torch.isnan(want).any()) == ('partial' in name and not c['accumulate'])


# ------------------------------------------------------------------------------------------ sdn_program: pack / unpack / copy runs
RUN_KINDS = (('pack', 'tap_major_ccp16_kp_padded_r24_c13'),           # 5120 elements: 4096 + 1024
             ('kmajor', 'kmajor_ccp32_r33_c20'),                      # 18432 = 4.5 x 4096
             ('unpack', 'rows_c65_3x3'),
             ('unpack', 'group4_1028_elements'),                      # 1024 + 4
             ('copy', 1025),                                          # floats: 1024 + 1
             ('pack', 'block_major_ccp32_r33_c20'),                   # 18432
             ('unpack', 'rows_c130_49_taps_accumulate'),
             ('unpack', 'group4_sc_above_sr_accumulate'),
             ('kmajor', 'kmajor_ccp64_convT_phase_taps'),
             ('copy', 4),
             ('unpack', 'rows_convT_partial_taps'),
             ('pack', 'tap_major_ccp48_convT_phase_taps'),            # 14336 = 3.5 x 4096
             ('copy', 16383))


def _run_record(b, pg, k, kind, what):
    """record k of a run: adds it to the builder and returns (ext pointers, output of the program, a function that makes the same
    call directly into a second output).  Every record has buffers of its own."""
    check, L, ptr, stream = api()
    names = ['%s%d' % (s, k) for s in ('src', 'tap', 'dst')]
    if kind == 'copy':
        gen = torch.Generator().manual_seed(8900 + k)
        src = dev(torch.randn(what, generator=gen))
        out, twin = nanf(what + 8), nanf(what + 8)
        b.op(pg.OP_COPY, buf=[b.ext(names[2]), b.ext(names[0])], l=[4 * what])

        def direct():
            twin[:what] = src
        return {names[0]: src, names[2]: out}, out, twin, direct
    if kind == 'unpack':
        c, (R, C, sr, sc, tapidx), dw, base = _unpack_inputs(what, extra=k)
        src, tap, out, twin = dev(dw), _tapidx(tapidx), dev(base), dev(base)
        b.op(pg.OP_UNPACK_GRAD, buf=[b.ext(names[0]), b.ext(names[1]), b.ext(names[2])], i=[R, C, len(tapidx), c['Ccp'], c['accumulate']],
             l=[sr, sc])

        def direct():
            check(L.sdn_conv_unpack_grad(ptr(src), R, C, sr, sc, ptr(tap), len(tapidx), c['Ccp'], ptr(twin), c['accumulate'], stream()))
        return {names[0]: src, names[1]: tap, names[2]: out}, out, twin, direct
    c = (u.PACK_CASES if kind == 'pack' else u.KMAJOR_CASES)[what]
    _, R, C, sr, sc, tapidx = u.weight_layout(c)
    src, tap, nt = dev(u.weight_inputs(what, c, extra=k)), _tapidx(tapidx), len(tapidx)
    n = 2 * c['prows'] * (c['Kp'] if kind == 'pack' else nt * c['Ccp'])
    out, twin = nanf(n, dtype=torch.bfloat16), nanf(n, dtype=torch.bfloat16)
    if kind == 'pack':
        b.op(pg.OP_PACK_WEIGHTS, buf=[b.ext(names[0]), b.ext(names[1]), b.ext(names[2])], i=[R, C, nt, c['Ccp'], c['Kp'], c['prows']], l=[sr, sc])

        def direct():
            check(L.sdn_conv_pack_weights(ptr(src), R, C, sr, sc, ptr(tap), nt, c['Ccp'], c['Kp'], c['prows'], ptr(twin), stream()))
    else:
        b.op(pg.OP_PACK_WEIGHTS_KMAJOR, buf=[b.ext(names[0]), b.ext(names[1]), b.ext(names[2])], i=[R, C, nt, c['Ccp'], c['prows']], l=[sr, sc])

        def direct():
            check(L.sdn_conv_pack_weights_kmajor(ptr(src), R, C, sr, sc, ptr(tap), nt, c['Ccp'], c['prows'], ptr(twin), stream()))
    return {names[0]: src, names[1]: tap, names[2]: out}, out, twin, direct


@pytest.mark.parametrize('count', [len(RUN_KINDS), 50])
def test_program_run_of_pack_unpack_copy_records_equals_per_record_calls(count):
    """One k_weights_multi launch over fragment packs, K-major packs, both unpack kernels and small copies whose sizes end inside a
    block (4096-element blocks for packs, 1024 for the rest), every record on buffers of its own: bit for bit what the per-record
    entry points write.  50 records are more than the 44 descriptors one launch carries: the run splits (the profiler sees two
    k_weights_multi launches, one for the shorter program), all 50 still agree."""
    from sdn_hip import program as pg
    b = pg.Builder()
    ext, pairs = {}, []
    for k in range(count):
        kind, what = RUN_KINDS[k % len(RUN_KINDS)]
        e, out, twin, direct = _run_record(b, pg, k, kind, what)
        ext.update(e)
        pairs.append((kind, what, out, twin, direct))
    prog = b.finish()
    assert prog.n_ops == count
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        prog.run({}, ext, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    launches = sum('k_weights_multi' in e.name for e in prof.events())
    assert launches == -(-count // 44), launches        # one launch carries at most 44 records: 50 split into 44 + 6
    for _, _, _, _, direct in pairs:
        direct()
    torch.cuda.synchronize()
    for k, (kind, what, out, twin, _) in enumerate(pairs):
        assert u.same_bits(out, twin), (k, kind, what)
        assert not bool(torch.isnan(out.float()).all()), (k, kind, what)


def _one_record(code, buf, ext, i=(), l=()):
    from sdn_hip import program as pg
    b = pg.Builder()
    b.op(getattr(pg, code), buf=[b.ext(n) for n in buf], i=i, l=l)
    b.finish().run({}, ext, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize('in_place', [0, 1])
@pytest.mark.parametrize('n4', u.ADD_N4[:2])
def test_program_add(n4, in_place):
    """OP_ADD: the float32 sum, exact, out of place and with out == a; the floats behind the range survive"""
    n = 4 * n4
    gen = torch.Generator().manual_seed(9000 + n4)
    a, bb = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ag, _ = guarded(a)
    bg = dev(bb)
    out = ag if in_place else nanf(n + 8)
    _one_record('OP_ADD', ['out', 'a', 'b'], {'out': out, 'a': ag, 'b': bg}, l=[n])
    assert u.same_bits(out[:n], a + bb)
    assert u.same_bits(out[n:], 12345.0 + torch.arange(8, dtype=F32)) if in_place else bool(torch.isnan(out[n:]).all())


def test_program_add_grid_stride_loop():
    """more than 8192 x 1024 float4 (134 MB a buffer): the only way into the grid-stride loop of k_add; in place"""
    n = 4 * u.ADD_N4[2]
    torch.manual_seed(9001)
    ag, bg = torch.randn(n + 8, device=DEV), torch.randn(n, device=DEV)
    a, bb = ag.cpu(), bg.cpu()
    _one_record('OP_ADD', ['out', 'a', 'b'], {'out': ag, 'a': ag, 'b': bg}, l=[n])
    got = ag.cpu()
    assert torch.equal(got[:n], a[:n] + bb) and torch.equal(got[n:], a[n:])


@pytest.mark.parametrize('cols', u.COLSUM_COLS)
@pytest.mark.parametrize('rows', u.COLSUM_ROWS)
def test_program_colsum(rows, cols):
    """OP_COLSUM: within one float32 ulp of the float64 column sums, identical between two runs, nothing written behind column C"""
    C, pitch = cols
    gen = torch.Generator().manual_seed(9100 + rows + C)
    g = torch.randn(rows, pitch, generator=gen) + 0.5
    ref = g[:, :C].double().sum(dim=0)
    gg = dev(g)
    outs = []
    for _ in range(2):
        out = nanf(C + 5)
        _one_record('OP_COLSUM', ['g', 'out'], {'g': gg, 'out': out}, i=[pitch, C], l=[rows])
        outs.append(out.cpu())
    assert u.same_bits(outs[0], outs[1]) and bool(torch.isnan(outs[0][C:]).all())
    err = (outs[0][:C].double() - ref).abs() / u.ulp32(ref.float())
    print('colsum | rows %d C %d | largest error %.3f ulp' % (rows, C, float(err.max())))
    assert float(err.max()) <= 1.0


# ------------------------------------------------------------------------------------------ sdn_bn_forward / sdn_bn_backward
@pytest.mark.parametrize('name', list(u.BN_CASES))
def test_batch_norm(name):
    """forward: out, mr, ss, the running statistics (exactly C floats; untouched in eval); backward, fed with the float32 rounding
    of the float64 forward (out, mr): gm exactly (it is a mask), dx, sums (d beta, d gamma).  Inputs with mean 3 and standard
    deviation 0.5, the conditioning of the stem.  The 134 MB case is the only one with rows_per_block above its floor."""
    check, L, ptr, stream = api()
    c = u.BN_CASES[name]
    rows, C, training, relu = c['rows'], c['C'], c['training'], c['relu']
    d = u.bn_inputs(name)
    f64, f32 = u.bn_forward_reference(d, training, relu, F64), u.bn_forward_reference(d, training, relu, F32)
    xg, resg, gamma, beta = dev(d['x']), dev(d['res']), dev(d['gamma']), dev(d['beta'])
    rm = rv = tail = None
    if c['running']:
        (rm, tail), (rv, _) = guarded(d['rm0']), guarded(d['rv0'])
    out, mr, ss = nanf(rows, C), nanf(C, 2), nanf(C, 2)
    sums = nanf(C, 2, dtype=F64) if training else None
    check(L.sdn_bn_forward(ptr(xg), rows, C, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), u.MOMENTUM, u.EPS, training, ptr(resg), relu,
                           ptr(out), ptr(mr), ptr(ss), ptr(sums), stream()))
    torch.cuda.synchronize()
    K = 'sdn_bn_forward'
    u.check_gate(K, name, 'out', out, f64['out'], f32['out'], u.FLOOR_ACT)
    for k, col in (('mean', 0), ('rstd', 1)):
        u.check_gate(K, name, k, mr[:, col], f64['mr'][:, col], f32['mr'][:, col], u.FLOOR_GRAD)
    for k, col in (('scale', 0), ('shift', 1)):
        u.check_gate(K, name, k, ss[:, col], f64['ss'][:, col], f32['ss'][:, col], u.FLOOR_GRAD)
    if c['running']:
        if training:
            u.check_gate(K, name, 'running_mean', rm[:C], f64['rm'], f32['rm'], u.FLOOR_GRAD)
            u.check_gate(K, name, 'running_var', rv[:C], f64['rv'], f32['rv'], u.FLOOR_GRAD)
        else:
            assert u.same_bits(rm[:C], d['rm0']) and u.same_bits(rv[:C], d['rv0'])
        assert u.same_bits(rm[C:], tail) and u.same_bits(rv[C:], tail)
    del out, ss, f32
    # ---- backward
    out32 = f64['out'].float()
    mr32 = f64['mr'].float()
    b64 = u.bn_backward_reference(d, out32, f64['mr'], training, relu, F64)
    b32 = u.bn_backward_reference(d, out32, mr32, training, relu, F32)
    gm, dx, sums = nanf(rows, C), nanf(rows, C), nanf(C, 2, dtype=F64)
    gg, outg, mrg = dev(d['g']), dev(out32) if relu else None, dev(mr32)
    check(L.sdn_bn_backward(ptr(gg), ptr(outg), ptr(xg), ptr(mrg), ptr(gamma), rows, C, training,
                            relu, ptr(gm), ptr(dx), ptr(sums), stream()))
    torch.cuda.synchronize()
    K = 'sdn_bn_backward'
    assert u.same_bits(gm, b32['gm'])
    u.check_gate(K, name, 'dx', dx, b64['dx'], b32['dx'], u.FLOOR_GRAD)
    u.check_gate(K, name, 'd beta', sums[:, 0], b64['sums'][:, 0], b32['sums'][:, 0], u.FLOOR_GRAD)
    u.check_gate(K, name, 'd gamma', sums[:, 1], b64['sums'][:, 1], b32['sums'][:, 1], u.FLOOR_GRAD)


# ------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize('kind', u.MAXPOOL_INPUTS)
@pytest.mark.parametrize('shape', list(u.MAXPOOL_SHAPES))
def test_max_pool(shape, kind):
    """values, NaN positions and routing equal F.max_pool2d on the CPU (ties after ReLU go to the first maximum in scan order, a
    window of -inf to its first element); in a window that holds a NaN only the value is asserted.  Backward, fed with the
    reference routing: exact where at most one window contributes, the 1e-6 gate where up to four do."""
    check, L, ptr, stream = api()
    N, H, W, C = u.MAXPOOL_SHAPES[shape]
    x, g = u.maxpool_inputs(shape, kind)
    OH, OW = g.shape[1:3]
    want, widx, has_nan = u.maxpool_reference(x)
    tv, ti = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    tv, ti = tv.permute(0, 2, 3, 1), ti.permute(0, 2, 3, 1)
    out = nanf(N, OH, OW, C)
    idx = torch.full((N, OH, OW, C), 99, dtype=torch.int8, device=DEV)
    xg, gg, widxg = dev(x), dev(g), dev(widx)
    check(L.sdn_maxpool3x3s2_fwd(ptr(xg), N, H, W, C, ptr(out), ptr(idx), stream()))
    torch.cuda.synchronize()
    assert u.same_bits(out, want) and torch.equal(torch.isnan(out.cpu()), torch.isnan(tv))
    assert torch.equal(out.cpu()[~has_nan], tv[~has_nan])
    idx = idx.cpu()
    assert bool(((idx >= 0) & (idx < 9)).all())
    assert torch.equal(idx[~has_nan], widx[~has_nan])
    assert torch.equal(u.maxpool_flat_index(idx, H, W)[~has_nan], ti[~has_nan])
    # ---- backward
    gin = nanf(N, H, W, C)
    check(L.sdn_maxpool3x3s2_bwd(ptr(gg), ptr(widxg), N, H, W, C, ptr(gin), stream()))
    torch.cuda.synchronize()
    r64, cnt = u.maxpool_bwd_reference(g, widx, H, W, F64)
    r32, _ = u.maxpool_bwd_reference(g, widx, H, W, F32)
    u.check_gate('sdn_maxpool3x3s2_bwd', '%s/%s' % (shape, kind), 'gin', gin, r64, r32, u.FLOOR_FOLD)
    assert u.same_bits(gin.cpu()[cnt <= 1], r32[cnt <= 1])


@pytest.mark.parametrize('name', list(u.AVGPOOL_CASES))
def test_average_pool(name):
    """the mean over HW positions against float64, e32 from an explicitly sequential float32 sum (the kernel's order), and the
    broadcast backward"""
    check, L, ptr, stream = api()
    N, HW, C = u.AVGPOOL_CASES[name]
    x, g = u.avgpool_inputs(name)
    out, gin, xg, gg = nanf(N, C), nanf(N, HW, C), dev(x), dev(g)
    check(L.sdn_avgpool_global(ptr(xg), N, HW, C, ptr(out), 0, stream()))
    check(L.sdn_avgpool_global(ptr(gg), N, HW, C, ptr(gin), 1, stream()))
    torch.cuda.synchronize()
    u.check_gate('sdn_avgpool_global', name, 'out', out, u.avgpool_reference(x, F64), u.avgpool_reference(x, F32), u.FLOOR_FOLD)
    u.check_gate('sdn_avgpool_global', name, 'gin', gin, u.avgpool_bwd_reference(g, HW, F64), u.avgpool_bwd_reference(g, HW, F32), u.FLOOR_FOLD)
