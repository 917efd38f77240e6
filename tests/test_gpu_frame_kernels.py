"""The small fused kernels of the geometric frame step -- FFD decode, pose algebra, perspective transform, silhouette loss (and the
L1 loss beside it) -- against float64 references at the sizes the workload runs and at every block, wave and loop boundary of
their launch geometry.  Cases, generators, references and the self-calibrating gates: tests/frame_kernels_util.py (its
conditions are asserted on the CPU by tests/test_frame_kernels_host.py).  Every case names the code path its shape reaches.

Before each kernel call the allocator is poisoned: blocks of the sizes the op is about to ask for are filled with NaN and freed,
so that the `torch.empty` buffers of the op (key, acc, sums, gP, the outputs) come back holding NaN and a read of unwritten
scratch shows up in the result."""
import pytest
import torch

import frame_kernels_util as u

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PTF_NAMES = ('vertices', 'scales', 'rotations', 'translations', 'perspective_translations')


def poison(*nbytes):
    """NaN-filled blocks of each given size and one of their sum, freed at once: the caching allocator hands the op's
    `torch.empty` requests of those sizes the very same bytes"""
    sizes = [int(b) for b in nbytes if b]
    blocks = [torch.full(((s + 3) // 4,), float('nan'), device=DEV) for s in sizes]
    blocks.append(torch.full(((sum(sizes) + 3) // 4 + 1,), float('nan'), device=DEV))
    del blocks


def ptf_poison(n, V):
    from sdn_hip import perspective_transform_scratch
    key, acc = perspective_transform_scratch(n, V)
    poison(12 * n * V, 12 * n * V, key, acc, 4 * n, 12 * n, 12 * n, 12 * n, 16 * n)


def gpu_ptf(a, given=None, grad_out=True, grad_zooms=True):
    """the fused op through PerspectiveTransform.forward, the functional of frame_kernels_util.ptf_reference: (out, zooms, grads)
    on the CPU"""
    from derender3d.models.transforms import PerspectiveTransform
    x = {k: a[k].to(DEV).requires_grad_(True) for k in PTF_NAMES if k in a}
    n, V, _ = a['vertices'].shape
    kw = dict(x)
    if given is not None:
        x['zooms'] = given.to(DEV).requires_grad_(True)
        kw['zooms'] = x['zooms']
    else:
        x['zoom_tos'] = a['zoom_tos'].to(DEV).requires_grad_(True)
        kw['zoom_tos'] = x['zoom_tos']
    ptf_poison(n, V)
    res = PerspectiveTransform()(**kw)
    out, zooms = (res, x['zooms']) if given is not None else res
    assert 'PerspectiveTransformFn' in type(out.grad_fn).__name__
    loss = 0
    if grad_out:
        loss = loss + (out * a['w'].to(DEV)).sum()
    if grad_zooms:
        loss = loss + (zooms * a['wz'].to(DEV)).sum()
    ptf_poison(n, V)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad.cpu() if v.grad is not None else torch.zeros(v.shape)) for k, v in x.items()}
    return out.detach().cpu(), zooms.detach().cpu(), grads


def compare_ptf(case, got, ref64, ref32):
    (o, z, g), (o64, z64, g64), (o32, z32, g32) = got, ref64, ref32
    u.assert_close('ptf', case, 'out', o, o64, o32, 1e-6, 1e-6 * float(o64.abs().max()))
    u.assert_close('ptf', case, 'zooms', z, z64, z32, 1e-6, 0.0)
    assert set(g) == set(g64)
    for k in g:
        assert g[k].shape == g64[k].shape, k
        u.check_gate('ptf', case, 'd ' + k, g[k], g64[k], g32[k], u.FLOOR_GRAD)


@pytest.mark.parametrize('form', ['fit', 'given'])
@pytest.mark.parametrize('name', list(u.PTF_CASES))
def test_perspective_transform_shapes(name, form):
    """Every shape of frame_kernels_util.PTF_CASES (the path each one reaches is its note there: one wave, a second block, s_parts ==
    16 with and without a stride, more than 256 block minima, a planted argmin >= 65536, cdiv(n, 64) == 2 in k_ptf_bwd_c) in both
    forms -- zoom-to-fit with one tensor as both translations, and given zooms that take a gradient with two distinct tensors.
    The planted argmin is vertex 0, the last vertex and a vertex of another block, one per object.  Outputs, zooms and all five
    (six) gradients of a random functional of out and zooms against float64."""
    distinct = form == 'given'
    a, _ = u.ptf_case(name, distinct)
    given = u.given_zooms(a['vertices'].shape[0]) if distinct else None
    print(name, u.PTF_CASES[name][4])
    compare_ptf('%s/%s' % (name, form), gpu_ptf(a, given), u.ptf_reference(a, torch.float64, given),
                u.ptf_reference(a, torch.float32, given))


@pytest.mark.parametrize('arrival', ['zooms_only', 'out_only'])
def test_perspective_transform_gradient_arrival(arrival):
    """v4097 (s_parts == 16 with a second trip), zoom-to-fit: a gradient arriving for zooms only (g_out is None inside the op) and
    for out only (g_zooms is None)"""
    a, _ = u.ptf_case('v4097')
    kw = dict(grad_out=arrival == 'out_only', grad_zooms=arrival == 'zooms_only')
    compare_ptf('v4097/' + arrival, gpu_ptf(a, **kw), u.ptf_reference(a, torch.float64, **kw), u.ptf_reference(a, torch.float32, **kw))


@pytest.mark.parametrize('form', ['fit_two_tensors', 'given_one_tensor', 'scales_1x3'])
def test_perspective_transform_calling_forms(form):
    """v4097: zoom-to-fit with two distinct tensors as translations and perspective translations (k_ptf_bwd_c writes both), given
    zooms with one tensor for both (the summed gradient), and scales of shape [1, 3] broadcast to n (the `expand` in
    PerspectiveTransform.forward: the gradient is the sum over the objects)"""
    if form == 'scales_1x3':
        a, _ = u.broadcast_scales_case()
        a['scales'] = a['scales'][:1].clone()
        got = gpu_ptf(a)
        assert got[2]['scales'].shape == (1, 3)
        compare_ptf(form, got, u.ptf_reference(a, torch.float64, scales_rows=1), u.ptf_reference(a, torch.float32, scales_rows=1))
        return
    a, _ = u.ptf_case('v4097', form == 'fit_two_tensors')
    given = u.given_zooms(3) if form == 'given_one_tensor' else None
    compare_ptf(form, gpu_ptf(a, given), u.ptf_reference(a, torch.float64, given), u.ptf_reference(a, torch.float32, given))


@pytest.mark.parametrize('copies', u.PAD_COPIES)
@pytest.mark.parametrize('vertex0_wins', [True, False])
def test_perspective_transform_padding_ties(vertex0_wins, copies):
    """1, 255 and 1000 copies of vertex 0 appended to each object, as FFDBank pads, with vertex 0 as the planted argmin (every copy
    ties with the winner; the key carries the vertex index, so the lowest index wins, as torch's min(dim) picks the first) and with
    another vertex planted.  zooms are bit-equal to the unpadded run; in the kernel and in the float64 reference alike the zoom
    gradient lands on one row -- index 0 or the planted vertex -- and every other row, the copies included, gets exactly what g_out
    alone gives it: the rows of the same functional under the given-zoom form, which has no argmin term."""
    a, _ = u.pad_case(vertex0_wins)
    n, V, _ = a['vertices'].shape
    winner = [u.margin64(a, b)[0] for b in range(n)]
    assert all((i == 0) == vertex0_wins for i in winner)
    _, z_plain, _ = gpu_ptf(a)
    p = u.pad_with_vertex0(a, copies)
    got = gpu_ptf(p)
    assert torch.equal(got[1], z_plain)
    ref64 = u.ptf_reference(p, torch.float64)
    compare_ptf('pad%d/%s' % (copies, vertex0_wins), got, ref64, u.ptf_reference(p, torch.float32))
    for zooms, fit, run in ((got[1], got[2]['vertices'], lambda z: gpu_ptf(p, z)),
                            (ref64[1], ref64[2]['vertices'], lambda z: u.ptf_reference(p, torch.float64, z))):
        alone = run(zooms)[2]['vertices']
        differs = (fit != alone.to(fit.dtype)).any(dim=2)
        for b in range(n):
            assert torch.nonzero(differs[b]).reshape(-1).tolist() == [winner[b]], (b, winner[b])


def test_perspective_transform_nan_ratio_never_wins():
    """One vertex sits exactly at the origin after the transform (translation 0, perspective translation (0, 0, -1), vertex 0):
    its ratio is 0 / 0.  The kernel leaves it out of the minimum (torch's own min would return NaN): everything equals the float64
    reference computed without that vertex in the minimum, and its out row is still written -- (0, 0, 0)."""
    a = u.nan_case()
    skip = (0, u.NAN_VERTEX)
    got = gpu_ptf(a)
    assert got[0][0, u.NAN_VERTEX].tolist() == [0.0, 0.0, 0.0] and bool(torch.isfinite(got[1]).all())
    compare_ptf('nan', got, u.ptf_reference(a, torch.float64, skip=skip), u.ptf_reference(a, torch.float32, skip=skip))


def test_perspective_transform_equal_x_and_y_at_the_argmin():
    """|x| == |y| at the argmin (identity rotation, unit scale, translation == perspective translation on the axis: zero shear).
    The kernel sends the whole d max(|x|, |y|) to x, today's torch splits it evenly.  Both are subgradients; only what they agree on
    is asserted: every other vertex's gradient, the z part and the SUM of the x and y parts of that vertex's gradient and of the
    scale gradient (x == y there), the translation gradient (one tensor: the vertex lies in the plane z = 0 of the object, where the
    x and y parts of the two roles cancel), the quaternion gradient except its d component (a turn about the optical axis moves the
    vertex off the diagonal), and the zoom_to gradient."""
    a = u.diagonal_case()

    def fold(res):
        out, zooms, g = res
        gv = g['vertices'].clone()
        gv[0, u.DIAG_VERTEX, 0] += gv[0, u.DIAG_VERTEX, 1]
        gv[0, u.DIAG_VERTEX, 1] = 0
        gs = torch.stack((g['scales'][0, 0] + g['scales'][0, 1], g['scales'][0, 2]))
        return out, zooms, dict(vertices=gv, scales=gs, rotations=g['rotations'][:, :3], translations=g['translations'],
                                zoom_tos=g['zoom_tos'])
    compare_ptf('diagonal', fold(gpu_ptf(a)), fold(u.ptf_reference(a, torch.float64)), fold(u.ptf_reference(a, torch.float32)))


def test_perspective_transform_batch_independence_and_determinism():
    """v4097, n = 3: each object run alone gives bit-identical out, zooms and vertex gradients to the batched run (the index
    formulas key[n + b gridDim.x + i] and acc[20 n + 16 b + i] keep the objects apart); the parameter gradients meet in float atomics
    and are held to the gate.  Two batched runs agree bit for bit on out, zooms, the vertex gradient and the zoom_to gradient."""
    a, _ = u.ptf_case('v4097')
    o, z, g = gpu_ptf(a)
    o2, z2, g2 = gpu_ptf(a)
    assert torch.equal(o, o2) and torch.equal(z, z2) and torch.equal(g['vertices'], g2['vertices']) and torch.equal(g['zoom_tos'], g2['zoom_tos'])
    alone = []
    for b in range(3):
        ob, zb, gb = gpu_ptf({k: v[b:b + 1].clone() for k, v in a.items()})
        assert torch.equal(ob, o[b:b + 1]) and torch.equal(zb, z[b:b + 1]) and torch.equal(gb['vertices'], g['vertices'][b:b + 1])
        assert torch.equal(gb['zoom_tos'], g['zoom_tos'][b:b + 1])
        alone.append(gb)
    stacked = {k: torch.cat([gb[k] for gb in alone], dim=0) for k in g}   # the tensors of the batched run, object by object
    compare_ptf('alone', (o, z, stacked), u.ptf_reference(a, torch.float64), u.ptf_reference(a, torch.float32))


# ------------------------------------------------------------------------------------------ FFD decode
def gpu_ffd(P, Bt, cls, w, *constraint):
    from sdn_hip import ops
    n, vmax, ncoef = cls.numel(), Bt.shape[2], Bt.shape[1]
    x = P.to(DEV).requires_grad_(True)
    args = [t.to(DEV) for t in (Bt, cls) + constraint]
    poison(12 * n * vmax, 12 * n * ncoef)
    out = ops.FFDDecode.apply(x, *args)
    loss = (out * w.to(DEV)).sum()
    poison(12 * n * ncoef, 12 * n * ncoef)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize('name', list(u.FFD_CASES))
def test_ffd_decode_without_constraint(name):
    """ops.FFDDecode on P [n, 3, ncoef] for ncoef in {5, 7, 64, 512} (5 and 7 fire the FFD_JB tail guard of k_ffd_bwd), vmax in
    {1, 255, 257, 1023, 1025, 18714} (a second block column of k_ffd_fwd from 257, a second FFD backward trip from 1025), n in
    {1, 5} with repeated and distinct classes out of 3, against a float64 einsum.  The coefficient gradient is bit-identical
    across two runs (the kernel's header promises a fixed order)."""
    Bt, P, cls, w = u.ffd_inputs(name)
    print(name, u.FFD_CASES[name][3])
    o64, g64 = u.ffd_reference(Bt, P, cls, w, torch.float64)
    o32, g32 = u.ffd_reference(Bt, P, cls, w, torch.float32)
    out, grad = gpu_ffd(P, Bt, cls, w)
    u.assert_close('ffd', name, 'vertices', out, o64, o32, 1e-6, 2e-6)
    u.check_gate('ffd', name, 'd P', grad, g64, g32, u.FLOOR_GRAD)
    out2, grad2 = gpu_ffd(P, Bt, cls, w)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)


def test_ffd_decode_refuses_513_coefficients():
    """ncoef = 513 > NCOEF_MAX is refused with the library's message, and a valid call afterwards still succeeds"""
    from sdn_hip import SdnHipError, ops
    Bt = torch.rand(1, 513, 4, device=DEV)
    P = torch.rand(1, 3, 513, device=DEV)
    cls = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(SdnHipError, match=r'sdn_ffd_decode: bad arguments \(ncoef <= 512\)'):
        ops.FFDDecode.apply(P, Bt, cls)
    out = ops.FFDDecode.apply(P[:, :, :512].contiguous(), Bt[:, :512].contiguous(), cls)
    want = torch.einsum('bcj,bjv->bvc', P[:, :, :512].double().cpu(), Bt[:, :512].double().cpu())
    assert u.rel_l2(out, want) <= 1e-6


@pytest.mark.parametrize('ncoef', [1, 5, 512])
def test_ffd_coefficients_through_decode(ncoef):
    """sdn_ffd_coefficients at m = 3 ncoef in {3, 15, 1536} -- fewer outputs than one 64-wide group, a k range whose quarters are
    uneven, 24 output groups -- through ops.FFDDecode with a dense constraint map and a base: vertices, and the coefficient
    gradient, which takes the transposed map"""
    Bt, coeffs, C, base, cls, w = u.ffd_constraint_inputs(ncoef)
    o64, g64 = u.ffd_constraint_reference(Bt, coeffs, C, base, cls, w, torch.float64)
    o32, g32 = u.ffd_constraint_reference(Bt, coeffs, C, base, cls, w, torch.float32)
    out, grad = gpu_ffd(coeffs, Bt, cls, w, C, base)
    u.assert_close('ffd_coefficients', 'm%d' % (3 * ncoef), 'vertices', out, o64, o32, 1e-6, 2e-6)
    u.check_gate('ffd_coefficients', 'm%d' % (3 * ncoef), 'd coefficients', grad, g64, g32, u.FLOOR_GRAD)


def _bank():
    from derender3d.models.transforms import FFDBank
    ffds, _, faces = u.bank_templates()
    return FFDBank(ffds, faces).to(DEV)


def test_ffd_bank_decode_with_the_models_constraints():
    """A bank of two synthetic templates of 300 and 1100 vertices under the symmetry and homogeneity constraints the models use:
    decoded vertices and coefficient gradients against per-object float64 FFD.forward on the unpadded templates; the 800 padded rows
    of the smaller template equal its row 0; the gradient is bit-identical across two runs"""
    bank = _bank()
    classes = (0, 1, 1, 0, 1)
    coeffs = u.bank_coeffs(classes)
    w = torch.randn(len(classes), max(u.BANK_NVERTS), 3, generator=torch.Generator().manual_seed(7403))
    for i, k in enumerate(classes):
        w[i, u.BANK_NVERTS[k]:] = 0      # the reference has no padded rows
    v64, g64 = u.bank_reference(coeffs, classes, w, torch.float64)
    v32, g32 = u.bank_reference(coeffs, classes, w, torch.float32)
    grads = []
    for _ in range(2):
        x = coeffs.to(DEV).requires_grad_(True)
        poison(12 * 5 * 1100, 12 * 5 * 64, 12 * 5 * 64)
        verts, _faces = bank.decode(x, torch.tensor(classes, device=DEV))
        loss = (verts * w.to(DEV)).sum()
        poison(12 * 5 * 64, 12 * 5 * 64)
        loss.backward()
        grads.append(x.grad.cpu())
    for i, k in enumerate(classes):
        nv = u.BANK_NVERTS[k]
        u.assert_close('ffd_bank', 'object%d' % i, 'vertices', verts[i, :nv], v64[i], v32[i], 1e-6, 2e-6)
        if nv < verts.shape[1]:
            assert torch.equal(verts[i, nv:], verts[i, :1].expand(verts.shape[1] - nv, 3))
    u.check_gate('ffd_bank', 'constrained', 'd coefficients', grads[0], g64, g32, u.FLOOR_GRAD)
    assert torch.equal(grads[0], grads[1])


def test_chain_bank_decode_transform_on_padded_templates():
    """Bank decode -> transform with zoom-to-fit -> a random functional of out and zooms, for two objects of different classes.
    The pose of the smaller template's object was chosen (frame_kernels_util.chain_case, on the CPU, from the reference alone) so that
    its float64 argmin is vertex 0: its 800 padding copies tie with the winner.  The coefficient gradient equals the float64
    chain on the UNPADDED templates (the zooms are printed beside the float32 chain's)."""
    from derender3d.models.transforms import PerspectiveTransform
    bank = _bank()
    coeffs, pose = u.chain_case()
    w = pose['w'].clone()
    w[0, u.BANK_NVERTS[0]:] = 0
    _, z64, g64 = u.chain_reference(coeffs, pose, torch.float64)
    _, z32, g32 = u.chain_reference(coeffs, pose, torch.float32)
    x = coeffs.to(DEV).requires_grad_(True)
    verts, _faces = bank.decode(x, torch.tensor(u.CHAIN_CLASSES, device=DEV))
    ptf_poison(2, 1100)
    out, zooms = PerspectiveTransform()(verts, scales=pose['scales'].to(DEV), rotations=pose['rotations'].to(DEV),
                                        translations=pose['translations'].to(DEV), zoom_tos=pose['zoom_tos'].to(DEV))
    loss = (out * w.to(DEV)).sum() + (zooms * pose['wz'].to(DEV)).sum()
    ptf_poison(2, 1100)
    loss.backward()
    print('chain | zooms: float32 reference %.3e, measured %.3e relative' % (u.rel_l2(z32, z64), u.rel_l2(zooms, z64)))
    u.check_gate('chain', 'padded', 'd coefficients', x.grad, g64, g32, u.FLOOR_GRAD)


# ------------------------------------------------------------------------------------------ silhouette loss
def gpu_sil(m, t, ign, f, want_m=True, want_f=True):
    from derender3d.losses import silhouette_ffd_loss
    mg = m.detach().requires_grad_(want_m)
    fg = f.detach().requires_grad_(want_f) if f is not None else None
    poison(8 * (3 + 3 * 512), 4)
    loss = silhouette_ffd_loss(mg, t, fg, ign)
    scaled = loss * u.SIL_SCALE
    poison(4 * m.numel(), 4 * u.SIL_NFFD)
    scaled.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), (mg.grad.cpu() if want_m else None), (fg.grad.cpu() if fg is not None and want_f else None)


def compare_sil(case, got, ref64, ref32):
    for name, g, r64, r32 in zip(('loss', 'd masks', 'd ffd'), got, ref64, ref32):
        if r64 is not None:
            u.check_gate('sil_loss', case, name, g, r64, r32, u.FLOOR_LOSS)


@pytest.mark.parametrize('with_ffd', [True, False], ids=['ffd', 'noffd'])
@pytest.mark.parametrize('with_ign', [True, False], ids=['ignore', 'noignore'])
@pytest.mark.parametrize('n', list(u.SIL_COUNTS))
def test_silhouette_loss_element_counts(n, with_ign, with_ffd):
    """Element counts 1, 3, 5, 1023 (vec4 == 0), 4 * 1024 * 64 + 4 (65 blocks: the second trip of the finish kernel's block loop),
    16 * 384 * 384 (nblocks == 512, the cap) and 16 * 384 * 384 + 1 (vec4 == 0 at full size), with and without an ignore map and an
    FFD term: value and both gradients against float64; two runs are bit-identical, as the kernel states."""
    m, t, ign, f = u.sil_inputs(n)
    if n == u.SIL_FULL:
        m, t, ign = (x.reshape(16, 1, 384, 384) for x in (m, t, ign))
    ign = ign if with_ign else None
    f = f if with_ffd else None
    print(n, u.SIL_COUNTS[n])
    dev = lambda x: None if x is None else x.to(DEV)   # noqa: E731
    got = gpu_sil(dev(m), dev(t), dev(ign), dev(f))
    compare_sil('n%d' % n, got, u.sil_reference(m, t, ign, f, torch.float64), u.sil_reference(m, t, ign, f, torch.float32))
    again = gpu_sil(dev(m), dev(t), dev(ign), dev(f))
    for x, y in zip(got, again):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize('which', ['masks', 'target', 'ignore'])
def test_silhouette_loss_scalar_path_by_misalignment(which):
    """vec4 == 0 by alignment alone (n = 4096 is a multiple of 4): one operand in turn is a contiguous view that starts 4 bytes
    into its buffer"""
    n = 4096
    host = dict(zip(('masks', 'target', 'ignore', 'ffd'), u.sil_inputs(n)))
    devt = {k: v.to(DEV) for k, v in host.items()}
    shifted = torch.empty(n + 1, device=DEV)[1:]
    shifted.copy_(devt[which])
    devt[which] = shifted
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    assert all(devt[k].data_ptr() % 16 == 0 for k in host if k != which)
    got = gpu_sil(devt['masks'], devt['target'], devt['ignore'], devt['ffd'])
    args = (host['masks'], host['target'], host['ignore'], host['ffd'])
    compare_sil('shifted ' + which, got, u.sil_reference(*args, torch.float64), u.sil_reference(*args, torch.float32))


@pytest.mark.parametrize('n', [1023, 4 * 1024 * 64 + 4])
def test_silhouette_loss_ignore_extremes_and_single_gradients(n):
    """ignore all ones: loss 0 and exact zero gradients; ignore all zeros: the run without an ignore map, bit for bit; a gradient
    asked for masks only and for ffd only -- on the scalar and on the 16-byte path"""
    m, t, ign, f = (x.to(DEV) for x in u.sil_inputs(n))
    loss, gm, gf = gpu_sil(m, t, torch.ones_like(m), f)
    assert float(loss) == 0.0 and int(torch.count_nonzero(gm)) == 0 and int(torch.count_nonzero(gf)) == 0
    plain = gpu_sil(m, t, None, f)
    zeros = gpu_sil(m, t, torch.zeros_like(m), f)
    for x, y in zip(plain, zeros):
        assert torch.equal(x, y)
    full = gpu_sil(m, t, ign, f)
    only_m = gpu_sil(m, t, ign, f, want_f=False)
    only_f = gpu_sil(m, t, ign, f, want_m=False)
    assert only_m[2] is None and only_f[1] is None
    assert torch.equal(only_m[0], full[0]) and torch.equal(only_m[1], full[1]) and torch.equal(only_f[2], full[2])
    host = u.sil_inputs(n)
    compare_sil('n%d' % n, full, u.sil_reference(*host, torch.float64), u.sil_reference(*host, torch.float32))


# ------------------------------------------------------------------------------------------ pose algebra, pose parameters
@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('n', u.POSE_N)
def test_pose_algebra_object_counts(n, training):
    """sdn_pose_algebra / _bwd at n in {1, 64, 65, 130} (65: cdiv(n, 64) == 2 with one live thread in the second block; 130: three
    blocks) in both modes, with the inputs and gates of test_fused_pose_algebra_matches_the_elementwise_path.  alpha is compared
    modulo 2 pi, through cos and sin of the difference, and -pi <= alpha <= pi is asserted separately: objects are planted whose
    float64 alpha lies 5e-4 and 2e-7 from each end of the range, where float32 may legitimately land on the other end."""
    import math
    base = u.pose_inputs(n, training)
    poison(*([4 * n * k for k in (1, 1, 4, 3, 1, 2, 3, 3, 1)]))
    got, gz, gg = u.pose_run(base, training, DEV, torch.float32)
    ref, rz, rg = u.pose_run(base, training, 'cpu', torch.float64)
    _, _, g32 = u.pose_run(base, training, 'cpu', torch.float32)
    for k in u.POSE_OUTS:
        assert got[k].shape == ref[k].shape, k
        tol = 2e-6 * max(1.0, float(ref[k].abs().max()))
        if k == '_alphas':
            d = got[k].double() - ref[k]
            assert float(torch.sin(d).abs().max()) <= tol and float(torch.cos(d).min()) > 0.0, k
            pi32 = float(torch.tensor(math.pi, dtype=torch.float32))   # the kernel's own ends: 0 - pi and fmod's largest result - pi
            assert float(got[k].min()) >= -pi32 and float(got[k].max()) <= pi32
        else:
            assert float((got[k].double() - ref[k]).abs().max()) <= tol, k
    assert float(((gz.double().reshape(-1) - rz.reshape(-1)) / rz.reshape(-1)).abs().max()) <= 1e-6
    for k in u.POSE_PARAMS:
        u.check_gate('pose_algebra', 'n%d/%s' % (n, training), 'd ' + k, gg[k], rg[k], g32[k], u.FLOOR_GRAD)
    sub = ('_rotations', '_scales', '_translations', 'persp')
    _, _, gg = u.pose_run(base, training, DEV, torch.float32, sub)
    _, _, rg = u.pose_run(base, training, 'cpu', torch.float64, sub)
    _, _, g32 = u.pose_run(base, training, 'cpu', torch.float32, sub)
    for k in u.POSE_PARAMS:
        u.check_gate('pose_algebra', 'n%d/%s/subset' % (n, training), 'd ' + k, gg[k], rg[k], g32[k], u.FLOOR_GRAD)


@pytest.mark.parametrize('n', u.POSE_N)
def test_pose_parameters_object_counts(n):
    """sdn_pose_params / _bwd at n in {1, 64, 65, 130} with the inputs and gates of
    test_fused_pose_parameters_and_silhouette_loss_match_the_elementwise_formulas (absolute: 1e-6 quaternion, 3e-6 scales, 1e-6 and
    1e-5 gradients), and a gradient for the quaternion only"""
    from sdn_hip import ops
    theta, ls, wq, ws = u.pose_params_inputs(n)
    q64, s64, gt64, gl64 = u.pose_params_reference(theta, ls, wq, ws, torch.float64)
    thg, lsg = theta.to(DEV).requires_grad_(True), ls.to(DEV).requires_grad_(True)
    poison(16 * n, 12 * n)
    q, s = ops.PoseParamsFn.apply(thg, lsg)
    assert float((q.detach().cpu().double() - q64).abs().max()) <= 1e-6
    assert float((s.detach().cpu().double() - s64).abs().max()) <= 3e-6
    loss = (q * wq.to(DEV)).sum() + (s * ws.to(DEV)).sum()
    poison(4 * n, 12 * n)
    loss.backward()
    assert float((thg.grad.cpu().double() - gt64).abs().max()) <= 1e-6
    assert float((lsg.grad.cpu().double() - gl64).abs().max()) <= 1e-5
    thg.grad = None
    q2, _ = ops.PoseParamsFn.apply(thg, lsg)
    (q2 * wq.to(DEV)).sum().backward()
    _, _, gt64q, _ = u.pose_params_reference(theta, ls, wq, ws, torch.float64, quat_only=True)
    assert float((thg.grad.cpu().double() - gt64q).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------ L1 loss
def test_l1_loss_grid_stride_trip():
    """More than 4 * 256 * 4096 elements (2 x 8 x 512 x 513 = 4 202 496): the 4096-block cap is reached and k_l1_sum and k_l1_grad
    take their grid-stride trip.  The gates of test_fused_l1_loss_matches_torch: value 1e-6 relative, gradients 1e-6 of their
    largest element, sgn(0) = 0 at planted ties."""
    from models import networks as N
    from sdn_hip import ops
    g = torch.Generator().manual_seed(7700)
    shape = (2, 8, 512, 513)
    assert shape[0] * shape[1] * shape[2] * shape[3] > 4 * 256 * 4096
    a = torch.randn(shape, generator=g)
    b = torch.randn(shape, generator=g)
    b[0, 0, 0, :2] = a[0, 0, 0, :2]
    b[-1, -1, -1, -3:] = a[-1, -1, -1, -3:]
    ag, bg = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    assert ops.l1_loss_supported(ag, bg)
    poison(8, 4)
    loss = N.L1Loss()(ag, bg)
    assert 'L1LossFn' in type(loss.grad_fn).__name__
    loss = loss * 3.0
    poison(4 * a.numel(), 4 * a.numel())
    loss.backward()
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(a64, b64) * 3.0
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    for got, want in ((ag.grad, a64.grad), (bg.grad, b64.grad)):
        assert float((got.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float(ag.grad[0, 0, 0, 0]) == 0.0 and float(bg.grad[0, 0, 0, 1]) == 0.0 and float(ag.grad[-1, -1, -1, -1]) == 0.0
