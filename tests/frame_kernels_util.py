"""Shared pieces of the frame-step kernel tests (tests/test_frame_kernels_host.py, tests/test_gpu_frame_kernels.py): the case
tables, the seeded input generators and the float64 references of the small fused kernels around the rasterizer --
csrc/transform.hip (perspective transform, pose algebra, pose parameters), csrc/fast_ffd.hip (FFD decode, constraint map) and
csrc/fast_loss.hip (silhouette + FFD-penalty loss, L1).  Nothing here needs a GPU.

References.  Each one is the plain torch expression, evaluated in float64 on the CPU from the float32 input values:
`PerspectiveTransform._forward_elementwise`, `FFD.forward` per object on the unpadded template, the
`mse + 100 mean(ffd ** 2)` expression of scripts/main.py:445-451, and `Derenderer3d._pose`.

Gates.  No number is taken from the kernel under test.  For every compared tensor the same reference expression is also
evaluated in float32 on the CPU; e32 is its relative L2 error against the float64 result and the kernel's gate is
max(floor, 4 e32) -- the factor 4 covers a different but legitimate summation order.  The floors are the gates the project
already uses: 2e-5 for transform, FFD and pose gradients, 1e-6 for the silhouette-loss value and gradients,
rtol 1e-6 / atol 1e-6 max|ref| for transform outputs, rtol 1e-6 / atol 2e-6 for decoded vertices.

The argmin of the zoom-to-fit ratio |z| / max(|x|, |y|) is planted by `plant_argmin`, which moves one vertex far off the
optical axis and returns the float64 relative margin between the smallest and the second-smallest ratio.  Every case without
a deliberate tie must have a margin of at least MIN_MARGIN = 1e-4, two orders above the float32 round-off of the ratio, so
that float32 and float64 agree on the argmin; tests/test_frame_kernels_host.py asserts that for every case of the tables below.

Worst (e32, gate, measured relative L2 error) per kernel -- the case nearest its gate -- over all cases of
tests/test_gpu_frame_kernels.py on an MI355X (the tests print every triple):
    perspective transform   pad1/True, d translations      2.73e-06   2.00e-05   9.82e-06
    FFD decode              c64_v18714, d P                2.77e-06   2.00e-05   1.36e-07
    FFD constraint map      m1536, d coefficients          2.99e-07   2.00e-05   3.57e-07
    FFD bank, constrained   d coefficients                 4.75e-07   2.00e-05   1.00e-07
    decode -> transform     d coefficients                 4.78e-07   2.00e-05   1.32e-07
    silhouette loss         shifted target, d ffd          1.40e-07   1.00e-06   6.15e-08
    pose algebra            n65, training, d theta_deltas  7.89e-08   2.00e-05   1.42e-07
Only one quantity comes near its gate: the gradient of ONE tensor passed as both translations and perspective translations.
Its x and y parts are the difference of two sums that nearly cancel (the object sits on the sheared axis), so float32 loses
digits in the reference expression as well: e32 is 1e-6 ... 5e-4 there (5.49e-04 at V = 1, where the kernel measures 5.17e-04
against a gate of 2.20e-03), and the kernel's own error moves by a third from run to run with the order of its float atomics.
"""
import copy
import functools
import math
import types

import torch

FLOOR_GRAD = 2e-5        # transform, FFD and pose gradients
FLOOR_LOSS = 1e-6        # silhouette-loss value and gradients
MIN_MARGIN = 1e-4
ZOOM_TO = 96 / (2 * 725.0)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def gate(floor, e32):
    return max(floor, 4.0 * e32)


def check_gate(kernel, case, name, got, ref64, ref32, floor):
    """print (e32, gate, measured) for one tensor and assert measured <= gate"""
    e32 = rel_l2(ref32, ref64)
    g = gate(floor, e32)
    err = rel_l2(got, ref64)
    print('%s | %s | %s: e32 %.3e gate %.3e measured %.3e' % (kernel, case, name, e32, g, err))
    assert err <= g, (kernel, case, name, e32, g, err)


def assert_close(kernel, case, name, got, ref64, ref32, rtol, atol):
    """the allclose-shaped floors of the outputs; prints the largest error in units of the allowance beside the same figure of
    the float32 evaluation of the reference"""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    allow = atol + rtol * ref64.abs()
    worst = float(((got - ref64).abs() / allow).max())
    worst32 = float(((ref32.detach().double() - ref64).abs() / allow).max())
    print('%s | %s | %s: rtol %.1e atol %.3e  float32 reference %.3f of the allowance, measured %.3f' %
          (kernel, case, name, rtol, atol, worst32, worst))
    assert worst <= 1.0, (kernel, case, name, worst)


# ------------------------------------------------------------------------------------------ perspective transform
def ptf_elementwise(**kw):
    from derender3d.models.transforms import PerspectiveTransform
    return PerspectiveTransform()._forward_elementwise(**kw)


def ptf_inputs(n, V, seed, distinct_persp=False):
    """the distribution of test_fused_perspective_transform_matches_elementwise: vertices randn * 0.4, scales rand + 0.8, unit
    quaternions, z in -[8, 28]; float32 CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    a = {
        'vertices': torch.randn(n, V, 3, generator=g) * 0.4,
        'scales': r(n, 3) + 0.8,
        'rotations': torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1),
        'translations': torch.stack([r(n) * 6 - 3, r(n) * 2, -(r(n) * 20 + 8)], 1),
        'zoom_tos': torch.full((n, 1), ZOOM_TO),
    }
    if distinct_persp:
        a['perspective_translations'] = a['translations'] + torch.randn(n, 3, generator=g) * 0.5
    a['w'] = torch.randn(n, V, 3, generator=g)
    a['wz'] = torch.randn(n, 1, generator=g)
    return a


def ptf_ratios64(a, b):
    """float64 ratios |z| / max(|x|, |y|) [V] of object b, through the reference expression"""
    d = {k: a[k][b:b + 1].double() for k in ('vertices', 'scales', 'rotations', 'translations')}
    p = a.get('perspective_translations')
    out = ptf_elementwise(perspective_translations=None if p is None else p[b:b + 1].double(), zooms=torch.ones(1, 1, dtype=torch.float64),
                          **d)[0]
    return out[:, 2].abs() / torch.max(out[:, 0].abs(), out[:, 1].abs())


def margin64(a, b):
    """(argmin, float64 relative margin between the smallest and the second-smallest ratio) of object b;
    NaN ratios (0 / 0) are left out, as in the kernel; one vertex has margin inf"""
    r = ptf_ratios64(a, b)
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    if r.numel() == 1:
        return 0, float('inf')
    two, idx = torch.topk(r, 2, largest=False)
    return int(idx[0]), float((two[1] - two[0]) / two[0])


def plant_argmin(a, b, index, offset=16.0):
    """Move vertex `index` of object b far off the optical axis: its scaled, rotated position becomes (offset, 0, 0), so that under
    a shear that (nearly) centres the object its ratio is about |t_z| / offset, below every other vertex's.  Returns the float64
    relative margin between the smallest and the second-smallest ratio of the object; where the minimum lies is for the caller
    to check (margin64)."""
    from derender3d.models.transforms import quaternion_matrix
    R = quaternion_matrix(a['rotations'][b:b + 1].double())[0]
    u = torch.tensor([offset, 0.0, 0.0], dtype=torch.float64)
    a['vertices'][b, index] = ((R.t() @ u) / a['scales'][b].double()).float()
    return margin64(a, b)[1]


# id: (n, V, seed, planted argmin per object, note)
PTF_CASES = {
    'v1': (3, 1, 7101, (0, 0, 0), 'one vertex, one block'),
    'v64': (3, 64, 7102, (0, 63, 32), 'one wave'),
    'v255': (3, 255, 7103, (0, 254, 128), 'one block with idle lanes'),
    'v256': (3, 256, 7104, (0, 255, 64), 'exactly one block'),
    'v257': (3, 257, 7105, (0, 256, 130), 'a second block of one vertex; the planted argmin of object 1 sits in it'),
    'v4096': (3, 4096, 7106, (0, 4095, 2049), 's_parts == 16 without a stride'),
    'v4097': (3, 4097, 7107, (0, 4096, 1111), 's_parts == 16 capped: the grid-stride loop of k_ptf_bwd_a takes a second trip'),
    'v18714': (3, 18714, 7108, (0, 18713, 9001), 'the largest mesh of the workload: 74 blocks, s_parts == 16 with 5 trips'),
    'v70001': (2, 70001, 7109, (69000, 300), 'more than 256 block minima per object (274): the i += 256 loop of k_ptf_fwd_b '
                                            'iterates; a planted argmin >= 65536; s_parts == 16 with a stride'),
    'n1': (1, 300, 7110, (299,), 'a single object'),
    'n65': (65, 300, 7111, tuple((37 * b + 5) % 300 for b in range(65)), 'cdiv(n, 64) == 2: k_ptf_bwd_c runs its second block'),
}


@functools.lru_cache(maxsize=None)
def _ptf_case(name, distinct_persp):
    n, V, seed, plant, _ = PTF_CASES[name]
    a = ptf_inputs(n, V, seed, distinct_persp)
    return a, [plant_argmin(a, b, plant[b]) for b in range(n)]


def ptf_case(name, distinct_persp=False):
    """(inputs, float64 margins per object) of a case; fresh clones, the cached draw stays unchanged"""
    a, margins = _ptf_case(name, bool(distinct_persp))
    return {k: v.clone() for k, v in a.items()}, list(margins)


def ptf_reference(a, dtype, given_zooms=None, grad_out=True, grad_zooms=True, skip=None, scales_rows=None):
    """The reference forward and backward of one case in `dtype` on the CPU.
    given_zooms [n, 1]: the training form (they take a gradient); else zoom-to-fit with a['zoom_tos'].
    skip (b, v): vertex v of object b is left out of the minimum (the NaN case) -- the zoom comes from the other vertices, the
    output row of v is still formed.  Only for n == 1.
    scales_rows: 1 for scales [1, 3] expanded to n.
    Returns (out, zooms, grads) with grads keyed like the inputs."""
    names = ['vertices', 'scales', 'rotations', 'translations'] + (['perspective_translations'] if 'perspective_translations' in a else [])
    x = {k: a[k].to(dtype).clone().requires_grad_(True) for k in names}
    n = a['vertices'].shape[0]
    kw = dict(x)
    if scales_rows is not None:
        kw['scales'] = x['scales'].expand(n, 3)
    if given_zooms is not None:
        x['zooms'] = given_zooms.to(dtype).clone().requires_grad_(True)
        out = ptf_elementwise(zooms=x['zooms'], **kw)
        zooms = x['zooms']
    else:
        x['zoom_tos'] = a['zoom_tos'].to(dtype).clone().requires_grad_(True)
        if skip is None:
            out, zooms = ptf_elementwise(zoom_tos=x['zoom_tos'], **kw)
        else:
            assert n == 1 and skip[0] == 0
            keep = [v for v in range(a['vertices'].shape[1]) if v != skip[1]]
            sub = dict(kw)
            sub['vertices'] = x['vertices'][:, keep]
            _, zooms = ptf_elementwise(zoom_tos=x['zoom_tos'], **sub)
            out = ptf_elementwise(zooms=zooms, **kw)
    loss = 0
    if grad_out:
        loss = loss + (out * a['w'].to(dtype)).sum()
    if grad_zooms:
        loss = loss + (zooms * a['wz'].to(dtype)).sum()
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in x.items()}
    return out.detach(), zooms.detach(), grads


def pad_with_vertex0(a, copies):
    """the inputs with `copies` copies of vertex 0 appended to every object, as FFDBank pads; the functional's weights of the copies
    are fresh random numbers"""
    p = dict(a)
    n, V, _ = a['vertices'].shape
    p['vertices'] = torch.cat((a['vertices'], a['vertices'][:, :1].expand(n, copies, 3)), dim=1).contiguous()
    g = torch.Generator().manual_seed(900 + copies)
    p['w'] = torch.cat((a['w'], torch.randn(n, copies, 3, generator=g)), dim=1).contiguous()
    return p


PAD_COPIES = (1, 255, 1000)
PAD_BASE = {True: 'v257', False: 'v4097'}    # vertex 0 planted as every object's argmin / as no object's


@functools.lru_cache(maxsize=None)
def _pad_case(vertex0_wins):
    n, V, seed, _, _ = PTF_CASES[PAD_BASE[vertex0_wins]]
    a = ptf_inputs(n, V, seed + 50)
    margins = [plant_argmin(a, b, 0 if vertex0_wins else 1 + 97 * (b + 1)) for b in range(n)]
    return a, margins


def pad_case(vertex0_wins):
    a, margins = _pad_case(bool(vertex0_wins))
    return {k: v.clone() for k, v in a.items()}, list(margins)


@functools.lru_cache(maxsize=None)
def _broadcast_scales_case():
    n, V, seed, plant, _ = PTF_CASES['v4097']
    a = ptf_inputs(n, V, seed + 70)
    a['scales'] = a['scales'][:1].expand(n, 3).clone()
    margins = [plant_argmin(a, b, plant[b]) for b in range(n)]
    return a, margins


def broadcast_scales_case():
    """the v4097 shape with one row of scales for every object (planted after the rows were made equal): the caller hands
    a['scales'][:1] to the op, which is the `expand` of PerspectiveTransform.forward"""
    a, margins = _broadcast_scales_case()
    return {k: v.clone() for k, v in a.items()}, list(margins)


def given_zooms(n, seed=7130):
    """zooms of the training form: (image_size / focal) / max(extent) is O(1)"""
    return torch.rand(n, 1, generator=torch.Generator().manual_seed(seed + n)) + 0.5


def nan_case():
    """n = 1, V = 300: translation 0, perspective translation (0, 0, -1), vertex NAN_VERTEX = 0: that vertex sits exactly at the
    origin after the transform, ratio 0 / 0.  The other vertices lie around z = -12 (their own offset, so that the ratios are
    those of an ordinary object; identity rotation keeps them there)."""
    a = ptf_inputs(1, 300, 7120)
    a['vertices'][:, :, 2] -= 12.0
    a['vertices'][0, NAN_VERTEX] = 0.0
    a['rotations'] = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    a['translations'] = torch.zeros(1, 3)
    a['perspective_translations'] = torch.tensor([[0.0, 0.0, -1.0]])
    return a


NAN_VERTEX = 0


def diagonal_case():
    """n = 1, V = 300: identity rotation, unit scale, translation == perspective translation on the optical axis (zero shear),
    and the planted argmin DIAG_VERTEX at (d, d, 0): |x| == |y| exactly at the argmin."""
    a = ptf_inputs(1, 300, 7121)
    a['scales'] = torch.ones(1, 3)
    a['rotations'] = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    a['translations'] = torch.tensor([[0.0, 0.0, -14.0]])
    a['vertices'][0, DIAG_VERTEX] = torch.tensor([16.0, 16.0, 0.0])
    return a


DIAG_VERTEX = 77


# ------------------------------------------------------------------------------------------ FFD decode
# (ncoef, vmax, classes of the objects out of 3, note)
FFD_CASES = {
    'c5_v257': (5, 257, (2,), 'FFD_JB tail: ncoef % 4 == 1; a second block column of k_ffd_fwd'),
    'c7_v1023': (7, 1023, (0, 1, 1, 2, 0), 'FFD_JB tail: ncoef % 4 == 3; one trip of the backward loop with idle lanes'),
    'c64_v1': (64, 1, (1, 1, 1, 1, 1), 'one vertex'),
    'c64_v255': (64, 255, (0,), 'one block column'),
    'c64_v1025': (64, 1025, (2, 0, 1, 0, 2), 'a second FFD backward trip (vmax > 1024) of one vertex'),
    'c64_v18714': (64, 18714, (0, 2, 2, 1, 0), 'the largest mesh of the workload: 19 backward trips, 74 block columns'),
    'c512_v257': (512, 257, (1, 0, 2, 2, 1), 'NCOEF_MAX: the whole LDS table'),
    'c5_v1025': (5, 1025, (0, 1, 2, 1, 0), 'the FFD_JB tail and a second backward trip together'),
}


def ffd_inputs(name):
    """Bt [3, ncoef, vmax]: non-negative weights that sum to 1 over the coefficients, like a Bernstein basis; P [n, 3, ncoef] in
    [-0.5, 0.5] like a control lattice; w [n, vmax, 3] the functional"""
    ncoef, vmax, classes, _ = FFD_CASES[name]
    g = torch.Generator().manual_seed(7200 + 31 * ncoef + vmax)
    Bt = torch.rand(3, ncoef, vmax, generator=g) ** 3
    Bt = (Bt / Bt.sum(dim=1, keepdim=True)).contiguous()
    n = len(classes)
    P = torch.rand(n, 3, ncoef, generator=g) - 0.5
    w = torch.randn(n, vmax, 3, generator=g)
    return Bt, P, torch.tensor(classes, dtype=torch.int32), w


def ffd_reference(Bt, P, cls, w, dtype):
    """(vertices [n, vmax, 3], d (vertices . w) / d P) as an einsum in `dtype`"""
    P = P.to(dtype).clone().requires_grad_(True)
    out = torch.einsum('bcj,bjv->bvc', P, Bt.to(dtype)[cls.long()])
    (out * w.to(dtype)).sum().backward()
    return out.detach(), P.grad


def ffd_constraint_inputs(ncoef, n=4, vmax=70):
    """a dense random constraint map [3 ncoef, 3 ncoef] and base [3, ncoef] for sdn_ffd_coefficients at m = 3 ncoef through
    ops.FFDDecode"""
    g = torch.Generator().manual_seed(7300 + ncoef)
    m = 3 * ncoef
    Bt = torch.rand(2, ncoef, vmax, generator=g) ** 3
    Bt = (Bt / Bt.sum(dim=1, keepdim=True)).contiguous()
    coeffs = torch.randn(n, m, generator=g) * 0.1
    C = torch.randn(m, m, generator=g) / m ** 0.5
    base = torch.rand(3, ncoef, generator=g) - 0.5
    cls = torch.tensor([k % 2 for k in range(n)], dtype=torch.int32)
    w = torch.randn(n, vmax, 3, generator=g)
    return Bt, coeffs, C, base, cls, w


def ffd_constraint_reference(Bt, coeffs, C, base, cls, w, dtype):
    x = coeffs.to(dtype).clone().requires_grad_(True)
    n, m = x.shape
    P = (base.to(dtype).reshape(1, m) + x @ C.to(dtype)).reshape(n, 3, m // 3)
    out = torch.einsum('bcj,bjv->bvc', P, Bt.to(dtype)[cls.long()])
    (out * w.to(dtype)).sum().backward()
    return out.detach(), x.grad


def model_constraints():
    """the symmetry and homogeneity constraints the models use (derender3d/models/__init__.py)"""
    from derender3d.models.transforms import FFD
    return [FFD.Constraint.symmetry(axis=FFD.Constraint.Axis.z),
            FFD.Constraint.homogeneity(axis=FFD.Constraint.Axis.y, index=[0, 1])]


BANK_NVERTS = (300, 1100)


@functools.lru_cache(maxsize=None)
def bank_templates():
    """two synthetic templates of 300 and 1100 random points in [-0.45, 0.45]^3 as (FFD float32, FFD float64, faces).  The point
    farthest from the centre is stored first: only a vertex on the hull can be the zoom-to-fit argmin, which chain_case needs
    vertex 0 to be."""
    from derender3d.models.transforms import FFD
    g = torch.Generator().manual_seed(7400)
    points = []
    for nv in BANK_NVERTS:
        p = torch.rand(nv, 3, generator=g) * 0.9 - 0.45
        far = int(p.norm(dim=1).argmax())
        p[[0, far]] = p[[far, 0]]
        points.append(p)
    ffds = [FFD(p, constraints=model_constraints()) for p in points]
    ffds64 = [copy.deepcopy(f).double() for f in ffds]
    faces = [torch.tensor([[0, 1, 2]], dtype=torch.int32) for _ in ffds]
    return ffds, ffds64, faces


def bank_coeffs(classes, seed=7401):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(len(classes), 192, generator=g) * 0.05


def bank_reference(coeffs, classes, w, dtype):
    """per-object FFD.forward on the unpadded templates: (list of vertices [nv_k, 3], coefficient gradients [n, 192]); w [n, vmax, 3]
    is read over each object's own vertices"""
    ffds, ffds64, _ = bank_templates()
    mods = ffds64 if dtype == torch.float64 else ffds
    x = coeffs.to(dtype).clone().requires_grad_(True)
    outs = [mods[k](x[i]) for i, k in enumerate(classes)]
    sum((o * w[i, :o.shape[0]].to(dtype)).sum() for i, o in enumerate(outs)).backward()
    return [o.detach() for o in outs], x.grad


CHAIN_CLASSES = (0, 1)


@functools.lru_cache(maxsize=None)
def chain_case():
    """Bank decode -> zoom-to-fit transform for two objects of classes (0, 1).  The pose of object 0 (the smaller template, padded
    with 800 copies of its vertex 0) is found by a search over seeds on the CPU, using the float64 reference only: the first seed
    whose argmin is vertex 0 with a margin >= MIN_MARGIN, so that the padding copies tie with the winner.  The vertices of the
    templates keep their random positions; 512 poses are tried per batch."""
    _, ffds64, _ = bank_templates()
    coeffs = bank_coeffs(CHAIN_CLASSES, seed=7402)
    v0 = ffds64[0](coeffs[0].double())                       # [300, 3]
    found = None
    for batch in range(64):
        a = ptf_inputs(512, 1, 7500 + batch)
        a['vertices'] = v0.float()[None].expand(512, -1, -1).contiguous()
        d = {k: a[k].double() for k in ('vertices', 'scales', 'rotations', 'translations')}
        out = ptf_elementwise(zooms=torch.ones(512, 1, dtype=torch.float64), **d)
        r = out[..., 2].abs() / torch.max(out[..., 0].abs(), out[..., 1].abs())
        two, idx = torch.topk(r, 2, dim=1, largest=False)
        ok = (idx[:, 0] == 0) & ((two[:, 1] - two[:, 0]) / two[:, 0] >= MIN_MARGIN)
        if bool(ok.any()):
            s = int(torch.nonzero(ok)[0])
            found = {k: a[k][s:s + 1].clone() for k in ('scales', 'rotations', 'translations', 'zoom_tos')}
            break
    assert found is not None, 'no pose puts the argmin on vertex 0'
    other = ptf_inputs(1, 1, 7499)
    pose = {k: torch.cat((found[k], other[k]), dim=0) for k in found}
    g = torch.Generator().manual_seed(7498)
    pose['w'] = torch.randn(2, max(BANK_NVERTS), 3, generator=g)
    pose['wz'] = torch.randn(2, 1, generator=g)
    return coeffs, pose


def chain_reference(coeffs, pose, dtype):
    """the chain on the UNPADDED templates, object by object: (outs, zooms, coefficient gradient [2, 192], argmins, margins)"""
    ffds, ffds64, _ = bank_templates()
    mods = ffds64 if dtype == torch.float64 else ffds
    x = coeffs.to(dtype).clone().requires_grad_(True)
    loss, outs, zooms = 0, [], []
    for i, k in enumerate(CHAIN_CLASSES):
        v = mods[k](x[i])[None]
        kw = {q: pose[q][i:i + 1].to(dtype) for q in ('scales', 'rotations', 'translations', 'zoom_tos')}
        out, z = ptf_elementwise(vertices=v, **kw)
        loss = loss + (out * pose['w'][i:i + 1, :v.shape[1]].to(dtype)).sum() + (z * pose['wz'][i:i + 1].to(dtype)).sum()
        outs.append(out.detach()[0])
        zooms.append(z.detach()[0])
    loss.backward()
    return outs, torch.stack(zooms), x.grad


def chain_margins(coeffs, pose):
    _, ffds64, _ = bank_templates()
    res = []
    for i, k in enumerate(CHAIN_CLASSES):
        a = {q: pose[q][i:i + 1] for q in ('scales', 'rotations', 'translations')}
        a['vertices'] = ffds64[k](coeffs[i].double())[None]
        res.append(margin64(a, 0))
    return res


# ------------------------------------------------------------------------------------------ silhouette loss
SIL_FULL = 16 * 384 * 384
# n: note
SIL_COUNTS = {
    1: 'vec4 == 0 (n % 4 != 0), one block, one thread with work',
    3: 'vec4 == 0',
    5: 'vec4 == 0; with 16-byte loads forced the fifth element would be dropped',
    1023: 'vec4 == 0, one block, four trips of its loop',
    4 * 1024 * 64 + 4: 'vec4 == 1 with 65 blocks: the b += 64 loop of k_sil_loss_finish takes its second trip',
    SIL_FULL: 'the frame of the workload: vec4 == 1, nblocks == 512 (the cap) with a stride',
    SIL_FULL + 1: 'vec4 == 0 at full size: nblocks == 512 on the scalar path',
}
SIL_NFFD = 16 * 192
SIL_SCALE = 1.7


def sil_inputs(n, seed=None):
    g = torch.Generator().manual_seed(7600 + (n % 9973) if seed is None else seed)
    masks = torch.rand(n, generator=g)
    target = (torch.rand(n, generator=g) > 0.5).float()
    ign = (torch.rand(n, generator=g) > 0.8).float()
    ffd = torch.randn(SIL_NFFD, generator=g) * 0.05
    return masks, target, ign, ffd


def sil_reference(masks, target, ign, ffd, dtype):
    """scripts/main.py:445-451 (without the FFD term when ffd is None): (loss, d masks, d ffd) of SIL_SCALE * loss"""
    m = masks.to(dtype).clone().requires_grad_(True)
    f = ffd.to(dtype).clone().requires_grad_(True) if ffd is not None else None
    loss = torch.nn.functional.mse_loss(m, target.to(dtype), reduction='none')
    if f is not None:
        loss = loss + 100 * torch.mean(f ** 2)
    if ign is not None:
        loss = loss * (1 - ign.to(dtype))
    loss = torch.mean(loss)
    (loss * SIL_SCALE).backward()
    return loss.detach(), m.grad, (f.grad if f is not None else None)


# ------------------------------------------------------------------------------------------ pose algebra
POSE_N = (1, 64, 65, 130)
POSE_PARAMS = ('_theta_deltas', '_log_scales', '_log_depths', '_translation2ds')
POSE_OUTS = ('_thetas', '_alphas', '_rotations', '_scales', '_depths', '_center2ds', '_translations', 'persp')
POSE_NEAR = 5e-4       # planted distance of alpha from an end of [-pi, pi]
POSE_NEAREST = 2e-7    # and of a second pair, within float32 round-off of the end: either end is a correct answer there


def pose_self(training):
    return types.SimpleNamespace(training=training, image_size=256, render_size=384, _force_no_sample=True,
                                 _classes=lambda blob, P: None)


def pose_planted(n):
    """{object: signed distance}: alpha = pi - d for d > 0, -pi - d for d < 0; the last objects (the second block for n > 64)
    and the first"""
    if n == 1:
        return {0: POSE_NEAR}
    return {0: POSE_NEAR, 1: -POSE_NEAREST, n - 2: POSE_NEAREST, n - 1: -POSE_NEAR}


def pose_inputs(n, training):
    """the inputs of test_fused_pose_algebra_matches_the_elementwise_path for n objects, with the yaw of the planted objects chosen
    so that the float64 alpha lies next to an end of its range"""
    from derender3d.models import Derenderer3d
    g = torch.Generator().manual_seed(31 + int(training) + 100 * n)
    base = {
        '_mroi_norms': torch.rand(n, 2, generator=g) * 0.8 - 0.4,
        '_droi_norms': torch.rand(n, 2, generator=g) * 0.5 + 0.1,
        '_focals': torch.rand(n, 1, generator=g) * 300 + 500,
        '_theta_deltas': torch.randn(n, 2, generator=g),
        '_log_scales': torch.randn(n, 3, generator=g) * 0.3,
        '_log_depths': torch.randn(n, 1, generator=g) * 0.3 + 1.0,
        '_translation2ds': torch.randn(n, 2, generator=g) * 0.2,
        '_class_probs': torch.softmax(torch.randn(n, 8, generator=g), dim=1),
    }
    P = Derenderer3d._pose(pose_self(training), {k: v.double() for k, v in base.items()})
    t = P['_translations']
    bearing = torch.atan(t[:, 0] / t[:, 2])
    for i, d in pose_planted(n).items():
        alpha = (math.pi - d) if d > 0 else (-math.pi - d)
        theta = float(bearing[i]) - alpha                      # alpha = -(theta - bearing)  (mod 2 pi)
        theta = math.atan2(math.sin(theta), math.cos(theta))
        base['_theta_deltas'][i] = torch.tensor([math.cos(theta), math.sin(theta)], dtype=torch.float64).float() * 1.3
    return base


def pose_run(base, training, device, dtype, subset=POSE_OUTS):
    """Derenderer3d._pose and the gradients of a random linear functional of the outputs in `subset`"""
    from derender3d.models import Derenderer3d
    blob = {k: v.detach().clone().to(device=device, dtype=dtype) for k, v in base.items()}   # fresh leaves: base stays untouched
    for k in POSE_PARAMS:
        blob[k].requires_grad_(True)
    P = Derenderer3d._pose(pose_self(training), blob)
    w = torch.Generator().manual_seed(5)
    loss = 0
    for k in POSE_OUTS:
        wk = torch.randn(P[k].shape, generator=w).to(device=device, dtype=dtype)
        if k in subset:
            loss = loss + (P[k] * wk).sum()
    loss.backward()
    zoom = P['_zooms'] if training else P['zoom_tos']
    return ({k: P[k].detach().cpu() for k in POSE_OUTS}, zoom.detach().cpu(), {k: blob[k].grad.cpu() for k in POSE_PARAMS})


def pose_params_inputs(n):
    """the inputs of test_fused_pose_parameters_and_silhouette_loss_match_the_elementwise_formulas for n objects"""
    g = torch.Generator().manual_seed(4 + 100 * n)
    theta = torch.rand(n, 1, generator=g) * 6.2 - 3.1
    ls = torch.randn(n, 3, generator=g) * 0.3
    return theta, ls, torch.randn(n, 4, generator=g), torch.randn(n, 3, generator=g)


def pose_params_reference(theta, ls, wq, ws, dtype, quat_only=False):
    th, l = theta.to(dtype).clone().requires_grad_(True), ls.to(dtype).clone().requires_grad_(True)
    zero = torch.zeros_like(th)
    q = torch.cat((torch.cos(th / 2), zero, torch.sin(th / 2), zero), dim=1)
    s = torch.exp(l)
    loss = (q * wq.to(dtype)).sum()
    if not quat_only:
        loss = loss + (s * ws.to(dtype)).sum()
    loss.backward()
    return q.detach(), s.detach(), th.grad, (l.grad if l.grad is not None else torch.zeros_like(l))
