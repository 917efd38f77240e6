"""What tests/test_gpu_frame_kernels.py takes for granted, checked without a GPU: every case of the tables in
tests/frame_kernels_util.py has its zoom-to-fit argmin where the table says, with a float64 margin of at least 1e-4 to the
runner-up (so float32 and float64 cannot disagree about it); torch's own tie semantics that the tie cases rely on; and
torch.autograd.gradcheck of the float64 reference wrappers at a tiny shape, so that a wrong reference cannot pass a wrong kernel."""
import math

import pytest
import torch

import frame_kernels_util as u


@pytest.mark.parametrize('distinct', [False, True], ids=['one_translation', 'two_translations'])
@pytest.mark.parametrize('name', list(u.PTF_CASES))
def test_planted_argmin_and_margin_of_every_transform_case(name, distinct):
    a, margins = u.ptf_case(name, distinct)
    n, V, _, plant, _ = u.PTF_CASES[name]
    assert a['vertices'].shape == (n, V, 3) and len(plant) == n
    for b in range(n):
        idx, m = u.margin64(a, b)
        assert idx == plant[b], (name, b, idx, plant[b])
        assert m == margins[b] and m >= u.MIN_MARGIN, (name, b, m)
    if name == 'v70001':
        assert plant[0] >= 65536 and -(-V // 256) > 256
    if name == 'v257':
        assert len({p // 256 for p in plant}) > 1   # a different block per object


@pytest.mark.parametrize('vertex0_wins', [True, False])
def test_padding_cases_tie_only_with_vertex_0(vertex0_wins):
    a, margins = u.pad_case(vertex0_wins)
    n, V, _ = a['vertices'].shape
    for b in range(n):
        idx, m = u.margin64(a, b)
        assert (idx == 0) == vertex0_wins and m >= u.MIN_MARGIN, (b, idx, m)
        for copies in u.PAD_COPIES:
            p = u.pad_with_vertex0(a, copies)
            assert p['vertices'].shape[1] == V + copies and torch.equal(p['vertices'][b, V:], a['vertices'][b, :1].expand(copies, 3))
            r = u.ptf_ratios64(p, b)
            assert int(torch.argmin(r)) == idx                  # the first index among equal values
            assert bool((r[V:] == r[0]).all())


def test_special_transform_cases():
    a, margins = u.broadcast_scales_case()
    for b in range(a['vertices'].shape[0]):
        idx, m = u.margin64(a, b)
        assert idx == u.PTF_CASES['v4097'][3][b] and m == margins[b] and m >= u.MIN_MARGIN
        assert torch.equal(a['scales'][b], a['scales'][0])
    a = u.nan_case()
    r = u.ptf_ratios64(a, 0)
    assert bool(torch.isnan(r[u.NAN_VERTEX])) and int(torch.isnan(r).sum()) == 1
    assert u.margin64(a, 0)[1] >= u.MIN_MARGIN and u.margin64(a, 0)[0] != u.NAN_VERTEX
    a = u.diagonal_case()
    idx, m = u.margin64(a, 0)
    assert idx == u.DIAG_VERTEX and m >= u.MIN_MARGIN
    out = u.ptf_elementwise(zooms=torch.ones(1, 1), **{k: a[k] for k in ('vertices', 'scales', 'rotations', 'translations')})
    x, y = out[0, u.DIAG_VERTEX, 0], out[0, u.DIAG_VERTEX, 1]
    assert float(x) == float(y) == 16.0                         # |x| == |y| in float32 as well, both positive


def test_chain_case_has_its_argmin_on_vertex_0_of_the_padded_template():
    coeffs, pose = u.chain_case()
    (i0, m0), (i1, m1) = u.chain_margins(coeffs, pose)
    assert i0 == 0 and m0 >= u.MIN_MARGIN
    assert m1 >= u.MIN_MARGIN
    assert u.BANK_NVERTS[u.CHAIN_CLASSES[0]] < max(u.BANK_NVERTS)


def test_torch_tie_semantics_the_tie_cases_rely_on():
    x = torch.tensor([[3.0, 1.0, 2.0, 1.0, 1.0]], dtype=torch.float64, requires_grad=True)
    v, i = x.min(dim=1)
    assert int(i) == 1
    v.sum().backward()
    assert x.grad.tolist() == [[0.0, 1.0, 0.0, 0.0, 0.0]]     # min(dim): the first index among equal values takes the gradient
    a = torch.tensor([2.0, 5.0], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([2.0, 1.0], dtype=torch.float64, requires_grad=True)
    torch.max(a, b).sum().backward()
    assert a.grad.tolist() == [0.5, 1.0] and b.grad.tolist() == [0.5, 0.0]   # max(a, b): an even split where a == b


@pytest.mark.parametrize('n', u.POSE_N)
@pytest.mark.parametrize('training', [False, True])
def test_pose_cases_have_alphas_next_to_both_ends(n, training):
    base = u.pose_inputs(n, training)
    out, _, _ = u.pose_run(base, training, 'cpu', torch.float64)
    alpha = out['_alphas'].reshape(-1)
    for i, d in u.pose_planted(n).items():
        end = math.pi if d > 0 else -math.pi
        assert abs(float(alpha[i]) - end) <= 1e-3 or abs(float(alpha[i]) + end) <= 1e-6, (i, d, float(alpha[i]))
        assert abs(math.sin(float(alpha[i]) - (end - d))) <= 1e-6
    assert bool(((alpha >= -math.pi) & (alpha <= math.pi)).all())


def test_gradcheck_of_the_float64_references():
    gc = torch.autograd.gradcheck
    g = torch.Generator().manual_seed(1)
    a = u.ptf_inputs(2, 5, 11, distinct_persp=True)
    d = lambda k: a[k].double().requires_grad_(True)   # noqa: E731
    fit = lambda v, s, q, t, p, z: u.ptf_elementwise(vertices=v, scales=s, rotations=q, translations=t,   # noqa: E731
                                                     perspective_translations=p, zoom_tos=z)
    assert gc(fit, (d('vertices'), d('scales'), d('rotations'), d('translations'), d('perspective_translations'), d('zoom_tos')))
    given = lambda v, s, q, t, p, z: u.ptf_elementwise(vertices=v, scales=s, rotations=q, translations=t,   # noqa: E731
                                                       perspective_translations=p, zooms=z)
    zooms = (torch.rand(2, 1, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    assert gc(given, (d('vertices'), d('scales'), d('rotations'), d('translations'), d('perspective_translations'), zooms))
    # FFD.forward in float64 on a tiny template, with the models' constraints
    from derender3d.models.transforms import FFD
    ffd = FFD(torch.rand(6, 3, generator=g) * 0.9 - 0.45, constraints=u.model_constraints()).double()
    assert gc(ffd, ((torch.randn(192, generator=g, dtype=torch.float64) * 0.05).requires_grad_(True),))
    # the einsum decode and the constraint map
    Bt = torch.rand(2, 5, 4, generator=g, dtype=torch.float64)
    cls = torch.tensor([1, 0, 1])
    assert gc(lambda P: torch.einsum('bcj,bjv->bvc', P, Bt[cls]), (torch.randn(3, 3, 5, generator=g, dtype=torch.float64).requires_grad_(True),))
    # the silhouette loss expression
    ign = (torch.rand(7, generator=g) > 0.5).double()
    tgt = (torch.rand(7, generator=g) > 0.5).double()

    def sil(m, f):
        return torch.mean((torch.nn.functional.mse_loss(m, tgt, reduction='none') + 100 * torch.mean(f ** 2)) * (1 - ign))
    assert gc(sil, (torch.rand(7, generator=g, dtype=torch.float64).requires_grad_(True),
                    (torch.randn(6, generator=g, dtype=torch.float64) * 0.05).requires_grad_(True)))
    # Derenderer3d._pose, both modes, away from the wrap of alpha
    from derender3d.models import Derenderer3d
    for training in (False, True):
        base = {k: v.double() for k, v in u.pose_inputs(3, training).items()}
        base['_theta_deltas'] = torch.tensor([[1.0, 0.3], [-0.4, 0.9], [0.2, -1.1]], dtype=torch.float64)

        def pose(delta, ls, ld, t2):
            blob = dict(base)
            blob.update(_theta_deltas=delta, _log_scales=ls, _log_depths=ld, _translation2ds=t2)
            P = Derenderer3d._pose(u.pose_self(training), blob)
            return tuple(P[k] for k in u.POSE_OUTS)
        assert gc(pose, tuple(base[k].clone().requires_grad_(True) for k in u.POSE_PARAMS))


def test_reference_wrappers_agree_with_their_plain_expressions():
    """ptf_reference with a vertex left out of the minimum equals the plain expression when that vertex is not the argmin; the
    functional's gradients are those of autograd on the plain expression"""
    a, _ = u.ptf_case('v64')
    one = {k: (v[:1].clone() if k != 'zoom_tos' else v[:1].clone()) for k, v in a.items()}
    o1, z1, g1 = u.ptf_reference(one, torch.float64)
    o2, z2, g2 = u.ptf_reference(one, torch.float64, skip=(0, 5))     # the argmin of object 0 is vertex 0
    assert torch.equal(z1, z2) and torch.allclose(o1, o2, rtol=0, atol=0)
    for k in g1:
        assert torch.allclose(g1[k], g2[k], rtol=1e-12, atol=1e-12), k
    # silhouette loss: value against a hand-written sum
    m, t, ign, f = u.sil_inputs(5)
    loss, gm, gf = u.sil_reference(m, t, ign, f, torch.float64)
    c = 100 * float((f.double() ** 2).mean())
    want = sum((float(m[i]) - float(t[i])) ** 2 * (1 - float(ign[i])) + c * (1 - float(ign[i])) for i in range(5)) / 5
    assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want))
    assert torch.allclose(gf, u.SIL_SCALE * 200 * f.double() * (1 - ign.double()).mean() / f.numel(), rtol=1e-12, atol=0)
