"""The references and case tables of tests/vertex_kernels_util.py, checked on the CPU: the float32 forward formulas are bit-equal to
oracle/nr_oracle.py, the written-out backward formulas equal float64 autograd of plain torch expressions, and every condition
the GPU tests rely on (camera depth, planted indices, exact inputs, degenerate faces, scenes in view) holds for every case."""
import itertools

import pytest
import torch

import vertex_kernels_util as u
from oracle import nr_oracle as no
from util import biteq

PROJECT_GRID = [(bs, nv, mode, w, flip) for (bs, nv) in u.PROJECT_SHAPES for mode in u.PROJECT_MODES for w in (False, True)
                for flip in (0, 1)]


def np32(t):
    return t.detach().numpy()


def oracle_project(c):
    v = c['verts'] * torch.tensor([-1.0, 1.0, 1.0]) if c['flip_x'] else c['verts']
    if c['mode'] == 1:
        v = no.look(v, c['eye'], c['direction'], c['up'])
    elif c['mode'] == 2:
        v = no.look_at(v, c['eye'], c['direction'], c['up'])
    if c['width'] is not None:
        v = torch.cat([no.perspective(v[b:b + 1], angle=c['angles'][b]) for b in range(len(v))])
    return v


def autograd_project(c):
    """float64 autograd of the plain expression: rotation as a matrix product, torch.linalg.cross / norm"""
    v = c['verts'].double().requires_grad_(True)
    o = v * torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64) if c['flip_x'] else v
    if c['mode'] != 0:
        e, d, up = c['eye'].double(), c['direction'].double(), c['up'].double()
        n = lambda x: x / (torch.linalg.norm(x, dim=1, keepdim=True) + 1e-5)   # noqa: E731
        za = n(d - e if c['mode'] == 2 else d)
        xa = n(torch.linalg.cross(up, za))
        ya = n(torch.linalg.cross(za, xa))
        o = torch.einsum('bnk,bjk->bnj', o - e[:, None], torch.stack([xa, ya, za], dim=1))
    if c['width'] is not None:
        w = c['width'].double().reshape(-1, 1)
        o = torch.stack([o[..., 0] / (o[..., 2] * w), o[..., 1] / (o[..., 2] * w), o[..., 2]], dim=-1)
    (o * c['grad'].double()).sum().backward()
    return v.grad


@pytest.mark.parametrize('bs,nv,mode,w,flip', PROJECT_GRID)
def test_project_reference(bs, nv, mode, w, flip):
    c = u.project_case(bs, nv, mode, w, flip)
    u.assert_depth_range(c)
    assert biteq(np32(u.project_fwd(*u.project_args(c))), np32(oracle_project(c)))
    g64 = u.project_bwd(*u.project_args(c), c['grad'], torch.float64)
    assert u.rel_l2(g64, autograd_project(c)) < 1e-13
    g32 = u.project_bwd(*u.project_args(c), c['grad'], torch.float32)
    assert g32.dtype == torch.float32 and u.rel_l2(g32, g64) < 2e-6      # well-conditioned at depth >= 1: the gate is the floor
    if bs > 1 and mode != 0:
        for k in ('eye', 'direction', 'up'):
            assert not torch.equal(c[k][0], c[k][1]), k
    if bs > 1 and w:
        assert len(set(c['width'].tolist())) == bs


def test_project_parallel_up_reference():
    for c in u.project_parallel_up_case():
        u.assert_depth_range(c)
        xa, ya, za, _ = u.camera_basis(c['mode'], c['eye'], c['direction'], c['up'], torch.float32)
        assert (xa == 0).all() and (ya == 0).all() and (za != 0).any()
        out = u.project_fwd(*u.project_args(c))
        assert biteq(np32(out), np32(oracle_project(c)))
        assert (out[..., :2] == 0).all() and (out[..., 2] >= 1).all()
        for dtype in (torch.float32, torch.float64):
            g = u.project_bwd(*u.project_args(c), c['grad'], dtype)
            assert torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_minimum_camera_depth_of_the_project_cases():
    lo = min(u.camera_depth64(u.project_case(*p))[0] for p in PROJECT_GRID)
    hi = max(u.camera_depth64(u.project_case(*p))[1] for p in PROJECT_GRID)
    print('camera depth over the A1 cases: min %.4f max %.4f' % (lo, hi))
    assert u.DEPTH_RANGE[0] <= lo and hi <= u.DEPTH_RANGE[1]


@pytest.mark.parametrize('fill_back', [False, True])
@pytest.mark.parametrize('nf0,bs,shared', u.GATHER_CASES)
def test_gather_reference_and_planted_indices(nf0, bs, shared, fill_back):
    c = u.gather_case(nf0, bs, shared, fill_back)
    idx = c['faces_idx']
    assert idx.shape == ((1 if shared else bs), nf0, 3) and idx.dtype == torch.int32
    assert int(idx.min()) >= 0 and int(idx.max()) < u.GATHER_NV
    full = idx.expand(bs, -1, -1)
    filled = torch.cat((full, full.flip(2)), dim=1) if fill_back else full
    assert biteq(np32(u.gather_fwd(c['verts'], idx, fill_back)), np32(no.vertices_to_faces(c['verts'], filled)))
    for b in range(idx.shape[0]):
        rows = [tuple(r) for r in idx[b].tolist()]
        used = set(itertools.chain.from_iterable(rows))
        assert not used & set(u.GATHER_UNUSED) and len(u.GATHER_UNUSED) >= 5
        assert {0, u.GATHER_NV - 1} <= used
        if nf0 >= 255:
            assert any(r[0] == r[1] != r[2] for r in rows) and any(r[0] == r[1] == r[2] for r in rows)
        if nf0 == 600:
            assert sum(u.GATHER_HUB in r for r in rows) >= 300
            assert {r.index(u.GATHER_HUB) for r in rows if u.GATHER_HUB in r} == {0, 1, 2}
    if not shared and bs > 1 and nf0 > 1:
        assert not torch.equal(idx[0], idx[1]) and not torch.equal(idx[1], idx[2])
    # backward: the index-add equals float64 autograd of the forward; integer gradients sum exactly in float32
    v = c['verts'].double().requires_grad_(True)
    (u.gather_fwd(v, idx, fill_back) * c['grad'].double()).sum().backward()
    assert u.rel_l2(u.gather_bwd(c['grad'], idx, u.GATHER_NV, fill_back, torch.float64), v.grad) < 1e-14
    assert float(c['grad_int'].abs().max()) <= 8 and torch.equal(c['grad_int'], c['grad_int'].round())
    g32 = u.gather_bwd(c['grad_int'], idx, u.GATHER_NV, fill_back, torch.float32)
    assert torch.equal(g32.double(), u.gather_bwd(c['grad_int'], idx, u.GATHER_NV, fill_back, torch.float64))
    assert (g32[:, list(u.GATHER_UNUSED)] == 0).all()


def autograd_normals(faces, grad):
    f = faces.double().requires_grad_(True)
    c = torch.linalg.cross(f[..., 0, :] - f[..., 1, :], f[..., 2, :] - f[..., 1, :])
    y = c / (torch.linalg.norm(c, dim=-1, keepdim=True) + 1e-5)
    (y * grad.double()).sum().backward()
    return f.grad


@pytest.mark.parametrize('family', u.NORMALS_FAMILIES)
@pytest.mark.parametrize('n', u.NORMALS_COUNTS)
def test_normals_reference(n, family):
    c = u.normals_case(n, family)
    f, g = c['faces'], c['grad']
    degenerate = c['equal'] + c['collinear']
    regular = [i for i in range(n) if i not in degenerate]
    assert degenerate and (n == 1 or c['collinear'])
    out = u.normals_fwd(f)
    idx = torch.arange(3 * n, dtype=torch.int32).reshape(1, n, 3)
    assert biteq(np32(out), np32(no.NRRenderer().face_normals(f.reshape(1, 3 * n, 3), idx)))
    assert (out[0, degenerate] == 0).all()                                # the exact zero vector
    for i in c['collinear']:
        assert len({tuple(r) for r in f[0, i].tolist()}) == 3
    for i in c['equal']:
        assert len({tuple(r) for r in f[0, i].tolist()}) == 1
    g64 = u.normals_bwd(f, g, torch.float64)
    g32 = u.normals_bwd(f, g, torch.float32)
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all()
    if regular:
        # away from |c| == 0 the written-out rule is the gradient of c / (|c| + 1e-5) through the cross product
        assert u.rel_l2(g64[0, regular], autograd_normals(f[:, regular], g[:, regular])[0]) < 1e-9
    # at |c| == 0 (autograd: NaN) the documented rule g_c = g_n / eps: zero for three equal vertices, huge but finite on a line
    assert (g64[0, c['equal']] == 0).all()
    for i in c['collinear']:
        gc = g[0, i].double() / 1e-5
        v10, v12 = (f[0, i, 0] - f[0, i, 1]).double(), (f[0, i, 2] - f[0, i, 1]).double()
        g10, g12 = torch.linalg.cross(v12, gc), torch.linalg.cross(gc, v10)
        assert torch.allclose(g64[0, i], torch.stack([g10, -(g10 + g12), g12]), rtol=1e-12, atol=0)
        assert float(g64[0, i].abs().max()) > 1e3
    if family == 'dyadic':
        f64 = f.double()
        c64 = torch.linalg.cross(f64[..., 0, :] - f64[..., 1, :], f64[..., 2, :] - f64[..., 1, :])
        c32 = u.cross3(f[..., 0, :] - f[..., 1, :], f[..., 2, :] - f[..., 1, :])
        assert torch.equal(c32.double(), c64)                             # exact in both precisions
        assert float((f * 64).abs().max()) <= 512 and torch.equal(f * 64, (f * 64).round())
        if regular:
            assert u.rel_l2(g32[0, regular], g64[0, regular]) < 1e-6      # so e32 is small and the gate is the floor


@pytest.mark.parametrize('name', u.MAPS_CASES)
def test_maps_scene_is_in_view_and_has_unreferenced_vertices(name):
    s = u.maps_scene(name)
    bs, nv = s['verts'].shape[:2]
    assert bs == 2 and nv == s['nv_mesh'] + u.MAPS_EXTRA_VERTS
    assert int(s['faces_idx'].max()) == s['nv_mesh'] - 1                   # the appended vertices are in no face
    assert s['faces_idx'].shape[0] == (1 if name == 'shared' else 2)
    if name != 'shared':
        assert not torch.equal(s['faces_idx'][0], s['faces_idx'][1])
    assert s['fill_back'] == (name != 'fill_back_off') and s['mode'] == (2 if name == 'look_at' else 1)
    for k in ('eye', 'direction', 'up'):
        assert not torch.equal(s[k][0], s[k][1])
    p = u.project_fwd(s['verts'], s['mode'], s['eye'], s['direction'], s['up'], u.maps_width(s), 1, torch.float64)
    assert float(p[..., :2].abs().max()) < 0.95 and 1.0 < float(p[..., 2].min()) and float(p[..., 2].max()) < 8.0
    with torch.no_grad():
        alpha, normal, depth = u.oracle_maps(s, s['verts'])
    assert alpha.shape == (2, u.MAPS_R, u.MAPS_R) and normal.shape == (2, 3, u.MAPS_R, u.MAPS_R) and depth.shape == alpha.shape
    cover = alpha.mean(dim=(1, 2))
    assert float(cover.min()) > 0.05 and float(cover.max()) < 0.6, cover
    assert float((alpha[0] - alpha[1]).abs().max()) > 0.5                  # two different views


def test_maps_oracle_equals_the_sdn_renderer_oracle_on_its_defaults():
    """the composition of oracle pieces used for the branch matrix is SDNRenderer's own on the settings SDNRenderer can express:
    mode look, fill_back, one viewing angle, eye 0"""
    s = u.maps_scene('shared')
    s['eye'] = torch.zeros(2, 3)
    s['direction'] = torch.tensor([[0.0, 0.0, -1.0]] * 2)
    s['up'] = torch.tensor([[0.0, 1.0, 0.0]] * 2)
    s['angles'] = (17.0, 17.0)
    v = s['verts'] + torch.tensor([0.0, 0.0, -3.5])
    r = no.SDNRenderer(image_size=u.MAPS_R, viewing_angle=17.0)
    faces = s['faces_idx'].expand(2, -1, -1)
    with torch.no_grad():
        a, n, d = u.oracle_maps(s, v)
        assert float(a.mean()) > 0.02
        assert biteq(np32(a), np32(r(v, faces, render_type=no.RenderType.Silhouette)[:, 0]))
        # (one object per call, as 3D-SDN renders: the reference's batched texture sampling reads item 0's faces for every item)
        normal = torch.cat([r(v[b:b + 1], faces[b:b + 1], render_type=no.RenderType.Normal) for b in range(2)])
        assert biteq(np32(n), np32(normal))
        assert biteq(np32(d), np32(r(v, faces, render_type=no.RenderType.Depth)[:, 0]))
