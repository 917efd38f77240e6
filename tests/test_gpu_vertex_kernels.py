"""The vertex-side kernels of the renderer (csrc/geometry.hip) against explicit float32 / float64 references at every block edge
of their launch geometry, and the branch matrix of sdn_render_maps_fwd / _bwd (csrc/raster_maps.hip) against the oracle.
Cases, inputs, references and the self-calibrating gates: tests/vertex_kernels_util.py (checked on the CPU by
tests/test_vertex_kernels_host.py).

A. ops.ProjectVertices, ops.GatherFaces, ops.FaceNormals: every forward is bit-equal to the float32 reference; every backward
   is compared with the float64 reference under gate(FLOOR_GRAD, e32) -- and bit for bit where the sums are exact.
B. the one-call path: four scenes x the gradient of the silhouette, the normal map, the depth map and all three, against the
   oracle composed from the pieces of oracle/nr_oracle.py; and the two C entry points called on buffers filled with 0xFF bytes
   (every float a NaN), which makes a read of a row the call itself did not write show up in the result.
Every test prints e32, its gate and the measured error (profiles/vertex_kernels.md holds the table of an MI355X run)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vertex_kernels_util as u
from util import biteq

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

PROJECT_GRID = [(bs, nv, mode, w, flip) for (bs, nv) in u.PROJECT_SHAPES for mode in u.PROJECT_MODES for w in (False, True)
                for flip in (0, 1)]


def dev(t):
    return None if t is None else t.to(DEV)


def np32(t):
    return t.detach().cpu().numpy()


def poison(*nbytes):
    """NaN-filled blocks of the sizes an op is about to ask for, freed at once: its `torch.empty` buffers come back holding NaN"""
    blocks = [torch.full(((int(b) + 3) // 4,), float('nan'), device=DEV) for b in nbytes if b]
    del blocks


def gpu_project(c):
    from sdn_hip import ops
    v = c['verts'].to(DEV).requires_grad_(True)
    poison(v.numel() * 4, v.numel() * 4)
    out = ops.ProjectVertices.apply(v, c['mode'], dev(c['eye']), dev(c['direction']), dev(c['up']), dev(c['width']), c['flip_x'])
    poison(v.numel() * 4)
    out.backward(c['grad'].to(DEV))
    return out.detach().cpu(), v.grad.cpu()


def check_project(c, case):
    out, gv = gpu_project(c)
    assert biteq(np32(out), np32(u.project_fwd(*u.project_args(c)))), case
    g64 = u.project_bwd(*u.project_args(c), c['grad'], torch.float64)
    g32 = u.project_bwd(*u.project_args(c), c['grad'], torch.float32)
    assert torch.isfinite(gv).all()
    u.check_gate('project', case, 'd vertices', gv, g64, g32, u.FLOOR_GRAD)
    return out, gv


@pytest.mark.parametrize('bs,nv,mode,w,flip', PROJECT_GRID)
def test_project_forward_and_backward(bs, nv, mode, w, flip):
    """k_project / k_project_bwd, one thread per vertex in blocks of 256: one vertex, 255, 256, 257, three items of 257 (the batch
    boundaries fall inside blocks) and two of 1025, in every camera mode, with and without a half-width per item, with and
    without the x flip.  eye, direction / at and up differ per item."""
    c = u.project_case(bs, nv, mode, w, flip)
    u.assert_depth_range(c)
    check_project(c, 'bs%d_nv%d_mode%d_w%d_flip%d' % (bs, nv, mode, w, flip))


def test_project_up_parallel_to_the_viewing_direction():
    """cross(up, z) is exactly zero: both other axes are the zero vector, x and y come out exactly 0, the gradient is finite"""
    for c in u.project_parallel_up_case():
        out, gv = check_project(c, 'parallel_up_mode%d' % c['mode'])
        assert (out[..., :2] == 0).all() and (out[..., 2] >= 1).all()
        assert float(gv.abs().max()) > 0


@pytest.mark.parametrize('fill_back', [False, True])
@pytest.mark.parametrize('nf0,bs,shared', u.GATHER_CASES)
def test_gather_forward_and_backward(nf0, bs, shared, fill_back):
    """k_gather_faces / k_gather_faces_bwd, one thread per face in blocks of 256: per-item index lists and one shared
    [1, nf0, 3] list (stride 0), with and without the fill_back twin; vertex 0, the last vertex, a hub vertex in >= 300 faces,
    vertices in no face and faces with repeated vertices are planted.  Integer-valued gradients make every partial sum exact in
    float32 in any order: the atomics must reproduce the index-add bit for bit, which also pins the twin's 2 - k mapping."""
    from sdn_hip import ops
    c = u.gather_case(nf0, bs, shared, fill_back)
    case = 'nf%d_bs%d_%s_fb%d' % (nf0, bs, 'shared' if shared else 'own', fill_back)
    v = c['verts'].to(DEV).requires_grad_(True)
    nf = 2 * nf0 if fill_back else nf0
    poison(bs * nf * 36)
    out = ops.GatherFaces.apply(v, c['faces_idx'].to(DEV), fill_back)
    assert biteq(np32(out), np32(u.gather_fwd(c['verts'], c['faces_idx'], fill_back))), case
    poison(v.numel() * 4)
    out.backward(c['grad_int'].to(DEV), retain_graph=True)
    gi = v.grad.cpu()
    ref = u.gather_bwd(c['grad_int'], c['faces_idx'], u.GATHER_NV, fill_back, torch.float32)
    assert torch.equal(gi, ref), (case, float((gi - ref).abs().max()))
    v.grad = None
    poison(v.numel() * 4)
    out.backward(c['grad'].to(DEV))
    gv = v.grad.cpu()
    u.check_gate('gather', case, 'd vertices', gv, u.gather_bwd(c['grad'], c['faces_idx'], u.GATHER_NV, fill_back, torch.float64),
                 u.gather_bwd(c['grad'], c['faces_idx'], u.GATHER_NV, fill_back, torch.float32), u.FLOOR_GRAD)
    unused = list(u.GATHER_UNUSED)
    assert (gi[:, unused] == 0).all() and (gv[:, unused] == 0).all()


@pytest.mark.parametrize('family', u.NORMALS_FAMILIES)
@pytest.mark.parametrize('n', u.NORMALS_COUNTS)
def test_face_normals_forward_and_backward(n, family):
    """k_face_normals / k_face_normals_bwd, one thread per face in blocks of 256, on exactly representable coordinates (k / 64:
    the cross product is exact, e32 is tiny, the gate is its floor) and on normal-distributed faces (the gate follows e32).
    Planted faces with three equal and with three collinear vertices: the forward is the exact zero vector, the backward is
    finite and follows the documented rule g_c = g_n / eps; those rows are gated on their own as well, since their gradients
    are 1e5 times larger than the others'."""
    from sdn_hip import ops
    c = u.normals_case(n, family)
    case = 'n%d_%s' % (n, family)
    f = c['faces'].to(DEV).requires_grad_(True)
    poison(n * 12)
    out = ops.FaceNormals.apply(f)
    assert biteq(np32(out), np32(u.normals_fwd(c['faces']))), case
    degenerate = c['equal'] + c['collinear']
    assert (out[0, degenerate] == 0).all()
    poison(n * 36)
    out.backward(c['grad'].to(DEV))
    gf = f.grad.cpu()
    assert torch.isfinite(gf).all()
    g64 = u.normals_bwd(c['faces'], c['grad'], torch.float64)
    g32 = u.normals_bwd(c['faces'], c['grad'], torch.float32)
    regular = [i for i in range(n) if i not in degenerate]
    u.check_gate('normals', case, 'd faces', gf, g64, g32, u.FLOOR_GRAD)
    if regular:
        u.check_gate('normals', case, 'd faces, regular rows', gf[0, regular], g64[0, regular], g32[0, regular], u.FLOOR_GRAD)
    if c['collinear']:
        u.check_gate('normals', case, 'd faces, collinear rows', gf[0, c['collinear']], g64[0, c['collinear']], g32[0, c['collinear']],
                     u.FLOOR_GRAD)
    assert (gf[0, c['equal']] == 0).all()


# ------------------------------------------------------------------------------------------ B: sdn_render_maps_fwd / _bwd
NEAR, FAR, EPS, EPS_ALPHA = 0.1, 100.0, 1e-3, 1e-4      # nr.Renderer's near / far / rasterizer_eps; rasterize_silhouettes' eps
BG = (0.0, 0.0, 0.0)


def rel_l2(a, b):
    return u.rel_l2(a, b)


def close_maps(h, o):
    import test_gpu_renderer
    test_gpu_renderer.close_maps(np32(h), np32(o))


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(maps, leaf) of the oracle for one scene, computed once; gradients are taken per subset with torch.autograd.grad"""
    s = u.maps_scene(name)
    vo = s['verts'].clone().requires_grad_(True)
    return u.oracle_maps(s, vo), vo


def oracle_grad(name, which):
    maps, vo = oracle_run(name)
    return torch.autograd.grad(u.maps_loss(maps, which), vo, retain_graph=True)[0]


def hip_run(name, which):
    """RenderMapsFn on one scene: (maps, vertex gradient of the functional of the maps in `which`) on the CPU"""
    from sdn_hip import ops
    s = u.maps_scene(name)
    v = s['verts'].to(DEV).requires_grad_(True)
    maps = ops.RenderMapsFn.apply(v, s['faces_idx'].to(DEV), s['fill_back'], s['mode'], dev(s['eye']), dev(s['direction']), dev(s['up']),
                                  dev(u.maps_width(s)), True, u.MAPS_R, True, NEAR, FAR, EPS, EPS_ALPHA, BG, True, True)
    u.maps_loss(maps, which, to=dev).backward()
    return tuple(m.detach().cpu() for m in maps), v.grad.cpu()


def stable_signs(g_ref):
    """x components whose sign no admissible error can turn: the gradient gate allows an error of 1e-4 |g|_2 <= 1e-4 sqrt(N) max|g|
    (2.2e-3 max|g| at N = 468 components) in all, so a component of at least 1e-2 max|g| keeps its sign in either precision"""
    gx = g_ref[..., 0]
    return gx.abs() >= 1e-2 * float(g_ref.abs().max())


@pytest.mark.parametrize('which', u.MAPS_SUBSETS)
@pytest.mark.parametrize('name', u.MAPS_CASES)
def test_render_maps_branches_against_the_oracle(name, which):
    """The one-call path on two objects with a pose, a camera and a viewing angle each -- default, fill_back off, one shared
    [1, nf0, 3] index list, and camera mode look_at -- with the silhouette ('m': the VertexSink branch), the normal map ('n': the
    second gather, with flip_x and sx = -1), the depth map ('d': no `visible` flags) and all three differentiated.  Maps under
    close_maps, the vertex gradient within 1e-4 relative L2 of the oracle's -- for 'n' and 'd' that is the
    branch's own gradient, not a sum the silhouette term dominates.  Vertices no face references get exactly 0, and the x
    components of the normal-map gradient carry the oracle's signs."""
    (ao, no_, do), _ = oracle_run(name)
    (a, n, d), g = hip_run(name, which)
    close_maps(a, ao)
    close_maps(n, no_)
    close_maps(d, do)
    go = oracle_grad(name, which)
    err = rel_l2(g, go)
    print('render_maps | %s | d %s: gate 1.000e-04 measured %.3e (|g| %.3e)' % (name, which, err, float(go.norm())))
    assert torch.isfinite(g).all() and float(go.norm()) > 0
    assert err < 1e-4, (name, which, err)
    nv_mesh = u.maps_scene(name)['nv_mesh']
    assert (go[:, nv_mesh:] == 0).all() and (g[:, nv_mesh:] == 0).all()
    if which == 'n':
        keep = stable_signs(go)
        assert int(keep.sum()) >= 20, int(keep.sum())
        assert torch.equal(torch.sign(g[..., 0][keep]), torch.sign(go[..., 0][keep]))


def ff_bytes(n):
    return torch.full((max(int(n), 4),), 255, dtype=torch.uint8, device=DEV)


def ff_floats(*shape):
    return ff_bytes(4 * int(np.prod(shape))).view(torch.float32).reshape(shape)


def raw_run(name, which):
    """sdn_render_maps_fwd / _bwd through the C ABI on buffers this test owns, every byte 0xFF beforehand: state, forward
    scratch, backward workspace, the three maps and the vertex gradient"""
    import sdn_hip
    from sdn_hip import AA, DEPTH, RGB, SAVE_MAPS, check, lib, ptr, stream
    s = u.maps_scene(name)
    v, f = s['verts'].to(DEV), s['faces_idx'].to(DEV)
    bs, nv = v.shape[:2]
    nf0 = f.shape[1]
    stride = 0 if f.shape[0] == 1 else nf0 * 3
    fill_back, R = int(s['fill_back']), u.MAPS_R
    flags = RGB | DEPTH | AA | SAVE_MAPS
    nstate, nbwd, nscr = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib().sdn_render_maps_bytes(bs, nv, nf0, fill_back, R, flags, ctypes.byref(nstate), ctypes.byref(nbwd), ctypes.byref(nscr)))
    state, scratch, ws = ff_bytes(nstate.value), ff_bytes(nscr.value), ff_bytes(nbwd.value)
    alpha, normal, depth, gv = ff_floats(bs, R, R), ff_floats(bs, 3, R, R), ff_floats(bs, R, R), ff_floats(bs, nv, 3)
    for t in (alpha, normal, depth, gv):
        assert torch.isnan(t).all()
    eye, direction, up, width = dev(s['eye']), dev(s['direction']), dev(s['up']), dev(u.maps_width(s))
    bg = sdn_hip.const_f32(BG, v.device)
    check(lib().sdn_render_maps_fwd(ptr(v), bs, nv, ptr(f), nf0, stride, fill_back, s['mode'], ptr(eye), ptr(direction), ptr(up),
                                    ptr(width), 1, R, flags, NEAR, FAR, EPS, ptr(bg), ptr(alpha), ptr(normal), ptr(depth),
                                    ptr(state), nstate.value, ptr(scratch), nscr.value, stream()))
    w = {k: t.to(DEV).contiguous() for k, t in u.maps_weights().items()}
    g = {k: (w[k] if k in which else None) for k in 'mnd'}
    check(lib().sdn_render_maps_bwd(ptr(v), bs, nv, ptr(f), nf0, stride, fill_back, s['mode'], ptr(eye), ptr(direction), ptr(up),
                                    ptr(width), 1, R, flags, EPS, EPS_ALPHA, ptr(bg), ptr(g['m']), ptr(g['n']), ptr(g['d']), ptr(gv),
                                    ptr(state), nstate.value, ptr(ws), nbwd.value, stream()))
    torch.cuda.synchronize()
    return (alpha.cpu(), normal.cpu(), depth.cpu()), gv.cpu()


@pytest.mark.parametrize('which', u.MAPS_SUBSETS)
@pytest.mark.parametrize('name', ['default', 'fill_back_off'])
def test_render_maps_on_buffers_of_nan(name, which):
    """The contracts of the one-call path that only unwritten memory can break: the forward is lazy (weight and colour maps of
    `state` stay unwritten until the backward re-derives them), the sparse gradient rows of invisible faces stay unwritten and
    k_gather_faces_bwd is steered past them by `visible`, which the depth-only branch does without.  With every buffer NaN
    beforehand, all outputs are finite, the maps equal RenderMapsFn's bit for bit, the gradient agrees with RenderMapsFn's within
    the float-atomics bound 1e-6 of the fused-against-composed test, and vertices no face references get exactly 0."""
    maps, g = raw_run(name, which)
    ref_maps, ref_g = hip_run(name, which)
    for m, r, k in zip(maps, ref_maps, ('alpha', 'normal', 'depth')):
        assert torch.isfinite(m).all(), k
        assert biteq(np32(m), np32(r)), k
    assert torch.isfinite(g).all(), int((~torch.isfinite(g)).sum())
    err = rel_l2(g, ref_g)
    print('render_maps on NaN buffers | %s | d %s: bound 1.000e-06 measured %.3e' % (name, which, err))
    assert err <= 1e-6, (name, which, err)
    nv_mesh = u.maps_scene(name)['nv_mesh']
    assert (g[:, nv_mesh:] == 0).all()
