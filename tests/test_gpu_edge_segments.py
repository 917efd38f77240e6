"""k_edge_segments -- the frame step's sum of the silhouette edge chunks per (face, edge, axis) run of chunk records, straight
onto the vertices (sdn_render_maps_bwd with only the silhouette differentiated) -- against the dense route it does not
touch: sdn_rasterize_bwd writes one gradient row per face (k_chunk_sum + k_edge_reduce, deterministic), the rows are
gathered to the vertices HERE, on the host, in float64, and pushed through the projection's backward.

Gate: relative L2 <= 1e-6, the gate of test_fused_render_maps_equals_the_composed_functions for vertex gradients that meet
in float atomics (the sums per run of chunks are formed in the dense route's order; what differs is where the two edges
that share a vertex coordinate meet: in a register there, in the atomic here).

Every scene is the smallest that reaches its condition, and the condition is CHECKED on the chunk plan read back from the
dense route's workspace (k_edge_plan writes the same records for both routes: same faces, same visible flags)."""
import functools

import numpy as np
import pytest
import torch

from sdn_hip import synth
from util import posed_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-6


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def read_plan(ws, bs, nf, S):
    """(counter, cap, chunk_base [bs*nf], chunk records [min(counter, cap), 4]) from a workspace of sdn_rasterize_bwd
    (bwd_layout of csrc/raster_bwd.hip)."""
    a256 = lambda n: (n + 255) // 256 * 256
    n = bs * nf
    cap = 4 * n + 65536
    off_rowcnt = 256 + a256(n * 4)
    off_base = off_rowcnt + a256(4 * bs * S * 4)
    off_desc = off_base + a256(n * 4)
    raw = ws.cpu().numpy()
    counter = int(raw[0:4].view(np.uint32)[0])
    base = raw[off_base:off_base + n * 4].view(np.int32).copy()
    desc = raw[off_desc:off_desc + min(counter, cap) * 16].view(np.uint32).reshape(-1, 4).copy()
    return counter, cap, base, desc


def segments(desc, n):
    """(first slot, length, face) of every run of valid records with equal {face, e}; number of invalid slots."""
    valid = desc[:, 0] < n
    key = np.where(valid, desc[:, 0].astype(np.int64) * 8 + desc[:, 1].astype(np.int64), -1 - np.arange(len(desc), dtype=np.int64))
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    length = np.diff(np.r_[start, len(key)])
    keep = valid[start]
    return start[keep], length[keep], desc[start[keep], 0].astype(np.int64), int((~valid).sum())


def both_routes(verts, faces, R, ang, fill_back=True, seed=3):
    """Vertex gradient of sum(mask * w) by the fused call (vertex sink) and by the dense route + float64 host gather."""
    from derender3d.models import renderer as rmod
    from neural_renderer.rasterize import DEFAULT_EPS
    from sdn_hip import ops
    bs, nv = verts.shape[:2]
    r = rmod.Renderer(image_size=R)
    r.viewing_angle = [ang] * bs if bs > 1 else ang
    fi = torch.tensor(np.ascontiguousarray(faces), device=DEV)
    g = torch.Generator(device='cuda').manual_seed(seed)
    w = torch.randn((bs, 1, R, R), generator=g, device=DEV)
    bag = rmod._defaults()
    saved = bag.fill_back
    bag.fill_back = fill_back
    try:
        vt = torch.tensor(verts, device=DEV, requires_grad=True)
        m, _, _ = r.render_maps(vt, fi, normal=False, depth=False)
        (m * w).sum().backward()
        fused = vt.grad.cpu().numpy()
    finally:
        bag.fill_back = saved
    # the dense route: project and gather as autograd Functions, rasterize with a leaf in between whose gradient is
    # sdn_rasterize_bwd's [bs, nf, 3, 3] rows
    vo = torch.tensor(verts, device=DEV, requires_grad=True)
    nr_, vflip = r._setup(vo)
    nr_.fill_back = fill_back
    proj = nr_.project(vflip)
    faces9 = nr_.gather(proj, fi).detach().requires_grad_(True)
    captured = {}
    real = ops.raster_bwd_workspace

    def grab(b, nf, S, device):
        captured['ws'], captured['dims'] = real(b, nf, S, device), (b, nf, S)
        return captured['ws']
    ops.raster_bwd_workspace = grab
    try:
        _, alpha, _ = ops.RasterizeMaps.apply(faces9, None, nr_.image_size, nr_.anti_aliasing, nr_.near, nr_.far, nr_.rasterizer_eps,
                                              nr_.background_color, False, True, False, DEFAULT_EPS, True)
        (alpha[:, None] * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.raster_bwd_workspace = real
    assert torch.equal(alpha[:, None], m), 'the two routes rasterized different masks'
    rows = faces9.grad.cpu().numpy().astype(np.float64)          # [bs, nf, 3, 3]
    nf0 = faces.shape[1]
    idx = np.broadcast_to(faces, (bs, nf0, 3))
    gp = np.zeros((bs, nv, 3), np.float64)
    for b in range(bs):
        np.add.at(gp[b], idx[b], rows[b, :nf0])
        if fill_back:                                           # face nf0 + f is face f with its vertices reversed
            np.add.at(gp[b], idx[b, :, ::-1], rows[b, nf0:])
    proj.backward(torch.tensor(gp, dtype=torch.float32, device=DEV))
    b_, nf, S = captured['dims']
    counter, cap, base, desc = read_plan(captured['ws'], b_, nf, S)
    return {'fused': fused, 'dense': vo.grad.cpu().numpy(), 'counter': counter, 'cap': cap, 'base': base, 'desc': desc,
            'n': b_ * nf, 'nf': nf, 'nf0': nf0, 'S': S, 'faces': faces}


def with_corner_marks(v, f, at=1.5):
    """Two tiny triangles in opposite corners: posed_mesh zooms the whole mesh to the image, they keep the rest off its border."""
    n = len(v)
    v = np.concatenate([v, [[at - 0.05, at - 0.05, 0], [at, at - 0.05, 0], [at, at, 0],
                            [-at, -at, 0], [-at + 0.05, -at, 0], [-at + 0.05, -at + 0.05, 0]]])
    f = np.concatenate([f, [[n, n + 1, n + 2], [n + 3, n + 4, n + 5]]])
    return v.astype(np.float32), f.astype(np.int32)


def panel_mesh(rng, cells, jitter, z_jitter=0.05, backdrop=True):
    """cells x cells jittered quads (two large triangles each) in the plane z = 0, in front of one triangle larger than all of
    them."""
    k = cells + 1
    gx, gy = np.meshgrid(np.linspace(-1, 1, k), np.linspace(-1, 1, k), indexing='ij')
    v = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3)
    v[:, :2] += rng.uniform(-jitter, jitter, (len(v), 2)) * (2.0 / cells)
    v[:, 2] += rng.uniform(-z_jitter, z_jitter, len(v))
    f = []
    for i in range(cells):
        for j in range(cells):
            a, b, c, d = i * k + j, (i + 1) * k + j, (i + 1) * k + j + 1, i * k + j + 1
            f += [(a, b, c), (a, c, d)]
    if backdrop:
        n = len(v)
        v = np.concatenate([v, [[-1.5, -1.3, -0.5], [1.5, -1.1, -0.5], [0.1, 1.5, -0.5]]])
        f.append((n, n + 1, n + 2))
    return v.astype(np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in ('car', 'car_no_fill_back'):
        v, f = synth.car_like(3000, seed=5)
        pv, ang = posed_mesh(v, f, render_size=96)
        return both_routes(pv, f[None], 96, ang, fill_back=(name == 'car'))
    if name == 'panels':
        v, f = panel_mesh(np.random.default_rng(11), 3, 0.3)
        pv, ang = posed_mesh(v, f, theta=0.25, scale=(1, 1, 1), translation=(0.4, -0.3, -9.0), render_size=192)
        return both_routes(pv, f[None], 192, ang)
    if name == 'axis_aligned':
        # un-jittered, un-rotated quads: their vertical and horizontal edges have (edge, axis) walks without a single pixel
        v, f = with_corner_marks(*panel_mesh(np.random.default_rng(12), 3, 0.0, z_jitter=0.0, backdrop=False))
        pv, ang = posed_mesh(v, f, theta=0.0, scale=(1, 1, 1), translation=(0.0, 0.0, -9.0), render_size=96)
        return both_routes(pv, f[None], 96, ang)
    if name == 'strips':
        # 300 slightly tilted strips, 1.5 pixels high with a pixel of background between them and ~690 pixels long, none hiding
        # another: ~175 chunks per triangle
        rng = np.random.default_rng(13)
        ns = 300
        y0 = np.linspace(-1.4, 1.4, ns + 1)
        v, f = [], []
        for s in range(ns):
            lo, hi = y0[s], y0[s] + 0.6 * (y0[s + 1] - y0[s])
            t = rng.uniform(-0.0008, 0.0008)
            n = len(v)
            v += [(-1.35, lo - t, 0), (1.35, lo + t, 0), (1.35, hi + t, 0), (-1.35, hi - t, 0)]
            f += [(n, n + 1, n + 2), (n, n + 2, n + 3)]
        v, f = with_corner_marks(np.asarray(v, np.float32), np.asarray(f, np.int32))
        pv, ang = posed_mesh(v, f, theta=0.0, scale=(1, 1, 1), translation=(0.0, 0.0, -9.0), render_size=384)
        return both_routes(pv, f[None], 384, ang)
    if name == 'two_objects':
        va, fa = synth.car_like(3000, seed=5)
        vb, fb = synth.car_like(3000, seed=6)
        assert va.shape == vb.shape and fa.shape == fb.shape
        pa, ang = posed_mesh(va, fa, render_size=96)
        pb, _ = posed_mesh(vb, fb, theta=2.1, render_size=96)
        perm = np.random.default_rng(14).permutation(len(fb))
        return both_routes(np.concatenate([pa, pb]), np.stack([fa, fb[perm]]), 96, ang)
    raise KeyError(name)


def check_gradient(s):
    assert np.isfinite(s['fused']).all()
    assert np.linalg.norm(s['dense']) > 0
    rel = rel_l2(s['fused'], s['dense'])
    print('relative L2 fused vs dense route: %.3e' % rel)
    assert rel <= GATE, rel


@pytest.mark.parametrize('name', ['car', 'car_no_fill_back'])
def test_short_segments_and_both_index_paths(name):
    s = scene(name)
    start, length, face, invalid = segments(s['desc'], s['n'])
    print('%d chunks in %d segments, mean length %.2f' % (len(s['desc']), len(length), length.mean()))
    assert s['counter'] <= s['cap'] and invalid == 0
    assert len(length) > 1000 and np.median(length) <= 2
    assert (s['nf'] == 2 * s['nf0']) == (name == 'car')
    check_gradient(s)


def test_long_segments_across_wave_and_block_boundaries():
    s = scene('panels')
    start, length, face, invalid = segments(s['desc'], s['n'])
    end = start + length - 1
    print('%d chunks, segment lengths: median %d, max %d' % (len(s['desc']), np.median(length), length.max()))
    assert s['counter'] <= s['cap'] and invalid == 0
    assert (length > 8).sum() >= 20                              # more than one round of eight chunks
    assert ((start // 64 != end // 64) & (length > 8)).sum() >= 5    # carried past the wave's last lane
    assert (start // 256 != end // 256).sum() >= 1               # ... and past the workgroup's
    assert (end - (start // 64 * 64 + 63) > 8).any()            # ... for more than one batch of eight
    check_gradient(s)


def test_an_empty_walk_between_two_segments_of_a_face():
    s = scene('axis_aligned')
    start, length, face, invalid = segments(s['desc'], s['n'])
    has = np.zeros(s['n'], np.int64)
    np.bitwise_or.at(has, s['desc'][:, 0].astype(np.int64), 1 << s['desc'][:, 1].astype(np.int64))
    has = has[has != 0]
    # a walk without chunks below one that has some: the next segment of the face follows directly
    gap = np.array([any(not (h >> e) & 1 and (h >> (e + 1)) != 0 for e in range(5)) for h in has])
    print('%d faces with chunks, %d with an empty walk in front of a later one' % (len(has), gap.sum()))
    assert gap.sum() >= 4
    check_gradient(s)


def test_overflow_faces_take_the_serial_walk_and_their_slots_add_nothing():
    s = scene('strips')
    start, length, face, invalid = segments(s['desc'], s['n'])
    serial = np.flatnonzero(s['base'] == -1)
    print('counter %d, cap %d, %d serial faces, %d invalid slots, longest segment %d' % (s['counter'], s['cap'], len(serial), invalid,
                                                                                         length.max()))
    assert s['counter'] > s['cap'] and len(serial) >= 20
    assert invalid > 0                        # a face's reservation straddled the cap: its slots below it are marked invalid
    assert length.max() > 64                  # (a segment longer than a wave as well)
    check_gradient(s)
    # the vertices of the serially walked faces alone, and the vertices no such face touches
    nf0 = s['nf0']
    fidx = s['faces'][0]
    touched = np.zeros(s['fused'].shape[1], bool)
    touched[fidx[serial % s['nf'] % nf0].ravel()] = True
    assert np.linalg.norm(s['dense'][0, touched]) > 0 and np.linalg.norm(s['dense'][0, ~touched]) > 0
    assert rel_l2(s['fused'][0, touched], s['dense'][0, touched]) <= GATE
    assert rel_l2(s['fused'][0, ~touched], s['dense'][0, ~touched]) <= GATE


def test_two_objects_with_their_own_index_lists():
    s = scene('two_objects')
    assert s['counter'] <= s['cap']
    check_gradient(s)
    for b in range(2):   # per object: a face's chunks never add to the other object's vertices
        rel = rel_l2(s['fused'][b], s['dense'][b])
        assert rel <= GATE, (b, rel)
    assert rel_l2(s['fused'][0], s['dense'][1]) > 0.1
