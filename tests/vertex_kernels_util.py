"""Shared pieces of the vertex-side kernel tests (tests/test_vertex_kernels_host.py, tests/test_gpu_vertex_kernels.py): case tables,
seeded inputs and the float32 / float64 references of csrc/geometry.hip -- k_project, k_gather_faces, k_face_normals and their
backward kernels -- and the scenes of the sdn_render_maps_fwd / _bwd branch matrix (csrc/raster_maps.hip).  Nothing here needs
a GPU.

References.  Every one is a set of explicit formulas evaluated by torch on the CPU in a chosen dtype:
  forward   float32, in the kernels' operation order: sums left to right, no fused multiply-add (torch's element-wise CPU ops
            round after every operation; csrc/geometry.hip is built with -ffp-contract=off), correctly rounded square root
            (numpy).  tests/test_vertex_kernels_host.py pins these bit for bit to oracle/nr_oracle.py; the kernels must be
            bit-equal to them.
  backward  the chain rule written out, evaluated in float64 from the float32 inputs (ref64) and once more in float32 (ref32).
            e32 = rel_l2(ref32, ref64); a kernel's gate is frame_kernels_util.gate(FLOOR_GRAD, e32) = max(2e-5, 4 e32).
            The host test checks the written-out backward formulas against float64 autograd of the forward formulas.
No number is taken from the kernels under test.

Face-normal backward at |c| == 0 (three equal or three collinear vertices): Chainer's normalize gives NaN there; the kernel
documents g_c = g_n / eps with coef = 0, and `normals_bwd` implements exactly that rule.
"""
import functools

import numpy as np
import torch

from frame_kernels_util import FLOOR_GRAD, check_gate, gate, rel_l2  # noqa: F401  (re-exported for the two test modules)

EPS = 1e-5            # chainer.functions.normalize: x / (|x| + 1e-5)
DEPTH_RANGE = (1.0, 8.0)


# ------------------------------------------------------------------------------------------ formulas
def _sqrt(x):
    """correctly rounded square root in the tensor's own dtype (torch's float32 CPU sqrt is off by an ulp on ~1 % of inputs)"""
    return torch.from_numpy(np.sqrt(x.numpy()))


def _norm3(x):
    return _sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])


def normalize3(x):
    return x / (_norm3(x) + EPS)[..., None]


def cross3(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                        a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)


def camera_basis(mode, eye, direction, up, dtype):
    """(xa, ya, za, e), each [bs, 3]: look.py:29-37 (mode 1), look_at.py:30-38 (mode 2: `direction` holds `at`)"""
    e, d, u = eye.to(dtype), direction.to(dtype), up.to(dtype)
    za = normalize3(d - e if mode == 2 else d)
    xa = normalize3(cross3(u, za))
    ya = normalize3(cross3(za, xa))
    return xa, ya, za, e


def _dot_rows(d, a):
    """(d0 a0 + d1 a1) + d2 a2 of [bs, n, 3] points with one [bs, 3] axis per item"""
    a = a[:, None, :]
    return (d[..., 0] * a[..., 0] + d[..., 1] * a[..., 1]) + d[..., 2] * a[..., 2]


def _camera_coords(verts, mode, eye, direction, up, flip_x, dtype):
    v = verts.to(dtype)
    if flip_x:
        v = torch.stack([v[..., 0] * -1.0, v[..., 1], v[..., 2]], dim=-1)
    if mode == 0:
        return v, None
    B = camera_basis(mode, eye, direction, up, dtype)
    d = v - B[3][:, None, :]
    return torch.stack([_dot_rows(d, B[0]), _dot_rows(d, B[1]), _dot_rows(d, B[2])], dim=-1), B


def project_fwd(verts, mode, eye, direction, up, width, flip_x, dtype=torch.float32):
    """k_project: x flip, camera rotation, x / z / w and y / z / w; z stays the camera depth"""
    o, _ = _camera_coords(verts, mode, eye, direction, up, flip_x, dtype)
    if width is not None:
        w = width.to(dtype).reshape(-1, 1)
        o = torch.stack([o[..., 0] / o[..., 2] / w, o[..., 1] / o[..., 2] / w, o[..., 2]], dim=-1)
    return o


def project_bwd(verts, mode, eye, direction, up, width, flip_x, grad_out, dtype):
    """the chain rule of project_fwd with respect to the vertices, written out"""
    o, B = _camera_coords(verts, mode, eye, direction, up, flip_x, dtype)
    g = grad_out.to(dtype)
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    if width is not None:
        w = width.to(dtype).reshape(-1, 1)
        z = o[..., 2]
        gx, gy = g0 / w, g1 / w
        # x' = (ox / oz) / w: d x' / d ox = 1 / (oz w), d x' / d oz = -(ox / oz) / (oz w)
        g2 = g2 - gx * (o[..., 0] / z) / z - gy * (o[..., 1] / z) / z
        g0, g1 = gx / z, gy / z
    if mode != 0:
        xa, ya, za = (a[:, None, :] for a in B[:3])
        t = [(g0 * xa[..., k] + g1 * ya[..., k]) + g2 * za[..., k] for k in range(3)]
        g0, g1, g2 = t
    if flip_x:
        g0 = g0 * -1.0
    return torch.stack([g0, g1, g2], dim=-1)


def _index(faces_idx, bs):
    """the [bs, nf0, 3] long index of a per-item or a shared [1, nf0, 3] list"""
    f = faces_idx.long()
    return f.expand(bs, -1, -1) if f.shape[0] == 1 else f


def gather_fwd(verts, faces_idx, fill_back):
    """k_gather_faces: out[b, f, k] = verts[b, idx[b, f, k]]; the fill_back twin f + nf0 holds the vertices in reverse order"""
    bs = verts.shape[0]
    idx = _index(faces_idx, bs)
    out = torch.stack([verts[b][idx[b]] for b in range(bs)])           # [bs, nf0, 3, 3]
    return torch.cat((out, out.flip(2)), dim=1) if fill_back else out


def gather_bwd(grad_faces, faces_idx, nv, fill_back, dtype):
    """index-add of every face row onto its three vertices; row k of the twin goes to vertex 2 - k"""
    g = grad_faces.to(dtype)
    bs = g.shape[0]
    idx = _index(faces_idx, bs)
    nf0 = idx.shape[1]
    gv = torch.zeros(bs, nv, 3, dtype=dtype)
    for b in range(bs):
        for k in range(3):
            gv[b].index_add_(0, idx[b, :, k], g[b, :nf0, k])
            if fill_back:
                gv[b].index_add_(0, idx[b, :, k], g[b, nf0:, 2 - k])
    return gv


def normals_fwd(faces, dtype=torch.float32):
    """k_face_normals: normalize(cross(v0 - v1, v2 - v1)) of faces [..., 3, 3]"""
    f = faces.to(dtype)
    return normalize3(cross3(f[..., 0, :] - f[..., 1, :], f[..., 2, :] - f[..., 1, :]))


def normals_bwd(faces, grad_normals, dtype):
    """y = c / s, s = |c| + eps: g_c = g_n / s - c (g_n . c) / (s^2 |c|), and g_c = g_n / eps where |c| == 0 (the kernel's
    documented rule; Chainer gives NaN); then the cross product's two gradients (cross.py:47-53)"""
    f, gn = faces.to(dtype), grad_normals.to(dtype)
    v10 = f[..., 0, :] - f[..., 1, :]
    v12 = f[..., 2, :] - f[..., 1, :]
    c = cross3(v10, v12)
    nrm = _norm3(c)
    s = nrm + EPS
    dot = (gn[..., 0] * c[..., 0] + gn[..., 1] * c[..., 1]) + gn[..., 2] * c[..., 2]
    zero = nrm == 0
    coef = torch.where(zero, torch.zeros_like(dot), dot / torch.where(zero, torch.ones_like(nrm), s * s * nrm))
    gc = gn / s[..., None] - c * coef[..., None]
    g10 = cross3(v12, gc)
    g12 = cross3(gc, v10)
    return torch.stack([g10, -(g10 + g12), g12], dim=-2)


# ------------------------------------------------------------------------------------------ A1: project
# (bs, nv): one vertex; one block with an idle lane; exactly one block; a second block of one vertex; batch boundaries inside
# blocks (257 = 256 + 1, so items 1 and 2 start at threads 1 and 2 of blocks 1 and 2); five blocks per item and a tail
PROJECT_SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (3, 257), (2, 1025))
PROJECT_MODES = (0, 1, 2)


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def widths_of(angles):
    from oracle import nr_oracle as no
    return None if angles is None else torch.tensor([float(no.perspective_width(a)) for a in angles], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _project_case(bs, nv, mode, with_width, flip_x):
    g = torch.Generator().manual_seed(8100 + 1000 * bs + nv + 7 * mode + 3 * int(with_width) + int(flip_x))
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)   # noqa: E731
    eye = r(bs, 3) * 2 - 1
    za = _unit(torch.randn(bs, 3, generator=g, dtype=torch.float64))
    side = torch.randn(bs, 3, generator=g, dtype=torch.float64)
    side = _unit(side - (side * za).sum(1, keepdim=True) * za)
    up = _unit(side + (r(bs, 1) * 1.4 - 0.7) * za)                     # at least 55 degrees off the viewing direction
    xa = _unit(cross3(up, za))
    ya = cross3(za, xa)
    # camera-space points: depth in [1.3, 7.5], |x|, |y| up to 0.6 depth
    z = 1.3 + 6.2 * r(bs, nv)
    x = (r(bs, nv) * 2 - 1) * 0.6 * z
    y = (r(bs, nv) * 2 - 1) * 0.6 * z
    if mode == 0:
        v = torch.stack([x, y, z], dim=-1)
        eye_t = dir_t = up_t = None
    else:
        v = eye[:, None] + x[..., None] * xa[:, None] + y[..., None] * ya[:, None] + z[..., None] * za[:, None]
        length = 0.5 + 2 * r(bs, 1)                                    # direction and up are not unit vectors
        eye_t = eye.float()
        dir_t = ((eye + za * length) if mode == 2 else za * length).float()
        up_t = (up * (0.5 + r(bs, 1))).float()
    if flip_x:
        v = v * torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64)
    # a different viewing angle per item; the half-width is tan(angle) as the host computes it (perspective.py:10-13)
    angles = [12.0 + 9.0 * b + float(r(1)) for b in range(bs)] if with_width else None
    return {'verts': v.float().contiguous(), 'mode': mode, 'eye': eye_t, 'direction': dir_t, 'up': up_t, 'angles': angles,
            'width': widths_of(angles), 'flip_x': int(flip_x), 'grad': torch.randn(bs, nv, 3, generator=g)}


def project_case(bs, nv, mode, with_width, flip_x):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _project_case(bs, nv, mode, bool(with_width), int(flip_x)).items()}


def project_parallel_up_case():
    """bs = 2, 257 vertices, mode 1 and 2: `up` is an exact multiple of the viewing direction, which lies along a coordinate axis,
    so cross(up, z) is exactly zero in float32: x axis = 0 / (0 + eps) = 0, y axis = cross(z, 0) = 0, projected x and y are exactly
    0 and the gradient stays finite.  One case per mode, the axis differs per item."""
    cases = []
    for mode in (1, 2):
        g = torch.Generator().manual_seed(8190 + mode)
        eye = torch.tensor([[0.25, -0.5, 0.75], [-1.0, 0.5, 0.125]])
        za = torch.tensor([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
        depth = 1.5 + 6 * torch.rand(2, 257, generator=g)
        side = torch.rand(2, 257, 3, generator=g) * 2 - 1
        v = eye[:, None] + depth[..., None] * za[:, None] + side * (1 - za.abs())[:, None]
        direction = (eye + 2 * za) if mode == 2 else 2 * za
        cases.append({'verts': v.contiguous(), 'mode': mode, 'eye': eye, 'direction': direction, 'up': za * torch.tensor([[3.0], [-0.5]]),
                      'angles': [16.0, 24.0], 'width': widths_of([16.0, 24.0]), 'flip_x': 0, 'grad': torch.randn(2, 257, 3, generator=g)})
    return cases


def camera_depth64(c):
    """(min, max) camera-space depth of a project case, float64"""
    z = project_fwd(c['verts'], c['mode'], c['eye'], c['direction'], c['up'], None, c['flip_x'], torch.float64)[..., 2]
    return float(z.min()), float(z.max())


def assert_depth_range(c):
    lo, hi = camera_depth64(c)
    assert DEPTH_RANGE[0] <= lo and hi <= DEPTH_RANGE[1], (lo, hi)
    return lo, hi


def project_args(c):
    return c['verts'], c['mode'], c['eye'], c['direction'], c['up'], c['width'], c['flip_x']


# ------------------------------------------------------------------------------------------ A2: gather
GATHER_NF0 = (1, 255, 256, 257, 600)
GATHER_BS = (1, 3)
GATHER_NV = 211
GATHER_HUB = 100                       # the vertex planted in >= 300 faces of the 600-face lists
GATHER_UNUSED = (3, 4, 5, 6, 7, 209)   # vertices in no face
HUB_FACES = 320


def _gather_list(nf0, seed):
    """one [nf0, 3] index list.  Planted, in this order, as far as nf0 has room: a face of vertex 0, vertex nv - 1 and the hub; a
    face (i, i, j); a face (i, i, i); HUB_FACES faces through the hub at changing corners; the rest random.  No face touches
    GATHER_UNUSED.  The rows are then shuffled."""
    g = torch.Generator().manual_seed(seed)
    allowed = torch.tensor([v for v in range(GATHER_NV) if v not in GATHER_UNUSED])
    rows = [(0, GATHER_NV - 1, GATHER_HUB), (17, 17, 42), (23, 23, 23)]
    rnd = allowed[torch.randint(0, len(allowed), (max(nf0, 3) + HUB_FACES, 3), generator=g)]
    if nf0 >= 600:
        for j in range(HUB_FACES):
            row = rnd[j].tolist()
            row[j % 3] = GATHER_HUB
            rows.append(tuple(row))
    rows += [tuple(x) for x in rnd[HUB_FACES:HUB_FACES + max(nf0 - len(rows), 0)].tolist()]
    rows = torch.tensor(rows[:nf0], dtype=torch.int32)
    return rows[torch.randperm(nf0, generator=g)]


@functools.lru_cache(maxsize=None)
def _gather_case(nf0, bs, shared, fill_back):
    seed = 8200 + 10 * nf0 + bs + 5 * int(shared) + int(fill_back)
    g = torch.Generator().manual_seed(seed)
    lists = 1 if shared else bs
    idx = torch.stack([_gather_list(nf0, seed + 100 * (b + 1)) for b in range(lists)])
    nf = 2 * nf0 if fill_back else nf0
    return {'verts': torch.randn(bs, GATHER_NV, 3, generator=g), 'faces_idx': idx, 'fill_back': bool(fill_back),
            'grad_int': torch.randint(-8, 9, (bs, nf, 3, 3), generator=g).float(),
            'grad': torch.randn(bs, nf, 3, 3, generator=g)}


def gather_case(nf0, bs, shared, fill_back):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _gather_case(nf0, bs, bool(shared), bool(fill_back)).items()}


# (nf0, bs, shared): per-item lists at both batch sizes, and the shared [1, nf0, 3] list at bs = 3 (faces_batch_stride == 0)
GATHER_CASES = [(nf0, bs, False) for nf0 in GATHER_NF0 for bs in GATHER_BS] + [(nf0, 3, True) for nf0 in GATHER_NF0]


# ------------------------------------------------------------------------------------------ A3: face normals
NORMALS_COUNTS = (1, 255, 256, 257, 1025)
NORMALS_FAMILIES = ('dyadic', 'normal')
NORMALS_BS = 1


def _degenerate_rows(n):
    """(rows of three equal vertices, rows of three collinear distinct vertices) for n faces: the first and the last face and one
    beside each block edge, as far as n has room"""
    equal = sorted({i for i in (0, 255, 600) if i < n})
    collinear = sorted({i for i in (n - 1, 256, 100) if 0 <= i < n and i not in equal})
    return equal, collinear


@functools.lru_cache(maxsize=None)
def _normals_case(n, family):
    g = torch.Generator().manual_seed(8300 + n + (7 if family == 'dyadic' else 0))
    if family == 'dyadic':
        # k / 64 with |k| <= 512: the differences (|k| <= 1024) and the cross product's terms (< 2^21 / 4096) are exact in float32
        f = torch.randint(-512, 513, (n, 3, 3), generator=g).float() / 64
    else:
        f = torch.randn(n, 3, 3, generator=g)
    equal, collinear = _degenerate_rows(n)
    for i in equal:
        p = torch.randint(-512, 513, (3,), generator=g).float() / 64
        f[i] = p[None].expand(3, 3)
    for i in collinear:
        # v0 = p + d, v1 = p, v2 = p + 3 d with dyadic p, d: v10 = d and v12 = 3 d exactly, so every term of the cross product
        # cancels exactly
        p = torch.randint(-128, 129, (3,), generator=g).float() / 64
        d = torch.randint(1, 65, (3,), generator=g).float() / 64
        f[i] = torch.stack([p + d, p, p + 3 * d])
    return {'faces': f[None].contiguous(), 'grad': torch.randn(1, n, 3, generator=g), 'equal': equal, 'collinear': collinear}


def normals_case(n, family):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _normals_case(n, family).items()}


# ------------------------------------------------------------------------------------------ B: the render-maps scenes
MAPS_R = 32
MAPS_EXTRA_VERTS = 6      # vertices appended to the mesh that no face references
MAPS_ANGLES = (15.0, 19.0)
MAPS_CASES = ('default', 'fill_back_off', 'shared', 'look_at')
MAPS_SUBSETS = ('m', 'n', 'd', 'mnd')


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def _maps_scene(name):
    from sdn_hip import synth
    assert name in MAPS_CASES
    v, f = synth.uv_sphere(8, 10)                                    # 72 vertices, 140 triangles
    nv0 = len(v)
    rng = np.random.default_rng(8400)
    eye = np.array([[0.1, -0.2, 0.3], [-0.3, 0.15, -0.2]])
    direction = np.array([[0.1, 0.05, -1.0], [-0.2, -0.1, -0.9]])
    up = np.array([[0.0, 1.0, 0.1], [0.15, 0.9, 0.0]])
    poses = ((_rot((1, 2, 0.5), 0.7), (0.9, 0.6, 0.75), 4.0, (0.12, -0.08)),
             (_rot((0.3, -1, 1), 2.1), (0.6, 0.8, 0.7), 3.4, (-0.1, 0.15)))
    verts, centres = [], []
    for b, (R, scale, dist, off) in enumerate(poses):
        za = direction[b] / np.linalg.norm(direction[b])
        xa = np.cross(up[b], za)
        xa /= np.linalg.norm(xa)
        ya = np.cross(za, xa)
        centre = eye[b] + dist * za + off[0] * xa + off[1] * ya
        p = (v.astype(np.float64) * np.asarray(scale)) @ R.T + centre
        extra = centre + rng.uniform(-0.5, 0.5, (MAPS_EXTRA_VERTS, 3))   # in view, referenced by no face
        verts.append(np.concatenate([p, extra]))
        centres.append(centre)
    # the entry points flip x themselves (flip_x = 1): hand them the mirror image of the scene laid out above
    verts = np.stack(verts) * np.array([-1.0, 1.0, 1.0])
    f = f.astype(np.int32)
    f1 = np.roll(f, 1, axis=1)[rng.permutation(len(f))]               # item 1: the same surface, other face order and first corner
    faces = f[None] if name == 'shared' else np.stack([f, f1])
    mode = 2 if name == 'look_at' else 1
    direction_t = np.stack(centres) if mode == 2 else direction       # look_at: `direction` holds the point looked at
    return {'verts': torch.tensor(verts, dtype=torch.float32), 'faces_idx': torch.tensor(faces), 'fill_back': name != 'fill_back_off',
            'mode': mode, 'eye': torch.tensor(eye, dtype=torch.float32), 'direction': torch.tensor(direction_t, dtype=torch.float32),
            'up': torch.tensor(up, dtype=torch.float32), 'angles': MAPS_ANGLES, 'nv_mesh': nv0}


def maps_scene(name):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _maps_scene(name).items()}


def maps_width(scene):
    return widths_of(scene['angles'])


@functools.lru_cache(maxsize=None)
def maps_weights():
    """the linear functionals of the three maps, bs = 2"""
    g = torch.Generator().manual_seed(8401)
    R = MAPS_R
    return {'m': torch.randn(2, R, R, generator=g), 'n': torch.randn(2, 3, R, R, generator=g), 'd': torch.randn(2, R, R, generator=g)}


def oracle_maps(scene, verts):
    """(alpha [bs, R, R], normal [bs, 3, R, R], depth [bs, R, R]) of `verts` (a leaf that takes the gradient) composed from the
    pieces of oracle/nr_oracle.py as derender3d's Renderer composes them (SDNRenderer.__call__ + NRRenderer.render_*), with the
    camera mode, fill_back and a viewing angle per item open to choice."""
    from oracle import nr_oracle as no
    bs = verts.shape[0]
    faces = scene['faces_idx'].expand(bs, -1, -1)
    if scene['fill_back']:
        faces = torch.cat((faces, faces.flip(2)), dim=1)
    v = verts * torch.tensor([-1.0, 1.0, 1.0])                                                      # renderer.py:243
    ref = no.NRRenderer()
    normals = ref.face_normals(v, faces)
    if scene['mode'] == 2:
        cam = no.look_at(v, scene['eye'], scene['direction'], scene['up'])
    else:
        cam = no.look(v, scene['eye'], scene['direction'], scene['up'])
    cam = torch.cat([no.perspective(cam[b:b + 1], angle=scene['angles'][b]) for b in range(bs)])
    f9 = no.vertices_to_faces(cam, faces)
    R = MAPS_R
    alpha = no.rasterize_silhouettes(f9, R, True)                                                   # module defaults (renderer.py:57)
    depth = no.rasterize_depth(f9, R, True)
    textures = normals[:, :, None, None, None, :].repeat(1, 1, 2, 2, 2, 1)
    # The colour pass runs item by item.  The reference's texture sampling takes the face's depths for its perspective correction
    # from `faces` without the batch offset (rasterize.py:390; restated as written in oracle/raster_oracle.c, K4): item b > 0 reads
    # item 0's face of the same index, its texture coordinate can then pass the end of the face's 2 x 2 x 2 texture and fetch the
    # next face's colour.  3D-SDN renders one object per call, where that line is right; so does this composition.
    rgb = torch.cat([no.rasterize(f9[b:b + 1], textures[b:b + 1], R, True, ref.near, ref.far, ref.rasterizer_eps, ref.background_color)
                     for b in range(bs)])
    x, y, z = torch.unbind(rgb, dim=1)
    return alpha, torch.stack([-x, y, z], dim=1), depth                                             # renderer.py:268-270


def maps_loss(maps, which, to=lambda t: t):
    """the functional of the maps named in `which` ('m', 'n', 'd' or 'mnd')"""
    w = maps_weights()
    return sum((maps[i] * to(w[k])).sum() for i, k in enumerate('mnd') if k in which)
