"""torch.autograd wrappers over the C ABI (device tensors in, device tensors out, no host hops).

Each Function mirrors one piece of the reference's Chainer graph (paths under
/root/reference/geometric/):
  ProjectVertices  look / look_at / perspective      neural_renderer/look.py, look_at.py, perspective.py
  GatherFaces      vertices_to_faces (+ fill_back)   neural_renderer/vertices_to_faces.py, renderer.py:41
  FaceNormals      normalize(cross(v10, v12))        derender3d/models/renderer.py:66-76
  RasterizeMaps    Rasterize + flip + 2x2 pool       neural_renderer/rasterize.py:19-974
"""
import ctypes
import functools
import threading

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import (AA, ACCUMULATE, ALPHA, COUNT_WORK, DEPTH, FACE_COLOR, K1_COVERAGE, RGB, SAVE_MAPS, SERIAL_EDGES, STREAM_FACES, c_floats, c_ints, c_ptrs, check, const_f32,
               deterministic, lib, perspective_transform_scratch, ptr, raster_bwd_workspace, raster_workspace, scene_id_workspace, size_query, stream,
               train_id_workspace, train_losses_scratch, want)

CAMERA_NONE, CAMERA_LOOK, CAMERA_LOOK_AT = 0, 1, 2

_tls = threading.local()

# a size the library answers for a shape, asked once per shape
_remembered = functools.lru_cache(maxsize=256)


# ---- the checks of the operators that never copy an argument: its type, then its shape (at the call site), then contiguity, then the
# device.  (The older operators go through want(): a CPU tensor is refused first, a non-contiguous one copied.) ----

def _is_tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(t)))


def _are_tensors(named):
    for name, t in named:
        _is_tensor(t, name)


def _count_tensor(t, name):
    """an optional count that is handed through unread: an int32 [1] tensor; _on_one_device then asks for the device"""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be None or an int32 [1] tensor on the device, got %r' % (name, type(t)))
    if t.dtype != torch.int32:
        raise TypeError('%s must be %s, got %s' % (name, torch.int32, t.dtype))
    if t.numel() != 1:
        raise ValueError('%s must hold one element, got %s' % (name, tuple(t.shape)))


def _four_floats(values, name):
    if isinstance(values, torch.Tensor):
        if values.is_cuda:
            raise TypeError('%s must be four host numbers; a tensor on %s would have to be read back' % (name, values.device))
        values = values.tolist()
    out = [float(v) for v in values]
    if len(out) != 4:
        raise ValueError('%s must hold four values, got %d' % (name, len(out)))
    return out


def _not_contiguous(name, t):
    return ValueError('%s must be contiguous (strides %s of %s)' % (name, t.stride(), tuple(t.shape)))


def _contiguous(named, fp32=()):
    """tensor by tensor: float32 where its name is in `fp32`, then contiguous"""
    for name, t in named:
        if name in fp32 and t.dtype != torch.float32:
            raise TypeError('%s must be %s, got %s' % (name, torch.float32, t.dtype))
        if not t.is_contiguous():
            raise _not_contiguous(name, t)


def _on_gpu(t, name, what):
    """`what` ends the refusal: 'the ... only runs on the GPU'"""
    if not t.is_cuda:
        raise NotImplementedError('%s is on %s; %s' % (name, t.device, what))


def _on_device_of(first, dev, named):
    """every tensor of `named` on `dev`, the device of the argument called `first`"""
    for name, t in named:
        if t.device != dev:
            raise ValueError('%s is on %s, %s on %s' % (name, t.device, first, dev))


def _on_one_device(named, what):
    """tensor by tensor: on the GPU, then on the device of the first"""
    first, dev = named[0][0], named[0][1].device
    for name, t in named:
        _on_gpu(t, name, what)
        _on_device_of(first, dev, ((name, t),))


class verification:
    """Thread-local verification / measurement switches for the rasterizer (no process-wide state: two threads -- e.g.
    nn.DataParallel replicas -- never see each other's settings; the backward pass uses what its forward call saw):
        serial_edges  backward walks every edge serially in the reference's exact summation order (SDN_SERIAL_EDGES)
        stream_faces  forward skips the per-tile face lists, i.e. forces the list-overflow path (SDN_STREAM_FACES)
        count_work    forward runs the counting build of k_raster_tiles; `last_work` then holds (candidate pixel tests,
                      tests passed, depth keys) of the most recent call on this thread (SDN_COUNT_WORK)
    Usage: `with ops.verification(serial_edges=True): ...`."""

    def __init__(self, serial_edges=None, stream_faces=None, count_work=None):
        new = dict(serial_edges=serial_edges, stream_faces=stream_faces, count_work=count_work)
        self.new = {k: v for k, v in new.items() if v is not None}   # unspecified switches keep their value (nesting)

    def __enter__(self):
        self.old = {k: getattr(_tls, k, False) for k in self.new}
        for k, v in self.new.items():
            setattr(_tls, k, bool(v))
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            setattr(_tls, k, v)
        return False


def _switch(name):
    return getattr(_tls, name, False)


_K1 = [False]


def set_k1_coverage(flag):
    """Process-wide: forward rasterizations use the coverage rule of the reference's DEFAULT kernel K1 (rasterize.py:102-236,
    what `scripts/env.sh:11` selects through NEURAL_RENDERER_UNSAFE=1) instead of the safe kernels' -- SDN_K1_COVERAGE, with
    exact depth ties settled by face order.  neural_renderer.use_unsafe_rasterizer / the environment variable set it."""
    _K1[0] = bool(flag)


def k1_coverage():
    return _K1[0]


def last_clocks():
    """shader-clock ticks per phase of the same counting launch (sdn_raster_phase_clocks), summed over its waves."""
    return getattr(_tls, 'last_clocks', None)


def last_work():
    """(candidates, passed, keys) of this thread's latest RasterizeMaps forward under verification(count_work=True)."""
    return getattr(_tls, 'last_work', None)


def perspective_width(angle):
    """tan(angle / 180. * 3.1416) in float32 (neural_renderer/perspective.py:10-13)."""
    a = np.float32(angle)
    a = np.float32(a / np.float32(180.))
    a = np.float32(a * np.float32(3.1416))
    return np.float32(np.tan(a, dtype=np.float32))


def _f32(t, name):
    return want(t, torch.float32, name)


@_remembered
def _ptf_scratch(n, V):
    """(key bytes, acc bytes) of sdn_perspective_transform / _bwd: the library's own answer, remembered per shape."""
    return perspective_transform_scratch(n, V)


class ProjectVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, camera_mode, eye, direction, up, width, flip_x):
        v = _f32(vertices, 'vertices')
        if v.dim() != 3 or v.shape[2] != 3:
            raise ValueError('vertices must be [batch, n, 3]')
        bs, nv = v.shape[:2]
        eye = _f32(eye, 'eye')
        direction = _f32(direction, 'direction')
        up = _f32(up, 'up')
        width = _f32(width, 'width')
        for t, n in ((eye, 'eye'), (direction, 'direction'), (up, 'up')):
            if t is not None and tuple(t.shape) != (bs, 3):
                raise ValueError('%s must be [batch, 3]' % n)
        if width is not None and width.numel() != bs:
            raise ValueError('width must have one entry per batch element')
        out = torch.empty_like(v)
        check(lib().sdn_project_vertices(ptr(v), bs, nv, int(camera_mode), ptr(eye), ptr(direction), ptr(up),
                                         ptr(width), int(flip_x), ptr(out), stream()))
        ctx.save_for_backward(v, eye, direction, up, width)
        ctx.cfg = (int(camera_mode), int(flip_x))
        return out

    @staticmethod
    def backward(ctx, g):
        v, eye, direction, up, width = ctx.saved_tensors
        mode, flip_x = ctx.cfg
        g = g.contiguous()
        gv = torch.empty_like(v)
        bs, nv = v.shape[:2]
        check(lib().sdn_project_vertices_bwd(ptr(v), bs, nv, mode, ptr(eye), ptr(direction), ptr(up), ptr(width),
                                             flip_x, ptr(g), ptr(gv), stream()))
        return gv, None, None, None, None, None, None


class GatherFaces(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, faces_idx, fill_back):
        v = _f32(vertices, 'vertices')
        f = want(faces_idx, torch.int32, 'faces')
        if v.dim() != 3 or v.shape[2] != 3:
            raise ValueError('vertices must be [batch, n, 3]')
        if f.dim() != 3 or f.shape[2] != 3:
            raise ValueError('faces must be [batch, n, 3]')
        bs, nv = v.shape[:2]
        if f.shape[0] not in (1, bs):
            raise ValueError('faces batch %d does not match vertices batch %d' % (f.shape[0], bs))
        nf0 = f.shape[1]
        stride = 0 if (f.shape[0] == 1 and bs > 1) else nf0 * 3
        nf = 2 * nf0 if fill_back else nf0
        out = torch.empty((bs, nf, 3, 3), dtype=torch.float32, device=v.device)
        check(lib().sdn_gather_faces(ptr(v), ptr(f), bs, nv, nf0, stride, int(bool(fill_back)), ptr(out), stream()))
        ctx.save_for_backward(f)
        ctx.cfg = (bs, nv, nf0, stride, int(bool(fill_back)))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:   # no gradient reached the faces (e.g. the normal map of a silhouette-only loss): no launches
            return None, None, None
        (f,) = ctx.saved_tensors
        bs, nv, nf0, stride, fill_back = ctx.cfg
        g = g.contiguous()
        gv = torch.empty((bs, nv, 3), dtype=torch.float32, device=g.device)
        check(lib().sdn_gather_faces_bwd(ptr(g), ptr(f), bs, nv, nf0, stride, fill_back, ptr(gv), stream()))
        return gv, None, None


class FaceNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, faces):
        f = _f32(faces, 'faces')
        if f.dim() != 4 or f.shape[2:] != (3, 3):
            raise ValueError('faces must be [batch, n, 3, 3]')
        out = torch.empty(f.shape[:2] + (3,), dtype=torch.float32, device=f.device)
        check(lib().sdn_face_normals(ptr(f), f.shape[0] * f.shape[1], ptr(out), stream()))
        ctx.save_for_backward(f)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:   # the colours took no gradient (autograd would otherwise hand over zeros and run the kernels)
            return None
        (f,) = ctx.saved_tensors
        g = g.contiguous()
        gf = torch.empty_like(f)
        check(lib().sdn_face_normals_bwd(ptr(f), ptr(g), f.shape[0] * f.shape[1], ptr(gf), stream()))
        return gf


class RasterizeMaps(torch.autograd.Function):
    """faces [bs,nf,3,3] (+ textures) -> (rgb [bs,3,R,R] | None, alpha [bs,R,R] | None, depth [bs,R,R] | None).

    `eps_alpha`: when both rgb and alpha are requested and eps_alpha is not None, the backward runs the
    silhouette term and the colour term as two separate passes with their own eps -- what two separate
    Rasterize calls (rasterize_silhouettes with the module default 1e-4 and rasterize with the
    Renderer's 1e-3, derender3d/models/renderer.py:37,90-92) would have produced.  With eps_alpha None the
    two terms share one pass and one eps like a single rasterize_rgbad call (rasterize.py:627-655).
    """

    @staticmethod
    def forward(ctx, faces, textures, image_size, anti_aliasing, near, far, eps, background_color, return_rgb,
                return_alpha, return_depth, eps_alpha, face_color):
        if not any((return_rgb, return_alpha, return_depth)):
            raise Exception('nothing to draw')  # neural_renderer/rasterize.py:25-27
        f = _f32(faces, 'faces')
        if f.dim() != 4 or f.shape[2:] != (3, 3):
            raise ValueError('faces must be [batch size, number of faces, 3, 3]')
        bs, nf = f.shape[:2]
        dev = f.device
        S = int(image_size) * 2 if anti_aliasing else int(image_size)
        R = int(image_size)
        flags = (RGB if return_rgb else 0) | (ALPHA if return_alpha else 0) | (DEPTH if return_depth else 0)
        flags |= AA if anti_aliasing else 0
        tex = None
        ts = 0
        if return_rgb:
            tex = _f32(textures, 'textures')
            if face_color:
                if tuple(tex.shape) != (bs, nf, 3):
                    raise ValueError('face colours must be [batch, faces, 3]')
                flags |= FACE_COLOR
                ts = 2
            else:
                if tex.dim() != 6 or tex.shape[0] != bs or tex.shape[1] != nf or tex.shape[5] != 3 or \
                        tex.shape[2] < 2 or tex.shape[2] != tex.shape[3] or tex.shape[3] != tex.shape[4]:
                    raise ValueError('textures must be [batch, faces, ts, ts, ts, 3] with ts >= 2')
                ts = tex.shape[2]
        need_grad = any(ctx.needs_input_grad[:2])
        if need_grad:
            flags |= SAVE_MAPS
        if _switch('stream_faces'):
            flags |= STREAM_FACES
        if _switch('count_work'):
            flags |= COUNT_WORK
        if k1_coverage():
            flags |= K1_COVERAGE
        bg = None
        bg_per_batch = 0
        if return_rgb:
            if isinstance(background_color, torch.Tensor):
                bg = background_color.to(device=dev, dtype=torch.float32).contiguous()
            else:
                bg = const_f32(background_color if background_color is not None else (0, 0, 0), dev)
            bg_per_batch = 1 if bg.dim() == 2 else 0
        face_inv = torch.empty((bs, nf, 3, 3), dtype=torch.float32, device=dev)
        fim = wmap = dmap = rgbmap = None
        if need_grad:
            fim = torch.empty((bs, S, S), dtype=torch.int32, device=dev)
            wmap = torch.empty((bs, S, S, 3), dtype=torch.float32, device=dev)
            dmap = torch.empty((bs, S, S), dtype=torch.float32, device=dev)
            if return_rgb:
                rgbmap = torch.empty((bs, S, S, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((bs, 3, R, R), dtype=torch.float32, device=dev) if return_rgb else None
        alpha = torch.empty((bs, R, R), dtype=torch.float32, device=dev) if return_alpha else None
        depth = torch.empty((bs, R, R), dtype=torch.float32, device=dev) if return_depth else None
        ws = raster_workspace(bs, nf, S, dev)
        check(lib().sdn_rasterize_fwd(ptr(f), ptr(tex), ts, bs, nf, S, float(near), float(far), float(eps), ptr(bg),
                                      bg_per_batch, flags, ptr(face_inv), ptr(fim), ptr(wmap), ptr(dmap),
                                      ptr(rgbmap), ptr(rgb), ptr(alpha), ptr(depth), ptr(ws), ws.numel(), stream()))
        if flags & COUNT_WORK:
            c = (ctypes.c_ulonglong * 3)()
            check(lib().sdn_raster_work_counters(ptr(ws), bs, nf, S, c, stream()))
            _tls.last_work = (int(c[0]), int(c[1]), int(c[2]))
            c8 = (ctypes.c_ulonglong * 8)()
            check(lib().sdn_raster_phase_clocks(ptr(ws), bs, nf, S, c8, stream()))
            _tls.last_clocks = dict(zip(('fetch_and_wait', 'lane_boxes', 'wave_boxes', 'thin', 'epilogue', 'total', 'longest_wave',
                                         'waves'), (int(v) for v in c8)))
            flags &= ~COUNT_WORK
        if need_grad:
            ctx.save_for_backward(f, tex, face_inv, fim, wmap, dmap, rgbmap)
        ctx.cfg = (ts, bs, nf, S, float(eps), None if eps_alpha is None else float(eps_alpha), flags,
                   SERIAL_EDGES if _switch('serial_edges') else 0)
        ctx.set_materialize_grads(False)
        return rgb, alpha, depth

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth):
        f, tex, face_inv, fim, wmap, dmap, rgbmap = ctx.saved_tensors
        ts, bs, nf, S, eps, eps_alpha, flags, serial = ctx.cfg   # `serial`: what the forward call's thread had set
        base = (flags & (AA | FACE_COLOR)) | serial
        g_rgb = None if g_rgb is None else g_rgb.contiguous()
        g_alpha = None if g_alpha is None else g_alpha.contiguous()
        g_depth = None if g_depth is None else g_depth.contiguous()
        grad_faces = torch.empty_like(f)
        want_tex_grad = (flags & RGB) and ctx.needs_input_grad[1] and g_rgb is not None
        grad_tex = torch.empty_like(tex) if want_tex_grad else None
        L = lib()
        ws = raster_bwd_workspace(bs, nf, S, f.device)

        def run(fl, e, gr, ga, gd, gt):
            check(L.sdn_rasterize_bwd(ptr(f), ptr(tex), ts, bs, nf, S, e, fl, ptr(face_inv), ptr(fim), ptr(wmap),
                                      ptr(dmap), ptr(rgbmap), ptr(gr), ptr(ga), ptr(gd), ptr(grad_faces), ptr(gt),
                                      ptr(ws), ws.numel(), stream()))

        split = (eps_alpha is not None) and (flags & RGB) and (flags & ALPHA)
        if split:
            # pass 1 stores the silhouette term, pass 2 adds colour (+ depth) and the texture scatter
            run(base | ALPHA, eps_alpha, None, g_alpha, None, None)
            if g_rgb is not None or g_depth is not None:
                if grad_tex is not None:
                    grad_tex.zero_()
                run(base | RGB | (flags & DEPTH) | ACCUMULATE, eps, g_rgb, None, g_depth, grad_tex)
        else:
            e = eps if (flags & RGB) or eps_alpha is None else eps_alpha
            run((flags & ~SAVE_MAPS & ~STREAM_FACES) | serial, e, g_rgb, g_alpha, g_depth, grad_tex)
        gf = grad_faces if ctx.needs_input_grad[0] else None
        return (gf, grad_tex) + (None,) * 11


class RenderMapsFn(torch.autograd.Function):
    """(alpha [bs,R,R], normal [bs,3,R,R] | None, depth [bs,R,R] | None) of a frame's objects: sdn_render_maps_fwd / _bwd, ONE C
    call each way instead of ProjectVertices + 2 x GatherFaces + FaceNormals + RasterizeMaps and two element-wise ops
    (derender3d/models/renderer.py:216-272 three times per object in the reference).  `vertices` are the caller's (not
    x-flipped); the result equals Renderer.render_maps' composition of the separate Functions bit for bit."""

    @staticmethod
    def forward(ctx, vertices, faces_idx, fill_back, camera_mode, eye, direction, up, width, flip_x, image_size,
                anti_aliasing, near, far, eps, eps_alpha, background_color, want_normal, want_depth):
        v = _f32(vertices, 'vertices')
        f = want(faces_idx, torch.int32, 'faces')
        if v.dim() != 3 or v.shape[2] != 3:
            raise ValueError('vertices must be [batch, n, 3]')
        if f.dim() != 3 or f.shape[2] != 3:
            raise ValueError('faces must be [batch, n, 3]')
        bs, nv = v.shape[:2]
        if f.shape[0] not in (1, bs):
            raise ValueError('faces batch %d does not match vertices batch %d' % (f.shape[0], bs))
        nf0 = f.shape[1]
        stride = 0 if (f.shape[0] == 1 and bs > 1) else nf0 * 3
        dev = v.device
        R = int(image_size)
        need_grad = ctx.needs_input_grad[0]
        flags = (RGB if want_normal else 0) | (DEPTH if want_depth else 0) | (AA if anti_aliasing else 0)
        flags |= SAVE_MAPS if need_grad else 0
        if _switch('stream_faces'):
            flags |= STREAM_FACES
        if k1_coverage():
            flags |= K1_COVERAGE
        nstate, nbwd, nscr = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(lib().sdn_render_maps_bytes(bs, nv, nf0, int(bool(fill_back)), R, flags, ctypes.byref(nstate), ctypes.byref(nbwd),
                                          ctypes.byref(nscr)))
        state = torch.empty(nstate.value, dtype=torch.uint8, device=dev)
        scratch = torch.empty(nscr.value, dtype=torch.uint8, device=dev)   # forward-only (tile lists): not saved for backward
        alpha = torch.empty((bs, R, R), dtype=torch.float32, device=dev)
        normal = torch.empty((bs, 3, R, R), dtype=torch.float32, device=dev) if want_normal else None
        depth = torch.empty((bs, R, R), dtype=torch.float32, device=dev) if want_depth else None
        bg = None
        bg_is_callers = isinstance(background_color, torch.Tensor)
        if want_normal:
            bg = background_color if bg_is_callers else \
                const_f32(background_color if background_color is not None else (0, 0, 0), dev)
            bg = bg.to(device=dev, dtype=torch.float32).contiguous()
            if bg.numel() != 3:
                raise ValueError('render_maps takes one background colour')
        cam = (int(camera_mode), _f32(eye, 'eye'), _f32(direction, 'direction'), _f32(up, 'up'), _f32(width, 'width'),
               int(bool(flip_x)))
        check(lib().sdn_render_maps_fwd(ptr(v), bs, nv, ptr(f), nf0, stride, int(bool(fill_back)), cam[0], ptr(cam[1]),
                                        ptr(cam[2]), ptr(cam[3]), ptr(cam[4]), cam[5], R, flags, float(near), float(far),
                                        float(eps), ptr(bg), ptr(alpha), ptr(normal), ptr(depth), ptr(state), state.numel(),
                                        ptr(scratch), scratch.numel(), stream()))
        if need_grad:
            # the background colour is handed to the backward call again (it re-derives the colour map).  A caller's own tensor
            # goes through save_for_backward so that an in-place change between forward and backward trips autograd's version
            # check instead of silently changing the normal / depth gradients; the const_f32 cache is never written
            if bg is not None and bg_is_callers:
                ctx.save_for_backward(v, f, state, cam[1], cam[2], cam[3], cam[4], bg)
                ctx.bg = None
            else:
                ctx.save_for_backward(v, f, state, cam[1], cam[2], cam[3], cam[4])
                ctx.bg = bg
            ctx.cfg = (bs, nv, nf0, stride, int(bool(fill_back)), cam[0], cam[5], R, flags & ~STREAM_FACES, float(eps),
                       float(eps_alpha), nbwd.value, SERIAL_EDGES if _switch('serial_edges') else 0)
        ctx.set_materialize_grads(False)
        return alpha, normal, depth

    @staticmethod
    def backward(ctx, g_alpha, g_normal, g_depth):
        saved = ctx.saved_tensors
        v, f, state, eye, direction, up, width = saved[:7]
        bg = saved[7] if len(saved) > 7 else ctx.bg
        bs, nv, nf0, stride, fill_back, mode, flip_x, R, flags, eps, eps_alpha, nbwd, serial = ctx.cfg
        if g_alpha is None and g_normal is None and g_depth is None:
            return (None,) * 18
        g_alpha = None if g_alpha is None else g_alpha.contiguous()
        g_normal = None if g_normal is None else g_normal.contiguous()
        g_depth = None if g_depth is None else g_depth.contiguous()
        ws = torch.empty(nbwd, dtype=torch.uint8, device=v.device)
        gv = torch.empty_like(v)
        check(lib().sdn_render_maps_bwd(ptr(v), bs, nv, ptr(f), nf0, stride, fill_back, mode, ptr(eye), ptr(direction), ptr(up),
                                        ptr(width), flip_x, R, flags | serial, eps, eps_alpha, ptr(bg), ptr(g_alpha),
                                        ptr(g_normal), ptr(g_depth), ptr(gv), ptr(state), state.numel(), ptr(ws), ws.numel(),
                                        stream()))
        return (gv,) + (None,) * 17


class FFDDecode(torch.autograd.Function):
    """verts [n, vmax, 3] = P [n, 3, ncoef] . Bt[cls] [ncoef, vmax]  (derender3d/models/transforms.py:97-99).
    With `constraint` [3 ncoef, 3 ncoef] (and `base` [3, ncoef]) the first argument holds raw coefficient rows [n, 3 ncoef] and
    P = base + coeffs . constraint is formed by the library as well (FFD.constrain, transforms.py:69-95, is linear): the
    whole decode is two launches each way and no torch op."""

    @staticmethod
    def forward(ctx, P, Bt, cls, constraint=None, base=None):
        P = _f32(P, 'P')
        Bt = _f32(Bt, 'Bt')
        cls = want(cls, torch.int32, 'cls')
        n = P.shape[0]
        ncoef = Bt.shape[1] if Bt.dim() == 3 else -1
        if constraint is not None:
            Cm = _f32(constraint, 'constraint')
            m = 3 * ncoef
            if P.dim() != 2 or P.shape[1] != m or tuple(Cm.shape) != (m, m) or (base is not None and base.numel() != m):
                raise ValueError('FFDDecode: coefficients [n, 3 ncoef], constraint [3 ncoef, 3 ncoef], base [3, ncoef]')
            base = None if base is None else _f32(base, 'base')
            coeffs = P
            P = torch.empty((n, 3, ncoef), dtype=torch.float32, device=coeffs.device)
            check(lib().sdn_ffd_coefficients(ptr(coeffs), ptr(Cm), ptr(base), n, m, 0, ptr(P), stream()))
        else:
            Cm = None
        if P.dim() != 3 or P.shape[1] != 3 or Bt.dim() != 3 or P.shape[2] != ncoef or cls.numel() != n:
            raise ValueError('FFDDecode: P [n,3,ncoef], Bt [classes,ncoef,vmax], cls [n]')
        vmax = Bt.shape[2]
        out = torch.empty((n, vmax, 3), dtype=torch.float32, device=P.device)
        check(lib().sdn_ffd_decode(ptr(Bt), ptr(P), ptr(cls), n, vmax, ncoef, ptr(out), stream()))
        if Cm is None:
            ctx.save_for_backward(Bt, cls)
        else:
            ctx.save_for_backward(Bt, cls, Cm)
        ctx.cfg = (n, vmax, ncoef)
        return out

    @staticmethod
    def backward(ctx, g):
        Bt, cls = ctx.saved_tensors[:2]
        n, vmax, ncoef = ctx.cfg
        g = g.contiguous()
        gP = torch.empty((n, 3, ncoef), dtype=torch.float32, device=g.device)
        check(lib().sdn_ffd_decode_bwd(ptr(Bt), ptr(cls), ptr(g), n, vmax, ncoef, ptr(gP), stream()))
        if len(ctx.saved_tensors) == 3:
            gc = torch.empty((n, 3 * ncoef), dtype=torch.float32, device=g.device)
            check(lib().sdn_ffd_coefficients(ptr(gP), ptr(ctx.saved_tensors[2]), None, n, 3 * ncoef, 1, ptr(gc), stream()))
            return gc, None, None, None, None
        return gP, None, None, None, None


class PoseParamsFn(torch.autograd.Function):
    """(rotations [n,4], scales [n,3]) = ((cos(theta/2), 0, sin(theta/2), 0), exp(log_scales)) -- Derenderer3d.render,
    derender3d/models/__init__.py:106-116: one launch each way instead of ten element-wise ones."""

    @staticmethod
    def forward(ctx, theta, log_scales):
        th = _f32(theta, 'theta').reshape(-1)
        n = th.shape[0]
        ls = _f32(log_scales, 'log_scales').reshape(n, 3)
        quat = torch.empty(n, 4, dtype=torch.float32, device=th.device)
        scales = torch.empty(n, 3, dtype=torch.float32, device=th.device)
        check(lib().sdn_pose_params(ptr(th), ptr(ls), n, ptr(quat), ptr(scales), stream()))
        ctx.save_for_backward(th, scales)
        ctx.shapes = (theta.shape, log_scales.shape)
        ctx.set_materialize_grads(False)
        return quat, scales

    @staticmethod
    def backward(ctx, g_quat, g_scales):
        th, scales = ctx.saved_tensors
        n = th.shape[0]
        want_t, want_s = ctx.needs_input_grad
        if g_quat is None and g_scales is None:
            return None, None
        gq = g_quat.contiguous() if g_quat is not None else None
        gs = g_scales.contiguous() if g_scales is not None else None
        gt = torch.empty(n, dtype=torch.float32, device=th.device) if want_t else None
        gl = torch.empty(n, 3, dtype=torch.float32, device=th.device) if want_s else None
        if gt is None and gl is None:
            return None, None
        check(lib().sdn_pose_params_bwd(ptr(th), ptr(scales), ptr(gq), ptr(gs), n, ptr(gt), ptr(gl), stream()))
        return (gt.reshape(ctx.shapes[0]) if gt is not None else None, gl.reshape(ctx.shapes[1]) if gl is not None else None)


class PoseAlgebraFn(torch.autograd.Function):
    """(thetas [n,1], alphas [n,1], rotations [n,4], scales [n,3], depths [n,1], center2ds [n,2], translations [n,3],
    persp [n,3], zooms [n,1]) of a frame's objects from the encoder outputs -- the pose algebra of Derenderer3d.render,
    derender3d/models/__init__.py:95-158, in one launch each way (sdn_pose_algebra / _bwd) instead of ~45 element-wise ops and
    their autograd nodes.  zooms: the given zooms of the training form, the `zoom_tos` of the test-time form."""

    @staticmethod
    def forward(ctx, centre, extent, focals, theta_deltas, log_scales, log_depths, translation2ds, training, image_size,
                render_size):
        c = _f32(centre, 'centre')
        n = c.shape[0]
        c = c.reshape(n, 2)
        e = _f32(extent, 'extent').reshape(n, 2)
        f = _f32(focals, 'focals').reshape(n)
        d = _f32(theta_deltas, 'theta_deltas').reshape(n, 2)
        ls = _f32(log_scales, 'log_scales').reshape(n, 3)
        ld = _f32(log_depths, 'log_depths').reshape(n)
        t2 = _f32(translation2ds, 'translation2ds').reshape(n, 2)
        dev = c.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        thetas, alphas, rot, scales, depths = new(n, 1), new(n, 1), new(n, 4), new(n, 3), new(n, 1)
        c2, trans, persp, zooms = new(n, 2), new(n, 3), new(n, 3), new(n, 1)
        check(lib().sdn_pose_algebra(ptr(c), ptr(e), ptr(f), ptr(d), ptr(ls), ptr(ld), ptr(t2), n, int(bool(training)),
                                     float(image_size), float(render_size), ptr(thetas), ptr(alphas), ptr(rot), ptr(scales),
                                     ptr(depths), ptr(c2), ptr(trans), ptr(persp), ptr(zooms), stream()))
        ctx.save_for_backward(c, e, d, thetas, scales, depths, c2, trans)
        ctx.training = int(bool(training))
        ctx.shapes = (theta_deltas.shape, log_scales.shape, log_depths.shape, translation2ds.shape)
        ctx.mark_non_differentiable(zooms)
        ctx.set_materialize_grads(False)
        return thetas, alphas, rot, scales, depths, c2, trans, persp, zooms

    @staticmethod
    def backward(ctx, g_thetas, g_alphas, g_rot, g_scales, g_depths, g_c2, g_trans, g_persp, _g_zooms):
        c, e, d, thetas, scales, depths, c2, trans = ctx.saved_tensors
        n = c.shape[0]
        gs = [g.contiguous() if g is not None else None for g in (g_thetas, g_alphas, g_rot, g_scales, g_depths, g_c2, g_trans,
                                                                  g_persp)]
        need = ctx.needs_input_grad[3:7]
        if all(g is None for g in gs) or not any(need):
            return (None,) * 10
        dev = c.device
        out = [torch.empty(shape, dtype=torch.float32, device=dev) if w else None
               for w, shape in zip(need, ((n, 2), (n, 3), (n,), (n, 2)))]
        check(lib().sdn_pose_algebra_bwd(ptr(c), ptr(e), ptr(d), ptr(thetas), ptr(scales), ptr(depths), ptr(c2), ptr(trans), n,
                                         ctx.training, *[ptr(g) for g in gs], *[ptr(o) for o in out], stream()))
        grads = [o.reshape(s) if o is not None else None for o, s in zip(out, ctx.shapes)]
        return (None, None, None, grads[0], grads[1], grads[2], grads[3], None, None, None)


class SilhouetteLossFn(torch.autograd.Function):
    """mean(mse_loss(masks, target, reduce=False) [* (1 - ignore)] + 100 * mean(ffd ** 2)) -- the loss of the test-time
    optimisation loop, geometric/scripts/main.py:445-451, forward in two launches (+ one memset), backward in one."""

    @staticmethod
    def forward(ctx, masks, target, ffd, ignore=None):
        m = _f32(masks, 'masks')
        t = _f32(target, 'target')
        if t.shape != m.shape:
            raise ValueError('target %s must have the shape of masks %s' % (tuple(t.shape), tuple(m.shape)))
        ig = None
        if ignore is not None:
            ig = _f32(ignore, 'ignore')
            if ig.shape != m.shape:
                raise ValueError('ignore must have the shape of masks')
        f = _f32(ffd, 'ffd') if ffd is not None else None
        sums = torch.empty(3 + 3 * 512, dtype=torch.float64, device=m.device)   # SDN_SIL_LOSS_SUMS
        out = torch.empty((), dtype=torch.float32, device=m.device)
        check(lib().sdn_silhouette_loss_fwd(ptr(m), ptr(t), ptr(ig), m.numel(), ptr(f), f.numel() if f is not None else 0,
                                            ptr(sums), ptr(out), stream()))
        ctx.save_for_backward(m, t, f, ig, sums)
        ctx.ffd_shape = ffd.shape if ffd is not None else None
        return out

    @staticmethod
    def backward(ctx, g):
        m, t, f, ig, sums = ctx.saved_tensors
        want_m, _, want_f, _ = ctx.needs_input_grad
        gm = torch.empty_like(m) if want_m else None
        gf = torch.empty_like(f) if (want_f and f is not None) else None
        if gm is None and gf is None:
            return None, None, None, None
        go = g.contiguous().reshape(1)
        check(lib().sdn_silhouette_loss_bwd(ptr(m), ptr(t), ptr(ig), m.numel(), ptr(f), f.numel() if f is not None else 0,
                                            ptr(sums), ptr(go), ptr(gm), ptr(gf), stream()))
        return gm, None, (gf.reshape(ctx.ffd_shape) if gf is not None else None), None


@_remembered
def _train_losses_scratch(B, R, nffd):
    """bytes of sdn_train_losses_*'s scratch: the library's own answer, remembered per shape"""
    return train_losses_scratch(B, R, nffd)


class TrainLossesFn(torch.autograd.Function):
    """The loss dict of BaseNet.step_batch (geometric/scripts/main.py:114-154) as one [7] tensor: theta_delta_loss,
    translation2d_loss, scale_loss, depth_loss, class_reward, mask_loss, ffd_coeff_reg -- sdn_train_losses_fwd / _bwd
    (include/sdn_hip.h), forward in two launches, backward in one; `targets` selects the items of each loss on the device.
    The tensors of a group `mode` does not ask for may be None; its slots are 0."""

    @staticmethod
    def forward(ctx, mode, mask_weight, ffd_coeff_reg, p_theta_deltas, p_translation2ds, p_log_scales, p_log_depths,
                p_class_log_probs, p_masks, p_ffd, thetas, translation2ds, log_scales, log_depths, masks, ignores, targets):
        names = ('_theta_deltas', '_translation2ds', '_log_scales', '_log_depths', '_class_log_probs', '_masks', '_ffd_coeffs',
                 'thetas', 'translation2ds', 'log_scales', 'log_depths', 'masks', 'ignores')
        given = (p_theta_deltas, p_translation2ds, p_log_scales, p_log_depths, p_class_log_probs, p_masks, p_ffd, thetas,
                 translation2ds, log_scales, log_depths, masks, ignores)
        td, t2, ls, ld, lp, pm, ff, th, bt2, bls, bld, bm, bi = (_f32(t, n) for t, n in zip(given, names))
        tg = want(targets, torch.int64, 'targets')
        B = tg.shape[0]
        R = pm.shape[-1] if pm is not None else 1
        S = bm.shape[-1] if bm is not None else R
        nffd = ff.numel() if ff is not None else 0
        scratch = torch.empty(_train_losses_scratch(B, R, nffd), dtype=torch.uint8, device=tg.device)
        out = torch.empty(7, dtype=torch.float32, device=tg.device)
        cfg = (B, R, S, int(mode), float(mask_weight), float(ffd_coeff_reg))
        check(lib().sdn_train_losses_fwd(ptr(td), ptr(t2), ptr(ls), ptr(ld), ptr(lp), ptr(pm), ptr(ff), nffd, ptr(th), ptr(bt2),
                                         ptr(bls), ptr(bld), ptr(bm), ptr(bi), ptr(tg), *cfg, ptr(scratch), ptr(out), stream()))
        ctx.save_for_backward(td, t2, ls, ld, pm, ff, th, bt2, bls, bld, bm, bi, tg, scratch)
        ctx.cfg = cfg
        ctx.lp = (lp.shape, lp.device) if lp is not None else None
        ctx.shapes = [t.shape if t is not None else None for t in given[:7]]
        return out

    @staticmethod
    def backward(ctx, g):
        td, t2, ls, ld, pm, ff, th, bt2, bls, bld, bm, bi, tg, scratch = ctx.saved_tensors
        src = (td, t2, ls, ld, None, pm, ff)
        grads = []
        for k, (need, t) in enumerate(zip(ctx.needs_input_grad[3:10], src)):
            if k == 4:   # _class_log_probs: its gradient needs m_i alone
                grads.append(torch.empty(ctx.lp[0], dtype=torch.float32, device=ctx.lp[1]) if need and ctx.lp is not None else None)
            else:
                grads.append(torch.empty_like(t) if need and t is not None else None)
        if all(x is None for x in grads):
            return (None,) * 17
        go = g.contiguous()
        nffd = ff.numel() if ff is not None else 0
        check(lib().sdn_train_losses_bwd(ptr(td), ptr(t2), ptr(ls), ptr(ld), ptr(pm), ptr(ff), nffd, ptr(th), ptr(bt2), ptr(bls),
                                         ptr(bld), ptr(bm), ptr(bi), ptr(tg), *ctx.cfg, ptr(scratch), ptr(go),
                                         *[ptr(x) for x in grads], stream()))
        grads = [x.reshape(s) if x is not None else None for x, s in zip(grads, ctx.shapes)]
        return (None, None, None) + tuple(grads) + (None,) * 7


class PerspectiveTransformFn(torch.autograd.Function):
    """(vertices [n,V,3], zooms [n,1]) = zoom_fit(shear(R(q) (v * s) + t))  -- derender3d/models/transforms.py:102-158 for
    a whole frame in two launches (forward) / three (backward) instead of ~25 element-wise ops and a batched GEMM."""

    @staticmethod
    def forward(ctx, vertices, scales, rotations, translations, persp, zoom_tos, zooms_given=None):
        """zoom_tos [n,1]: zoom-to-fit (test-time form); zooms_given [n,1] (then zoom_tos is None): the training form."""
        v = _f32(vertices, 'vertices')
        n, V, three = v.shape
        if three != 3:
            raise ValueError('vertices must be [n, V, 3]')
        s = _f32(scales, 'scales').reshape(n, 3)
        q = _f32(rotations, 'rotations').reshape(n, 4)
        t = _f32(translations, 'translations').reshape(n, 3)
        p = _f32(persp, 'perspective_translations').reshape(n, 3)
        fixed = zooms_given is not None
        if fixed:
            zg = _f32(zooms_given, 'zooms').reshape(n)
            zt = const_f32([1.0] * n, v.device)   # the backward kernels see zoom = key_ratio * 1 (a cached constant: no fill launch)
        else:
            zg = None
            zt = _f32(zoom_tos, 'zoom_tos').reshape(n)
        out = torch.empty_like(v)
        zooms = torch.empty(n, dtype=torch.float32, device=v.device)
        key = torch.empty(_ptf_scratch(n, V)[0], dtype=torch.uint8, device=v.device)   # key[n] + the per-block minima
        check(lib().sdn_perspective_transform(ptr(v), ptr(s), ptr(q), ptr(t), ptr(p), ptr(zt), ptr(zg), n, V, ptr(out),
                                              ptr(zooms), ptr(key), stream()))
        ctx.save_for_backward(v, s, q, t, p, zt, out, key, zg)
        ctx.shapes = (scales.shape, rotations.shape, translations.shape, persp.shape,
                      (zooms_given if fixed else zoom_tos).shape)
        ctx.fixed = fixed
        # Derenderer3d.render passes ONE tensor as translations and perspective_translations (derender3d/models/__init__.py:185-190):
        # autograd would add the two gradients with an element-wise launch; the library adds them when handed one pointer for both
        ctx.same_tp = translations is persp
        # (the zooms usually take no gradient -- the frame step's loss never reads them: autograd would hand backward a freshly
        # zero-filled tensor for them, one fill launch per step)
        ctx.set_materialize_grads(False)
        return out, zooms.reshape(n, 1)

    @staticmethod
    def backward(ctx, g_out, g_zooms):
        v, s, q, t, p, zt, out, key, zg = ctx.saved_tensors
        n, V, _ = v.shape
        dev = v.device
        if g_out is None and g_zooms is None:
            return (None,) * 7
        g_out = g_out.contiguous() if g_out is not None else torch.zeros_like(v)
        gz = g_zooms.reshape(n).contiguous() if g_zooms is not None else None
        gv = torch.empty_like(v)
        gs = torch.empty(n, 3, dtype=torch.float32, device=dev)
        gq = torch.empty(n, 4, dtype=torch.float32, device=dev)
        gt = torch.empty(n, 3, dtype=torch.float32, device=dev)
        gp = gt if ctx.same_tp else torch.empty(n, 3, dtype=torch.float32, device=dev)
        gzt = torch.empty(n, dtype=torch.float32, device=dev)
        acc = torch.empty(_ptf_scratch(n, V)[1], dtype=torch.uint8, device=dev)
        check(lib().sdn_perspective_transform_bwd(ptr(v), ptr(s), ptr(q), ptr(t), ptr(p), ptr(zt), n, V, ptr(out), ptr(key),
                                                  ptr(g_out), ptr(gz), ptr(gv), ptr(gs), ptr(gq), ptr(gt), ptr(gp),
                                                  ptr(gzt), ptr(acc), stream()))
        sh = ctx.shapes
        gpr = None if ctx.same_tp else gp.reshape(sh[3])   # (same tensor: gt already holds the sum)
        if ctx.fixed:   # the kernel reports d / d zoom_to at zoom_to = 1, zoom = zooms_given * zoom_to
            gzg = (gzt / zg).reshape(sh[4]) if ctx.needs_input_grad[6] else None   # (the optimisation loop's zooms are constants)
            return gv, gs.reshape(sh[0]), gq.reshape(sh[1]), gt.reshape(sh[2]), gpr, None, gzg
        return gv, gs.reshape(sh[0]), gq.reshape(sh[1]), gt.reshape(sh[2]), gpr, gzt.reshape(sh[4]), None


class SegmentMeanFn(torch.autograd.Function):
    """Instance-wise average pooling (textural/models/networks.py:310-325): out[n, c, p] = mean of x[., c, .] over the
    pixels that share p's segment id.  `seg` [N, H, W] int32 holds dense ids in [0, K).  Returns (out, means [C, K]).
    d out / d x is the same averaging operator (it is symmetric and idempotent), so backward is one more call."""

    @staticmethod
    def forward(ctx, x, seg, K):
        x = _f32(x, 'x')
        if seg.dtype != torch.int32 or not seg.is_cuda:
            raise TypeError('seg must be an int32 CUDA tensor')
        N, C, H, W = x.shape
        seg = seg.contiguous()
        sums = torch.empty(C, K, dtype=torch.float32, device=x.device)
        counts = torch.empty(K, dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        check(lib().sdn_segment_mean(ptr(x), ptr(seg), N, C, H * W, K, ptr(sums), ptr(counts), ptr(out), stream()))
        ctx.save_for_backward(seg)
        ctx.K = K
        means = sums / counts
        ctx.mark_non_differentiable(means)
        return out, means

    @staticmethod
    def backward(ctx, g_out, g_means):
        (seg,) = ctx.saved_tensors
        g = g_out.contiguous()
        N, C, H, W = g.shape
        K = ctx.K
        sums = torch.empty(C, K, dtype=torch.float32, device=g.device)
        counts = torch.empty(K, dtype=torch.float32, device=g.device)
        gx = torch.empty_like(g)
        check(lib().sdn_segment_mean(ptr(g), ptr(seg), N, C, H * W, K, ptr(sums), ptr(counts), ptr(gx), stream()))
        return gx, None, None


class AvgPool3x3S2Fn(torch.autograd.Function):
    """nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False) on [N, C, H, W] fp32 (any strides; channels-last
    views stay channels-last): textural/models/networks.py:190, 392, 406.  Own kernels because torch's backward of this op
    is wrong on ROCm for channels-last-strided inputs (csrc/fast_pool.hip)."""

    @staticmethod
    def forward(ctx, x):
        x = want_strided(x, 'input')
        N, C, H, W = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        inner_c = x.stride(1) == 1 and C > 1
        if inner_c:
            out = torch.empty((N, OH, OW, C), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
        else:
            out = torch.empty((N, C, OH, OW), dtype=torch.float32, device=x.device)
        L4 = ctypes.c_long * 4
        check(lib().sdn_avgpool3x3s2_fwd(ptr(x), N, C, H, W, L4(*x.stride()), ptr(out), L4(*out.stride()), int(inner_c),
                                         stream()))
        ctx.shape, ctx.inner_c = (N, C, H, W), inner_c
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W = ctx.shape
        g = want_strided(g, 'grad')
        if ctx.inner_c:
            gin = torch.empty((N, H, W, C), dtype=torch.float32, device=g.device).permute(0, 3, 1, 2)
        else:
            gin = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
        L4 = ctypes.c_long * 4
        check(lib().sdn_avgpool3x3s2_bwd(ptr(g), N, C, H, W, L4(*g.stride()), ptr(gin), L4(*gin.stride()), int(ctx.inner_c),
                                         stream()))
        return gin


def want_strided(t, name):
    """fp32 GPU tensor of any (non-overlapping) strides: no copy is made"""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise NotImplementedError('%s is on %s; this op only runs on the GPU' % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError('%s must be float32, got %s' % (name, t.dtype))
    if t.dim() != 4:
        raise ValueError('%s must be [N, C, H, W]' % name)
    return t


def avg_pool_3x3_s2(x):
    return AvgPool3x3S2Fn.apply(x)


def _dense_flat(t):
    """1-D view over the storage of a dense (non-overlapping, gap-free) tensor in memory order, or None."""
    order = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))
    p = t.permute(order)
    return p.reshape(-1) if p.is_contiguous() else None


def l1_loss_supported(a, b):
    """Both operands fp32 on the GPU, same shape and strides, dense and 16-byte aligned: what L1LossFn takes."""
    return (a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape
            and a.stride() == b.stride() and a.numel() > 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and _dense_flat(a) is not None)


class L1LossFn(torch.autograd.Function):
    """torch.nn.L1Loss()(a, b) = mean |a - b| as one read of both operands, the gradient as one more read and one write
    (csrc/fast_loss.hip).  The operands are walked in MEMORY order: they must share one dense layout (the discriminator
    feature maps are NCHW views of channels-last buffers), see l1_loss_supported."""

    @staticmethod
    def forward(ctx, a, b):
        if not l1_loss_supported(a, b):
            raise ValueError('L1LossFn: operands must be fp32 CUDA tensors of one dense, 16-byte aligned layout')
        fa, fb = _dense_flat(a), _dense_flat(b)
        acc = torch.empty(1, dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        check(lib().sdn_l1_loss_fwd(ptr(fa), ptr(fb), fa.numel(), ptr(acc), ptr(out), stream()))
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad
        g = g.to(torch.float32).reshape(1).contiguous()
        ga = torch.empty_like(a) if need_a else None   # preserve_format: the operands' own (dense) strides
        gb = torch.empty_like(b) if need_b else None
        if ga is None and gb is None:
            return None, None
        fga = _dense_flat(ga) if ga is not None else None
        fgb = _dense_flat(gb) if gb is not None else None
        if (ga is not None and (fga is None or ga.stride() != a.stride())) or \
                (gb is not None and (fgb is None or gb.stride() != a.stride())):
            raise RuntimeError('L1LossFn: empty_like did not keep the operands\' layout')
        check(lib().sdn_l1_loss_bwd(ptr(_dense_flat(a)), ptr(_dense_flat(b)), a.numel(), ptr(g), ptr(fga), ptr(fgb), stream()))
        return ga, gb


def edit_assemble(base_segm, edit_inst, obj_label, obj_pose, code_ids, codes, pose_channels=1):
    """The textural inputs of F edited frames in one launch (textural/edit_vkitti.py:62-103, edit_benchmark.py:87-126;
    csrc/fast_edit.hip).  base_segm [1 | F, 1, H, W] fp32 (one source label map for all frames, or one per frame),
    edit_inst [F, 1, H, W] uint8 raw object ids, obj_label / obj_pose [F, 256] int32 tables by raw id, code_ids [K] int32
    ascending, codes [C, K] fp32.  Returns (segm [F,1,H,W], inst [F,1,H,W], pose [F,pose_channels,H,W], feat [F,C,H,W],
    missing [F] int32): fp32 maps -- Pix2PixHDModel.encode_input converts label and pose to indices itself -- and, per
    frame, the number of pixels whose instance has no code (painted 0).  Nothing is copied to the host."""
    base_segm = _f32(base_segm, 'base_segm')
    edit_inst = want(edit_inst, torch.uint8, 'edit_inst')
    obj_label = want(obj_label, torch.int32, 'obj_label')
    obj_pose = want(obj_pose, torch.int32, 'obj_pose')
    code_ids = want(code_ids, torch.int32, 'code_ids')
    codes = _f32(codes, 'codes')
    if edit_inst.dim() != 4 or edit_inst.shape[1] != 1:
        raise ValueError('edit_inst must be [F, 1, H, W], got %s' % (tuple(edit_inst.shape),))
    F, _, H, W = edit_inst.shape
    if base_segm.dim() != 4 or tuple(base_segm.shape[1:]) != (1, H, W) or base_segm.shape[0] not in (1, F):
        raise ValueError('base_segm must be [1 or %d, 1, %d, %d], got %s' % (F, H, W, tuple(base_segm.shape)))
    if tuple(obj_label.shape) != (F, 256) or tuple(obj_pose.shape) != (F, 256):
        raise ValueError('obj_label and obj_pose must be [%d, 256]' % F)
    if code_ids.dim() != 1 or codes.dim() != 2 or codes.shape[1] != code_ids.shape[0] or code_ids.numel() < 1:
        raise ValueError('code_ids must be [K] and codes [C, K], got %s and %s' % (tuple(code_ids.shape), tuple(codes.shape)))
    if pose_channels not in (1, 2):
        raise ValueError('pose_channels must be 1 (binned pose) or 2 (feat_pose_num_bins == 0)')
    dev = edit_inst.device
    _on_device_of('edit_inst', dev, (('base_segm', base_segm), ('obj_label', obj_label), ('obj_pose', obj_pose), ('code_ids', code_ids),
                                     ('codes', codes)))
    C, K = codes.shape
    with torch.cuda.device(dev):   # the stream handed over is this device's current one
        segm = torch.empty(F, 1, H, W, dtype=torch.float32, device=dev)
        inst = torch.empty(F, 1, H, W, dtype=torch.float32, device=dev)
        pose = torch.empty(F, pose_channels, H, W, dtype=torch.float32, device=dev)
        feat = torch.empty(F, C, H, W, dtype=torch.float32, device=dev)
        missing = torch.empty(F, dtype=torch.int32, device=dev)
        check(lib().sdn_edit_assemble(ptr(base_segm), 0 if base_segm.shape[0] == 1 and F > 1 else H * W, ptr(edit_inst),
                                      ptr(obj_label), ptr(obj_pose), ptr(code_ids), ptr(codes), K, C, F, H * W, pose_channels,
                                      ptr(segm), ptr(inst), ptr(pose), ptr(feat), ptr(missing), stream()))
    return segm, inst, pose, feat, missing


SCENE_RGB, SCENE_MASK, SCENE_IGNORE = 1, 2, 4   # `kinds` of sdn_scene_crops


def scene_cover(masks):
    """Cover words of N BINARY maps (csrc/scene_crops.hip): masks [N, 1, H, W] fp32, every value exactly 0.0 or 1.0 (what
    Mask R-CNN delivers; verified only with SDN_DEBUG_CHECKS=1 in the environment, which makes the call synchronous) ->
    uint32 words as an int32 tensor [ceil(N / 32), H, W]: bit (n & 31) of word n // 32 is set where map n is.  Nothing is
    copied to the host."""
    masks = _f32(masks, 'masks')
    if masks.dim() != 4 or masks.shape[1] != 1 or masks.shape[0] < 1:
        raise ValueError('masks must be [N, 1, H, W] with N >= 1, got %s' % (tuple(masks.shape),))
    N, _, H, W = masks.shape
    with torch.cuda.device(masks.device):
        cover = torch.empty((N + 31) // 32, H, W, dtype=torch.int32, device=masks.device)
        check(lib().sdn_scene_cover(ptr(masks), N, H, W, ptr(cover), stream()))
    return cover


def scene_crops(kinds, rois_host, tables, H, W, image_size, mask_size, frame_u8=None, cover=None, ignore_cover=None, nearer=None,
                mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25)):
    """All per-object crops of one frame in one launch (sdn_scene_crops; geometric/scripts/main.py:365-373, 418-421 with
    derender3d/datasets.py:49-71, 141-172): crop_square + PIL bilinear resize + to_tensor (+ Normalize for the image), bit
    for bit.  kinds: a sum of SCENE_RGB (needs frame_u8 uint8 [3, H, W]), SCENE_MASK (needs cover = scene_cover(masks);
    the masks must be binary) and SCENE_IGNORE (needs ignore_cover and nearer int64 [N, ceil(N / 32)]).  rois_host: numpy
    int32 [N, 4] = (y0, x0, y1, x1); tables = (objs [N, 12], bounds, kk8) int32 CUDA tensors as
    derender3d.scene.crop_tables prepares them.  Returns (rgbs [N,3,S_i,S_i], masks [N,1,S_m,S_m], ignores [N,1,S_m,S_m]),
    None for a kind not asked for.  Nothing is copied to the host."""
    rois_host = np.ascontiguousarray(rois_host, dtype=np.int32)
    if rois_host.ndim != 2 or rois_host.shape[1] != 4:
        raise ValueError('rois must be [N, 4], got %s' % (rois_host.shape,))
    N = rois_host.shape[0]
    objs, bounds, kk8 = (want(t, torch.int32, name) for t, name in zip(tables, ('objs', 'bounds', 'kk8')))
    if tuple(objs.shape) != (N, 12):
        raise ValueError('objs must be [%d, 12] for %d rois, got %s' % (N, N, tuple(objs.shape)))
    dev = objs.device
    chunks = (N + 31) // 32
    if kinds & SCENE_RGB:
        frame_u8 = want(frame_u8, torch.uint8, 'frame_u8')
        if frame_u8 is None or tuple(frame_u8.shape) != (3, H, W):
            raise ValueError('frame_u8 must be uint8 [3, %d, %d]' % (H, W))
    if kinds & SCENE_MASK:
        cover = want(cover, torch.int32, 'cover')
    if kinds & SCENE_IGNORE:
        ignore_cover = want(ignore_cover, torch.int32, 'ignore_cover')
    for t, name, need in ((cover, 'cover', kinds & SCENE_MASK), (ignore_cover, 'ignore_cover', kinds & SCENE_IGNORE)):
        if need and (t is None or tuple(t.shape) != (chunks, H, W)):
            raise ValueError('%s must be the int32 [%d, %d, %d] tensor of scene_cover for %d objects' % (name, chunks, H, W, N))
    if kinds & SCENE_IGNORE:
        nearer = want(nearer, torch.int64, 'nearer')
        if nearer is None or tuple(nearer.shape) != (N, chunks):
            raise ValueError('nearer must be int64 [%d, %d]' % (N, chunks))
    with torch.cuda.device(dev):
        rgbs = torch.empty(N, 3, image_size, image_size, device=dev) if kinds & SCENE_RGB else None
        masks = torch.empty(N, 1, mask_size, mask_size, device=dev) if kinds & SCENE_MASK else None
        ignores = torch.empty(N, 1, mask_size, mask_size, device=dev) if kinds & SCENE_IGNORE else None
        check(lib().sdn_scene_crops(ptr(frame_u8) if kinds & SCENE_RGB else None, ptr(cover) if kinds & SCENE_MASK else None,
                                    ptr(ignore_cover) if kinds & SCENE_IGNORE else None, ptr(nearer) if kinds & SCENE_IGNORE else None,
                                    rois_host.ctypes.data, ptr(objs), ptr(bounds), ptr(kk8), N, H, W, image_size, mask_size, kinds,
                                    float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]), float(std[2]),
                                    ptr(rgbs), ptr(masks), ptr(ignores), stream()))
    return rgbs, masks, ignores


def scene_edit(theta_deltas, translation2ds, log_depths, mroi_norms, droi_norms, interests, records):
    """F edit lists applied to one de-rendered scene in one launch (sdn_scene_edit; geometric/scripts/main.py:481-514).
    theta_deltas, translation2ds, mroi_norms, droi_norms [N, 2], log_depths [N, 1] fp32, interests uint8 [N], records int32
    [F, P, 8] (derender3d.scene.edit_records), all CUDA.  Returns (theta_deltas [F,N,2], translation2ds [F,N,2], log_depths
    [F,N,1], interests uint8 [F,N]), bit-equal to the reference's element-wise torch statements.  Nothing is copied to the
    host."""
    th, tr, ld, mr, dr = (_f32(t, name) for t, name in ((theta_deltas, 'theta_deltas'), (translation2ds, 'translation2ds'),
                                                        (log_depths, 'log_depths'), (mroi_norms, 'mroi_norms'),
                                                        (droi_norms, 'droi_norms')))
    interests = want(interests, torch.uint8, 'interests')
    records = want(records, torch.int32, 'records')
    N = th.shape[0]
    if N < 1 or any(tuple(t.shape) != (N, 2) for t in (th, tr, mr, dr)) or ld.numel() != N or interests.numel() != N:
        raise ValueError('scene_edit: theta_deltas, translation2ds, mroi_norms, droi_norms must be [N, 2], log_depths [N, 1], '
                         'interests [N]; got %s' % ([tuple(t.shape) for t in (th, tr, ld, mr, dr, interests)],))
    if records.dim() != 3 or records.shape[2] != 8 or records.shape[0] < 1:
        raise ValueError('records must be int32 [F, P, 8], got %s' % (tuple(records.shape),))
    F, P = records.shape[0], records.shape[1]
    dev = th.device
    with torch.cuda.device(dev):
        o_th = torch.empty(F, N, 2, device=dev)
        o_tr = torch.empty(F, N, 2, device=dev)
        o_ld = torch.empty(F, N, 1, device=dev)
        o_in = torch.empty(F, N, dtype=torch.uint8, device=dev)
        check(lib().sdn_scene_edit(ptr(th), ptr(tr), ptr(ld), ptr(mr), ptr(dr), ptr(interests), ptr(records) if P else None, F, N,
                                   P, ptr(o_th), ptr(o_tr), ptr(o_ld), ptr(o_in), stream()))
    return o_th, o_tr, o_ld, o_in


UNMOLD_OBJ_INTS = 12   # one row of sdn_unmold_masks's object table


def unmold_masks(mrcnn_mask, objs_host, tables, H, W, planes=True, areas=True):
    """Mask R-CNN's soft masks as binary full-frame planes, all objects in one launch (sdn_unmold_masks; maskrcnn/utils.py:
    378-395 per detection on the host): bytescale, Pillow's bilinear resize to the box, >= 0.5, paste -- bit for bit.
    mrcnn_mask [D, C, Mh, Mw] fp32 CUDA in the network's own layout; objs_host numpy int32 [n, 12] rows (detection index,
    class id, y1, x1, y2, x2, tables of the rows, tables of the columns) and tables = (objs [n, 12], bounds, kk8) int32 CUDA
    tensors as geometric/maskrcnn/detections.unmold_tables prepares them.  Returns (masks [n, 1, H, W] fp32 holding 0.0 / 1.0
    or None, areas int32 [n] or None); planes=False makes only the areas.  Nothing is copied to the host."""
    mrcnn_mask = _f32(mrcnn_mask, 'mrcnn_mask')
    if mrcnn_mask.dim() != 4:
        raise ValueError('mrcnn_mask must be [D, C, Mh, Mw], got %s' % (tuple(mrcnn_mask.shape),))
    if not (planes or areas):
        raise ValueError('neither planes nor areas asked for')
    objs_host = np.ascontiguousarray(objs_host, dtype=np.int32)
    if objs_host.ndim != 2 or objs_host.shape[1] != UNMOLD_OBJ_INTS or objs_host.shape[0] < 1:
        raise ValueError('objs_host must be int32 [n, %d] with n >= 1, got %s' % (UNMOLD_OBJ_INTS, objs_host.shape))
    n = objs_host.shape[0]
    objs, bounds, kk8 = (want(t, torch.int32, name) for t, name in zip(tables, ('objs', 'bounds', 'kk8')))
    if tuple(objs.shape) != (n, UNMOLD_OBJ_INTS):
        raise ValueError('objs must be [%d, %d], got %s' % (n, UNMOLD_OBJ_INTS, tuple(objs.shape)))
    if bounds.dim() != 2 or bounds.shape[1] != 2 or kk8.dim() != 1:
        raise ValueError('bounds must be [M, 2] and kk8 [K], got %s, %s' % (tuple(bounds.shape), tuple(kk8.shape)))
    D, C, Mh, Mw = mrcnn_mask.shape
    dev = mrcnn_mask.device
    with torch.cuda.device(dev):
        masks = torch.empty(n, 1, H, W, device=dev) if planes else None
        counts = torch.empty(n, dtype=torch.int32, device=dev) if areas else None
        check(lib().sdn_unmold_masks(ptr(mrcnn_mask), D, C, Mh, Mw, objs_host.ctypes.data, ptr(objs), n, ptr(bounds), bounds.shape[0],
                                     ptr(kk8), kk8.shape[0], H, W, ptr(masks), ptr(counts), stream()))
    return masks, counts


def scene_gt_masks(scene_u8, codes):
    """--source gt (sdn_scene_gt_masks; geometric/scripts/main.py:745-746 with derender3d/datasets.py:75-76, 95-103 per object
    on the host): scene_u8 uint8 [H, W, 3] CUDA, the instance-colour image; codes uint8 [K, 3] CUDA.  Returns (masks
    [K, 1, H, W] fp32 = all(scene == code, axis 2), rois int32 [K, 4] = (first row, first column, last row + 1, last column
    + 1), areas int32 [K]).  A code that matches nothing has area 0 and an invalid roi (first > last); mask_to_roi raises for
    it, and derender3d.scene.scene_gt_inputs does.  Nothing is copied to the host."""
    scene_u8 = want(scene_u8, torch.uint8, 'scene_u8')
    codes = want(codes, torch.uint8, 'codes')
    if scene_u8.dim() != 3 or scene_u8.shape[2] != 3:
        raise ValueError('scene_u8 must be uint8 [H, W, 3], got %s' % (tuple(scene_u8.shape),))
    if codes.dim() != 2 or codes.shape[1] != 3 or codes.shape[0] < 1:
        raise ValueError('codes must be uint8 [K, 3] with K >= 1, got %s' % (tuple(codes.shape),))
    _on_device_of('scene_u8', scene_u8.device, (('codes', codes),))
    H, W, K = scene_u8.shape[0], scene_u8.shape[1], codes.shape[0]
    dev = scene_u8.device
    with torch.cuda.device(dev):
        masks = torch.empty(K, 1, H, W, device=dev)
        rois = torch.empty(K, 4, dtype=torch.int32, device=dev)
        areas = torch.empty(K, dtype=torch.int32, device=dev)
        check(lib().sdn_scene_gt_masks(ptr(scene_u8), ptr(codes), K, H, W, ptr(masks), ptr(rois), ptr(areas), stream()))
    return masks, rois, areas


SCENE_ID_OBJS, SCENE_ID_COLS = 1000, 8   # the table of sdn_scene_id_stats: one row per id of the category


def _id_maps(scene, disparity):
    scene = want(scene, torch.int32, 'scene')
    disparity = want(disparity, torch.int32, 'disparity')
    if scene.dim() != 2 or scene.numel() < 1:
        raise ValueError('scene must be int32 [H, W], got %s' % (tuple(scene.shape),))
    if tuple(disparity.shape) != tuple(scene.shape):
        raise ValueError('disparity must be int32 %s as the scene, got %s' % (tuple(scene.shape), tuple(disparity.shape)))
    _on_device_of('scene', scene.device, (('disparity', disparity),))
    return scene, disparity


def scene_id_stats(scene, disparity, category=26):
    """--dataset cityscapes --source gt, the statistics (sdn_scene_id_stats; geometric/scripts/main.py:766-780 with
    derender3d/datasets.py:95-103 per object on the host): scene int32 [H, W] CUDA, the instance-id map (id = category * 1000 +
    k); disparity int32 [H, W] CUDA with values in 0 .. 65535 (verified only with SDN_DEBUG_CHECKS=1 in the environment, which
    makes the call synchronous).  Returns the table int32 [1000, 8], row j = id - 1000 category: (area, y0, x0, y1, x1, n, lo,
    hi) -- pixel count, roi as mask_to_roi, the number of non-zero disparities under the mask and their order statistics of
    rank floor((n - 1) 0.95) and the next (0, 0 when n == 0): what np.percentile(., 95) interpolates between.  An absent id has
    area 0 and an invalid roi.  Nothing is copied to the host."""
    scene, disparity = _id_maps(scene, disparity)
    H, W = scene.shape
    dev = scene.device
    with torch.cuda.device(dev):
        table = torch.empty(SCENE_ID_OBJS, SCENE_ID_COLS, dtype=torch.int32, device=dev)
        workspace = scene_id_workspace(dev)
        check(lib().sdn_scene_id_stats(ptr(scene), ptr(disparity), int(category), H, W, ptr(table), ptr(workspace), stream()))
    return table


def scene_id_planes(scene, disparity, ids, thr, planes=True, ignore_planes=False, cover=True):
    """The scene inputs of n selected ids in one launch (sdn_scene_id_planes; main.py:770-786): scene, disparity int32 [H, W]
    CUDA; ids int32 [n] CUDA, the full instance ids; thr int32 [n] CUDA, floor(np.percentile(.., 95)) of each object
    (derender3d.scene.percentile95_threshold).  Returns (masks fp32 [n, 1, H, W] = scene == ids[k] or None, ignore_cover: uint32
    words as an int32 tensor [ceil(n / 32), H, W] in the layout of scene_cover, bit k set where disparity > thr[k], or None,
    ignores fp32 [n, 1, H, W] of the same predicate or None).  planes / cover: not both False.  Nothing is copied to the host."""
    scene, disparity = _id_maps(scene, disparity)
    ids = want(ids, torch.int32, 'ids')
    thr = want(thr, torch.int32, 'thr')
    if ids.dim() != 1 or ids.shape[0] < 1 or tuple(thr.shape) != tuple(ids.shape):
        raise ValueError('ids and thr must be int32 [n] with n >= 1, got %s and %s' % (tuple(ids.shape), tuple(thr.shape)))
    if not (planes or cover):
        raise ValueError('neither planes nor cover asked for')
    dev = scene.device
    _on_device_of('scene', dev, (('ids', ids), ('thr', thr)))
    H, W = scene.shape
    n = ids.shape[0]
    with torch.cuda.device(dev):
        masks = torch.empty(n, 1, H, W, device=dev) if planes else None
        words = torch.empty((n + 31) // 32, H, W, dtype=torch.int32, device=dev) if cover else None
        ignores = torch.empty(n, 1, H, W, device=dev) if ignore_planes else None
        check(lib().sdn_scene_id_planes(ptr(scene), ptr(disparity), ptr(ids), ptr(thr), n, H, W, ptr(masks), ptr(words), ptr(ignores),
                                        stream()))
    return masks, words, ignores


PAINT2D_REC_INTS = 16   # one row of sdn_scene_paint2d's record table


def scene_paint2d(cover, n, records_host=None, tables=None, frames=1):
    """The 2D / 2D+ baselines' instance maps, F frames in one launch (sdn_scene_paint2d; geometric/scripts/main.py:293-312 per
    object and frame on the host): every object's mask window resized by Pillow's bilinear filter and pasted, objects in index
    order -- bit for bit.  cover: scene_cover(masks) of the n = N masks, int32 [ceil(N / 32), H, W]; records_host numpy int32 [F, N, 16] rows
    (active, window r0, c0, h, w, output h', w', paste top, left, tables of the rows, tables of the columns, unused) and
    tables = (records [F, N, 16], bounds [M, 2], kk8 [K]) int32 CUDA tensors as derender3d.scene2d.paint_tables prepares
    them.  Without records ("identity") `frames` copies of the unedited masks painted in index order (main.py:236-238).
    Returns uint8 [F, 1, H, W]: object index + 1, 0 where nothing is.  Nothing is copied to the host."""
    cover = want(cover, torch.int32, 'cover')
    if cover.dim() != 3:
        raise ValueError('cover must be the int32 [ceil(N / 32), H, W] tensor of scene_cover, got %s' % (tuple(cover.shape),))
    chunks, H, W = cover.shape
    dev = cover.device
    N = int(n)
    if (N + 31) // 32 != chunks:
        raise ValueError('cover holds %d words per pixel, %d objects need %d' % (chunks, N, (N + 31) // 32))
    if records_host is None:
        if tables is not None:
            raise ValueError('scene_paint2d: tables without records_host')
        F = int(frames)
        with torch.cuda.device(dev):
            out = torch.empty(F, 1, H, W, dtype=torch.uint8, device=dev)
            check(lib().sdn_scene_paint2d(ptr(cover), None, None, F, N, None, 0, None, 0, H, W, ptr(out), stream()))
        return out
    records_host = np.ascontiguousarray(records_host, dtype=np.int32)
    if records_host.ndim != 3 or records_host.shape[2] != PAINT2D_REC_INTS or records_host.shape[0] < 1 or records_host.shape[1] < 1:
        raise ValueError('records_host must be int32 [F, N, %d] with F, N >= 1, got %s' % (PAINT2D_REC_INTS, records_host.shape))
    F = records_host.shape[0]
    if records_host.shape[1] != N:
        raise ValueError('records_host holds %d objects per frame, n is %d' % (records_host.shape[1], N))
    recs, bounds, kk8 = (want(t, torch.int32, name) for t, name in zip(tables, ('records', 'bounds', 'kk8')))
    if tuple(recs.shape) != (F, N, PAINT2D_REC_INTS):
        raise ValueError('records must be [%d, %d, %d], got %s' % (F, N, PAINT2D_REC_INTS, tuple(recs.shape)))
    if bounds.dim() != 2 or bounds.shape[1] != 2 or kk8.dim() != 1:
        raise ValueError('bounds must be [M, 2] and kk8 [K], got %s, %s' % (tuple(bounds.shape), tuple(kk8.shape)))
    _on_device_of('cover', dev, (('records', recs), ('bounds', bounds), ('kk8', kk8)))
    with torch.cuda.device(dev):
        out = torch.empty(F, 1, H, W, dtype=torch.uint8, device=dev)
        check(lib().sdn_scene_paint2d(ptr(cover), records_host.ctypes.data, ptr(recs), F, N, ptr(bounds), bounds.shape[0],
                                      ptr(kk8), kk8.shape[0], H, W, ptr(out), stream()))
    return out


ASSEMBLE_INST_NONE, ASSEMBLE_INST_TABLE, ASSEMBLE_INST_FILL, ASSEMBLE_INST_INT = 0, 1, 2, 3   # `inst_mode` of sdn_assemble_maps


def _assemble_items(items_host, items, name):
    items_host = np.ascontiguousarray(items_host, dtype=np.int32)
    if items_host.ndim != 2 or items_host.shape[1] != 4 or items_host.shape[0] < 1:
        raise ValueError('%s: items_host must be int32 [B, 4] with B >= 1, got %s' % (name, items_host.shape))
    items = want(items, torch.int32, 'items')
    if tuple(items.shape) != items_host.shape:
        raise ValueError('%s: items must be int32 %s as items_host, got %s' % (name, items_host.shape, tuple(items.shape)))
    return items_host, items


def _assemble_on(dev, name, tensors):
    for t, n in tensors:
        if t is not None and t.device != dev:
            raise ValueError('%s: %s is on %s, items on %s' % (name, n, t.device, dev))


def assemble_planes(src, items_host, items, xtab, ytab, lut, C, H, W, sh, sw, h, w, normalize=True, mean=0.5, std=0.5, add=None):
    """get_transform(opt, params)(image) for B items x C uint8 planes in one launch (sdn_assemble_planes; textural/data/
    base_dataset.py:41-66 per item with PIL on the host): Pillow's resize [H, W] -> [sh, sw] evaluated only inside each item's crop
    window [h, w], flip, ToTensor, Normalize, + add -- bit for bit.  src int64 [B] CUDA: the address of each item's uint8
    [C, H, W] map, 0 for an absent map (planes of 0.0); items_host numpy int32 [B, 4] rows (crop x1, y1, flip, unused) and
    items, the same on the device; xtab = (xmin int32 [sw], xk int32 [sw, taps]) or None exactly when sw == W, ytab likewise
    for the rows; lut fp32 [256] (ToTensor).  The caller keeps the maps alive.  Returns fp32 [B, C, h, w].  Nothing is copied
    to the host."""
    items_host, items = _assemble_items(items_host, items, 'assemble_planes')
    B = items_host.shape[0]
    src = want(src, torch.int64, 'src')
    lut = _f32(lut, 'lut')
    if tuple(src.shape) != (B,) or tuple(lut.shape) != (256,):
        raise ValueError('assemble_planes: src must be int64 [%d] and lut fp32 [256], got %s and %s'
                         % (B, tuple(src.shape), tuple(lut.shape)))
    tabs = []
    for tab, n, axis in ((xtab, sw, 'x'), (ytab, sh, 'y')):
        if tab is None:
            tabs.append((None, None, 0))
            continue
        lo, k = want(tab[0], torch.int32, axis + 'min'), want(tab[1], torch.int32, axis + 'k')
        if tuple(lo.shape) != (n,) or k.dim() != 2 or k.shape[0] != n or k.shape[1] < 1:
            raise ValueError('assemble_planes: %smin must be int32 [%d] and %sk [%d, taps], got %s and %s'
                             % (axis, n, axis, n, tuple(lo.shape), tuple(k.shape)))
        tabs.append((lo, k, k.shape[1]))
    dev = items.device
    _assemble_on(dev, 'assemble_planes', [(src, 'src'), (lut, 'lut')] + [(t, 'a table') for tab in tabs for t in tab[:2]])
    with torch.cuda.device(dev):
        out = torch.empty(B, C, h, w, dtype=torch.float32, device=dev)
        check(lib().sdn_assemble_planes(ptr(src), items_host.ctypes.data, ptr(items), ptr(tabs[0][0]), ptr(tabs[0][1]), tabs[0][2],
                                        ptr(tabs[1][0]), ptr(tabs[1][1]), tabs[1][2], ptr(lut), B, C, H, W, sh, sw, h, w,
                                        int(bool(normalize)), float(mean), float(std), int(add is not None),
                                        float(add) if add is not None else 0.0, ptr(out), stream()))
    return out


def assemble_maps(segm, inst, pose, items_host, items, nx, ny, tabs, inst_mode, H, W, sh, sw, h, w, wrap16=False, pose_has=None,
                  pose_val=None, min_area=1, inst_nx=None, inst_ny=None):
    """The label, instance and pose maps of B items in two launches (sdn_assemble_maps; textural/data/vkitti_dataset.py:52-57,
    68-118 and cityscapes_dataset.py:41-42, 55-93, 102-105 per item on the host).  segm, inst, pose: int64 [B] CUDA address
    tables of the items' uint8 [H, W] maps (inst: int32 [H, W] maps for ASSEMBLE_INST_INT; an entry 0 = the map is absent: inst
    is the label, or 0 for ASSEMBLE_INST_INT, whose output is an integer tensor; inst None for ASSEMBLE_INST_NONE, pose None
    without the pose feature); items_host / items as for assemble_planes; nx int32 [sw], ny int32 [sh] NEAREST source indices,
    None exactly where the size does not change (inst_nx, inst_ny: other indices for the instance map of ASSEMBLE_INST_INT,
    each only where that size changes, see include/sdn_hip.h); tabs fp32 [4, 256] (label, label at an instance value of 0,
    fill of such an instance, instance value).  pose_has int32 [B, 256], pose_val int32 [B, 256] (bins) or fp32 [B, 256, 2]
    (cos, sin) by raw id; an id is painted where its transformed pixel count is >= min_area.  Returns (label fp32 [B,1,h,w],
    inst fp32 -- for ASSEMBLE_INST_INT int32, or int16 with wrap16 -- [B,1,h,w] or None, pose int32 [B,1,h,w] / fp32 [B,2,h,w]
    or None, missing int32 [B]: pixels of painted-size ids without a record).  Nothing is copied to the host."""
    items_host, items = _assemble_items(items_host, items, 'assemble_maps')
    B = items_host.shape[0]
    segm = want(segm, torch.int64, 'segm')
    inst = want(inst, torch.int64, 'inst')
    pose = want(pose, torch.int64, 'pose')
    nx = want(nx, torch.int32, 'nx')
    ny = want(ny, torch.int32, 'ny')
    inst_nx = want(inst_nx, torch.int32, 'inst_nx')
    inst_ny = want(inst_ny, torch.int32, 'inst_ny')
    tabs = _f32(tabs, 'tabs')
    for t, name in ((segm, 'segm'), (inst, 'inst'), (pose, 'pose')):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError('assemble_maps: %s must be int64 [%d], got %s' % (name, B, tuple(t.shape)))
    if tuple(tabs.shape) != (4, 256):
        raise ValueError('assemble_maps: tabs must be fp32 [4, 256], got %s' % (tuple(tabs.shape),))
    for t, n, name in ((nx, sw, 'nx'), (ny, sh, 'ny'), (inst_nx, sw, 'inst_nx'), (inst_ny, sh, 'inst_ny')):
        if t is not None and tuple(t.shape) != (n,):
            raise ValueError('assemble_maps: %s must be int32 [%d], got %s' % (name, n, tuple(t.shape)))
    if inst_mode not in (ASSEMBLE_INST_NONE, ASSEMBLE_INST_TABLE, ASSEMBLE_INST_FILL, ASSEMBLE_INST_INT):
        raise ValueError('assemble_maps: inst_mode %r' % (inst_mode,))
    if (inst_mode != ASSEMBLE_INST_NONE) != (inst is not None):
        raise ValueError('assemble_maps: an instance address table exactly when inst_mode is not ASSEMBLE_INST_NONE')
    ch = 0
    if pose is not None:
        pose_has = want(pose_has, torch.int32, 'pose_has')
        if pose_val is None or pose_has is None or pose_val.dtype not in (torch.int32, torch.float32):
            raise ValueError('assemble_maps: the pose plane needs pose_has int32 and pose_val int32 or fp32')
        pose_val = want(pose_val, pose_val.dtype, 'pose_val')
        ch = 1 if pose_val.dtype == torch.int32 else 2
        if tuple(pose_has.shape) != (B, 256) or tuple(pose_val.shape) != ((B, 256) if ch == 1 else (B, 256, 2)):
            raise ValueError('assemble_maps: pose_has must be [%d, 256] and pose_val int32 [%d, 256] or fp32 [%d, 256, 2], got %s, %s'
                             % (B, B, B, tuple(pose_has.shape), tuple(pose_val.shape)))
    dev = items.device
    _assemble_on(dev, 'assemble_maps', [(segm, 'segm'), (inst, 'inst'), (pose, 'pose'), (nx, 'nx'), (ny, 'ny'), (inst_nx, 'inst_nx'),
                                        (inst_ny, 'inst_ny'), (tabs, 'tabs'), (pose_has, 'pose_has'),
                                        (pose_val if pose is not None else None, 'pose_val')])
    with torch.cuda.device(dev):
        label = torch.empty(B, 1, h, w, dtype=torch.float32, device=dev)
        inst_out = None
        if inst_mode != ASSEMBLE_INST_NONE:
            kind = torch.float32 if inst_mode != ASSEMBLE_INST_INT else (torch.int16 if wrap16 else torch.int32)
            inst_out = torch.empty(B, 1, h, w, dtype=kind, device=dev)
        pose_out = counts = None
        if ch:
            pose_out = torch.empty(B, ch, h, w, dtype=torch.int32 if ch == 1 else torch.float32, device=dev)
            counts = torch.empty(B, 256, dtype=torch.int32, device=dev)
        missing = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib().sdn_assemble_maps(ptr(segm), ptr(inst), ptr(pose), items_host.ctypes.data, ptr(items), ptr(nx), ptr(ny),
                                      ptr(inst_nx), ptr(inst_ny), ptr(tabs), int(inst_mode), int(bool(wrap16)), B, H, W, sh, sw, h, w,
                                      ptr(label), ptr(inst_out), ptr(pose_has) if ch else None, ptr(pose_val) if ch else None,
                                      ch if ch else 1, int(min_area), ptr(pose_out), ptr(counts), ptr(missing), stream()))
    return label, inst_out, pose_out, missing


TRAIN_ITEM_INTS = 12   # one row of sdn_train_crops's item table
TRAIN_BRIGHTNESS, TRAIN_CONTRAST, TRAIN_SATURATION, TRAIN_HUE = 0, 1, 2, 3


def train_rois(scenes_u8, items):
    """The rois and pixel counts of B (frame, colour code) pairs over several frames in one call (sdn_train_rois;
    derender3d/datasets.py:345-347 per object on the host): scenes_u8 uint8 [Fr, H, W, 3] CUDA, items int32 [B, 4] CUDA rows
    (frame index, r, g, b).  Returns table int32 [B, 5] CUDA = (first row, first column, last row + 1, last column + 1, area) of
    all(scenes[frame] == code, axis 2); a code that matches nothing (or a frame index outside Fr) has the invalid row
    (INT_MAX, INT_MAX, 0, 0, 0) of scene_gt_masks.  Nothing is copied to the host."""
    scenes_u8 = want(scenes_u8, torch.uint8, 'scenes_u8')
    items = want(items, torch.int32, 'items')
    if scenes_u8.dim() != 4 or scenes_u8.shape[3] != 3 or scenes_u8.shape[0] < 1:
        raise ValueError('scenes_u8 must be uint8 [Fr, H, W, 3], got %s' % (tuple(scenes_u8.shape),))
    if items.dim() != 2 or items.shape[1] != 4 or items.shape[0] < 1:
        raise ValueError('items must be int32 [B, 4] with B >= 1, got %s' % (tuple(items.shape),))
    _on_device_of('scenes_u8', scenes_u8.device, (('items', items),))
    Fr, H, W, _ = scenes_u8.shape
    B = items.shape[0]
    with torch.cuda.device(items.device):
        table = torch.empty(B, 5, dtype=torch.int32, device=items.device)
        check(lib().sdn_train_rois(ptr(scenes_u8), ptr(items), Fr, B, H, W, ptr(table), stream()))
    return table


def train_crops(frames_u8, scenes_u8, rois_host, objs_host, items_host, tables, items, nearer, image_size=224, mask_size=256,
                mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25)):
    """The crops of B training items over several frames (sdn_train_crops; derender3d/datasets.py:141-172, 390-391, 415-417):
    crop_square + colour jitter + PIL bilinear resize + to_tensor (+ Normalize for the image), bit for bit.  frames_u8 uint8
    [Fr, 3, H, W], scenes_u8 uint8 [Fr, H, W, 3] CUDA; rois_host numpy int32 [B, 4]; objs_host numpy int32 [B, 12] and tables =
    (objs, bounds, kk8) its CUDA copy with Pillow's tables (derender3d.scene.crop_tables); items_host numpy int32 [B, 12] and
    items its CUDA copy (derender3d.train_items.item_table); nearer uint8 [total, 3] CUDA, the items' nearer codes (may be
    empty).  Returns (images [B,3,S_i,S_i], masks [B,1,S_m,S_m], ignores [B,1,S_m,S_m]).  Nothing is copied to the host."""
    frames_u8 = want(frames_u8, torch.uint8, 'frames_u8')
    scenes_u8 = want(scenes_u8, torch.uint8, 'scenes_u8')
    if frames_u8.dim() != 4 or frames_u8.shape[1] != 3 or frames_u8.shape[0] < 1:
        raise ValueError('frames_u8 must be uint8 [Fr, 3, H, W], got %s' % (tuple(frames_u8.shape),))
    Fr, _, H, W = frames_u8.shape
    if tuple(scenes_u8.shape) != (Fr, H, W, 3):
        raise ValueError('scenes_u8 must be uint8 [%d, %d, %d, 3], got %s' % (Fr, H, W, tuple(scenes_u8.shape)))
    rois_host = np.ascontiguousarray(rois_host, dtype=np.int32)
    objs_host = np.ascontiguousarray(objs_host, dtype=np.int32)
    items_host = np.ascontiguousarray(items_host, dtype=np.int32)
    if rois_host.ndim != 2 or rois_host.shape[1] != 4 or rois_host.shape[0] < 1:
        raise ValueError('rois must be [B, 4] with B >= 1, got %s' % (rois_host.shape,))
    B = rois_host.shape[0]
    if objs_host.shape != (B, 12) or items_host.shape != (B, TRAIN_ITEM_INTS):
        raise ValueError('objs_host must be [%d, 12] and items_host [%d, %d], got %s, %s'
                         % (B, B, TRAIN_ITEM_INTS, objs_host.shape, items_host.shape))
    objs, bounds, kk8 = (want(t, torch.int32, name) for t, name in zip(tables, ('objs', 'bounds', 'kk8')))
    items = want(items, torch.int32, 'items')
    nearer = want(nearer, torch.uint8, 'nearer')
    if tuple(objs.shape) != (B, 12) or tuple(items.shape) != (B, TRAIN_ITEM_INTS):
        raise ValueError('objs must be [%d, 12] and items [%d, %d], got %s, %s'
                         % (B, B, TRAIN_ITEM_INTS, tuple(objs.shape), tuple(items.shape)))
    if bounds.dim() != 2 or bounds.shape[1] != 2 or kk8.dim() != 1:
        raise ValueError('bounds must be [M, 2] and kk8 [K], got %s, %s' % (tuple(bounds.shape), tuple(kk8.shape)))
    if nearer.dim() != 2 or nearer.shape[1] != 3:
        raise ValueError('nearer must be uint8 [total, 3], got %s' % (tuple(nearer.shape),))
    dev = frames_u8.device
    _on_device_of('frames_u8', dev, (('scenes_u8', scenes_u8), ('objs', objs), ('bounds', bounds), ('kk8', kk8), ('items', items),
                                     ('nearer', nearer)))
    with torch.cuda.device(dev):
        images = torch.empty(B, 3, image_size, image_size, device=dev)
        masks = torch.empty(B, 1, mask_size, mask_size, device=dev)
        ignores = torch.empty(B, 1, mask_size, mask_size, device=dev)
        work = torch.empty(B, dtype=torch.int64, device=dev)
        check(lib().sdn_train_crops(ptr(frames_u8), ptr(scenes_u8), Fr, H, W, rois_host.ctypes.data, objs_host.ctypes.data, ptr(objs),
                                    items_host.ctypes.data, ptr(items), B, ptr(bounds), bounds.shape[0], ptr(kk8), kk8.shape[0],
                                    ptr(nearer) if nearer.shape[0] else None, nearer.shape[0], image_size, mask_size,
                                    float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]), float(std[2]),
                                    ptr(work), ptr(images), ptr(masks), ptr(ignores), stream()))
    return images, masks, ignores


TRAIN_ID_ITEM_INTS, TRAIN_ID_COLS = 8, 8   # one row of sdn_train_id_stats' item table, one row of its output
TRAIN_MIXED_ITEM_INTS = 32                 # one row of sdn_train_crops_mixed's item table


def train_id_stats(items, max_pixels):
    """The statistics of B (frame, id) items over several frames in one call (sdn_train_id_stats; derender3d/datasets.py:938-955
    per object on the host): items int32 [B, 8] CUDA rows (address of the int32 [H, W] id map as two ints, address of the int32
    [H, W] disparity map or 0, H, W, id, unused) -- derender3d.train_items.id_item_table --, max_pixels the largest H W among
    them.  Returns table int32 [B, 8] CUDA rows (area, y0, x0, y1, x1, n, lo, hi) as scene_id_stats' rows; an absent id has
    area 0 and the roi (INT_MAX, INT_MAX, 0, 0).  The maps the rows name must stay alive until the call has run.  Nothing is
    copied to the host."""
    items = want(items, torch.int32, 'items')
    if items.dim() != 2 or items.shape[1] != TRAIN_ID_ITEM_INTS or items.shape[0] < 1:
        raise ValueError('items must be int32 [B, %d] with B >= 1, got %s' % (TRAIN_ID_ITEM_INTS, tuple(items.shape)))
    B = items.shape[0]
    dev = items.device
    with torch.cuda.device(dev):
        table = torch.empty(B, TRAIN_ID_COLS, dtype=torch.int32, device=dev)
        workspace = train_id_workspace(B, dev)
        check(lib().sdn_train_id_stats(ptr(items), B, int(max_pixels), ptr(table), ptr(workspace), stream()))
    return table


def train_crops_mixed(rois_host, objs_host, items_host, tables, items, nearer, image_size=224, mask_size=256, maps=True):
    """The crops of B training items whose frames, normalisations, mask and ignore sources differ per item
    (sdn_train_crops_mixed; derender3d/datasets.py:141-172 as the KITTI, Cityscapes and VKitti classes call them), bit for bit
    with sdn_train_crops.  rois_host numpy int32 [B, 4]; objs_host numpy int32 [B, 12] and tables = (objs, bounds, kk8) its CUDA
    copy with Pillow's tables, made with each item's own frame size (derender3d.scene.crop_tables with one H and W per roi); items_host numpy
    int32 [B, 32] and items its CUDA copy (derender3d.train_items.mixed_item_table; include/sdn_hip.h lists the row); nearer
    uint8 [total, 3] CUDA (may be empty).  maps False: a batch without masks and ignores.  The tensors the rows name must stay
    alive until the call has run.  Returns (images [B,3,S_i,S_i], masks [B,1,S_m,S_m] | None, ignores | None)."""
    rois_host = np.ascontiguousarray(rois_host, dtype=np.int32)
    objs_host = np.ascontiguousarray(objs_host, dtype=np.int32)
    items_host = np.ascontiguousarray(items_host, dtype=np.int32)
    if rois_host.ndim != 2 or rois_host.shape[1] != 4 or rois_host.shape[0] < 1:
        raise ValueError('rois must be [B, 4] with B >= 1, got %s' % (rois_host.shape,))
    B = rois_host.shape[0]
    if objs_host.shape != (B, 12) or items_host.shape != (B, TRAIN_MIXED_ITEM_INTS):
        raise ValueError('objs_host must be [%d, 12] and items_host [%d, %d], got %s, %s'
                         % (B, B, TRAIN_MIXED_ITEM_INTS, objs_host.shape, items_host.shape))
    objs, bounds, kk8 = (want(t, torch.int32, name) for t, name in zip(tables, ('objs', 'bounds', 'kk8')))
    items = want(items, torch.int32, 'items')
    nearer = want(nearer, torch.uint8, 'nearer')
    if tuple(objs.shape) != (B, 12) or tuple(items.shape) != (B, TRAIN_MIXED_ITEM_INTS):
        raise ValueError('objs must be [%d, 12] and items [%d, %d], got %s, %s'
                         % (B, B, TRAIN_MIXED_ITEM_INTS, tuple(objs.shape), tuple(items.shape)))
    if bounds.dim() != 2 or bounds.shape[1] != 2 or kk8.dim() != 1:
        raise ValueError('bounds must be [M, 2] and kk8 [K], got %s, %s' % (tuple(bounds.shape), tuple(kk8.shape)))
    if nearer.dim() != 2 or nearer.shape[1] != 3:
        raise ValueError('nearer must be uint8 [total, 3], got %s' % (tuple(nearer.shape),))
    dev = items.device
    _on_device_of('items', dev, (('objs', objs), ('bounds', bounds), ('kk8', kk8), ('nearer', nearer)))
    with torch.cuda.device(dev):
        images = torch.empty(B, 3, image_size, image_size, device=dev)
        masks = torch.empty(B, 1, mask_size, mask_size, device=dev) if maps else None
        ignores = torch.empty(B, 1, mask_size, mask_size, device=dev) if maps else None
        work = torch.empty(B, dtype=torch.int64, device=dev)
        check(lib().sdn_train_crops_mixed(rois_host.ctypes.data, objs_host.ctypes.data, ptr(objs), items_host.ctypes.data, ptr(items),
                                          B, ptr(bounds), bounds.shape[0], ptr(kk8), kk8.shape[0],
                                          ptr(nearer) if nearer.shape[0] else None, nearer.shape[0], image_size, mask_size,
                                          ptr(work), ptr(images), ptr(masks), ptr(ignores), stream()))
    return images, masks, ignores


SEGM_MAX_SCALES, SEGM_MAX_CLASSES, SEGM_MAX_COLORS, SEGM_UNKNOWN = 8, 32, 1024, -32768   # csrc/segm_tail_check.h


def segm_scale_table(scores):
    """The HOST table of sdn_segm_fuse for a list of fp32 [B, C, h_s, w_s] CUDA maps: numpy int32 [S, 4] rows (address as two
    ints, low word first; h_s; w_s)."""
    rows = np.zeros((len(scores), 2), dtype=np.uint64)
    for s, t in enumerate(scores):
        rows[s, 0] = t.data_ptr()
        rows[s, 1] = (int(t.shape[3]) << 32) | int(t.shape[2])
    return rows.view(np.int32).reshape(len(scores), 4)


def segm_fuse(scores, H, W, probs=False):
    """Multi-scale fusion of class scores to a label map (sdn_segm_fuse; semantic/vkitti_test.py:58-72 with models.py:401-402:
    upsample, softmax, average over the scales on the device, torch.max on the host).  scores: a list of S fp32 [B, C, h_s, w_s]
    CUDA tensors, one per test scale, the decoder's scores BEFORE upsample and softmax.  Returns labels uint8 [B, 1, H, W] --
    what textural.edit.EditSession and textural.data.assemble take -- and, with probs, also the averaged probabilities fp32
    [B, C, H, W].  Nothing is copied to the host."""
    scores = [want(t, torch.float32, 'scores[%d]' % s) for s, t in enumerate(scores)]
    if not scores:
        raise ValueError('scores is empty')
    if any(t.dim() != 4 for t in scores):
        raise ValueError('every score map must be [B, C, h, w], got %s' % ([tuple(t.shape) for t in scores],))
    B, C = scores[0].shape[:2]
    dev = scores[0].device
    for s, t in enumerate(scores):
        if t.shape[0] != B or t.shape[1] != C or t.device != dev:
            raise ValueError('scores[%d] is %s on %s, scores[0] %s on %s' % (s, tuple(t.shape), t.device, tuple(scores[0].shape), dev))
    table = segm_scale_table(scores)
    with torch.cuda.device(dev):
        labels = torch.empty(B, 1, H, W, dtype=torch.uint8, device=dev)
        pred = torch.empty(B, C, H, W, device=dev) if probs else None
        check(lib().sdn_segm_fuse(table.ctypes.data, len(scores), B, C, int(H), int(W), ptr(labels), ptr(pred), stream()))
    return (labels, pred) if probs else labels


def segm_labels_from_colors(scene_u8, table_host, table):
    """Ground-truth labels of a semantic colour image (sdn_segm_labels_from_colors; semantic/vkitti_dataset.py:206-209, 238: a
    dictionary look-up per pixel through np.apply_along_axis).  scene_u8 uint8 [B, H, W, 3] CUDA; table_host numpy int32 [2 K]
    (K ascending codes r | g << 8 | b << 16, then their labels) and table its CUDA copy -- semantic.segm_tail.color_table.
    Returns (labels_gt int16 [B, H, W] = label - 1, unknown int32 [B]: the pixels per frame whose colour is not in the table,
    which got -32768).  Nothing is copied to the host."""
    scene_u8 = want(scene_u8, torch.uint8, 'scene_u8')
    table = want(table, torch.int32, 'table')
    table_host = np.ascontiguousarray(table_host, dtype=np.int32)
    if scene_u8.dim() != 4 or scene_u8.shape[3] != 3:
        raise ValueError('scene_u8 must be uint8 [B, H, W, 3], got %s' % (tuple(scene_u8.shape),))
    if table_host.ndim != 1 or table_host.size % 2 or table_host.size < 2 or tuple(table.shape) != table_host.shape:
        raise ValueError('table_host and table must be int32 [2 K] with K >= 1, got %s, %s' % (table_host.shape, tuple(table.shape)))
    _on_device_of('scene_u8', scene_u8.device, (('table', table),))
    B, H, W = scene_u8.shape[:3]
    dev = scene_u8.device
    with torch.cuda.device(dev):
        labels_gt = torch.empty(B, H, W, dtype=torch.int16, device=dev)
        unknown = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib().sdn_segm_labels_from_colors(ptr(scene_u8), B, H, W, table_host.ctypes.data, ptr(table), table_host.size // 2,
                                                ptr(labels_gt), ptr(unknown), stream()))
    return labels_gt, unknown


def segm_confusion(labels, labels_gt, num_class):
    """The integers of accuracy() and intersectionAndUnion() (sdn_segm_confusion; semantic/utils.py:101-129 in numpy per
    frame).  labels uint8 [B, 1, H, W] CUDA, labels_gt int16 [B, H, W] CUDA.  Returns counts int64 [B, 3 C + 3]:
    area_intersection[C], area_pred[C], area_lab[C], acc_sum, valid_sum, the number of unknown-colour pixels.  Nothing is
    copied to the host."""
    labels = want(labels, torch.uint8, 'labels')
    labels_gt = want(labels_gt, torch.int16, 'labels_gt')
    if labels.dim() != 4 or labels.shape[1] != 1:
        raise ValueError('labels must be uint8 [B, 1, H, W], got %s' % (tuple(labels.shape),))
    B, _, H, W = labels.shape
    if tuple(labels_gt.shape) != (B, H, W):
        raise ValueError('labels_gt must be int16 [%d, %d, %d], got %s' % (B, H, W, tuple(labels_gt.shape)))
    _on_device_of('labels', labels.device, (('labels_gt', labels_gt),))
    C = int(num_class)
    dev = labels.device
    with torch.cuda.device(dev):
        counts = torch.empty(B, 3 * C + 3, dtype=torch.int64, device=dev)
        check(lib().sdn_segm_confusion(ptr(labels), ptr(labels_gt), B, H, W, C, ptr(counts), stream()))
    return counts


SEGM_TRAIN_ITEM_INTS, SEGM_TRAIN_STAT_PIXELS = 20, 2048   # csrc/segm_train_check.h: SGT_ITEM_INTS, SGT_STAT_PIXELS


def segm_train_batch(frames_u8, scenes_u8, tables_host, Hb, Wb, rate, mean, std):
    """One training batch of the semantic branch (sdn_segm_train_batch; semantic/vkitti_dataset.py:111-159 per item on the
    host): colour jitter, flip, Pillow's BILINEAR resize, BGR + Normalize and the zero padding for the images, the two NEAREST
    resizes composed into one gather for the labels.  frames_u8, scenes_u8 uint8 [B, H, W, 3] CUDA; tables_host numpy int32 [n]:
    the B item rows of 20 ints and every table they name (semantic.train_items.table_buffer; include/sdn_hip.h lists the row).
    It is uploaded here, in one copy.  Returns (img_data fp32 [B, 3, Hb, Wb], seg_label int64 [B, Hb // rate, Wb // rate],
    unknown int32 [B]).  Nothing is copied to the host."""
    frames_u8 = want(frames_u8, torch.uint8, 'frames_u8')
    scenes_u8 = want(scenes_u8, torch.uint8, 'scenes_u8')
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        raise ValueError('frames_u8 must be uint8 [B, H, W, 3], got %s' % (tuple(frames_u8.shape),))
    B, H, W, _ = frames_u8.shape
    if tuple(scenes_u8.shape) != (B, H, W, 3):
        raise ValueError('scenes_u8 must be uint8 [%d, %d, %d, 3], got %s' % (B, H, W, tuple(scenes_u8.shape)))
    dev = frames_u8.device
    _on_device_of('frames_u8', dev, (('scenes_u8', scenes_u8),))
    tables_host = np.ascontiguousarray(tables_host, dtype=np.int32)
    if tables_host.ndim != 1 or tables_host.size < B * SEGM_TRAIN_ITEM_INTS:
        raise ValueError('tables_host must be int32 [n] with n >= %d, got %s' % (B * SEGM_TRAIN_ITEM_INTS, tables_host.shape))
    Hb, Wb, rate = int(Hb), int(Wb), int(rate)
    if Hb < 1 or Wb < 1 or rate < 1 or rate > Hb or rate > Wb:
        raise ValueError('bad batch sizes: %d x %d at label rate %d' % (Hb, Wb, rate))
    with torch.cuda.device(dev):
        tables = torch.from_numpy(tables_host).to(dev)   # the one upload
        work = torch.empty(B * (-(-H * W // SEGM_TRAIN_STAT_PIXELS)), dtype=torch.int32, device=dev)
        img = torch.empty(B, 3, Hb, Wb, device=dev)
        lab = torch.empty(B, Hb // rate, Wb // rate, dtype=torch.int64, device=dev)
        unknown = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib().sdn_segm_train_batch(ptr(frames_u8), ptr(scenes_u8), B, H, W, tables_host.ctypes.data, ptr(tables), tables_host.size,
                                         Hb, Wb, rate, float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]),
                                         float(std[2]), ptr(work), work.numel(), ptr(img), ptr(lab), ptr(unknown), stream()))
    return img, lab, unknown


SEGM_LOSS_PIXELS, SEGM_LOSS_PART_BYTES = 256, 32   # csrc/segm_loss_check.h: SGL_PIXELS, SGL_PART_BYTES


class SegmLossFn(torch.autograd.Function):
    """The training branch of SegmentationModule.forward after the network call (semantic/models.py:39-45 with pixel_acc,
    :15-21, the decoders' log_softmax, :279-280, 412-413, and nn.NLLLoss(ignore_index=-1), vkitti_train.py:133) on the class
    SCORES of both decoder heads -- sdn_segm_loss_fwd / _bwd (include/sdn_hip.h), forward in two launches, backward in one.
    Returns (out fp32 [4]: loss, acc, loss_main, loss_deepsup; counts int64 [3]: acc_sum, pixel_sum, bad).  `segm_loss` below
    checks types and shapes; a CPU tensor raises NotImplementedError here."""

    @staticmethod
    def forward(ctx, scores, scores_deepsup, seg_label, deep_sup_scale):
        s0, s1, lab = _f32(scores, 'scores'), _f32(scores_deepsup, 'scores_deepsup'), want(seg_label, torch.int64, 'seg_label')
        B, C, h, w = s0.shape
        scale = float(deep_sup_scale) if s1 is not None else 0.0
        dev = s0.device
        with torch.cuda.device(dev):
            scratch = torch.empty(B * (-(-h * w // SEGM_LOSS_PIXELS)) * SEGM_LOSS_PART_BYTES, dtype=torch.uint8, device=dev)
            lse = torch.empty(2, B, h, w, dtype=torch.float32, device=dev)
            out = torch.empty(4, dtype=torch.float32, device=dev)
            counts = torch.empty(3, dtype=torch.int64, device=dev)
            check(lib().sdn_segm_loss_fwd(ptr(s0), ptr(s1), ptr(lab), B, C, h, w, scale, ptr(scratch), scratch.numel(), ptr(lse), ptr(out),
                                          ptr(counts), stream()))
        ctx.save_for_backward(s0, s1, lab, lse, counts)
        ctx.scale = scale
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_counts):
        s0, s1, lab, lse, counts = ctx.saved_tensors
        need0 = ctx.needs_input_grad[0]
        need1 = s1 is not None and ctx.needs_input_grad[1]
        if not (need0 or need1):
            return None, None, None, None
        B, C, h, w = s0.shape
        with torch.cuda.device(s0.device):
            go = g_out.to(torch.float32).contiguous()
            g0 = torch.empty_like(s0) if need0 else None
            g1 = torch.empty_like(s1) if need1 else None
            check(lib().sdn_segm_loss_bwd(ptr(s0), ptr(s1), ptr(lab), B, C, h, w, ctx.scale, ptr(lse), ptr(counts), ptr(go), ptr(g0),
                                          ptr(g1), stream()))
        return g0, g1, None, None


def segm_loss(scores, scores_deepsup, seg_label, deep_sup_scale):
    """(out fp32 [4] = loss, acc, loss_main, loss_deepsup; counts int64 [3] = acc_sum, pixel_sum, bad) of the semantic training
    step for the decoder's class scores fp32 [B, C, h, w] (scores_deepsup: the same shape, or None), seg_label int64 [B, h, w]
    (-1: ignored; any other label outside [0, C) is ignored too and counted in bad) and the Python float deep_sup_scale.
    Differentiable in both score tensors; counts is not.  Nothing is copied to the host.  A wrong type or dtype raises
    TypeError, a wrong shape ValueError, a CPU tensor NotImplementedError."""
    for t, name, dtype in ((scores, 'scores', torch.float32), (scores_deepsup, 'scores_deepsup', torch.float32),
                           (seg_label, 'seg_label', torch.int64)):
        if t is None and name == 'scores_deepsup':
            continue
        _is_tensor(t, name)
        if t.dtype != dtype:
            raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if scores.dim() != 4:
        raise ValueError('scores must be fp32 [B, C, h, w], got %s' % (tuple(scores.shape),))
    B, C, h, w = scores.shape
    if C < 1 or C > SEGM_MAX_CLASSES or B < 1 or h < 1 or w < 1:
        raise ValueError('scores is %s; 1 to %d classes and no empty axis are supported' % (tuple(scores.shape), SEGM_MAX_CLASSES))
    if scores_deepsup is not None and (scores_deepsup.shape != scores.shape or scores_deepsup.device != scores.device):
        raise ValueError('scores_deepsup is %s on %s, scores %s on %s' % (tuple(scores_deepsup.shape), scores_deepsup.device,
                                                                        tuple(scores.shape), scores.device))
    if tuple(seg_label.shape) != (B, h, w) or seg_label.device != scores.device:
        raise ValueError('seg_label must be int64 [%d, %d, %d] on %s, got %s on %s' % (B, h, w, scores.device, tuple(seg_label.shape),
                                                                                     seg_label.device))
    return SegmLossFn.apply(scores, scores_deepsup, seg_label, 0.0 if deep_sup_scale is None else deep_sup_scale)


MRCNN_LOSS_CHUNK, MRCNN_MAX_CLASSES, MRCNN_MAX_ANCHORS = 1024, 128, 1 << 24   # csrc/mrcnn_loss_check.h: MRL_CHUNK, MRL_MAX_CLASSES, MRL_MAX_ANCHORS
_MRCNN_INTS = (torch.int32, torch.int64)


def mrcnn_loss_bytes(A, R):
    """(bytes of `workspace`, bytes of `saved`) of sdn_mrcnn_loss_fwd / _bwd, asked of the library"""
    return size_query(lib().sdn_mrcnn_loss_workspace_bytes, (int(A), int(R)), 2)


class MrcnnLossFn(torch.autograd.Function):
    """compute_losses of the reference's Mask R-CNN (geometric/maskrcnn/model.py:1004-1147) and the sum of :1955 --
    sdn_mrcnn_loss_fwd / _bwd (include/sdn_hip.h), forward in three launches, backward in one.  Returns (out fp32 [6]: the five
    losses and their sum; counts int64 [4]: n_rpn_valid, n_rpn_pos, n_roi_pos, bad).  The five head arguments are None for R = 0.
    `mrcnn_loss` below checks types and shapes; a CPU tensor raises NotImplementedError here."""

    @staticmethod
    def forward(ctx, rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas,
                mrcnn_bbox, target_mask, mrcnn_mask):
        match = want(rpn_match, rpn_match.dtype, 'rpn_match')
        tb, xl, xb = _f32(rpn_bbox, 'rpn_bbox'), _f32(rpn_class_logits, 'rpn_class_logits'), _f32(rpn_pred_bbox, 'rpn_pred_bbox')
        ids = want(target_class_ids, target_class_ids.dtype, 'target_class_ids') if target_class_ids is not None else None
        hl, hd, hb = _f32(mrcnn_class_logits, 'mrcnn_class_logits'), _f32(target_deltas, 'target_deltas'), _f32(mrcnn_bbox, 'mrcnn_bbox')
        tm, hm = _f32(target_mask, 'target_mask'), _f32(mrcnn_mask, 'mrcnn_mask')
        batch, A, T = xl.shape[0], xl.shape[1], tb.shape[1]
        R, (C, h, w) = (0, (0, 0, 0)) if ids is None else (hm.shape[0], hm.shape[1:])
        sizes = (batch, A, T, R, C, h, w)
        flags = (int(match.dtype == torch.int64), int(ids is not None and ids.dtype == torch.int64))
        dev = xl.device
        with torch.cuda.device(dev):
            wbytes, sbytes = mrcnn_loss_bytes(A, R)
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            saved = torch.empty(sbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(6, dtype=torch.float32, device=dev)
            counts = torch.empty(4, dtype=torch.int64, device=dev)
            check(lib().sdn_mrcnn_loss_fwd(ptr(match), flags[0], ptr(tb), ptr(xl), ptr(xb), batch, A, T, ptr(ids), flags[1], ptr(hl), ptr(hd),
                                           ptr(hb), ptr(tm), ptr(hm), R, C, h, w, ptr(work), wbytes, ptr(saved), sbytes, ptr(out),
                                           ptr(counts), stream()))
        ctx.save_for_backward(match, tb, xl, xb, ids, hl, hd, hb, tm, hm, saved)
        ctx.sizes, ctx.flags = sizes, flags
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_counts):
        match, tb, xl, xb, ids, hl, hd, hb, tm, hm, saved = ctx.saved_tensors
        batch, A, T, R, C, h, w = ctx.sizes
        need = [ctx.needs_input_grad[i] and t is not None for i, t in ((2, xl), (3, xb), (5, hl), (7, hb), (9, hm))]
        grads = [None] * 10
        if not any(need):
            return tuple(grads)
        with torch.cuda.device(xl.device):
            go = g_out.to(torch.float32).contiguous()
            gs = [torch.empty_like(t) if n else None for n, t in zip(need, (xl, xb, hl, hb, hm))]
            check(lib().sdn_mrcnn_loss_bwd(ptr(match), ctx.flags[0], ptr(tb), ptr(xl), ptr(xb), batch, A, T, ptr(ids), ctx.flags[1], ptr(hl),
                                           ptr(hd), ptr(hb), ptr(tm), ptr(hm), R, C, h, w, ptr(saved), saved.numel(), ptr(go), ptr(gs[0]),
                                           ptr(gs[1]), ptr(gs[2]), ptr(gs[3]), ptr(gs[4]), stream()))
        for i, g in zip((2, 3, 5, 7, 9), gs):
            grads[i] = g
        return tuple(grads)


def mrcnn_loss(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas, mrcnn_bbox,
               target_mask, mrcnn_mask):
    """(out fp32 [6] = rpn_class_loss, rpn_bbox_loss, mrcnn_class_loss, mrcnn_bbox_loss, mrcnn_mask_loss and their sum; counts
    int64 [4] = n_rpn_valid, n_rpn_pos, n_roi_pos, bad) of a Mask R-CNN training step, the arguments of the reference's
    compute_losses (model.py:1139): rpn_match int32 / int64 [1, A, 1], rpn_bbox fp32 [1, T, 4], rpn_class_logits fp32 [1, A, 2],
    rpn_pred_bbox fp32 [1, A, 4], target_class_ids int32 / int64 [R], mrcnn_class_logits fp32 [R, C], target_deltas fp32 [R, 4],
    mrcnn_bbox fp32 [R, C, 4], target_mask fp32 [R, h, w], mrcnn_mask fp32 [R, C, h, w].  An empty target_class_ids means R = 0: the
    other head tensors are not looked at.  Differentiable in the five predictions; the targets get no gradient and counts is not
    differentiable.  Nothing is copied to the host.  A wrong type or dtype raises TypeError, a wrong shape ValueError, a CPU tensor
    NotImplementedError."""
    named = (('rpn_match', rpn_match, _MRCNN_INTS), ('rpn_bbox', rpn_bbox, (torch.float32,)),
             ('rpn_class_logits', rpn_class_logits, (torch.float32,)), ('rpn_pred_bbox', rpn_pred_bbox, (torch.float32,)),
             ('target_class_ids', target_class_ids, _MRCNN_INTS), ('mrcnn_class_logits', mrcnn_class_logits, (torch.float32,)),
             ('target_deltas', target_deltas, (torch.float32,)), ('mrcnn_bbox', mrcnn_bbox, (torch.float32,)),
             ('target_mask', target_mask, (torch.float32,)), ('mrcnn_mask', mrcnn_mask, (torch.float32,)))
    _are_tensors([(name, t) for name, t, _ in named])
    R = target_class_ids.numel()
    for name, t, dtypes in (named if R else named[:4]):
        if t.dtype not in dtypes:
            raise TypeError('%s must be %s, got %s' % (name, ' or '.join(str(d) for d in dtypes), t.dtype))
        _on_device_of('rpn_class_logits', rpn_class_logits.device, ((name, t),))
    if rpn_class_logits.dim() != 3 or rpn_class_logits.shape[2] != 2 or rpn_class_logits.shape[1] < 1:
        raise ValueError('rpn_class_logits must be fp32 [1, A, 2], got %s' % (tuple(rpn_class_logits.shape),))
    batch, A = rpn_class_logits.shape[:2]
    if batch != 1:
        raise ValueError('the RPN tensors have batch %d; only one image per step is supported: the reference trims the targets with '
                         'target_bbox[0, :n] (geometric/maskrcnn/model.py:1053), which has no meaning for more' % batch)
    if A > MRCNN_MAX_ANCHORS:
        raise ValueError('%d anchors; at most %d are supported' % (A, MRCNN_MAX_ANCHORS))
    if tuple(rpn_match.shape) != (1, A, 1):
        raise ValueError('rpn_match must be [1, %d, 1], got %s' % (A, tuple(rpn_match.shape)))
    if tuple(rpn_pred_bbox.shape) != (1, A, 4):
        raise ValueError('rpn_pred_bbox must be fp32 [1, %d, 4], got %s' % (A, tuple(rpn_pred_bbox.shape)))
    if rpn_bbox.dim() != 3 or rpn_bbox.shape[0] != 1 or rpn_bbox.shape[1] < 1 or rpn_bbox.shape[2] != 4:
        raise ValueError('rpn_bbox must be fp32 [1, T, 4], got %s' % (tuple(rpn_bbox.shape),))
    if R == 0:
        return MrcnnLossFn.apply(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, None, None, None, None, None, None)
    if target_class_ids.dim() != 1:
        raise ValueError('target_class_ids must be [R], got %s' % (tuple(target_class_ids.shape),))
    if mrcnn_mask.dim() != 4 or mrcnn_mask.shape[0] != R or min(mrcnn_mask.shape) < 1:
        raise ValueError('mrcnn_mask must be fp32 [%d, C, h, w], got %s' % (R, tuple(mrcnn_mask.shape)))
    _, C, h, w = mrcnn_mask.shape
    if C < 2 or C > MRCNN_MAX_CLASSES:
        raise ValueError('mrcnn_mask is %s; 2 to %d classes are supported' % (tuple(mrcnn_mask.shape), MRCNN_MAX_CLASSES))
    for name, t, shape in (('mrcnn_class_logits', mrcnn_class_logits, (R, C)), ('target_deltas', target_deltas, (R, 4)),
                           ('mrcnn_bbox', mrcnn_bbox, (R, C, 4)), ('target_mask', target_mask, (R, h, w))):
        if tuple(t.shape) != shape:
            raise ValueError('%s must be fp32 %s, got %s' % (name, list(shape), tuple(t.shape)))
    return MrcnnLossFn.apply(rpn_match, rpn_bbox, rpn_class_logits, rpn_pred_bbox, target_class_ids, mrcnn_class_logits, target_deltas,
                             mrcnn_bbox, target_mask, mrcnn_mask)


PYRAMID_LEVELS, PYRAMID_MAX_POOL, PYRAMID_CHANNELS = 4, 32, 64   # csrc/pyramid_roi_align_check.h: PRA_LEVELS, PRA_MAX_POOL, PRA_CHANNELS


def pyramid_grad_floats(C, H, W):
    """(float offsets of the four maps' gradients, floats of the one buffer that holds them) of sdn_pyramid_roi_align_bwd, asked of
    the library"""
    offsets, total = (ctypes.c_size_t * PYRAMID_LEVELS)(), ctypes.c_size_t(0)
    four = lambda values: (ctypes.c_int * PYRAMID_LEVELS)(*[int(v) for v in values])   # noqa: E731  (the library reads four of each)
    check(lib().sdn_pyramid_roi_align_grad_floats(int(C), four(H), four(W), offsets, ctypes.byref(total)))
    return list(offsets), total.value


def pyramid_backward_path():
    """'ordered' or 'atomic': the backward a pyramid_roi_align gradient takes if it runs now.  'ordered' under
    torch.use_deterministic_algorithms(True) or SDN_DETERMINISTIC=1 (sdn_hip.deterministic): sdn_pyramid_roi_align_bwd_ordered, a
    gather per destination in a fixed order, the same bits every run.  'atomic' otherwise: sdn_pyramid_roi_align_bwd."""
    return 'ordered' if deterministic() else 'atomic'


def pyramid_ordered_workspace_bytes(R):
    """bytes of the workspace of sdn_pyramid_roi_align_bwd_ordered for R boxes, asked of the library"""
    return size_query(lib().sdn_pyramid_roi_align_bwd_ordered_workspace_bytes, (int(R),))


class PyramidRoiAlignFn(torch.autograd.Function):
    """pyramid_roi_align of the reference's Mask R-CNN (geometric/maskrcnn/model.py:414-502) -- sdn_pyramid_roi_align_fwd / _bwd /
    _bwd_ordered (include/sdn_hip.h), forward in one launch, backward in a zero fill and one scatter launch, or, where
    pyramid_backward_path() says 'ordered' when the backward runs, in a record launch and one gather launch.  Returns (pooled fp32
    [R, C, pool, pool] in box order, levels int32 [R]).  `pyramid_roi_align` below checks types and shapes."""

    @staticmethod
    def forward(ctx, boxes, p2, p3, p4, p5, pool, image_area):
        maps = (p2, p3, p4, p5)
        R, C = boxes.shape[0], p2.shape[0]
        H, W = [m.shape[1] for m in maps], [m.shape[2] for m in maps]
        dev = boxes.device
        with torch.cuda.device(dev):
            pooled = torch.empty(R, C, pool, pool, dtype=torch.float32, device=dev)
            levels = torch.empty(R, dtype=torch.int32, device=dev)
            check(lib().sdn_pyramid_roi_align_fwd(ptr(boxes), R, c_ptrs(maps), c_ints(H), c_ints(W), C, pool, image_area, 0.0, ptr(pooled),
                                                  ptr(levels), stream()))
        ctx.save_for_backward(boxes)
        ctx.sizes = (R, C, H, W, pool, image_area)
        ctx.mark_non_differentiable(levels)
        return pooled, levels

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pooled, _g_levels):
        (boxes,) = ctx.saved_tensors
        R, C, H, W, pool, image_area = ctx.sizes
        if not any(ctx.needs_input_grad[1:5]):
            return (None,) * 7
        with torch.cuda.device(boxes.device):
            g = g_pooled.to(torch.float32).contiguous()
            offsets, total = pyramid_grad_floats(C, H, W)
            buf = torch.empty(total, dtype=torch.float32, device=boxes.device)
            if pyramid_backward_path() == 'ordered':
                nbytes = pyramid_ordered_workspace_bytes(R)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=boxes.device) if nbytes else None   # the caching allocator aligns to 512
                check(lib().sdn_pyramid_roi_align_bwd_ordered(ptr(g), ptr(boxes), R, c_ints(H), c_ints(W), C, pool, image_area, ptr(buf),
                                                              ptr(ws), nbytes, stream()))
            else:
                check(lib().sdn_pyramid_roi_align_bwd(ptr(g), ptr(boxes), R, c_ints(H), c_ints(W), C, pool, image_area, ptr(buf), stream()))
        views = [buf[o:o + C * h * w].view(C, h, w) if need else None for o, h, w, need in zip(offsets, H, W, ctx.needs_input_grad[1:5])]
        return (None,) + tuple(views) + (None, None)


def pyramid_roi_align(boxes, maps, pool, image_area):
    """(pooled fp32 [R, C, pool, pool], levels int32 [R]) of the reference's pyramid_roi_align (model.py:414-502): boxes fp32 [R, 4] =
    (y1, x1, y2, x2) normalised, maps = (P2, P3, P4, P5), each fp32 [C, H_l, W_l], image_area = float(image_shape[0] * image_shape[1]).
    Row r of pooled is box r, sampled with crop_and_resize's arithmetic from level levels[r] (2 .. 5; a box of area <= 0 or with a NaN
    goes to level 2).  Differentiable in the four maps only: the boxes get None (the reference detaches them, :473), levels is not
    differentiable.  The four gradients are views of one buffer; by default they are sums of fp32 atomic adds and so not bit-reproducible from
    run to run.  Under torch.use_deterministic_algorithms(True) or SDN_DETERMINISTIC=1, read when the backward runs
    (pyramid_backward_path()), they are fixed-order fp64 sums of the reference's fp32 terms rounded once: the same bits every run.
    Nothing is copied to the host in either direction.  A wrong type or dtype raises TypeError, a wrong shape or a
    non-contiguous tensor ValueError, a CPU tensor NotImplementedError."""
    maps = tuple(maps)
    if len(maps) != PYRAMID_LEVELS:
        raise ValueError('%d feature maps; the four levels P2 .. P5 are needed' % len(maps))
    named = [('boxes', boxes)] + [('P%d' % (l + 2), m) for l, m in enumerate(maps)]
    for name, t in named:
        if want(t, torch.float32, name) is not t:       # TypeError / NotImplementedError; a copy means it was not contiguous
            raise _not_contiguous(name, t)
        _on_device_of('boxes', boxes.device, ((name, t),))
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError('boxes must be fp32 [R, 4], got %s' % (tuple(boxes.shape),))
    for name, m in named[1:]:
        if m.dim() != 3 or min(m.shape) < 1:
            raise ValueError('%s must be fp32 [C, H, W] with no empty axis, got %s' % (name, tuple(m.shape)))
        if m.shape[0] != maps[0].shape[0]:
            raise ValueError('%s has %d channels, P2 %d' % (name, m.shape[0], maps[0].shape[0]))
    pool = int(pool)
    if pool < 1 or pool > PYRAMID_MAX_POOL:
        raise ValueError('pool %d; 1 to %d are supported' % (pool, PYRAMID_MAX_POOL))
    image_area = float(image_area)
    if not (0.0 < image_area < float('inf')):
        raise ValueError('image_area %r must be finite and positive' % image_area)
    return PyramidRoiAlignFn.apply(boxes.detach(), maps[0], maps[1], maps[2], maps[3], pool, image_area)


PROPOSAL_MAX_PRE_NMS, PROPOSAL_MAX_ANCHORS, PROPOSAL_CHUNK = 8192, 1 << 24, 1024   # csrc/proposal_layer_check.h: PROP_MAX_PRE_NMS, PROP_MAX_ANCHORS, PROP_CHUNK


def proposal_workspace_bytes(A, K, P):
    """bytes of the workspace of sdn_proposal_layer, asked of the library"""
    return size_query(lib().sdn_proposal_layer_workspace_bytes, [int(v) for v in (A, K, P)])


def _proposal_rows(t, name, cols):
    _is_tensor(t, name)
    if t.dim() == 3:
        if t.shape[0] != 1:
            raise ValueError('%s has batch %d; only 1 is supported, as in the reference ("Currently only supports batchsize 1", '
                             'geometric/maskrcnn/model.py:358)' % (name, t.shape[0]))
        rows = t[0]        # a view: nothing is copied, and the caller's tensor keeps its shape
    else:
        rows = t
    if rows.dim() != 2 or rows.shape[1] != cols:
        raise ValueError('%s must be fp32 [A, %d] or [1, A, %d], got %s' % (name, cols, cols, tuple(t.shape)))
    return rows


def proposal_layer(rpn_probs, rpn_bbox, anchors, std_dev, height, width, proposal_count, nms_threshold, pre_nms_limit=6000, strict=True):
    """The reference's proposal_layer (geometric/maskrcnn/model.py:344-407, apply_box_deltas :307-328, clip_boxes :331-341) --
    sdn_proposal_layer (include/sdn_hip.h): rpn_probs fp32 [A, 2] = (bg, fg) or [1, A, 2], rpn_bbox fp32 [A, 4] or [1, A, 4], anchors
    fp32 [A, 4] = (y1, x1, y2, x2) in pixels, std_dev four floats, height and width of the image in pixels, proposal_count P,
    pre_nms_limit 1 .. 8192, K = min(pre_nms_limit, A).  Returns

        order    int32 [K]     the K anchors with the largest fg score, best first, equal scores lower index first
        boxes_px fp32 [K, 4]   those anchors decoded and clipped, in pixels
        keep     int32 [P]     positions in `order` of the boxes the NMS keeps, -1 behind count
        count    int32 [1]
        rois     fp32 [P, 4]   boxes_px[keep] / (height, width, height, width), +0.0 behind count

    strict=True suppresses on IoU > nms_threshold (the reference's CUDA rule), strict=False on >= (its CPU rule).  No result carries a
    gradient: the reference detaches the boxes at the only place that differentiates past them (:473), and detection_target_layer
    takes .data.  Nothing is copied to the host.  A wrong type or dtype raises TypeError, a wrong shape or size or a non-contiguous
    tensor ValueError, a CPU tensor NotImplementedError: there is no torch form."""
    probs = _proposal_rows(rpn_probs, 'rpn_probs', 2)
    deltas = _proposal_rows(rpn_bbox, 'rpn_bbox', 4)
    _is_tensor(anchors, 'anchors')
    if anchors.dim() != 2 or anchors.shape[1] != 4:
        raise ValueError('anchors must be fp32 [A, 4], got %s' % (tuple(anchors.shape),))
    A = anchors.shape[0]
    if A == 0:
        raise ValueError('no anchors: A = 0')
    if A >= PROPOSAL_MAX_ANCHORS:
        raise ValueError('A = %d; fewer than 2^24 anchors are supported' % A)
    if probs.shape[0] != A or deltas.shape[0] != A:
        raise ValueError('rpn_probs has %d rows, rpn_bbox %d, anchors %d' % (probs.shape[0], deltas.shape[0], A))
    P, limit = int(proposal_count), int(pre_nms_limit)
    if limit < 1 or limit > PROPOSAL_MAX_PRE_NMS:
        raise ValueError('pre_nms_limit %d; 1 to %d are supported' % (limit, PROPOSAL_MAX_PRE_NMS))
    if P < 1:
        raise ValueError('proposal_count %d; at least 1' % P)
    if P > limit:
        raise ValueError('proposal_count %d exceeds pre_nms_limit %d' % (P, limit))
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError('image %d x %d' % (height, width))
    std = [float(v) for v in std_dev]
    if len(std) != 4:
        raise ValueError('std_dev must hold four values, got %d' % len(std))
    named = (('rpn_probs', probs), ('rpn_bbox', deltas), ('anchors', anchors))
    _contiguous(named, fp32=('rpn_probs', 'rpn_bbox', 'anchors'))
    _on_one_device(named, 'the proposal layer only runs on the GPU')
    K = min(limit, A)
    dev = probs.device
    with torch.cuda.device(dev):
        order = torch.empty(K, dtype=torch.int32, device=dev)
        boxes_px = torch.empty(K, 4, dtype=torch.float32, device=dev)
        keep = torch.empty(P, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        rois = torch.empty(P, 4, dtype=torch.float32, device=dev)
        ws = torch.empty(proposal_workspace_bytes(A, K, P), dtype=torch.uint8, device=dev)
        check(lib().sdn_proposal_layer(ptr(probs.detach()), ptr(deltas.detach()), ptr(anchors.detach()), A, c_floats(std), height,
                                       width, K, P, float(nms_threshold), int(bool(strict)), ptr(order), ptr(boxes_px), ptr(keep), ptr(count),
                                       ptr(rois), ptr(ws), ws.numel(), stream()))
    return order, boxes_px, keep, count, rois


DETECTION_MAX_ROIS, DETECTION_MAX_INSTANCES = 8192, 8192   # csrc/detection_layer_check.h: DET_MAX_ROIS, DET_MAX_INSTANCES


def detection_workspace_bytes(N, C, D):
    """bytes of the workspace of sdn_detection_layer, asked of the library"""
    return size_query(lib().sdn_detection_layer_workspace_bytes, [int(v) for v in (N, C, D)])


def detection_layer(rois, probs, deltas, window, std_dev, height, width, min_confidence, nms_threshold, max_instances, roi_count=None,
                    strict=True):
    """The reference's refine_detections (geometric/maskrcnn/model.py:744-837, apply_box_deltas :307-328, clip_to_window :731-741) --
    sdn_detection_layer (include/sdn_hip.h): rois fp32 [N, 4] = (y1, x1, y2, x2) normalised, probs fp32 [N, C], deltas fp32 [N, C, 4],
    window four host numbers (y1, x1, y2, x2) in pixels, std_dev four floats, height and width of the image in pixels, min_confidence
    (0 or None: no confidence test, :796), max_instances D; 1 <= N <= 8192, 1 <= D <= 8192.  roi_count: None, or an int32 [1] tensor on
    the device: rows at or behind it are never detections (the count of proposals_padded, handed through unread).  Returns

        class_ids  int32 [N]     first index of every row's maximum (a NaN is the maximum)
        scores     fp32  [N]
        boxes_px   fp32  [N, 4]  decoded, scaled, clipped to the window, rounded half to even
        keep       int32 [D]     row of each detection, best score first, -1 behind count
        count      int32 [1]
        detections fp32  [D, 6]  (y1, x1, y2, x2, class_id, score), +0.0 behind count
        boxes_norm fp32  [D, 4]  detections[:, :4] / (height, width, height, width), +0.0 behind count

    strict=True suppresses on IoU > nms_threshold (the reference's CUDA rule), strict=False on >= (its CPU rule).  Where no row is valid
    count is 0 (the reference raises).  No result carries a gradient.  Nothing is copied to the host.  A wrong type or dtype raises
    TypeError, a wrong shape or size or a non-contiguous tensor ValueError, a CPU tensor NotImplementedError: there is no torch
    form."""
    named = (('rois', rois), ('probs', probs), ('deltas', deltas))
    _are_tensors(named)
    if rois.dim() != 2 or rois.shape[1] != 4:
        raise ValueError('rois must be fp32 [N, 4], got %s' % (tuple(rois.shape),))
    N = rois.shape[0]
    if probs.dim() != 2 or probs.shape[0] != N:
        raise ValueError('probs must be fp32 [N, C] with N = %d, got %s' % (N, tuple(probs.shape)))
    C = probs.shape[1]
    if deltas.dim() != 3 or tuple(deltas.shape) != (N, C, 4):
        raise ValueError('deltas must be fp32 [N, C, 4] = %s, got %s' % ((N, C, 4), tuple(deltas.shape)))
    if N < 1 or N > DETECTION_MAX_ROIS:
        raise ValueError('N = %d; 1 to %d rois are supported' % (N, DETECTION_MAX_ROIS))
    if C < 1:
        raise ValueError('no classes: C = 0')
    D = int(max_instances)
    if D < 1 or D > DETECTION_MAX_INSTANCES:
        raise ValueError('max_instances %d; 1 to %d are supported' % (D, DETECTION_MAX_INSTANCES))
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError('image %d x %d' % (height, width))
    win, std = _four_floats(window, 'window'), _four_floats(std_dev, 'std_dev')
    min_confidence = float(min_confidence) if min_confidence else 0.0
    if roi_count is not None:
        _count_tensor(roi_count, 'roi_count')
        named = named + (('roi_count', roi_count),)
    _contiguous(named[:3], fp32=('rois', 'probs', 'deltas'))
    _on_one_device(named, 'the detection layer only runs on the GPU')
    dev = rois.device
    with torch.cuda.device(dev):
        class_ids = torch.empty(N, dtype=torch.int32, device=dev)
        scores = torch.empty(N, dtype=torch.float32, device=dev)
        boxes_px = torch.empty(N, 4, dtype=torch.float32, device=dev)
        keep = torch.empty(D, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        detections = torch.empty(D, 6, dtype=torch.float32, device=dev)
        boxes_norm = torch.empty(D, 4, dtype=torch.float32, device=dev)
        ws = torch.empty(detection_workspace_bytes(N, C, D), dtype=torch.uint8, device=dev)
        check(lib().sdn_detection_layer(ptr(rois.detach()), ptr(probs.detach()), ptr(deltas.detach()), N, C, c_floats(win),
                                        c_floats(std), height, width, min_confidence, float(nms_threshold), D, int(bool(strict)),
                                        ptr(roi_count) if roi_count is not None else None, ptr(class_ids), ptr(scores), ptr(boxes_px),
                                        ptr(keep), ptr(count), ptr(detections), ptr(boxes_norm), ptr(ws), ws.numel(), stream()))
    return class_ids, scores, boxes_px, keep, count, detections, boxes_norm


# csrc/detection_targets_check.h: DT_MAX_ROIS, DT_MAX_TARGETS, DT_MAX_BOXES, DT_MAX_MASK_SIDE
TARGETS_MAX_ROIS, TARGETS_MAX_PER_IMAGE, TARGETS_MAX_BOXES, TARGETS_MAX_MASK_SIDE = 8192, 8192, 128, 64


def detection_targets_workspace_bytes(N, G, mask_h, mask_w, R, H, W):
    """bytes of the workspace of sdn_detection_targets, asked of the library"""
    return size_query(lib().sdn_detection_targets_workspace_bytes, [int(v) for v in (N, G, mask_h, mask_w, R, H, W)])


def detection_targets(proposals, gt_class_ids, gt_boxes, gt_masks, keys, rois_per_image, positive_ratio, std_dev, mask_shape,
                      use_mini_mask=True, roi_count=None):
    """The reference's detection_target_layer for one image (geometric/maskrcnn/model.py:545-724, bbox_overlaps :508-542,
    utils.box_refinement utils.py:92-113) -- sdn_detection_targets (include/sdn_hip.h): proposals fp32 [N, 4] = (y1, x1, y2, x2)
    normalised, gt_class_ids int32 or int64 [G], gt_boxes fp32 [G, 4] normalised, gt_masks fp32 [G, mh, mw], keys fp32 [2, N] (the
    randomness as data: row 0 orders the positives, row 1 the negatives, smallest first, equal keys lower row first), rois_per_image R,
    positive_ratio in (0, 1], std_dev four positive floats, mask_shape (H, W) each 1 to 64; 1 <= N <= 8192, 1 <= G <= 128,
    1 <= R <= 8192.  roi_count: None, or an int32 [1] tensor on the device: rows at or behind it are never sampled (the count of
    proposals_padded, handed through unread).  Returns, positives first, then negatives:

        rois             fp32  [R, 4]     the sampled proposals, +0.0 behind count
        target_class_ids int32 [R]        the matched box's id, 0 for negatives, -1 behind count
        target_deltas    fp32  [R, 4]     box_refinement / std_dev, +0.0 for negatives and behind count
        target_mask      fp32  [R, H, W]  the matched mask cropped and rounded half to even, +0.0 for negatives and behind count
        rows             int32 [R]        proposal row of every output row, -1 behind count
        assign           int32 [R]        matched box among the G for positives, else -1
        count            int32 [1]
        n_pos            int32 [1]

    use_mini_mask=True crops the roi re-expressed in the matched box's frame (:642-650), False the roi itself from a full-size mask.
    Where there is no positive, or the crowd filter leaves no box (the reference raises), count is 0.  No result carries a gradient.
    Nothing is copied to the host.  A wrong type or dtype raises TypeError, a wrong shape or size or a non-contiguous tensor
    ValueError, a CPU tensor NotImplementedError: there is no torch form."""
    named = (('proposals', proposals), ('gt_class_ids', gt_class_ids), ('gt_boxes', gt_boxes), ('gt_masks', gt_masks), ('keys', keys))
    _are_tensors(named)
    if proposals.dim() != 2 or proposals.shape[1] != 4:
        raise ValueError('proposals must be fp32 [N, 4], got %s' % (tuple(proposals.shape),))
    N = proposals.shape[0]
    if N < 1 or N > TARGETS_MAX_ROIS:
        raise ValueError('N = %d; 1 to %d proposals are supported' % (N, TARGETS_MAX_ROIS))
    if gt_class_ids.dim() != 1:
        raise ValueError('gt_class_ids must be [G], got %s' % (tuple(gt_class_ids.shape),))
    G = gt_class_ids.shape[0]
    if G < 1 or G > TARGETS_MAX_BOXES:
        raise ValueError('G = %d; 1 to %d boxes are supported' % (G, TARGETS_MAX_BOXES))
    if tuple(gt_boxes.shape) != (G, 4):
        raise ValueError('gt_boxes must be fp32 [G, 4] = %s, got %s' % ((G, 4), tuple(gt_boxes.shape)))
    if gt_masks.dim() != 3 or gt_masks.shape[0] != G or gt_masks.shape[1] < 1 or gt_masks.shape[2] < 1:
        raise ValueError('gt_masks must be fp32 [G, mh, mw] with G = %d, got %s' % (G, tuple(gt_masks.shape)))
    if tuple(keys.shape) != (2, N):
        raise ValueError('keys must be fp32 [2, N] = %s, got %s' % ((2, N), tuple(keys.shape)))
    R = int(rois_per_image)
    if R < 1 or R > TARGETS_MAX_PER_IMAGE:
        raise ValueError('rois_per_image %d; 1 to %d are supported' % (R, TARGETS_MAX_PER_IMAGE))
    ratio = float(positive_ratio)
    if not (0.0 < ratio <= 1.0):
        raise ValueError('positive_ratio %r; it must lie in (0, 1]' % (positive_ratio,))
    std = _four_floats(std_dev, 'std_dev')
    if not all(v > 0 for v in std):
        raise ValueError('std_dev must be positive, got %s' % (std,))
    shape = [int(v) for v in mask_shape]
    if len(shape) != 2 or not all(1 <= v <= TARGETS_MAX_MASK_SIDE for v in shape):
        raise ValueError('mask_shape %s; two sides of 1 to %d are supported' % (tuple(shape), TARGETS_MAX_MASK_SIDE))
    H, W = shape
    if gt_class_ids.dtype not in (torch.int32, torch.int64):
        raise TypeError('gt_class_ids must be %s or %s, got %s' % (torch.int32, torch.int64, gt_class_ids.dtype))
    if roi_count is not None:
        _count_tensor(roi_count, 'roi_count')
        named = named + (('roi_count', roi_count),)
    _contiguous(named[:5], fp32=('proposals', 'gt_boxes', 'gt_masks', 'keys'))
    _on_one_device(named, 'the detection targets only run on the GPU')
    dev = proposals.device
    mh, mw = gt_masks.shape[1], gt_masks.shape[2]
    with torch.cuda.device(dev):
        rois = torch.empty(R, 4, dtype=torch.float32, device=dev)
        target_class_ids = torch.empty(R, dtype=torch.int32, device=dev)
        target_deltas = torch.empty(R, 4, dtype=torch.float32, device=dev)
        target_mask = torch.empty(R, H, W, dtype=torch.float32, device=dev)
        rows = torch.empty(R, dtype=torch.int32, device=dev)
        assign = torch.empty(R, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        n_pos = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(detection_targets_workspace_bytes(N, G, mh, mw, R, H, W), dtype=torch.uint8, device=dev)
        check(lib().sdn_detection_targets(ptr(proposals.detach()), ptr(gt_class_ids), ptr(gt_boxes.detach()), ptr(gt_masks.detach()),
                                          ptr(keys.detach()), N, G, mh, mw, int(gt_class_ids.dtype == torch.int64),
                                          ptr(roi_count) if roi_count is not None else None, R, ratio, c_floats(std), H, W,
                                          int(bool(use_mini_mask)), ptr(rois), ptr(target_class_ids), ptr(target_deltas), ptr(target_mask),
                                          ptr(rows), ptr(assign), ptr(count), ptr(n_pos), ptr(ws), ws.numel(), stream()))
    return rois, target_class_ids, target_deltas, target_mask, rows, assign, count, n_pos


# csrc/rpn_targets_check.h: RT_MAX_ANCHORS, RT_MAX_BOXES, RT_MAX_TARGETS
RPN_TARGETS_MAX_ANCHORS, RPN_TARGETS_MAX_BOXES, RPN_TARGETS_MAX_PER_IMAGE = (1 << 24) - 1, 128, 8192


def rpn_targets_workspace_bytes(A, G, T):
    """bytes of the workspace of sdn_rpn_targets, asked of the library"""
    return size_query(lib().sdn_rpn_targets_workspace_bytes, [int(v) for v in (A, G, T)])


def rpn_targets(anchors, gt_class_ids, gt_boxes, keys, anchors_per_image, std_dev, gt_count=None):
    """The reference's build_rpn_targets for one image (geometric/maskrcnn/model.py:1214-1322, compute_overlaps / compute_iou
    utils.py:52-89) -- sdn_rpn_targets (include/sdn_hip.h): anchors fp64 [A, 4] = (y1, x1, y2, x2) in pixels, gt_class_ids int32 or
    int64 [G], gt_boxes fp32 or int32 [G, 4] in pixels (widened exactly to fp64), keys fp32 [2, A] (the randomness as data: of too
    many positives those with the smallest keys[0] stay, of too many negatives those with the smallest keys[1]; equal keys keep the
    lower anchor), anchors_per_image T = RPN_TRAIN_ANCHORS_PER_IMAGE, std_dev = RPN_BBOX_STD_DEV, four positive numbers;
    1 <= A < 2^24, 1 <= G <= 128, 2 <= T <= 8192.  gt_count: None, or an int32 [1] tensor on the device: boxes at or behind it are not
    read.  Returns

        rpn_match int32 [A]     1 positive, -1 negative, 0 neutral
        rpn_bbox  fp32  [T, 4]  row k: the deltas of the k-th positive anchor in anchor order / std_dev, +0.0 behind n_pos
        rows      int32 [T]     the anchor of every row, -1 behind n_pos
        counts    int32 [2]     n_pos, n_neg after sampling

    All arithmetic is fp64, only rpn_bbox is rounded to fp32 at the end.  Where the crowd filter leaves no box (the reference
    raises) there is no positive.  No result carries a gradient.  Nothing is copied to the host.  A wrong type or dtype raises
    TypeError, a wrong shape or size or a non-contiguous tensor ValueError, a CPU tensor NotImplementedError: there is no torch
    form."""
    named = (('anchors', anchors), ('gt_class_ids', gt_class_ids), ('gt_boxes', gt_boxes), ('keys', keys))
    _are_tensors(named)
    if anchors.dim() != 2 or anchors.shape[1] != 4:
        raise ValueError('anchors must be fp64 [A, 4], got %s' % (tuple(anchors.shape),))
    A = anchors.shape[0]
    if A < 1 or A > RPN_TARGETS_MAX_ANCHORS:
        raise ValueError('A = %d; 1 to %d anchors are supported' % (A, RPN_TARGETS_MAX_ANCHORS))
    if gt_class_ids.dim() != 1:
        raise ValueError('gt_class_ids must be [G], got %s' % (tuple(gt_class_ids.shape),))
    G = gt_class_ids.shape[0]
    if G < 1 or G > RPN_TARGETS_MAX_BOXES:
        raise ValueError('G = %d; 1 to %d boxes are supported' % (G, RPN_TARGETS_MAX_BOXES))
    if tuple(gt_boxes.shape) != (G, 4):
        raise ValueError('gt_boxes must be [G, 4] = %s, got %s' % ((G, 4), tuple(gt_boxes.shape)))
    if tuple(keys.shape) != (2, A):
        raise ValueError('keys must be fp32 [2, A] = %s, got %s' % ((2, A), tuple(keys.shape)))
    T = int(anchors_per_image)
    if T < 2 or T > RPN_TARGETS_MAX_PER_IMAGE:
        raise ValueError('anchors_per_image %d; 2 to %d are supported' % (T, RPN_TARGETS_MAX_PER_IMAGE))
    std = _four_floats(std_dev, 'std_dev')
    if not all(v > 0 for v in std):
        raise ValueError('std_dev must be positive, got %s' % (std,))
    if anchors.dtype != torch.float64:
        raise TypeError('anchors must be %s (the reference\'s anchors are float64), got %s' % (torch.float64, anchors.dtype))
    if gt_class_ids.dtype not in (torch.int32, torch.int64):
        raise TypeError('gt_class_ids must be %s or %s, got %s' % (torch.int32, torch.int64, gt_class_ids.dtype))
    if gt_boxes.dtype not in (torch.float32, torch.int32):
        raise TypeError('gt_boxes must be %s or %s, got %s' % (torch.float32, torch.int32, gt_boxes.dtype))
    if keys.dtype != torch.float32:
        raise TypeError('keys must be %s, got %s' % (torch.float32, keys.dtype))
    if gt_count is not None:
        _count_tensor(gt_count, 'gt_count')
        named = named + (('gt_count', gt_count),)
    _contiguous(named[:4])
    _on_one_device(named, 'the RPN targets only run on the GPU')
    dev = anchors.device
    with torch.cuda.device(dev):
        rpn_match = torch.empty(A, dtype=torch.int32, device=dev)
        rpn_bbox = torch.empty(T, 4, dtype=torch.float32, device=dev)
        rows = torch.empty(T, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(rpn_targets_workspace_bytes(A, G, T), dtype=torch.uint8, device=dev)
        check(lib().sdn_rpn_targets(ptr(anchors.detach()), ptr(gt_class_ids), ptr(gt_boxes.detach()), ptr(keys.detach()), A, G,
                                    int(gt_class_ids.dtype == torch.int64), int(gt_boxes.dtype == torch.int32),
                                    ptr(gt_count) if gt_count is not None else None, T, (ctypes.c_double * 4)(*std), ptr(rpn_match),
                                    ptr(rpn_bbox), ptr(rows), ptr(counts), ptr(ws), ws.numel(), stream()))
    return rpn_match, rpn_bbox, rows, counts


# csrc/training_item_check.h: TRI_MAX_DIM, TRI_MAX_MINI, TRI_MAX_BOXES, TRI_PLAN_INTS
TRAINING_ITEM_MAX_DIM, TRAINING_ITEM_MAX_MINI, TRAINING_ITEM_MAX_BOXES, TRAINING_ITEM_PLAN_INTS = 1024, 56, 128, 24


def training_item_workspace_bytes(B, H, W, G):
    """bytes of the workspace of sdn_training_item (G >= 1) and sdn_training_item_image (G = 0), asked of the library"""
    return size_query(lib().sdn_training_item_workspace_bytes, [int(v) for v in (B, H, W, G)])


def _training_item_plan(plan_host, name='plan_host'):
    plan_host = np.ascontiguousarray(plan_host, dtype=np.int32)
    if plan_host.ndim != 1 or plan_host.size < TRAINING_ITEM_PLAN_INTS:
        raise ValueError('%s must be int32 [n] with n >= %d, got %s' % (name, TRAINING_ITEM_PLAN_INTS, plan_host.shape))
    return plan_host


def training_item_image(frames_u8, plan_host):
    """The image half of the Mask R-CNN training item for B frames of one size (utils.resize_image, utils.py:272-320, np.fliplr,
    mold_image, geometric/maskrcnn/model.py:2196-2201) -- sdn_training_item_image (include/sdn_hip.h): frames_u8 uint8 [B, H, W, 3]
    on the device, plan_host numpy int32 [n], the parameter block (maskrcnn.training_item.plan_block; csrc/training_item_check.h
    lists its head).  It is uploaded here, in one copy.  Returns image fp32 [B, 3, M, M].  Nothing is copied to the host.  A wrong
    type or dtype raises TypeError, a wrong shape ValueError, a CPU tensor NotImplementedError: there is no torch form."""
    _are_tensors((('frames_u8', frames_u8),))
    if frames_u8.dtype != torch.uint8:
        raise TypeError('frames_u8 must be %s, got %s' % (torch.uint8, frames_u8.dtype))
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        raise ValueError('frames_u8 must be uint8 [B, H, W, 3], got %s' % (tuple(frames_u8.shape),))
    plan_host = _training_item_plan(plan_host)
    _contiguous((('frames_u8', frames_u8),))
    _on_one_device((('frames_u8', frames_u8),), 'the training item only runs on the GPU')
    B, H, W, _ = frames_u8.shape
    M = int(plan_host[4])
    if M < 1 or M > TRAINING_ITEM_MAX_DIM:
        raise ValueError('IMAGE_MAX_DIM %d; 1 to %d is supported' % (M, TRAINING_ITEM_MAX_DIM))
    dev = frames_u8.device
    with torch.cuda.device(dev):
        plan = torch.from_numpy(plan_host).to(dev)   # the one upload
        ws = torch.empty(training_item_workspace_bytes(B, H, W, 0), dtype=torch.uint8, device=dev)
        image = torch.empty(B, 3, M, M, dtype=torch.float32, device=dev)
        check(lib().sdn_training_item_image(ptr(frames_u8), B, H, W, plan_host.ctypes.data, ptr(plan), plan_host.size, ptr(ws), ws.numel(),
                                            ptr(image), stream()))
    return image


def training_item(frame_u8, inst_map, ids, plan_host, use_mini_mask, mini_shape):
    """The Mask R-CNN training item of one image (load_image_gt, geometric/maskrcnn/model.py:1154-1211, with utils.resize_image,
    resize_mask, extract_bboxes and minimize_mask, utils.py:26-49 and 272-353, mold_image, model.py:2196-2201, and the division of
    :1790-1794) -- sdn_training_item (include/sdn_hip.h): frame_u8 uint8 [H, W, 3]; inst_map int32 [H, W] or uint8 [H, W, 3] (the id
    of a pixel is r << 16 | g << 8 | b); ids int32 [G], 1 <= G <= 128; plan_host numpy int32 [n], the parameter block
    (maskrcnn.training_item.plan_block), uploaded here in one copy; mini_shape (mh, mw), each 1 to 56, read with use_mini_mask.
    Returns

        image         fp32  [3, M, M]
        gt_boxes_int  int32 [G, 4]      (y1, x1, y2, x2) in the padded, mirrored frame; zeros for an instance without a pixel
        gt_boxes      fp32  [G, 4]
        gt_boxes_norm fp32  [G, 4]      gt_boxes / M in fp32
        gt_masks      fp32  [G, mh, mw] with use_mini_mask, [G, M, M] without; 0 / 1
        areas         int32 [G]
        bad           int32 [1]         instances without a pixel

    Nothing is copied to the host.  A wrong type or dtype raises TypeError, a wrong shape or size or a non-contiguous tensor
    ValueError, a CPU tensor NotImplementedError: there is no torch form."""
    named = (('frame_u8', frame_u8), ('inst_map', inst_map), ('ids', ids))
    _are_tensors(named)
    if frame_u8.dtype != torch.uint8:
        raise TypeError('frame_u8 must be %s, got %s' % (torch.uint8, frame_u8.dtype))
    if frame_u8.dim() != 3 or frame_u8.shape[2] != 3:
        raise ValueError('frame_u8 must be uint8 [H, W, 3], got %s' % (tuple(frame_u8.shape),))
    H, W, _ = frame_u8.shape
    if inst_map.dtype == torch.int32:
        if tuple(inst_map.shape) != (H, W):
            raise ValueError('an int32 inst_map must be [H, W] = %s, got %s' % ((H, W), tuple(inst_map.shape)))
    elif inst_map.dtype == torch.uint8:
        if tuple(inst_map.shape) != (H, W, 3):
            raise ValueError('a uint8 inst_map must be [H, W, 3] = %s, got %s' % ((H, W, 3), tuple(inst_map.shape)))
    else:
        raise TypeError('inst_map must be %s [H, W] or %s [H, W, 3], got %s' % (torch.int32, torch.uint8, inst_map.dtype))
    if ids.dtype != torch.int32:
        raise TypeError('ids must be %s, got %s' % (torch.int32, ids.dtype))
    if ids.dim() != 1:
        raise ValueError('ids must be [G], got %s' % (tuple(ids.shape),))
    G = ids.shape[0]
    if G < 1 or G > TRAINING_ITEM_MAX_BOXES:
        raise ValueError('G = %d; 1 to %d instances are supported' % (G, TRAINING_ITEM_MAX_BOXES))
    plan_host = _training_item_plan(plan_host)
    M = int(plan_host[4])
    if M < 1 or M > TRAINING_ITEM_MAX_DIM:
        raise ValueError('IMAGE_MAX_DIM %d; 1 to %d is supported' % (M, TRAINING_ITEM_MAX_DIM))
    mini = bool(use_mini_mask)
    mh, mw = (int(mini_shape[0]), int(mini_shape[1])) if mini else (M, M)
    if mini and (mh < 1 or mw < 1 or mh > TRAINING_ITEM_MAX_MINI or mw > TRAINING_ITEM_MAX_MINI):
        raise ValueError('mini-masks of %d x %d; each side 1 to %d is supported' % (mh, mw, TRAINING_ITEM_MAX_MINI))
    _contiguous(named)
    _on_one_device(named, 'the training item only runs on the GPU')
    dev = frame_u8.device
    with torch.cuda.device(dev):
        plan = torch.from_numpy(plan_host).to(dev)   # the one upload
        ws = torch.empty(training_item_workspace_bytes(1, H, W, G), dtype=torch.uint8, device=dev)
        image = torch.empty(3, M, M, dtype=torch.float32, device=dev)
        boxes_int = torch.empty(G, 4, dtype=torch.int32, device=dev)
        boxes = torch.empty(G, 4, dtype=torch.float32, device=dev)
        boxes_norm = torch.empty(G, 4, dtype=torch.float32, device=dev)
        masks = torch.empty(G, mh, mw, dtype=torch.float32, device=dev)
        areas = torch.empty(G, dtype=torch.int32, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib().sdn_training_item(ptr(frame_u8), ptr(inst_map), int(inst_map.dtype == torch.uint8), ptr(ids), H, W, G,
                                      plan_host.ctypes.data, ptr(plan), plan_host.size, int(mini), mh if mini else 0, mw if mini else 0,
                                      ptr(ws), ws.numel(), ptr(image), ptr(boxes_int), ptr(boxes), ptr(boxes_norm), ptr(masks), ptr(areas),
                                      ptr(bad), stream()))
    return image, boxes_int, boxes, boxes_norm, masks, areas, bad


RPN_OUTPUTS_MAX_LEVELS, RPN_OUTPUTS_MAX_K, RPN_OUTPUTS_TILE = 8, 16, 64   # csrc/rpn_outputs_check.h: RPO_MAX_LEVELS, RPO_MAX_K, RPO_TILE
RPN_OUTPUTS_MAX_BATCH = 65535                                             # RPO_MAX_BATCH


class RpnOutputsFn(torch.autograd.Function):
    """The tail of RPN.forward on every pyramid level and the three cats of MaskRCNN.predict (geometric/maskrcnn/model.py:896-911,
    :1729-1740) -- sdn_rpn_outputs_fwd / _bwd (include/sdn_hip.h), one launch each way.  Inputs: the L class maps, then the L box maps.
    Returns (rpn_class_logits [B, A, 2], rpn_probs [B, A, 2], rpn_bbox [B, A, 4]).  An output that nothing differentiates arrives in
    backward as None and is not read: no buffer of zeros is made for it.  `rpn_outputs` below checks types and shapes."""

    @staticmethod
    def forward(ctx, *maps):
        L = len(maps) // 2
        cls, box = maps[:L], maps[L:]
        B, k = cls[0].shape[0], cls[0].shape[1] // 2
        H, W = [m.shape[2] for m in cls], [m.shape[3] for m in cls]
        A = k * sum(h * w for h, w in zip(H, W))
        dev = cls[0].device
        with torch.cuda.device(dev):
            logits = torch.empty(B, A, 2, dtype=torch.float32, device=dev)
            probs = torch.empty(B, A, 2, dtype=torch.float32, device=dev)
            bbox = torch.empty(B, A, 4, dtype=torch.float32, device=dev)
            check(lib().sdn_rpn_outputs_fwd(c_ptrs(cls), c_ptrs(box), c_ints(H), c_ints(W), L, k, B, ptr(logits), ptr(probs),
                                            ptr(bbox), stream()))
        ctx.save_for_backward(probs)
        ctx.sizes = (L, k, B, H, W)
        ctx.set_materialize_grads(False)
        return logits, probs, bbox

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits, g_probs, g_bbox):
        L, k, B, H, W = ctx.sizes
        if not any(ctx.needs_input_grad):
            return (None,) * (2 * L)
        (probs,) = ctx.saved_tensors
        dev = probs.device
        with torch.cuda.device(dev):
            g_logits, g_probs, g_bbox = [None if g is None else g.to(torch.float32).contiguous() for g in (g_logits, g_probs, g_bbox)]
            g_cls = [torch.empty(B, 2 * k, h, w, dtype=torch.float32, device=dev) for h, w in zip(H, W)]
            g_box = [torch.empty(B, 4 * k, h, w, dtype=torch.float32, device=dev) for h, w in zip(H, W)]
            check(lib().sdn_rpn_outputs_bwd(ptr(g_logits), ptr(g_probs), ptr(g_bbox), ptr(probs), c_ints(H), c_ints(W), L, k, B,
                                            c_ptrs(g_cls), c_ptrs(g_box), stream()))
        return tuple(g if need else None for g, need in zip(g_cls + g_box, ctx.needs_input_grad))


def rpn_outputs(class_maps, bbox_maps):
    """(rpn_class_logits fp32 [B, A, 2], rpn_probs fp32 [B, A, 2], rpn_bbox fp32 [B, A, 4]) from the outputs of conv_class and conv_bbox
    on the L pyramid levels (1 <= L <= 8): class_maps[l] fp32 [B, 2k, H_l, W_l], bbox_maps[l] fp32 [B, 4k, H_l, W_l], contiguous CUDA
    tensors, k anchors per location (1 <= k <= 16), A = k * sum H_l W_l.  It is what RPN.forward does after its convs
    (geometric/maskrcnn/model.py:896-911) and the cat over the levels of :1739: level l starts at anchor k * sum_{m<l} H_m W_m, anchor
    (y * W + x) * k + a, component j, is channel a * 2 + j (boxes: a * 4 + j) at pixel (y, x).  Logits and boxes are copies bit for
    bit, rpn_probs the fp32 softmax over (bg, fg).  One launch forward, one backward; differentiable in all 2L maps, the same bits
    every run; nothing is copied to the host.  A wrong type or dtype raises TypeError, a wrong shape or size or a non-contiguous tensor
    ValueError, a CPU tensor NotImplementedError: there is no torch form."""
    try:
        cls, box = list(class_maps), list(bbox_maps)
    except TypeError:
        raise TypeError('class_maps and bbox_maps must be sequences of tensors')
    if not 1 <= len(cls) <= RPN_OUTPUTS_MAX_LEVELS or len(box) != len(cls):
        raise ValueError('%d class maps and %d box maps; 1 to %d levels with one of each are supported' % (len(cls), len(box),
                                                                                                            RPN_OUTPUTS_MAX_LEVELS))
    named = [('class_maps[%d]' % l, m) for l, m in enumerate(cls)] + [('bbox_maps[%d]' % l, m) for l, m in enumerate(box)]
    _are_tensors(named)
    for name, m in named:
        if m.dtype != torch.float32:
            raise TypeError('%s must be %s, got %s' % (name, torch.float32, m.dtype))
        if m.dim() != 4 or min(m.shape) < 1:
            raise ValueError('%s must be fp32 [B, channels, H, W] without an empty axis, got %s' % (name, tuple(m.shape)))
    B, c2 = cls[0].shape[0], cls[0].shape[1]
    k = c2 // 2
    if c2 % 2 or not 1 <= k <= RPN_OUTPUTS_MAX_K:
        raise ValueError('class_maps[0] has %d channels; 2k with k = 1 to %d anchors per location are supported' % (c2, RPN_OUTPUTS_MAX_K))
    if B > RPN_OUTPUTS_MAX_BATCH:
        raise ValueError('batch %d; 1 to %d are supported' % (B, RPN_OUTPUTS_MAX_BATCH))
    for l, (c, b) in enumerate(zip(cls, box)):
        if tuple(c.shape) != (B, 2 * k, c.shape[2], c.shape[3]):
            raise ValueError('class_maps[%d] must be [%d, %d, H, W], got %s' % (l, B, 2 * k, tuple(c.shape)))
        if tuple(b.shape) != (B, 4 * k, c.shape[2], c.shape[3]):
            raise ValueError('bbox_maps[%d] must be [%d, %d, %d, %d], got %s' % (l, B, 4 * k, c.shape[2], c.shape[3], tuple(b.shape)))
    A = k * sum(c.shape[2] * c.shape[3] for c in cls)
    if B * A * 4 >= 2 ** 31:
        raise ValueError('B * A * 4 = %d must stay below 2^31' % (B * A * 4))
    _contiguous(named)
    _on_one_device(named, 'the RPN output kernels only run on the GPU')
    return RpnOutputsFn.apply(*(cls + box))


DERENDER_HEADS_MAX_CLASSES, DERENDER_HEADS_MAX_N = 16, 65535   # csrc/derender_heads_check.h: DH_MAX_CLASSES, DH_MAX_N
DERENDER_HEADS_ROWS, DERENDER_HEADS_SLAB = 16, 128               # DH_ROWS, DH_SLAB
DERENDER_HEADS_KEYS = ('_theta_deltas', '_translation2ds', '_log_scales', '_log_depths', '_class_probs', '_ffd_coeffs')


@_remembered
def _dh_workspace_bytes(*sizes):
    """the library's own answer, remembered per shape"""
    return size_query(lib().sdn_derender_heads_workspace_bytes, sizes)


def derender_heads_workspace_bytes(n, F, Hd, classes, coeffs):
    """bytes of the workspace of sdn_derender_heads_bwd: the library's own answer, remembered per shape"""
    return _dh_workspace_bytes(int(n), int(F), int(Hd), int(classes), int(coeffs))


def _dh_pieces(out, n, classes, coeffs):
    """the six output groups, contiguous pieces of the one buffer `out` [n * O] (include/sdn_hip.h)"""
    widths, pieces, at = (2, 2, 3, 1, classes, classes * coeffs), [], 0
    for w in widths:
        pieces.append(out[at:at + n * w].view(n, w))
        at += n * w
    pieces[5] = pieces[5].view(n, classes, coeffs)
    return pieces


class DerenderHeadsFn(torch.autograd.Function):
    """The Derenderer's heads (geometric/derender3d/models/derenderer.py:34-56 of the reference, models/__init__.py:70-77) --
    sdn_derender_heads_fwd / _bwd (include/sdn_hip.h), four launches each way.  Inputs: pooled, roi_norms or None, centre or None,
    extent or None, the four (weight, bias) pairs flat, the class count.  Returns the six output groups, and with roi_norms the
    centre and the extent behind them (no gradient).  Only what needs_input_grad asks for is computed; an output that nothing
    differentiates arrives as None and is not read.  `derender_heads` below checks types and shapes."""

    @staticmethod
    def forward(ctx, pooled, roi_norms, centre, extent, w0, b0, w1, b1, w2, b2, w3, b3, classes):
        n, F = pooled.shape
        Hd, O = w0.shape[0], w3.shape[0]
        coeffs = (O - 8 - classes) // classes
        dev = pooled.device
        with torch.cuda.device(dev):
            out = torch.empty(n * O, dtype=torch.float32, device=dev)
            saved = torch.empty(n * (3 * Hd + 1), dtype=torch.float32, device=dev)
            made = []
            if roi_norms is not None:
                centre, extent = (torch.empty(n, 2, dtype=torch.float32, device=dev) for _ in range(2))
                made = [centre, extent]
            check(lib().sdn_derender_heads_fwd(ptr(pooled), ptr(roi_norms), None if made else ptr(centre), None if made else ptr(extent),
                                               ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), n, F, Hd, classes,
                                               coeffs, ptr(out), ptr(made[0]) if made else None, ptr(made[1]) if made else None, None,
                                               ptr(saved), stream()))
        ctx.save_for_backward(pooled, centre, extent, w0, w1, w2, w3, out, saved)
        ctx.sizes = (n, F, Hd, classes, coeffs)
        ctx.set_materialize_grads(False)
        if made:
            ctx.mark_non_differentiable(*made)
        return tuple(_dh_pieces(out, n, classes, coeffs) + made)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        need = ctx.needs_input_grad
        wanted = [need[0]] + list(need[4:12])            # pooled, then w0, b0, .. w3, b3
        if not any(wanted):
            return (None,) * 13
        n, F, Hd, classes, coeffs = ctx.sizes
        pooled, centre, extent, w0, w1, w2, w3, out, saved = ctx.saved_tensors
        dev = pooled.device
        shapes = [(n, F), (Hd, F), (Hd,), (Hd, Hd + 4), (Hd,), (Hd, Hd), (Hd,), tuple(w3.shape), (w3.shape[0],)]
        with torch.cuda.device(dev):
            g = [None if t is None else t.to(torch.float32).contiguous() for t in grads[:6]]
            gin = [torch.empty(shape, dtype=torch.float32, device=dev) if w else None for shape, w in zip(shapes, wanted)]
            ws = torch.empty(derender_heads_workspace_bytes(n, F, Hd, classes, coeffs), dtype=torch.uint8, device=dev)
            check(lib().sdn_derender_heads_bwd(*[ptr(t) for t in g], ptr(pooled), ptr(centre), ptr(extent), ptr(w0), ptr(w1), ptr(w2),
                                               ptr(w3), ptr(out), ptr(saved), n, F, Hd, classes, coeffs, *[ptr(t) for t in gin], ptr(ws),
                                               ws.numel(), stream()))
        return (gin[0], None, None, None) + tuple(gin[1:]) + (None,)


def _dh_layer(layer, name):
    """(weight, bias) of an nn.Linear or of a pair"""
    if isinstance(layer, (tuple, list)) and len(layer) == 2:
        return layer[0], layer[1]
    if hasattr(layer, 'weight') and hasattr(layer, 'bias') and layer.bias is not None:
        return layer.weight, layer.bias
    raise TypeError('%s must be an nn.Linear with a bias or a (weight, bias) pair, got %r' % (name, type(layer)))


def derender_heads(pooled, rois, fc, fc1, fc2, fc3, num_classes):
    """The blob of Derenderer.forward from the ResNet's pooled features: pooled fp32 [n, F]; rois either roi_norms fp32 [n, 4] (then the
    blob also holds `_mroi_norms` = (br + tl) / 2 and `_droi_norms` = br - tl, bit-equal to torch) or the pair (centre, extent) of fp32
    [n, 2]; fc (F -> Hd), fc1 (Hd + 4 -> Hd), fc2 (Hd -> Hd), fc3 (Hd -> 8 + classes + classes * coeffs): nn.Linear modules or
    (weight, bias) pairs, read in place.  F and Hd multiples of 4, 1 to 16 classes, n up to 65535; n = 0 returns empty tensors without
    a launch.  Returns `_theta_deltas` [n, 2], `_translation2ds` [n, 2], `_log_scales` [n, 3], `_log_depths` [n, 1], `_class_probs`
    [n, classes], `_ffd_coeffs` [n, classes, coeffs], pieces of one buffer.  Four launches forward, at most four backward,
    differentiable in pooled and the eight parameters, the same bits every run; an object's row does not depend on its batch.  A wrong
    type or dtype raises TypeError, a wrong shape or size, a non-contiguous tensor or a roi tensor that requires a gradient ValueError,
    a CPU tensor NotImplementedError: there is no torch form."""
    if isinstance(rois, torch.Tensor):
        roi_norms, pair, named = rois, None, [('pooled', pooled), ('roi_norms', rois)]
    elif isinstance(rois, (tuple, list)) and len(rois) == 2:
        roi_norms, pair, named = None, tuple(rois), [('pooled', pooled), ('centre', rois[0]), ('extent', rois[1])]
    else:
        raise TypeError('rois must be roi_norms [n, 4] or the pair (centre, extent), got %r' % type(rois))
    classes = int(num_classes)
    layers = []
    for name, layer in (('fc', fc), ('fc1', fc1), ('fc2', fc2), ('fc3', fc3)):
        w, b = _dh_layer(layer, name)
        layers += [(name + '.weight', w), (name + '.bias', b)]
    named += layers
    _are_tensors(named)
    for name, t in named:
        if t.dtype != torch.float32:
            raise TypeError('%s must be %s, got %s' % (name, torch.float32, t.dtype))
    if pooled.dim() != 2:
        raise ValueError('pooled must be fp32 [n, F], got %s' % (tuple(pooled.shape),))
    n, F = pooled.shape
    if not 1 <= classes <= DERENDER_HEADS_MAX_CLASSES:
        raise ValueError('%d classes; 1 to %d are supported' % (classes, DERENDER_HEADS_MAX_CLASSES))
    if n > DERENDER_HEADS_MAX_N:
        raise ValueError('n %d; up to %d objects are supported' % (n, DERENDER_HEADS_MAX_N))
    w0, w3 = layers[0][1], layers[6][1]
    Hd, O = (w0.shape[0], w3.shape[0]) if w0.dim() == 2 and w3.dim() == 2 else (0, 0)
    if F < 4 or F % 4 or Hd < 4 or Hd % 4:
        raise ValueError('F %d and Hd %d (fc.weight %s); positive multiples of 4 are supported' % (F, Hd, tuple(w0.shape)))
    coeffs = (O - 8 - classes) // classes
    if coeffs < 1 or 8 + classes + classes * coeffs != O:
        raise ValueError('fc3 has %d outputs; 8 + classes + classes * coeffs with %d classes is supported' % (O, classes))
    shapes = [(Hd, F), (Hd,), (Hd, Hd + 4), (Hd,), (Hd, Hd), (Hd,), (O, Hd), (O,)]
    for (name, t), shape in zip(layers, shapes):
        if tuple(t.shape) != shape:
            raise ValueError('%s must be %s, got %s' % (name, list(shape), tuple(t.shape)))
    for name, t in named[1:len(named) - 8]:
        shape = (n, 4) if roi_norms is not None else (n, 2)
        if tuple(t.shape) != shape:
            raise ValueError('%s must be %s, got %s' % (name, list(shape), tuple(t.shape)))
        if t.requires_grad:
            raise ValueError('%s requires a gradient; the heads give none to the roi vectors' % name)
    if max(n * O, n * F, O * Hd, Hd * F) >= 2 ** 31:
        raise ValueError('n * O, n * F, O * Hd and Hd * F must stay below 2^31')
    _contiguous(named)
    _on_one_device(named, 'the derenderer heads only run on the GPU')
    if n == 0:
        empty = [pooled.new_empty(0, w) for w in (2, 2, 3, 1, classes)] + [pooled.new_empty(0, classes, coeffs)]
        blob = dict(zip(DERENDER_HEADS_KEYS, empty))
        if roi_norms is not None:
            blob['_mroi_norms'], blob['_droi_norms'] = pooled.new_empty(0, 2), pooled.new_empty(0, 2)
        return blob
    centre, extent = pair if pair is not None else (None, None)
    got = DerenderHeadsFn.apply(pooled, roi_norms, centre, extent, *[t for _name, t in layers], classes)
    blob = dict(zip(DERENDER_HEADS_KEYS, got[:6]))
    if roi_norms is not None:
        blob['_mroi_norms'], blob['_droi_norms'] = got[6], got[7]
    return blob


SEGM_PPM_MAX_SCALES, SEGM_PPM_MAX_SIDE = 4, 8   # csrc/segm_ppm_check.h: PPM_MAX_SCALES, PPM_MAX_SIDE


class SegmPpmPoolFn(torch.autograd.Function):
    """First half of the pyramid pooling module (semantic/models.py:336-346, 387-397): sdn_segm_ppm_pool forward,
    sdn_segm_ppm_pool_bwd backward, one launch each.  Returns (cat [B, C + sum K, h, w] with conv5 in its first C channels and
    the others left for SegmPpmFillFn, p_1 .. p_S [B, C, s_k, s_k]: torch's AdaptiveAvgPool2d(s_k) of conv5, contiguous segments
    of one buffer).  `segm_ppm_pool` below checks types and shapes."""

    @staticmethod
    def forward(ctx, conv5, scales, branch_channels):
        x = _f32(conv5, 'conv5')
        B, C, h, w = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            cat = torch.empty(B, C + sum(branch_channels), h, w, dtype=torch.float32, device=dev)
            pooled = torch.empty(B * C * sum(s * s for s in scales), dtype=torch.float32, device=dev)
            check(lib().sdn_segm_ppm_pool(ptr(x), B, C, h, w, c_ints(scales), c_ints(branch_channels), len(scales), ptr(cat),
                                          ptr(pooled), stream()))
        ps, at = [], 0
        for s in scales:
            ps.append(pooled[at:at + B * C * s * s].view(B, C, s, s))
            at += B * C * s * s
        ctx.scales, ctx.channels, ctx.shape = tuple(scales), tuple(branch_channels), (B, C, h, w)
        ctx.set_materialize_grads(False)   # an unused output arrives as None, not as a tensor of zeros to be read
        return (cat,) + tuple(ps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cat, *g_p):
        if not ctx.needs_input_grad[0] or (g_cat is None and all(g is None for g in g_p)):
            return None, None, None
        B, C, h, w = ctx.shape
        given = [g for g in (g_cat,) + tuple(g_p) if g is not None]
        dev = given[0].device
        with torch.cuda.device(dev):
            g_cat = None if g_cat is None else g_cat.to(torch.float32).contiguous()
            g_p = [None if g is None else g.to(torch.float32).contiguous() for g in g_p]
            gx = torch.empty(B, C, h, w, dtype=torch.float32, device=dev)
            check(lib().sdn_segm_ppm_pool_bwd(ptr(g_cat), c_ptrs(g_p), B, C, h, w, c_ints(ctx.scales), c_ints(ctx.channels),
                                              len(ctx.scales), ptr(gx), stream()))
        return gx, None, None


class SegmPpmFillFn(torch.autograd.Function):
    """Second half of the pyramid pooling module: sdn_segm_ppm_fill writes the bilinear upsampling of the branch outputs y_k
    [B, K_k, s_k, s_k] into the channels >= C of `cat`, IN PLACE (ctx.mark_dirty), and returns cat; sdn_segm_ppm_fill_bwd gives
    the gradients of the y_k that need one, and the gradient of `cat` is the incoming one itself, uncopied -- SegmPpmPoolFn's
    backward reads its first C channels."""

    @staticmethod
    def forward(ctx, cat, C, *ys):
        ys = [_f32(y, 'y[%d]' % k) for k, y in enumerate(ys)]
        B, _, h, w = cat.shape
        scales, channels = [int(y.shape[2]) for y in ys], [int(y.shape[1]) for y in ys]
        with torch.cuda.device(cat.device):
            check(lib().sdn_segm_ppm_fill(c_ptrs(ys), B, C, h, w, c_ints(scales), c_ints(channels), len(ys), ptr(cat), stream()))
        ctx.mark_dirty(cat)
        ctx.scales, ctx.channels, ctx.C = scales, channels, C
        return cat

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        need = ctx.needs_input_grad[2:]
        gys = [None] * len(need)
        if any(need):
            B, _, h, w = g.shape
            with torch.cuda.device(g.device):
                g = g.to(torch.float32).contiguous()
                gys = [torch.empty(B, K, s, s, dtype=torch.float32, device=g.device) if n else None
                       for n, K, s in zip(need, ctx.channels, ctx.scales)]
                check(lib().sdn_segm_ppm_fill_bwd(ptr(g), B, ctx.C, h, w, c_ints(ctx.scales), c_ints(ctx.channels), len(need),
                                                  c_ptrs(gys), stream()))
        return (g if ctx.needs_input_grad[0] else None, None) + tuple(gys)


def _ppm_tensor(t, name):
    _is_tensor(t, name)
    if t.dtype != torch.float32:
        raise TypeError('%s must be torch.float32, got %s' % (name, t.dtype))
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError('%s must be fp32 [B, C, h, w] without an empty axis, got %s' % (name, tuple(t.shape)))


def segm_ppm_pool(conv5, scales, branch_channels):
    """(cat, p_1 .. p_S) of SegmPpmPoolFn for conv5 CUDA fp32 [B, C, h, w], `scales` (1 to 4 ints in 1 .. 8; the decoders use
    (1, 2, 3, 6)) and `branch_channels` (K_k >= 1 per scale).  cat [B, C + sum K_k, h, w] holds conv5 in its first C channels,
    bit for bit; its other channels are UNWRITTEN until segm_ppm_fill.  p_k equals F.adaptive_avg_pool2d(conv5, s_k).
    Differentiable in conv5 through both cat and every p_k.  A wrong type or dtype raises TypeError, a wrong shape or size
    ValueError, a CPU tensor NotImplementedError; the library is not touched before."""
    try:
        scales, branch_channels = [int(s) for s in scales], [int(k) for k in branch_channels]
    except TypeError:
        raise TypeError('scales and branch_channels must be sequences of ints')
    if not 1 <= len(scales) <= SEGM_PPM_MAX_SCALES or len(branch_channels) != len(scales):
        raise ValueError('1 to %d scales with as many branch_channels, got %r and %r' % (SEGM_PPM_MAX_SCALES, scales, branch_channels))
    if any(s < 1 or s > SEGM_PPM_MAX_SIDE for s in scales) or any(k < 1 for k in branch_channels):
        raise ValueError('scales must lie in 1 .. %d and branch_channels be >= 1, got %r and %r' % (SEGM_PPM_MAX_SIDE, scales, branch_channels))
    if isinstance(conv5, torch.Tensor) and conv5.dtype == torch.float32 and conv5.dim() != 4:
        raise ValueError('conv5 must be fp32 [B, C, h, w], got %s' % (tuple(conv5.shape),))
    _ppm_tensor(conv5, 'conv5')
    B, C, h, w = conv5.shape
    if B * (C + sum(branch_channels)) * h * w >= 2 ** 31:
        raise ValueError('B * (C + sum K) * h * w = %d must stay below 2^31' % (B * (C + sum(branch_channels)) * h * w))
    _on_gpu(conv5, 'conv5', 'the pyramid pooling kernels only run on the GPU')
    return SegmPpmPoolFn.apply(conv5, tuple(scales), tuple(branch_channels))


def segm_ppm_fill(cat, C, *ys):
    """Writes the bilinear upsampling (align_corners=False) of the branch outputs y_1 .. y_S (as arguments, or one list of
    them), y_k CUDA fp32 [B, K_k, s_k, s_k], into cat[:, C:] IN PLACE and returns cat: branch k takes the K_k channels after
    C + sum_{k' < k} K_k'.  cat must be the contiguous [B, C + sum K_k, h, w] tensor of segm_ppm_pool.  Differentiable in cat
    and every y_k.  A wrong type or dtype raises TypeError, a wrong shape ValueError, a CPU tensor NotImplementedError; the
    library is not touched before."""
    ys = list(ys[0]) if len(ys) == 1 and isinstance(ys[0], (list, tuple)) else list(ys)
    if not 1 <= len(ys) <= SEGM_PPM_MAX_SCALES:
        raise ValueError('1 to %d branch outputs, got %d' % (SEGM_PPM_MAX_SCALES, len(ys)))
    for t, name in [(cat, 'cat')] + [(y, 'y[%d]' % k) for k, y in enumerate(ys)]:
        if isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() != 4:
            raise ValueError('%s must be fp32 with four axes, got %s' % (name, tuple(t.shape)))
    C = int(C)
    devs = [t.device for t in [cat] + ys if isinstance(t, torch.Tensor)]
    for t, name in [(cat, 'cat')] + [(y, 'y[%d]' % k) for k, y in enumerate(ys)]:
        _is_tensor(t, name)
        if t.dtype != torch.float32:
            raise TypeError('%s must be torch.float32, got %s' % (name, t.dtype))
    B, Ctot, h, w = cat.shape
    for k, y in enumerate(ys):
        if y.shape[0] != B or y.shape[1] < 1 or y.shape[2] != y.shape[3] or not 1 <= y.shape[2] <= SEGM_PPM_MAX_SIDE:
            raise ValueError('y[%d] must be [%d, K, s, s] with K >= 1 and s in 1 .. %d, got %s' % (k, B, SEGM_PPM_MAX_SIDE, tuple(y.shape)))
    if C < 1 or C + sum(int(y.shape[1]) for y in ys) != Ctot or min(cat.shape) < 1:
        raise ValueError('cat has %d channels; C = %d and the branches hold %r' % (Ctot, C, [int(y.shape[1]) for y in ys]))
    if B * Ctot * h * w >= 2 ** 31:
        raise ValueError('B * Ctot * h * w = %d must stay below 2^31' % (B * Ctot * h * w))
    if any(d != devs[0] for d in devs):
        raise ValueError('cat and the branch outputs are on different devices: %r' % (devs,))
    _on_gpu(cat, 'cat', 'the pyramid pooling kernels only run on the GPU')
    if not cat.is_contiguous():
        raise ValueError('cat must be contiguous: it is written in place')
    return SegmPpmFillFn.apply(cat, C, *ys)


# ---- the input side of the textural networks (csrc/encode_input.hip) ---------------------------------------------------------------
MAP_U8, MAP_I16, MAP_I32, MAP_F32 = 0, 1, 2, 3                 # include/sdn_hip.h: SDN_MAP_*
ENCODE_MAX_CHANNELS = 256                                       # csrc/encode_input_check.h: ENC_MAX_CHANNELS
INST_KEY_MIN, INST_KEY_BITS = -32768, 1 << 21                   # the key window [INST_KEY_MIN, INST_KEY_MIN + INST_KEY_BITS)
INST_HEAD_AT = (INST_KEY_BITS // 32) * 4                        # byte of (K, overflow) in the workspace, behind the bitmap
_MAP_DTYPES = {torch.uint8: MAP_U8, torch.int16: MAP_I16, torch.int32: MAP_I32, torch.float32: MAP_F32}
ENCODE_LABEL_DTYPES = (torch.uint8, torch.int32, torch.float32)
ENCODE_INST_DTYPES = (torch.int16, torch.int32, torch.float32)
ENCODE_POSE_DTYPES = (torch.int32, torch.float32)


def _index_map(t, name, dtypes, like=None):
    """a contiguous [N, 1, H, W] map of one of `dtypes`, of `like`'s shape and device when given"""
    _is_tensor(t, name)
    if t.dtype not in dtypes:
        raise TypeError('%s must be one of %s, got %s' % (name, ', '.join(str(d) for d in dtypes), t.dtype))
    if t.dim() != 4 or t.shape[1] != 1 or min(t.shape) < 1:
        raise ValueError('%s must be [N, 1, H, W] without an empty axis, got %s' % (name, tuple(t.shape)))
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError('%s is %s on %s, label %s on %s' % (name, tuple(t.shape), t.device, tuple(like.shape), like.device))
    if t.numel() >= 2 ** 31:
        raise ValueError('%s holds %d elements; the sizes must stay below 2^31' % (name, t.numel()))


def encode_maps(label, inst, pose, label_nc, pose_ch):
    """The label planes, edge plane and pose planes of Pix2PixHDModel.encode_input in one launch (sdn_encode_maps;
    textural/models/pix2pixHD_model.py:124-166, 343-349).  label CUDA [N, 1, H, W] uint8 / int32 / float32; inst likewise int16 /
    int32 / float32, or None for no edge plane; pose int32 / float32, or None with pose_ch 0.  1 <= label_nc <= 256,
    pose_ch = feat_pose_num_bins + 1 <= 256.  Returns (input_label fp32 [N, label_nc (+ 1 with inst), H, W],
    pose_onehot fp32 [N, pose_ch, H, W] or None, bad int32 [2] on the device): the planes of `scatter_(1, map.long(), 1.0)` and
    get_edges; an index outside [0, channels) or a NaN sets no plane and is counted in bad[0] (label) / bad[1] (pose), where the
    reference's scatter_ trips a device-side assert.  A map that is not contiguous is copied.  A wrong type or dtype raises
    TypeError, a wrong shape or size ValueError, a CPU tensor NotImplementedError; the library is not touched before."""
    label_nc, pose_ch = int(label_nc), int(pose_ch)
    _index_map(label, 'label', ENCODE_LABEL_DTYPES)
    if inst is not None:
        _index_map(inst, 'inst', ENCODE_INST_DTYPES, label)
    if not 1 <= label_nc <= ENCODE_MAX_CHANNELS or not 0 <= pose_ch <= ENCODE_MAX_CHANNELS:
        raise ValueError('label_nc must lie in 1 .. %d and pose_ch in 0 .. %d, got %d and %d'
                         % (ENCODE_MAX_CHANNELS, ENCODE_MAX_CHANNELS, label_nc, pose_ch))
    if (pose is None) != (pose_ch == 0):
        raise ValueError('pose and pose_ch go together: pose is %s with pose_ch %d' % ('None' if pose is None else 'given', pose_ch))
    if pose is not None:
        _index_map(pose, 'pose', ENCODE_POSE_DTYPES, label)
    N, _, H, W = label.shape
    planes = label_nc + (0 if inst is None else 1)
    if N * max(planes, pose_ch) * H * W >= 2 ** 31:
        raise ValueError('N * channels * H * W = %d must stay below 2^31' % (N * max(planes, pose_ch) * H * W))
    if label.device.type != 'cuda':   # (the device's type, not is_cuda as _on_gpu asks: kept as it was, so inline)
        raise NotImplementedError('label is on %s; the input encoding kernels only run on the GPU' % (label.device,))
    label = label.contiguous()
    inst = None if inst is None else inst.contiguous()
    pose = None if pose is None else pose.contiguous()
    dev = label.device
    with torch.cuda.device(dev):
        input_label = torch.empty(N, planes, H, W, dtype=torch.float32, device=dev)
        pose_onehot = torch.empty(N, pose_ch, H, W, dtype=torch.float32, device=dev) if pose_ch else None
        bad = torch.empty(2, dtype=torch.int32, device=dev)
        check(lib().sdn_encode_maps(ptr(label), _MAP_DTYPES[label.dtype], ptr(inst), _MAP_DTYPES[inst.dtype] if inst is not None else 0,
                                    ptr(pose), _MAP_DTYPES[pose.dtype] if pose is not None else 0, N, H, W, label_nc, pose_ch,
                                    ptr(input_label), ptr(pose_onehot), ptr(bad), stream()))
    return input_label, pose_onehot, bad


_inst_workspaces = {}


def inst_index_workspace(device):
    """The workspace of sdn_inst_index_* on `device` (a presence bitmap of the key window, its prefix counts, K and overflow: 512
    KiB + 16 bytes), one per device and calling stream; sdn_inst_index_build clears what it needs."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _inst_workspaces.get(key)
    if ws is None:
        ws = _inst_workspaces[key] = torch.empty(size_query(lib().sdn_inst_index_workspace_bytes), dtype=torch.uint8, device=device)
    return ws


def inst_index(inst, with_counts=False):
    """The instance numbering of Encoder.forward without a sort (sdn_inst_index_build / _rank; textural/models/networks.py:310-325:
    inst[i] = inst[i] * bs + i, then the unique values of every pixel).  inst CUDA contiguous [N, 1, H, W] int16 / int32 /
    float32; it is DISAMBIGUATED IN PLACE, as the reference does.  Returns (ids int64 [K] ascending, seg int32 [N, H, W] with
    ids[seg] == inst.long(), counts int64 [K] pixels per id or None, info): what torch.unique(inst.reshape(-1).long(),
    return_inverse=True, return_counts=with_counts) gives.  One 8-byte copy to the host (K and overflow).  info['path'] is
    'device', or 'torch' when info['overflow'] pixels had a key outside [-32768, 2^21 - 32768) or NaN / Inf: torch.unique then
    runs on the already disambiguated map.  A wrong type or dtype raises TypeError, a wrong shape or a map that is not contiguous
    ValueError, a CPU tensor NotImplementedError; the library is not touched before."""
    _index_map(inst, 'inst', ENCODE_INST_DTYPES)
    if inst.device.type != 'cuda':   # (as in encode_maps)
        raise NotImplementedError('inst is on %s; the instance numbering kernels only run on the GPU' % (inst.device,))
    if not inst.is_contiguous():
        raise ValueError('inst must be contiguous: it is disambiguated in place')
    N, _, H, W = inst.shape
    dev = inst.device
    dt = _MAP_DTYPES[inst.dtype]
    with torch.cuda.device(dev):
        ws = inst_index_workspace(dev)
        cap = min(N * H * W, INST_KEY_BITS)
        ids = torch.empty(cap, dtype=torch.int64, device=dev)
        counts = torch.empty(cap, dtype=torch.int64, device=dev) if with_counts else None
        seg = torch.empty(N, H, W, dtype=torch.int32, device=dev)
        check(lib().sdn_inst_index_build(ptr(inst), dt, N, H, W, ptr(ws), ws.numel(), ptr(ids), ptr(counts), cap, stream()))
        check(lib().sdn_inst_index_rank(ptr(inst), dt, N, H, W, ptr(ws), ws.numel(), ptr(seg), ptr(counts), stream()))
        K, overflow = ws[INST_HEAD_AT:INST_HEAD_AT + 8].view(torch.int32).tolist()   # the one copy to the host
    if overflow:
        got = torch.unique(inst.reshape(-1).long(), return_inverse=True, return_counts=with_counts)
        return got[0], got[1].to(torch.int32).reshape(N, H, W), (got[2] if with_counts else None), {'path': 'torch', 'overflow': overflow}
    return ids[:K], seg, (counts[:K] if with_counts else None), {'path': 'device', 'overflow': 0}
