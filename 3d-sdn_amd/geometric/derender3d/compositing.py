"""Per-frame compositing of the rendered objects on the device + the wire format to the textural branch.

Reference: geometric/scripts/main.py:541-622 -- for every object, far to near: PIL-resize its 384 x 384 silhouette,
normal and depth renders to `render_size / zoom` pixels, paste them into frame-sized canvases at the projected centre,
and blend `(1 - mask) * map + mask * new` into the instance / normal / depth maps; then write NNNNN.png (uint8 instance
ids), NNNNN-normal.png, NNNNN-depth.png (16 bit) and NNNNN.json.  The reference does this with ~10 PIL / numpy round
trips per object on the host.

Here the host only prepares what PIL's resampler would precompute (ImagingResample's `precompute_coeffs` /
`normalize_coeffs_8bpc`: per output pixel a source window and its bilinear weights, 22-bit fixed point for the 8-bit
images, double for the float depth), and ONE kernel (sdn_composite_frame, csrc/raster_composite.hip) walks the frame:
every pixel finds the nearest object whose resized, rounded mask covers it and evaluates PIL's two-pass resampling
(horizontal, rounded to the pixel type, then vertical) for that pixel only.  Results are bit-identical to the PIL
path (tests/test_composite.py, tests/test_gpu_composite.py).

This module has no CPU fallback: CPU tensors raise NotImplementedError.
"""
import functools
import json
import os

import numpy as np
import torch

from sdn_hip.pillow import PRECISION_BITS, fixed_point, resample_tables  # noqa: E402,F401  (moved there: the semantic branch shares them)


def resample_u8_numpy(img, out_size):
    """Host emulation of ImagingResample on an 8-bit [H, W] image (square resize) -- used by the CPU tests to pin the
    tables against the real PIL; the device kernel evaluates the same sums per pixel."""
    R = img.shape[0]
    if out_size == R:
        return img.copy()
    ksize, bounds, kk = resample_tables(R, out_size)
    k8 = fixed_point(kk).astype(np.int64)
    half = 1 << (PRECISION_BITS - 1)
    tmp = np.zeros((R, out_size), dtype=np.int64)
    for ox in range(out_size):
        x0, c = bounds[ox]
        tmp[:, ox] = half + (img[:, x0:x0 + c].astype(np.int64) * k8[ox, :c]).sum(axis=1)
    tmp = np.clip(tmp >> PRECISION_BITS, 0, 255)
    out = np.zeros((out_size, out_size), dtype=np.int64)
    for oy in range(out_size):
        y0, c = bounds[oy]
        out[oy] = half + (tmp[y0:y0 + c] * k8[oy, :c, None]).sum(axis=0)
    return np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_f32_numpy(img, out_size):
    """The 32-bit float path of ImagingResample (double accumulation, float32 store after each pass)."""
    R = img.shape[0]
    if out_size == R:
        return img.copy()
    ksize, bounds, kk = resample_tables(R, out_size)
    tmp = np.zeros((R, out_size), dtype=np.float32)
    for ox in range(out_size):
        x0, c = bounds[ox]
        acc = np.zeros(R, dtype=np.float64)
        for x in range(c):
            acc = acc + img[:, x0 + x].astype(np.float64) * kk[ox, x]
        tmp[:, ox] = acc.astype(np.float32)
    out = np.zeros((out_size, out_size), dtype=np.float32)
    for oy in range(out_size):
        y0, c = bounds[oy]
        acc = np.zeros(out_size, dtype=np.float64)
        for y in range(c):
            acc = acc + tmp[y0 + y].astype(np.float64) * kk[oy, y]
        out[oy] = acc.astype(np.float32)
    return out


def paste_geometry(zooms, center2ds, focal, u0, v0, render_size):
    """Per object: (size, left, top) exactly as main.py:556-569 computes them (float32 tensor arithmetic, int())."""
    z = np.asarray(zooms, dtype=np.float32).reshape(-1)
    c = np.asarray(center2ds, dtype=np.float32).reshape(-1, 2)
    out = []
    for i in range(z.shape[0]):
        size = int(np.float32(render_size) / z[i])
        left = int(c[i, 1] * np.float32(focal) + np.float32(u0) - np.float32(size // 2))
        top = int(c[i, 0] * np.float32(focal) + np.float32(v0) - np.float32(size // 2))
        out.append((size, left, top))
    return out


def host_state(depths, zooms, center2ds, *more):
    """The few per-object scalars compositing and the JSON record need on the HOST (depths for the painter's order, zooms and
    projected centres for the paste geometry, plus whatever `more` [n] / [n,1] tensors the caller wants, e.g. the alphas of the
    JSON record) in ONE device-to-host copy -- composite_frame otherwise reads them one by one, each a device synchronisation.
    Accepts tensors of SEVERAL frames stacked along dim 0 ([F, n, ...]).  -> float32 numpy array [..., n, 4 + len(more)]:
    depth, zoom, centre y, centre x, more..."""
    # the leading shape [..., n] comes from center2ds [..., n, 2], whose last dimension is never the object count (ADVICE r05:
    # guessing it from a trailing 1 of `depths` mis-read stacked frames of ONE object, [F, 1], as [F] + a singleton)
    lead = center2ds.shape[:-1]
    cols = [depths.reshape(*lead, 1).float(), zooms.reshape(*lead, 1).float(), center2ds.reshape(*lead, 2).float()]
    cols += [m.reshape(*lead, 1).float() for m in more]
    return torch.cat(cols, dim=-1).detach().cpu().numpy()


def composite_frame(masks, normals, depth_maps, depths, zooms, center2ds, interests, focal, u0, v0, height, width,
                    render_size=None, image_masks=None, host=None):
    """Device version of main.py:541-602.  masks [n,1,R,R], normals [n,3,R,R], depth_maps [n,1,R,R] (CUDA float32),
    depths [n,1], zooms [n]/[n,1], center2ds [n,2] = (y, x), interests [n].  host: this frame's row block of host_state()
    ([n, >= 4]: depth, zoom, centre y, centre x) -- then nothing is read back from the device here.  Returns
    (instance [1,H,W], normal [3,H,W], depth [1,H,W], painter order) as CUDA tensors / list."""
    from sdn_hip import check, lib, ptr, stream
    if not masks.is_cuda:
        raise NotImplementedError('composite_frame runs on the GPU only (no CPU fallback)')
    import ctypes
    dev = masks.device
    n, _, R, _ = masks.shape
    render_size = R if render_size is None else render_size
    if host is None:
        # far -> near (one host sync, as the reference); stable, so that equal depths keep index order on this path and on
        # the host= path below alike
        order = torch.sort(depths[:, 0], dim=0, descending=True, stable=True)[1].tolist()
        zooms_h = zooms.detach().reshape(-1).float().cpu().numpy()
        c2d_h = center2ds.detach().float().cpu().numpy()
    else:
        host = np.asarray(host, dtype=np.float32)
        # ties keep index order, as the stable device sort above
        order = [int(i) for i in np.argsort(-host[:, 0], kind='stable')]
        zooms_h, c2d_h = host[:, 1], host[:, 2:4]
    geo = paste_geometry(zooms_h, c2d_h, focal, u0, v0, render_size)
    interests_h = [bool(v) for v in (interests.reshape(-1).tolist() if isinstance(interests, torch.Tensor) else interests)]
    inst = torch.zeros(1, height, width, device=dev)
    nrm = torch.full((3, height, width), 0.5, device=dev)
    dep = torch.full((1, height, width), 1.0, device=dev)
    masks_c, normals_c, depth_c = masks.contiguous().float(), normals.contiguous().float(), depth_maps.contiguous().float()
    zooms_d = zooms.detach().reshape(-1).float().contiguous()

    def flush(run):
        if not run:
            return
        # tables of the distinct sizes in this run
        table, bounds_all, k8_all, kf_all = {}, [], [], []
        for i in run:
            size = geo[i][0]
            if size == R or size in table:
                continue
            if size < 1:
                raise ValueError('object %d: paste size %d (zoom %g)' % (i, size, float(zooms_h[i])))
            ksize, bounds, kk = resample_tables(R, size)
            table[size] = (sum(b.shape[0] for b in bounds_all), ksize)
            bounds_all.append(bounds)
            k8_all.append((fixed_point(kk).reshape(-1), kk.reshape(-1)))
        objs = np.zeros((len(run), 6), dtype=np.int32)
        koff = {}
        off = 0
        for (size, (boff, ksize)), (k8, kf) in zip(table.items(), k8_all):
            koff[size] = off
            off += k8.shape[0]
        for j, i in enumerate(run):
            size, left, top = geo[i]
            boff, ksize = table.get(size, (0, 0))
            objs[j] = (i, size, left, top, boff, koff.get(size, 0))
        ksz = np.array([table.get(geo[i][0], (0, 0))[1] for i in run], dtype=np.int32)
        # ONE host-to-device copy for the four small tables (r05: they were four pageable copies per frame, each of which holds
        # the host until the stream has taken it): float64 weights first (8-byte aligned), then the int32 tables
        kf_h = np.concatenate([b for _, b in k8_all]) if k8_all else np.zeros(1, np.float64)
        bounds_h = (np.concatenate(bounds_all) if bounds_all else np.zeros((1, 2), np.int32)).astype(np.int32).reshape(-1)
        k8_h = (np.concatenate([a for a, _ in k8_all]) if k8_all else np.zeros(1, np.int32)).astype(np.int32)
        objs_h = np.concatenate([objs, ksz[:, None]], axis=1).astype(np.int32).reshape(-1)
        blob = np.concatenate([kf_h.astype(np.float64).view(np.uint8), bounds_h.view(np.uint8), k8_h.view(np.uint8),
                               objs_h.view(np.uint8)])
        blob_d = torch.from_numpy(blob).pin_memory().to(dev, non_blocking=True)
        o0 = kf_h.size * 8
        o1 = o0 + bounds_h.size * 4
        o2 = o1 + k8_h.size * 4
        kf_d = blob_d[:o0].view(torch.float64)
        bounds_d = blob_d[o0:o1].view(torch.int32)
        k8_d = blob_d[o1:o2].view(torch.int32)
        objs_d = blob_d[o2:].view(torch.int32)
        check(lib().sdn_composite_frame(ptr(masks_c), ptr(normals_c), ptr(depth_c), ptr(zooms_d), n, R, ptr(objs_d),
                                        len(run), ptr(bounds_d), ptr(k8_d), ptr(kf_d), height, width, ptr(inst),
                                        ptr(nrm), ptr(dep), stream()))

    run = []
    for i in order:
        if interests_h[i]:
            run.append(i)
        elif image_masks is not None:
            flush(run)
            run = []
            m = image_masks[i].to(dev)
            inst = (1 - m) * inst + m * (1 + i)
    flush(run)
    return inst, nrm, dep, order


def frame_json(order, interests, class_ids, depths, alphas, metas=None):
    """The NNNNN.json record of main.py:549-559: {object id: {class_id, depth, alpha, ...meta}} for interesting objects."""
    out = {}
    for i in order:
        if bool(interests[i]):
            rec = {'class_id': int(class_ids[i]), 'depth': float(depths[i]), 'alpha': float(alphas[i])}
            if metas is not None:
                rec.update(metas[i])
            out[i + 1] = rec
    return out


def wire_tensors(instance_map, normal_map, depth_map):
    """The pixel values of the wire format (main.py:604-622) as tensors on the maps' device: instance ids uint8 [1,H,W],
    normal uint8 [3,H,W] = trunc(255 n), depth int32 [1,H,W] = trunc(65535 d) (a 16-bit PNG).  These are exactly what
    write_frame stores, so the textural input assembly (textural/data/assemble.py) can consume them without the PNG round
    trip."""
    inst = instance_map.detach().to(torch.uint8)
    nrm = normal_map.detach().mul(255).to(torch.uint8)
    d16 = (depth_map.detach() * 65535).to(torch.int32)
    return inst, nrm, d16


def write_frame(image_dir, name, instance_map, normal_map, depth_map, json_obj):
    """The wire format to the textural branch (main.py:604-622): NNNNN.json, NNNNN.png (uint8 instance ids),
    NNNNN-normal.png (RGB, trunc(255 n)), NNNNN-depth.png (16 bit, trunc(65535 d)).  Host I/O through PIL."""
    import PIL.Image
    with open(os.path.join(image_dir, '%s.json' % name), 'w') as f:
        json.dump(json_obj, f, indent=4)
    inst_t, nrm_t, d16_t = wire_tensors(instance_map, normal_map, depth_map)
    inst = inst_t.cpu().numpy().transpose(1, 2, 0)
    PIL.Image.fromarray(inst[:, :, 0], mode='L').save(os.path.join(image_dir, '%s.png' % name))
    nrm = nrm_t.cpu().numpy().transpose(1, 2, 0)
    PIL.Image.fromarray(nrm, mode='RGB').save(os.path.join(image_dir, '%s-normal.png' % name))
    d16 = np.uint16(d16_t.cpu().numpy().transpose(1, 2, 0))
    pil = PIL.Image.new('I', d16.T.shape[1:])
    pil.frombytes(d16.tobytes(), 'raw', 'I;16')
    pil.save(os.path.join(image_dir, '%s-depth.png' % name))
