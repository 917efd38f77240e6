"""Host restatement of the training item of the geometric branch, for the tests of derender3d/train_items.py.

The four colour ops as Pillow computes them (torchvision 0.2.1's adjust_brightness / _contrast / _saturation / _hue call
ImageEnhance.Brightness / Contrast / Color and convert('HSV')), in numpy, statement for statement what csrc/train_items.hip
holds for the device: fp32 where Pillow's C uses float, float64 where a double literal promotes the expression.
tests/test_geo_train_items.py pins every function here against the installed Pillow."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'geo_train_golden.npz')

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
OPS = ('brightness', 'contrast', 'saturation', 'hue')

TARGET_KEYS = ('rois', 'roi_norms', 'thetas', 'rotations', 'translations', 'translation2ds', 'scales', 'log_scales', 'log_depths',
               'widths', 'heights', 'focals', 'u0s', 'v0s', 'targets')
# the entries whose value passes through numpy's log / cos / sin (datasets.py:367, 376, 379-383)
LIBM_KEYS = ('rotations', 'log_scales', 'log_depths')


def blend(deg, img, alpha):
    """Image.blend(deg, img, alpha) on uint8 arrays (Blend.c): deg + alpha (img - deg) in fp32; truncated for alpha in
    [0, 1], clipped outside"""
    a = np.float32(alpha)
    d, v = deg.astype(np.int32), img.astype(np.int32)
    t = d.astype(np.float32) + a * (v - d).astype(np.float32)
    if 0.0 <= a <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def luma(rgb):
    """convert('L') of uint8 [..., 3] (Convert.c: L24 >> 16)"""
    c = rgb.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16).astype(np.uint8)


def _round(x):
    """C's round() of non-negative float64: half away from zero, without forming x + 0.5"""
    f = np.floor(x)
    return (f + ((x - f) >= 0.5)).astype(np.int64)


def rgb_to_hsv(rgb):
    """convert('HSV') of uint8 [..., 3] (Convert.c: rgb2hsv_row)"""
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    with np.errstate(divide='ignore', invalid='ignore'):
        cr = (maxc - minc).astype(np.float32)
        s = cr / maxc.astype(np.float32)
        rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32),
                              (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32))).astype(np.float32)
        t = h.astype(np.float64) / 6.0 + 1.0
        t = np.where(t >= 1.0, t - 1.0, t)          # fmod(t, 1.0) for t in [5/6, 11/6]
        h = t.astype(np.float32)
        uh = np.clip(np.nan_to_num(h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip(np.nan_to_num(s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    uh, us = np.where(grey, 0, uh), np.where(grey, 0, us)
    return np.stack([uh, us, maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """convert('RGB') of a uint8 [..., 3] HSV image (Convert.c: hsv2rgb)"""
    h, s, v = (hsv[..., k].astype(np.float32) for k in range(3))
    h6 = h.astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32)
    fs = (s.astype(np.float64) / 255.0).astype(np.float32)
    vd = v.astype(np.float64)
    p = np.clip(_round(vd * (1.0 - fs.astype(np.float64))), 0, 255)
    q = np.clip(_round(vd * (1.0 - (fs * f).astype(np.float64))), 0, 255)
    t = np.clip(_round(vd * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))), 0, 255)
    vi = hsv[..., 2].astype(np.int64)
    sel = i % 6
    r = np.choose(sel, [vi, q, p, p, t, vi])
    g = np.choose(sel, [t, vi, vi, q, p, p])
    b = np.choose(sel, [p, p, t, vi, vi, q])
    grey = hsv[..., 1] == 0
    return np.stack([np.where(grey, vi, r), np.where(grey, vi, g), np.where(grey, vi, b)], axis=-1).astype(np.uint8)


def contrast_grey(lsum, n):
    """int(mean(L) + 0.5) in integers: (2 sum + n) // (2 n)"""
    return int((2 * int(lsum) + int(n)) // (2 * int(n)))


def color_jitter(rgb, order, factors, hue_shift):
    """the ops of `order` on a uint8 [s, s, 3] crop, as torchvision 0.2.1's ColorJitter applies drawn parameters"""
    out = np.ascontiguousarray(rgb).copy()
    for op in order:
        if op == BRIGHTNESS:
            out = blend(np.zeros_like(out), out, factors[0])
        elif op == CONTRAST:
            l = luma(out)
            grey = contrast_grey(l.astype(np.int64).sum(), l.size)
            out = blend(np.full_like(out, grey), out, factors[1])
        elif op == SATURATION:
            out = blend(np.repeat(luma(out)[..., None], 3, axis=-1), out, factors[2])
        elif op == HUE:
            hsv = rgb_to_hsv(out)
            hsv[..., 0] = hsv[..., 0] + np.uint8(hue_shift)     # uint8 addition wraps
            out = hsv_to_rgb(hsv)
        else:
            raise ValueError('op %r' % (op,))
    return out


_golden = None


def golden():
    """the fixture, loaded once and shared (read-only)"""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN, allow_pickle=False)
        _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def item_order(g, i, tag='t'):
    """the ops of item i of batch `tag` as a list"""
    return [int(o) for o in g[tag + '_order'][i][:int(g[tag + '_nops'][i])]]


def window(plane, win, fill):
    """Transforms.crop_square's s x s window of a [H, W] or [H, W, C] uint8 plane from derender3d.scene.crop_windows' row: `fill`
    outside the frame, 0 beyond the padded image (the quirk column / row)"""
    oy, ox, s, xlim, ylim = (int(v) for v in win)
    Hh, Ww = plane.shape[:2]
    fy, fx = np.meshgrid(oy + np.arange(s), ox + np.arange(s), indexing='ij')
    inside = (fy >= 0) & (fy < Hh) & (fx >= 0) & (fx < Ww)
    out = np.full((s, s) + plane.shape[2:], fill, dtype=np.uint8)
    out[inside] = plane[fy[inside], fx[inside]]
    out[(fx >= xlim) | (fy >= ylim)] = 0
    return out


def host_item(frame_rgb, scene, code, nearer_codes, roi, order, factors, hue_shift, mean, std, image_size=224, mask_size=256):
    """one item's (image, mask, ignore) on the host from the restated pieces: window, colour ops, Pillow's resize tables
    (derender3d.compositing.resample_u8_numpy), to_tensor, Normalize in fp32"""
    from derender3d import compositing as comp
    from derender3d import scene as sc
    Hh, Ww = scene.shape[:2]
    win = sc.crop_windows([roi], Hh, Ww)[0]
    rgb = color_jitter(window(frame_rgb, win, 127), order, factors, hue_shift)
    image = np.stack([comp.resample_u8_numpy(rgb[..., c], image_size) for c in range(3)])
    image = image.astype(np.float32) / np.float32(255)
    image = (image - np.float32(mean)[:, None, None]) / np.float32(std)[:, None, None]
    own = np.all(scene == np.asarray(code, np.uint8), axis=2)
    count = np.zeros(scene.shape[:2], np.int64)
    for c in nearer_codes:
        count += np.all(scene == np.asarray(c, np.uint8), axis=2)
    planes = []
    for plane, fill in ((np.uint8(255) * own.astype(np.uint8), 0), (((255 * count) & 255).astype(np.uint8), 255)):
        planes.append(comp.resample_u8_numpy(window(plane, win, fill), mask_size).astype(np.float32)[None] / np.float32(255))
    return image, planes[0], planes[1]


def batch_items(g, tag):
    """the fixture's batch `tag` ('t': training, 'e': is_train False) as the arguments of train_batch: (frames uint8
    [Fr, 3, H, W], scenes uint8 [Fr, H, W, 3], items, jitter, rois) in numpy"""
    from derender3d import train_items as ti
    p = tag + '_'
    frames = np.ascontiguousarray(g[p + 'frames'].transpose(0, 3, 1, 2))
    items = []
    for b in range(g[p + 'item_frame'].shape[0]):
        f = int(g[p + 'item_frame'][b])
        rows = g['%sf%d_rows' % (p, f)]
        items.append(ti.Item(f, int(g[p + 'item_index'][b]), {k: rows[:, j] for j, k in enumerate(ti.ROW_KEYS)},
                             g['%sf%d_codes' % (p, f)]))
    jitter = [(item_order(g, b, tag), tuple(float(v) for v in g[p + 'factors'][b]), int(g[p + 'hue_shift'][b]))
              for b in range(len(items))]
    return frames, g[p + 'scenes'], items, jitter, g[p + 'rois_used']
