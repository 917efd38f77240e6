"""Shared by tests/test_detections_golden.py (CPU) and tests/test_gpu_detections.py: the fixture and a numpy emulation of
sdn_unmold_masks / sdn_scene_gt_masks (csrc/scene_masks.hip), step for step: bytescale in float32, Pillow's two passes from
compositing.resample_tables / fixed_point (the integer sums of compositing.resample_u8_numpy, for a rectangle), >= 128, paste."""
import os

import numpy as np

from derender3d import compositing as comp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'detections_golden.npz')


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def planes(g, tag):
    """the fixture's packed masks -> uint8 [N, 1, H, W]"""
    H, W = g[tag + '_image_shape'][:2] if tag + '_image_shape' in g else g[tag + '_scene'].shape[:2]
    n = len(g[tag + '_areas'])
    return np.unpackbits(g[tag + '_masks_bits'])[:n * H * W].reshape(n, 1, H, W)


def bytescale_f32(plane):
    """scipy 1.0.1 misc/pilutil.py bytescale as numpy 1.14 evaluates it on a float32 array: the float64 scalar 255.0 / cscale
    is rounded to float32 and every array operation is a float32 operation (numpy 2.x would promote to float64)"""
    plane = np.asarray(plane)
    assert plane.dtype == np.float32
    cmin, cmax = plane.min(), plane.max()
    cscale = np.float32(cmax - cmin)
    if cscale == 0:
        cscale = np.float32(1)
    scale = np.float32(255.0 / float(cscale))
    t = (plane - cmin) * scale + np.float32(0)
    t = np.minimum(np.maximum(t, np.float32(0)), np.float32(255)) + np.float32(0.5)
    assert t.dtype == np.float32
    return t.astype(np.uint8)


def resample_u8_rect(img, out_h, out_w):
    """ImagingResample on an 8-bit [h, w] image to [out_h, out_w]: horizontal pass first, rounded to uint8, then vertical; a
    pass whose sizes are equal is skipped (the sums of compositing.resample_u8_numpy, which is square only)"""
    half = 1 << (comp.PRECISION_BITS - 1)
    cur = img.astype(np.int64)
    if out_w != img.shape[1]:
        _, bounds, kk = comp.resample_tables(img.shape[1], out_w)
        k8 = comp.fixed_point(kk).astype(np.int64)
        tmp = np.zeros((cur.shape[0], out_w), np.int64)
        for ox in range(out_w):
            x0, c = bounds[ox]
            tmp[:, ox] = half + (cur[:, x0:x0 + c] * k8[ox, :c]).sum(axis=1)
        cur = np.clip(tmp >> comp.PRECISION_BITS, 0, 255)
    if out_h != img.shape[0]:
        _, bounds, kk = comp.resample_tables(img.shape[0], out_h)
        k8 = comp.fixed_point(kk).astype(np.int64)
        tmp = np.zeros((out_h, cur.shape[1]), np.int64)
        for oy in range(out_h):
            y0, c = bounds[oy]
            tmp[oy] = half + (cur[y0:y0 + c] * k8[oy, :c, None]).sum(axis=0)
        cur = np.clip(tmp >> comp.PRECISION_BITS, 0, 255)
    return cur.astype(np.uint8)


def unmold_emulated(mrcnn_mask, objs, H, W):
    """the kernel on the host: objs int32 [n, >= 6] rows (detection, class, y1, x1, y2, x2) -> (uint8 [n, 1, H, W], areas)"""
    out = np.zeros((len(objs), 1, H, W), np.uint8)
    for i, (d, c, y1, x1, y2, x2) in enumerate(np.asarray(objs)[:, :6].tolist()):
        v = resample_u8_rect(bytescale_f32(mrcnn_mask[d, c]), y2 - y1, x2 - x1)
        out[i, 0, y1:y2, x1:x2] = v >= 128        # (float32)v / 255 >= 0.5
    return out, out.reshape(len(objs), -1).sum(axis=1).astype(np.int32)


def gt_emulated(scene, codes):
    K, (H, W) = len(codes), scene.shape[:2]
    masks = np.zeros((K, 1, H, W), np.uint8)
    rois = np.zeros((K, 4), np.int32)
    for k, code in enumerate(np.asarray(codes)):
        m = (scene == code[None, None, :]).all(axis=2)
        masks[k, 0] = m
        ys, xs = np.nonzero(m)
        rois[k] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1) if ys.size else (2 ** 31 - 1, 2 ** 31 - 1, 0, 0)
    return masks, rois, masks.reshape(K, -1).sum(axis=1).astype(np.int32)


class Camera:
    def __init__(self, focal, u0, v0):
        self.focal, self.u0, self.v0 = focal, u0, v0
