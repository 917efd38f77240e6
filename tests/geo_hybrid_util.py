"""The fixture of the hybrid training items (tests/golden/make_geo_hybrid_golden.py) as the arguments of
derender3d.train_items.hybrid_batch, and the host emulation of one mixed item on top of tests/geo_train_util.py."""
import os

import numpy as np

import geo_train_util as u

GOLDEN = os.path.join(u.HERE, 'golden', 'geo_hybrid_golden.npz')
VK, KO, KS, CS, MR = range(5)
FLOAT_KEYS = ('rois', 'roi_norms', 'thetas', 'rotations', 'translations', 'translation2ds', 'scales', 'log_scales', 'log_depths',
              'widths', 'heights', 'focals', 'u0s', 'v0s')
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


def batch_tags(g):
    return [str(t) for t in g['batches']]


def frame_arrays(g, key):
    """{rgb [H, W, 3] uint8, scene | ids | disp} of one frame of the fixture"""
    pre = 'F_%s_' % key
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def host_items(g, tag):
    """(frame keys, items, jitter, rois, is_train) of batch `tag`; the items name their frame by index into the keys"""
    from derender3d import train_items as ti
    p = tag + '_'
    keys = [str(k) for k in g[p + 'frame_keys']]
    items = []
    for b, kind in enumerate(g[p + 'kind']):
        f, d = int(g[p + 'item_frame'][b]), g[p + 'data'][b]
        if kind == VK:
            rows = g[keys[f] + '_rows']
            items.append(ti.Item(f, int(g[p + 'obj'][b]), {k: rows[:, j] for j, k in enumerate(ti.ROW_KEYS)}, g[keys[f] + '_codes']))
        elif kind == KO:
            items.append(ti.KittiObjectItem(f, d[:11], d[11:14]))
        elif kind == KS:
            items.append(ti.KittiSemanticsItem(f, int(g[p + 'obj'][b]), d[:4].astype(np.int64)))
        elif kind == CS:
            items.append(ti.CityscapesItem(f, int(g[p + 'obj'][b])))
        else:
            items.append(ti.MaskItem(f, int(g[p + 'obj'][b]), d[:4].astype(np.int64), d[4:7]))
    jitter = [(u.item_order(g, b, tag), tuple(float(v) for v in g[p + 'factors'][b]), int(g[p + 'hue_shift'][b])) for b in range(len(items))]
    return keys, items, jitter, g[p + 'rois_used'], bool(g[p + 'is_train'])


def device_frames(g, keys):
    """the SourceFrames of the frame keys on the GPU"""
    import torch
    from derender3d import train_items as ti
    out = []
    for key in keys:
        a = frame_arrays(g, key)
        t = lambda x, dt: None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=dt).cuda()
        out.append(ti.SourceFrame(t(a['rgb'].transpose(2, 0, 1), torch.uint8), t(a.get('scene'), torch.uint8), t(a.get('ids'), torch.int32),
                                  t(a.get('disp'), torch.int32)))
    return out


def order_statistics(values):
    """(n, lo, hi) of the non-zero values: rank floor(0.95 (n - 1)) and the next, as sdn_train_id_stats defines them"""
    v = np.sort(values[values != 0])
    n = v.size
    if not n:
        return 0, 0, 0
    i = (19 * (n - 1)) // 20
    return n, int(v[i]), int(v[min(i + 1, n - 1)])


def host_mixed_item(g, tag, b, item, frame, roi, jitter):
    """(image, mask | None, ignore | None) of item b on the host: geo_train_util's window, colour ops and Pillow's tables with
    the item's own frame, sources and normalisation"""
    from derender3d import compositing as comp
    from derender3d import scene as sc
    from derender3d import train_items as ti
    kind = int(g[tag + '_kind'][b])
    rgb = frame['rgb']
    Hh, Ww = rgb.shape[:2]
    win = sc.crop_windows([roi], Hh, Ww)[0]
    mean, std = (ti.VKITTI_MEAN, ti.VKITTI_STD) if kind == VK else (ti.IMAGENET_MEAN, ti.IMAGENET_STD)
    crop = u.color_jitter(u.window(rgb, win, 127), *jitter)
    image = np.stack([comp.resample_u8_numpy(crop[..., c], 224) for c in range(3)]).astype(np.float32) / np.float32(255)
    image = (image - np.float32(mean)[:, None, None]) / np.float32(std)[:, None, None]
    if kind == KO:
        return image, None, None
    plane = lambda p, fill: comp.resample_u8_numpy(u.window(p, win, fill), 256).astype(np.float32)[None] / np.float32(255)
    zeros = np.zeros((1, 256, 256), np.float32)
    if kind == VK:
        scene = frame['scene']
        own = np.all(scene == item.code, axis=2)
        count = np.zeros(scene.shape[:2], np.int64)
        for c in item.codes[ti.nearer_objects(item.rows, item.index)]:
            count += np.all(scene == c, axis=2)
        return image, plane(np.uint8(255) * own.astype(np.uint8), 0), plane(((255 * count) & 255).astype(np.uint8), 255)
    own = frame['ids'] == item.obj_index
    mask = plane(np.uint8(255) * own.astype(np.uint8), 0)
    if kind != CS:
        return image, mask, zeros
    n, lo, hi = order_statistics(frame['disp'][own])
    thr = int(sc.percentile95_threshold([n], [lo], [hi])[0])
    return image, mask, plane(np.uint8(255) * (frame['disp'] > thr).astype(np.uint8), 255)
