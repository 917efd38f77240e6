"""Shared by tests/test_cityscapes_gt_golden.py (CPU) and tests/test_gpu_cityscapes_gt.py: the fixture and a numpy emulation of
sdn_scene_id_stats / sdn_scene_id_planes (csrc/scene_ids.hip) in the kernels' own integer algorithm -- the id range test per
pixel, the 256-bin histogram of the high byte, the ranks i = 19 (n - 1) / 20 and min(i + 1, n - 1) located in it, the
low-byte histograms of the one or two target bins -- never a sort."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cityscapes_gt_golden.npz')
CASES = ('a', 'b', 'c')
INT_MAX = 2 ** 31 - 1


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def maps(g, tag):
    """the fixture's inputs as the kernels take them: (scene, disparity) int32 [H, W]"""
    return g[tag + '_scene'].astype(np.int32), g[tag + '_disparity'].astype(np.int32)


def planes(g, tag, what):
    """the fixture's packed reference planes -> uint8 [K, 1, H, W]; what: 'masks' or 'ignores'; all objects, ascending ids"""
    H, W = g[tag + '_scene'].shape
    n = len(g[tag + '_ids'])
    return np.unpackbits(g['%s_%s_bits' % (tag, what)])[:n * H * W].reshape(n, 1, H, W)


def find_rank(hist, rank):
    """(bin, rank inside the bin) of the element of zero-based rank `rank` in a histogram, as k_ids_select / k_ids_pick scan it
    (for sdn_scene_id_stats and sdn_train_id_stats alike)"""
    incl = np.cumsum(hist.astype(np.int64))
    b = int(np.searchsorted(incl, rank, side='right'))
    assert b < len(hist), 'rank beyond the histogram'
    return b, int(rank - (incl[b] - hist[b]))


def integer_rank(n):
    """floor((n - 1) 0.95) as the device derives it"""
    return (19 * (n - 1)) // 20


def stats_emulated(scene, disparity, category=26):
    """sdn_scene_id_stats on the host -> int32 [1000, 8]: (area, y0, x0, y1, x1, n, lo, hi) per j = id - 1000 category"""
    scene, disparity = np.asarray(scene, np.int64), np.asarray(disparity, np.int64)
    table = np.zeros((1000, 8), np.int32)
    table[:, 1:3] = INT_MAX
    j_map = scene - 1000 * category
    inside = (j_map >= 0) & (j_map < 1000)
    for j in np.unique(j_map[inside]).tolist():
        m = j_map == j
        ys, xs = np.nonzero(m)
        table[j, :5] = (m.sum(), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
        d = disparity[m]
        d = d[d != 0]
        n = int(d.size)
        table[j, 5] = n
        if n == 0:
            continue
        hist_hi = np.bincount((d >> 8) & 255, minlength=256)                    # pass A
        i = integer_rank(n)
        i1 = min(i + 1, n - 1)
        (bin_i, res_i), (bin_i1, res_i1) = find_rank(hist_hi, i), find_rank(hist_hi, i1)
        lo_hist = [np.bincount(d[((d >> 8) & 255) == b] & 255, minlength=256) for b in (bin_i, bin_i1)]   # pass B
        table[j, 6] = (bin_i << 8) | find_rank(lo_hist[0], res_i)[0]
        table[j, 7] = (bin_i1 << 8) | find_rank(lo_hist[1], res_i1)[0]
    return table


def planes_emulated(scene, disparity, ids, thr):
    """sdn_scene_id_planes on the host -> (masks uint8 [n, 1, H, W], ignores uint8 [n, 1, H, W], cover uint32 [ceil(n / 32), H, W])"""
    scene, disparity = np.asarray(scene), np.asarray(disparity)
    n = len(ids)
    masks = np.stack([(scene == i)[None] for i in ids]).astype(np.uint8)
    ignores = np.stack([(disparity > t)[None] for t in thr]).astype(np.uint8)
    cover = np.zeros(((n + 31) // 32,) + scene.shape, np.uint32)
    for k in range(n):
        cover[k // 32] |= ignores[k, 0].astype(np.uint32) << np.uint32(k & 31)
    return masks, ignores, cover


def select_emulated(table, category=26, max_objects=16):
    """the host step of derender3d.scene.cityscapes_gt_inputs, restated: present ids ascending, the largest first"""
    from derender3d import scene as sc
    from maskrcnn import detections as det
    present = np.flatnonzero(table[:, 0] > 0)
    sels = det.select_largest(table[present, 0].astype(np.float32), max_objects)
    rows = table[present[sels]]
    return sels, (present[sels] + 1000 * category).astype(np.int32), rows[:, 1:5], rows[:, 0], \
        sc.percentile95_threshold(rows[:, 5], rows[:, 6], rows[:, 7])


def big_frame(seed=7, H=1024, W=2048, cars=20):
    """a seeded frame of the real size: elliptical cars (the largest about 10^5 pixels) whose disparities cluster around a
    per-car level, road and sky of other categories, holes of disparity 0 -> (scene, disparity) int32"""
    rng = np.random.default_rng(seed)
    scene = np.full((H, W), 7, np.int32)
    scene[:H // 3] = 23
    disparity = rng.integers(0, 6000, (H, W)).astype(np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(cars):
        ry, rx = (170, 190) if k == 0 else (int(rng.integers(8, 90)), int(rng.integers(10, 140)))
        cy, cx = int(rng.integers(ry, H - ry)), int(rng.integers(rx, W - rx))
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        scene[m] = 26000 + (k if k < cars - 1 else 999)
        level = int(rng.integers(300, 30000))
        disparity[m] = np.clip(level + rng.normal(0, 0.02 * level + 3, int(m.sum())), 1, 65535).astype(np.int32)
    scene[H - 40:H - 30, 100:400] = 24003
    scene[H - 30:H - 20, 100:400] = 27001
    scene[5, 5] = 26
    disparity[rng.random((H, W)) < 0.03] = 0
    return scene, disparity


class Camera:
    def __init__(self, focal, u0, v0):
        self.focal, self.u0, self.v0 = focal, u0, v0
