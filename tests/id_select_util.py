"""Shared by tests/test_id_select_cases_host.py (CPU) and tests/test_gpu_id_select_edges.py: a plain reference of the
order-statistic selects (sdn_scene_id_stats in csrc/scene_ids.hip, sdn_train_id_stats in csrc/train_hybrid.hip), the constructed
inputs that drive every path of their kernels, and a census of what an input contains.

The reference is a sort: np.unique over the id map, a boolean mask per id, np.nonzero for the roi, np.sort of the non-zero
disparities under the mask and two indexings.  No histogram and no rank search, so it shares no step with the kernels or with
cityscapes_util.stats_emulated.  Everything here is numpy on the host; nothing comes from a kernel."""
import numpy as np

INT_MAX = 2 ** 31 - 1
INT_MIN = -2 ** 31
OBJS, COLS = 1000, 8          # the table: one row per id of the category; area, y0, x0, y1, x1, n, lo, hi
ID_CHUNK = 2048               # csrc/scene_ids.hip: ID_CHUNK = ID_THREADS * ID_ITERS, the consecutive pixels of one workgroup
WAVE = 64                     # the wave size of gfx950: the lanes of a wave hold 64 consecutive pixels of a chunk
ID_SLOTS = 16                 # csrc/scene_ids.hip: ID_SLOTS, the objects a workgroup aggregates in LDS
MAX_CATEGORY = INT_MAX // 1000 - 1   # the largest category sdn_scene_id_stats accepts
BACKGROUND = 7                # an id of no category that a test reads


# ---------------------------------------------------------------------------------------------------- the plain reference
def _row(mask, disparity):
    """(area, y0, x0, y1, x1, n, lo, hi) of one boolean mask with at least one pixel set: by a sort"""
    ys, xs = np.nonzero(mask)
    d = disparity[mask]
    v = np.sort(d[d != 0])
    n = int(v.size)
    lo = hi = 0
    if n:
        i = (19 * (n - 1)) // 20
        lo, hi = int(v[i]), int(v[min(i + 1, n - 1)])
    return int(mask.sum()), int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1, n, lo, hi


def plain_stats(scene, disparity, category=26):
    """int32 [1000, 8]: row j = id - 1000 category is (area, roi as mask_to_roi, n, lo, hi); an absent id has area 0 and the
    invalid roi (INT_MAX, INT_MAX, 0, 0)"""
    scene, disparity = np.asarray(scene, np.int64), np.asarray(disparity, np.int64)
    table = np.zeros((OBJS, COLS), np.int32)
    table[:, 1:3] = INT_MAX
    first = 1000 * int(category)
    for v in np.unique(scene).tolist():
        if first <= v < first + OBJS:
            table[v - first] = _row(scene == v, disparity)
    return table


def plain_item_row(scene, disparity, obj_id):
    """one row of sdn_train_id_stats: the item (map, id); disparity None: a frame without a disparity map (n = 0)"""
    scene = np.asarray(scene, np.int64)
    mask = scene == int(obj_id)
    if not mask.any():
        return np.array([0, INT_MAX, INT_MAX, 0, 0, 0, 0, 0], np.int32)
    disparity = np.zeros_like(scene) if disparity is None else np.asarray(disparity, np.int64)
    return np.array(_row(mask, disparity), np.int32)


def plain_thresholds(scene, disparity, category=26):
    """int32 [1000]: floor(np.percentile(d[d != 0], 95)) of every id's disparities, 0 where it has no non-zero value"""
    scene, disparity = np.asarray(scene, np.int64), np.asarray(disparity, np.int64)
    thr = np.zeros(OBJS, np.int32)
    first = 1000 * int(category)
    for v in np.unique(scene).tolist():
        if first <= v < first + OBJS:
            d = disparity[scene == v]
            d = d[d != 0]
            if d.size:
                thr[v - first] = int(np.floor(np.percentile(d, 95)))
    return thr


# ---------------------------------------------------------------------------------------------------- the census
def census(scene, disparity, category=26):
    """What an input holds, from the input and plain_stats alone.  Objects are the ids of the category.
      most_per_chunk / fewest_per_chunk   distinct objects in a 2048-pixel chunk of the flat map (a workgroup's pixels)
      most_per_run / fewest_per_run       distinct objects in an aligned run of 64 pixels (a wave's pixels)
      n0, n1                              objects with n == 0, n == 1
      tied                                objects with n >= 2 and lo == hi
      same_bin                            objects with lo != hi in one high-byte bin
      straddling                          objects with lo >> 8 != hi >> 8 (the second low-byte histogram)
      ns                                  the set of n over the present objects"""
    flat = np.asarray(scene, np.int64).reshape(-1) - 1000 * int(category)
    flat = np.where((flat >= 0) & (flat < OBJS), flat, -1)

    def distinct(step):
        return [len(set(flat[p:p + step].tolist()) - {-1}) for p in range(0, flat.size, step)]

    per_chunk, per_run = distinct(ID_CHUNK), distinct(WAVE)
    t = plain_stats(scene, disparity, category)
    t = t[t[:, 0] > 0]
    n, lo, hi = t[:, 5], t[:, 6], t[:, 7]
    return {'objects': int(len(t)), 'most_per_chunk': max(per_chunk), 'fewest_per_chunk': min(per_chunk),
            'most_per_run': max(per_run), 'fewest_per_run': min(per_run),
            'n0': int((n == 0).sum()), 'n1': int((n == 1).sum()), 'tied': int(((n >= 2) & (lo == hi)).sum()),
            'same_bin': int(((lo != hi) & (lo >> 8 == hi >> 8)).sum()), 'straddling': int((lo >> 8 != hi >> 8).sum()),
            'ns': set(n.tolist())}


# ---------------------------------------------------------------------------------------------------- the cases
def _scatter(objects, W, rng, spare=40):
    """objects: [(id, values)] -> (scene, disparity) int32 [H, W]: every object's values on pixels drawn in shuffled order, the
    rest background with random disparities (which nothing may count)"""
    total = sum(len(v) for _, v in objects) + spare
    H = -(-total // W)
    scene = np.full(H * W, BACKGROUND, np.int32)
    disparity = rng.integers(0, 65536, H * W).astype(np.int32)
    order = rng.permutation(H * W)
    at = 0
    for obj_id, values in objects:
        px = order[at:at + len(values)]
        scene[px] = obj_id
        disparity[px] = values
        at += len(values)
    return scene.reshape(H, W), disparity.reshape(H, W)


def crowd():
    """24 x 96 (two chunks: 2048 and 256 pixels); id 26000 + j with j = (7 x + 13 y) % 40, j = 39 replaced by 999; disparity
    uniform in 0 .. 65535 with about 20 % zeros; one pixel each of 65535 and 65534.  All 40 objects in either chunk and at
    least 37 in every run of 64 pixels: 24 of them find no LDS slot and add to global memory; nearly every object has its two
    order statistics in different high-byte bins."""
    rng = np.random.default_rng(11)
    H, W = 24, 96
    yy, xx = np.mgrid[0:H, 0:W]
    j = (7 * xx + 13 * yy) % 40
    scene = (26000 + np.where(j == 39, 999, j)).astype(np.int32)
    disparity = rng.integers(0, 65536, (H, W)).astype(np.int32)
    disparity[rng.random((H, W)) < 0.2] = 0
    disparity[3, 5], disparity[20, 90] = 65535, 65534
    return scene, disparity, 26


RANK_NS = (1, 2, 3, 19, 20, 21, 22, 40, 41, 42, 61, 101)


def ranks():
    """width 71 (odd); one object per n in RANK_NS, id 26000 + 7 k; its non-zero values pairwise distinct (so a rank off by
    one gives another lo or hi), over the whole range for even k and inside three neighbouring high-byte bins for odd k;
    1 + k % 4 zeros under the same mask (area != n); pixels in shuffled order."""
    rng = np.random.default_rng(12)
    objects = []
    for k, n in enumerate(RANK_NS):
        if k % 2 == 0:
            values = rng.choice(65535, n, replace=False) + 1
        else:
            values = 256 * int(rng.integers(1, 250)) + rng.choice(768, n, replace=False)
        objects.append((26000 + 7 * k, np.concatenate([values, np.zeros(1 + k % 4, np.int64)])))
    return _scatter(objects, 71, rng) + (26,)


# id -> (what, lo, hi) of the `bins` case; n is chosen so that the ranks i and i + 1 fall on the stated values
BINS = {26100: ('all 1', 1, 1), 26101: ('all 256', 256, 256), 26102: ('all 65535', 65535, 65535),
        26103: ('lo and hi inside a run of five ties', 0x5A5A, 0x5A5A), 26104: ('adjacent low bytes in one bin', 0x2010, 0x2011),
        26105: ('adjacent bins', 0x12FF, 0x1300), 26106: ('bins 0 and 255', 255, 65535),
        26107: ('300 pixels, one non-zero', 4660, 4660), 26108: ('only zeros', 0, 0)}


def bins():
    """width 53; one object per value pattern of BINS, pixels in shuffled order:
      all values equal: 1 (n = 5), 256 (n = 7), 65535 (n = 30)
      n = 40, ranks 37 and 38 inside the five ties 0x5A5A at ranks 35 .. 39
      n = 21, ranks 19 and 20 are 0x2010 and 0x2011, five smaller values in the same bin
      n = 41, ranks 38 and 39 are 0x12FF and 0x1300, ties on either side
      n = 20, ranks 18 and 19 are 255 and 65535
      300 pixels with a single non-zero value (n = 1); 50 pixels of zeros (n = 0: lo = hi = 0, threshold 0)"""
    rng = np.random.default_rng(13)
    z = lambda k: np.zeros(k, np.int64)
    objects = [
        (26100, np.concatenate([np.full(5, 1), z(2)])),
        (26101, np.concatenate([np.full(7, 256), z(1)])),
        (26102, np.concatenate([np.full(30, 65535), z(3)])),
        (26103, np.concatenate([rng.choice(0x5A00, 35, replace=False) + 1, np.full(5, 0x5A5A), z(4)])),
        (26104, np.concatenate([rng.choice(0x1F00, 14, replace=False) + 1, [0x2001, 0x2003, 0x2003, 0x2007, 0x200F, 0x2010, 0x2011],
                                z(2)])),
        (26105, np.concatenate([rng.choice(0x1200, 34, replace=False) + 1, [0x12F0, 0x12FE, 0x12FE, 0x12FF, 0x12FF, 0x1300, 0x1300],
                                z(5)])),
        (26106, np.concatenate([rng.integers(1, 255, 18), [255, 65535], z(1)])),
        (26107, np.concatenate([[4660], z(299)])),
        (26108, z(50)),
    ]
    return _scatter(objects, 53, rng) + (26,)


EDGE_IDS = (25999, 26000, 26999, 27000, 26, 0, -1, INT_MIN, INT_MAX, 1000 * MAX_CATEGORY, 1000 * MAX_CATEGORY + 999)


def edges_of_the_category(category=26):
    """9 x 23; the ids of EDGE_IDS in one map, 12 to 22 pixels each with random disparities: the two ids around either end of
    category 26, a bare 26, 0, -1, INT32_MIN, INT32_MAX and both ends of the largest category.  Read with category 26 (objects
    0 and 999), 0 (objects 0 and 26, and the background's 7) and MAX_CATEGORY (objects 0 and 999; INT32_MAX lies above its range): only ids inside
    [1000 c, 1000 c + 1000) are counted."""
    rng = np.random.default_rng(14)
    objects = []
    for k, obj_id in enumerate(EDGE_IDS):
        values = rng.integers(1, 65536, 12 + k)
        values[rng.random(values.size) < 0.2] = 0
        objects.append((obj_id, values))
    H, W = 9, 23
    scene, disparity = _scatter(objects, W, rng, spare=H * W - sum(len(v) for _, v in objects))
    assert scene.shape == (H, W)
    return scene, disparity, int(category)


SHAPES = ((1, 2047), (1, 2048), (1, 2049), (2049, 1), (3, 1), (2, 1025))


def shapes(H, W):
    """One object set on H x W: where the flat index p has p % 3 != 0 the id 26000 + (5 p) % 7, background elsewhere; 26500 on
    every corner pixel; then the one-pixel object 26999 on the last pixel (which is a corner: 26500 keeps the others, so on a
    map of one row or one column its roi ends one pixel short of the far end, and on 2 x 1025 it spans the map).  SHAPES are
    the five one-dimensional maps around one chunk and of three pixels, and 2 x 1025 for a roi over both axes."""
    rng = np.random.default_rng(15)
    p = np.arange(H * W)
    scene = np.where(p % 3 != 0, 26000 + (5 * p) % 7, BACKGROUND).astype(np.int32).reshape(H, W)
    for y in (0, H - 1):
        for x in (0, W - 1):
            scene[y, x] = 26500
    scene[H - 1, W - 1] = 26999
    disparity = rng.integers(0, 65536, (H, W)).astype(np.int32)
    disparity[rng.random((H, W)) < 0.25] = 0
    disparity[H - 1, W - 1] = 40000
    return scene, disparity, 26


def cases():
    """name -> (scene int32 [H, W], disparity int32 [H, W], category)"""
    out = {'crowd': crowd(), 'ranks': ranks(), 'bins': bins(),
           'edges_of_the_category': edges_of_the_category(26), 'edges_of_the_category@0': edges_of_the_category(0),
           'edges_of_the_category@max': edges_of_the_category(MAX_CATEGORY)}
    for H, W in SHAPES:
        out['shapes@%dx%d' % (H, W)] = shapes(H, W)
    return out


CASE_NAMES = ('crowd', 'ranks', 'bins', 'edges_of_the_category', 'edges_of_the_category@0', 'edges_of_the_category@max') + tuple(
    'shapes@%dx%d' % s for s in SHAPES)


# ---------------------------------------------------------------------------------------------------- the cases as item lists
def item_cases():
    """name -> (maps, records) for derender3d.train_items.id_item_table: maps a list of (scene, disparity) int32 [H, W],
    records a list of (frame index, id, has_disparity).
      single   B = 1: the n = 101 object of `ranks`
      mixed    every case map, a 72 x 96 map of three `crowd`s below each other (four chunks) and a 1 x 1 frame, in one batch:
               every id a map holds, of any category (background, -1, INT32_MIN and INT32_MAX too); per map an absent id and
               an item without a disparity map; the first item of every map twice"""
    c = cases()
    maps, records = [], []
    names = [k for k in CASE_NAMES if not k.startswith('edges_of_the_category@')]     # the same map three times otherwise
    for name in names:
        scene, disparity, _ = c[name]
        maps.append((scene, disparity))
    scene, disparity, _ = c['crowd']
    rng = np.random.default_rng(16)
    tall = rng.integers(0, 65536, (72, 96)).astype(np.int32)
    tall[rng.random(tall.shape) < 0.2] = 0
    maps.append((np.ascontiguousarray(np.tile(scene, (3, 1))), tall))
    maps.append((np.array([[26005]], np.int32), np.array([[777]], np.int32)))
    for f, (scene, _) in enumerate(maps):
        present = np.unique(scene).tolist()
        records += [(f, v, True) for v in present]
        records += [(f, 26777, True), (f, present[-1], False), (f, present[0], True)]
    single = ([c['ranks'][:2]], [(0, 26000 + 7 * RANK_NS.index(101), True)])
    return {'single': single, 'mixed': (maps, records)}
