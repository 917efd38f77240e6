"""Shared pieces of the semantic training-batch tests (tests/test_segm_train_host.py, tests/test_gpu_segm_train.py) and of the
fixture's generator (tests/golden/make_segm_train_golden.py): the cases, their seeded inputs and parameters, and a numpy
restatement of semantic/vkitti_dataset.py:111-159 built from the project's own tables (sdn_hip.pillow) and from
tests/geo_train_util.py's colour arithmetic.  The generator makes the expected values with the installed Pillow and torch's CPU
instead; the host test holds the two against each other."""
import hashlib
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import geo_train_util as gu  # noqa: E402

GOLD = os.path.join(HERE, 'golden', 'segm_train_golden.npz')

# the small cases: frames 45 x 150, three items with a table each
SMALL = dict(H=45, W=150, B=3, frame_size=(45, 150), img_max_size=170, padding_constant=8, segm_downsampling_rate=8)
SMALL_SHORTS = (12, 20, 33, 45, 60)   # 9-tap filters; -; h no multiple of 8; no resample; limited by img_max_size, an upscale
# the real-size case: two frames, short sizes 300 and 100 (one batch each), item 1 flipped, four ops with contrast on both
REAL = dict(H=375, W=1242, B=2, frame_size=(375, 1242), img_max_size=1274, padding_constant=8, segm_downsampling_rate=8)
REAL_SHORTS = (300, 100)
REAL_FLIPS = (False, True)
REAL_ROWS_300 = tuple(range(0, 24)) + tuple(range(140, 164)) + tuple(range(276, 300))   # the stored rows of short size 300
DEFAULT_SHORTS = (100, 150, 200, 300, 375)

MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229, 0.224, 0.225)


def digest(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def case_name(short, flip):
    return 's%d%s' % (short, 'f' if flip else 'n')


# ---- inputs, from numpy's frozen RandomState stream --------------------------------------------------------------------------
def _palette(rs, n):
    """n distinct colours"""
    seen = set()
    while len(seen) < n:
        seen.add(tuple(int(v) for v in rs.randint(0, 256, 3)))
    return np.array(sorted(seen), dtype=np.uint8)[rs.permutation(n)]


def _blocky(rs, H, W, cell, colours):
    """[H, W, 3]: cells of `cell` pixels, each one of `colours`"""
    idx = rs.randint(0, len(colours), (-(-H // cell), -(-W // cell)))
    return colours[np.kron(idx, np.ones((cell, cell), dtype=np.int64))[:H, :W]]


def small_inputs():
    """(frames uint8 [3, 45, 150, 3] noise, scenes uint8 [3, 45, 150, 3], tables: 3 (codes [K, 3], labels [K])).  Item 1's
    scene holds a colour outside its table over columns 65 .. 84 (sampled in every case, flipped or not); item 2's holds one
    at (0, 0), which no case samples.  Item 0's table lists an unlabelled colour (label 0)."""
    rs = np.random.RandomState(2101)
    H, W, B = SMALL['H'], SMALL['W'], SMALL['B']
    frames = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    scenes, tables = [], []
    for i in range(B):
        K = (5, 9, 14)[i]
        colours = _palette(rs, K + 1)
        labels = rs.randint(1, 15, K)
        if i == 0:
            labels[2] = 0
        scene = _blocky(rs, H, W, (5, 3, 7)[i], colours[:K])
        if i == 1:
            scene[:, 65:85] = colours[K]
        if i == 2:
            scene[0, 0] = colours[K]
        scenes.append(scene)
        tables.append((colours[:K].copy(), labels.astype(np.int64)))
    return frames, np.stack(scenes).astype(np.uint8), tables


def small_jitters():
    """30 parameter sets, one per (case, item): all 24 orders of the four ops, none, contrast alone, and partial orders.  The
    factors reach beyond [0, 1] so that Image.blend's clipped branch runs too."""
    rs = np.random.RandomState(2102)
    orders = [list(p) for p in itertools.permutations(range(4))] + [None, [1], [3, 0], [2], [1, 3, 2], [0, 1, 2, 3]]
    out = []
    for o in orders:
        factors = tuple(float(v) for v in rs.uniform(0.6, 1.4, 3))
        shift = int(rs.randint(0, 256))
        out.append(None if o is None else (o, factors, shift))
    return out


def small_case(short, flip):
    """(flips, jitters) of the case: its three items take the parameter sets 3 k .. 3 k + 2, k the case's number"""
    k = SMALL_SHORTS.index(short) * 2 + (1 if flip else 0)
    return [bool(flip)] * SMALL['B'], small_jitters()[3 * k:3 * k + 3]


def real_inputs():
    """(frames uint8 [2, 375, 1242, 3]: cells of 6 pixels of 64 colours (the noise is the small cases'), scenes, tables).
    5.6 MB: drawn again from the seed wherever they are needed; the fixture holds their SHA-256."""
    rs = np.random.RandomState(2103)
    H, W, B = REAL['H'], REAL['W'], REAL['B']
    frames, scenes, tables = [], [], []
    for i in range(B):
        frames.append(_blocky(rs, H, W, 6, _palette(rs, 64)))
        colours = _palette(rs, 30)
        scenes.append(_blocky(rs, H, W, 11, colours))
        tables.append((colours, rs.randint(0, 15, 30).astype(np.int64)))
    return np.stack(frames), np.stack(scenes).astype(np.uint8), tables


def real_jitters():
    rs = np.random.RandomState(2104)
    return [([3, 1, 0, 2], tuple(float(v) for v in rs.uniform(0.8, 1.2, 3)), 240),
            ([0, 2, 1, 3], tuple(float(v) for v in rs.uniform(0.8, 1.2, 3)), 17)]


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def _pass(img, n_out, axis):
    """one pass of ImagingResample over `axis` of a uint8 [H, W, C] image: 22-bit coefficients, rounded to bytes"""
    from sdn_hip import pillow
    n_in = img.shape[axis]
    if n_in == n_out:   # Pillow skips the pass
        return img
    ksize, bounds, kk = pillow.resample_tables(n_in, n_out)
    k8 = pillow.fixed_point(kk).astype(np.int64)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.zeros((n_out,) + src.shape[1:], dtype=np.int64)
    for o in range(n_out):
        a, c = bounds[o]
        out[o] = (1 << (pillow.PRECISION_BITS - 1)) + np.tensordot(k8[o, :c], src[a:a + c], axes=(0, 0))
    return np.moveaxis(np.clip(out >> pillow.PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def bilinear_resize(img, h, w):
    """Image.resize((w, h), BILINEAR) of a uint8 [H, W, 3] array: the horizontal pass into bytes, then the vertical"""
    return _pass(_pass(img, w, 1), h, 0)


def host_pixels(frame, jitter, flip, h, w):
    """vkitti_dataset.py:124, :135, :139 on one frame: uint8 [h, w, 3], RGB"""
    img = frame if jitter is None else gu.color_jitter(frame, *jitter)
    if flip:
        img = img[:, ::-1]
    return bilinear_resize(np.ascontiguousarray(img), h, w)


def normalise(px):
    """:152-154 in numpy: fp32 [3, h, w]; output channel c is colour plane 2 - c, less mean[c], over std[c], both rounded to fp32"""
    out = np.empty((3,) + px.shape[:2], dtype=np.float32)
    for c in range(3):
        out[c] = (px[:, :, 2 - c].astype(np.float32) - np.float32(MEAN[c])) / np.float32(STD[c])
    return out


def scene_labels(scene, codes, labels):
    """(label of every scene pixel int64 [H, W], 0 where the colour is unknown; unknown bool [H, W]): the dictionary of :120"""
    table = {tuple(int(v) for v in c): int(l) for c, l in zip(codes, labels)}
    H, W, _ = scene.shape
    lab = np.zeros((H, W), dtype=np.int64)
    unk = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            v = table.get(tuple(int(c) for c in scene[y, x]))
            if v is None:
                unk[y, x] = True
            else:
                lab[y, x] = v
    return lab, unk


def host_batch(frames, scenes, tables, short, flips, jitters, cfg):
    """The batch with the project's host arithmetic: {'sizes', 'Hb', 'Wb', 'px': B uint8 [h, w, 3], 'img_data' fp32
    [B, 3, Hb, Wb], 'seg_label' int64 [B, Hb / rate, Wb / rate], 'unknown' int64 [B]}"""
    from semantic import train_items as st
    rate = cfg['segm_downsampling_rate']
    sizes, Hb, Wb = st.batch_sizes(short, cfg['B'], cfg['img_max_size'], cfg['padding_constant'], rate, cfg['frame_size'])
    B = cfg['B']
    img = np.zeros((B, 3, Hb, Wb), dtype=np.float32)
    lab = np.zeros((B, Hb // rate, Wb // rate), dtype=np.int64)
    unknown = np.zeros(B, dtype=np.int64)
    px = []
    for i in range(B):
        h, w = int(sizes[i, 0]), int(sizes[i, 1])
        px.append(host_pixels(frames[i], jitters[i], flips[i], h, w))
        img[i, :, :h, :w] = normalise(px[-1])
        full, unk = scene_labels(scenes[i], *tables[i])
        lab[i] = st.label_formula(full, h, w, rate, Hb // rate, Wb // rate, flips[i])
        unknown[i] = int((st.label_formula(unk.astype(np.int64), h, w, rate, Hb // rate, Wb // rate, flips[i]) == 0).sum())
    return {'sizes': sizes, 'Hb': Hb, 'Wb': Wb, 'px': px, 'img_data': img, 'seg_label': lab, 'unknown': unknown}


def expected_img(px_list, lut, Hb, Wb):
    """the expected img_data from the fixture's uint8 pixels and its table of torch's CPU normalisation of every byte
    (lut fp32 [3, 256]; the generator proved torch's full result equal to this gather, and stored that result's SHA-256)"""
    out = np.zeros((len(px_list), 3, Hb, Wb), dtype=np.float32)
    for i, px in enumerate(px_list):
        h, w = px.shape[:2]
        for c in range(3):
            out[i, c, :h, :w] = lut[c][px[:, :, 2 - c]]
    return out
