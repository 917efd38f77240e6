"""The training batch of the semantic branch on the device: colour jitter, flip, resize, BGR normalisation, labels and the zero
padding into one batch (reference: semantic/vkitti_dataset.py:74-163, TrainDataset.__getitem__).

    sizes, Hb, Wb = batch_sizes(short_size, B)                       # :83-106, host integers
    short_size, flip, jitter = draw_item([100, 150, 200, 300, 375])  # the host-side draws, one call per item
    out = segm_train_batch(frames_u8, scenes_u8, tables, short_size, flips, jitters)
    out['img_data'], out['seg_label']                                # what the reference's loader hands the network

The reference does all of :111-159 on the host, per item: a Python call per pixel for the label, ColorJitter through Pillow,
cv2.flip, three scipy.misc.imresize calls (Pillow's resize), Normalize, and a copy into the padded batch tensors.  Here the
host prepares Pillow's tables (sdn_hip.pillow) and the item rows, everything goes up in ONE copy, and sdn_segm_train_batch
(csrc/segm_train.hip) does the rest in at most three launches, bit for bit.  The parameters are data: reproducing the
reference's RNG stream is not attempted.

Out of scope: ValDataset / TestDataset (their cv2.resize cannot be pinned), reading files, the DataLoader.

GPU only: CPU tensors raise NotImplementedError; there is no torch form."""
import random

import numpy as np
import torch

from sdn_hip import pillow as _pillow
from sdn_hip.pillow import jitter_params  # noqa: F401  (re-exported: the draw of one item's ColorJitter)

from .segm_tail import color_table

ITEM_INTS = 20      # one row of sdn_segm_train_batch's item table (csrc/segm_train_check.h: SegTrainItem)
STAT_PIXELS = 2048  # SGT_STAT_PIXELS: frame pixels per partial sum of the contrast op
NO_JITTER = ((), (1.0, 1.0, 1.0), 0)
# vkitti_dataset.py:44: Normalize(mean=[0.485 * 255, ...], std=[0.229, ...]) applied AFTER the RGB -> BGR swap of :152
MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229, 0.224, 0.225)


def round2nearest_multiple(x, p):
    """vkitti_dataset.py:17-18: the smallest multiple of p that is >= x."""
    return ((x - 1) // p + 1) * p


def batch_sizes(short_size, batch_per_gpu, img_max_size=1274, padding_constant=8, segm_downsampling_rate=8, frame_size=(375, 1242)):
    """vkitti_dataset.py:91-106, statement for statement: (sizes int32 [B, 2] = every item's resized (height, width), Hb, Wb =
    the batch's height and width).  The scale is min(short_size / min(frame_size), img_max_size / max(frame_size)) in float64,
    the float products are stored into an np.int32 array (truncation), the maxima are rounded up to multiples of
    padding_constant.  frame_size is the pair the reference hard-codes at :93.  ValueError where the reference asserts
    (padding_constant < segm_downsampling_rate)."""
    B = int(batch_per_gpu)
    if B < 1:
        raise ValueError('batch_per_gpu must be at least 1, got %r' % (batch_per_gpu,))
    if padding_constant < segm_downsampling_rate:
        raise ValueError('padding constant must be equal or large than segm downsamping rate (%r < %r)'
                         % (padding_constant, segm_downsampling_rate))
    sizes = np.zeros((B, 2), np.int32)
    for i in range(B):
        img_height, img_width = frame_size
        this_scale = min(short_size / min(img_height, img_width), img_max_size / max(img_height, img_width))
        img_resized_height, img_resized_width = img_height * this_scale, img_width * this_scale
        sizes[i, :] = img_resized_height, img_resized_width
    Hb = int(round2nearest_multiple(np.max(sizes[:, 0]), padding_constant))
    Wb = int(round2nearest_multiple(np.max(sizes[:, 1]), padding_constant))
    return sizes, Hb, Wb


def draw_item(img_sizes, random_flip=True, jitter=(.2, .2, .2, .1), rng=random, nprng=np.random):
    """The host-side draws of one item -> (short_size, flip, jitter): the short size (:84-87, np.random.choice of a list; the
    reference draws it ONCE per batch: a caller that draws per item uses the first item's for the batch), the flip bit (:133)
    and the parameters of ColorJitter(brightness, contrast, saturation, hue) (:46, :124) as sdn_hip.pillow.jitter_params
    returns them: (order, factors, hue_shift).  jitter None: no colour jitter."""
    short_size = int(nprng.choice(img_sizes)) if isinstance(img_sizes, (list, tuple, np.ndarray)) else int(img_sizes)
    flip = bool(nprng.choice([0, 1]) == 1) if random_flip else False
    jit = NO_JITTER if jitter is None else jitter_params(*jitter, rng=rng)
    return short_size, flip, jit


def label_formula(labels_full, h, w, rate, Hl, Wl, flip=False):
    """The composed label gather on the host (numpy): labels_full int [H, W] = the table label of every scene pixel (0:
    unlabelled).  Returns int64 [Hl, Wl]: labels_full[ytab[rate y + rate / 2], flip(xtab[rate x + rate / 2])] - 1 where both
    indices lie inside (h, w), -1 elsewhere -- what :136, :140-150 and :157-159 compute with two Pillow NEAREST calls."""
    H, W = labels_full.shape
    ytab, xtab = _pillow.nearest_table(H, h), _pillow.nearest_table(W, w)
    out = np.full((Hl, Wl), -1, dtype=np.int64)
    sy, sx = rate * np.arange(Hl) + rate // 2, rate * np.arange(Wl) + rate // 2
    oky, okx = sy < h, sx < w
    fy, fx = ytab[sy[oky]], xtab[sx[okx]]
    if flip:
        fx = W - 1 - fx
    out[np.ix_(oky, okx)] = labels_full[np.ix_(fy, fx)].astype(np.int64) - 1
    return out


def _as_tables(tables, B):
    """B sorted colour tables (numpy int32 [2 K], color_table's layout) from one shared table or B (codes, labels) pairs."""
    if isinstance(tables, np.ndarray):
        tables = [tables] * B
    tables = list(tables)
    if len(tables) != B:
        raise ValueError('%d colour tables for %d items' % (len(tables), B))
    out = []
    for t in tables:
        if isinstance(t, np.ndarray) and t.ndim == 1:
            t = np.ascontiguousarray(t, dtype=np.int32)
            if t.size < 2 or t.size % 2:
                raise ValueError('a colour table must be int32 [2 K] with K >= 1, got %s' % (t.shape,))
        else:
            codes, labels = t
            t = color_table(codes, labels)
        out.append(t)
    return out


def table_buffer(sizes, tables, flips, jitters, H, W):
    """The ONE int32 buffer of sdn_segm_train_batch (include/sdn_hip.h): B item rows of ITEM_INTS, then Pillow's bilinear
    bounds and 22-bit coefficients, the NEAREST index tables and the colour tables the rows name, each stored once however
    many items share it."""
    B = len(sizes)
    rows = np.zeros((B, ITEM_INTS), dtype=np.int32)
    rowsf = rows.view(np.float32)
    parts, placed = [], {}
    used = [B * ITEM_INTS]

    def place(key, make):
        if key not in placed:
            a = np.ascontiguousarray(make(), dtype=np.int32).reshape(-1)
            placed[key] = used[0]
            parts.append(a)
            used[0] += a.size
        return placed[key]

    def bilinear(i, col, n_in, n_out):
        if n_in == n_out:   # Pillow skips the pass
            return
        ksize, bounds, kk = _pillow.resample_tables(n_in, n_out)
        rows[i, col] = place(('b', n_in, n_out), lambda: bounds)
        rows[i, col + 1] = place(('k', n_in, n_out), lambda: _pillow.fixed_point(kk))
        rows[i, col + 2] = ksize

    for i in range(B):
        h, w = int(sizes[i][0]), int(sizes[i][1])
        order, factors, hue_shift = NO_JITTER if jitters[i] is None else jitters[i]
        order = [int(o) for o in order]
        if len(order) > 4 or len(set(order)) != len(order) or any(o not in (0, 1, 2, 3) for o in order):
            raise ValueError('item %d: order %r is not a permutation of distinct ops' % (i, order))
        if not 0 <= int(hue_shift) <= 255:
            raise ValueError('item %d: hue shift %r outside 0 .. 255' % (i, hue_shift))
        if h < 1 or w < 1:
            raise ValueError('item %d: resized to %d x %d' % (i, h, w))
        rows[i, 0], rows[i, 1], rows[i, 2] = h, w, 1 if flips[i] else 0
        rows[i, 3] = len(order)
        rows[i, 4] = sum(o << (4 * k) for k, o in enumerate(order))
        rowsf[i, 5:8] = np.float32(factors)
        rows[i, 8] = int(hue_shift)
        bilinear(i, 9, W, w)
        bilinear(i, 12, H, h)
        rows[i, 15] = place(('n', W, w), lambda: _pillow.nearest_table(W, w))
        rows[i, 16] = place(('n', H, h), lambda: _pillow.nearest_table(H, h))
        t = tables[i]
        rows[i, 17] = place(('c', t.tobytes()), lambda: t)
        rows[i, 18] = t.size // 2
    return np.concatenate([rows.reshape(-1)] + parts)


def segm_train_batch(frames_u8, scenes_u8, tables, short_size, flips, jitters, img_max_size=1274, padding_constant=8,
                     segm_downsampling_rate=8, frame_size=None):
    """One training batch of the semantic branch (vkitti_dataset.py:83-163), every tensor on the device.

    frames_u8, scenes_u8: uint8 [B, H, W, 3] CUDA, the RGB frames and the semantic colour images.  tables: B (codes [K, 3],
    labels [K]) pairs, the (r, g, b) -> label rows of each item's scene -- or one `color_table` for all items.  short_size: the
    batch's short size (:85).  flips: B booleans.  jitters: B results of `jitter_params`, or None for no jitter (a None entry:
    none for that item).  frame_size: the (height, width) `batch_sizes` scales, by default (H, W); the reference hard-codes
    (375, 1242).

    Returns {'img_data': fp32 [B, 3, Hb, Wb], 'seg_label': int64 [B, Hb // rate, Wb // rate], 'unknown': int32 [B]}.

    img_data[b, c, y, x] = (float(px[y, x, 2 - c]) - m_c) / s_c, px the jittered, flipped, Pillow-BILINEAR-resized frame, with
    m = (0.485 * 255, 0.456 * 255, 0.406 * 255) and s = (0.229, 0.224, 0.225) indexed by the OUTPUT channel: the reference
    swaps RGB to BGR first (:152) and then applies Normalize with its RGB-ordered constants (:44, :154), so the red mean meets
    the blue plane.  That quirk is kept.  The arithmetic is torch's CPU t.sub_(m).div_(s) on fp32.  Zero beyond the item.
    seg_label is the label - 1 at the positions the two NEAREST resizes sample (`label_formula`), -1 elsewhere.  unknown counts,
    per item, the SAMPLED scene pixels whose colour is not in the item's table (the reference raises KeyError at :120 for any
    such pixel of the frame); they get -1.

    Nothing crosses to the host; the item rows, Pillow's tables and the colour tables go up in one copy.  ValueError /
    SdnHipError before any launch for a contrast op on a frame of more than 2^21 pixels, sizes that do not fit the kernel's LDS
    plan, mismatched B, or a table of more than SEGM_MAX_COLORS colours."""
    from sdn_hip import ops
    for t, name in ((frames_u8, 'frames_u8'), (scenes_u8, 'scenes_u8')):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(t)))
        if not t.is_cuda:
            raise NotImplementedError('%s is on %s; the semantic training batch only runs on the GPU' % (name, t.device))
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
            raise ValueError('%s must be uint8 [B, H, W, 3], got %s %s' % (name, t.dtype, tuple(t.shape)))
    B, H, W, _ = frames_u8.shape
    if tuple(scenes_u8.shape) != (B, H, W, 3):
        raise ValueError('scenes_u8 must be uint8 [%d, %d, %d, 3], got %s' % (B, H, W, tuple(scenes_u8.shape)))
    jitters = [None] * B if jitters is None else list(jitters)
    flips = list(flips)
    if len(flips) != B or len(jitters) != B:
        raise ValueError('%d flips and %d jitters for %d items' % (len(flips), len(jitters), B))
    tabs = _as_tables(tables, B)
    sizes, Hb, Wb = batch_sizes(short_size, B, img_max_size, padding_constant, segm_downsampling_rate,
                                (H, W) if frame_size is None else tuple(frame_size))
    buf = table_buffer(sizes, tabs, flips, jitters, H, W)
    img, lab, unknown = ops.segm_train_batch(frames_u8, scenes_u8, buf, Hb, Wb, int(segm_downsampling_rate), MEAN, STD)
    return {'img_data': img, 'seg_label': lab, 'unknown': unknown}
