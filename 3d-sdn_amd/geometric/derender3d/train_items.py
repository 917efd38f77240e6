"""The training items of the geometric branch on the device: a VKITTI batch with roi and colour jitter.

Reference: geometric/derender3d/datasets.py:332-420 (VKitti.__getitem__) with :37-46 (Transforms.roi_jitter), :141-172
(BaseDataset.transform_rgb / transform_mask / transform_ignore, including Transforms.color_jitter) and data_loader.py:17-37
(collate_fn).  The reference prepares every object on the host: one full-frame np.all per object of the frame, three PIL round
trips and, when training, four ImageEnhance / HSV passes over the crop.  Here a batch of B items that may span several frames
is two entry points: sdn_train_rois (the mask_to_roi boxes, B x 5 integers to the host, because the roi jitter's range
depends on the roi) and sdn_train_crops (images, masks, ignores of all items; the colour jitter is applied on the device, bit
for bit with Pillow, from parameters drawn on the host).  The regression targets are host arithmetic on a few numbers per item
(`vkitti_targets`, float64 as the reference) and travel with the second upload.

`train_batch` returns the dict collate_fn would hand BaseNet.step_batch.  Host traffic per batch: one upload (the items'
frames and codes, the nearer codes), one download (the roi table), one upload (windows, Pillow's tables, jitter, targets).

Out of scope: the full-frame `image_masks` / `image_ignores` entries (read only by evaluate-mode consumers); the KITTI and
Cityscapes training classes; reading files (pandas, PNGs: the caller supplies frames, scene images and motgt rows);
HybridDataset.

GPU only: CPU tensors raise NotImplementedError."""
import random

import numpy as np
import torch

from derender3d import TargetType
from derender3d import scene as _scene

ITEM_INTS = 12     # one row of sdn_train_crops's item table
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

TARGET_KEYS = ('rois', 'roi_norms', 'thetas', 'rotations', 'translations', 'translation2ds', 'scales', 'log_scales', 'log_depths',
               'widths', 'heights', 'focals', 'u0s', 'v0s')
ROW_KEYS = ('ry', 'l3d', 'h3d', 'w3d', 'x3d', 'y3d', 'z3d')


class VKittiCamera:
    """derender3d/datasets.py:207-213"""
    width = 1242
    height = 375

    focal = 725.0
    u0 = 620.5
    v0 = 187.0


VKITTI_MEAN, VKITTI_STD = (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)     # datasets.py:204-205


def roi_jitter(roi, ratio=0.1, rng=random):
    """Transforms.roi_jitter (datasets.py:37-46) with the reference's draws in its order: every edge of (top, left, bottom,
    right) moves by one rng.randint, the rows within +- int(ratio * height), the columns within +- int(ratio * width)."""
    reach = (int(ratio * (roi[2] - roi[0])), int(ratio * (roi[3] - roi[1])))       # (rows, columns)
    return [int(edge) + rng.randint(-reach[k % 2], reach[k % 2]) for k, edge in enumerate(roi)]


def jitter_params(brightness=.5, contrast=.5, saturation=.5, hue=.5, rng=random):
    """The draws of torchvision 0.2.1's ColorJitter.get_params -> (order, factors, hue_shift): `order` the ops present
    (BRIGHTNESS, CONTRAST, SATURATION, HUE) as shuffled, `factors` the brightness, contrast and saturation factors (1.0 for an
    absent op), `hue_shift` what adjust_hue adds to the H plane: int(hue_factor * 255) % 256, C's truncation toward zero and the
    wrap of np.uint8(...).  One uniform draw per present op in the order brightness, contrast, saturation, hue, then one shuffle
    of the list of ops.

    torchvision is not among this project's dependencies: the SAMPLING here is a restatement and is not pinned against it.
    Only the APPLICATION of given parameters (sdn_train_crops) is pinned, against Pillow."""
    order, factors, hue_shift = [], [1.0, 1.0, 1.0], 0
    if brightness > 0:
        factors[0] = rng.uniform(max(0, 1 - brightness), 1 + brightness)
        order.append(BRIGHTNESS)
    if contrast > 0:
        factors[1] = rng.uniform(max(0, 1 - contrast), 1 + contrast)
        order.append(CONTRAST)
    if saturation > 0:
        factors[2] = rng.uniform(max(0, 1 - saturation), 1 + saturation)
        order.append(SATURATION)
    if hue > 0:
        hue_shift = int(rng.uniform(-hue, hue) * 255) % 256
        order.append(HUE)
    rng.shuffle(order)
    return order, tuple(factors), hue_shift


def squared_distances(x3d, y3d, h3d, z3d):
    """What datasets.py:378 / :385-386 order the objects of a frame by: the squared distance of the box centre (the motgt
    position is the bottom centre, so half the height comes off y), float64.  The three squares are added left to right, as
    numpy's sum over three elements adds them, so an object's own value is the same in both places."""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x3d, y3d - np.asarray(h3d, dtype=np.float64) / 2, z3d))
    return x * x + y * y + z * z


def nearer_objects(rows_of_frame, index):
    """The rows of a frame whose box centre is strictly nearer than row `index`'s (datasets.py:391, `depths < depth`):
    the objects whose masks make up that object's ignore map."""
    d = squared_distances(rows_of_frame['x3d'], rows_of_frame['y3d'], rows_of_frame['h3d'], rows_of_frame['z3d'])
    return np.flatnonzero(d < d[index])


def batch_targets(rows, rois, camera=VKittiCamera):
    """The regression targets of B items at once (datasets.py:351-383, 397-410), float64 with the reference's operations in
    its order, each rounded to float32 once at the end.  rows: float64 [B, 7] in the order of ROW_KEYS; rois: int [B, 4].
    Returns {key: float32 [B, k]} for TARGET_KEYS."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(ROW_KEYS))
    rois = np.asarray(rois).astype(np.int64).reshape(-1, 4)
    B = rows.shape[0]
    ry, length, height, width, x, y, z = rows.T
    # the roi in camera units, its centre and its extent, (row, column) each
    principal = np.array([camera.v0, camera.u0, camera.v0, camera.u0])
    normed = (rois - principal) / camera.focal
    centre = (normed[:, 2:] + normed[:, :2]) / 2.0
    extent = normed[:, 2:] - normed[:, :2]
    # pose: the yaw as a quaternion about the vertical axis; size; the box centre in the renderer's axes (y up, z backwards)
    half = ry / 2
    zero = np.zeros(B)
    quaternion = np.stack([np.cos(half), zero, -np.sin(half), zero], axis=1)
    size = np.stack([length, height, 1.2206 * width], axis=1)
    position = np.stack([x, -(y - height / 2), -z], axis=1)
    # where the centre projects, relative to the roi
    offset = np.stack([(position[:, 1] / position[:, 2] - centre[:, 0]) / extent[:, 0],
                       (-position[:, 0] / position[:, 2] - centre[:, 1]) / extent[:, 1]], axis=1)
    offset = np.clip(offset, -6, 6)
    distance2 = squared_distances(x, y, height, z)
    log_depth = np.log(distance2) + np.log(extent[:, 0]) + np.log(extent[:, 1])
    const = lambda v: np.full((B, 1), v)
    values = {'rois': rois, 'roi_norms': normed, 'thetas': -ry[:, None], 'rotations': quaternion, 'translations': position,
              'translation2ds': offset, 'scales': size, 'log_scales': np.log(size), 'log_depths': log_depth[:, None],
              'widths': const(camera.width), 'heights': const(camera.height), 'focals': const(camera.focal),
              'u0s': const(camera.u0), 'v0s': const(camera.v0)}
    return {k: np.ascontiguousarray(values[k], dtype=np.float32) for k in TARGET_KEYS}


def vkitti_targets(row, rows_of_frame, roi, camera=VKittiCamera):
    """datasets.py:351-391 for one object.  row: its motgt values (a mapping with ry, l3d, h3d, w3d, x3d, y3d, z3d);
    rows_of_frame: the same columns of every object of the frame (a mapping of arrays; x3d, y3d, h3d, z3d are read); roi: the
    (jittered) integer roi.  Returns (entries, nearer): the float32 arrays of TARGET_KEYS and the int `targets`
    (TargetType.pretrain | finetune), and the indices of the frame's objects that are strictly nearer."""
    entries = {k: v[0] for k, v in batch_targets([[row[k] for k in ROW_KEYS]], [roi], camera).items()}
    entries['targets'] = TargetType.pretrain | TargetType.finetune
    own = squared_distances(row['x3d'], row['y3d'], row['h3d'], row['z3d'])
    others = squared_distances(rows_of_frame['x3d'], rows_of_frame['y3d'], rows_of_frame['h3d'], rows_of_frame['z3d'])
    return entries, np.flatnonzero(others < own)


class Item:
    """One training item as host data: `frame` the index into the batch's frames, `index` the object's row among the frame's
    motgt rows, `rows` those rows (a mapping of float64 arrays: ry, l3d, h3d, w3d, x3d, y3d, z3d) and `codes` uint8 [K, 3] the
    scene colour of every row.  The item's own code is codes[index]."""

    def __init__(self, frame, index, rows, codes):
        self.frame, self.index, self.rows = int(frame), int(index), rows
        self.codes = np.ascontiguousarray(np.asarray(codes).astype(np.uint8).reshape(-1, 3))
        if not 0 <= self.index < self.codes.shape[0]:
            raise ValueError('object %d of a frame with %d rows' % (self.index, self.codes.shape[0]))

    @property
    def code(self):
        return self.codes[self.index]

    def row(self):
        return {k: self.rows[k][self.index] for k in ROW_KEYS}


def item_table(frames, codes, near_offsets, near_counts, jitters):
    """The item table of sdn_train_crops: int32 [B, 12] (include/sdn_hip.h).  jitters: per item (order, factors, hue_shift)."""
    B = len(frames)
    tab = np.zeros((B, ITEM_INTS), dtype=np.int32)
    tabf = tab.view(np.float32)
    for i in range(B):
        order, factors, hue_shift = jitters[i]
        order = [int(o) for o in order]
        if len(order) > 4 or len(set(order)) != len(order) or any(o not in (BRIGHTNESS, CONTRAST, SATURATION, HUE) for o in order):
            raise ValueError('item %d: order %r is not a permutation of distinct ops' % (i, order))
        if not 0 <= int(hue_shift) <= 255:
            raise ValueError('item %d: hue shift %r outside 0 .. 255' % (i, hue_shift))
        c = codes[i]
        tab[i, 0] = frames[i]
        tab[i, 1] = int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
        tab[i, 2], tab[i, 3] = near_offsets[i], near_counts[i]
        tab[i, 4] = len(order)
        tab[i, 5] = sum(o << (4 * k) for k, o in enumerate(order))
        tabf[i, 6:9] = np.float32(factors)
        tab[i, 9] = int(hue_shift)
    return tab


NO_JITTER = ((), (1.0, 1.0, 1.0), 0)


def train_batch(frames_u8, scenes_u8, items, is_train, jitter=None, image_size=224, mask_size=256, mean=VKITTI_MEAN,
                std=VKITTI_STD, rois=None, rng=random):
    """B training items as the batch collate_fn gives BaseNet.step_batch, every tensor on the device.

    frames_u8 uint8 [Fr, 3, H, W], scenes_u8 uint8 [Fr, H, W, 3] (the instance-colour images), both CUDA; items: a sequence
    of `Item`.  Per item, in the sequence's order, the reference's draws: with is_train the roi is jittered (`roi_jitter` on
    `rng`) and the colour jitter's parameters are drawn (`jitter_params` on `rng`).  jitter: per item (order, factors,
    hue_shift) instead of drawing them -- parameters as data; rois: per item the roi to use instead of jittering the mask's
    (int [B, 4]).  is_train False: no jitter of either kind, exactly the crops of sdn_scene_crops.
    Returns images [B, 3, S_i, S_i], masks, ignores [B, 1, S_m, S_m], the float32 entries of `batch_targets` [B, k]
    and targets int64 [B].  IndexError for an item whose code matches no pixel of its frame (Transforms.mask_to_roi)."""
    from sdn_hip import ops
    _scene._on_gpu(frames_u8, 'frames_u8')
    _scene._on_gpu(scenes_u8, 'scenes_u8')
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[1] != 3:
        raise ValueError('frames_u8 must be uint8 [Fr, 3, H, W], got %s %s' % (frames_u8.dtype, tuple(frames_u8.shape)))
    Fr, _, H, W = (int(v) for v in frames_u8.shape)
    if scenes_u8.dtype != torch.uint8 or tuple(scenes_u8.shape) != (Fr, H, W, 3):
        raise ValueError('scenes_u8 must be uint8 [%d, %d, %d, 3], got %s %s' % (Fr, H, W, scenes_u8.dtype, tuple(scenes_u8.shape)))
    items = list(items)
    B = len(items)
    if B < 1:
        raise ValueError('no items')
    if jitter is not None and len(jitter) != B:
        raise ValueError('%d jitter records for %d items' % (len(jitter), B))
    if rois is not None and np.asarray(rois).shape != (B, 4):
        raise ValueError('rois must be [%d, 4], got %s' % (B, np.asarray(rois).shape))
    for i, it in enumerate(items):
        if not 0 <= it.frame < Fr:
            raise ValueError('item %d names frame %d of %d' % (i, it.frame, Fr))
    dev = frames_u8.device

    # ---- upload 1: (frame, code) per item and the nearer codes, which depend on the motgt rows alone
    depth_order = [nearer_objects(it.rows, it.index) for it in items]
    near_codes = [it.codes[idx] for it, idx in zip(items, depth_order)]
    near_counts = [c.shape[0] for c in near_codes]
    near_offsets = np.concatenate([[0], np.cumsum(near_counts)[:-1]]).astype(np.int64)
    total = int(sum(near_counts))
    packed = np.zeros(4 * ((3 * total + 3) // 4 + 1), dtype=np.uint8)      # the codes as bytes inside the int32 blob
    if total:
        packed[:3 * total] = np.concatenate(near_codes).reshape(-1)
    first = np.asarray([[it.frame] + [int(v) for v in it.code] for it in items], dtype=np.int32)
    first_d, near_d = _scene.upload_int32([first, packed.view(np.int32)], dev)
    nearer = near_d.view(torch.uint8)[:3 * total].view(total, 3)

    # ---- the one download: mask_to_roi of every item
    table = ops.train_rois(scenes_u8, first_d).cpu().numpy()
    empty = np.flatnonzero(table[:, 4] == 0)
    if empty.size:
        i = int(empty[0])
        raise IndexError('item %d: code %s matches no pixel of frame %d' % (i, items[i].code.tolist(), items[i].frame))

    # ---- the draws, per item as the reference's __getitem__ makes them: roi, then colour
    used_rois, jitters = np.zeros((B, 4), dtype=np.int32), []
    for i in range(B):
        roi = [int(v) for v in table[i, :4]]
        if rois is not None:
            roi = [int(v) for v in np.asarray(rois)[i]]
        elif is_train:
            roi = roi_jitter(roi, rng=rng)
        used_rois[i] = roi
        if jitter is not None:
            jitters.append(jitter[i])
        elif is_train:
            jitters.append(jitter_params(rng=rng))
        else:
            jitters.append(NO_JITTER)
    entries = batch_targets([[it.rows[k][it.index] for k in ROW_KEYS] for it in items], used_rois)

    # ---- upload 2: windows, Pillow's tables, the item table, the targets
    objs, bounds, kk8 = _scene.crop_tables(used_rois, H, W, image_size, mask_size)
    item_tab = item_table([it.frame for it in items], [it.code for it in items], near_offsets, near_counts, jitters)
    floats = np.ascontiguousarray(np.concatenate([entries[k] for k in TARGET_KEYS], axis=1))
    objs_d, bounds_d, kk8_d, item_d, floats_d = _scene.upload_int32([objs, bounds, kk8, item_tab, floats.view(np.int32)], dev)
    images, masks, ignores = ops.train_crops(frames_u8, scenes_u8, used_rois, objs, item_tab, (objs_d, bounds_d, kk8_d), item_d,
                                             nearer, image_size, mask_size, mean, std)
    batch = {'images': images, 'masks': masks, 'ignores': ignores}
    floats_d = floats_d.view(torch.float32)
    off = 0
    for k in TARGET_KEYS:
        n = entries[k].shape[1]
        batch[k] = floats_d[:, off:off + n].contiguous()
        off += n
    batch['targets'] = torch.full((B,), int(TargetType.pretrain | TargetType.finetune), dtype=torch.int64, device=dev)
    return batch
