"""The training items of the geometric branch on the device: VKITTI, KITTI, Cityscapes and hybrid batches with roi and colour
jitter.

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

`hybrid_batch` does the same for the other training sets and for batches that mix them (datasets.py:549-606 KittiObject,
:737-769 KittiSemantics, :930-971 CityscapesSemantics, :1077-1112 CityscapesMaskRCNN; KittiSemanticsHybrid :772-777 and
CityscapesSemanticsHybrid :1115-1123 through collate_fn's zero fill): frames of several sizes (`SourceFrame`), per-item
normalisation, masks from a colour code or an instance-id map, ignore maps from nearer codes, from disparity >
np.percentile(., 95) or all zero.  Its entry points are sdn_train_id_stats (the Cityscapes items' rois and order statistics)
and sdn_train_crops_mixed; `hybrid_weights` is HybridDataset.get_weights (:184-190).

Out of scope: the full-frame `image_masks` / `image_ignores` entries (read only by evaluate-mode consumers); reading files
(pandas, PNGs, the json caches: the caller supplies frames, id and disparity maps, label rows, cached rois and cameras); the
samplers of data_loader.py:40-82 (`hybrid_weights` gives WeightedRandomSampler its weights, the draw of indices stays with the
caller).

GPU only: CPU tensors raise NotImplementedError."""
import random

import numpy as np
import torch

from derender3d import TargetType
from derender3d import scene as _scene
from sdn_hip.pillow import BRIGHTNESS, CONTRAST, HUE, SATURATION, jitter_params  # noqa: F401  (moved there: the semantic branch shares them)

ITEM_INTS = 12     # one row of sdn_train_crops's item table

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


# ---------------------------------------------------------------------------------------------------- the other training sets
class KittiCamera:
    """derender3d/datasets.py:427-430 (KittiBaseDataset.Camera)"""
    focal = 725.0
    u0 = 610.0
    v0 = 185.0


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # datasets.py:424-425, :785-786
MIXED_ITEM_INTS = 32      # one row of sdn_train_crops_mixed's item table
ID_ITEM_INTS = 8          # one row of sdn_train_id_stats' item table
MASK_NONE, MASK_CODE, MASK_ID = 0, 1, 2
IGNORE_ZERO, IGNORE_NEARER, IGNORE_DISPARITY = 0, 1, 2
KITTI_ROW_KEYS = ('top', 'left', 'bottom', 'right', 'ry', 'l', 'h', 'w', 'x', 'y', 'z')
KITTI_OBJECT_KEYS = ('focals', 'roi_norms', 'thetas', 'translation2ds', 'log_scales', 'log_depths')


class SourceFrame:
    """The CUDA tensors of one frame, any size: rgb_u8 uint8 [3, H, W]; scene_u8 uint8 [H, W, 3] (VKITTI's instance colours);
    ids int32 [H, W] (an instance-id map); disparity int32 [H, W] (values 0 .. 65535).  All contiguous: the kernels are handed
    their addresses."""

    def __init__(self, rgb_u8, scene_u8=None, ids=None, disparity=None):
        _scene._on_gpu(rgb_u8, 'rgb_u8')
        if rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 3 or rgb_u8.shape[0] != 3 or not rgb_u8.is_contiguous():
            raise ValueError('rgb_u8 must be contiguous uint8 [3, H, W], got %s %s' % (rgb_u8.dtype, tuple(rgb_u8.shape)))
        self.H, self.W = int(rgb_u8.shape[1]), int(rgb_u8.shape[2])
        for t, name, dtype, shape in ((scene_u8, 'scene_u8', torch.uint8, (self.H, self.W, 3)), (ids, 'ids', torch.int32, (self.H, self.W)),
                                      (disparity, 'disparity', torch.int32, (self.H, self.W))):
            if t is None:
                continue
            _scene._on_gpu(t, name)
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != rgb_u8.device:
                raise ValueError('%s must be contiguous %s %s on %s, got %s %s on %s'
                                 % (name, dtype, shape, rgb_u8.device, t.dtype, tuple(t.shape), t.device))
        self.rgb_u8, self.scene_u8, self.ids, self.disparity = rgb_u8, scene_u8, ids, disparity


class KittiObjectItem:
    """KittiObject.__getitem__ (datasets.py:549-606).  frame: index into the batch's frames; row: the label's top, left,
    bottom, right, ry, l, h, w, x, y, z (a mapping or a sequence in that order); camera: (focal, u0, v0) of the frame's
    calibration.  The crop uses int() of the edges, roi_norms the floats; no roi jitter; no masks or ignores."""
    targets = int(TargetType.pretrain)
    mean, std = IMAGENET_MEAN, IMAGENET_STD

    def __init__(self, frame, row, camera):
        self.frame = int(frame)
        self.row = np.asarray([row[k] for k in KITTI_ROW_KEYS] if hasattr(row, 'keys') else row, dtype=np.float64).reshape(11)
        self.camera = np.asarray(camera, dtype=np.float64).reshape(3)


class KittiSemanticsItem:
    """KittiSemantics.__getitem__ (datasets.py:737-769).  roi: the object's cached box (the reference reads it from its json
    cache); the mask is ids == obj_index; the ignore map is zero."""
    targets = int(TargetType.finetune)
    mean, std = IMAGENET_MEAN, IMAGENET_STD

    def __init__(self, frame, obj_index, roi):
        self.frame, self.obj_index, self.roi = int(frame), int(obj_index), [int(v) for v in roi]


class CityscapesItem:
    """CityscapesSemantics.__getitem__ (datasets.py:930-971): the roi from the mask ids == obj_index, the ignore map from
    disparity > np.percentile(non-zero disparities under the mask, 95)."""
    targets = int(TargetType.finetune)
    mean, std = IMAGENET_MEAN, IMAGENET_STD

    def __init__(self, frame, obj_index):
        self.frame, self.obj_index = int(frame), int(obj_index)


class MaskItem:
    """CityscapesMaskRCNN.__getitem__ (datasets.py:1077-1112).  roi: the cached box; camera: (f, u0, v0) of the frame's camera
    file; the mask is ids == obj_index (ids: the detector's index image); the ignore map is zero."""
    targets = int(TargetType.finetune)
    mean, std = IMAGENET_MEAN, IMAGENET_STD

    def __init__(self, frame, obj_index, roi, camera):
        self.frame, self.obj_index, self.roi = int(frame), int(obj_index), [int(v) for v in roi]
        self.camera = np.asarray(camera, dtype=np.float64).reshape(3)


def kitti_object_targets(rows, cameras):
    """The regression targets of B KittiObject items (datasets.py:557-596), float64 with the reference's operations in its
    order, each rounded to float32 once at the end.  rows: float64 [B, 11] in the order of KITTI_ROW_KEYS; cameras: float64
    [B, 3] rows (focal, u0, v0).  Returns {key: float32 [B, k]} for KITTI_OBJECT_KEYS."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(KITTI_ROW_KEYS))
    cameras = np.asarray(cameras, dtype=np.float64).reshape(-1, 3)
    top, left, bottom, right, ry, length, height, width, x, y, z = rows.T
    focal, u0, v0 = cameras.T
    normed = np.stack([(top - v0) / focal, (left - u0) / focal, (bottom - v0) / focal, (right - u0) / focal], axis=1)
    centre = (normed[:, 2:] + normed[:, :2]) / 2.0
    extent = normed[:, 2:] - normed[:, :2]
    size = np.stack([length, height, width], axis=1)
    position = np.stack([x, -(y - height / 2), -z], axis=1)
    offset = np.stack([(position[:, 1] / position[:, 2] - centre[:, 0]) / extent[:, 0],
                       (-position[:, 0] / position[:, 2] - centre[:, 1]) / extent[:, 1]], axis=1)
    offset = np.clip(offset, -6, 6)
    log_depth = np.log(squared_distances(x, y, height, z)) + np.log(extent[:, 0]) + np.log(extent[:, 1])
    values = {'focals': focal[:, None], 'roi_norms': normed, 'thetas': -ry[:, None], 'translation2ds': offset,
              'log_scales': np.log(size), 'log_depths': log_depth[:, None]}
    return {k: np.ascontiguousarray(values[k], dtype=np.float32) for k in KITTI_OBJECT_KEYS}


def roi_targets(roi, focal, u0, v0):
    """roi_norms of an integer roi (datasets.py:752-757, :943-948, :1091-1096): float64, rounded to float32 once"""
    principal = np.array([v0, u0, v0, u0], dtype=np.float64)
    return np.float32((np.asarray(roi, dtype=np.int64) - principal) / np.float64(focal))


def hybrid_weights(lengths, weights=None):
    """HybridDataset.get_weights (datasets.py:184-190): the sampling weight of every element of the concatenated sets, a set's
    weight spread evenly over its `lengths[k]` elements."""
    if weights is None:
        weights = [1.0] * len(lengths)
    return np.concatenate([weight * np.ones(int(n)) / int(n) for n, weight in zip(lengths, weights)], axis=0)


def id_item_table(records):
    """The item table of sdn_train_id_stats: int32 [B, 8].  records: per item (ids int32 [H, W] CUDA, disparity int32 [H, W]
    CUDA or None, id)."""
    tab = np.zeros((len(records), ID_ITEM_INTS), dtype=np.int32)
    wide = tab.view(np.uint64)
    for i, (ids, disparity, obj_index) in enumerate(records):
        wide[i, 0] = ids.data_ptr()
        wide[i, 1] = 0 if disparity is None else disparity.data_ptr()
        tab[i, 4], tab[i, 5], tab[i, 6] = ids.shape[0], ids.shape[1], int(obj_index)
    return tab


def mixed_item_table(records):
    """The item table of sdn_train_crops_mixed: int32 [B, 32] (include/sdn_hip.h).  records: per item a mapping with frame (uint8
    [3, H, W] CUDA), mask = (kind, tensor or None, code or id), ignore = (kind, tensor or None, thr, near_off, near_cnt),
    jitter = (order, factors, hue_shift), mean, std."""
    B = len(records)
    tab = np.zeros((B, MIXED_ITEM_INTS), dtype=np.int32)
    wide, tabf = tab.view(np.uint64), tab.view(np.float32)
    for i, rec in enumerate(records):
        order, factors, hue_shift = rec['jitter']
        order = [int(o) for o in order]
        if len(order) > 4 or len(set(order)) != len(order) or any(o not in (BRIGHTNESS, CONTRAST, SATURATION, HUE) for o in order):
            raise ValueError('item %d: order %r is not a permutation of distinct ops' % (i, order))
        if not 0 <= int(hue_shift) <= 255:
            raise ValueError('item %d: hue shift %r outside 0 .. 255' % (i, hue_shift))
        frame = rec['frame']
        mask_kind, mask_src, code = rec['mask']
        ignore_kind, ignore_src, thr, near_off, near_cnt = rec['ignore']
        wide[i, 0] = frame.data_ptr()
        wide[i, 1] = 0 if mask_src is None else mask_src.data_ptr()
        wide[i, 2] = 0 if ignore_src is None else ignore_src.data_ptr()
        tab[i, 6], tab[i, 7] = frame.shape[1], frame.shape[2]
        tab[i, 8], tab[i, 9] = mask_kind, code
        tab[i, 10], tab[i, 11], tab[i, 12], tab[i, 13] = ignore_kind, thr, near_off, near_cnt
        tab[i, 14] = len(order)
        tab[i, 15] = sum(o << (4 * k) for k, o in enumerate(order))
        tabf[i, 16:19] = np.float32(factors)
        tab[i, 19] = int(hue_shift)
        tabf[i, 20:23] = np.float32(rec['mean'])
        tabf[i, 23:26] = np.float32(rec['std'])
    return tab


def item_targets(item):
    """the `targets` bits of one item: pretrain | finetune (VKITTI), pretrain (KittiObject) or finetune"""
    return int(TargetType.pretrain | TargetType.finetune) if isinstance(item, Item) else int(item.targets)


def item_entries(item, roi, height, width):
    """The float32 entries of one item as its __getitem__ returns them, from the roi used and the size of its frame:
    {key: float32 [k]}.  `has_maps(item)` says whether the item also has `masks` and `ignores`."""
    if isinstance(item, Item):
        return {k: v[0] for k, v in batch_targets([[item.rows[k][item.index] for k in ROW_KEYS]], [roi]).items()}
    if isinstance(item, KittiObjectItem):
        return {k: v[0] for k, v in kitti_object_targets([item.row], [item.camera]).items()}
    if isinstance(item, KittiSemanticsItem):
        return {'focals': np.float32([KittiCamera.focal]),
                'roi_norms': roi_targets(roi, KittiCamera.focal, (width - 1) / 2, (height - 1) / 2)}
    if isinstance(item, CityscapesItem):
        focal, u0, v0 = _scene.CityscapesCamera.focal, _scene.CityscapesCamera.u0, _scene.CityscapesCamera.v0
    elif isinstance(item, MaskItem):
        focal, u0, v0 = item.camera
    else:
        raise TypeError('%r is not a training item' % (type(item),))
    e = {'widths': np.float32([width]), 'heights': np.float32([height]), 'focals': np.float32([focal]), 'u0s': np.float32([u0]),
         'v0s': np.float32([v0]), 'roi_norms': roi_targets(roi, focal, u0, v0)}
    if isinstance(item, CityscapesItem):
        e['rois'] = np.float32(roi)
    return e


def has_maps(item):
    """whether the item's dict holds `masks` and `ignores` (every kind but KittiObjectItem)"""
    return not isinstance(item, KittiObjectItem)


def collate_entries(items, entries):
    """collate_fn (data_loader.py:17-37) on the host entries of a batch: the union of the items' keys in the order of
    TARGET_KEYS, each [B, k] float32 with zero rows where an item lacks the key, and `targets` int64 [B].
    Returns ({key: array}, maps) -- maps: whether the batch holds `masks` and `ignores`."""
    out = {}
    for k in TARGET_KEYS:
        present = [e[k] for e in entries if k in e]
        if present:
            out[k] = np.stack([e[k] if k in e else np.zeros_like(present[0]) for e in entries]).astype(np.float32)
    out['targets'] = np.asarray([item_targets(it) for it in items], dtype=np.int64)
    return out, any(has_maps(it) for it in items)


def _pack_code(c):
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def hybrid_batch(frames, items, is_train, jitter=None, rois=None, rng=random, image_size=224, mask_size=256):
    """B training items of any of the geometric training sets as the batch collate_fn (data_loader.py:17-37) gives
    BaseNet.step_batch for that list of items, every tensor on the device.

    frames: a sequence of `SourceFrame`; items: a sequence of `Item` (VKITTI: the frame needs scene_u8), `KittiObjectItem`,
    `KittiSemanticsItem`, `MaskItem` (the frame needs ids) and `CityscapesItem` (ids and disparity), each naming its frame by
    index.  The dict holds the union of the items' keys, every key [B, ...]; where an item lacks a key its row is zero;
    `targets` int64 [B] per item (pretrain | finetune, pretrain or finetune); a batch of one kind holds only that kind's keys.
    Per item, in the sequence's order, the reference's draws in its order: with is_train the roi jitter where the class jitters
    (not KittiObjectItem), then the colour jitter's parameters.  jitter: per item (order, factors, hue_shift) instead of
    drawing them; rois: per item the roi to use instead of jittering (int [B, 4]; the row of a KittiObjectItem is not read).
    Host traffic: one upload (item records), one download (sdn_train_id_stats' table for the Cityscapes items, sdn_train_rois'
    rows for the VKITTI items), one upload (windows, Pillow's tables, item rows, nearer codes, targets); both launches and the
    download are skipped when no item needs them.  IndexError for an item whose id or code matches no pixel of its frame."""
    from sdn_hip import ops
    frames, items = list(frames), list(items)
    B = len(items)
    if B < 1:
        raise ValueError('no items')
    if not frames or any(not isinstance(f, SourceFrame) for f in frames):
        raise TypeError('frames must be a non-empty sequence of SourceFrame')
    if jitter is not None and len(jitter) != B:
        raise ValueError('%d jitter records for %d items' % (len(jitter), B))
    if rois is not None and np.asarray(rois).shape != (B, 4):
        raise ValueError('rois must be [%d, 4], got %s' % (B, np.asarray(rois).shape))
    dev = frames[0].rgb_u8.device
    for i, it in enumerate(items):
        if not 0 <= it.frame < len(frames):
            raise ValueError('item %d names frame %d of %d' % (i, it.frame, len(frames)))
        fr = frames[it.frame]
        if fr.rgb_u8.device != dev:
            raise ValueError('frame %d is on %s, frame 0 on %s' % (it.frame, fr.rgb_u8.device, dev))
        need = {Item: ('scene_u8',), CityscapesItem: ('ids', 'disparity'), KittiSemanticsItem: ('ids',), MaskItem: ('ids',),
                KittiObjectItem: ()}.get(type(it))
        if need is None:
            raise TypeError('item %d: %r is not a training item' % (i, type(it)))
        for name in need:
            if getattr(fr, name) is None:
                raise ValueError('item %d (%s) needs `%s` of frame %d' % (i, type(it).__name__, name, it.frame))

    # ---- upload 1, the launches and the one download: the rois that come from a mask
    vk = [i for i, it in enumerate(items) if isinstance(it, Item)]
    cs = [i for i, it in enumerate(items) if isinstance(it, CityscapesItem)]
    mask_rows = {}
    if vk or cs:
        vk_frames = sorted({items[i].frame for i in vk})
        groups = [[i for i in vk if items[i].frame == f] for f in vk_frames]
        arrays = [id_item_table([(frames[items[i].frame].ids, frames[items[i].frame].disparity, items[i].obj_index) for i in cs])] if cs else []
        arrays += [np.asarray([[0] + [int(v) for v in items[i].code] for i in grp], dtype=np.int32) for grp in groups]
        uploaded = _scene.upload_int32(arrays, dev)           # the id records first: the blob's start is aligned to 8 bytes
        parts = []
        if cs:
            largest = max(frames[items[i].frame].H * frames[items[i].frame].W for i in cs)
            parts.append(ops.train_id_stats(uploaded[0], largest).reshape(-1))
        for f, rows_d in zip(vk_frames, uploaded[1 if cs else 0:]):
            parts.append(ops.train_rois(frames[f].scene_u8[None], rows_d).reshape(-1))
        host = (torch.cat(parts) if len(parts) > 1 else parts[0]).cpu().numpy()
        off = 0
        if cs:
            for k, i in enumerate(cs):
                mask_rows[i] = host[8 * k:8 * k + 8]
            off = 8 * len(cs)
        for grp in groups:
            for k, i in enumerate(grp):
                mask_rows[i] = host[off + 5 * k:off + 5 * k + 5]
            off += 5 * len(grp)
        for i in vk + cs:
            area = mask_rows[i][4] if i in vk else mask_rows[i][0]
            if area == 0:
                what = 'code %s' % items[i].code.tolist() if i in vk else 'id %d' % items[i].obj_index
                raise IndexError('item %d: %s matches no pixel of frame %d' % (i, what, items[i].frame))

    # ---- the draws, per item as the reference's __getitem__ makes them: roi, then colour; and the host entries
    used_rois, jitters, entries, records = np.zeros((B, 4), dtype=np.int32), [], [], []
    near_codes = []
    near_total = 0
    for i, it in enumerate(items):
        fr = frames[it.frame]
        if isinstance(it, KittiObjectItem):
            roi = [int(v) for v in it.row[:4]]
        else:
            if isinstance(it, Item):
                roi = [int(v) for v in mask_rows[i][:4]]
            elif isinstance(it, CityscapesItem):
                roi = [int(v) for v in mask_rows[i][1:5]]
            else:
                roi = list(it.roi)
            if rois is not None:
                roi = [int(v) for v in np.asarray(rois)[i]]
            elif is_train:
                roi = roi_jitter(roi, rng=rng)
        used_rois[i] = roi
        jitters.append(jitter[i] if jitter is not None else (jitter_params(rng=rng) if is_train else NO_JITTER))
        mask, ignore, mean, std = (MASK_NONE, None, 0), (IGNORE_ZERO, None, 0, 0, 0), IMAGENET_MEAN, IMAGENET_STD
        if isinstance(it, Item):
            codes = it.codes[nearer_objects(it.rows, it.index)]
            mask = (MASK_CODE, fr.scene_u8, _pack_code(it.code))
            ignore = (IGNORE_NEARER, fr.scene_u8, 0, near_total, codes.shape[0])
            near_codes.append(codes)
            near_total += codes.shape[0]
            mean, std = VKITTI_MEAN, VKITTI_STD
        elif not isinstance(it, KittiObjectItem):
            mask = (MASK_ID, fr.ids, it.obj_index)
            if isinstance(it, CityscapesItem):
                n, lo, hi = (int(v) for v in mask_rows[i][5:8])
                ignore = (IGNORE_DISPARITY, fr.disparity, int(_scene.percentile95_threshold([n], [lo], [hi])[0]), 0, 0)
        entries.append(item_entries(it, roi, fr.H, fr.W))
        records.append({'frame': fr.rgb_u8, 'mask': mask, 'ignore': ignore, 'jitter': jitters[-1], 'mean': mean, 'std': std})

    # ---- upload 2: the item rows (first: aligned to 8 bytes), windows, Pillow's tables, nearer codes, targets
    host, maps = collate_entries(items, entries)
    keys = [k for k in host if k != 'targets']
    widths = {k: host[k].shape[1] for k in keys}
    floats = np.concatenate([host[k] for k in keys] + [host['targets'].astype(np.int32).view(np.float32)[:, None]], axis=1)
    item_tab = mixed_item_table(records)
    objs, bounds, kk8 = _scene.crop_tables(used_rois, [frames[it.frame].H for it in items], [frames[it.frame].W for it in items],
                                           image_size, mask_size)
    packed = np.zeros(4 * ((3 * near_total + 3) // 4 + 1), dtype=np.uint8)      # the codes as bytes inside the int32 blob
    if near_total:
        packed[:3 * near_total] = np.concatenate(near_codes).reshape(-1)
    item_d, objs_d, bounds_d, kk8_d, near_d, floats_d = _scene.upload_int32(
        [item_tab, objs, bounds, kk8, packed.view(np.int32), np.ascontiguousarray(floats).view(np.int32)], dev)
    nearer = near_d.view(torch.uint8)[:3 * near_total].view(near_total, 3)
    images, masks, ignores = ops.train_crops_mixed(used_rois, objs, item_tab, (objs_d, bounds_d, kk8_d), item_d, nearer, image_size,
                                                   mask_size, maps=maps)
    batch = {'images': images}
    if maps:
        batch['masks'], batch['ignores'] = masks, ignores
    off = 0
    for k in keys:
        batch[k] = floats_d.view(torch.float32)[:, off:off + widths[k]].contiguous()
        off += widths[k]
    batch['targets'] = floats_d[:, off].to(torch.int64)
    return batch
