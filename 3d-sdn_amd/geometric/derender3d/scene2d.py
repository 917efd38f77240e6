"""The 2D and 2D+ edit baselines: every object's detector mask cut out at its roi, scaled, moved and painted back.

Reference: geometric/scripts/main.py `_test_2d` / `_test_2d_plus` (:215-322, dispatched at :834-844); no de-rendering:
  :236-238  the unedited masks painted in index order (NAME-ref.png)
  :244-251  roi centres and extents in PIXELS
  :256-291  every operation of the edit JSON matched to an object in pixel coordinates; `delete` clears the interest,
            `modify` moves the centre by (to - from) and scales the extent by zoom (2D+: the columns by zoom cos(ry))
  :293-312  per interesting object: PIL resize of the mask window to (int(d0), int(d1)), paste at (int(m1 - d1 / 2),
            int(m0 - d0 / 2)), round, blend in index order
  :314-318  NAME.json {index + 1: {'class_id'}} and NAME.png
The reference runs one to_pil_image, resize, new, paste, to_tensor and upload per object and frame, each `int(...)` of a
CUDA scalar a device synchronisation.  Here the host computes what the reference computes on float32 tensors with torch
CPU float32 tensors in the same order (the `int()` truncations then land on the same integers) and Pillow's resampling
tables (derender3d/compositing.py), uploads them in one copy, and one sdn_scene_paint2d launch paints F frames out of the
cover words of sdn_scene_cover.  Nothing is copied back: `Scene2D(...).edit(lists)` -> frames ->
`EditSession.render_batch([(fr.inst_u8, fr.json, None) for fr in frames])` for a model without pose and normal features.

Unlike `_test`, all objects start interesting (:234): the class and area test is not applied.

GPU only: CPU tensors raise NotImplementedError."""
import json
import os

import numpy as np
import torch

from derender3d import compositing as _comp
from derender3d import scene as _scene

REC_INTS = 16      # one row of sdn_scene_paint2d's record table


# ---------------------------------------------------------------------------------------------------- host half
def resample_u8_rect_numpy(img, out_h, out_w):
    """Host emulation of ImagingResample on an 8-bit [h, w] image resized to [out_h, out_w], one table per axis: the
    horizontal pass first, rounded and clipped to 8 bits, then the vertical pass; a pass is skipped when its size does not
    change.  Used by the CPU tests to pin the per-axis tables against the real PIL; sdn_scene_paint2d evaluates the same
    sums per pixel."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    if out_h < 1 or out_w < 1:
        raise ValueError('height and width must be > 0')
    half = 1 << (_comp.PRECISION_BITS - 1)
    cur = img.astype(np.int64)
    if out_w != w:
        _, bounds, kk = _comp.resample_tables(w, out_w)
        k8 = _comp.fixed_point(kk).astype(np.int64)
        tmp = np.zeros((h, out_w), dtype=np.int64)
        for ox in range(out_w):
            x0, c = bounds[ox]
            tmp[:, ox] = half + (cur[:, x0:x0 + c] * k8[ox, :c]).sum(axis=1)
        cur = np.clip(tmp >> _comp.PRECISION_BITS, 0, 255)
    if out_h != h:
        _, bounds, kk = _comp.resample_tables(h, out_h)
        k8 = _comp.fixed_point(kk).astype(np.int64)
        tmp = np.zeros((out_h, cur.shape[1]), dtype=np.int64)
        for oy in range(out_h):
            y0, c = bounds[oy]
            tmp[oy] = half + (cur[y0:y0 + c] * k8[oy, :c, None]).sum(axis=0)
        cur = np.clip(tmp >> _comp.PRECISION_BITS, 0, 255)
    return cur.astype(np.uint8)


def check_rois(rois, height, width):
    """rois (y0, x0, y1, x1) as int32 [N, 4]; ValueError for an empty roi or one that leaves the frame (the reference slices
    the mask with it, :301)."""
    rois = np.ascontiguousarray(np.asarray(rois, dtype=np.int32).reshape(-1, 4))
    for i, (y0, x0, y1, x1) in enumerate(rois.tolist()):
        if y1 - y0 < 1 or x1 - x0 < 1:
            raise ValueError('roi %d (%d, %d, %d, %d) is empty' % (i, y0, x0, y1, x1))
        if y0 < 0 or x0 < 0 or y1 > height or x1 > width:
            raise ValueError('roi %d (%d, %d, %d, %d) leaves the %d x %d frame' % (i, y0, x0, y1, x1, height, width))
    return rois


def roi_extents(rois):
    """main.py:244-251 in float32 on the host: (mrois, drois) float32 [N, 2], the centres and extents (row, column) in pixels"""
    r = torch.as_tensor(np.asarray(rois, dtype=np.int32).reshape(-1, 4))
    mrois = torch.stack([r[:, 2] + r[:, 0], r[:, 3] + r[:, 1]], dim=1).float() / 2.0
    drois = torch.stack([r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]], dim=1).float()
    return mrois, drois


def match_operations(mrois, operations):
    """main.py:257-268: [(object index, operation index)] in the reference's iteration order, matched in PIXEL coordinates
    (scene.match_operations works in camera-normalised units).  mrois: float32 [N, 2] host tensor (roi_extents)."""
    ops_ = torch.tensor([[float(op['from']['v']), float(op['from']['u'])] for op in operations])
    mrois = torch.as_tensor(mrois, dtype=torch.float32)
    diffs = torch.sum((mrois[:, None, :] - ops_[None, :, :]) ** 2, dim=2)
    if len(mrois) < len(ops_):
        return [(i, int(j)) for i, j in enumerate(torch.argmin(diffs, dim=1))]
    return [(int(i), j) for j, i in enumerate(torch.argmin(diffs, dim=0))]


def edit_geometry(rois, operations, use_ry=False):
    """main.py:244-291 for one operation list -> (mrois, drois float32 [N, 2], interests list of bool, matched pairs).  All
    objects start interesting (:234).  A later operation matched to the same object reads what the earlier one left."""
    mrois, drois = roi_extents(rois)
    mrois, drois = mrois.clone(), drois.clone()
    interests = [True] * mrois.shape[0]
    pairs = match_operations(mrois, operations) if operations else []
    for obj, j in pairs:
        op = operations[j]
        u, v = float(op['from']['u']), float(op['from']['v'])
        if op['type'] == 'delete':
            interests[obj] = False
        elif op['type'] == 'modify':
            u2, v2 = float(op['to'].get('u', u)), float(op['to'].get('v', v))
            zoom, ry = float(op['zoom']), float(op['ry'])
            mrois[obj] = mrois[obj] + torch.tensor([v2 - v, u2 - u])
            if use_ry:
                drois[obj] = torch.tensor([zoom * drois[obj, 0], zoom * float(np.cos(ry)) * drois[obj, 1]])
            else:
                drois[obj] = zoom * drois[obj]
        # the reference ignores other types silently
    return mrois, drois, interests, pairs


def paste_boxes(mrois, drois):
    """main.py:303-308: per object (output rows, output columns, paste top, paste left), float32 tensor arithmetic and
    int() as the reference"""
    out = []
    for i in range(mrois.shape[0]):
        oh, ow = int(drois[i, 0]), int(drois[i, 1])
        left = int(mrois[i, 1] - drois[i, 1] / 2)
        top = int(mrois[i, 0] - drois[i, 0] / 2)
        out.append((oh, ow, top, left))
    return out


def paint_tables(rois, boxes, interests, height, width):
    """The host tables of sdn_scene_paint2d for F frames: (records int32 [F, N, 16], bounds int32 [M, 2], kk8 int32 [K]).
    rois int32 [N, 4]; boxes[f][n] = (output rows, columns, paste top, left) (paste_boxes); interests[f][n].  One Pillow
    table (compositing.resample_tables + fixed_point) per axis and distinct (in, out) pair; none when they are equal, where
    Pillow skips the pass.  ValueError for an interesting object whose output size is below 1 in either axis (Pillow:
    "height and width must be > 0").  An object whose paste box misses the frame is marked inactive: it paints nothing."""
    rois = check_rois(rois, height, width)
    F, N = len(boxes), rois.shape[0]
    table, bounds_all, k8_all = {}, [], []
    nb = nk = 0
    rec = np.zeros((F, N, REC_INTS), dtype=np.int32)
    for f in range(F):
        for n, (y0, x0, y1, x1) in enumerate(rois.tolist()):
            if not interests[f][n]:
                continue
            oh, ow, top, left = boxes[f][n]
            if oh < 1 or ow < 1:
                raise ValueError('frame %d object %d: output size %d x %d; height and width must be > 0' % (f, n, oh, ow))
            if top >= height or left >= width or top + oh <= 0 or left + ow <= 0:
                continue
            h, w = y1 - y0, x1 - x0
            rec[f, n, :9] = (1, y0, x0, h, w, oh, ow, top, left)
            for col, in_size, out_size in ((9, h, oh), (12, w, ow)):
                if in_size == out_size:
                    continue
                if (in_size, out_size) not in table:
                    ksize, bounds, kk = _comp.resample_tables(in_size, out_size)
                    table[(in_size, out_size)] = (nb, nk, ksize)
                    bounds_all.append(bounds.astype(np.int32))
                    k8_all.append(_comp.fixed_point(kk).reshape(-1))
                    nb += bounds.shape[0]
                    nk += k8_all[-1].shape[0]
                rec[f, n, col:col + 3] = table[(in_size, out_size)]
    bounds = np.concatenate(bounds_all) if bounds_all else np.zeros((1, 2), np.int32)
    kk8 = np.concatenate(k8_all).astype(np.int32) if k8_all else np.zeros(1, np.int32)
    return rec, bounds, kk8


def frame_json(interests, class_ids):
    """The NAME.json record of main.py:296-299: {object index + 1: {'class_id'}} for the interesting objects"""
    return {i + 1: {'class_id': int(class_ids[i])} for i in range(len(class_ids)) if interests[i]}


# ---------------------------------------------------------------------------------------------------- the session
class Frame2D:
    """One painted frame in the wire format of the textural branch: inst_u8 uint8 [1, H, W] (object index + 1), json
    {object id: {'class_id'}}, interests (host list)."""

    def __init__(self, inst_u8, json_obj, interests):
        self.inst_u8, self.json, self.interests = inst_u8, json_obj, interests

    def write(self, image_dir, name):
        """NAME.json and NAME.png (main.py:314-318; the -visualize.png overlay is not written).  Host I/O through PIL."""
        import PIL.Image
        with open(os.path.join(image_dir, '%s.json' % name), 'w') as f:
            json.dump(self.json, f, indent=4)
        PIL.Image.fromarray(self.inst_u8[0].cpu().numpy(), mode='L').save(os.path.join(image_dir, '%s.png' % name))


class Scene2D:
    """One frame's detector output for the 2D / 2D+ baselines; needs no model and no camera.

    class_ids [N], rois [N, 4] = (y0, x0, y1, x1) host sequences; masks float32 [N, 1, H, W] CUDA, binary (exactly 0.0 or
    1.0, as for SceneSession).  height / width, when given, must be the masks'.  The cover words are built once.
    Readable: class_ids, rois, cover, image_masks, height, width."""

    def __init__(self, class_ids, masks, rois, height=None, width=None):
        from sdn_hip import ops
        _scene._on_gpu(masks, 'masks')
        n = len(class_ids)
        if masks.dim() != 4 or masks.shape[1] != 1 or masks.shape[0] != n:
            raise ValueError('masks must be [%d, 1, H, W] for %d class ids, got %s' % (n, n, tuple(masks.shape)))
        H, W = int(masks.shape[2]), int(masks.shape[3])
        if (height is not None and int(height) != H) or (width is not None and int(width) != W):
            raise ValueError('the masks are %d x %d, height / width say %s x %s' % (H, W, height, width))
        self.image_masks = masks
        self._init(class_ids, ops.scene_cover(masks), rois, H, W)

    def _init(self, class_ids, cover, rois, height, width):
        n = len(class_ids)
        if n < 1 or n > 255:
            raise ValueError('%d objects; the instance map holds ids 1..255' % n)
        self.class_ids = [int(c) for c in class_ids]
        self.height, self.width = int(height), int(width)
        self.rois = check_rois(rois, self.height, self.width)
        if self.rois.shape[0] != n:
            raise ValueError('%d class ids, %d rois' % (n, self.rois.shape[0]))
        self.cover = cover
        self.n = n
        return self

    @classmethod
    def from_cover(cls, class_ids, cover, rois):
        """A session over cover words that exist already (ops.scene_cover of the N masks: int32 [ceil(N / 32), H, W])"""
        _scene._on_gpu(cover, 'cover')
        if cover.dim() != 3 or cover.shape[0] != (len(class_ids) + 31) // 32:
            raise ValueError('cover must be [%d, H, W] for %d objects, got %s'
                             % ((len(class_ids) + 31) // 32, len(class_ids), tuple(cover.shape)))
        self = cls.__new__(cls)
        self.image_masks = None
        return self._init(class_ids, cover, rois, cover.shape[1], cover.shape[2])

    @classmethod
    def from_detections(cls, image_u8, detections, mrcnn_mask, window, max_objects=16):
        """SceneSession.from_detections without the model and the camera: the `max_objects` largest detections' masks are
        unmolded on the device (sdn_unmold_masks).  image_u8 [3, H, W] gives the frame size.  Readable besides Scene2D's:
        detection_sels, scores, mask_areas."""
        from maskrcnn import detections as _det
        _scene._on_gpu(image_u8, 'image_u8')
        _scene._on_gpu(mrcnn_mask, 'mrcnn_mask')
        H, W = int(image_u8.shape[1]), int(image_u8.shape[2])
        det_host = detections.detach().cpu().numpy() if isinstance(detections, torch.Tensor) else np.asarray(detections)
        boxes, class_ids, scores, keep = _det.unmold_boxes(det_host, (H, W), window)
        if boxes.shape[0] < 1:
            raise ValueError('no detections')
        plan = _det.UnmoldPlan(mrcnn_mask, boxes, class_ids, keep, H, W)
        areas = plan.areas().cpu().numpy()
        sels = _det.select_largest(areas, max_objects)
        masks, _ = plan.masks(sels)
        self = cls(class_ids[sels], masks, boxes[sels], H, W)
        self.detection_sels, self.scores, self.mask_areas = sels, scores[sels], areas[sels]
        return self

    @classmethod
    def from_scene_gt(cls, image_u8, scene_u8, codes, class_ids, metas=None, max_objects=16):
        """SceneSession.from_scene_gt without the model and the camera (main.py:724-761, 812-818): scene_u8 uint8 [H, W, 3]
        CUDA, codes [K, 3], class_ids [K]; the `max_objects` largest are kept.  image_u8 may be None (the scene gives the
        frame size).  Readable besides Scene2D's: detection_sels, mask_areas, metas."""
        from maskrcnn import detections as _det
        masks, rois, areas = _scene.scene_gt_inputs(scene_u8, codes)
        if len(class_ids) != rois.shape[0]:
            raise ValueError('%d class ids for %d codes' % (len(class_ids), rois.shape[0]))
        if image_u8 is not None and tuple(image_u8.shape[-2:]) != tuple(masks.shape[-2:]):
            raise ValueError('image_u8 is %s, the scene %s' % (tuple(image_u8.shape[-2:]), tuple(masks.shape[-2:])))
        sels = _det.select_largest(areas, max_objects)
        if len(sels) < masks.shape[0] or not np.array_equal(sels, np.arange(len(sels))):
            masks = masks.index_select(0, torch.as_tensor(sels.copy(), dtype=torch.long).to(masks.device))
        self = cls(np.asarray(class_ids)[sels], masks, rois[sels])
        self.detection_sels, self.mask_areas = sels, areas[sels]
        self.metas = [metas[i] for i in sels.tolist()] if metas is not None else None
        return self

    @classmethod
    def from_cityscapes_gt(cls, image_u8, scene, disparity, category=26, max_objects=16):
        """SceneSession.from_cityscapes_gt without the model and the camera (main.py:763-795, 812-818): scene, disparity int32
        [H, W] CUDA; every id of `category` is an object of class 1, the `max_objects` largest are kept.  Masks and rois only:
        the baselines take no ignore maps.  image_u8 may be None (the scene gives the frame size).  Readable besides Scene2D's:
        detection_sels, mask_areas, instance_ids."""
        masks, _, rois, areas, ids, _, sels = _scene._cityscapes_gt(scene, disparity, category, max_objects, cover=False)
        if image_u8 is not None and tuple(image_u8.shape[-2:]) != tuple(masks.shape[-2:]):
            raise ValueError('image_u8 is %s, the scene %s' % (tuple(image_u8.shape[-2:]), tuple(masks.shape[-2:])))
        self = cls([1] * len(ids), masks, rois)
        self.detection_sels, self.mask_areas, self.instance_ids = sels, areas, ids
        return self

    def reference_map(self):
        """The unedited masks painted in index order (main.py:236-238, NAME-ref.png) -> uint8 [1, H, W].  No device-to-host
        copy."""
        from sdn_hip import ops
        return ops.scene_paint2d(self.cover, self.n)[0]

    def edit(self, operation_lists, use_ry=False):
        """F operation lists (the edit JSON's `operations`) -> F `Frame2D`s: main.py:256-312 with one sdn_scene_paint2d launch
        for all F.  use_ry: the 2D+ baseline (the column extent is also scaled by cos(ry)).  ValueError, before any launch,
        for an interesting object whose output size is 0 in either axis.  No device-to-host copy."""
        from sdn_hip import ops
        operation_lists = [list(o) for o in operation_lists]
        if len(operation_lists) < 1:
            raise ValueError('no operation lists')
        boxes, interests = [], []
        for ops_ in operation_lists:
            mrois, drois, keep, _ = edit_geometry(self.rois, ops_, use_ry)
            boxes.append(paste_boxes(mrois, drois))
            interests.append(keep)
        rec, bounds, kk8 = paint_tables(self.rois, boxes, interests, self.height, self.width)
        tables = _scene.upload_int32([rec, bounds, kk8], self.cover.device)
        out = ops.scene_paint2d(self.cover, self.n, rec, tables)
        return [Frame2D(out[f], frame_json(interests[f], self.class_ids), list(interests[f])) for f in range(len(operation_lists))]
