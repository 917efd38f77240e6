"""From a frame, the detector's output and edit operations to the edited frames the textural branch consumes.

Reference: geometric/scripts/main.py `_test` (:325-622) around the model, with derender3d/datasets.py:49-71
(Transforms.crop_square) and :141-172 (BaseDataset.transform_rgb / transform_mask / transform_ignore):
  :342-403  interests, per-object crops of the frame and of the masks, normalised rois, the encoder
  :405-459  the test-time optimisation: occlusion ("ignore") maps from the masks sorted by predicted depth, Adam on four keys
  :461-514  the edit: every operation of the edit JSON matched to an object, `delete` or `modify`
  :516-622  render, composite, write (derender3d/compositing.py)
The reference crops on the host (three PIL round trips per object, each mask fetched from the device) and edits with about
ten element-wise launches per operation.  Here the crops of all objects are one launch (sdn_scene_crops after the cover
pre-pass sdn_scene_cover), F edit lists are one launch (sdn_scene_edit) and one render of the stacked [F N] blob; the host
prepares only what is host data anyway (rois, Pillow's resampling tables, the JSON).  `SceneSession` is the counterpart of
textural/edit.py's `EditSession`: `SceneSession(...).edit(lists)` -> frames -> `EditSession(...).render_batch(frames)`.
`SceneSession.from_detections` starts from the detector's heads (maskrcnn/detections.py, sdn_unmold_masks) and
`SceneSession.from_scene_gt` from a ground-truth instance image (sdn_scene_gt_masks; main.py:724-761) and
`SceneSession.from_cityscapes_gt` from a Cityscapes instance-id map and its disparity map (sdn_scene_id_stats,
sdn_scene_id_planes; main.py:763-795), the one source that supplies its own ignore maps.
`SceneSession.edit_2d` paints the 2D / 2D+ baselines of the same frame (derender3d/scene2d.py; main.py:215-322).

Two quirks of the reference are kept on purpose (parity is the contract):
  * crop_square pads the right / bottom by max(0, roi end + d - size) although its window ends one pixel further when
    s - w (s - h) is odd; PIL's crop fills that column (row) with 0, not with the fill value;
  * the ignore map of SORTED POSITION j (union of the masks of the j nearest objects) is cropped with the roi of OBJECT j
    (`zip(image_ignores, rois)`, main.py:419).  `ignore_pairing='object'` gives object n the union of the objects nearer
    than n instead.

GPU only: CPU tensors raise NotImplementedError."""
import numpy as np
import torch

from derender3d import compositing as _comp

OBJ_INTS = 12      # one row of sdn_scene_crops's object table
REC_INTS = 8       # one record of sdn_scene_edit
DELETE, MODIFY = 0, 1


# ---------------------------------------------------------------------------------------------------- crops: host half
def crop_windows(rois, height, width):
    """Transforms.crop_square's window per roi (y0, x0, y1, x1) -> int32 [N, 5]: frame coordinates (y, x) of the window's
    first pixel, its side s = max(h, w), and the frame coordinates (x limit, y limit) where the padded image ends: the
    reference pads by max(0, roi[3] + dw - W) / max(0, roi[2] + dh - H), the window ends at roi[1] - dw + s, one further
    when s - w is odd, and what lies beyond the padded image is 0 (PIL's crop)."""
    rois = np.asarray(rois, dtype=np.int64).reshape(-1, 4)
    out = np.zeros((rois.shape[0], 5), dtype=np.int32)
    for i, (y0, x0, y1, x1) in enumerate(rois.tolist()):
        h, w = y1 - y0, x1 - x0
        if h < 1 or w < 1:
            raise ValueError('roi %d (%d, %d, %d, %d) is empty' % (i, y0, x0, y1, x1))
        s = max(h, w)
        dh, dw = (s - h) // 2, (s - w) // 2
        out[i] = (y0 - dh, x0 - dw, s, width + max(0, x1 + dw - width), height + max(0, y1 + dh - height))
    return out


def crop_tables(rois, height, width, image_size, mask_size):
    """The host tables of sdn_scene_crops: (objs int32 [N, 12], bounds int32 [M, 2], kk8 int32 [K]).  One Pillow table
    (compositing.resample_tables + fixed_point) per distinct (window side, output size); none when they are equal, where
    Pillow skips the resampling (ksize 0).  height, width: of the one frame, or one per roi (sdn_train_crops_mixed)."""
    rois = np.asarray(rois, dtype=np.int64).reshape(-1, 4)
    heights, widths = (np.broadcast_to(np.asarray(v, dtype=np.int64), (rois.shape[0],)) for v in (height, width))
    table, bounds_all, k8_all = {}, [], []
    nb = nk = 0
    objs = np.zeros((rois.shape[0], OBJ_INTS), dtype=np.int32)
    for i in range(rois.shape[0]):
        try:
            objs[i, :5] = crop_windows(rois[i], int(heights[i]), int(widths[i]))[0]
        except ValueError:
            raise ValueError('roi %d (%d, %d, %d, %d) is empty' % ((i,) + tuple(rois[i].tolist())))
        s = int(objs[i, 2])
        for col, size in ((5, image_size), (8, mask_size)):
            if s == size:
                continue
            if (s, size) not in table:
                ksize, bounds, kk = _comp.resample_tables(s, size)
                table[(s, size)] = (nb, nk, ksize)
                bounds_all.append(bounds.astype(np.int32))
                k8_all.append(_comp.fixed_point(kk).reshape(-1))
                nb += bounds.shape[0]
                nk += k8_all[-1].shape[0]
            objs[i, col:col + 3] = table[(s, size)]
    bounds = np.concatenate(bounds_all) if bounds_all else np.zeros((1, 2), np.int32)
    kk8 = np.concatenate(k8_all).astype(np.int32) if k8_all else np.zeros(1, np.int32)
    return objs, bounds, kk8


def upload_int32(arrays, device):
    """Several int32 host arrays as ONE pinned blob and one host-to-device copy (as composite_frame.flush) -> device views."""
    flat = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in arrays]
    blob = torch.from_numpy(np.concatenate(flat)).pin_memory().to(device, non_blocking=True)
    out, off = [], 0
    for a, f in zip(arrays, flat):
        out.append(blob[off:off + f.size].view(np.asarray(a).shape))
        off += f.size
    return out


def roi_norms_host(rois, camera):
    """main.py:375-393 in float32 on the host (the rois are host data): roi_norms [N, 4], _mroi_norms, _droi_norms [N, 2]."""
    r = torch.as_tensor(np.asarray(rois, dtype=np.int32).reshape(-1, 4))
    roi_norms = (r.float() - torch.tensor([camera.v0, camera.u0, camera.v0, camera.u0])) / camera.focal
    mroi = torch.stack([roi_norms[:, 2] + roi_norms[:, 0], roi_norms[:, 3] + roi_norms[:, 1]], dim=1) / 2.0
    droi = torch.stack([roi_norms[:, 2] - roi_norms[:, 0], roi_norms[:, 3] - roi_norms[:, 1]], dim=1)
    return roi_norms, mroi, droi


# ---------------------------------------------------------------------------------------------------- crops: device half
class CropPlan:
    """The rois of one frame with their uploaded tables; shared by the image / mask call and the ignore call."""

    def __init__(self, rois, height, width, image_size, mask_size, device):
        self.rois = np.ascontiguousarray(np.asarray(rois, dtype=np.int32).reshape(-1, 4))
        if self.rois.shape[0] < 1:
            raise ValueError('no rois')
        self.height, self.width, self.image_size, self.mask_size = height, width, image_size, mask_size
        self.tables = upload_int32(crop_tables(self.rois, height, width, image_size, mask_size), device)
        self.n = self.rois.shape[0]


def _on_gpu(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise NotImplementedError('%s is on %s; the scene inputs are made on the GPU only (no CPU fallback)' % (name, t.device))


def image_mask_crops(plan, image_u8, masks, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25)):
    """main.py:365-373 for all objects: (rgbs [N,3,S_i,S_i], masks [N,1,S_m,S_m], cover).  image_u8 uint8 [3,H,W], masks
    [N,1,H,W] float32, BINARY (exactly 0.0 or 1.0 -- the reference's np.uint8(mask * 255) of anything else is not
    reproduced).  `cover` (the masks as one bit per object and pixel) is what `ignore_crops` takes.  No device-to-host copy."""
    from sdn_hip import ops
    _on_gpu(image_u8, 'image_u8')
    _on_gpu(masks, 'masks')
    if masks.dim() != 4 or tuple(masks.shape) != (plan.n, 1, plan.height, plan.width):
        raise ValueError('masks must be [%d, 1, %d, %d] for %d rois, got %s'
                         % (plan.n, plan.height, plan.width, plan.n, tuple(masks.shape)))
    cover = ops.scene_cover(masks)
    rgbs, crops, _ = ops.scene_crops(ops.SCENE_RGB | ops.SCENE_MASK, plan.rois, plan.tables, plan.height, plan.width,
                                     plan.image_size, plan.mask_size, frame_u8=image_u8, cover=cover, mean=mean, std=std)
    return rgbs, crops, cover


def _object_bits(index):
    """int64 [len, ceil(len / 32)]: row k holds bit (index[k] & 31) in word index[k] // 32"""
    n = index.shape[0]
    one = torch.zeros(n, (n + 31) // 32, dtype=torch.int64, device=index.device)
    return one.scatter_(1, (index >> 5)[:, None], torch.ones_like(index)[:, None] << (index & 31)[:, None])


def nearer_words(order, pairing='reference'):
    """Per ignore slot the set of objects whose masks it unites, as words for sdn_scene_crops: int64 [N, ceil(N / 32)].
    order: int64 [N] CUDA, the objects near to far (main.py:408).  'reference': slot j = the objects order[0..j-1]
    (main.py:409-414; the slot is then cropped with rois[j], :419); 'object': slot n = the objects nearer than object n."""
    if pairing not in ('reference', 'object'):
        raise ValueError("ignore_pairing must be 'reference' or 'object', got %r" % (pairing,))
    one = _object_bits(order)
    before = torch.cumsum(one, dim=0) - one      # the bits are distinct: the sum is the union
    if pairing == 'object':
        before = torch.zeros_like(before).index_copy_(0, order, before)
    return before


def ignore_crops(plan, cover, log_depths=None, droi_norms=None, pairing='reference', image_ignores=None, ignore_cover=None):
    """main.py:405-421 for all objects -> ignores [N,1,S_m,S_m].  Either the depth order (log_depths [N,1], droi_norms [N,2]:
    sorted on the device, stable, ties keep index order) over the masks' `cover`, or caller-supplied binary image_ignores
    [N,1,H,W] (main.py:416), or the same maps as cover words already (ignore_cover int32 [ceil(N / 32), H, W]: bit n = map n,
    as ops.scene_cover(image_ignores) would make them; not both).  No device-to-host copy."""
    from sdn_hip import ops
    if image_ignores is not None and ignore_cover is not None:
        raise ValueError('image_ignores and ignore_cover are the same maps in two forms: pass one of them')
    if image_ignores is not None or ignore_cover is not None:
        if image_ignores is not None:
            _on_gpu(image_ignores, 'image_ignores')
            if tuple(image_ignores.shape) != (plan.n, 1, plan.height, plan.width):
                raise ValueError('image_ignores must be [%d, 1, %d, %d], got %s'
                                 % (plan.n, plan.height, plan.width, tuple(image_ignores.shape)))
            icover = ops.scene_cover(image_ignores)
        else:
            _on_gpu(ignore_cover, 'ignore_cover')
            if ignore_cover.dtype != torch.int32 or tuple(ignore_cover.shape) != ((plan.n + 31) // 32, plan.height, plan.width):
                raise ValueError('ignore_cover must be int32 [%d, %d, %d], got %s %s'
                                 % ((plan.n + 31) // 32, plan.height, plan.width, ignore_cover.dtype, tuple(ignore_cover.shape)))
            icover = ignore_cover
        nearer = _object_bits(torch.arange(plan.n, device=icover.device))     # slot n = map n alone
    else:
        _on_gpu(log_depths, 'log_depths')
        if log_depths.numel() != plan.n or tuple(droi_norms.shape) != (plan.n, 2):
            raise ValueError('log_depths must be [%d, 1] and droi_norms [%d, 2]' % (plan.n, plan.n))
        depths = log_depths.detach().reshape(-1, 1) - torch.sum(torch.log(droi_norms.detach()), dim=1, keepdim=True)
        order = torch.sort(depths, dim=0, stable=True)[1].reshape(-1)
        icover, nearer = cover, nearer_words(order, pairing)
    return ops.scene_crops(ops.SCENE_IGNORE, plan.rois, plan.tables, plan.height, plan.width, plan.image_size, plan.mask_size,
                           ignore_cover=icover, nearer=nearer)[2]


def scene_gt_inputs(scene_u8, codes):
    """main.py:745-746 for K objects in one launch: (masks float32 [K, 1, H, W] CUDA, rois numpy int32 [K, 4], areas numpy
    int32 [K]) of an instance-colour image scene_u8 uint8 [H, W, 3] CUDA and K colour codes [K, 3] (host sequence or CUDA
    uint8).  One device-to-host copy (5 K integers).  IndexError for a code that matches no pixel: Transforms.mask_to_roi
    (derender3d/datasets.py:95-103) indexes an empty array there."""
    from sdn_hip import ops
    _on_gpu(scene_u8, 'scene_u8')
    if not isinstance(codes, torch.Tensor):
        codes = torch.from_numpy(np.ascontiguousarray(np.asarray(codes).astype(np.uint8).reshape(-1, 3))).to(scene_u8.device)
    masks, rois, areas = ops.scene_gt_masks(scene_u8, codes)
    packed = torch.cat([rois, areas[:, None]], dim=1).cpu().numpy()
    rois, areas = np.ascontiguousarray(packed[:, :4]), np.ascontiguousarray(packed[:, 4])
    empty = np.where(areas == 0)[0]
    if empty.size:
        raise IndexError('code %d (%s) matches no pixel of the scene' % (int(empty[0]), codes[int(empty[0])].tolist()))
    return masks, rois, areas



# ---------------------------------------------------------------------------------------------------- Cityscapes ground truth
class CityscapesCamera:
    """derender3d/datasets.py:788-791, the one camera the reference uses for every Cityscapes frame"""
    focal = 2250.0
    u0 = 925.0
    v0 = 460.0


def percentile95_threshold(n, lo, hi):
    """floor(np.percentile(values, 95)) from the two order statistics it interpolates between, for arrays of objects: n the
    number of values, lo / hi those of rank floor((n - 1) 0.95) and the next (sdn_scene_id_stats) -> int32 thr; 0 where n == 0
    (main.py:778).  float64, operation for operation numpy's default `linear` method (lib/_function_base_impl.py: _lerp): the
    rounding of lo + (hi - lo) g decides pixels where it lands on an integer.  The disparities are integers, so
    `disparity > percentile` is `disparity > thr`."""
    n = np.asarray(n, dtype=np.int64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = (n - 1) * np.true_divide(95, 100)
    g = v - np.floor(v)
    d = hi - lo
    t = lo + d * g
    t = np.where(g >= 0.5, hi - d * (1 - g), t)
    t = np.where(d == 0, lo, t)
    return np.where(n > 0, np.floor(t), 0).astype(np.int32)


def _cityscapes_select(scene, disparity, category, max_objects):
    """the statistics of every id of the category, ONE device-to-host copy (the table), and the host's part of main.py:766-780,
    812: (sels, ids, rois, areas, thr) of the `max_objects` largest, largest first, numpy; sels are positions among the present
    ids in ascending order, the rest int32"""
    from maskrcnn import detections as _det
    from sdn_hip import ops
    _on_gpu(scene, 'scene')
    _on_gpu(disparity, 'disparity')
    table = ops.scene_id_stats(scene, disparity, category).cpu().numpy()
    present = np.flatnonzero(table[:, 0] > 0)                     # ascending ids: np.unique's order
    if present.size == 0:
        raise ValueError('no object of category %d in the scene' % category)    # the reference's np.stack([]) raises
    sels = _det.select_largest(table[present, 0].astype(np.float32), max_objects)    # float32 sums, as main.py:812 sorts them
    rows = table[present[sels]]
    ids = (present[sels] + 1000 * int(category)).astype(np.int32)
    thr = percentile95_threshold(rows[:, 5], rows[:, 6], rows[:, 7])
    return sels, ids, np.ascontiguousarray(rows[:, 1:5]), np.ascontiguousarray(rows[:, 0]), thr


def cityscapes_gt_inputs(scene, disparity, category=26, max_objects=16):
    """main.py:763-795, 812-818 without the maps leaving the device: scene int32 [H, W] CUDA, the instance-id map (id =
    category * 1000 + k); disparity int32 [H, W] CUDA, a 16-bit map's values.  sdn_scene_id_stats, one device-to-host copy
    (the table), on the host the present ids in ascending order, the `max_objects` largest masks and their thresholds, one
    upload (ids and thr), one sdn_scene_id_planes launch.  Returns (masks float32 [n, 1, H, W] CUDA, ignore_cover int32
    [ceil(n / 32), H, W] CUDA: bit k = disparity > percentile 95 of object k's non-zero disparities, rois, areas, ids, thr:
    numpy int32) of the selected objects, largest first.  ValueError when the scene holds no object of the category."""
    return _cityscapes_gt(scene, disparity, category, max_objects)[:6]


def _cityscapes_gt(scene, disparity, category, max_objects, cover=True):
    from sdn_hip import ops
    sels, ids, rois, areas, thr = _cityscapes_select(scene, disparity, category, max_objects)
    ids_d, thr_d = upload_int32([ids, thr], scene.device)
    masks, words, _ = ops.scene_id_planes(scene, disparity, ids_d, thr_d, cover=cover)
    return masks, words, rois, areas, ids, thr, sels


# ---------------------------------------------------------------------------------------------------- edit: host half
def match_operations(mroi_norms, operations, camera):
    """main.py:468-479: [(object index, operation index)] in the reference's iteration order.  mroi_norms: float32 [N, 2]
    host tensor (roi_norms_host)."""
    ops_ = torch.tensor([[(float(op['from']['v']) - camera.v0) / camera.focal,
                          (float(op['from']['u']) - camera.u0) / camera.focal] for op in operations])
    mroi = torch.as_tensor(mroi_norms, dtype=torch.float32)
    diffs = torch.sum((mroi[:, None, :] - ops_[None, :, :]) ** 2, dim=2)
    if len(mroi) < len(ops_):
        return [(i, int(j)) for i, j in enumerate(torch.argmin(diffs, dim=1))]
    return [(int(i), j) for j, i in enumerate(torch.argmin(diffs, dim=0))]


def edit_records(operation_lists, mroi_norms, camera):
    """The records of sdn_scene_edit for F operation lists: int32 [F, P, 8] (P = the longest list of pairs, at least 1;
    object -1 marks an unused slot) and the matched pairs per list.  The transcendental values are computed as the
    reference does, on CPU float32 tensors (main.py:502-506)."""
    pairs = [match_operations(mroi_norms, ops_, camera) if ops_ else [] for ops_ in operation_lists]
    P = max([len(p) for p in pairs] + [1])
    rec = np.zeros((len(pairs), P, REC_INTS), dtype=np.int32)
    rec[:, :, 0] = -1
    recf = rec.view(np.float32)
    for f, (ops_, pp) in enumerate(zip(operation_lists, pairs)):
        for k, (obj, j) in enumerate(pp):
            op = ops_[j]
            u, v = float(op['from']['u']), float(op['from']['v'])
            rec[f, k, 0] = obj
            if op['type'] == 'delete':
                rec[f, k, 1] = DELETE
            elif op['type'] == 'modify':
                u, v = float(op['to'].get('u', u)), float(op['to'].get('v', v))
                centre = torch.tensor([(v - camera.v0) / camera.focal, (u - camera.u0) / camera.focal])
                rec[f, k, 1] = MODIFY
                recf[f, k, 2:4] = centre.numpy()
                recf[f, k, 4] = (2 * torch.log(torch.tensor(float(op['zoom'])))).item()
                recf[f, k, 5] = torch.cos(torch.tensor(-float(op['ry']))).item()
                recf[f, k, 6] = torch.sin(torch.tensor(-float(op['ry']))).item()
            else:    # the reference ignores other types silently (:488-491); so does the kernel for an unused slot
                rec[f, k, 0] = -1
    return rec, pairs


# ---------------------------------------------------------------------------------------------------- the session
class Frame:
    """One composited frame in the wire format of the textural branch: inst_u8 [1,H,W], json {object id: record},
    normal_u8 [3,H,W], depth_i32 [1,H,W] (a 16-bit PNG's values), interests (host list).  The float maps are kept for
    `write`."""

    def __init__(self, maps, json_obj, interests):
        self.maps = maps
        self.inst_u8, self.normal_u8, self.depth_i32 = _comp.wire_tensors(*maps)
        self.json, self.interests = json_obj, interests

    def write(self, image_dir, name):
        _comp.write_frame(image_dir, name, self.maps[0], self.maps[1], self.maps[2], self.json)


_OPT_KEYS = ('_theta_deltas', '_translation2ds', '_log_scales', '_ffd_coeffs')
_ENCODER_KEYS = ('_theta_deltas', '_translation2ds', '_log_scales', '_log_depths', '_class_probs', '_ffd_coeffs')


class SceneSession:
    """One frame and the detector's output for it; de-rendered at construction.

    model      a Derenderer3d in eval() and reproject mode
    camera     anything with focal, u0, v0 (the reference's dataset.Camera)
    image_u8   uint8 [3, H, W] CUDA;  masks float32 [N, 1, H, W] CUDA, binary;  class_ids [N], rois [N, 4] host sequences
    image_ignores  optional binary [N, 1, H, W] CUDA occlusion maps instead of the depth order (main.py:416)
    ignore_cover   the same maps as cover words, int32 [ceil(N / 32), H, W] CUDA (cityscapes_gt_inputs); not both
    ignore_pairing 'reference' (sorted position j with roi j, main.py:419) or 'object'
    mask_areas optional host sequence [N]: the pixel count of every mask, where the caller has it (from_detections,
               from_scene_gt); the interest test then reads it instead of summing the planes
    Readable: rgbs, masks, ignores (the crops), blob, interests (host list of bool), image_masks."""

    def __init__(self, model, camera, image_u8, class_ids, masks, rois, image_ignores=None, all_interested=False,
                 mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), image_size=224, mask_size=256, ignore_pairing='reference',
                 metas=None, mask_areas=None, ignore_cover=None):
        if image_ignores is not None and ignore_cover is not None:
            raise ValueError('image_ignores and ignore_cover are the same maps in two forms: pass one of them')
        _on_gpu(image_u8, 'image_u8')
        _on_gpu(masks, 'masks')
        if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[0] != 3:
            raise ValueError('image_u8 must be uint8 [3, H, W], got %s %s' % (image_u8.dtype, tuple(image_u8.shape)))
        n = len(class_ids)
        rois = np.asarray(rois, dtype=np.int32).reshape(-1, 4)
        if n < 1 or rois.shape[0] != n or masks.shape[0] != n:
            raise ValueError('%d class ids, %d rois, %d masks' % (n, rois.shape[0], masks.shape[0]))
        if ignore_pairing not in ('reference', 'object'):
            raise ValueError("ignore_pairing must be 'reference' or 'object', got %r" % (ignore_pairing,))
        dev = image_u8.device
        self.model, self.camera, self.metas = model, camera, metas
        self.class_ids = [int(c) for c in class_ids]
        self.height, self.width = int(image_u8.shape[1]), int(image_u8.shape[2])
        self.image_masks = masks
        self.plan = CropPlan(rois, self.height, self.width, image_size, mask_size, dev)
        roi_norms, mroi, droi = roi_norms_host(rois, camera)
        self.mroi_norms_host = mroi
        packed = torch.cat([roi_norms, mroi, droi], dim=1).pin_memory().to(dev, non_blocking=True)
        self.rgbs, self.masks, self.cover = image_mask_crops(self.plan, image_u8, masks, mean, std)
        blob = {'_roi_norms': packed[:, 0:4].contiguous(), '_mroi_norms': packed[:, 4:6].contiguous(),
                '_droi_norms': packed[:, 6:8].contiguous(), '_focals': torch.full((n, 1), float(camera.focal), device=dev)}
        with torch.no_grad():
            blob.update(model.derenderer(self.rgbs, blob['_mroi_norms'], blob['_droi_norms']))
        self.blob = blob
        # main.py:347-355; the one device-to-host copy of the construction, issued after the encoder is queued
        if all_interested:
            self.interests = [True] * n
        elif mask_areas is not None:
            if len(mask_areas) != n:
                raise ValueError('%d mask areas for %d objects' % (len(mask_areas), n))
            self.interests = [c in (1, 2) and int(a) > 16 * 16 for c, a in zip(self.class_ids, mask_areas)]
        else:
            big = (masks.sum(dim=3).sum(dim=2).reshape(-1) > 16 * 16).cpu().tolist()
            self.interests = [c in (1, 2) and bool(b) for c, b in zip(self.class_ids, big)]
        self._interests_dev = torch.tensor(self.interests, dtype=torch.uint8).to(dev)
        self.ignore_pairing = ignore_pairing
        self.ignores = ignore_crops(self.plan, self.cover, blob['_log_depths'], blob['_droi_norms'], ignore_pairing,
                                    image_ignores=image_ignores, ignore_cover=ignore_cover)
        self._stacked = {}
        self.last_losses = None

    # ------------------------------------------------------------------------------------------------ from the detector
    @classmethod
    def from_detections(cls, model, camera, image_u8, detections, mrcnn_mask, window, max_objects=16, **kwargs):
        """The session of a frame from what the detector's heads emit (maskrcnn/model.py:1636: detections [D, 6] in the
        molded image's pixels, mrcnn_mask float32 [D, C, Mh, Mw], both CUDA) and the molded image's `window`
        (maskrcnn.detections.mold_window): model.py:1638-1653, 2084-2143 and main.py:797-818 without the masks leaving the
        device.  The D x 6 table goes to the host for the box arithmetic; one sdn_unmold_masks launch counts the pixels of
        every detection's mask (D integers to the host), the `max_objects` largest are selected as main.py:812 does, and a
        second launch writes the planes of those only.  ValueError without a detection or for a box that leaves the frame
        (the reference skips such a frame, main.py:809).  Readable besides SceneSession's: detection_sels (indices among the
        surviving detections, largest first), rois, scores, mask_areas."""
        from maskrcnn import detections as _det
        _on_gpu(image_u8, 'image_u8')
        _on_gpu(mrcnn_mask, 'mrcnn_mask')
        H, W = int(image_u8.shape[1]), int(image_u8.shape[2])
        det_host = detections.detach().cpu().numpy() if isinstance(detections, torch.Tensor) else np.asarray(detections)
        boxes, class_ids, scores, keep = _det.unmold_boxes(det_host, (H, W), window)
        if boxes.shape[0] < 1:
            raise ValueError('no detections')
        plan = _det.UnmoldPlan(mrcnn_mask, boxes, class_ids, keep, H, W)
        areas = plan.areas().cpu().numpy()
        sels = _det.select_largest(areas, max_objects)
        masks, _ = plan.masks(sels)
        self = cls(model, camera, image_u8, class_ids[sels], masks, boxes[sels], mask_areas=areas[sels], **kwargs)
        self.detection_sels, self.rois, self.scores, self.mask_areas = sels, boxes[sels], scores[sels], areas[sels]
        return self

    @classmethod
    def from_scene_gt(cls, model, camera, image_u8, scene_u8, codes, class_ids, metas=None, max_objects=16, **kwargs):
        """The session of a frame from ground truth (main.py:724-761, 812-818): scene_u8 uint8 [H, W, 3] CUDA, the instance-
        colour image; codes [K, 3] the objects' colours (host or CUDA), class_ids [K], metas optional list [K].  One
        sdn_scene_gt_masks launch makes the K masks, rois and pixel counts (5 K integers to the host); the `max_objects`
        largest are kept.  IndexError for a code that matches no pixel, as Transforms.mask_to_roi."""
        masks, rois, areas = scene_gt_inputs(scene_u8, codes)
        if len(class_ids) != rois.shape[0]:
            raise ValueError('%d class ids for %d codes' % (len(class_ids), rois.shape[0]))
        from maskrcnn import detections as _det
        sels = _det.select_largest(areas, max_objects)
        class_ids = np.asarray(class_ids)[sels]
        metas = [metas[i] for i in sels.tolist()] if metas is not None else None
        if len(sels) < masks.shape[0] or not np.array_equal(sels, np.arange(len(sels))):
            masks = masks.index_select(0, torch.as_tensor(sels.copy(), dtype=torch.long).to(masks.device))
        self = cls(model, camera, image_u8, class_ids, masks, rois[sels], metas=metas, mask_areas=areas[sels], **kwargs)
        self.detection_sels, self.rois, self.mask_areas = sels, rois[sels], areas[sels]
        return self

    @classmethod
    def from_cityscapes_gt(cls, model, camera, image_u8, scene, disparity, category=26, max_objects=16, **kwargs):
        """The session of a frame from Cityscapes ground truth (main.py:763-795, 812-818): scene int32 [H, W] CUDA, the
        instance-id map; disparity int32 [H, W] CUDA.  Every id of `category` (26: cars) is an object of class 1; the
        `max_objects` largest are kept; each object's ignore map is disparity > percentile 95 of its own non-zero disparities
        (cityscapes_gt_inputs).  camera: CityscapesCamera for the dataset's frames.  ValueError without an object.  Readable
        besides SceneSession's: detection_sels (positions among the present ids in ascending order, largest first), rois,
        mask_areas, instance_ids, ignore_thresholds."""
        masks, cover, rois, areas, ids, thr, sels = _cityscapes_gt(scene, disparity, category, max_objects)
        self = cls(model, camera, image_u8, [1] * len(ids), masks, rois, mask_areas=areas, ignore_cover=cover, **kwargs)
        self.rois, self.mask_areas, self.instance_ids, self.ignore_thresholds = rois, areas, ids, thr
        self.detection_sels = sels
        return self

    # ------------------------------------------------------------------------------------------------ optimisation
    @staticmethod
    def _pad_like(image, like, mode='constant'):
        """Transforms.pad_like (datasets.py:28-33)"""
        p2, p3 = like.shape[2] - image.shape[2], like.shape[3] - image.shape[3]
        return torch.nn.functional.pad(image, (p3 // 2, p3 // 2, p2 // 2, p2 // 2), mode=mode)

    def optimize(self, num_opts, lr=3e-2):
        """main.py:405-459: Adam on the pose delta, 2-D offset, log scale and FFD coefficients against the mask crops,
        occluded pixels ignored.  Returns the losses of the iterations (read back once, after the loop)."""
        from derender3d.losses import silhouette_ffd_loss
        model = self.model
        was_training, was_no_sample = model.training, model._force_no_sample
        losses = []
        model.train()
        model._force_no_sample = True
        try:
            blob = self.blob
            for key in _ENCODER_KEYS:
                blob[key] = blob[key].clone().detach()
            params = [blob[key].requires_grad_() for key in _OPT_KEYS]
            optimizer = torch.optim.Adam(params, lr=lr)
            target = ignores = None
            for _ in range(num_opts):
                optimizer.zero_grad()
                blob.update(model.render(blob))
                rendered = blob['_masks']
                if target is None:
                    target = self._pad_like(self.masks, rendered)
                    ignores = self._pad_like(self.ignores, rendered, mode='replicate')
                loss = silhouette_ffd_loss(rendered, target, blob['_ffd_coeffs'], ignores)
                loss.backward()
                optimizer.step()
                losses.append(loss.detach())
        finally:
            model.train(was_training)
            model._force_no_sample = was_no_sample
            for key in _OPT_KEYS:
                self.blob[key] = self.blob[key].detach()
        self.last_losses = torch.stack(losses).cpu().tolist() if losses else []
        return self.last_losses

    # ------------------------------------------------------------------------------------------------ edit / reconstruct
    def _stack(self, F):
        """the blob's rows repeated for F frames; the focal lengths are kept per F (Derenderer3d caches the viewing angles
        for as long as it is handed the same tensor, and reads them back otherwise)"""
        keys = ('_roi_norms', '_mroi_norms', '_droi_norms', '_log_scales', '_class_probs', '_ffd_coeffs')
        rep = {k: self.blob[k].detach().unsqueeze(0).expand(F, *self.blob[k].shape).reshape(F * self.plan.n, *self.blob[k].shape[1:])
               for k in keys}
        if F not in self._stacked:
            self._stacked[F] = self.blob['_focals'].repeat(F, 1)
        rep['_focals'] = self._stacked[F]
        return rep

    def _frames(self, blob, interests, F, paste_masks):
        n = self.plan.n
        cam = self.camera
        hs = _comp.host_state(blob['_depths'].reshape(F, n, 1), blob['_zooms'].reshape(F, n), blob['_center2ds'].reshape(F, n, 2),
                              blob['_alphas'].reshape(F, n))          # the one device-to-host copy for all F frames
        R = blob['_masks'].shape[-1]
        frames = []
        for f in range(F):
            rows = slice(f * n, (f + 1) * n)
            inst, nrm, dep, order = _comp.composite_frame(
                blob['_masks'][rows], blob['_normals'][rows], blob['_depth_maps'][rows], blob['_depths'][rows], blob['_zooms'][rows],
                blob['_center2ds'][rows], interests[f], cam.focal, cam.u0, cam.v0, self.height, self.width, R,
                image_masks=self.image_masks if paste_masks else None, host=hs[f])
            js = _comp.frame_json(order, interests[f], self.class_ids, hs[f][:, 0], hs[f][:, 4], self.metas)
            frames.append(Frame((inst, nrm, dep), js, list(interests[f])))
        return frames

    def edit(self, operation_lists):
        """F operation lists (the edit JSON's `operations`) -> F `Frame`s: main.py:461-622 with one
        sdn_scene_edit launch and one render for all F.  A non-interesting object is dropped (also for an empty list:
        `operations == []` is not None at main.py:604).  [(fr.inst_u8, fr.json, fr.normal_u8) for fr in frames] is what
        EditSession.render_batch takes."""
        from sdn_hip import ops
        operation_lists = [list(o) for o in operation_lists]
        F, n = len(operation_lists), self.plan.n
        if F < 1:
            raise ValueError('no operation lists')
        records, pairs = edit_records(operation_lists, self.mroi_norms_host, self.camera)
        interests = []
        for ops_, pp in zip(operation_lists, pairs):
            row = list(self.interests)
            for obj, j in pp:
                if ops_[j]['type'] == 'delete':
                    row[obj] = False
            interests.append(row)
        b = self.blob
        dev = b['_log_depths'].device
        (rec_d,) = upload_int32([records], dev)
        with torch.no_grad():
            theta, trans, logd, self.last_interests = ops.scene_edit(b['_theta_deltas'].detach(), b['_translation2ds'].detach(),
                                                                     b['_log_depths'].detach(), b['_mroi_norms'], b['_droi_norms'],
                                                                     self._interests_dev, rec_d)
            blob = self._stack(F)
            blob['_theta_deltas'] = theta.reshape(F * n, 2)
            blob['_translation2ds'] = trans.reshape(F * n, 2)
            blob['_log_depths'] = logd.reshape(F * n, 1)
            blob.update(self.model.render(blob))
        self.last_blob = blob
        return self._frames(blob, interests, F, paste_masks=False)

    def edit_2d(self, operation_lists, use_ry=False):
        """The 2D (use_ry: 2D+) baseline of the same frame (main.py:215-322; derender3d/scene2d.py): F operation lists -> F
        `Frame2D`s painted from this session's cover words.  All objects are interesting there, whatever `interests` says."""
        from derender3d import scene2d
        return scene2d.Scene2D.from_cover(self.class_ids, self.cover, self.plan.rois).edit(operation_lists, use_ry)

    def reconstruct(self):
        """The reference's `operations=None`: no edit; the detector masks of non-interesting objects are pasted
        (main.py:604-607).  -> one Frame."""
        with torch.no_grad():
            blob = dict(self.blob)
            blob.update(self.model.render({k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in self.blob.items()}))
        self.last_blob = blob
        return self._frames(blob, [list(self.interests)], 1, paste_masks=True)[0]
