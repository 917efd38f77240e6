"""From the detector heads to the scene inputs: the tail of MaskRCNN.detect on the device.

Reference: geometric/maskrcnn/model.py:1638-1653 (detect copies `detections` and `mrcnn_mask` to the host), :2084-2143
(unmold_detections), maskrcnn/utils.py:378-395 (unmold_mask: scipy.misc.imresize to the box, >= 0.5, paste) and :292-320
(resize_image's window), geometric/scripts/main.py:805-818 (layout, the 16 largest).  The reference resizes every soft mask
with PIL on the host, stacks D full-frame uint8 planes, sums them all and uploads the survivors as float32.

Here the box arithmetic stays on the host, in the reference's number formats (`unmold_boxes`: D x 6 numbers) and the masks never leave
the device: one sdn_unmold_masks launch (csrc/scene_masks.hip) makes all planes, bit-identical to the host path, and counts
their pixels.  `derender3d.scene.SceneSession.from_detections` runs it twice -- areas of all detections, then planes of the
selected ones only.

GPU only for the masks: CPU tensors raise NotImplementedError."""
import numpy as np
import torch

from derender3d import compositing as _comp

OBJ_INTS = 12      # one row of sdn_unmold_masks's object table


def mold_window(image_shape, min_dim, max_dim):
    """Where the image lies in the detector's max_dim x max_dim input, and by how much it was scaled: the `window`
    (y1, x1, y2, x2) and `scale` that utils.resize_image(image, min_dim, max_dim, padding=True) reports (utils.py:292-320),
    from the sizes alone.  The image is enlarged, never reduced, until its short side reaches min_dim; if its long side would
    then pass max_dim (Python's round, as there) the factor becomes max_dim / long side; the scaled image (sides rounded the
    same way) is centred, the odd pixel of padding going to the bottom / right."""
    if not max_dim:
        raise ValueError('max_dim is needed: the detector input is the max_dim x max_dim padded square')
    rows, cols = int(image_shape[0]), int(image_shape[1])
    short, long_side = min(rows, cols), max(rows, cols)
    factor = 1
    if min_dim and min_dim > short:
        factor = min_dim / short
    if round(long_side * factor) > max_dim:
        factor = max_dim / long_side
    if factor != 1:
        rows, cols = round(rows * factor), round(cols * factor)
    top, left = (max_dim - rows) // 2, (max_dim - cols) // 2
    return (top, left, top + rows, left + cols), factor


def unmold_boxes(detections_host, image_shape, window):
    """The host half of MaskRCNN.unmold_detections (model.py:2101-2132): detections_host numpy [D, 6] = (y1, x1, y2, x2,
    class_id, score) in the molded image's pixels, rows of zeros behind the last detection.  The arithmetic is the
    reference's: the detections end at the first row whose class id is 0; a corner is (corner - window origin) * factor in
    float64 with factor = min(H / window height, W / window width), cut to int32 toward zero; boxes whose height x width is
    not positive are dropped.  Returns (boxes int32 [N, 4] in image pixels, class_ids int32 [N], scores [N], keep int [N]:
    the rows of `detections_host` -- and of mrcnn_mask -- that survive)."""
    table = np.asarray(detections_host)
    win = np.asarray(window)
    background = np.flatnonzero(table[:, 4] == 0)
    count = int(background[0]) if background.size else table.shape[0]
    factor = min(image_shape[0] / (win[2] - win[0]), image_shape[1] / (win[3] - win[1]))
    origin = np.tile(win[:2], 2)                                     # (y, x, y, x), integers: the difference is float64
    boxes = ((table[:count, :4] - origin) * factor).astype(np.int32)
    alive = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 0
    keep = np.flatnonzero(alive)
    return boxes[keep], table[:count, 4].astype(np.int32)[keep], table[:count, 5][keep], keep


def select_largest(areas, limit=16):
    """main.py:812 on the pixel counts: the indices of the `limit` largest masks, largest first (ties as numpy puts them)."""
    areas = np.asarray(areas)
    return np.flipud(np.argsort(areas))[:min(len(areas), limit)]


def check_boxes(boxes, class_ids, height, width, num_classes):
    """The reference's `full_mask[y1:y2, x1:x2] = mask` (utils.py:394) raises for a box that leaves the frame -- a negative
    coordinate or one beyond the size changes the slice's shape -- and main.py:809 skips the frame; its fancy index raises
    for a class outside mrcnn_mask (model.py:2110).  ValueError for both."""
    for i, (y1, x1, y2, x2) in enumerate(np.asarray(boxes).reshape(-1, 4).tolist()):
        if y1 < 0 or x1 < 0 or y2 > height or x2 > width:
            raise ValueError('detection %d: box (%d, %d, %d, %d) leaves the %d x %d frame' % (i, y1, x1, y2, x2, height, width))
        if y2 <= y1 or x2 <= x1:
            raise ValueError('detection %d: box (%d, %d, %d, %d) is empty' % (i, y1, x1, y2, x2))
    ids = np.asarray(class_ids)
    if ids.size and (ids.min() < 0 or ids.max() >= num_classes):
        raise ValueError('class ids %d .. %d outside the %d class planes of mrcnn_mask' % (ids.min(), ids.max(), num_classes))


def unmold_tables(boxes, class_ids, keep, mask_h, mask_w):
    """The host tables of sdn_unmold_masks: (objs int32 [N, 12], bounds int32 [M, 2], kk8 int32 [K]).  A row of objs:
    (detection index, class id, y1, x1, y2, x2), then (first row of bounds, first element of kk8, ksize) of the resize of the
    rows mask_h -> y2 - y1 and the same of the columns mask_w -> x2 - x1; ksize 0 where the sizes are equal and Pillow skips
    the pass.  One Pillow table (compositing.resample_tables + fixed_point) per distinct (mask side, box side)."""
    boxes = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    objs = np.zeros((boxes.shape[0], OBJ_INTS), dtype=np.int32)
    objs[:, 0], objs[:, 1], objs[:, 2:6] = keep, class_ids, boxes
    table, bounds_all, k8_all = {}, [], []
    nb = nk = 0
    for i, (y1, x1, y2, x2) in enumerate(boxes.tolist()):
        for col, src, size in ((6, mask_h, y2 - y1), (9, mask_w, x2 - x1)):
            if size < 1:
                raise ValueError('box %d (%d, %d, %d, %d) is empty' % (i, y1, x1, y2, x2))
            if src == size:
                continue
            if (src, size) not in table:
                ksize, bounds, kk = _comp.resample_tables(src, size)
                table[(src, size)] = (nb, nk, ksize)
                bounds_all.append(bounds.astype(np.int32))
                k8_all.append(_comp.fixed_point(kk).reshape(-1))
                nb += bounds.shape[0]
                nk += k8_all[-1].shape[0]
            objs[i, col:col + 3] = table[(src, size)]
    bounds = np.concatenate(bounds_all) if bounds_all else np.zeros((1, 2), np.int32)
    kk8 = np.concatenate(k8_all).astype(np.int32) if k8_all else np.zeros(1, np.int32)
    return objs, bounds, kk8


def _upload_int32(arrays, device):
    """several int32 host arrays as one pinned blob and one host-to-device copy -> device views"""
    flat = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in arrays]
    blob = torch.from_numpy(np.concatenate(flat)).pin_memory().to(device, non_blocking=True)
    out, off = [], 0
    for a, f in zip(arrays, flat):
        out.append(blob[off:off + f.size].view(np.asarray(a).shape))
        off += f.size
    return out


class UnmoldPlan:
    """The surviving detections of one frame with their uploaded tables.  `areas()` and `masks(sel)` are one launch each."""

    def __init__(self, mrcnn_mask, boxes, class_ids, keep, height, width):
        if not isinstance(mrcnn_mask, torch.Tensor):
            raise TypeError('mrcnn_mask must be a torch.Tensor')
        if not mrcnn_mask.is_cuda:
            raise NotImplementedError('mrcnn_mask is on %s; the masks are unmolded on the GPU only (no CPU fallback)'
                                      % (mrcnn_mask.device,))
        if mrcnn_mask.dim() != 4 or mrcnn_mask.dtype != torch.float32:
            raise ValueError('mrcnn_mask must be float32 [D, C, Mh, Mw], got %s %s' % (mrcnn_mask.dtype, tuple(mrcnn_mask.shape)))
        self.boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        self.n = self.boxes.shape[0]
        if self.n < 1:
            raise ValueError('no detections')
        if int(np.max(keep)) >= mrcnn_mask.shape[0]:
            raise ValueError('detection row %d outside the %d rows of mrcnn_mask' % (int(np.max(keep)), mrcnn_mask.shape[0]))
        check_boxes(self.boxes, class_ids, height, width, mrcnn_mask.shape[1])
        self.mrcnn_mask, self.height, self.width = mrcnn_mask.contiguous(), height, width
        self.objs_host, bounds, kk8 = unmold_tables(self.boxes, class_ids, keep, mrcnn_mask.shape[2], mrcnn_mask.shape[3])
        self.tables = _upload_int32((self.objs_host, bounds, kk8), mrcnn_mask.device)

    def areas(self):
        """int32 [n] CUDA: the pixel count of every detection's mask; no plane is written"""
        from sdn_hip import ops
        return ops.unmold_masks(self.mrcnn_mask, self.objs_host, self.tables, self.height, self.width, planes=False)[1]

    def masks(self, sel=None):
        """(masks [len(sel), 1, H, W] float32 CUDA holding 0.0 / 1.0, areas int32 CUDA) of the detections `sel` (host indices,
        in that order; None: all)"""
        from sdn_hip import ops
        if sel is None:
            return ops.unmold_masks(self.mrcnn_mask, self.objs_host, self.tables, self.height, self.width)
        rows = np.ascontiguousarray(self.objs_host[np.asarray(sel, dtype=np.int64)])
        (objs,) = _upload_int32((rows,), self.mrcnn_mask.device)
        return ops.unmold_masks(self.mrcnn_mask, rows, (objs, self.tables[1], self.tables[2]), self.height, self.width)


def unmold_detections(detections, mrcnn_mask, image_shape, window):
    """MaskRCNN.unmold_detections (model.py:2084-2143) with the masks made on the device.  detections [D, 6] (CUDA tensor,
    copied to the host once; or a host array), mrcnn_mask float32 [D, C, Mh, Mw] CUDA in the network's own layout (the
    reference's permute to [D, Mh, Mw, C] serves its numpy indexing only).  Returns (boxes int32 [N, 4], class_ids int32 [N],
    scores [N]: numpy; masks float32 [N, 1, H, W] CUDA, binary -- the layout main.py:805-806 converts to).  N = 0 gives
    empty arrays and a [0, 1, H, W] tensor.  ValueError for a box that leaves the frame, where the reference's slice
    assignment raises."""
    if isinstance(detections, torch.Tensor):
        detections = detections.detach().cpu().numpy()
    boxes, class_ids, scores, keep = unmold_boxes(detections, image_shape, window)
    H, W = int(image_shape[0]), int(image_shape[1])
    if boxes.shape[0] == 0:
        if not mrcnn_mask.is_cuda:
            raise NotImplementedError('mrcnn_mask is on %s; the masks are unmolded on the GPU only' % (mrcnn_mask.device,))
        return boxes, class_ids, scores, torch.empty(0, 1, H, W, device=mrcnn_mask.device)
    plan = UnmoldPlan(mrcnn_mask, boxes, class_ids, keep, H, W)
    return boxes, class_ids, scores, plan.masks()[0]
