"""The training item of Mask R-CNN on the device: what Dataset.__getitem__ (reference: geometric/maskrcnn/model.py:1371-1409) makes per
item on the host through load_image_gt (:1154-1211) -- the colour jitter of load_image (datasets/vkitti.py:104-111),
utils.resize_image (utils.py:272-320), resize_mask (:323-335), np.fliplr, extract_bboxes (:26-49), minimize_mask (:338-353) and
mold_image (model.py:2196-2201) -- and the inference entry mold_inputs (:2046-2082).

    from maskrcnn.training_item import training_item
    item = training_item(frame_u8, inst_map, ids, class_ids, config, flip=random.randint(0, 1), jitter=pillow.jitter_params(...))
    rpn_match, rpn_bbox, _, _ = rpn_targets_padded(anchors, item.gt_class_ids, item.gt_boxes, config)
    ... detection_targets_padded(rois, item.gt_class_ids, item.gt_boxes_norm[0], item.gt_masks, config)

One image per call, as the reference's DataLoader(batch_size=1) (:1864).  The frame and the instance map are CUDA tensors; a CPU
tensor raises NotImplementedError and there is no torch form.  The host builds one parameter block from the frame's SIZE (the plan of
resize_image, Pillow's coefficient tables of the frame's resize, the index tables of ndimage.zoom, the mean table, the jitter's
draws) and uploads it in one copy; csrc/training_item.hip behind sdn_hip.ops.training_item does the rest in three launches, four with
a contrast op, and nothing crosses back to the host: all shapes follow from G and the config.

What is reproduced, bit for bit:
  * the image: scipy.misc.imresize of a uint8 RGB array is Pillow's resize((out_w, out_h), BILINEAR) -- the horizontal pass into
    bytes, then the vertical one, a pass of equal sizes skipped, no resize at scale == 1; the jitter on the source pixels before it;
    zero padding, THEN the mirror of the padded image (with an odd pad the two sides differ); fp32(fp64(byte) - MEAN_PIXEL[c]), so a
    padding pixel is fp32(0 - MEAN_PIXEL[c]).  The window in image_meta is not mirrored, as in the reference.
  * the masks: ndimage.zoom(order=0) is a gather, so zoom(inst_map == id) == (zoom(inst_map) == id); the index tables are built here
    in float64 (zoom_table), -1 where zoom yields the constant 0 (the last index of some size pairs, by one ulp).
  * the boxes: first and last + 1 row and column of every instance in the padded, mirrored frame; zeros for one without a pixel.
  * the mini-masks: bytescale of the crop (0 / 255, but all 0 for a crop whose every pixel is set: cmax == cmin, so a solid rectangle
    gets an all-zero mini-mask), Pillow's resize of an 'L' image of the crop's size, whose coefficients only the device can know:
    they are computed there in fp64, operation for operation sdn_hip.pillow.resample_tables / fixed_point; then >= 128.
One deviation, where the reference raises: an instance that vanished in the zoom gets an all-zero mask and counts in `bad`.

Out of scope:
  * the id selection of load_mask (np.unique, counts > 50, the category filters): a property of the stored frame, not of the draw;
    the caller computes `ids` and `class_ids` once per frame and caches them;
  * the float image of the Cityscapes train subset (datasets/cityscapes.py:119-127: image + noise, min-max rescaled by imresize);
  * G > MAX_GT_INSTANCES (model.py:1389-1394: a random subset) and G outside [1, 128]: both raise ValueError.
"""
import collections
import functools
import types

import numpy as np
import torch

from sdn_hip import ops, pillow

TrainingItem = collections.namedtuple('TrainingItem', ['image', 'image_meta', 'window', 'gt_class_ids', 'gt_boxes', 'gt_boxes_int',
                                                       'gt_boxes_norm', 'gt_masks', 'areas', 'bad'])

PLAN_INTS = ops.TRAINING_ITEM_PLAN_INTS


def resize_plan(shape, config):
    """The arithmetic of utils.resize_image (utils.py:292-319) on a shape, statement for statement, plain Python numbers:
    (out_h, out_w, window, scale, padding)."""
    h, w = int(shape[0]), int(shape[1])
    min_dim, max_dim, padding = config.IMAGE_MIN_DIM, config.IMAGE_MAX_DIM, config.IMAGE_PADDING
    window = (0, 0, h, w)
    scale = 1
    if min_dim:
        scale = max(1, min_dim / min(h, w))
    if max_dim:
        image_max = max(h, w)
        if round(image_max * scale) > max_dim:
            scale = max_dim / image_max
    if scale != 1:
        h, w = round(h * scale), round(w * scale)
    if not padding:
        raise ValueError('IMAGE_PADDING is false: not supported (every consumer takes IMAGE_MAX_DIM x IMAGE_MAX_DIM images)')
    if h > max_dim or w > max_dim:
        raise ValueError('the frame resized to %d x %d exceeds IMAGE_MAX_DIM %d' % (h, w, max_dim))
    top_pad = (max_dim - h) // 2
    bottom_pad = max_dim - h - top_pad
    left_pad = (max_dim - w) // 2
    right_pad = max_dim - w - left_pad
    padding = [(top_pad, bottom_pad), (left_pad, right_pad), (0, 0)]
    window = (top_pad, left_pad, h + top_pad, w + left_pad)
    return h, w, window, scale, padding


def zoom_table(n_in, n_out):
    """The source index of every output index of scipy.ndimage.zoom(order=0, mode='constant') along an axis of n_in made n_out long:
    floor(c + 0.5) with c = i * ((n_in - 1) / (n_out - 1)) in float64, -1 where c > n_in - 1 (the constant 0).  numpy int32 [n_out]."""
    table = np.zeros(n_out, np.int32)
    if n_out > 1:
        step = float(n_in - 1) / float(n_out - 1)
        for i in range(n_out):
            c = i * step
            table[i] = -1 if c > n_in - 1 else int(np.floor(c + 0.5))
    return table


def compose_image_meta(image_id, image_shape, window, active_class_ids):
    """compose_image_meta (model.py:2150-2169): one numpy row (image_id, shape, window, active_class_ids)"""
    return np.array([image_id] + list(image_shape) + list(window) + list(active_class_ids))


def color_keys(codes_u8):
    """the int32 keys r << 16 | g << 8 | b of uint8 [G, 3] instance colours (datasets/vkitti_utils.py:11-42 gives every instance its
    own): the `ids` of a uint8 [H, W, 3] inst_map.  A tensor gives a tensor on its device, anything else numpy."""
    if isinstance(codes_u8, torch.Tensor):
        c = codes_u8.to(torch.int32)
        return ((c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]).contiguous()
    c = np.asarray(codes_u8).astype(np.int32)
    return (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]


def mean_table(config):
    """fp32(fp64(byte) - MEAN_PIXEL[c]) for every byte: float32 [3, 256] (mold_image on image.astype(np.float32), then .float())"""
    mean = np.asarray(config.MEAN_PIXEL, np.float64).reshape(3)
    return (np.arange(256, dtype=np.float64)[None, :] - mean[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=32)
def _size_block(H, W, min_dim, max_dim, padding, mean_pixel):
    """what of the parameter block follows from the frame's size and the config alone: (block with flip and jitter left open,
    window); cached, treat the array as read-only"""
    config = types.SimpleNamespace(IMAGE_MIN_DIM=min_dim, IMAGE_MAX_DIM=max_dim, IMAGE_PADDING=padding, MEAN_PIXEL=mean_pixel)
    oh, ow, window, _scale, pads = resize_plan((H, W), config)
    parts, at = [], PLAN_INTS

    def put(a):
        nonlocal at
        a = np.ascontiguousarray(a).reshape(-1).view(np.int32)
        parts.append(a)
        at += a.size
        return at - a.size

    def axis(n_in, n_out):
        if n_in == n_out:   # Pillow skips the pass
            return 0, 0, 0
        ksize, bounds, kk = pillow.resample_tables(n_in, n_out)
        return put(bounds.astype(np.int32)), put(pillow.fixed_point(kk)), ksize

    xb, xk, xksize = axis(W, ow)
    yb, yk, yksize = axis(H, oh)
    ytab, xtab = put(zoom_table(H, oh)), put(zoom_table(W, ow))
    mean = put(mean_table(config))
    head = np.zeros(PLAN_INTS, np.int32)
    head[:7] = [H, W, oh, ow, int(max_dim), pads[0][0], pads[1][0]]
    head[10:13] = np.ones(3, np.float32).view(np.int32)
    head[14:23] = [xb, xk, xksize, yb, yk, yksize, ytab, xtab, mean]
    block = np.concatenate([head] + parts)
    block.setflags(write=False)
    return block, window


def plan_block(shape, config, flip=False, jitter=None):
    """The parameter block of sdn_training_item for frames of this shape (csrc/training_item_check.h: TriPlan): numpy int32 [n].
    The tables depend on the frame's size and the config alone and are kept per size; flip and jitter fill four fields of the head.
    Returns (block, window)."""
    order, factors, hue = jitter if jitter is not None else ((), (1.0, 1.0, 1.0), 0)
    order = [int(op) for op in order]
    if len(order) > 4 or len(set(order)) != len(order) or any(op < 0 or op > 3 for op in order):
        raise ValueError('jitter order %s is not a list of distinct ops 0 .. 3' % (order,))
    if not 0 <= int(hue) <= 255:
        raise ValueError('hue shift %s; 0 to 255 (pillow.jitter_params)' % (hue,))
    sized, window = _size_block(int(shape[0]), int(shape[1]), config.IMAGE_MIN_DIM, config.IMAGE_MAX_DIM, bool(config.IMAGE_PADDING),
                                tuple(float(v) for v in np.asarray(config.MEAN_PIXEL).reshape(-1)))
    block = sized.copy()
    block[7:10] = [int(bool(flip)), len(order), sum(op << (4 * k) for k, op in enumerate(order))]
    block[10:13] = np.asarray(factors, np.float32).view(np.int32)
    block[13] = int(hue)
    return block, window


def _active(config, active_class_ids):
    if active_class_ids is None:   # one source: every class of the dataset is active (utils.Dataset.prepare)
        return np.ones([config.NUM_CLASSES], dtype=np.int32)
    return np.asarray(active_class_ids, np.int32)


def training_item(frame_u8, inst_map, ids, class_ids, config, flip=False, jitter=None, use_mini_mask=None, image_id=0,
                  active_class_ids=None):
    """One training item, see the module's docstring.  frame_u8 uint8 [H, W, 3]; inst_map int32 [H, W] (the Cityscapes id map widened,
    datasets/cityscapes.py:100) or uint8 [H, W, 3] (a VKITTI scene map: the key of a pixel is r << 16 | g << 8 | b, color_keys); ids
    int32 [G], the kept ids or keys; class_ids [G]; all on the device.  flip: the outcome of random.randint(0, 1), drawn by the caller;
    jitter: what pillow.jitter_params returns, or None; use_mini_mask None reads config.USE_MINI_MASK.  Returns a TrainingItem:

        image         fp32  [3, M, M]                     M = config.IMAGE_MAX_DIM
        image_meta    numpy, host                          compose_image_meta(image_id, frame shape, window, active_class_ids)
        window        (y1, x1, y2, x2), host
        gt_class_ids  int32 [G]
        gt_boxes      fp32  [G, 4]                         pixels (model.py:1406)
        gt_boxes_int  int32 [G, 4]
        gt_boxes_norm fp32  [1, G, 4]                      gt_boxes / (M, M, M, M) in fp32 (:1790-1794)
        gt_masks      fp32  [G, mh, mw] or [G, M, M]       0 / 1 (:1407)
        areas         int32 [G]                            pixels of every instance after resize, padding and mirror
        bad           int32 [1]                            instances without a pixel: zero box, zero mask

    Raises ValueError for G outside [1, 128] or above config.MAX_GT_INSTANCES and for a plan resize_plan refuses."""
    if not isinstance(ids, torch.Tensor):
        raise TypeError('ids must be a torch.Tensor, got %r' % (type(ids),))
    if ids.dim() != 1:
        raise ValueError('ids must be [G], got %s' % (tuple(ids.shape),))
    G = ids.shape[0]
    if G < 1 or G > ops.TRAINING_ITEM_MAX_BOXES:
        raise ValueError('G = %d; 1 to %d instances are supported' % (G, ops.TRAINING_ITEM_MAX_BOXES))
    if G > config.MAX_GT_INSTANCES:
        raise ValueError('G = %d exceeds MAX_GT_INSTANCES %d: the random subset of model.py:1389-1394 is the caller\'s' % (G, config.MAX_GT_INSTANCES))
    if not isinstance(frame_u8, torch.Tensor):
        raise TypeError('frame_u8 must be a torch.Tensor, got %r' % (type(frame_u8),))
    if frame_u8.dim() != 3 or frame_u8.shape[2] != 3:
        raise ValueError('frame_u8 must be uint8 [H, W, 3], got %s' % (tuple(frame_u8.shape),))
    if not isinstance(class_ids, torch.Tensor):
        class_ids = torch.as_tensor(np.asarray(class_ids))
    if tuple(class_ids.shape) != (G,):
        raise ValueError('class_ids must be [G] = %s, got %s' % ((G,), tuple(class_ids.shape)))
    if use_mini_mask is None:
        use_mini_mask = config.USE_MINI_MASK
    block, window = plan_block(frame_u8.shape, config, flip=flip, jitter=jitter)
    image, boxes_int, boxes, boxes_norm, masks, areas, bad = ops.training_item(frame_u8, inst_map, ids, block, use_mini_mask,
                                                                                tuple(config.MINI_MASK_SHAPE))
    meta = compose_image_meta(image_id, tuple(frame_u8.shape), window, _active(config, active_class_ids))
    gt_class_ids = class_ids.to(device=frame_u8.device, dtype=torch.int32)
    return TrainingItem(image, meta, window, gt_class_ids, boxes, boxes_int, boxes_norm.unsqueeze(0), masks, areas, bad)


def load_image_gt(frame_u8, inst_map, ids, class_ids, config, image_id=0, active_class_ids=None, flip=False, jitter=None,
                  use_mini_mask=False):
    """The reference's load_image_gt (model.py:1154-1211) with the dataset object replaced by what it would have loaded: (image,
    image_meta, class_ids, bbox, mask) in its order.  bbox is int32 [G, 4] and mask [h, w, G] (a view of [G, h, w], fp32 0 / 1) as
    there; image is already molded, fp32 [3, M, M] (every consumer molds it first); all but image_meta stay on the device."""
    item = training_item(frame_u8, inst_map, ids, class_ids, config, flip=flip, jitter=jitter, use_mini_mask=use_mini_mask,
                         image_id=image_id, active_class_ids=active_class_ids)
    return item.image, item.image_meta, item.gt_class_ids, item.gt_boxes_int, item.gt_masks.permute(1, 2, 0)


def mold_inputs(frames_u8, config):
    """MaskRCNN.mold_inputs (model.py:2046-2082) for a list of uint8 [H, W, 3] frames on the device: (molded_images fp32 [N, 3, M, M] on
    the device, image_metas numpy [N, 8 + NUM_CLASSES], windows numpy [N, 4]).  The image kernel alone, one launch per distinct frame
    size.  A CPU tensor raises NotImplementedError."""
    frames = list(frames_u8)
    if not frames:
        raise ValueError('mold_inputs needs at least one frame')
    groups = collections.OrderedDict()
    for n, f in enumerate(frames):
        if not isinstance(f, torch.Tensor):
            raise TypeError('frame %d must be a torch.Tensor, got %r' % (n, type(f)))
        if f.dim() != 3 or f.shape[2] != 3:
            raise ValueError('frame %d must be uint8 [H, W, 3], got %s' % (n, tuple(f.shape)))
        if not f.is_cuda:
            raise NotImplementedError('frame %d is on %s; the training item only runs on the GPU' % (n, f.device))
        groups.setdefault(tuple(f.shape), []).append(n)
    M = int(config.IMAGE_MAX_DIM)
    metas, windows = [None] * len(frames), [None] * len(frames)
    molded = None
    for shape, members in groups.items():
        block, window = plan_block(shape, config)
        batch = frames[members[0]].unsqueeze(0) if len(members) == 1 else torch.stack([frames[n] for n in members])
        image = ops.training_item_image(batch.contiguous(), block)
        if len(groups) == 1:
            molded = image
        else:
            if molded is None:
                molded = torch.empty(len(frames), 3, M, M, dtype=torch.float32, device=image.device)
            molded[torch.as_tensor(members, device=image.device)] = image
        for n in members:
            metas[n] = compose_image_meta(0, shape, window, np.zeros([config.NUM_CLASSES], dtype=np.int32))
            windows[n] = window
    return molded, np.stack(metas), np.stack(windows)
