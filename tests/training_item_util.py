"""What maskrcnn.training_item must give, restated without the reference: resize_image, resize_mask, extract_bboxes and minimize_mask
of geometric/maskrcnn/utils.py and load_image_gt / Dataset.__getitem__ of model.py in numpy, over the real Pillow and the real
scipy.ndimage.zoom, the colour jitter through geo_train_util.color_jitter.  scipy.misc.imresize is gone from scipy: `imresize` states
scipy 1.0.1's (misc/pilutil.py: toimage -> bytescale -> Image -> resize -> fromimage), as tests/golden/make_detections_golden.py
documents it.  tests/golden/make_training_item_golden.py asserts that this file and the reference's own functions agree bit for bit
on every case of the fixture; the tests use it where a fixture would be too large (the 375 x 1242 case, the jitter)."""
import os

import numpy as np
import PIL.Image
import scipy.ndimage

import geo_train_util

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'training_item_golden.npz')
MEAN_PIXEL = np.array([123.7, 116.8, 103.9])
CASES = ('down', 'up', 'same', 'exact', 'many')


class Config(object):
    """the stand-in for the reference's Config: what the training item reads"""
    IMAGE_PADDING = True
    MEAN_PIXEL = MEAN_PIXEL
    USE_MINI_MASK = True
    MAX_GT_INSTANCES = 128
    NUM_CLASSES = 4

    def __init__(self, min_dim, max_dim, mini):
        self.IMAGE_MIN_DIM, self.IMAGE_MAX_DIM, self.MINI_MASK_SHAPE = int(min_dim), int(max_dim), (int(mini), int(mini))


def case_config(g, name):
    return Config(*[int(v) for v in g[name + '_dims']])


_golden = None


def golden():
    """the fixture, loaded once and shared (read-only)"""
    global _golden
    if _golden is None:
        z = np.load(GOLD, allow_pickle=False)
        _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def unpack(g, key, shape):
    """a bool array stored through np.packbits"""
    n = int(np.prod(shape))
    return np.unpackbits(g[key])[:n].reshape(shape).astype(bool)


def bytescale(data):
    """pilutil.bytescale(data), cmin = cmax = None, low = 0, high = 255; the data here are 0 / 1 in float64, where every step is exact"""
    if data.dtype == np.uint8:
        return data
    cmin, cmax = data.min(), data.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    scale = 255.0 / cscale
    bytedata = (data - cmin) * scale + 0
    return (bytedata.clip(0, 255) + 0.5).astype(np.uint8)


def imresize(arr, size, interp='bilinear', mode=None):
    """scipy 1.0.1's imresize for a uint8 [H, W, 3] array (bytescale is the identity, mode RGB) and a 2-D float array (mode L)"""
    assert interp == 'bilinear' and mode is None
    arr = np.asarray(arr)
    if arr.ndim == 3:
        assert arr.dtype == np.uint8 and arr.shape[2] == 3
        im = PIL.Image.frombytes('RGB', (arr.shape[1], arr.shape[0]), np.ascontiguousarray(arr).tobytes())
    else:
        data = bytescale(arr)
        im = PIL.Image.frombytes('L', (data.shape[1], data.shape[0]), np.ascontiguousarray(data).tobytes())
    return np.array(im.resize((int(size[1]), int(size[0])), resample=PIL.Image.BILINEAR))


def resize_image(image, min_dim, max_dim, padding):
    h, w = image.shape[:2]
    window = (0, 0, h, w)
    scale = 1
    if min_dim:
        scale = max(1, min_dim / min(h, w))
    if max_dim:
        image_max = max(h, w)
        if round(image_max * scale) > max_dim:
            scale = max_dim / image_max
    if scale != 1:
        image = imresize(image, (round(h * scale), round(w * scale)))
    if padding:
        h, w = image.shape[:2]
        top_pad = (max_dim - h) // 2
        bottom_pad = max_dim - h - top_pad
        left_pad = (max_dim - w) // 2
        right_pad = max_dim - w - left_pad
        padding = [(top_pad, bottom_pad), (left_pad, right_pad), (0, 0)]
        image = np.pad(image, padding, mode='constant', constant_values=0)
        window = (top_pad, left_pad, h + top_pad, w + left_pad)
    return image, window, scale, padding


def resize_mask(mask, scale, padding):
    mask = scipy.ndimage.zoom(mask, zoom=[scale, scale, 1], order=0)
    return np.pad(mask, padding, mode='constant', constant_values=0)


def extract_bboxes(mask):
    boxes = np.zeros([mask.shape[-1], 4], dtype=np.int32)
    for i in range(mask.shape[-1]):
        m = mask[:, :, i]
        cols = np.where(np.any(m, axis=0))[0]
        rows = np.where(np.any(m, axis=1))[0]
        if cols.shape[0]:
            boxes[i] = [rows[0], cols[0], rows[-1] + 1, cols[-1] + 1]
    return boxes


def minimize_mask(bbox, mask, mini_shape):
    """minimize_mask, but where the reference raises (a box without area) the mini-mask stays zero and the instance is counted"""
    mini = np.zeros(tuple(mini_shape) + (mask.shape[-1],), dtype=bool)
    bad = 0
    for i in range(mask.shape[-1]):
        y1, x1, y2, x2 = bbox[i][:4]
        m = mask[:, :, i][y1:y2, x1:x2]
        if m.size == 0:
            bad += 1
            continue
        m = imresize(m.astype(float), mini_shape, interp='bilinear')
        mini[:, :, i] = np.where(m >= 128, 1, 0)
    return mini, bad


def instance_stack(inst_map, ids):
    """bool [H, W, G]: what load_mask hands on for the kept ids (int32 [H, W]) or colour keys (uint8 [H, W, 3])"""
    inst_map = np.asarray(inst_map)
    if inst_map.ndim == 3:
        inst_map = (inst_map[..., 0].astype(np.int32) << 16) | (inst_map[..., 1].astype(np.int32) << 8) | inst_map[..., 2].astype(np.int32)
    return np.stack([inst_map == int(i) for i in ids], axis=-1)


def mold(image_u8, config):
    """mold_image on image.astype(np.float32), the transpose and .float() of Dataset.__getitem__: float32 [3, M, M]"""
    molded = image_u8.astype(np.float32) - config.MEAN_PIXEL
    assert molded.dtype == np.float64
    return np.ascontiguousarray(molded.transpose(2, 0, 1)).astype(np.float32)


def training_item(frame, inst_map, ids, config, flip=False, jitter=None, use_mini_mask=True):
    """dict of what the item must hold, as numpy"""
    if jitter is not None:
        order, factors, hue = jitter
        frame = geo_train_util.color_jitter(frame, list(order), factors, hue)
    image, window, scale, padding = resize_image(frame, config.IMAGE_MIN_DIM, config.IMAGE_MAX_DIM, config.IMAGE_PADDING)
    mask = resize_mask(instance_stack(inst_map, ids), scale, padding)
    if flip:
        image, mask = np.fliplr(image), np.fliplr(mask)
    bbox = extract_bboxes(mask)
    areas = mask.reshape(-1, mask.shape[-1]).sum(axis=0).astype(np.int32)
    bad = int((areas == 0).sum())
    if use_mini_mask:
        mask, raised = minimize_mask(bbox, mask, config.MINI_MASK_SHAPE)
        assert raised == bad
    M = float(config.IMAGE_MAX_DIM)
    return {'image_u8': np.ascontiguousarray(image), 'image': mold(image, config), 'window': window,
            'gt_boxes_int': bbox, 'gt_boxes': bbox.astype(np.float32),
            'gt_boxes_norm': (bbox.astype(np.float32) / np.array([M, M, M, M], np.float32))[None],
            'gt_masks': np.ascontiguousarray(mask.astype(int).transpose(2, 0, 1)).astype(np.float32),
            'areas': areas, 'bad': np.array([bad], np.int32)}


def zoom_by_gather(mask, scale):
    """ndimage.zoom(mask, [scale, scale, 1], order=0) through maskrcnn.training_item.zoom_table: a gather, 0 where a table holds -1"""
    from maskrcnn.training_item import zoom_table
    h, w = mask.shape[:2]
    yt, xt = zoom_table(h, int(round(h * scale))), zoom_table(w, int(round(w * scale)))
    out = mask[np.maximum(yt, 0)][:, np.maximum(xt, 0)].copy()
    out[yt < 0] = 0
    out[:, xt < 0] = 0
    return out


def coefficient_walk(n_in, n_out):
    """Pillow's precompute_coeffs and normalize_coeffs_8bpc for the bilinear filter as csrc/training_item_check.h's tri_ksize and
    tri_coeffs do them on the device: one output at a time, plain float64 operations in the C loop's order.
    Returns (ksize, bounds [n_out][2], coefficients [n_out][ksize]) as lists of ints."""
    scale = float(np.float32(n_in) - np.float32(0.0)) / float(n_out)
    filterscale = 1.0 if scale < 1.0 else scale
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, coeffs = [], []
    for xx in range(n_out):
        center = 0.0 + (float(xx) + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n_in:
            xmax = n_in
        xmax -= xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            arg = (float(x + xmin) - center + 0.5) * ss
            if arg < 0.0:
                arg = -arg
            w = 1.0 - arg if arg < 1.0 else 0.0
            ws.append(w)
            ww += w
        k = [int(0.5 + (w / ww if ww != 0.0 else w) * float(1 << 22)) for w in ws]
        bounds.append([xmin, xmax])
        coeffs.append(k + [0] * (ksize - xmax))
    return ksize, bounds, coeffs
