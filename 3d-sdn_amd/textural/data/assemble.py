"""Textural input assembly on the device: what the reference's VKITTI loader does per item with PIL
and numpy on the host -- textural/data/vkitti_dataset.py:44-142 on top of base_dataset.py:21-110 -- as tensor
operations that run wherever the input tensors live, so that the geometric branch's maps (or the decoded PNGs of its
wire format) become the generator's inputs without a host round trip.

The one non-trivial piece is PIL's resizing.  `resize_u8` reproduces it bit for bit:
  * BICUBIC / BILINEAR (images, normal maps): Pillow's ImagingResample -- per output pixel a source window and weights
    (precompute_coeffs), 22-bit fixed point, horizontal pass rounded to uint8, then vertical;
  * NEAREST (label / instance / pose maps): Pillow's ImagingScaleAffine -- source index = (int) of a running double sum.
The tables are prepared on the host (numpy, cached per size) and the passes are integer gathers and sums on the tensor's
device.  tests/test_assemble.py pins every step against the real PIL of this image; tests/test_gpu_assemble.py runs
the same comparison with CUDA tensors.

`--feat_depth` (the 16-bit PNG branch, vkitti_dataset.py:131-137) is `depth_feature`.  Every division the loader performs
(ToTensor's / 255, the depth branch's / 65535) is a look-up in a table computed on the HOST: torch's device kernels turn
a division by a scalar into a multiplication by its reciprocal, which is not the same rounding.
Not covered: colour jitter, file discovery -- host-side data loading proper stays the caller's business.
"""
import functools
import os
from math import cos, pi, sin

import numpy as np
import torch

from sdn_hip import pillow as _pillow

PRECISION_BITS = 32 - 8 - 2  # Pillow, Resample.c


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


_FILTERS = {'bicubic': (_bicubic, 2.0), 'bilinear': (_bilinear, 1.0)}


@functools.lru_cache(maxsize=64)
def _resample_table(in_size, out_size, method):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc.  Returns (idx int64 [out, ksize] clamped source indices,
    k8 int64 [out, ksize] fixed-point weights, zero beyond each window)."""
    filt, support0 = _FILTERS[method]
    scale = np.float64(np.float32(in_size) - np.float32(0.0)) / out_size
    filterscale = max(scale, 1.0)
    support = support0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    cnt = xmax - xmin
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        w = np.where(x < cnt, filt((x + xmin - center + 0.5) * ss), 0.0)
        kk[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    kk[nz] = kk[nz] / ww[nz, None]
    v = kk * float(1 << PRECISION_BITS)
    k8 = np.where(kk < 0, np.trunc(-0.5 + v), np.trunc(0.5 + v)).astype(np.int64)
    idx = np.minimum(xmin[:, None] + np.arange(ksize)[None, :], in_size - 1)
    return torch.from_numpy(idx), torch.from_numpy(k8)


@functools.lru_cache(maxsize=64)
def _nearest_table(in_size, out_size):
    """Pillow's NEAREST source indices (sdn_hip.pillow.nearest_table) as a tensor."""
    return torch.from_numpy(_pillow.nearest_table(in_size, out_size))


_TABLES_ON = {}


def _on(dev, fn, *key):
    """the (host-built, lru-cached) index / weight table fn(*key) as tensors on `dev`, uploaded ONCE per device: `.to(dev)` of a
    pageable host tensor is a synchronous copy queued behind the stream's kernels, i.e. one device synchronisation per resize
    axis -- 14 of them per frame made configs[4] host-paced (208 ms of a 64-frame pass, profiles/r05zb_host_profile_pipe.txt)"""
    if os.environ.get('SDN_ASSEMBLE_UPLOAD_TABLES') == '1':   # A/B switch: the upload per call of r01-r04
        r = fn(*key)
        return tuple(x.to(dev) for x in r) if isinstance(r, tuple) else r.to(dev)
    k = (fn.__name__, str(dev)) + key
    t = _TABLES_ON.get(k)
    if t is None:
        if len(_TABLES_ON) > 256:
            _TABLES_ON.clear()
        r = fn(*key)
        t = _TABLES_ON[k] = tuple(x.to(dev) for x in r) if isinstance(r, tuple) else r.to(dev)
    return t


def resize_nearest(img, oh, ow):
    """PIL NEAREST for any pixel type ([C, H, W]): pure index selection."""
    C, H, W = img.shape
    if (oh, ow) == (H, W):
        return img.clone()
    dev = img.device
    return img[:, _on(dev, _nearest_table, H, oh)][:, :, _on(dev, _nearest_table, W, ow)]


def _resize(img, oh, ow, method):
    return resize_nearest(img, oh, ow) if method == 'nearest' else resize_u8(img, oh, ow, method)


def resize_u8(img, oh, ow, method):
    """img uint8 [C, H, W] on any device -> uint8 [C, oh, ow], bit-identical to PIL.Image.resize((ow, oh), method)."""
    if img.dtype != torch.uint8 or img.dim() != 3:
        raise TypeError('resize_u8 expects a uint8 [C, H, W] tensor')
    C, H, W = img.shape
    if (oh, ow) == (H, W):
        return img.clone()
    dev = img.device
    if method == 'nearest':
        return resize_nearest(img, oh, ow)
    half = 1 << (PRECISION_BITS - 1)
    cur = img.to(torch.int64)
    if ow != W:  # horizontal pass, rounded and clipped to the pixel type
        idx, k8 = _on(dev, _resample_table, W, ow, method)
        acc = (cur[:, :, idx] * k8).sum(dim=3) + half
        cur = (acc >> PRECISION_BITS).clamp_(0, 255)
    if oh != H:
        idx, k8 = _on(dev, _resample_table, H, oh, method)
        acc = (cur[:, idx] * k8[None, :, :, None]).sum(dim=2) + half
        cur = (acc >> PRECISION_BITS).clamp_(0, 255)
    return cur.to(torch.uint8)


@functools.lru_cache(maxsize=1)
def _to_tensor_lut():
    """float32(k) / float32(255), correctly rounded, for k = 0..255 -- computed on the HOST.  torch's device kernels
    evaluate `x.div(255)` as `x * (1 / 255)`, which differs from the division ToTensor performs on the CPU for many k
    (and then k / 255 * 255 != k: a label of 6.9999995 truncates to class 6 in Pix2PixHDModel's one-hot encoding)."""
    return torch.from_numpy((np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32))


@functools.lru_cache(maxsize=2)
def _depth_lut(wrap_int16):
    """1.0 - float32(d) / 65535.0 for the 65536 values of a 16-bit depth PNG (vkitti_dataset.py:131-137), computed on
    the host with the CPU loader's own operations.  wrap_int16: torchvision 0.2.x's ToTensor reads a mode-'I;16' image
    through np.int16 (values >= 32768 come out negative); PIL versions that open 16-bit PNGs as mode 'I' do not."""
    d = np.arange(65536, dtype=np.int64)
    if wrap_int16:
        d = d.astype(np.uint16).view(np.int16).astype(np.int64)
    t = torch.from_numpy(d).float() / 65535.0
    return 1.0 - t


_LUT_ON = {}


def to_tensor_u8(img):
    """torchvision's ToTensor arithmetic (uint8 -> float32, / 255) for a uint8 tensor on any device, bit-identical to the
    CPU result: a 256-entry table look-up instead of a device-side division."""
    if img.dtype != torch.uint8:
        raise TypeError('to_tensor_u8 expects uint8')
    lut = _LUT_ON.get(img.device)
    if lut is None:
        lut = _LUT_ON[img.device] = _to_tensor_lut().to(img.device)
    return lut[img.long()]


# ---------------------------------------------------------------------------------------------------------------------
# base_dataset.py: get_transform as a function of (options, params) on a uint8 [C, H, W] tensor
def load_size_after_scaling(opt, h, w):
    """(h, w) after the resize step of get_transform (base_dataset.py:45-49, 82-91)."""
    roc = opt.resize_or_crop
    if 'resize' in roc:
        return opt.loadSize, opt.loadSize
    if 'scale_width' in roc:
        if w == opt.loadSize:
            return h, w
        nh = int(opt.loadSize * h / w)
        return (192 if nh == 188 else nh), opt.loadSize   # the reference's hack for 375 x 1242 -> 192 x 624
    return h, w


def _geometry(img, opt, params, method):
    """The PIL-image part of get_transform (base_dataset.py:41-61): resize / scale width, crop, make_power_2, flip, on an
    integer [C, H, W] tensor (uint8 for every method; any integer type for 'nearest', which only moves pixels)."""
    C, H, W = img.shape
    roc = opt.resize_or_crop
    oh, ow = load_size_after_scaling(opt, H, W)
    img = _resize(img, oh, ow, method)
    if 'crop' in roc:
        x1, y1 = params['crop_pos']
        tw, th = opt.fineWidth, opt.fineHeight
        if ow > tw or oh > th:
            out = torch.zeros(C, th, tw, dtype=img.dtype, device=img.device)   # PIL pads a crop box beyond the image
            ys, xs = max(0, min(th, oh - y1)), max(0, min(tw, ow - x1))
            out[:, :ys, :xs] = img[:, y1:y1 + ys, x1:x1 + xs]
            img = out
    if roc == 'none':
        base = float(2 ** opt.n_downsample_global)
        if opt.netG == 'local':
            base *= (2 ** opt.n_local_enhancers)
        h2, w2 = int(round(img.shape[1] / base) * base), int(round(img.shape[2] / base) * base)
        img = _resize(img, h2, w2, method)
    if opt.isTrain and not opt.no_flip and params['flip']:
        img = torch.flip(img, dims=(2,))
    return img


def transform(img, opt, params, method='bicubic', normalize=True):
    """get_transform(opt, params, method, normalize)(PIL image) for a uint8 [C, H, W] tensor (base_dataset.py:41-66):
    the image geometry above, then ToTensor (/ 255) and Normalize((x - 0.5) / 0.5)."""
    t = to_tensor_u8(_geometry(img, opt, params, method))
    if normalize:
        t = (t - 0.5) / 0.5   # exact on every device: x - 0.5 is one IEEE subtraction, / 0.5 is a multiplication by 2
    return t


def pose_bins(num_bins):
    return np.array(list(range(-180, 181, 360 // num_bins))) / 180


def depth_feature(depth, opt, params, wrap_int16=False):
    """The `--feat_depth` branch (vkitti_dataset.py:131-137): the geometric branch's NNNNN-depth.png (16-bit, values
    0..65535, integer [1, H, W] tensor of any integer type wide enough) through transform_A's geometry (NEAREST), then
    1.0 - float(d) / 65535.0.  The division is a host-built table look-up, for the reason given at to_tensor_u8."""
    if depth.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16):
        raise TypeError('depth_feature expects the integer pixel values of the 16-bit PNG')
    g = _geometry(depth, opt, params, 'nearest').long()
    if int(g.min()) < 0 or int(g.max()) > 65535:
        raise ValueError('depth values outside 0..65535')
    key = ('depth', bool(wrap_int16), g.device)
    lut = _LUT_ON.get(key)
    if lut is None:
        lut = _LUT_ON[key] = _depth_lut(bool(wrap_int16)).to(g.device)
    return lut[g]


def assemble_item(opt, params, segm, image, inst=None, pose_inst=None, pose_json=None, normal=None, depth=None,
                  depth_wrap_int16=False):
    """vkitti_dataset.__getitem__ (:44-142) from already decoded maps, all uint8 [C, H, W] tensors on one device:
    segm [1,H,W] label ids, image [3,H,W] RGB, inst [1,H,W] instance ids, pose_inst [1,H,W] + pose_json (the geometric
    branch's NNNNN.png / NNNNN.json), normal [3,H,W] (NNNNN-normal.png).  Returns the loader's dict entries
    label / inst / image / pose / normal (0 where the loader leaves its default)."""
    out = {'label': 0, 'inst': 0, 'image': 0, 'pose': 0, 'normal': 0, 'feat': 0, 'depth': 0}
    if opt.label_nc == 0:
        A = transform(segm.expand(3, -1, -1) if segm.shape[0] == 1 else segm, opt, params)
    else:
        A = transform(segm, opt, params, method='nearest', normalize=False) * 255.0
    if opt.segm_precomputed_path:
        A = A + 1
    out['image'] = transform(image, opt, params)
    if not opt.no_instance:
        if inst is None:
            inst_t = A
        else:
            inst_t = transform(inst, opt, params, method='nearest', normalize=False)
            if opt.inst_precomputed_path:
                inst_t = inst_t * 255.0
                inst_t = inst_t * 1000
                if opt.segm_precomputed_path:   # car labels without an instance become "misc" (:75-78)
                    A = A.clone()
                    A[(inst_t == 0) & (A == 2)] = 5
                    A[(inst_t == 0) & (A == 12)] = 5
                inst_t = torch.where(inst_t == 0, A, inst_t)
        out['inst'] = inst_t
    out['label'] = A
    if opt.feat_pose:
        nb = opt.feat_pose_num_bins
        H, W = A.shape[1], A.shape[2]
        if nb > 0:
            pose = torch.zeros(1, H, W, dtype=torch.float64, device=A.device)
        else:
            pose = torch.zeros(2, H, W, dtype=torch.float64, device=A.device)
        if pose_inst is not None and pose_json is not None:
            inst_map = (transform(pose_inst, opt, params, method='nearest', normalize=False) * 255.0)[0]
            bins = pose_bins(nb) if nb else None
            for key, rec in pose_json.items():      # the loader walks np.unique(inst_map); ids absent from the map
                k = int(key)                        # give empty masks here
                if k == 0:
                    continue
                m = inst_map == float(k)
                alpha = rec['alpha']
                if nb > 0:
                    pose[0][m] = float(np.digitize(alpha / pi, bins))
                else:
                    pose[0][m] = cos(alpha)
                    pose[1][m] = sin(alpha)
        out['pose'] = pose.int() if nb else pose.float()
    if opt.feat_normal:
        if normal is not None:
            out['normal'] = transform(normal, opt, params) + 1 / 255   # "bias caused by 0..256 instead of 0..255" (:125)
        else:
            out['normal'] = torch.zeros_like(out['image'])
    if getattr(opt, 'feat_depth', None):
        out['depth'] = depth_feature(depth, opt, params, depth_wrap_int16) if depth is not None else torch.zeros_like(A)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the edit path: textural/edit_vkitti.py:62-103, edit_benchmark.py:87-126
EDIT_CLASS_LABEL = {1: 2, 2: 12}   # class_id of NNNNN.json -> label id (car, van), edit_vkitti.py:79


def edit_tables(opt, edit_json):
    """The two per-frame look-up tables of sdn_edit_assemble, built on the host from one NNNNN.json: (obj_label, obj_pose),
    int32 [256] indexed by raw object id.  obj_label[k] = {1: 2, 2: 12}[class_id] (0: k is not in the JSON),
    obj_pose[k] = np.digitize(alpha / pi, bins) (edit_vkitti.py:73-82; 0 without pose bins).  compositing.frame_json
    numbers objects from 1 and NNNNN.png holds uint8, so a key outside 1..255 is refused; an unknown class_id raises
    KeyError as the reference's dict look-up does."""
    nb = opt.feat_pose_num_bins
    bins = pose_bins(nb) if nb else None
    label = np.zeros(256, dtype=np.int32)
    pose = np.zeros(256, dtype=np.int32)
    for key, rec in edit_json.items():
        k = int(key)
        if not 1 <= k <= 255:
            raise ValueError('object id %d of the edit JSON is outside 1..255' % k)
        label[k] = EDIT_CLASS_LABEL[rec['class_id']]
        if nb:
            pose[k] = int(np.digitize(rec['alpha'] / pi, bins))
    return label, pose


def assemble_edit(opt, params, base_item, edit_inst_u8, edit_json, codes, normal_u8=None):
    """The generator inputs of EDITED frames (the `for` body of edit_vkitti.py:62-103 / edit_benchmark.py:87-126) in one
    kernel launch, with the source frame's appearance codes painted at each instance's new pixels on the device.
      base_item     assemble_item's dict of the SOURCE frame (both *_precomputed_path options set: label + 1, car pixels
                    without an instance already "misc"), or a list of F such dicts (one source per frame, edit_benchmark)
      edit_inst_u8  uint8 [1, H, W] raw object ids of NNNNN.png (compositing.wire_tensors), or a list of F of them
      edit_json     the frame's NNNNN.json dict {object id: {'class_id', 'alpha', ...}}, or a list of F
      codes         (ids, means [K, feat_num]) of Encoder.feat_table on the source frame
      normal_u8     uint8 [3, H, W] of NNNNN-normal.png, None ("no cars"), or a list of F of either
    Returns a dict of batched tensors: label / inst [F,1,h,w], pose [F,1|2,h,w], feat [F,feat_num,h,w] (fp32: what
    Pix2PixHDModel.fake_inference takes), normal [F,3,h,w] (transform(normal) + 1/255, zeros where absent or without
    --feat_normal), missing int32 [F] (pixels whose instance has no source code; they are painted 0) -- all on the device,
    nothing is read back -- and obj_label / obj_pose, the host-built int32 [F, 256] tables."""
    from sdn_hip import ops as _ops
    many = isinstance(edit_inst_u8, (list, tuple))
    insts = list(edit_inst_u8) if many else [edit_inst_u8]
    F = len(insts)
    jsons = list(edit_json) if many else [edit_json]
    normals = list(normal_u8) if isinstance(normal_u8, (list, tuple)) else [normal_u8] * F
    bases = list(base_item) if isinstance(base_item, (list, tuple)) else [base_item]
    if F < 1 or len(jsons) != F or len(normals) != F or len(bases) not in (1, F):
        raise ValueError('assemble_edit: %d instance maps, %d JSON records, %d normal maps, %d source items'
                         % (F, len(jsons), len(normals), len(bases)))
    tables = [edit_tables(opt, js) for js in jsons]
    obj_label = np.stack([t[0] for t in tables])
    obj_pose = np.stack([t[1] for t in tables])
    ids, means = codes
    for t in insts + [b['label'] for b in bases] + [ids, means]:
        if not isinstance(t, torch.Tensor):
            raise TypeError('assemble_edit expects torch tensors')
        if not t.is_cuda:   # as every op of this project: no host path
            raise NotImplementedError('assemble_edit: a tensor is on %s; the edit assembly only runs on the GPU' % t.device)
    dev = insts[0].device
    edit = torch.stack([_geometry(t, opt, params, 'nearest') for t in insts])
    base = torch.stack([b['label'] for b in bases]).float()
    label, inst, pose, feat, missing = _ops.edit_assemble(
        base, edit, torch.from_numpy(obj_label).to(dev), torch.from_numpy(obj_pose).to(dev), ids.to(torch.int32),
        means.t().contiguous(), pose_channels=1 if opt.feat_pose_num_bins else 2)
    zero = None
    nrm = []
    for n in normals:
        if n is not None and opt.feat_normal:
            nrm.append(transform(n, opt, params) + 1 / 255)   # "bias caused by 0..256 instead 0..255" (edit_vkitti.py:93)
        else:
            if zero is None:
                zero = torch.zeros(3, label.shape[2], label.shape[3], dtype=torch.float32, device=dev)
            nrm.append(zero)
    return {'label': label, 'inst': inst, 'pose': pose, 'feat': feat, 'missing': missing, 'normal': torch.stack(nrm),
            'obj_label': obj_label, 'obj_pose': obj_pose}


# ---------------------------------------------------------------------------------------------------------------------
# the loader's item as kernels, batched (csrc/assemble.hip): vkitti_dataset.py:44-129 and cityscapes_dataset.py:32-111
# data/cityscapes_labels.py restated as data: CITYSCAPES_LABEL_TABLE[id] = trainId + 1, 0 for the void classes (trainId 255),
# for the label ids 0..33 (cityscapes_dataset.py:102-105; the 'license plate' row has id -1 and matches no pixel)
CITYSCAPES_LABEL_TABLE = [0, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 3, 4, 5, 0, 0, 0, 6, 0, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0, 0, 17,
                          18, 19]
MIN_POSE_AREA = {'vkitti': 1, 'cityscapes': 256}   # cityscapes_dataset.py:82: smaller instances get no pose


@functools.lru_cache(maxsize=64)
def _nearest_table_generic(in_size, out_size):
    """Pillow's NEAREST for the image modes ImagingScaleAffine does not serve (mode 'I;16': ImagingGenericTransform with
    affine_transform): the source index of output x is (int)(a (x + 0.5)), evaluated per pixel -- not the running sum of
    _nearest_table, which lands one lower where a (x + 0.5) is an integer the sum falls short of (128 -> 96, x = 4).  Pillow
    takes that path whenever it resizes such an image at all; on an axis that keeps its size the index is x itself."""
    a = np.float64(in_size) / out_size
    idx = (a * (np.arange(out_size, dtype=np.float64) + 0.5) + 0.0).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, in_size - 1))


def batch_geometry(opt, H, W):
    """(sh, sw, h, w, crops) of get_transform for an [H, W] source: the size after the mode's one resize (Scale, __scale_width
    or __make_power_2), the output size, and whether __crop applies (base_dataset.py:41-98)."""
    roc = opt.resize_or_crop
    sh, sw = load_size_after_scaling(opt, H, W)
    if roc == 'none':
        base = float(2 ** opt.n_downsample_global)
        if opt.netG == 'local':
            base *= (2 ** opt.n_local_enhancers)
        sh, sw = int(round(H / base) * base), int(round(W / base) * base)
    if 'crop' in roc and (sw > opt.fineWidth or sh > opt.fineHeight):
        return sh, sw, opt.fineHeight, opt.fineWidth, True
    return sh, sw, sh, sw, False


def _label_tables(opt, dataset, inst_int):
    """(tabs fp32 [4, 256], inst_mode): every per-value statement of the two loaders evaluated on the HOST with the loader's
    own torch operations, for all 256 byte values -- rows: the label of a segm byte, the label where the instance value is 0,
    the value that fills such an instance, the instance value of an inst byte (sdn_assemble_maps)."""
    from sdn_hip import ops as _ops
    lut = _to_tensor_lut()
    A = lut * 255.0
    inst = lut.clone()
    mode = _ops.ASSEMBLE_INST_TABLE
    if opt.inst_precomputed_path:
        inst = inst * 255.0
        inst = inst * 1000
        mode = _ops.ASSEMBLE_INST_FILL
    if dataset == 'vkitti':
        if opt.segm_precomputed_path:
            A = A + 1
        A0 = A.clone()
        if opt.inst_precomputed_path and opt.segm_precomputed_path:   # vkitti_dataset.py:75-78
            A0[A == 2] = 5
            A0[A == 12] = 5
        rows = (A, A0, A0, inst)
    else:
        post = A.clone()
        if not opt.segm_precomputed_path:                             # cityscapes_dataset.py:102-105
            for i, v in enumerate(CITYSCAPES_LABEL_TABLE):
                post[A == i] = v
        rows = (post, post, A, inst)                                  # :63 fills from the label BEFORE the mapping
    if opt.no_instance:
        mode = _ops.ASSEMBLE_INST_NONE
    elif inst_int:
        mode = _ops.ASSEMBLE_INST_INT
    return torch.stack(rows).numpy().astype(np.float32), mode


def _pose_tables(opt, dataset, pose_jsons):
    """(has int32 [B, 256], val int32 [B, 256] | fp32 [B, 256, 2]) by raw pose id p: the record the loader looks up for the
    map value float32(p / 255) * 255 -- cityscapes: d[str(int(value))] (:84); vkitti: the record whose int(key) equals the
    value (assemble_item) -- and np.digitize(alpha / pi, bins), or (cos, sin) of the host's libm rounded to fp32."""
    nb = opt.feat_pose_num_bins
    B = len(pose_jsons)
    value = (_to_tensor_lut() * 255.0).numpy()
    has = np.zeros((B, 256), dtype=np.int32)
    val = np.zeros((B, 256), dtype=np.int32) if nb else np.zeros((B, 256, 2), dtype=np.float32)
    bins = pose_bins(nb) if nb else None
    for b, js in enumerate(pose_jsons):
        if js is None:
            continue
        recs = {}
        if dataset == 'vkitti':
            for key, rec in js.items():
                recs[float(int(key))] = rec
        for p in range(1, 256):
            rec = recs.get(float(value[p])) if dataset == 'vkitti' else js.get(str(int(value[p])))
            if rec is None:
                continue
            alpha = rec['alpha']
            has[b, p] = 1
            if nb:
                val[b, p] = int(np.digitize(alpha / pi, bins))
            else:
                val[b, p] = (cos(alpha), sin(alpha))
    return has, val


def _upload(dev, parts):
    """the host arrays `parts` {name: numpy int32 / fp32 / int64 array} as ONE host-to-device copy: a dict of device views."""
    off, total = {}, 0
    for k, a in parts.items():
        off[k] = total
        total += (a.nbytes // 4 + 3) // 4 * 4   # 16-byte sections: the int64 address tables stay aligned
    blob = np.zeros(total, dtype=np.int32)
    for k, a in parts.items():
        blob[off[k]:off[k] + a.nbytes // 4] = np.ascontiguousarray(a).reshape(-1).view(np.int32)
    d = torch.from_numpy(blob).to(dev)
    kinds = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64}
    return {k: d[off[k]:off[k] + a.nbytes // 4].view(kinds[a.dtype]).view(a.shape) for k, a in parts.items()}


def assemble_batch(opt, params_list, frames, dataset='vkitti', inst_wrap_int16=False):
    """B items of the reference's loader in four kernel launches (csrc/assemble.hip), computing only each item's crop window:
    dataset='vkitti' is vkitti_dataset.__getitem__ (:44-129, bit-equal to assemble_item), dataset='cityscapes' is
    cityscapes_dataset.__getitem__ (:32-111).
      params_list  B dicts {'crop_pos': (x, y), 'flip': bool} (get_params)
      frames       B dicts of decoded maps on ONE GPU, all of one source size: 'segm' uint8 [1, H, W], 'image' uint8 [3, H, W],
                   'inst' uint8 [1, H, W] -- or, for the Cityscapes ground-truth instance ids, an integer [1, H, W] tensor of a
                   wider type, handed through unscaled --, 'pose_inst' uint8 [1, H, W] with 'pose_json' (the geometric branch's
                   NNNNN.png / .json), 'normal' uint8 [3, H, W].  inst / pose_inst / pose_json / normal absent or None: the
                   loader's FileNotFoundError branch of that item.
      inst_wrap_int16  the 16-bit instance map is a mode 'I;16' image: torchvision 0.2.x's ToTensor reads it through np.int16
                   (Cityscapes ids reach 33 999 and come out negative; the result is int16) and Pillow resizes it with its
                   generic transform (_nearest_table_generic).  PIL versions that open the PNG as mode 'I' give int32.
    Returns {'label', 'inst' [B,1,h,w], 'image', 'normal' [B,3,h,w], 'pose' [B,1,h,w] int32 | [B,2,h,w] fp32, 'missing' int32
    [B]} (0 where the loader leaves its default): 'missing' counts the pixels of pose ids that are large enough to be painted
    but have no record in the JSON -- the reference raises KeyError there; they are painted 0.  The tables and the per-item
    parameters go to the device in one copy; nothing is read back.  `--feat_depth` stays with depth_feature."""
    from sdn_hip import ops as _ops
    if dataset not in MIN_POSE_AREA:
        raise ValueError('assemble_batch: dataset must be vkitti or cityscapes, got %r' % (dataset,))
    B = len(frames)
    if B < 1 or len(params_list) != B:
        raise ValueError('assemble_batch: %d frames, %d params' % (B, len(params_list)))
    if opt.label_nc == 0:
        raise NotImplementedError('assemble_batch: label_nc == 0 (the label map as an RGB image) is assemble_item\'s')
    maps = {k: [f.get(k) for f in frames] for k in ('segm', 'image', 'inst', 'pose_inst', 'normal')}
    jsons = [f.get('pose_json') for f in frames]
    planes = {'segm': 1, 'image': 3, 'inst': 1, 'pose_inst': 1, 'normal': 3}
    shape = None
    dev = None
    for k, ts in maps.items():
        for b, t in enumerate(ts):
            if t is None:
                if k in ('segm', 'image'):
                    raise ValueError('assemble_batch: frame %d has no %s' % (b, k))
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError('assemble_batch expects torch tensors, frame %d %s is %r' % (b, k, type(t)))
            if not t.is_cuda:   # as every op of this project: no host path
                raise NotImplementedError('assemble_batch: frame %d %s is on %s; the batched assembly only runs on the GPU'
                                          % (b, k, t.device))
            if t.dim() != 3 or t.shape[0] != planes[k]:
                raise ValueError('assemble_batch: frame %d %s must be [%d, H, W], got %s' % (b, k, planes[k], tuple(t.shape)))
            if shape is None:
                shape, dev = tuple(t.shape[1:]), t.device
            if tuple(t.shape[1:]) != shape:
                raise ValueError('assemble_batch: frame %d %s is %s, the call\'s source size is %s'
                                 % (b, k, tuple(t.shape[1:]), shape))
            if t.device != dev:
                raise ValueError('assemble_batch: frame %d %s is on %s, the call on %s' % (b, k, t.device, dev))
            if t.dtype != torch.uint8 and (k != 'inst' or t.dtype.is_floating_point or t.dtype == torch.bool):
                raise TypeError('assemble_batch: frame %d %s must be uint8, got %s' % (b, k, t.dtype))
    H, W = shape
    use_inst = not opt.no_instance
    wide = [t is not None and t.dtype != torch.uint8 for t in maps['inst']] if use_inst else [False] * B
    if any(wide):
        if opt.inst_precomputed_path:
            raise TypeError('assemble_batch: a precomputed instance map is uint8')
        if not all(wide):
            raise ValueError('assemble_batch: integer and uint8 (or missing) instance maps in one call give tensors of '
                             'different types; assemble them in separate calls')
    sh, sw, h, w, crops = batch_geometry(opt, H, W)
    items = np.zeros((B, 4), dtype=np.int32)
    for b, p in enumerate(params_list):
        if crops:
            items[b, 0], items[b, 1] = int(p['crop_pos'][0]), int(p['crop_pos'][1])
        items[b, 2] = 1 if (opt.isTrain and not opt.no_flip and p['flip']) else 0
    if (items[:, :2] < 0).any():
        raise ValueError('assemble_batch: negative crop position')

    keep = []   # contiguous copies live until the launches are queued

    def addresses(ts, dtype=torch.uint8):
        a = np.zeros(B, dtype=np.int64)
        for b, t in enumerate(ts):
            if t is not None:
                t = t.to(dtype).contiguous()
                keep.append(t)
                a[b] = t.data_ptr()
        return a

    tabs, inst_mode = _label_tables(opt, dataset, any(wide))
    parts = {'items': items, 'lut': _to_tensor_lut().numpy(), 'tabs': tabs, 'segm': addresses(maps['segm']),
             'image': addresses(maps['image'])}
    if sw != W:
        idx, k8 = _resample_table(W, sw, 'bicubic')
        parts['xmin'], parts['xk'] = idx[:, 0].numpy().astype(np.int32), k8.numpy().astype(np.int32)
        parts['nx'] = _nearest_table(W, sw).numpy().astype(np.int32)
    if sh != H:
        idx, k8 = _resample_table(H, sh, 'bicubic')
        parts['ymin'], parts['yk'] = idx[:, 0].numpy().astype(np.int32), k8.numpy().astype(np.int32)
        parts['ny'] = _nearest_table(H, sh).numpy().astype(np.int32)
    if any(wide) and inst_wrap_int16:   # a mode 'I;16' map: the generic transform's indices on every axis that changes
        if sw != W:
            parts['inst_nx'] = _nearest_table_generic(W, sw).numpy().astype(np.int32)
        if sh != H:
            parts['inst_ny'] = _nearest_table_generic(H, sh).numpy().astype(np.int32)
    if use_inst:
        parts['inst'] = addresses(maps['inst'], torch.int32 if any(wide) else torch.uint8)
    if opt.feat_pose:
        present = [t if js is not None else None for t, js in zip(maps['pose_inst'], jsons)]
        parts['pose'] = addresses(present)
        parts['pose_has'], parts['pose_val'] = _pose_tables(opt, dataset, [js if t is not None else None
                                                                           for t, js in zip(maps['pose_inst'], jsons)])
    if opt.feat_normal:
        parts['normal'] = addresses(maps['normal'])
    with torch.cuda.device(dev):
        d = _upload(dev, parts)
        xtab = (d['xmin'], d['xk']) if sw != W else None
        ytab = (d['ymin'], d['yk']) if sh != H else None
        out = {'label': 0, 'inst': 0, 'image': 0, 'pose': 0, 'normal': 0}
        out['image'] = _ops.assemble_planes(d['image'], items, d['items'], xtab, ytab, d['lut'], 3, H, W, sh, sw, h, w)
        if opt.feat_normal:   # "bias caused by 0..256 instead 0..255" (vkitti_dataset.py:125, cityscapes_dataset.py:98)
            out['normal'] = _ops.assemble_planes(d['normal'], items, d['items'], xtab, ytab, d['lut'], 3, H, W, sh, sw, h, w,
                                                 add=np.float32(1 / 255))
        label, inst, pose, missing = _ops.assemble_maps(
            d['segm'], d.get('inst'), d.get('pose'), items, d['items'], d.get('nx'), d.get('ny'), d['tabs'], inst_mode, H, W, sh,
            sw, h, w, wrap16=inst_wrap_int16, pose_has=d.get('pose_has'), pose_val=d.get('pose_val'),
            min_area=MIN_POSE_AREA[dataset], inst_nx=d.get('inst_nx'), inst_ny=d.get('inst_ny'))
    out['label'], out['missing'] = label, missing
    if use_inst:
        out['inst'] = inst
    if opt.feat_pose:
        out['pose'] = pose
    return out
