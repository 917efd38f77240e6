"""Test helpers of the batched loader (csrc/assemble.hip, textural/data/assemble.py: assemble_batch):
  * cityscapes_item: textural/data/cityscapes_dataset.py:32-111 restated statement by statement on REAL PIL images that are
    handed in instead of being opened from files (get_transform and ToTensor are oracle/loader_oracle.py's);
  * emulate_planes / emulate_maps: the two kernels' integer algorithm in numpy, window-only evaluation included -- what is
    outside an item's window is never computed (it is poisoned, so that a read of it shows);
  * fixture access for tests/golden/cityscapes_loader_golden.npz.
"""
import json
import os
from math import cos, pi, sin
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from oracle import loader_oracle as lo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cityscapes_loader_golden.npz')
OPT_KEYS = ('resize_or_crop', 'loadSize', 'fineWidth', 'fineHeight', 'isTrain', 'no_flip', 'n_downsample_global', 'netG',
            'n_local_enhancers', 'label_nc', 'no_instance', 'feat_pose_num_bins')


def cityscapes_item(opt, params, A, B, inst=None, pose_inst=None, pose_json=None, normal_map=None, label_table=None):
    """cityscapes_dataset.py:32-111; a missing file (FileNotFoundError branch) is None.  label_table[id] = trainId + 1, 0 for
    void: `self.labels` as integers."""
    transform_A = lo.get_transform(opt, params, method=Image.NEAREST, normalize=False)
    A_tensor = transform_A(A) * 255.0
    B_tensor = inst_tensor = pose_tensor = normal_tensor = 0
    transform_B = lo.get_transform(opt, params)
    B_tensor = transform_B(B.convert('RGB'))
    if not opt.no_instance:
        if inst is not None:
            inst_tensor = transform_A(inst)
            if opt.inst_precomputed_path:
                inst_tensor = inst_tensor * 255.0
                inst_tensor *= 1000
                inst_tensor[inst_tensor == 0] = A_tensor[inst_tensor == 0]
        else:
            inst_tensor = A_tensor
    if opt.feat_pose:
        if opt.feat_pose_num_bins > 0:
            pose_tensor = np.zeros((1, A_tensor.size(1), A_tensor.size(2)))
        else:
            pose_tensor = np.zeros((2, A_tensor.size(1), A_tensor.size(2)))
        if pose_inst is not None and pose_json is not None:
            d = pose_json
            inst_map = transform_A(pose_inst) * 255.0
            inst_map = inst_map.numpy()[0]
            if opt.feat_pose_num_bins:
                bins = np.array(list(range(-180, 181, 360 // opt.feat_pose_num_bins))) / 180
            for i in np.unique(inst_map):
                if i == 0 or (inst_map == i).sum() < 256:
                    continue
                alpha = d[str(int(i))]['alpha']
                if opt.feat_pose_num_bins > 0:
                    pose_tensor[0, inst_map == i] = np.digitize(alpha / pi, bins)
                else:
                    pose_tensor[0, inst_map == i] = cos(alpha)
                    pose_tensor[1, inst_map == i] = sin(alpha)
        pose_tensor = torch.from_numpy(pose_tensor)
        pose_tensor = pose_tensor.int() if opt.feat_pose_num_bins else pose_tensor.float()
    if opt.feat_normal:
        if normal_map is not None:
            normal_tensor = transform_B(normal_map) + 1 / 255
        else:
            normal_tensor = torch.zeros(B_tensor.size())
    if not opt.segm_precomputed_path:
        _A_tensor = A_tensor.clone()
        for i, v in enumerate(label_table):
            A_tensor[_A_tensor == i] = v
    return {'label': A_tensor, 'inst': inst_tensor, 'image': B_tensor, 'pose': pose_tensor, 'normal': normal_tensor}


# ---------------------------------------------------------------------------------------------------------------------
BITS = 22
POISON = -(1 << 20)


def _window(asm, opt, params, H, W):
    sh, sw, h, w, crops = asm.batch_geometry(opt, H, W)
    x1, y1 = (int(params['crop_pos'][0]), int(params['crop_pos'][1])) if crops else (0, 0)
    flip = bool(opt.isTrain and not opt.no_flip and params['flip'])
    return sh, sw, h, w, x1, y1, flip


def emulate_planes(asm, opt, params, src, method='bicubic', normalize=True, add=None):
    """k_assemble_planes for one item: src uint8 [C, H, W] numpy.  The horizontal pass runs for the source rows
    the window's rows need and the window's columns only; everything else stays POISON."""
    C, H, W = src.shape
    sh, sw, h, w, x1, y1, flip = _window(asm, opt, params, H, W)
    lut = asm._to_tensor_lut().numpy()
    xs = x1 + np.arange(w)
    ys = y1 + np.arange(h)
    xin, yin = xs < sw, ys < sh
    src = src.astype(np.int64)
    if sh != H:
        yidx, yk = (t.numpy() for t in asm._resample_table(H, sh, method))
        rows = np.unique(yidx[ys[yin]])
    else:
        rows = ys[yin]
    hp = np.full((C, H, w), POISON, dtype=np.int64)   # [plane, source row, window column]
    cols = xs[xin]
    if sw != W:
        xidx, xk = (t.numpy() for t in asm._resample_table(W, sw, method))
        acc = (src[:, rows][:, :, xidx[cols]] * xk[cols][None, None]).sum(-1) + (1 << (BITS - 1))
        hp[:, rows[:, None], np.nonzero(xin)[0][None, :]] = np.clip(acc >> BITS, 0, 255)
    else:
        hp[:, rows[:, None], np.nonzero(xin)[0][None, :]] = src[:, rows][:, :, cols]
    win = np.zeros((C, h, w), dtype=np.int64)   # PIL's crop: 0 beyond the scaled image
    vy, vx = np.nonzero(yin)[0], np.nonzero(xin)[0]
    if sh != H:
        taps = hp[:, yidx[ys[yin]]][:, :, :, vx]                      # [C, rows, ksize, cols]
        assert (taps != POISON).all(), 'the vertical pass read a pixel the horizontal pass did not compute'
        acc = (taps * yk[ys[yin]][None, :, :, None]).sum(2) + (1 << (BITS - 1))
        win[:, vy[:, None], vx[None, :]] = np.clip(acc >> BITS, 0, 255)
    else:
        win[:, vy[:, None], vx[None, :]] = hp[:, ys[yin]][:, :, vx]
    assert (win != POISON).all()
    if flip:
        win = win[:, :, ::-1]
    f = lut[win]
    if normalize:
        f = (f - np.float32(0.5)) / np.float32(0.5)
    if add is not None:
        f = f + np.float32(add)
    return f.astype(np.float32)


def emulate_maps(asm, opt, params, dataset, segm, inst=None, pose_inst=None, pose_json=None, wrap16=False):
    """k_assemble_gather + k_assemble_paint for one item: segm / inst / pose_inst numpy [H, W] (inst of a wider integer type: the
    ground-truth ids, handed through).  Returns (label, inst, pose, missing, counts)."""
    from sdn_hip import ops
    H, W = segm.shape
    sh, sw, h, w, x1, y1, flip = _window(asm, opt, params, H, W)
    wide = inst is not None and inst.dtype != np.uint8
    tabs, mode = asm._label_tables(opt, dataset, wide)
    y, x = np.mgrid[0:h, 0:w]
    xs, ys = x1 + (w - 1 - x if flip else x), y1 + y
    inside = (xs < sw) & (ys < sh)
    nx = asm._nearest_table(W, sw).numpy() if sw != W else np.arange(W)
    ny = asm._nearest_table(H, sh).numpy() if sh != H else np.arange(H)
    sx, sy = nx[np.where(inside, xs, 0)], ny[np.where(inside, ys, 0)]

    def gather(m):
        return np.where(inside, m[sy, sx], 0)
    s = gather(segm)
    label = tabs[0][s]
    inst_out = None
    if mode != ops.ASSEMBLE_INST_NONE:
        if inst is None:
            inst_out = label.copy()
        elif mode == ops.ASSEMBLE_INST_INT:
            if wrap16 and (sw != W or sh != H):   # a mode 'I;16' image: Pillow's generic transform, whichever axis changes
                gx = asm._nearest_table_generic(W, sw).numpy() if sw != W else np.arange(W)
                gy = asm._nearest_table_generic(H, sh).numpy() if sh != H else np.arange(H)
                inst_out = np.where(inside, inst.astype(np.int32)[gy[np.where(inside, ys, 0)], gx[np.where(inside, xs, 0)]], 0)
            else:
                inst_out = gather(inst.astype(np.int32))
            inst_out = inst_out.astype(np.int16) if wrap16 else inst_out.astype(np.int32)
        else:
            v = tabs[3][gather(inst)]
            if mode == ops.ASSEMBLE_INST_FILL:
                zero = v == 0
                label = np.where(zero, tabs[1][s], label)
                v = np.where(zero, tabs[2][s], v)
            inst_out = v
    pose = missing = counts = None
    if opt.feat_pose:
        nb = opt.feat_pose_num_bins
        has, val = asm._pose_tables(opt, dataset, [pose_json if pose_inst is not None else None])
        pose = np.zeros((1, h, w), np.int32) if nb else np.zeros((2, h, w), np.float32)
        missing = 0
        counts = np.zeros(256, dtype=np.int64)
        if pose_inst is not None and pose_json is not None:
            ids = gather(pose_inst)
            counts = np.bincount(ids.reshape(-1), minlength=256)
            paint = (ids != 0) & (counts[ids] >= asm.MIN_POSE_AREA[dataset])
            known = has[0][ids] == 1
            missing = int((paint & ~known).sum())
            if nb:
                pose[0] = np.where(paint & known, val[0][ids], 0)
            else:
                pose[:] = np.where((paint & known)[None], val[0][ids].transpose(2, 0, 1), np.float32(0))
    return label[None].astype(np.float32), None if inst_out is None else inst_out[None], pose, missing, counts


# ---------------------------------------------------------------------------------------------------------------------
def load_gold():
    return np.load(GOLD)


def case_opt(z, ci):
    cfg = json.loads(str(z['c%d/cfg' % ci]))
    opt = SimpleNamespace(**{k: cfg[k] for k in OPT_KEYS})
    opt.segm_precomputed_path = 'p' if cfg['segm_precomputed'] else ''
    opt.inst_precomputed_path = 'q' if cfg['inst_precomputed'] else ''
    opt.feat_pose = 'x'
    opt.feat_normal = 'x'
    return opt, cfg


def case_item(z, ci, i):
    """(params, sources) of item i of case ci: sources = dict of numpy maps as the loader's files held them (None: no file)"""
    opt, cfg = case_opt(z, ci)
    q = 'c%d/i%d/' % (ci, i)
    f = 'f%d/' % int(z[q + 'frame'])
    params = {'crop_pos': (int(z[q + 'crop_pos'][0]), int(z[q + 'crop_pos'][1])), 'flip': bool(z[q + 'flip'])}
    src = {'segm': z[f + 'segm'], 'image': z[f + 'rgb'], 'inst': None, 'pose_inst': None, 'pose_json': None, 'normal': None}
    if 'inst' in cfg['files']:
        src['inst'] = z[f + 'inst8'] if cfg['inst_precomputed'] else z[f + 'inst16']
    if 'pose' in cfg['files']:
        src['pose_inst'], src['pose_json'] = z[f + 'posemap'], json.loads(str(z[f + 'json']))
    if 'normal' in cfg['files']:
        src['normal'] = z[f + 'normalmap']
    return params, src


def case_expected(z, ci, i):
    return {k: z['c%d/i%d/%s' % (ci, i, k)] for k in ('label', 'inst', 'image', 'pose', 'normal')}


def wraps_int16(z, ci):
    return str(z['c%d/inst_mode' % ci]) == 'I;16'


def pil(a):
    """a source map as the PIL image the loader opens: uint8 [H, W] 'L', [H, W, 3] 'RGB', uint16 [H, W] a 16-bit PNG"""
    if a.dtype == np.uint16:
        import io
        b = io.BytesIO()
        Image.fromarray(a).save(b, 'PNG')
        b.seek(0)
        return Image.open(b)
    return Image.fromarray(a, 'RGB' if a.ndim == 3 else 'L')
