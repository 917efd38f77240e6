"""Shared by tests/test_scene2d_host.py and tests/test_gpu_scene2d.py: the 2D / 2D+ baselines (geometric/scripts/main.py
:215-322) restated with PIL.Image and torch CPU float32 tensors -- Pillow itself, executed here, is the yardstick -- and a
numpy emulation of the arithmetic of csrc/scene_paint2d.hip on the product's host tables."""
import numpy as np
import PIL.Image
import torch


# ------------------------------------------------------------------------------------------- the PIL restatement
def geometry(rois, operations, use_ry=False):
    """centres, extents (float32 [N, 2], pixels) and interests after the operations; every float32 statement in the
    reference's order"""
    r = torch.tensor(np.asarray(rois), dtype=torch.int32)
    centre = torch.stack([r[:, 2] + r[:, 0], r[:, 3] + r[:, 1]], dim=1).float() / 2.0
    extent = torch.stack([r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]], dim=1).float()
    keep = torch.ones(len(r)).byte()
    if operations:
        at = torch.tensor([[float(o['from']['v']), float(o['from']['u'])] for o in operations])
        d2 = torch.sum((centre[:, None, :] - at[None, :, :]) ** 2, dim=2)
        if len(centre) < len(at):
            pairs = [(obj, int(op)) for obj, op in enumerate(torch.argmin(d2, dim=1))]
        else:
            pairs = [(int(obj), op) for op, obj in enumerate(torch.argmin(d2, dim=0))]
        for obj, k in pairs:
            o = operations[k]
            u, v = float(o['from']['u']), float(o['from']['v'])
            if o['type'] == 'delete':
                keep[obj] = 0
            elif o['type'] == 'modify':
                to_u, to_v = float(o['to'].get('u', u)), float(o['to'].get('v', v))
                zoom, ry = float(o['zoom']), float(o['ry'])
                centre[obj] = centre[obj] + torch.tensor([to_v - v, to_u - u])
                if use_ry:
                    extent[obj] = torch.tensor([zoom * extent[obj, 0], zoom * float(np.cos(ry)) * extent[obj, 1]])
                else:
                    extent[obj] = zoom * extent[obj]
    return centre, extent, [bool(k) for k in keep.tolist()]


def boxes(centre, extent):
    """(output rows, output columns, paste top, paste left) per object"""
    return [(int(extent[i, 0]), int(extent[i, 1]), int(centre[i, 0] - extent[i, 0] / 2), int(centre[i, 1] - extent[i, 1] / 2))
            for i in range(len(centre))]


def pasted_mask(mask, roi, box, height, width):
    """one object's resized mask in the frame: float32 [1, H, W] of 0.0 / 1.0.  mask: float [H, W] holding 0 / 1."""
    oh, ow, top, left = box
    y0, x0, y1, x1 = [int(v) for v in roi]
    pil = PIL.Image.fromarray(np.uint8(np.asarray(mask)[y0:y1, x0:x1] * 255))
    assert pil.mode == 'L'
    pil = pil.resize((ow, oh), PIL.Image.BILINEAR)
    canvas = PIL.Image.new('L', (width, height))
    canvas.paste(pil, box=(left, top))
    t = torch.from_numpy(np.array(canvas, dtype=np.uint8)[None]).float().div(255)
    return torch.round(t)


def baseline(class_ids, masks, rois, operations, use_ry=False):
    """the edited instance map, JSON record and interests of one operation list: (uint8 [1, H, W] array, dict, list)"""
    masks = np.asarray(masks, dtype=np.float32)
    n, _, height, width = masks.shape
    centre, extent, keep = geometry(rois, operations, use_ry)
    bx = boxes(centre, extent)
    inst = torch.zeros(1, height, width)
    js = {}
    for i in range(n):
        if keep[i]:
            js[i + 1] = {'class_id': int(class_ids[i])}
            m = pasted_mask(masks[i, 0], rois[i], bx[i], height, width)
            inst = (1 - m) * inst + m * (1 + i)
    return inst.numpy().astype(np.uint8), js, keep


def reference_map(masks):
    """the unedited masks painted in index order: uint8 [1, H, W] array"""
    masks = torch.from_numpy(np.asarray(masks, dtype=np.float32))
    inst = torch.zeros_like(masks[0])
    for i in range(len(masks)):
        inst = (1 - masks[i]) * inst + masks[i] * (1 + i)
    return inst.numpy().astype(np.uint8)


# ------------------------------------------------------------------------------------------- the kernel's arithmetic
def emulate_paint(masks, records, bounds, kk8):
    """k_scene_paint2d in numpy on the host tables of derender3d.scene2d.paint_tables -> uint8 [F, 1, H, W]"""
    masks = np.asarray(masks, dtype=np.float32)
    n, _, H, W = masks.shape
    F = records.shape[0]
    out = np.zeros((F, 1, H, W), dtype=np.uint8)
    half = 1 << 21

    def one_pass(img, axis, boff, koff, ksize, size):
        if ksize == 0:
            assert img.shape[axis] == size
            return img
        img = np.moveaxis(img, axis, 0)
        b = bounds[boff:boff + size].astype(np.int64)
        k = kk8[koff:koff + size * ksize].reshape(size, ksize).astype(np.int64)
        res = np.zeros((size,) + img.shape[1:], dtype=np.int64)
        for o in range(size):
            s0, c = b[o]
            res[o] = half + (img[s0:s0 + c] * k[o, :c, None]).sum(axis=0)
        return np.moveaxis(np.clip(res >> 22, 0, 255), 0, axis)

    for f in range(F):
        for i in range(n):                       # ascending: a later object overwrites, as the kernel's downward walk finds
            active, r0, c0, h, w, oh, ow, top, left = [int(v) for v in records[f, i, :9]]
            if not active:
                continue
            win = (masks[i, 0, r0:r0 + h, c0:c0 + w] != 0).astype(np.int64) * 255
            res = one_pass(one_pass(win, 1, *[int(v) for v in records[f, i, 12:15]], ow), 0, *[int(v) for v in records[f, i, 9:12]], oh)
            ya, yb, xa, xb = max(top, 0), min(top + oh, H), max(left, 0), min(left + ow, W)
            if ya >= yb or xa >= xb:
                continue
            hit = res[ya - top:yb - top, xa - left:xb - left] >= 128
            out[f, 0, ya:yb, xa:xb][hit] = i + 1
    return out
