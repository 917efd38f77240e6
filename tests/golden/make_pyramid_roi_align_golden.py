#!/usr/bin/env python3
"""Generate tests/golden/pyramid_roi_align_golden.npz: the reference's pyramid RoIAlign, EXECUTED from its own source.

geometric/maskrcnn/model.py cannot be imported here (old torch idioms, its compiled nms / roialign extensions).  This script takes
with `ast`, from where they lie, log2 (model.py:95-100) and pyramid_roi_align (:414-502) and runs them under the installed torch on
the CPU in float32, on the seeded inputs of tests/pyramid_roi_align_util.py.  The one name they need from the compiled extension,
CropAndResizeFunction, is bound to an autograd wrapper around oracle.maskrcnn_np.crop_forward / crop_backward with impl='ref': the
reference's own crop_and_resize.c, compiled unmodified by oracle/build_ref.py into oracle/_ref.

Per case the fixture holds: the checksums of the inputs, the boxes, the level of every box, the pooled output (in full for the
small cases, its checksum always), the reference's float32 gradients of the four maps for the seeded `grads`, the float64
gradients of the restatement, the float32 run's distance from them per level map (relative to the map's largest float64 gradient
magnitude) and the GPU test's gate per level map: 1e-6, or 4 x that distance where the reference's own float32 sum does not stay
within 1e-6.  Before anything is stored the restatement's levels are asserted equal to the reference's on every case, and its
float32 forward equal to the reference's bit for bit.  Only data goes into the fixture.  Runs only where the reference exists."""
import ast
import os
import sys

import numpy as np
import torch
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pyramid_roi_align_util as u   # noqa: E402
from oracle import maskrcnn_np as mnp   # noqa: E402

REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
MODEL = os.path.join(REF, 'geometric', 'maskrcnn', 'model.py')
FUNCTIONS = (('log2', 95, 100), ('pyramid_roi_align', 414, 502))


class _RefCrop(torch.autograd.Function):
    """crop_and_resize.py:10-49 of the reference, on its C code through oracle/_ref"""

    @staticmethod
    def forward(ctx, image, boxes, box_ind, crop_height, crop_width, extrapolation_value, calls):
        calls.append((image.data_ptr(), boxes.numpy().copy()))
        crops = mnp.crop_forward(image.numpy(), boxes.numpy(), box_ind.numpy(), crop_height, crop_width, extrapolation_value, impl='ref')
        ctx.save_for_backward(boxes, box_ind)
        ctx.im_size = tuple(image.shape)
        return torch.from_numpy(crops)

    @staticmethod
    def backward(ctx, grad_outputs):
        boxes, box_ind = ctx.saved_tensors
        g = mnp.crop_backward(grad_outputs.contiguous().numpy(), boxes.numpy(), box_ind.numpy(), ctx.im_size, impl='ref')
        return torch.from_numpy(g), None, None, None, None, None, None


def reference_functions(calls):
    class CropAndResizeFunction(object):
        def __init__(self, crop_height, crop_width, extrapolation_value=0):
            self.args = (crop_height, crop_width, extrapolation_value)

        def __call__(self, image, boxes, box_ind):
            assert box_ind.dtype == torch.int32 and image.dim() == 4 and image.shape[0] == 1
            return _RefCrop.apply(image, boxes, box_ind, *self.args, calls)

    body = ast.parse(open(MODEL).read()).body
    ns = {'torch': torch, 'Variable': Variable, 'CropAndResizeFunction': CropAndResizeFunction}
    for name, first, last in FUNCTIONS:
        (fn,) = [st for st in body if isinstance(st, ast.FunctionDef) and st.name == name]
        assert (fn.lineno, fn.end_lineno) == (first, last), (name, fn.lineno, fn.end_lineno)
        exec(compile(ast.Module(body=[fn], type_ignores=[]), MODEL, 'exec'), ns)
    return ns


def run_reference(ns, calls, c):
    """(levels [R], pooled [R, C, p, p] float32, the four maps' float32 gradients) of the reference's own code"""
    del calls[:]
    boxes = torch.from_numpy(c['boxes'].copy())
    maps = [torch.from_numpy(m.copy())[None].requires_grad_() for m in c['maps']]
    inputs = [boxes[None]] + maps
    pooled = ns['pyramid_roi_align'](inputs, c['pool'], u.IMAGE_SHAPE)
    assert tuple(pooled.shape) == (c['R'], c['C'], c['pool'], c['pool']) and pooled.dtype == torch.float32
    pooled.backward(torch.from_numpy(c['grads'].copy()))
    grads = [m.grad[0].numpy() if m.grad is not None else np.zeros(m.shape[1:], np.float32) for m in maps]
    # the level of every box, from what the reference handed to its crop: which map, which boxes
    where = {m.data_ptr(): l for l, m in enumerate(maps)}
    rows = {c['boxes'][r].tobytes(): r for r in range(c['R'])}
    assert len(rows) == c['R'], 'two equal boxes'
    levels = np.zeros(c['R'], np.int32)
    for image_ptr, level_boxes in calls:
        for b in level_boxes:
            levels[rows[b.tobytes()]] = where[image_ptr] + 2
    assert levels.min() >= 2 and sum(len(b) for _, b in calls) == c['R']
    return levels, pooled.detach().numpy(), grads


def main():
    assert mnp.have('ref'), 'oracle/_ref/libmaskrcnn_ref.so is missing: run `python __graft_entry__.py build` where the reference exists'
    calls = []
    ns = reference_functions(calls)
    out = {'image_shape': np.asarray(u.IMAGE_SHAPE, np.int64)}
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        levels, pooled, grads32 = run_reference(ns, calls, c)
        # the restatement is the reference: levels equal, the float32 forward equal bit for bit
        assert np.array_equal(u.levels(c), levels), (name, u.levels(c), levels)
        assert (u.margin(u.level_values(c['boxes'])) > u.MARGIN).all(), name
        mine32 = u.forward(c, np.float32)
        assert mine32.dtype == np.float32 and mine32.tobytes() == pooled.tobytes(), name
        mine32_back = u.backward(c, np.float32)
        grads64 = u.backward(c, np.float64)
        err = u.grad_error(grads32, grads64)
        assert np.isfinite(err).all() and (u.grad_error(mine32_back, grads64) < 1e-4).all(), (name, err)
        gate = u.gate_of(err)
        for l in range(u.LEVELS):
            if not (levels == l + 2).any():
                assert not grads32[l].any() and not grads64[l].any() and err[l] == 0.0, (name, l)
        print('%-10s levels %s; float32 run within %s of the float64 gradients; gates %s'
              % (name, np.bincount(levels - 2, minlength=4).tolist(), ' '.join('%.2e' % e for e in err), ' '.join('%.2e' % g for g in gate)))
        out[p + 'crc_boxes'] = np.uint32(u.checksum(c['boxes']))
        out[p + 'crc_grads'] = np.uint32(u.checksum(c['grads']))
        out[p + 'crc_maps'] = np.asarray([u.checksum(m) for m in c['maps']], np.uint32)
        out[p + 'boxes'] = c['boxes']
        out[p + 'levels'] = levels.astype(np.int8)
        out[p + 'crc_pooled'] = np.uint32(u.checksum(pooled))
        if name in u.STORED_WHOLE:
            out[p + 'pooled'] = pooled
        for l in range(u.LEVELS):
            out[p + 'grad32_%d' % l] = grads32[l]
            out[p + 'grad64_%d' % l] = grads64[l]
        out[p + 'fp32_error'], out[p + 'gate'] = err, gate

    # what the cases are there for
    lv = {name: out[name + '/levels'] for name in u.CASES}
    assert all(set(lv[n].tolist()) == {2, 3, 4, 5} for n in ('mixed7', 'mixed14', 'big', 'thin'))
    assert np.array_equal(out['mixed7/boxes'], out['mixed14/boxes']) and np.array_equal(lv['mixed7'], lv['mixed14'])
    assert set(lv['onelevel'].tolist()) == {3} and set(lv['clamp'].tolist()) == {2, 5}
    v = u.level_values(out['clamp/boxes'])
    assert (v < 1.5).sum() == 8 and (v > 5.5).sum() == 8
    v = u.level_values(out['degenerate/boxes'])
    assert np.isneginf(v[:3]).all() and np.isnan(v[3:5]).all() and np.isfinite(v[5]) and lv['degenerate'].tolist() == [2, 2, 2, 2, 2, 5]
    b = out['outside/boxes']
    assert ((b.min(1) < 0) | (b.max(1) > 1)).all()
    o = out['outside/pooled']
    assert (o == 0).all(axis=1).any() and (o != 0).any()              # some samples off the map, in every channel at once
    assert len(lv['single']) == 1 and len(lv['big']) == 1000 and u.CASES['c67']['C'] % u.CHANNELS == 3

    path = u.GOLD
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print('wrote %s: %d arrays, %.1f KiB' % (path, len(out), size / 1024))


if __name__ == '__main__':
    sys.exit(main())
