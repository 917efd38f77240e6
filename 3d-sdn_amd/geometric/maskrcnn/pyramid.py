"""RoIAlign over the feature pyramid on the device: pyramid_roi_align (reference: geometric/maskrcnn/model.py:414-502, with log2
of :95-100), the first step of the classifier and the mask head (:939, 979), in inference and in training.

    from maskrcnn.pyramid import pyramid_roi_align       # instead of the one in maskrcnn.model
    x = pyramid_roi_align([rois] + feature_maps, pool_size, image_shape)

The reference walks the four levels on the host: per level an ix.any() and a torch.nonzero, each of which waits for the device, an
index gather, one crop, and at the end two cats, a sort and a gather that copies the whole result once more.  Here a box's level is
computed where the box is sampled and row r of the result is box r: one launch forward, a zero fill and one scatter launch backward,
nothing crosses to the host.  The kernels are csrc/pyramid_roi_align.hip behind sdn_hip.ops.pyramid_roi_align; CPU tensors raise
NotImplementedError and there is no torch form.  The values are those of the reference's crop_and_resize.c bit for bit; by default
the map gradients are sums of fp32 atomic adds (as in the reference's CUDA kernel) and so not bit-reproducible from run to run.
Under torch.use_deterministic_algorithms(True) or SDN_DETERMINISTIC=1 the backward is a record launch and one gather launch
instead (sdn_pyramid_roi_align_bwd_ordered): every gradient element is a fixed-order sum stored once, the same bits every run;
sdn_hip.ops.pyramid_backward_path() tells which of the two a backward would take.
"""
import torch

from sdn_hip import ops


def _squeezed(t, name, dims):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(t)))
    if t.dim() == dims + 1:
        if t.shape[0] != 1:
            raise ValueError('%s has batch %d; only 1 is supported, as in the reference ("Currently only supports batchsize 1", '
                             'geometric/maskrcnn/model.py:433)' % (name, t.shape[0]))
        return t.squeeze(0)        # a view both ways: its backward is an unsqueeze, where t[0]'s would zero and copy a whole map
    if t.dim() != dims:
        raise ValueError('%s must have %d or %d dimensions, got %s' % (name, dims, dims + 1, tuple(t.shape)))
    return t


def pyramid_levels(inputs, pool_size, image_shape):
    """(pooled fp32 [R, C, pool_size, pool_size], levels int32 [R]): pyramid_roi_align below together with the level (2 .. 5) every box
    was sampled from."""
    inputs = list(inputs)
    if len(inputs) != 1 + ops.PYRAMID_LEVELS:
        raise ValueError('inputs must be [boxes, P2, P3, P4, P5], got %d entries (%d feature maps)' % (len(inputs), max(len(inputs) - 1, 0)))
    boxes = _squeezed(inputs[0], 'boxes', 2)
    maps = [_squeezed(m, 'P%d' % (l + 2), 3) for l, m in enumerate(inputs[1:])]
    if boxes.shape[1] != 4:
        raise ValueError('boxes must be [1, R, 4] or [R, 4], got %s' % (tuple(inputs[0].shape),))
    for l, m in enumerate(maps):
        if m.shape[0] != maps[0].shape[0]:
            raise ValueError('P%d has %d channels, P2 %d' % (l + 2, m.shape[0], maps[0].shape[0]))
    return ops.pyramid_roi_align(boxes, maps, pool_size, float(image_shape[0] * image_shape[1]))


def pyramid_roi_align(inputs, pool_size, image_shape):
    """The reference's pyramid_roi_align (model.py:414-502), name, signature and return value.  inputs = [boxes, P2, P3, P4, P5]: boxes
    fp32 [1, R, 4] = (y1, x1, y2, x2) normalised, the maps fp32 [1, C, H_l, W_l] (or without the batch axis), contiguous CUDA tensors;
    pool_size an int (1 .. 32); image_shape = (height, width, ...) of the input image in pixels.  Returns the pooled regions fp32
    [R, C, pool_size, pool_size] in the order of the boxes, differentiable in the four maps; the boxes get no gradient (:473).

    Unlike the reference, `inputs` is not changed (it squeezes the list's entries in place, :434-435), and R = 0 returns an empty
    [0, C, pool_size, pool_size] where the reference fails in torch.cat (:492).  A box of area <= 0 or with a NaN goes to P2, as in the
    reference's CPU run.  A batch other than 1, fewer or more than four maps or differing channel counts raise ValueError; CPU,
    non-fp32 and non-contiguous tensors raise NotImplementedError, TypeError and ValueError."""
    return pyramid_levels(inputs, pool_size, image_shape)[0]
