"""The proposal layer on the device: proposal_layer (reference: geometric/maskrcnn/model.py:344-407, with apply_box_deltas of :307-328
and clip_boxes of :331-341), the step between the RPN heads and pyramid_roi_align, once per image in inference and in training
(:1747-1751).

    from maskrcnn.proposals import proposal_layer        # instead of the one in maskrcnn.model
    rpn_rois = proposal_layer([rpn_class, rpn_bbox], proposal_count, nms_threshold, anchors, config)

The reference sorts all anchor scores (261 888 for a 1024 x 1024 image) to use the best 6000, gathers three times, decodes and clips in
about twenty element-wise launches and runs an NMS whose CUDA path copies the pair mask to the host.  Here an exact radix select finds
the 6000th score, one workgroup sorts the survivors, decodes and clips them, and the NMS of csrc/raster_boxes.hip, stopped at
proposal_count, writes the normalised boxes itself: csrc/proposal_layer.hip behind sdn_hip.ops.proposal_layer.  CPU tensors raise
NotImplementedError and there is no torch form.  Selection, order and the kept set follow torch.sort(descending=True, stable=True) and
this project's pth_nms exactly; the boxes are the reference's fp32 arithmetic operation by operation, expf being the only operation
whose last bit may differ from a CPU run.  No result carries a gradient, as in the reference (:473; detection_target_layer takes
.data).
"""
from sdn_hip import ops


def proposals_padded(inputs, proposal_count, nms_threshold, anchors, config=None, pre_nms_limit=6000, strict=True):
    """(rois fp32 [1, proposal_count, 4], count int32 [1]): the proposals of proposal_layer below in a buffer of fixed size, rows behind
    count +0.0, with nothing crossing to the host -- the form for a caller that keeps the step on the device (a captured graph, a
    training step without host waits).  No result carries a gradient."""
    inputs = list(inputs)
    if len(inputs) != 2:
        raise ValueError('inputs must be [rpn_probs, rpn_bbox], got %d entries' % len(inputs))
    if config is None:
        raise ValueError('config is needed: RPN_BBOX_STD_DEV and IMAGE_SHAPE are read from it (model.py:367, :385)')
    height, width = config.IMAGE_SHAPE[:2]
    _order, _boxes_px, _keep, count, rois = ops.proposal_layer(inputs[0], inputs[1], anchors, config.RPN_BBOX_STD_DEV, height, width,
                                                               proposal_count, nms_threshold, pre_nms_limit=pre_nms_limit, strict=strict)
    return rois.unsqueeze(0), count


def proposal_layer(inputs, proposal_count, nms_threshold, anchors, config=None):
    """The reference's proposal_layer (model.py:344-407), name, signature and return value.  inputs = [rpn_probs, rpn_bbox]: fp32
    [1, A, 2] = (bg, fg) and fp32 [1, A, 4] (or without the batch axis), anchors fp32 [A, 4] = (y1, x1, y2, x2) in pixels, contiguous
    CUDA tensors; config gives RPN_BBOX_STD_DEV and IMAGE_SHAPE.  Returns the proposals fp32 [1, n, 4] in normalised coordinates,
    n <= proposal_count, best score first.  The result carries no gradient (:473).

    The size of the result depends on the data, as in the reference, so the kept count is read once: the call's only host wait
    (proposals_padded has none).  Unlike the reference, `inputs` is not changed (it squeezes the list's entries in place, :359-360),
    and suppression is on IoU > nms_threshold, the rule of the reference's CUDA kernel.  A batch other than 1, no anchors, 2^24 anchors
    or more, differing anchor counts, proposal_count < 1 or above 6000 raise ValueError; CPU, non-fp32 and non-contiguous tensors raise
    NotImplementedError, TypeError and ValueError."""
    rois, count = proposals_padded(inputs, proposal_count, nms_threshold, anchors, config)
    return rois[:, :int(count.item())]
