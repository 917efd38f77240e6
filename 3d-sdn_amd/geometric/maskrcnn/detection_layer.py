"""The detection layer on the device: detection_layer / refine_detections (reference: geometric/maskrcnn/model.py:731-855, with
apply_box_deltas of :307-328), the step between the classifier head and the mask head of MaskRCNN.predict(mode='inference')
(:1742-1781), once per image.

    from maskrcnn.detection_layer import detection_layer        # instead of the one in maskrcnn.model
    detections = detection_layer(config, rpn_rois, mrcnn_class, mrcnn_bbox, image_meta)

The reference takes an arg-max, decodes, scales, clips and rounds in about fifteen element-wise launches and then loops in Python over
the classes present, each pass with a nonzero, a sort, three gathers and an NMS whose CUDA path copies the pair mask to the host;
every nonzero and every NMS makes the host wait.  Here one kernel does the per-row work, one workgroup sorts the valid rows by score,
the pair mask of csrc/raster_boxes.hip's NMS takes the class test as well, and one wave scans it, stopped at DETECTION_MAX_INSTANCES:
csrc/detection_layer.hip behind sdn_hip.ops.detection_layer.  CPU tensors raise NotImplementedError and there is no torch form.  The
boxes are the reference's fp32 arithmetic operation by operation, expf being the only operation whose last bit may differ from a CPU
run; they are rounded to whole pixels, so the detections are the reference's unless a coordinate lies within that last bit of a half.
Equal scores are ordered lower row first (the reference's sorts leave that open).  No result carries a gradient.
"""
from sdn_hip import ops


def _config_values(config):
    if config is None:
        raise ValueError('config is needed: RPN_BBOX_STD_DEV, IMAGE_SHAPE, DETECTION_MIN_CONFIDENCE, DETECTION_NMS_THRESHOLD and '
                         'DETECTION_MAX_INSTANCES are read from it (model.py:772-827)')
    height, width = config.IMAGE_SHAPE[:2]
    return (config.RPN_BBOX_STD_DEV, height, width, config.DETECTION_MIN_CONFIDENCE, config.DETECTION_NMS_THRESHOLD,
            config.DETECTION_MAX_INSTANCES)


def detections_padded(rois, probs, deltas, window, config, roi_count=None, strict=True):
    """(detections fp32 [D, 6], boxes_norm fp32 [1, D, 4], count int32 [1]) with D = config.DETECTION_MAX_INSTANCES: the detections of
    refine_detections below in buffers of fixed size, rows behind count +0.0, with nothing crossing to the host -- the form for a
    caller that keeps the frame on the device.  detections is what detections.unmold_boxes takes (it ends at the first class id 0),
    boxes_norm what the mask head's pyramid_roi_align takes (:1769).  rois fp32 [N, 4] or [1, N, 4]; roi_count: the count of
    proposals_padded (int32 [1] on the device), so that its zero padding is never a detection, or None for all N rows."""
    if hasattr(rois, 'dim') and rois.dim() == 3:
        if rois.shape[0] != 1:
            raise ValueError('rois has batch %d; only 1 is supported, as in the reference ("Currently only supports batchsize 1", '
                             'geometric/maskrcnn/model.py:848)' % rois.shape[0])
        rois = rois[0]
    std_dev, height, width, min_confidence, nms_threshold, max_instances = _config_values(config)
    out = ops.detection_layer(rois, probs, deltas, window, std_dev, height, width, min_confidence, nms_threshold, max_instances,
                              roi_count=roi_count, strict=strict)
    _class_ids, _scores, _boxes_px, _keep, count, detections, boxes_norm = out
    return detections, boxes_norm.unsqueeze(0), count


def refine_detections(rois, probs, deltas, window, config):
    """The reference's refine_detections (model.py:744-837), name, signature and return value: rois fp32 [N, 4] normalised, probs fp32
    [N, C], deltas fp32 [N, C, 4], contiguous CUDA tensors; window four host numbers (y1, x1, y2, x2) in pixels.  Returns fp32 [n, 6] =
    (y1, x1, y2, x2, class_id, score) in pixels, n <= config.DETECTION_MAX_INSTANCES, best score first.

    The size of the result depends on the data, so the count is read once: the call's only host wait (detections_padded has none).
    Unlike the reference, which raises where no row is a detection, this returns [0, 6]; suppression is on IoU > threshold, the rule
    of the reference's CUDA kernel."""
    detections, _boxes_norm, count = detections_padded(rois, probs, deltas, window, config)
    return detections[:int(count.item())]


def detection_layer(config, rois, mrcnn_class, mrcnn_bbox, image_meta):
    """The reference's detection_layer (model.py:840-855): rois fp32 [1, N, 4], mrcnn_class fp32 [N, C], mrcnn_bbox fp32 [N, C, 4];
    image_meta a host array or CPU tensor [1, 8 + C] whose entries 4:8 are the window (parse_image_meta, :2172).  Returns
    refine_detections' [n, 6]."""
    if hasattr(image_meta, 'is_cuda') and image_meta.is_cuda:
        raise TypeError('image_meta must be a host array or a CPU tensor, as in the reference; it is on %s' % (image_meta.device,))
    if len(image_meta.shape) != 2 or image_meta.shape[0] != 1 or image_meta.shape[1] < 8:
        raise ValueError('image_meta must be [1, 8 + classes], got %s' % (tuple(image_meta.shape),))
    window = [float(v) for v in image_meta[0, 4:8]]
    if hasattr(rois, 'dim') and rois.dim() == 3 and rois.shape[0] == 1:
        rois = rois[0]           # :849, a view
    return refine_detections(rois, mrcnn_class, mrcnn_bbox, window, config)
