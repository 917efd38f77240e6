"""MaskRCNN.predict and MaskRCNN.detect on the device (reference: geometric/maskrcnn/model.py:1705-1821 and :1611-1654, with the tail
of RPN.forward, :896-911, and the forwards of the two heads, :938-954 and :978-997).

    from maskrcnn.predict import use_device_predict
    use_device_predict(model)                      # instance-level predict and detect; state_dict and module names unchanged
    detections, mrcnn_mask = model.predict([molded_images, image_metas], mode='inference')
    results = model.detect([frame_u8])

The reference's predict calls its own proposal_layer, detection_layer and detection_target_layer and, inside Classifier.forward and
Mask.forward, its pyramid_roi_align; each of them waits for the device several times, and the RPN's outputs are made by two permuted
copies and a softmax per level and three cats.  Here the chain is

    fpn -> rpn_forward (the caller's convs, then ONE rpn_outputs launch) -> proposals_padded
        inference: classifier_head -> detections_padded(roi_count=...) -> mask_head on boxes_norm
        training:  detection_targets_padded(roi_count=..., keys=...) -> classifier_head and mask_head on the padded rois

on one stream, with no side stream, and nothing crosses to the host: predict_padded returns buffers of fixed size with their counts
beside them, so it can be captured in a graph and replayed.  Rows behind a count are padding: detections of class id 0, training rows
of class id -1, which losses.mrcnn_losses leaves out -- the empty-tensor branch of :1803-1812 is not needed there while count > 0.  predict is
predict_padded, one read of the count and slices, the way proposal_layer is defined from proposals_padded, so it has no second
numerical path.  The backbone, the FPN and the heads' conv / BN / linear layers stay the caller's torch modules.

Still torch ops in the chain: the `gt_boxes / scale` division of :1794, the modules' own layers, and the views and slices.

Out of scope: fusing the two 1 x 1 convs of the RPN into the kernel; half precision; generate_inst_map(s) (:1656-1703);
train_epoch's optimizer loop (:1925-1990); the id selection of load_mask.  CPU tensors raise NotImplementedError and there is no
torch form.
"""
import types

import torch
from torch import nn

from sdn_hip import const_f32, ops

from .detection_layer import detections_padded
from .detection_targets import detection_targets_padded
from .detections import unmold_detections
from .proposals import proposals_padded
from .pyramid import pyramid_roi_align
from .training_item import mold_inputs


def rpn_outputs(class_maps, bbox_maps):
    """[rpn_class_logits fp32 [B, A, 2], rpn_probs fp32 [B, A, 2], rpn_bbox fp32 [B, A, 4]] from the outputs of conv_class and
    conv_bbox on every pyramid level: what RPN.forward returns (model.py:913) after the cat over the levels of :1739.  One launch
    forward, one backward (sdn_hip.ops.rpn_outputs)."""
    return list(ops.rpn_outputs(class_maps, bbox_maps))


def rpn_forward(rpn, feature_maps):
    """The loop over the pyramid levels of MaskRCNN.predict (model.py:1729-1740): the caller's rpn.padding, conv_shared, relu,
    conv_class and conv_bbox on each level (:891-894, :906), then one rpn_outputs call in place of the permutes, the softmaxes and
    the cats.  Returns [rpn_class_logits, rpn_probs, rpn_bbox]."""
    class_maps, bbox_maps = [], []
    for p in feature_maps:
        x = rpn.relu(rpn.conv_shared(rpn.padding(p)))
        class_maps.append(rpn.conv_class(x).contiguous())
        bbox_maps.append(rpn.conv_bbox(x).contiguous())
    return rpn_outputs(class_maps, bbox_maps)


def classifier_head(classifier, maps, rois):
    """Classifier.forward (model.py:938-954) on this library's pyramid_roi_align: the module's own conv1, bn1, relu, conv2, bn2, relu,
    linear_class, softmax and linear_bbox in the reference's order.  maps = [P2, P3, P4, P5], rois fp32 [1, N, 4] normalised.  Returns
    [mrcnn_class_logits [N, C], mrcnn_probs [N, C], mrcnn_bbox [N, C, 4]]."""
    x = pyramid_roi_align([rois] + list(maps), classifier.pool_size, classifier.image_shape)
    x = classifier.relu(classifier.bn1(classifier.conv1(x)))
    x = classifier.relu(classifier.bn2(classifier.conv2(x)))
    x = x.view(-1, classifier.linear_class.in_features)
    mrcnn_class_logits = classifier.linear_class(x)
    mrcnn_probs = classifier.softmax(mrcnn_class_logits)
    mrcnn_bbox = classifier.linear_bbox(x)
    mrcnn_bbox = mrcnn_bbox.view(mrcnn_bbox.size()[0], -1, 4)
    return [mrcnn_class_logits, mrcnn_probs, mrcnn_bbox]


def mask_head(mask, maps, rois):
    """Mask.forward (model.py:978-997) on this library's pyramid_roi_align: the module's own four padded convs with BN and ReLU, the
    deconv, relu, conv5 and the sigmoid.  Returns the mask probabilities fp32 [N, C, 2 * pool, 2 * pool]."""
    x = pyramid_roi_align([rois] + list(maps), mask.pool_size, mask.image_shape)
    x = mask.relu(mask.bn1(mask.conv1(mask.padding(x))))
    x = mask.relu(mask.bn2(mask.conv2(mask.padding(x))))
    x = mask.relu(mask.bn3(mask.conv3(mask.padding(x))))
    x = mask.relu(mask.bn4(mask.conv4(mask.padding(x))))
    x = mask.relu(mask.deconv(x))
    return mask.sigmoid(mask.conv5(x))


def _bn_eval(m):
    if m.__class__.__name__.find('BatchNorm') != -1:    # :1715-1718
        m.eval()


def _set_mode(model, mode):
    """:1709-1720: eval() in inference; train() with every BatchNorm in eval() in training"""
    if mode not in ('inference', 'training'):
        raise ValueError("mode must be 'inference' or 'training', got %r" % (mode,))
    modules = [model] if isinstance(model, nn.Module) else [getattr(model, n) for n in ('fpn', 'rpn', 'classifier', 'mask')]
    for m in modules:
        if mode == 'inference':
            m.eval()
        else:
            m.train()
            m.apply(_bn_eval)


def _one_image(molded_images, anchors):
    if not isinstance(molded_images, torch.Tensor):
        raise TypeError('molded_images must be a torch.Tensor, got %r' % (type(molded_images),))
    if molded_images.dim() != 4:
        raise ValueError('molded_images must be fp32 [1, 3, H, W], got %s' % (tuple(molded_images.shape),))
    if molded_images.shape[0] != 1:
        raise ValueError('molded_images has batch %d; only 1 is supported, as in the reference ("Currently only supports batchsize 1", '
                         'geometric/maskrcnn/model.py:358, :570, :848)' % molded_images.shape[0])
    if not molded_images.is_cuda:
        raise NotImplementedError('molded_images is on %s; predict only runs on the GPU' % (molded_images.device,))
    if not isinstance(anchors, torch.Tensor) or not anchors.is_cuda:
        raise NotImplementedError('model.anchors must be fp32 [A, 4] on the device; predict only runs on the GPU')


def predict_padded(model, input, mode, keys=None):
    """MaskRCNN.predict (model.py:1705-1821) in buffers of fixed size, with nothing crossing to the host.  model: anything with fpn,
    rpn, classifier, mask (the reference's modules), anchors (fp32 [A, 4] in pixels on the device) and config.  input: the
    reference's list -- [molded_images fp32 [1, 3, H, W], image_metas (host array or CPU tensor [1, 8 + classes])], and in training
    gt_class_ids [1, G], gt_boxes fp32 [1, G, 4] in pixels and gt_masks fp32 [1, G, mh, mw] behind them.

    mode='inference' returns (detections fp32 [D, 6] = (y1, x1, y2, x2, class_id, score) in pixels, mrcnn_mask fp32 [D, C, 2p, 2p],
    count int32 [1]) with D = config.DETECTION_MAX_INSTANCES; rows of detections behind count are +0.0, and their masks are those of
    the all-zero box.
    mode='training' returns (rpn_class_logits [1, A, 2], rpn_bbox [1, A, 4], target_class_ids int32 [R], mrcnn_class_logits [R, C],
    target_deltas [R, 4], mrcnn_bbox [R, C, 4], target_mask [R, h, w], mrcnn_mask [R, C, h, w], count int32 [1], n_pos int32 [1])
    with R = config.TRAIN_ROIS_PER_IMAGE: the reference's eight tensors in padded form, rows behind count with class id -1, which
    losses.mrcnn_losses leaves out.  With count 0 (no positive proposal) every row is padding and mrcnn_losses gives the head losses
    as torch's mean of nothing, NaN: a caller of the padded form guards the step with count on the device; predict returns the
    reference's empty tensors there, for which the head losses are 0.  keys: the sampling keys of detection_targets_padded (fp32 [2, POST_NMS_ROIS_TRAINING]) or None
    to draw them on the device.

    The BatchNorm-in-eval rule of :1714-1720 is kept.  One stream; the window is read from image_metas on the host, which is where
    it lives.  A batch other than 1 raises ValueError, a CPU model or image NotImplementedError."""
    molded_images, image_metas = input[0], input[1]
    config = model.config
    _one_image(molded_images, model.anchors)
    _set_mode(model, mode)
    p2, p3, p4, p5, p6 = model.fpn(molded_images)
    mrcnn_feature_maps = [p2, p3, p4, p5]                                        # P6 is used in the RPN only (:1725)
    rpn_class_logits, rpn_class, rpn_bbox = rpn_forward(model.rpn, [p2, p3, p4, p5, p6])
    proposal_count = config.POST_NMS_ROIS_TRAINING if mode == 'training' else config.POST_NMS_ROIS_INFERENCE
    rpn_rois, roi_count = proposals_padded([rpn_class, rpn_bbox], proposal_count, config.RPN_NMS_THRESHOLD, model.anchors, config)
    if mode == 'inference':
        if len(image_metas.shape) != 2 or image_metas.shape[0] != 1 or image_metas.shape[1] < 8:
            raise ValueError('image_metas must be [1, 8 + classes], got %s' % (tuple(image_metas.shape),))
        window = [float(v) for v in image_metas[0, 4:8]]                         # parse_image_meta, :2172
        _logits, mrcnn_class, mrcnn_bbox = classifier_head(model.classifier, mrcnn_feature_maps, rpn_rois)
        detections, boxes_norm, count = detections_padded(rpn_rois, mrcnn_class.detach(), mrcnn_bbox.detach(), window, config,
                                                          roi_count=roi_count)
        mrcnn_mask = mask_head(model.mask, mrcnn_feature_maps, boxes_norm)
        return detections, mrcnn_mask, count
    gt_class_ids, gt_boxes, gt_masks = input[2], input[3], input[4]
    h, w = config.IMAGE_SHAPE[:2]
    gt_boxes = gt_boxes / const_f32([h, w, h, w], gt_boxes.device)               # :1790-1794, still a torch op
    rois, target_class_ids, target_deltas, target_mask, count, n_pos = detection_targets_padded(
        rpn_rois, gt_class_ids, gt_boxes, gt_masks, config, keys=keys, roi_count=roi_count)
    mrcnn_class_logits, _probs, mrcnn_bbox = classifier_head(model.classifier, mrcnn_feature_maps, rois)
    mrcnn_mask = mask_head(model.mask, mrcnn_feature_maps, rois)
    return (rpn_class_logits, rpn_bbox, target_class_ids, mrcnn_class_logits, target_deltas, mrcnn_bbox, target_mask, mrcnn_mask,
            count, n_pos)


def predict(model, input, mode, keys=None):
    """The reference's MaskRCNN.predict (model.py:1705-1821), return values and shapes: in inference [detections fp32 [1, n, 6],
    mrcnn_mask fp32 [1, n, C, 2p, 2p]]; in training the list [rpn_class_logits, rpn_bbox, target_class_ids, mrcnn_class_logits,
    target_deltas, mrcnn_bbox, target_mask, mrcnn_mask] with n rows in the last six.  It is predict_padded, one read of the count (the
    call's only host wait) and slices.  With no RoI sampled in training the last six are the reference's empty tensors (:1803-1812),
    which losses.mrcnn_losses takes as R = 0; with no detection in inference, where the reference raises, n = 0."""
    out = predict_padded(model, input, mode, keys=keys)
    if mode == 'inference':
        detections, mrcnn_mask, count = out
        n = int(count.item())
        return [detections[:n].unsqueeze(0), mrcnn_mask[:n].unsqueeze(0)]
    n = int(out[8].item())
    if n == 0:
        dev = out[0].device
        empty = lambda dtype: torch.empty(0, dtype=dtype, device=dev)   # noqa: E731
        return [out[0], out[1], empty(torch.int32), empty(torch.float32), empty(torch.float32), empty(torch.float32),
                empty(torch.float32), empty(torch.float32)]
    return [out[0], out[1]] + [t[:n] for t in out[2:8]]


def detect(model, frames_u8):
    """The reference's MaskRCNN.detect (model.py:1611-1654) for a list of uint8 [H, W, 3] frames on the device: mold_inputs, then per
    image predict_padded(mode='inference') and unmold_detections (one image per call to predict, as the reference's own callers
    do).  Returns the reference's list of dicts -- rois int32 [N, 4], class_ids int32 [N], scores [N] as numpy arrays -- with masks
    fp32 [N, 1, H, W] left on the device.  The detections' [D, 6] table is the one thing copied to the host, by unmold_detections."""
    frames = list(frames_u8)
    molded_images, image_metas, windows = mold_inputs(frames, model.config)
    results = []
    for i, frame in enumerate(frames):
        with torch.no_grad():                                                    # volatile=True, :1631
            detections, mrcnn_mask, _count = predict_padded(model, [molded_images[i:i + 1], image_metas[i:i + 1]], 'inference')
        rois, class_ids, scores, masks = unmold_detections(detections, mrcnn_mask, tuple(frame.shape), windows[i])
        results.append({'rois': rois, 'class_ids': class_ids, 'scores': scores, 'masks': masks})
    return results


class PredictHandle(object):
    """what use_device_predict returns: .remove() gives the model its class's predict and detect back"""

    def __init__(self, model):
        self.model = model

    def remove(self):
        for name in ('predict', 'detect'):
            self.model.__dict__.pop(name, None)


def use_device_predict(model):
    """Gives `model` (a MaskRCNN, or any nn.Module with its attributes fpn, rpn, classifier, mask, anchors and config) instance-level
    predict(input, mode) and detect(frames_u8) that run the chain above, in the manner of semantic.ppm.use_device_ppm: the same
    parameters, buffers, module names and state_dict.  Returns a PredictHandle."""
    if not isinstance(model, nn.Module):
        raise TypeError('model must be an nn.Module, got %r' % (type(model),))
    for name in ('fpn', 'rpn', 'classifier', 'mask', 'anchors', 'config'):
        if not hasattr(model, name):
            raise ValueError('%s has no attribute %s' % (type(model).__name__, name))
    if 'predict' in model.__dict__ or 'detect' in model.__dict__:
        raise ValueError('this model already has an instance-level predict or detect')
    if not isinstance(model.anchors, torch.Tensor) or not model.anchors.is_cuda:
        raise NotImplementedError('model.anchors must be on the device; predict only runs on the GPU')
    # nn.Module.__setattr__ files Modules, Parameters and buffers only: a bound function goes to the instance's __dict__
    model.predict = types.MethodType(lambda self, input, mode, keys=None: predict(self, input, mode, keys=keys), model)
    model.detect = types.MethodType(lambda self, frames_u8: detect(self, frames_u8), model)
    return PredictHandle(model)
