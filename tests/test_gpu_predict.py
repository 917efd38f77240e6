"""maskrcnn.predict on the GPU behind the stand-in network of tests/predict_util.py: predict_padded in both modes against the same
chain written out here from the public pieces, predict against its slices, the fixture's conditions on the device, the losses and
their backward through the whole chain, the case without a positive, detect against its three steps done by hand, the installer, and
a whole inference captured in a graph and replayed on a second image -- the test that nothing in the chain waits for the host."""
import numpy as np
import pytest
import torch

import predict_util as u
from maskrcnn import predict as pr          # the feature itself: without it this module does not import
from maskrcnn.detection_layer import detections_padded
from maskrcnn.detection_targets import detection_targets_padded
from maskrcnn.detections import unmold_detections
from maskrcnn.losses import mrcnn_losses
from maskrcnn.proposals import proposals_padded
from maskrcnn.pyramid import pyramid_roi_align
from maskrcnn.rpn_targets import rpn_targets_padded
from maskrcnn.training_item import mold_inputs
from sdn_hip.ops import rpn_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

DEV = 'cuda:0'


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.fixture(scope='module')
def model():
    return u.StandIn().to_device(DEV)


@pytest.fixture(scope='module')
def frame():
    return u.painted_frame()


def rpn_by_hand(model, maps):
    cls, box = [], []
    for p in maps:
        x = model.rpn.relu(model.rpn.conv_shared(model.rpn.padding(p)))
        cls.append(model.rpn.conv_class(x))
        box.append(model.rpn.conv_bbox(x))
    return rpn_outputs(cls, box)


def classifier_by_hand(h, maps, rois):
    x = pyramid_roi_align([rois] + maps, h.pool_size, h.image_shape)
    x = h.relu(h.bn1(h.conv1(x)))
    x = h.relu(h.bn2(h.conv2(x))).view(-1, u.WIDTH)
    logits = h.linear_class(x)
    return logits, h.softmax(logits), h.linear_bbox(x).view(x.shape[0], -1, 4)


def mask_by_hand(h, maps, rois):
    x = pyramid_roi_align([rois] + maps, h.pool_size, h.image_shape)
    for conv, bn in ((h.conv1, h.bn1), (h.conv2, h.bn2), (h.conv3, h.bn3), (h.conv4, h.bn4)):
        x = h.relu(bn(conv(h.padding(x))))
    return h.sigmoid(h.conv5(h.relu(h.deconv(x))))


def inference_by_hand(model, image):
    cfg = model.config
    model.eval()
    maps = model.fpn(image)
    _logits, probs, deltas = rpn_by_hand(model, maps)
    rois, roi_count = proposals_padded([probs, deltas], cfg.POST_NMS_ROIS_INFERENCE, cfg.RPN_NMS_THRESHOLD, model.anchors, cfg)
    _l, mrcnn_class, mrcnn_bbox = classifier_by_hand(model.classifier, maps[:4], rois)
    detections, boxes_norm, count = detections_padded(rois, mrcnn_class.detach(), mrcnn_bbox.detach(), (0, 0, u.SIDE, u.SIDE), cfg,
                                                      roi_count=roi_count)
    return detections, mask_by_hand(model.mask, maps[:4], boxes_norm), count


def training_by_hand(model, inp, keys):
    cfg = model.config
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    maps = model.fpn(inp[0])
    logits, probs, deltas = rpn_by_hand(model, maps)
    rois, roi_count = proposals_padded([probs, deltas], cfg.POST_NMS_ROIS_TRAINING, cfg.RPN_NMS_THRESHOLD, model.anchors, cfg)
    gt_boxes = inp[3] / torch.tensor([u.SIDE, u.SIDE, u.SIDE, u.SIDE], dtype=torch.float32, device=DEV)
    rois, ids, target_deltas, target_mask, count, n_pos = detection_targets_padded(rois, inp[2], gt_boxes, inp[4], cfg, keys=keys,
                                                                                   roi_count=roi_count)
    mrcnn_logits, _p, mrcnn_bbox = classifier_by_hand(model.classifier, maps[:4], rois)
    return (logits, deltas, ids, mrcnn_logits, target_deltas, mrcnn_bbox, target_mask, mask_by_hand(model.mask, maps[:4], rois), count, n_pos)


def test_inference_is_the_chain_of_the_public_pieces_and_meets_the_fixtures_conditions(model, frame):
    image = u.molded(frame).to(DEV)
    with torch.no_grad():
        got = pr.predict_padded(model, [image, u.image_metas()], 'inference')
        want = inference_by_hand(model, image)
    cfg = model.config
    D, p = cfg.DETECTION_MAX_INSTANCES, cfg.MASK_POOL_SIZE
    assert got[0].shape == (D, 6) and got[1].shape == (D, u.CLASSES, 2 * p, 2 * p) and got[2].shape == (1,) and got[2].dtype == torch.int32
    for a, b in zip(got, want):
        assert bits(a) == bits(b)
    assert not model.training
    n = int(got[2])
    det = got[0].cpu().numpy()
    print('detections on the device: %d' % n, det[:n].tolist())
    assert n >= 2 and (det[:n, 5] >= np.float32(cfg.DETECTION_MIN_CONFIDENCE)).all() and (det[n:] == 0).all()
    assert set(det[:n, 4].astype(int).tolist()) == {1, 2}
    for box in u.GT_BOXES:                                                  # each painted square is detected
        assert np.abs(det[:n, :4] - box).max(axis=1).min() <= 2.0
    assert torch.isfinite(got[1]).all() and float(got[1].min()) >= 0.0 and float(got[1].max()) <= 1.0
    # predict: one read of the count and slices, in the reference's shapes
    with torch.no_grad():
        detections, mrcnn_mask = pr.predict(model, [image, u.image_metas()], 'inference')
    assert detections.shape == (1, n, 6) and mrcnn_mask.shape == (1, n, u.CLASSES, 2 * p, 2 * p)
    assert bits(detections[0]) == bits(got[0][:n]) and bits(mrcnn_mask[0]) == bits(got[1][:n])


def test_training_is_the_chain_of_the_public_pieces_and_meets_the_fixtures_conditions(model, frame):
    inp, keys = u.training_input(frame, DEV), u.sampling_keys().to(DEV)
    got = pr.predict_padded(model, inp, 'training', keys=keys)
    assert model.training and not model.classifier.bn1.training and not model.mask.bn4.training       # model.py:1714-1720
    want = training_by_hand(model, inp, keys)
    cfg = model.config
    R, A = cfg.TRAIN_ROIS_PER_IMAGE, model.anchors.shape[0]
    shapes = [(1, A, 2), (1, A, 4), (R,), (R, u.CLASSES), (R, 4), (R, u.CLASSES, 4), (R, 28, 28), (R, u.CLASSES, 28, 28), (1,), (1,)]
    assert len(got) == 10 and [tuple(t.shape) for t in got] == shapes
    for a, b in zip(got, want):
        assert bits(a) == bits(b)
    count, n_pos = int(got[8]), int(got[9])
    print('training rows on the device: count %d, n_pos %d' % (count, n_pos))
    assert n_pos >= 2 and n_pos < count < R
    ids = got[2].cpu().numpy()
    assert (ids[:n_pos] > 0).all() and (ids[n_pos:count] == 0).all() and (ids[count:] == -1).all()
    assert set(ids[:n_pos].tolist()) == {1, 2}
    out = pr.predict(model, inp, 'training', keys=keys)
    assert len(out) == 8 and bits(out[0]) == bits(got[0]) and bits(out[1]) == bits(got[1])
    for a, b in zip(out[2:], got[2:8]):
        assert a.shape[0] == count and bits(a) == bits(b[:count])


def test_the_losses_are_finite_and_their_backward_reaches_every_module(model, frame):
    inp, keys = u.training_input(frame, DEV), u.sampling_keys().to(DEV)
    cfg = model.config
    anchors = torch.from_numpy(u.anchors64()).to(DEV)
    rpn_keys = torch.rand(2, anchors.shape[0], generator=torch.Generator().manual_seed(9)).to(DEV)
    rpn_match, rpn_bbox, _rows, counts = rpn_targets_padded(anchors, inp[2][0], inp[3][0], cfg, keys=rpn_keys)
    model.zero_grad()
    out = pr.predict_padded(model, inp, 'training', keys=keys)
    res = mrcnn_losses(rpn_match, rpn_bbox, out[0], out[1], *out[2:8])
    values = {k: float(res[k].detach()) for k in ('rpn_class_loss', 'rpn_bbox_loss', 'mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss', 'loss')}
    print(values, counts.tolist(), int(res['n_roi_pos']), int(res['bad']))
    assert all(np.isfinite(v) and v > 0 for v in values.values()) and int(res['n_roi_pos']) == int(out[9])
    assert int(res['bad']) == cfg.TRAIN_ROIS_PER_IMAGE - int(out[8])            # the rows behind the count, class id -1, and nothing else
    res['loss'].backward()
    for name in ('fpn', 'rpn', 'classifier', 'mask'):
        params = list(getattr(model, name).named_parameters())
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for _n, p in params), name
        nonzero = [n for n, p in params if float(p.grad.abs().sum()) > 0]
        print(name, '%d of %d parameters with a non-zero gradient' % (len(nonzero), len(params)))
        assert nonzero, name
        if name != 'fpn':                       # every layer of the RPN and of both heads; of the FPN the levels that hold sampled anchors
            assert len(nonzero) == len(params), (name, sorted(set(n for n, _p in params) - set(nonzero)))
    model.zero_grad()


def test_training_without_a_positive(model, frame):
    inp, keys = u.training_input(frame, DEV), u.sampling_keys().to(DEV)
    inp[2] = torch.tensor([[1]], dtype=torch.int32, device=DEV)
    inp[3] = torch.tensor([[[1.0, 1.0, 3.0, 3.0]]], device=DEV)           # 2 x 2 pixels: below IoU 0.5 with every anchor (64 pixels at least)
    inp[4] = inp[4][:, :1].contiguous()
    cfg = model.config
    anchors = torch.from_numpy(u.anchors64()).to(DEV)
    rpn_keys = torch.rand(2, anchors.shape[0], generator=torch.Generator().manual_seed(9)).to(DEV)
    rpn_match, rpn_bbox, _rows, _counts = rpn_targets_padded(anchors, inp[2][0], inp[3][0], cfg, keys=rpn_keys)
    padded = pr.predict_padded(model, inp, 'training', keys=keys)
    assert int(padded[8]) == 0 and int(padded[9]) == 0 and (padded[2] == -1).all()
    # R padded rows, none of them a RoI: mrcnn_losses takes torch's mean over an empty selection, NaN (its docstring); the caller of the
    # padded form guards the step with the count on the device.  predict's empty tensors are R = 0, for which the head losses are 0.
    res = mrcnn_losses(rpn_match, rpn_bbox, padded[0], padded[1], *padded[2:8])
    heads = [float(res[k].detach()) for k in ('mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss')]
    print('padded head losses without a RoI:', heads, 'left out:', int(res['bad']))
    assert all(np.isnan(v) for v in heads) and int(res['bad']) == cfg.TRAIN_ROIS_PER_IMAGE and int(res['n_roi_pos']) == 0
    out = pr.predict(model, inp, 'training', keys=keys)
    assert len(out) == 8 and bits(out[0]) == bits(padded[0]) and bits(out[1]) == bits(padded[1])
    assert [tuple(t.shape) for t in out[2:]] == [(0,)] * 6 and out[2].dtype == torch.int32 and all(t.is_cuda for t in out[2:])   # :1803-1812
    res = mrcnn_losses(rpn_match, rpn_bbox, *out)
    assert all(float(res[k].detach()) == 0.0 for k in ('mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss'))
    assert np.isfinite(float(res['rpn_class_loss'].detach())) and np.isfinite(float(res['loss'].detach()))


def test_detect_is_mold_predict_unmold_and_the_installer_keeps_the_state_dict(frame):
    model = u.StandIn().to_device(DEV)
    keys = list(model.state_dict().keys())
    names = [n for n, _m in model.named_modules()]
    handle = pr.use_device_predict(model)
    assert list(model.state_dict().keys()) == keys and [n for n, _m in model.named_modules()] == names
    with pytest.raises(ValueError, match='already has an instance-level predict'):
        pr.use_device_predict(model)
    frame_u8 = torch.from_numpy(frame).to(DEV)
    results = model.detect([frame_u8])
    molded_images, metas, windows = mold_inputs([frame_u8], model.config)
    assert bits(molded_images) == bits(u.molded(frame)) and metas.shape == (1, 8 + u.CLASSES) and tuple(windows[0]) == (0, 0, u.SIDE, u.SIDE)
    with torch.no_grad():
        detections, mrcnn_mask, count = pr.predict_padded(model, [molded_images, metas], 'inference')
    rois, class_ids, scores, masks = unmold_detections(detections, mrcnn_mask, frame.shape, windows[0])
    assert len(results) == 1 and sorted(results[0]) == ['class_ids', 'masks', 'rois', 'scores']
    r = results[0]
    assert len(r['rois']) == len(rois) >= 2 and int(count) >= len(rois) and r['rois'].dtype == np.int32 and r['masks'].is_cuda and r['masks'].shape == (len(rois), 1, u.SIDE, u.SIDE)
    assert np.array_equal(r['rois'], rois) and np.array_equal(r['class_ids'], class_ids) and np.array_equal(r['scores'], scores)
    assert bits(r['masks']) == bits(masks)
    # the installed predict is predict
    with torch.no_grad():
        a = model.predict([molded_images, metas], 'inference')
        b = pr.predict(model, [molded_images, metas], 'inference')
    assert all(bits(x) == bits(y) for x, y in zip(a, b))
    handle.remove()
    assert 'predict' not in model.__dict__ and 'detect' not in model.__dict__


def test_a_whole_inference_is_captured_in_a_graph_and_replayed_on_a_second_image(model, frame):
    """three warm-up calls, one capture on one stream, a replay on new image contents: nothing in predict_padded waits for the host"""
    second = u.painted_frame(shift=1)
    static = u.molded(frame).to(DEV)
    metas = u.image_metas()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            pr.predict_padded(model, [static, metas], 'inference')
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = pr.predict_padded(model, [static, metas], 'inference')
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        first = pr.predict_padded(model, [static, metas], 'inference')
    assert all(bits(a) == bits(b) for a, b in zip(out, first))
    static.copy_(u.molded(second).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    with torch.no_grad():
        eager = pr.predict_padded(model, [static, metas], 'inference')
    assert all(bits(a) == bits(b) for a, b in zip(replayed, eager))
    assert int(eager[2]) >= 2 and bits(eager[0]) != bits(first[0])           # the second image has its own detections
