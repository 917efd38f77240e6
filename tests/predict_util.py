"""What the tests of maskrcnn.predict and sdn_hip.ops.rpn_outputs share.

  - rpn_tail: the torch expressions of the RPN's tail -- per level permute(0, 2, 3, 1).contiguous().view of the class map and of the
    box map and a softmax over the last axis, then a cat over the levels per output -- written from the layout that
    include/sdn_hip.h states for sdn_rpn_outputs_fwd; fp32 or fp64, any device.  index_loop is the same map as explicit loops.
  - StandIn: a seeded stand-in network with the reference's attribute names (fpn, rpn, classifier, mask, anchors, config) and small
    widths: FPN depth 8, heads 16 wide, a 128 x 128 image, strides 4 .. 64, anchors from maskrcnn.rpn_targets.generate_pyramid_anchors.
    It makes the decision layers do work: the FPN's level convs pass pooled image planes through (channel 0: the plane the level's
    RPN scores, channels 1 and 2: the planes the classifier reads), the RPN's class conv turns channel 0 into the fg logit, the
    classifier averages channels 1 and 2 over the RoI.  painted_frame paints three squares that are anchors; GT_BOXES are those
    anchors, so their proposals are positives, and the classifier finds classes 1, 2, 1 there.
  - cpu_chain: the stand-in on the CPU with the numpy restatements of the decision layers (tests/proposal_layer_util.py,
    tests/detection_targets_util.py, tests/detection_layer_util.py, tests/pyramid_roi_align_util.py), for the fixture's conditions.
"""
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import detection_layer_util as dlu
import detection_targets_util as dtu
import proposal_layer_util as plu
import pyramid_roi_align_util as pra
from maskrcnn.rpn_targets import generate_pyramid_anchors

f32 = np.float32
SIDE = 128
STRIDES = (4, 8, 16, 32, 64)
SCALES = (8, 16, 32, 64, 128)
RATIOS = (0.5, 1, 2)
DEPTH, WIDTH, CLASSES = 8, 16, 3
SHAPES = tuple((SIDE // s, SIDE // s) for s in STRIDES)
# three squares that are anchors (y1, x1, y2, x2) in pixels: level (stride, scale), centre = cell * stride, ratio 1
GT_BOXES = np.array([[32, 32, 64, 64],      # stride 16, scale 32, cell (3, 3), painted on plane 1, class 1
                     [88, 80, 104, 96],     # stride 8, scale 16, cell (12, 11), painted on plane 0, class 2
                     [80, 16, 112, 48]],    # stride 16, scale 32, cell (6, 2), painted on plane 1, class 1
                    f32)
GT_PLANES = (1, 0, 1)
GT_CLASS_IDS = np.array([1, 2, 1], np.int32)
RPN_PLANE = (2, 0, 1, 2, 2)                 # the image plane whose pooled value is channel 0 of each level: plane 2 holds no square


def config():
    return types.SimpleNamespace(
        IMAGE_SHAPE=np.array([SIDE, SIDE, 3]), IMAGE_MIN_DIM=SIDE, IMAGE_MAX_DIM=SIDE, IMAGE_PADDING=True, MEAN_PIXEL=np.zeros(3),
        NUM_CLASSES=CLASSES, GPU_COUNT=1, BACKBONE_STRIDES=list(STRIDES), RPN_ANCHOR_SCALES=SCALES, RPN_ANCHOR_RATIOS=list(RATIOS),
        RPN_ANCHOR_STRIDE=1, RPN_NMS_THRESHOLD=0.5, RPN_TRAIN_ANCHORS_PER_IMAGE=32, POST_NMS_ROIS_TRAINING=64, POST_NMS_ROIS_INFERENCE=32,
        RPN_BBOX_STD_DEV=np.array([0.1, 0.1, 0.2, 0.2]), BBOX_STD_DEV=np.array([0.1, 0.1, 0.2, 0.2]), TRAIN_ROIS_PER_IMAGE=16,
        ROI_POSITIVE_RATIO=0.33, USE_MINI_MASK=True, MINI_MASK_SHAPE=(14, 14), MASK_SHAPE=[28, 28], POOL_SIZE=7, MASK_POOL_SIZE=14,
        DETECTION_MIN_CONFIDENCE=0.6, DETECTION_NMS_THRESHOLD=0.3, DETECTION_MAX_INSTANCES=8)


# ---- the torch expressions of the RPN's tail -------------------------------------------------------------------------------------------
def rpn_tail(class_maps, bbox_maps):
    """[rpn_class_logits [B, A, 2], rpn_probs [B, A, 2], rpn_bbox [B, A, 4]] in the maps' dtype"""
    logits, probs, boxes = [], [], []
    for c, b in zip(class_maps, bbox_maps):
        x = c.permute(0, 2, 3, 1).contiguous().view(c.size(0), -1, 2)
        logits.append(x)
        probs.append(torch.softmax(x, dim=2))
        boxes.append(b.permute(0, 2, 3, 1).contiguous().view(b.size(0), -1, 4))
    return [torch.cat(logits, dim=1), torch.cat(probs, dim=1), torch.cat(boxes, dim=1)]


def index_loop(class_maps, bbox_maps):
    """the same three arrays by explicit loops over (level, image, y, x, anchor, component), numpy in, numpy out (no softmax: the
    second entry is None)"""
    B, k = class_maps[0].shape[0], class_maps[0].shape[1] // 2
    A = k * sum(m.shape[2] * m.shape[3] for m in class_maps)
    logits, boxes = np.zeros((B, A, 2), class_maps[0].dtype), np.zeros((B, A, 4), bbox_maps[0].dtype)
    start = 0
    for c, b in zip(class_maps, bbox_maps):
        H, W = c.shape[2:]
        for n in range(B):
            for y in range(H):
                for x in range(W):
                    for a in range(k):
                        row = start + (y * W + x) * k + a
                        for j in range(2):
                            logits[n, row, j] = c[n, a * 2 + j, y, x]
                        for j in range(4):
                            boxes[n, row, j] = b[n, a * 4 + j, y, x]
        start += k * H * W
    return logits, None, boxes


def draw_maps(levels, k, B, seed, device='cpu', dtype=torch.float32):
    """seeded class and box maps for the level list [(H, W), ...]"""
    g = torch.Generator().manual_seed(seed)
    cls = [(torch.randn(B, 2 * k, h, w, generator=g) * 3.0).to(device=device, dtype=dtype) for h, w in levels]
    box = [torch.randn(B, 4 * k, h, w, generator=g).to(device=device, dtype=dtype) for h, w in levels]
    return cls, box


# ---- the stand-in network --------------------------------------------------------------------------------------------------------------
class SamePad(nn.Module):
    """SamePad2d(kernel_size=3, stride=1) of the reference: one pixel of zeros all round"""

    def forward(self, x):
        return F.pad(x, (1, 1, 1, 1))


class FPN(nn.Module):
    """Level l: the image in byte units, averaged over stride x stride windows CENTRED on the level's anchor centres (cell * stride),
    then the level's own 1 x 1 conv to DEPTH channels."""

    def __init__(self, g):
        super(FPN, self).__init__()
        self.lateral = nn.ModuleList([nn.Conv2d(3, DEPTH, kernel_size=1) for _ in STRIDES])
        for l, conv in enumerate(self.lateral):
            w = torch.randn(DEPTH, 3, 1, 1, generator=g) * (0.02 / 255.0)
            w[0:3] = 0.0
            w[0, RPN_PLANE[l]] = 1.0 / 255.0           # channel 0: what the RPN scores at this level
            w[1, 1] = w[2, 0] = 1.0 / 255.0            # channels 1, 2: the planes of classes 1 and 2, at every level
            conv.weight.data.copy_(w)
            conv.bias.data.zero_()

    def forward(self, image):
        out = []
        for stride, conv in zip(STRIDES, self.lateral):
            half = stride // 2
            out.append(conv(F.avg_pool2d(F.pad(image, (half, stride - half, half, stride - half)), stride, stride)[:, :, :SIDE // stride,
                                                                                                                 :SIDE // stride]))
        return out


class RPN(nn.Module):
    def __init__(self, g):
        super(RPN, self).__init__()
        k = len(RATIOS)
        self.padding = SamePad()
        self.conv_shared = nn.Conv2d(DEPTH, WIDTH, kernel_size=3, stride=1)
        self.relu = nn.ReLU(inplace=True)
        self.conv_class = nn.Conv2d(WIDTH, 2 * k, kernel_size=1, stride=1)
        self.softmax = nn.Softmax(dim=2)
        self.conv_bbox = nn.Conv2d(WIDTH, 4 * k, kernel_size=1, stride=1)
        w = torch.randn(WIDTH, DEPTH, 3, 3, generator=g) * 0.02
        w[0] = 0.0
        w[0, 0, 1, 1] = 1.0                             # channel 0 passes the FPN's channel 0 on
        self.conv_shared.weight.data.copy_(w)
        self.conv_shared.bias.data.zero_()
        w = torch.randn(2 * k, WIDTH, 1, 1, generator=g) * 0.05
        b = torch.zeros(2 * k)
        for a, gain in enumerate((4.0, 6.0, 4.0)):      # fg - bg = 2 * (gain * paint - 3): the ratio-1 anchor of a painted cell leads
            w[2 * a, 0], w[2 * a + 1, 0] = -gain, gain
            b[2 * a], b[2 * a + 1] = 3.0, -3.0
        self.conv_class.weight.data.copy_(w)
        self.conv_class.bias.data.copy_(b)
        self.conv_bbox.weight.data.copy_(torch.randn(4 * k, WIDTH, 1, 1, generator=g) * 0.1)
        self.conv_bbox.bias.data.zero_()


class Classifier(nn.Module):
    def __init__(self, g, pool_size, image_shape):
        super(Classifier, self).__init__()
        self.depth, self.pool_size, self.image_shape, self.num_classes = DEPTH, pool_size, image_shape, CLASSES
        self.conv1 = nn.Conv2d(DEPTH, WIDTH, kernel_size=pool_size, stride=1)
        self.bn1 = nn.BatchNorm2d(WIDTH, eps=0.001, momentum=0.01)
        self.conv2 = nn.Conv2d(WIDTH, WIDTH, kernel_size=1, stride=1)
        self.bn2 = nn.BatchNorm2d(WIDTH, eps=0.001, momentum=0.01)
        self.relu = nn.ReLU(inplace=True)
        self.linear_class = nn.Linear(WIDTH, CLASSES)
        self.softmax = nn.Softmax(dim=1)
        self.linear_bbox = nn.Linear(WIDTH, CLASSES * 4)
        w = torch.randn(WIDTH, DEPTH, pool_size, pool_size, generator=g) * 0.01
        w[0:2] = 0.0
        w[0, 1] = w[1, 2] = 1.0 / (pool_size * pool_size)   # features 0, 1: the RoI's mean of the FPN's channels 1, 2
        self.conv1.weight.data.copy_(w)
        self.conv1.bias.data.zero_()
        w = torch.randn(WIDTH, WIDTH, 1, 1, generator=g) * 0.02
        w[0:2] = 0.0
        w[0, 0] = w[1, 1] = 1.0
        self.conv2.weight.data.copy_(w)
        self.conv2.bias.data.zero_()
        w = torch.randn(CLASSES, WIDTH, generator=g) * 0.05
        w[:, 0:2] = torch.tensor([[0.0, 0.0], [8.0, -4.0], [-4.0, 8.0]])
        self.linear_class.weight.data.copy_(w)
        self.linear_class.bias.data.copy_(torch.tensor([0.0, -2.0, -2.0]))
        self.linear_bbox.weight.data.copy_(torch.randn(CLASSES * 4, WIDTH, generator=g) * 0.1)
        self.linear_bbox.bias.data.zero_()


class Mask(nn.Module):
    def __init__(self, g, pool_size, image_shape):
        super(Mask, self).__init__()
        self.depth, self.pool_size, self.image_shape, self.num_classes = DEPTH, pool_size, image_shape, CLASSES
        self.padding = SamePad()
        self.conv1 = nn.Conv2d(DEPTH, WIDTH, kernel_size=3, stride=1)
        self.bn1 = nn.BatchNorm2d(WIDTH, eps=0.001)
        self.conv2 = nn.Conv2d(WIDTH, WIDTH, kernel_size=3, stride=1)
        self.bn2 = nn.BatchNorm2d(WIDTH, eps=0.001)
        self.conv3 = nn.Conv2d(WIDTH, WIDTH, kernel_size=3, stride=1)
        self.bn3 = nn.BatchNorm2d(WIDTH, eps=0.001)
        self.conv4 = nn.Conv2d(WIDTH, WIDTH, kernel_size=3, stride=1)
        self.bn4 = nn.BatchNorm2d(WIDTH, eps=0.001)
        self.deconv = nn.ConvTranspose2d(WIDTH, WIDTH, kernel_size=2, stride=2)
        self.conv5 = nn.Conv2d(WIDTH, CLASSES, kernel_size=1, stride=1)
        self.sigmoid = nn.Sigmoid()
        self.relu = nn.ReLU(inplace=True)
        for m in (self.conv1, self.conv2, self.conv3, self.conv4, self.deconv, self.conv5):
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=g) * 0.15)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)


class StandIn(nn.Module):
    """the reference's MaskRCNN as far as predict and detect read it"""

    def __init__(self, seed=7):
        super(StandIn, self).__init__()
        g = torch.Generator().manual_seed(seed)
        self.config = config()
        self.fpn = FPN(g)
        self.rpn = RPN(g)
        self.classifier = Classifier(g, self.config.POOL_SIZE, self.config.IMAGE_SHAPE)
        self.mask = Mask(g, self.config.MASK_POOL_SIZE, self.config.IMAGE_SHAPE)
        self.anchors = torch.from_numpy(anchors64().astype(f32))          # model.py:1480-1486: a plain attribute, not a buffer

    def to_device(self, device):
        self.to(device)
        self.anchors = self.anchors.to(device)
        return self


def anchors64():
    return generate_pyramid_anchors(SCALES, RATIOS, np.array(SHAPES), STRIDES, 1)


def painted_frame(shift=0, squares=(0, 1, 2)):
    """uint8 [SIDE, SIDE, 3]: a faint seeded texture with the chosen squares of GT_BOXES painted 255 on their planes, moved `shift`
    cells of their level to the right (shift 0: the squares are the anchors GT_BOXES)"""
    rs = np.random.RandomState(11)
    frame = rs.randint(0, 24, (SIDE, SIDE, 3)).astype(np.uint8)
    for n in squares:
        y1, x1, y2, x2 = GT_BOXES[n].astype(int)
        dx = shift * (16 if n != 1 else 8)
        frame[y1:y2, x1 + dx:x2 + dx, GT_PLANES[n]] = 255
    return frame


def molded(frame):
    """what mold_inputs makes of the frame under config(): no resize, no padding, MEAN_PIXEL 0 -- fp32 [1, 3, SIDE, SIDE]"""
    return torch.from_numpy(frame.astype(f32)).permute(2, 0, 1).unsqueeze(0).contiguous()


def image_metas():
    return np.array([[0, SIDE, SIDE, 3, 0, 0, SIDE, SIDE] + [0] * CLASSES])


def gt_masks():
    """mini-masks fp32 [G, 14, 14]: a disc in each box"""
    yy, xx = np.mgrid[0:14, 0:14]
    disc = (((yy - 6.5) ** 2 + (xx - 6.5) ** 2) <= 36.0).astype(f32)
    return np.stack([disc] * len(GT_BOXES))


def training_input(frame, device):
    return [molded(frame).to(device), image_metas(), torch.from_numpy(GT_CLASS_IDS[None]).to(device),
            torch.from_numpy(GT_BOXES[None]).to(device), torch.from_numpy(gt_masks()[None]).to(device)]


def sampling_keys(seed=5):
    n = config().POST_NMS_ROIS_TRAINING
    return torch.rand(2, n, generator=torch.Generator().manual_seed(seed))


# ---- the stand-in on the CPU, with the restatements of the decision layers -----------------------------------------------------------
def cpu_pyramid_roi_align(boxes, maps, pool):
    """pyramid_roi_align for the stand-in's image: the level formula of model.py:445-457 with the restatement's sampling"""
    b = boxes.astype(np.float64)
    with np.errstate(all='ignore'):
        v = 4.0 + np.log(np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / (224.0 / np.sqrt(float(SIDE * SIDE)))) / np.log(2.0)
    lv = pra.levels_of(v)
    out = np.zeros((len(boxes), maps[0].shape[0], pool * pool), f32)
    for r in range(len(boxes)):
        m = maps[lv[r] - 2]
        flat = m.reshape(m.shape[0], -1)
        inside, (tl, tr, bl, br), xl, yl = pra.sample_table(boxes[r], m.shape[1], m.shape[2], pool)
        top = flat[:, tl] + (flat[:, tr] - flat[:, tl]) * xl
        bottom = flat[:, bl] + (flat[:, br] - flat[:, bl]) * xl
        out[r] = np.where(inside, top + (bottom - top) * yl, f32(0))
    return out.reshape(len(boxes), -1, pool, pool)


def cpu_chain(model, frame, keys=None):
    """The stand-in on the CPU in eval mode: dict with the proposal case and its contract for both proposal counts, the detection
    case and its contract, and the sampling of the detection targets -- everything the fixture's conditions are stated on."""
    cfg = model.config
    model.eval()
    with torch.no_grad():
        maps = model.fpn(molded(frame))
        cls, box = [], []
        for p in maps:
            x = model.rpn.relu(model.rpn.conv_shared(model.rpn.padding(p)))
            cls.append(model.rpn.conv_class(x))
            box.append(model.rpn.conv_bbox(x))
        _logits, probs, deltas = rpn_tail(cls, box)
    anchors = anchors64().astype(f32)
    A = anchors.shape[0]
    out = {}
    for mode, P in (('training', cfg.POST_NMS_ROIS_TRAINING), ('inference', cfg.POST_NMS_ROIS_INFERENCE)):
        c = dict(probs=probs[0].numpy(), deltas=deltas[0].numpy(), anchors=anchors, std_dev=tuple(cfg.RPN_BBOX_STD_DEV), image=(SIDE, SIDE),
                 thr=cfg.RPN_NMS_THRESHOLD, K=min(6000, A), P=P)
        out[mode + '_proposals'] = (c, plu.contract(c))
    # inference: the classifier on the proposals, then the detection layer
    rois = out['inference_proposals'][1]['rois']
    n = len(rois)
    padded = np.zeros((cfg.POST_NMS_ROIS_INFERENCE, 4), f32)
    padded[:n] = rois
    with torch.no_grad():
        x = torch.from_numpy(cpu_pyramid_roi_align(padded, [m[0].numpy() for m in maps[:4]], cfg.POOL_SIZE))
        h = model.classifier
        x = h.relu(h.bn1(h.conv1(x)))
        x = h.relu(h.bn2(h.conv2(x))).view(-1, WIDTH)
        mrcnn_probs = h.softmax(h.linear_class(x)).numpy()
        mrcnn_bbox = h.linear_bbox(x).view(len(padded), -1, 4).numpy()
    d = dict(rois=padded, probs=mrcnn_probs, deltas=mrcnn_bbox, std_dev=tuple(cfg.RPN_BBOX_STD_DEV), image=(SIDE, SIDE),
             window=(0, 0, SIDE, SIDE), N=len(padded), C=CLASSES, roi_count=n, conf=cfg.DETECTION_MIN_CONFIDENCE,
             thr=cfg.DETECTION_NMS_THRESHOLD, D=cfg.DETECTION_MAX_INSTANCES)
    out['detections'] = (d, dlu.contract(d))
    # training: the sampling of the detection targets on the training proposals
    rois = out['training_proposals'][1]['rois']
    n = len(rois)
    padded = np.zeros((cfg.POST_NMS_ROIS_TRAINING, 4), f32)
    padded[:n] = rois
    keys = sampling_keys() if keys is None else keys
    t = dict(proposals=padded, gt_class_ids=GT_CLASS_IDS, gt_boxes=(GT_BOXES / f32(SIDE)).astype(f32), N=len(padded), G=len(GT_BOXES),
             roi_count=n, R=cfg.TRAIN_ROIS_PER_IMAGE, ratio=cfg.ROI_POSITIVE_RATIO, keys=keys.numpy())
    out['targets'] = (t, dtu.select(t))
    return out
