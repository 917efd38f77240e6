"""From the segmentation decoder's class scores to the label map of the textural branch and to IoU / accuracy, on the device
(reference: semantic/vkitti_test.py:56-73, vkitti_eval.py:64-107, models.py:401-402, utils.py:5-38, 101-129,
vkitti_dataset.py:206-209, 238).

    labels = fuse_predictions(scores, (H, W))          # uint8 [B, 1, H, W]: labels[b] is EditSession's base_segm_u8
    gt, unknown = labels_from_colors(scene_u8, codes, labels)
    ev = SegmEvaluator(14); ev.update(labels, gt); ev.summary()

The kernels are csrc/segm_tail.hip behind sdn_hip.ops; CPU tensors raise NotImplementedError and there is no torch form.
"""
import numpy as np
import torch

from sdn_hip import ops


def fuse_predictions(scores, seg_size, return_probs=False):
    """scores: a list of S (1 to 8) CUDA fp32 [B, C, h_s, w_s] tensors, the decoder's class scores of each test scale before
    upsample and softmax; seg_size (H, W).  Returns the label map uint8 [B, 1, H, W] = arg-max over the classes of the mean
    over the scales of softmax(upsample(scores_s, seg_size, 'bilinear')) -- vkitti_test.py:58-72 without a full-resolution
    tensor or a copy to the host -- and with return_probs also that mean, fp32 [B, C, H, W]."""
    H, W = seg_size
    return ops.segm_fuse(list(scores), int(H), int(W), probs=bool(return_probs))


def color_table(codes, labels):
    """The sorted table of labels_from_colors: codes [K, 3] uint8 colours (r, g, b as the scene image stores them), labels [K]
    (0 .. 255; 0 is unlabelled and becomes -1).  Returns numpy int32 [2 K]: the codes r | g << 8 | b << 16 ascending, then
    their labels.  A colour listed twice must carry one label."""
    codes = np.asarray(codes)
    labels = np.asarray(labels)
    if codes.ndim != 2 or codes.shape[1] != 3 or codes.shape[0] < 1 or labels.shape != (codes.shape[0],):
        raise ValueError('codes must be [K, 3] and labels [K] with K >= 1, got %s, %s' % (codes.shape, labels.shape))
    if codes.min() < 0 or codes.max() > 255 or labels.min() < 0 or labels.max() > 255:
        raise ValueError('colour components and labels must lie in 0 .. 255')
    packed = codes[:, 0].astype(np.int64) | (codes[:, 1].astype(np.int64) << 8) | (codes[:, 2].astype(np.int64) << 16)
    order = np.argsort(packed, kind='stable')
    packed, lab = packed[order], labels.astype(np.int64)[order]
    same = packed[1:] == packed[:-1]
    if np.any(same & (lab[1:] != lab[:-1])):
        raise ValueError('a colour is listed with two labels')
    keep = np.concatenate(([True], ~same))
    packed, lab = packed[keep], lab[keep]
    if packed.size > ops.SEGM_MAX_COLORS:
        raise ValueError('%d distinct colours; at most %d are supported' % (packed.size, ops.SEGM_MAX_COLORS))
    return np.concatenate((packed, lab)).astype(np.int32)


_tables = {}


def _device_table(table_host, device):
    # a scene's table does not change between frames: uploaded once
    key = (table_host.tobytes(), str(device))
    t = _tables.get(key)
    if t is None:
        if len(_tables) > 64:
            _tables.clear()
        t = _tables[key] = torch.from_numpy(table_host).to(device)
    return t


def labels_from_colors(scene_u8, codes, labels):
    """The ground-truth label map of vkitti_dataset.py:206-209, 238: scene_u8 uint8 [B, H, W, 3] (or [H, W, 3]) CUDA, the
    semantic colour image; codes [K, 3] and labels [K] on the host, the (r, g, b) -> label rows of the scene's table.  Returns
    (labels_gt int16 [B, H, W] = label - 1, unknown int32 [B]).  A colour outside the table gets -32768 and is counted in
    `unknown` instead of the reference's KeyError, which SegmEvaluator.summary raises."""
    if isinstance(scene_u8, torch.Tensor) and scene_u8.dim() == 3:
        scene_u8 = scene_u8[None]
    table_host = color_table(codes, labels)
    if not isinstance(scene_u8, torch.Tensor):
        raise TypeError('scene_u8 must be a torch.Tensor, got %r' % (type(scene_u8),))
    if not scene_u8.is_cuda:
        raise NotImplementedError('scene_u8 is on %s; the semantic tail only runs on the GPU' % (scene_u8.device,))
    table = _device_table(table_host, scene_u8.device)
    return ops.segm_labels_from_colors(scene_u8, table_host, table)


def summarize(counts, num_class):
    """The evaluation's numbers from the per-frame integer rows (numpy int64 [F, 3 C + 3]), in float64, operation for operation
    as vkitti_eval.py:83-107 with utils.py's AverageMeter: per frame acc = acc_sum / (valid_sum + 1e-10), the running sum
    acc * valid_sum over the running valid_sum; iou = sum of intersections / (sum of unions + 1e-10).  Returns a dict with
    iou [C], mean_iou, accuracy, acc_per_frame [F]."""
    counts = np.asarray(counts, dtype=np.int64)
    C = int(num_class)
    if counts.ndim != 2 or counts.shape[1] != 3 * C + 3 or counts.shape[0] < 1:
        raise ValueError('counts must be int64 [F, %d] with F >= 1, got %s' % (3 * C + 3, counts.shape))
    bad = np.nonzero(counts[:, 3 * C + 2])[0]
    if bad.size:
        raise KeyError('frame %d holds %d pixels whose colour is not in the table' % (int(bad[0]), int(counts[bad[0], 3 * C + 2])))
    inter = counts[:, :C]
    union = counts[:, C:2 * C] + counts[:, 2 * C:3 * C] - inter
    accs, total, count, avg = [], None, None, None
    for f in range(counts.shape[0]):
        acc_sum, valid_sum = counts[f, 3 * C], counts[f, 3 * C + 1]
        acc = float(acc_sum) / (valid_sum + 1e-10)   # utils.py:105
        accs.append(acc)
        if total is None:                             # AverageMeter.initialize
            avg, total, count = acc, acc * valid_sum, valid_sum
        else:                                         # AverageMeter.add
            total = total + acc * valid_sum
            count = count + valid_sum
            avg = total / count
    iou = inter.sum(axis=0) / (union.sum(axis=0) + 1e-10)
    return {'iou': iou, 'mean_iou': iou.mean(), 'accuracy': avg, 'acc_per_frame': np.asarray(accs, dtype=np.float64)}


class SegmEvaluator:
    """accuracy() and intersectionAndUnion() over any number of frames with one copy to the host at the end.  update() only
    launches: every call's integer rows stay on the device; summary() fetches them once."""

    def __init__(self, num_class):
        self.num_class = int(num_class)
        self._rows = []   # int64 [B, 3 C + 3] per update, on the device

    def update(self, labels, labels_gt):
        """labels uint8 [B, 1, H, W], labels_gt int16 [B, H, W], both CUDA."""
        self._rows.append(ops.segm_confusion(labels, labels_gt, self.num_class))

    def counts(self):
        """The rows of every frame so far, numpy int64 [F, 3 C + 3] (the one device-to-host copy)."""
        if not self._rows:
            raise ValueError('no frame has been evaluated')
        return torch.cat(self._rows, 0).cpu().numpy()

    def summary(self):
        """{'iou': [C], 'mean_iou', 'accuracy', 'acc_per_frame'} in float64; KeyError if a frame held an unknown colour."""
        return summarize(self.counts(), self.num_class)


def _decoder_of(segmentation_module):
    dec = getattr(segmentation_module, 'decoder', None)
    if dec is None or not hasattr(dec, 'conv_last'):
        raise ValueError('segmentation_module.decoder.conv_last not found: predict() reads the class scores there')
    return dec


def predict(segmentation_module, img_resized_list, seg_size, return_probs=False):
    """The loop of vkitti_test.py:56-73 around the caller's SegmentationModule (semantic/models.py): one forward pass per
    scale, then fuse_predictions.

    The fusion needs the class scores BEFORE upsample and softmax.  The module does not return them: built with
    use_softmax=True it returns the full-resolution softmax (the 26 MB tensor this path avoids), built with use_softmax=False
    it returns log_softmax at 1/8 resolution, which differs from the scores by a constant PER PIXEL -- and the reference
    interpolates first, so that constant does not cancel in the later softmax.  The scores are therefore taken from
    decoder.conv_last with a forward hook (all four decoders of models.py end in a layer of that name), and the module's own
    return value is dropped; build the decoder with use_softmax=False so that the dropped tail is the small one."""
    dec = _decoder_of(segmentation_module)
    scores, grabbed = [], []
    hook = dec.conv_last.register_forward_hook(lambda mod, inp, out: grabbed.append(out))
    try:
        with torch.no_grad():
            for img in img_resized_list:
                del grabbed[:]
                segmentation_module({'img_data': img}, segSize=tuple(seg_size))
                if len(grabbed) != 1:
                    raise RuntimeError('decoder.conv_last ran %d times in one forward pass' % len(grabbed))
                scores.append(grabbed[0].detach().float().contiguous())
    finally:
        hook.remove()
    return fuse_predictions(scores, seg_size, return_probs=return_probs)
