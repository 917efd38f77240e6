"""The loss of a semantic training step on the device: the body of SegmentationModule.forward after the network call
(reference: semantic/models.py:15-21, 39-45; the decoders' log_softmax, models.py:279-280, 412-413; nn.NLLLoss(ignore_index=-1),
vkitti_train.py:133).

    batch = segm_train_batch(...)                                   # img_data, seg_label
    loss, acc = train_forward(segmentation_module, batch)           # instead of segmentation_module(batch)
    loss.backward()

or, with the scores at hand, `segm_losses(scores, batch['seg_label'], scores_deepsup, 0.4)`.  The kernels are csrc/segm_loss.hip
behind sdn_hip.ops.segm_loss; CPU tensors raise NotImplementedError and there is no torch form.
"""
import torch

from sdn_hip import ops

LOSS_KEYS = ('loss', 'acc', 'loss_main', 'loss_deepsup')
COUNT_KEYS = ('acc_sum', 'pixel_sum', 'bad')


def segm_losses(scores, seg_label, scores_deepsup=None, deep_sup_scale=None):
    """scores (and scores_deepsup, or None): CUDA fp32 [B, C, h, w], the outputs of decoder.conv_last (conv_last_deepsup) BEFORE
    log_softmax; seg_label: CUDA int64 [B, h, w] as segm_train_batch returns it (-1: ignored); deep_sup_scale: a Python float,
    required with scores_deepsup.  Returns a dict of 0-dim tensors:
        loss          loss_main + loss_deepsup * deep_sup_scale (models.py:42), or loss_main without a deepsup head
        acc           pixel_acc of the main head (models.py:15-21), fp32; no gradient
        loss_main     NLLLoss(ignore_index=-1) of log_softmax(scores); NaN when no pixel is valid, as torch's
        loss_deepsup  the same of scores_deepsup; 0 without one
        acc_sum, pixel_sum, bad   int64: the integers of pixel_acc and the number of labels outside [-1, C)
    The four fp32 values are views of one [4] tensor, the three integers of one [3] tensor; nothing is copied to the host.

    Two deviations from the reference, both where it has no defined answer: a label outside [-1, C) (NLLLoss raises) is ignored in
    the loss and the accuracy and counted in `bad`; a pixel with a NaN score predicts by a strict `>` scan from class 0 (the NaN
    never wins; torch.max returns the NaN's class) -- its loss is NaN as in torch.  Exact ties go to the lowest class, as
    torch.max on the CPU."""
    if scores_deepsup is not None and deep_sup_scale is None:
        raise ValueError('scores_deepsup needs a deep_sup_scale')
    if isinstance(scores, torch.Tensor) and scores.is_cuda:
        scores = scores.contiguous()                 # an autograd op: the gradient flows back through the strides
    if isinstance(scores_deepsup, torch.Tensor) and scores_deepsup.is_cuda:
        scores_deepsup = scores_deepsup.contiguous()
    out, counts = ops.segm_loss(scores, scores_deepsup, seg_label, deep_sup_scale)
    res = {k: out[i] for i, k in enumerate(LOSS_KEYS)}
    res.update({k: counts[i] for i, k in enumerate(COUNT_KEYS)})
    return res


def _layer(decoder, name):
    layer = getattr(decoder, name, None)
    if layer is None:
        raise ValueError('segmentation_module.decoder.%s not found: train_forward() reads the class scores there' % name)
    return layer


def train_forward(segmentation_module, feed_dict):
    """The training branch of SegmentationModule.forward (semantic/models.py:33-45): returns (loss, acc) as the reference does,
    both 0-dim fp32 CUDA tensors; loss carries the gradient to the network.

    A caller changes one line of the training loop, vkitti_train.py:37:
        loss, acc = segmentation_module(batch_data)      ->      loss, acc = train_forward(segmentation_module, batch_data)
    with batch_data = segm_train_batch(...) (or any dict with CUDA 'img_data' and int64 'seg_label'); `loss.mean()`,
    `acc.mean()` and `loss.backward()` after it stay as they are.  Under nn.DataParallel / a user-defined scatter, call it per
    replica on that replica's module and dict.

    The module returns log-probabilities (its decoders end in log_softmax), not scores, so the scores are taken with forward
    hooks on decoder.conv_last and, when segmentation_module.deep_sup_scale is not None, decoder.conv_last_deepsup -- the
    mechanism segm_tail.predict uses -- and the module's own return value (its log_softmax, NLLLoss and pixel_acc) is dropped.
    The forward pass runs with gradients enabled."""
    dec = getattr(segmentation_module, 'decoder', None)
    if dec is None:
        raise ValueError('segmentation_module.decoder not found: train_forward() reads the class scores there')
    scale = getattr(segmentation_module, 'deep_sup_scale', None)
    names = ('conv_last',) if scale is None else ('conv_last', 'conv_last_deepsup')
    layers = [_layer(dec, n) for n in names]   # refused before any hook is set
    grabbed = {n: [] for n in names}
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: grabbed[n].append(out)) for m, n in zip(layers, names)]
    try:
        segmentation_module(feed_dict)
    finally:
        for hk in hooks:
            hk.remove()
    for n in names:
        if len(grabbed[n]) != 1:
            raise RuntimeError('decoder.%s ran %d times in one forward pass' % (n, len(grabbed[n])))
    res = segm_losses(grabbed['conv_last'][0], feed_dict['seg_label'],
                      grabbed['conv_last_deepsup'][0] if scale is not None else None, scale)
    return res['loss'], res['acc']
