"""The pyramid pooling module of the semantic decoders on the device (reference: semantic/models.py:336-346, 387-397, the loop
over self.ppm and the torch.cat in PPMBilinear.forward / PPMBilinearDeepsup.forward).

    handle = use_device_ppm(segmentation_module.decoder)      # once; handle.remove() puts the class's forward back

or, inside a forward of one's own, `x = decoder.conv_last(ppm_concat(decoder, conv5))`.  The reference pools conv5 four times,
runs each branch's 1 x 1 conv / BN / ReLU, upsamples the four results and concatenates five tensors; here conv5 is read once
(ppm_pool: the copy into the concatenated tensor and all pooled tensors in one launch), the branch modules run as they are on the
pooled tensors, and ppm_fill writes their upsampled outputs into the remaining channels in one launch.  Backward is two launches
as well.  The kernels are csrc/segm_ppm.hip behind sdn_hip.ops.segm_ppm_pool / segm_ppm_fill; CPU tensors raise
NotImplementedError and there is no torch form.  The branch modules (SyncBN included), conv_last and the C1 decoders stay the
caller's.
"""
import types

import numpy as np
import torch
from torch import nn

from sdn_hip import ops


def ppm_pool(conv5, scales, branch_channels):
    """(cat, p_1 .. p_S): cat CUDA fp32 [B, C + sum K_k, h, w] with conv5 in its first C channels (bit for bit) and the others
    unwritten until ppm_fill; p_k [B, C, s_k, s_k] = AdaptiveAvgPool2d(s_k)(conv5).  See sdn_hip.ops.segm_ppm_pool."""
    return ops.segm_ppm_pool(conv5, scales, branch_channels)


def ppm_fill(cat, C, *ys):
    """Writes the bilinear upsampling (align_corners=False) of the branch outputs y_k [B, K_k, s_k, s_k] (as arguments, or one
    list of them) into cat[:, C:] in place and returns cat.  See sdn_hip.ops.segm_ppm_fill."""
    return ops.segm_ppm_fill(cat, C, *ys)


def ppm_bins(n, s):
    """The s bins of nn.AdaptiveAvgPool2d over n positions: a list of (start, end), end exclusive: floor(i n / s) and
    ceil((i + 1) n / s) in exact integers.  Host mirror of csrc/segm_ppm_check.h: ppm_bin_start / ppm_bin_end."""
    n, s = int(n), int(s)
    if n < 1 or s < 1:
        raise ValueError('n and s must be >= 1, got %d and %d' % (n, s))
    return [((i * n) // s, ((i + 1) * n + s - 1) // s) for i in range(s)]


def ppm_lerp(n, s):
    """(i0 int32 [n], i1 int32 [n], lam float32 [n]): the taps and the weight of the second tap of the bilinear upsampling of s
    positions to n, align_corners=False, by torch's fp32 rule.  Host mirror of csrc/segm_ppm_check.h: ppm_taps."""
    n, s = int(n), int(s)
    if n < 1 or s < 1:
        raise ValueError('n and s must be >= 1, got %d and %d' % (n, s))
    scale = np.float32(s) / np.float32(n)
    src = scale * (np.arange(n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int32), s - 1)
    i1 = np.minimum(i0 + 1, s - 1).astype(np.int32)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def _branches(decoder):
    """[(s_k, K_k, the branch's modules after its pooling layer)] of decoder.ppm"""
    ppm = getattr(decoder, 'ppm', None)
    if ppm is None or not hasattr(decoder, 'conv_last'):
        raise ValueError('%s has no ppm / conv_last: only the pyramid pooling decoders (PPMBilinear, PPMBilinearDeepsup) have the '
                         'module this replaces' % type(decoder).__name__)
    if not 1 <= len(ppm) <= ops.SEGM_PPM_MAX_SCALES:
        raise ValueError('decoder.ppm has %d branches; 1 to %d are supported' % (len(ppm), ops.SEGM_PPM_MAX_SCALES))
    out = []
    for k, branch in enumerate(ppm):
        pool = branch[0]
        size = getattr(pool, 'output_size', None)
        if not isinstance(pool, nn.AdaptiveAvgPool2d):
            raise ValueError('decoder.ppm[%d][0] is %s, not nn.AdaptiveAvgPool2d' % (k, type(pool).__name__))
        if isinstance(size, (tuple, list)):
            if len(size) != 2 or size[0] != size[1]:
                raise ValueError('decoder.ppm[%d] pools to %r; only square sizes are supported' % (k, size))
            size = size[0]
        if isinstance(size, bool) or not isinstance(size, int):
            raise ValueError('decoder.ppm[%d] pools to %r; an int or an equal pair is needed' % (k, size))
        if not 1 <= size <= ops.SEGM_PPM_MAX_SIDE:
            raise ValueError('decoder.ppm[%d] pools to %d; 1 to %d are supported' % (k, size, ops.SEGM_PPM_MAX_SIDE))
        tail = branch[1:]
        convs = [m for m in tail if isinstance(m, nn.Conv2d)]
        if not convs:
            raise ValueError('decoder.ppm[%d] has no Conv2d after its pooling layer: its output channels are unknown' % k)
        out.append((size, int(convs[0].out_channels), tail))
    return out


def ppm_concat(decoder, conv5):
    """The tensor decoder.conv_last takes: torch.cat([conv5] + [upsample(branch(conv5)) for branch in decoder.ppm], 1) of
    models.py:339-346 / 390-397, for conv5 CUDA fp32 [B, C, h, w].  s_k is read from decoder.ppm[k][0].output_size (an int or an
    equal pair), K_k from the Conv2d of decoder.ppm[k][1:]; those modules run on the pooled tensors as they are, so their
    parameters, running statistics and train / eval behaviour are the caller's."""
    branches = _branches(decoder)
    if isinstance(conv5, torch.Tensor) and conv5.is_cuda:
        conv5 = conv5.contiguous()                 # an autograd op: the gradient flows back through the strides
    res = ppm_pool(conv5, [s for s, _, _ in branches], [k for _, k, _ in branches])
    cat, pooled = res[0], res[1:]
    ys = [tail(p) for (_, _, tail), p in zip(branches, pooled)]
    for k, ((s, K, _), y) in enumerate(zip(branches, ys)):
        if tuple(y.shape) != (conv5.shape[0], K, s, s):
            raise ValueError('decoder.ppm[%d][1:] returned %s for a pooled tensor [%d, %d, %d, %d]; [.., %d, %d, %d] was expected'
                             % (k, tuple(y.shape), conv5.shape[0], conv5.shape[1], s, s, K, s, s))
    return ppm_fill(cat, conv5.shape[1], ys)


def _forward(self, conv_out, segSize=None):
    """PPMBilinear.forward / PPMBilinearDeepsup.forward with ppm_concat for the pooling loop and the cat"""
    x = self.conv_last(ppm_concat(self, conv_out[-1]))
    if self.use_softmax:          # inference: probabilities at segSize
        x = nn.functional.interpolate(x, size=segSize, mode='bilinear', align_corners=False)
        return nn.functional.softmax(x, dim=1)
    x = nn.functional.log_softmax(x, dim=1)
    if not hasattr(self, 'cbr_deepsup'):
        return x
    d = self.cbr_deepsup(conv_out[-2])
    if hasattr(self, 'dropout_deepsup'):
        d = self.dropout_deepsup(d)
    d = self.conv_last_deepsup(d)
    return x, nn.functional.log_softmax(d, dim=1)


class PpmHandle:
    """What use_device_ppm returns: remove() restores the class's forward; also a context manager"""

    def __init__(self, decoder):
        self.decoder = decoder

    def remove(self):
        if self.decoder is not None:
            self.decoder.__dict__.pop('forward', None)
            self.decoder = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.remove()
        return False


def use_device_ppm(decoder):
    """Gives `decoder` (a PPMBilinear or PPMBilinearDeepsup, or any module with their attributes: ppm, conv_last, use_softmax,
    optionally cbr_deepsup / dropout_deepsup / conv_last_deepsup) an instance-level forward that does what the class's does with
    ppm_concat in place of the pooling loop and the cat: the same return values -- softmax at segSize with use_softmax, else
    log_softmax, a pair with deep supervision -- and the same parameters, buffers and state_dict.  segm_tail.predict and
    train_loss.train_forward work on a decoder so patched: they hook conv_last.  Returns a PpmHandle."""
    if not isinstance(decoder, nn.Module):
        raise TypeError('decoder must be an nn.Module, got %r' % (type(decoder),))
    _branches(decoder)            # refused here, with the reason, not at the first forward
    if not hasattr(decoder, 'use_softmax'):
        raise ValueError('%s has no use_softmax attribute' % type(decoder).__name__)
    if hasattr(decoder, 'cbr_deepsup') != hasattr(decoder, 'conv_last_deepsup'):
        raise ValueError('%s has one of cbr_deepsup / conv_last_deepsup without the other' % type(decoder).__name__)
    if 'forward' in decoder.__dict__:
        raise ValueError('this decoder already has an instance-level forward')
    decoder.forward = types.MethodType(_forward, decoder)
    return PpmHandle(decoder)
