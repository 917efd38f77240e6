"""Shared pieces of the semantic-loss tests (tests/test_segm_loss_host.py, tests/test_gpu_segm_loss.py) and of the fixture's
generator (tests/golden/make_segm_loss_golden.py): the cases, the seeded inputs and the reference's expressions restated with
torch (semantic/models.py:15-21, 39-44 with the decoders' log_softmax, :279-280, 412-413, and nn.NLLLoss(ignore_index=-1),
vkitti_train.py:133).  The generator runs the reference's own pixel_acc beside the restated one and asserts that they agree
before it stores anything."""
import os

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'segm_loss_golden.npz')

BLOCK_PIXELS = 256      # csrc/segm_loss_check.h: SGL_PIXELS, the pixels of an item that one workgroup takes
SCALE = 0.4             # the reference's default --deep_sup_scale
# weights of the backward pass: d(total) / d(loss, acc, loss_main, loss_deepsup).  Distinct, so that a swapped grad_out slot or
# a missing deep_sup_scale shows; acc carries no gradient, whatever its weight
WEIGHTS = {'loss': 0.7, 'acc': 2.1, 'loss_main': 1.3, 'loss_deepsup': 0.45}
SAMPLE_STRIDE = 8       # the float64 gradients of the two larger cases are stored as every 8th element plus their 2-norm

# name: (seed, (B, C, h, w), deepsup head, label recipe)
CASES = {
    'small': (4101, (2, 14, 5, 7), True, 'plain'),        # the scalar path, less than one workgroup
    'maxc': (4102, (1, 32, 9, 65), True, 'plain'),        # C at its limit, 585 pixels: odd, three workgroups on the scalar path
    'c1': (4103, (2, 1, 4, 4), True, 'plain'),            # C = 1: loss 0, gradient 0
    'blocks': (4104, (3, 14, 12, 40), True, 'mixed'),     # 480 pixels: 16-byte loads, two workgroups per item; item 1 all -1;
                                                          # labels C and -2 among the others
    'blocks_nodeep': (4104, (3, 14, 12, 40), False, 'mixed'),   # the same inputs without the deepsup head
    'ignored': (4105, (2, 14, 5, 7), True, 'ignored'),    # no valid pixel: loss NaN, acc 0, gradient 0
}
STORED_WHOLE = ('small', 'c1', 'ignored')   # cases whose float64 gradients the fixture holds in full
assert 12 * 40 > BLOCK_PIXELS and (12 * 40) % 4 == 0 and (9 * 65) % 4 != 0 and 9 * 65 > 2 * BLOCK_PIXELS


def draw_scores(rs, shape):
    """seeded normals times 4, rounded to multiples of 1 / 8: the two best classes of a pixel are exactly tied or at least
    0.125 apart, so the arg-max of the scores, of fp32 log-probabilities and of float64 ones agree"""
    return (np.round(rs.randn(*shape) * 4.0 * 8.0) / 8.0).astype(np.float32)


def draw_case(name):
    """(scores fp32 [B, C, h, w], scores_deepsup or None, seg_label int64 [B, h, w]) from numpy's frozen RandomState stream"""
    seed, (B, C, h, w), deepsup, recipe = CASES[name]
    rs = np.random.RandomState(seed)
    scores = draw_scores(rs, (B, C, h, w))
    deep = draw_scores(rs, (B, C, h, w))          # drawn for every case, so that both variants of `blocks` share their inputs
    label = rs.randint(-1, C, (B, h, w)).astype(np.int64)
    best = scores.argmax(axis=1)
    label = np.where(rs.rand(B, h, w) < 0.5, best, label)   # a good share of hits
    if recipe == 'mixed':
        label[1] = -1
        bad = rs.rand(B, h, w) < 0.04
        bad[1] = False
        label = np.where(bad, np.where(rs.rand(B, h, w) < 0.5, C, -2), label)
    elif recipe == 'ignored':
        label[:] = -1
    return scores, (deep if deepsup else None), label


def clean_labels(label, C):
    """(labels with everything outside [0, C) turned into the ignore label -1, the number of labels that were neither valid
    nor -1).  The reference's NLLLoss raises on such a label; the device treats it as ignored and counts it."""
    label = torch.as_tensor(label)
    ok = (label >= 0) & (label < C)
    return torch.where(ok, label, torch.full_like(label, -1)), int((~ok & (label != -1)).sum())


def pixel_acc(pred, label):
    """semantic/models.py:15-21, statement for statement; returns (acc, acc_sum, pixel_sum)"""
    _, preds = torch.max(pred, dim=1)
    valid = (label >= 0).long()
    acc_sum = torch.sum(valid * (preds == label).long())
    pixel_sum = torch.sum(valid)
    acc = acc_sum.float() / (pixel_sum.float() + 1e-10)
    return acc, acc_sum, pixel_sum


def reference(scores, deepsup, label, scale=SCALE, dtype=torch.float64, acc_fn=None):
    """models.py:39-45 on the SCORES (the decoders' log_softmax first), in `dtype` on the CPU, with autograd for the gradients
    of sum(WEIGHTS[k] * loss_k).  Returns a dict: loss, loss_main, loss_deepsup (Python floats of dtype's values), acc (the fp32
    tensor value as a numpy float32), acc_sum, pixel_sum, bad, preds, grad, grad_deepsup (numpy, dtype's)."""
    C = scores.shape[1]
    lab, bad = clean_labels(label, C)
    x = torch.as_tensor(scores).to(dtype).requires_grad_()
    xd = torch.as_tensor(deepsup).to(dtype).requires_grad_() if deepsup is not None else None
    crit = nn.NLLLoss(ignore_index=-1)                       # vkitti_train.py:133
    pred = F.log_softmax(x, dim=1)                           # models.py:412
    loss_main = crit(pred, lab)                              # models.py:39
    loss = loss_main
    loss_deepsup = None
    if xd is not None:
        loss_deepsup = crit(F.log_softmax(xd, dim=1), lab)   # :413, :41
        loss = loss + loss_deepsup * scale                   # :42
    acc, acc_sum, pixel_sum = pixel_acc(pred.detach(), lab)  # :44
    if acc_fn is not None:
        theirs = acc_fn(pred.detach(), lab)
        assert theirs.dtype == acc.dtype and theirs.numpy().tobytes() == acc.numpy().tobytes(), 'pixel_acc differs from the reference'
    total = WEIGHTS['loss'] * loss + WEIGHTS['loss_main'] * loss_main
    if loss_deepsup is not None:
        total = total + WEIGHTS['loss_deepsup'] * loss_deepsup
    total.backward()
    return {
        'loss': float(loss.detach()), 'loss_main': float(loss_main.detach()),
        'loss_deepsup': float(loss_deepsup.detach()) if loss_deepsup is not None else 0.0,
        'acc': acc.numpy().astype(np.float32), 'acc_sum': int(acc_sum), 'pixel_sum': int(pixel_sum), 'bad': bad,
        'preds': torch.max(pred.detach(), dim=1)[1].numpy(),
        'grad': x.grad.numpy(), 'grad_deepsup': xd.grad.numpy() if xd is not None else None,
    }


def acc_fp32(acc_sum, pixel_sum):
    """models.py:20 in fp32, operation for operation"""
    return np.float32(acc_sum) / (np.float32(pixel_sum) + np.float32(1e-10))


def top_two_gap(scores):
    """per pixel the best score minus the second best, [B, h, w]; C >= 2"""
    s = np.sort(np.asarray(scores, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]
