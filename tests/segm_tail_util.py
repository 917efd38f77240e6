"""Shared pieces of the semantic-tail tests (tests/test_segm_tail_host.py, tests/test_gpu_segm_tail.py) and of the fixture's
generator (tests/golden/make_segm_tail_golden.py): the case shapes, the seeded score maps and the reference pipeline restated
with torch.nn.functional (semantic/models.py:401-402, vkitti_test.py:58-72).  The generator proves the restatement equal,
bit for bit, to the reference decoder's own tail before it stores anything."""
import hashlib
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'segm_tail_golden.npz')

# name: (seed, B, C, (H, W), [(h_s, w_s), ...])
CASES = {
    'a': (11, 1, 14, (37, 50), [(5, 7), (8, 11), (13, 19)]),                 # non-integer ratios, clamped borders
    'b': (12, 1, 3, (9, 70), [(9, 70)]),                                     # the identity scale, wider than a wave
    'c': (13, 2, 32, (33, 65), [(2, 3), (5, 9), (9, 17), (17, 33), (24, 40), (33, 65), (40, 80), (12, 70)]),   # the limits
}
FULL = (14, 1, 14, (375, 1242), [(13, 42), (19, 63), (25, 83), (38, 125), (47, 156)])   # seeded in the GPU test only
# The full-size case draws SMOOTH maps (draw_smooth_scores).  At x near 1242 the fp32 source position of the reference carries an
# error of an ulp of 156 (1.5e-5); times the slope between two neighbouring scores that is the reference's own error e_ref.
# With independent 3 * randn per map pixel the slopes are as steep as they can be: e_ref is 8e-6 .. 1.1e-5 for every seed
# (torch fp32 against float64, sixteen seeds tried) and 0.10 .. 0.13 % of the pixels lie inside the 8 e_ref band, whatever the
# amplitude (0.5 to 10 times randn tried) -- the inputs themselves miss the 0.1 % the label gate presupposes.  Maps of the same
# amplitude (std 3.1) that vary over four map pixels, as a decoder's do, give e_ref 2.9e-6 and 0.04 % inside the band.
# Case c's eight maps (1.0 MB) and its float64 probabilities (1.1 MB) do not fit a committed file: the fixture holds their
# SHA-256 / a strided sample instead, the maps are redrawn from the seed and the float64 pipeline is run again by the test.
SAMPLE_STRIDE = 16


def draw_scores(seed, B, C, sizes):
    """3 * randn per map from numpy's frozen RandomState stream (identical on every numpy)."""
    rs = np.random.RandomState(seed)
    return [(3.0 * rs.randn(B, C, h, w)).astype(np.float32) for h, w in sizes]


def _linear(n, m):
    """[n, m] weights of the linear interpolation from m knots to n samples, end on end"""
    pos = np.linspace(0, m - 1, n)
    i0 = np.minimum(pos.astype(np.int64), m - 2)
    f = pos - i0
    w = np.zeros((n, m))
    w[np.arange(n), i0] = 1 - f
    w[np.arange(n), i0 + 1] += f
    return w


def draw_smooth_scores(seed, B, C, sizes, step=4, amp=4.5):
    """Per map a randn field on a grid of one knot per `step` map pixels, interpolated linearly to the map; amp 4.5 restores
    the standard deviation 3 the interpolation takes away."""
    rs = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        hc, wc = max(2, -(-h // step) + 1), max(2, -(-w // step) + 1)
        g = rs.randn(B, C, hc, wc)
        out.append((amp * np.einsum('yi,bcij,xj->bcyx', _linear(h, hc), g, _linear(w, wc))).astype(np.float32))
    return out


def digest(arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def pipeline(scores, seg_size, dtype=torch.float32, device='cpu'):
    """pred = sum_s softmax(upsample(scores_s, seg_size, 'bilinear'), dim=1) / S, scale by scale as vkitti_test.py:58-70 does
    (align_corners=False: torch 0.4's default for upsample, which is what the reference runs)."""
    H, W = seg_size
    first = torch.as_tensor(scores[0])
    pred = torch.zeros(first.shape[0], first.shape[1], H, W, dtype=dtype, device=device)
    for t in scores:
        x = torch.as_tensor(t).to(device=device, dtype=dtype)
        x = torch.nn.functional.interpolate(x, size=(H, W), mode='bilinear', align_corners=False)
        x = torch.nn.functional.softmax(x, dim=1)
        pred = pred + x / len(scores)
    return pred


def margins(pred64):
    """(argmax, top-1 minus top-2) of float64 probabilities [B, C, H, W]; a pixel with a NaN gets margin NaN."""
    p = torch.as_tensor(pred64)
    top = torch.topk(p, 2, dim=1)
    return top.indices[:, 0], top.values[:, 0] - top.values[:, 1]


def check_gates(name, pred_dev, labels_dev, pred64, e_ref, band_cap=0.001):
    """The issue's gates on one case; prints each figure before it asserts.  Returns (ratio, band fraction)."""
    pred64 = torch.as_tensor(pred64)
    err = float((pred_dev.double() - pred64).abs().max())
    ratio = err / e_ref
    arg, margin = margins(pred64)
    clear = margin > 8 * e_ref
    band = 1.0 - float(clear.double().mean())
    wrong = int((labels_dev[:, 0].long()[clear] != arg[clear]).sum())
    print('segm_tail case %s: max |pred_dev - pred64| = %.3e = %.2f e_ref (e_ref %.3e); %d of %d pixels inside the 8 e_ref band; '
          '%d labels differ outside it' % (name, err, ratio, e_ref, int((~clear).sum()), clear.numel(), wrong))
    assert err <= 4 * e_ref, 'probabilities: %.3e is %.2f e_ref, the gate is 4' % (err, ratio)
    assert band <= band_cap, '%.4f %% of the pixels lie inside the band' % (100 * band)
    assert wrong == 0, '%d labels differ from argmax(pred64) outside the band' % wrong
    return ratio, band
