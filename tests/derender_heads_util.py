"""What the tests of sdn_hip.ops.derender_heads share: the cases, the seeded fixtures, the restatement and the gate.

The restatement (`heads`) is the reference's own expressions -- geometric/derender3d/models/derenderer.py:34-56 and the roi
arithmetic of models/__init__.py:70-77 -- written with torch CPU functional ops, runnable in fp32 and in fp64; `norm_grad_loop` and
`softmax_grad_loop` are the two non-linear gradients as explicit loops, which the host test holds against autograd.

The gate is the project's own (README, "pyramid RoIAlign"): a group of values is within 1e-6 of the group's largest fp64 magnitude,
or, where the fp32 restatement's own distance from fp64 is larger than that, within 4 x that distance; always measured against the
fp64 restatement.

Fixture conditions (checked on the CPU by tests/test_derender_heads_host.py for every case): every hidden pre-activation lies at least
16 x the fp32 restatement's largest distance from fp64 at that layer away from 0, so fp32 and fp64 take the same side of every ReLU;
every raw pose pair has an fp64 norm of at least 0.1, except the one deliberate zero row of the case 'zero_row'.  SEEDS holds, per
case, a seed for which this holds."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ('_theta_deltas', '_translation2ds', '_log_scales', '_log_depths', '_class_probs', '_ffd_coeffs')
PARAMS = ('fc.weight', 'fc.bias', 'fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'fc3.weight', 'fc3.bias')

# name: (F, Hd, classes, grid size g (coeffs = 3 g^3), n)
CASES = {
    'real_16': (512, 256, 8, 4, 16),     # the real widths, O = 1552: one row tile
    'real_1': (512, 256, 8, 4, 1),       # one row
    'real_17': (512, 256, 8, 4, 17),     # one row past a tile
    'real_67': (512, 256, 8, 4, 67),     # several tiles with a tail; two object chunks of a weight gradient
    'one_class': (8, 4, 1, 1, 19),       # the degenerate softmax; every width below a tile
    'odd': (36, 20, 3, 2, 19),           # O = 83: unaligned tails everywhere
    'sixteen': (16, 8, 16, 1, 19),       # 16 classes: the head columns fill 24 of the first workgroup's 32
    'zero_row': (36, 20, 3, 2, 5),       # object 2 has an exactly zero pose pair
}
SEEDS = {'real_16': 3, 'real_1': 1, 'real_17': 3, 'real_67': 3,'one_class': 1, 'odd': 1, 'sixteen': 1, 'zero_row': 1}
ZERO_ROW = 2
MARGIN, MIN_NORM = 16.0, 0.1


def widths(name):
    f, hd, classes, g, n = CASES[name]
    coeffs = 3 * g ** 3
    return f, hd, classes, coeffs, 8 + classes + classes * coeffs, n


def draw(name, seed=None):
    """(pooled [n, F] >= 0, roi_norms [n, 4], the eight parameters in PARAMS' order), fp32 on the CPU"""
    f, hd, classes, coeffs, O, n = widths(name)
    g = torch.Generator().manual_seed(1000 * (SEEDS[name] if seed is None else seed) + 7)

    def linear(out, inp):   # nn.Linear's own initial range
        bound = inp ** -0.5
        return [(torch.rand(out, inp, generator=g) * 2 - 1) * bound, (torch.rand(out, generator=g) * 2 - 1) * bound]
    params = linear(hd, f) + linear(hd, hd + 4) + linear(hd, hd) + linear(O, hd)
    params[7][0:2] = torch.tensor([0.8, -0.6])           # the raw pose pair stays away from zero
    pooled = torch.rand(n, f, generator=g)                # pooled post-ReLU features
    top_left = -torch.rand(n, 2, generator=g) * 0.5
    roi_norms = torch.cat((top_left, top_left + 0.1 + torch.rand(n, 2, generator=g) * 0.5), dim=1)
    if name == 'zero_row':
        # an object whose activations are all zero gets the bias of fc3 alone: no hidden bias above zero, a zero feature row, a zero roi
        for i in (1, 3, 5):
            params[i] = -params[i].abs() * 0.05
        params[7][0:2] = 0.0
        params[6][0:2] *= 64.0                            # the other objects' pairs stay long enough
        pooled[ZERO_ROW] = 0.0
        roi_norms[ZERO_ROW] = 0.0
    return pooled, roi_norms, params


def heads(pooled, rois, params, classes, keep=None):
    """the reference's expressions; rois: roi_norms [n, 4] or (centre, extent).  `keep`, a dict, receives the pre-activations, the row
    and the roi vectors."""
    w0, b0, w1, b1, w2, b2, w3, b3 = params
    if isinstance(rois, torch.Tensor):
        top_left, bottom_right = rois[:, 0:2], rois[:, 2:4]
        centre, extent = (bottom_right + top_left) / 2.0, bottom_right - top_left
    else:
        centre, extent = rois
    z0 = F.linear(pooled, w0, b0)
    z1 = F.linear(torch.cat((F.relu(z0), centre, extent), dim=1), w1, b1)
    z2 = F.linear(F.relu(z1), w2, b2)
    row = F.linear(F.relu(z2), w3, b3)
    if keep is not None:
        keep.update(pre=(z0, z1, z2), row=row, centre=centre, extent=extent)
    n = row.shape[0]
    delta, logits = row[:, 0:2], row[:, 8:8 + classes]
    return {
        '_theta_deltas': delta / torch.norm(delta, p=2, dim=1, keepdim=True),
        '_translation2ds': row[:, 2:4],
        '_log_scales': row[:, 4:7],
        '_log_depths': row[:, 7:8],
        '_class_probs': torch.softmax(logits, dim=1),
        '_ffd_coeffs': row[:, 8 + classes:].reshape(n, classes, -1),
    }


def norm_grad_loop(row2, g):
    """d loss / d (r0, r1) of d = r / |r| given g = d loss / d d, object by object: (g - d (d.g)) / |r|"""
    out = np.zeros_like(row2)
    for i in range(row2.shape[0]):
        norm = (row2[i, 0] ** 2 + row2[i, 1] ** 2) ** 0.5
        d = row2[i] / norm
        dot = d[0] * g[i, 0] + d[1] * g[i, 1]
        for c in range(2):
            out[i, c] = (g[i, c] - d[c] * dot) / norm
    return out


def softmax_grad_loop(p, g):
    """d loss / d logits given g = d loss / d p, object by object: p (g - sum p g)"""
    out = np.zeros_like(p)
    for i in range(p.shape[0]):
        dot = 0.0
        for c in range(p.shape[1]):
            dot += p[i, c] * g[i, c]
        for c in range(p.shape[1]):
            out[i, c] = p[i, c] * (g[i, c] - dot)
    return out


def out_grads(name, seed=5):
    """one gradient per output group, magnitudes below 1"""
    f, hd, classes, coeffs, O, n = widths(name)
    g = torch.Generator().manual_seed(seed)
    shapes = [(n, 2), (n, 2), (n, 3), (n, 1), (n, classes), (n, classes, coeffs)]
    return {k: torch.rand(s, generator=g) * 2 - 1 for k, s in zip(KEYS, shapes)}


@functools.lru_cache(maxsize=None)
def reference(name, subset=KEYS):
    """{'out32', 'out64': the blobs; 'grad32', 'grad64': the gradients of pooled and the eight parameters for the output gradients of
    `subset` (out_grads); 'keep32', 'keep64'}; computed once per case and subset, shared and never modified"""
    pooled, roi_norms, params = draw(name)
    classes = widths(name)[2]
    res = {}
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        leaves = [pooled.to(dtype).requires_grad_(True)] + [p.to(dtype).requires_grad_(True) for p in params]
        keep = {}
        blob = heads(leaves[0], roi_norms.to(dtype), leaves[1:], classes, keep)
        g = out_grads(name)
        grads = torch.autograd.grad([blob[k] for k in subset], leaves, [g[k].to(dtype) for k in subset], allow_unused=True)
        res['out' + tag] = {k: v.detach() for k, v in blob.items()}
        res['grad' + tag] = dict(zip(('pooled',) + PARAMS, grads))
        res['keep' + tag] = {k: ([t.detach() for t in v] if isinstance(v, tuple) else v.detach()) for k, v in keep.items()}
    return res


def gate(got, want64, want32):
    """(distance of got from fp64, the bound): 1e-6 of the group's largest fp64 magnitude, or 4 x the fp32 restatement's own distance"""
    want64 = want64.double()
    scale = float(want64.abs().max())
    own = float((want32.double() - want64).abs().max())
    distance = float((got.detach().cpu().double() - want64).abs().max())
    return distance, max(1e-6 * scale, 4.0 * own), own, scale


def fixture_figures(name, seed=None):
    """(smallest |pre-activation| / fp32 distance per hidden layer, ReLU masks equal, the pose pairs' fp64 norms)"""
    pooled, roi_norms, params = draw(name, seed)
    classes = widths(name)[2]
    keep32, keep64 = {}, {}
    heads(pooled, roi_norms, params, classes, keep32)
    heads(pooled.double(), roi_norms.double(), [p.double() for p in params], classes, keep64)
    ratios, same = [], True
    rows = torch.ones(pooled.shape[0], dtype=torch.bool)
    if name == 'zero_row':
        rows[ZERO_ROW] = False      # its pre-activations are the (non-positive) biases themselves, exact in both precisions
    for z32, z64 in zip(keep32['pre'], keep64['pre']):
        own = float((z32.double() - z64).abs().max())
        ratios.append(float(z64[rows].abs().min()) / max(own, 1e-300))
        same = same and bool(((z32 > 0) == (z64 > 0)).all())
    return ratios, same, torch.norm(keep64['row'][:, 0:2], dim=1)
