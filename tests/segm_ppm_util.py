"""Shared pieces of the pyramid-pooling tests (tests/test_segm_ppm_host.py, tests/test_gpu_segm_ppm.py) and of the fixture's
generator (tests/golden/make_segm_ppm_golden.py): the cases, the seeded inputs, the float64 truth -- torch's own
adaptive_avg_pool2d, interpolate(bilinear, align_corners=False), cat and autograd on the CPU, which is what the loop of
semantic/models.py:339-346 / 390-397 runs -- and a stand-in decoder with the attribute layout semantic.ppm reads.  The generator
runs the reference's own PPMBilinearDeepsup beside `module_reference` and asserts that they agree before it stores anything."""
import os

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'segm_ppm_golden.npz')

REF_SCALES = (1, 2, 3, 6)
# name: (seed, B, C, K per branch, h, w, scales)
CASES = {
    'odd': (5101, 2, 8, (4, 4, 4, 4), 7, 13, REF_SCALES),        # nothing divides: overlapping bins, the scalar path
    'even': (5102, 2, 8, (4, 4, 4, 4), 6, 12, REF_SCALES),       # disjoint bins, identity upsample at s = h = 6, 16-byte path
    'tiny1': (5103, 1, 4, (2, 2, 2, 2), 1, 1, REF_SCALES),       # h < s: the pixel lies in every bin
    'tiny53': (5104, 2, 4, (2, 2, 2, 2), 5, 3, REF_SCALES),      # h < 6, w < 6: more than two bins per pixel, bilinear shrinking
    'wide': (5105, 1, 4, (2, 2, 2, 2), 13, 156, REF_SCALES),     # the real row width, sums of 2028 terms, 16-byte path
    'mixed': (5106, 2, 5, (1, 2, 3, 5), 9, 10, REF_SCALES),      # unequal K, odd C, plane bases off 16 bytes
    'fewer2': (5107, 2, 8, (4,), 7, 13, (2,)),                   # S = 1
    'fewer18': (5108, 2, 8, (4, 4), 11, 17, (1, 8)),             # S = 2, scale 8
    # beyond one LDS tile of the kernels (16 rows x 256 columns; 8 rows when the scales have 32 column bins between them)
    'tiles4': (5109, 1, 2, (1, 1, 1, 1), 19, 260, REF_SCALES),   # two row chunks, two column tiles, 16-byte path
    'tiles1': (5110, 1, 2, (1, 1, 1, 1), 17, 259, (8, 8, 8, 8)), # three row chunks of 8, two column tiles, the scalar path
}
QUANTITIES = ('pooled', 'branches', 'grad_conv5', 'grad_y')

# the module-level fixture: the reference's PPMBilinearDeepsup(num_class=5, fc_dim=16); its 512 branch channels are hard-coded
MOD_CLASSES, MOD_FC, MOD_K, MOD_H, MOD_W = 5, 16, 512, 7, 13
MOD_BATCH = {'eval': 1, 'train': 2}     # B = 1 makes BN raise on the 1 x 1 branch in training
MOD_SEED = {'eval': 5201, 'train': 5202, 'state': 5203}
MOD_QUANTITIES = ('cat', 'grad_conv5', 'grad_w0', 'grad_w1', 'grad_w2', 'grad_w3')
SAMPLE_STRIDE = {'cat': 32, 'grad_conv5': 1, 'grad_w0': 8, 'grad_w1': 8, 'grad_w2': 8, 'grad_w3': 8}


def draw_case(name):
    """dict of numpy arrays from numpy's frozen RandomState stream: conv5 fp32 [B, C, h, w]; ys: the branch outputs fp32
    [B, K_k, s_k, s_k], non-negative as after a ReLU; go fp32 [B, Ctot, h, w] and gps fp32 [B, C, s_k, s_k]: the upstream
    gradients of total = sum(go * cat) + sum_k sum(gp_k * p_k)"""
    seed, B, C, K, h, w, scales = CASES[name]
    rs = np.random.RandomState(seed)
    conv5 = (rs.randn(B, C, h, w) * 2.0 + 0.5).astype(np.float32)
    ys = [np.maximum(rs.randn(B, k, s, s), 0.0).astype(np.float32) for k, s in zip(K, scales)]
    go = rs.randn(B, C + sum(K), h, w).astype(np.float32)
    gps = [rs.randn(B, C, s, s).astype(np.float32) for s in scales]
    return dict(conv5=conv5, ys=ys, go=go, gps=gps, scales=tuple(scales), K=tuple(K), C=C)


def reference(case, dtype=torch.float64):
    """torch on the CPU in `dtype`: (pooled list, cat, grad_conv5, grad_y list) as numpy arrays of that dtype"""
    x = torch.as_tensor(case['conv5']).to(dtype).requires_grad_()
    ys = [torch.as_tensor(y).to(dtype).requires_grad_() for y in case['ys']]
    h, w = x.shape[2:]
    ps = [F.adaptive_avg_pool2d(x, s) for s in case['scales']]
    cat = torch.cat([x] + [F.interpolate(y, size=(h, w), mode='bilinear', align_corners=False) for y in ys], 1)
    total = (torch.as_tensor(case['go']).to(dtype) * cat).sum()
    for gp, p in zip(case['gps'], ps):
        total = total + (torch.as_tensor(gp).to(dtype) * p).sum()
    total.backward()
    return dict(pooled=[p.detach().numpy() for p in ps], cat=cat.detach().numpy(), grad_conv5=x.grad.numpy(),
                grad_y=[y.grad.numpy() for y in ys])


def rel(got, want):
    """relative 2-norm of the difference, in float64; the absolute norm where the truth is all zeros"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.linalg.norm(got))


def flat(arrays):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays])


def errors(got, want, C):
    """the four gated figures of a case: pooled tensors, the channels >= C of cat, grad_conv5, grad_y -- each the relative
    2-norm over everything of its kind"""
    return {'pooled': rel(flat(got['pooled']), flat(want['pooled'])),
            'branches': rel(np.asarray(got['cat'])[:, C:], np.asarray(want['cat'])[:, C:]),
            'grad_conv5': rel(got['grad_conv5'], want['grad_conv5']),
            'grad_y': rel(flat(got['grad_y']), flat(want['grad_y']))}


# ---- the stand-in decoder -------------------------------------------------------------------------------------------------------
class Decoder(nn.Module):
    """The attribute layout of the reference's PPMBilinear / PPMBilinearDeepsup (models.py:311-334, 359-385) and what their
    forward does, written for the tests: ppm is a ModuleList of Sequential(AdaptiveAvgPool2d, Conv2d 1 x 1 without bias,
    BatchNorm2d, ReLU), conv_last a Sequential, cbr_deepsup / conv_last_deepsup / dropout_deepsup optional.  The module names
    and indices are the reference's, so its state_dict keys fit."""

    def __init__(self, num_class=MOD_CLASSES, fc_dim=MOD_FC, branch=MOD_K, mid=8, pool_scales=REF_SCALES, deepsup=False,
                 use_softmax=False, pair_sizes=False):
        super().__init__()
        self.use_softmax = use_softmax
        self.ppm = nn.ModuleList([nn.Sequential(nn.AdaptiveAvgPool2d((s, s) if pair_sizes else s),
                                                nn.Conv2d(fc_dim, branch, kernel_size=1, bias=False),
                                                nn.BatchNorm2d(branch), nn.ReLU(inplace=True)) for s in pool_scales])
        self.conv_last = nn.Sequential(nn.Conv2d(fc_dim + len(pool_scales) * branch, mid, kernel_size=3, padding=1, bias=False),
                                       nn.BatchNorm2d(mid), nn.ReLU(inplace=True), nn.Dropout2d(0.1),
                                       nn.Conv2d(mid, num_class, kernel_size=1))
        if deepsup:
            self.cbr_deepsup = nn.Sequential(nn.Conv2d(fc_dim // 2, fc_dim // 4, kernel_size=3, padding=1, bias=False),
                                             nn.BatchNorm2d(fc_dim // 4), nn.ReLU(inplace=True))
            self.conv_last_deepsup = nn.Conv2d(fc_dim // 4, num_class, 1, 1, 0)
            self.dropout_deepsup = nn.Dropout2d(0.1)

    def concat(self, conv5):
        h, w = conv5.shape[2:]
        outs = [conv5]
        for branch in self.ppm:
            outs.append(F.interpolate(branch(conv5), size=(h, w), mode='bilinear', align_corners=False))
        return torch.cat(outs, 1)

    def forward(self, conv_out, segSize=None):
        x = self.conv_last(self.concat(conv_out[-1]))
        if self.use_softmax:
            x = F.interpolate(x, size=segSize, mode='bilinear', align_corners=False)
            return F.softmax(x, dim=1)
        x = F.log_softmax(x, dim=1)
        if not hasattr(self, 'cbr_deepsup'):
            return x
        d = self.conv_last_deepsup(self.dropout_deepsup(self.cbr_deepsup(conv_out[-2])))
        return x, F.log_softmax(d, dim=1)


def draw_state():
    """the ppm.* part of the state_dict, float64 values that fp32 holds exactly: the 1 x 1 weights are multiples of 1 / 64 (the
    fixture keeps them as int8), the BN parameters and running statistics fp32 draws"""
    rs = np.random.RandomState(MOD_SEED['state'])
    state = {}
    for k in range(len(REF_SCALES)):
        q = np.clip(np.round(rs.randn(MOD_K, MOD_FC, 1, 1) * 16.0), -127, 127)
        state['ppm.%d.1.weight' % k] = q / 64.0
        state['ppm.%d.2.weight' % k] = (0.5 + rs.rand(MOD_K)).astype(np.float32).astype(np.float64)
        state['ppm.%d.2.bias' % k] = (rs.randn(MOD_K) * 0.3).astype(np.float32).astype(np.float64)
        state['ppm.%d.2.running_mean' % k] = (rs.randn(MOD_K) * 0.5).astype(np.float32).astype(np.float64)
        state['ppm.%d.2.running_var' % k] = (0.5 + rs.rand(MOD_K)).astype(np.float32).astype(np.float64)
    return state


def draw_module_case(mode):
    """(conv5 fp32 [B, 16, 7, 13], go fp32 [B, 16 + 4 * 512, 7, 13]: the upstream gradient on conv_last's input)"""
    rs = np.random.RandomState(MOD_SEED[mode])
    B = MOD_BATCH[mode]
    conv5 = (rs.randn(B, MOD_FC, MOD_H, MOD_W) * 1.5).astype(np.float32)
    go = rs.randn(B, MOD_FC + len(REF_SCALES) * MOD_K, MOD_H, MOD_W).astype(np.float32)
    return conv5, go


def load_ppm_state(decoder, state):
    """the fixture's ppm.* tensors into a decoder (either the stand-in or the reference's), everything else left as built"""
    own = decoder.state_dict()
    for k, v in state.items():
        assert k in own, k
        own[k] = torch.as_tensor(np.asarray(v)).to(own[k].dtype).reshape(own[k].shape)
    decoder.load_state_dict(own)


def module_results(decoder, concat, conv5, go):
    """MOD_QUANTITIES of `concat(conv5)` on `decoder` (already in the wanted mode, dtype and device) as float64 numpy arrays:
    the concatenated tensor and the gradients of sum(go * cat) in conv5 and the four 1 x 1 weights"""
    dev = next(decoder.parameters()).device
    dtype = next(decoder.parameters()).dtype
    x = torch.as_tensor(conv5).to(device=dev, dtype=dtype).requires_grad_()
    cat = concat(x)
    ws = [decoder.ppm[k][1].weight for k in range(len(decoder.ppm))]
    grads = torch.autograd.grad((torch.as_tensor(go).to(device=dev, dtype=dtype) * cat).sum(), [x] + ws)
    out = {'cat': cat, 'grad_conv5': grads[0]}
    out.update({'grad_w%d' % k: g for k, g in enumerate(grads[1:])})
    return {k: v.detach().cpu().double().numpy() for k, v in out.items()}


def module_reference(mode, dtype=torch.float64, state=None):
    """the stand-in decoder on the CPU in `dtype` with the drawn state: MOD_QUANTITIES"""
    torch.manual_seed(MOD_SEED[mode])
    dec = Decoder().to(dtype)
    load_ppm_state(dec, draw_state() if state is None else state)
    dec.train(mode == 'train')
    conv5, go = draw_module_case(mode)
    return module_results(dec, dec.concat, conv5, go)


def fixture_state(gold):
    """the ppm.* state of the fixture as float64 numpy arrays"""
    state = {}
    for k in range(len(REF_SCALES)):
        state['ppm.%d.1.weight' % k] = gold['state/ppm.%d.1.weight_q64' % k].astype(np.float64) / 64.0
        for name in ('weight', 'bias', 'running_mean', 'running_var'):
            state['ppm.%d.2.%s' % (k, name)] = gold['state/ppm.%d.2.%s' % (k, name)].astype(np.float64)
    return state


def check_against_fixture(gold, mode, res, tol=1e-12):
    """float64 results of a module case against the fixture's samples and 2-norms"""
    for q in MOD_QUANTITIES:
        a = res[q].reshape(-1)
        want, norm = gold['%s/%s_sample' % (mode, q)], float(gold['%s/%s_norm' % (mode, q)])
        assert np.allclose(a[::SAMPLE_STRIDE[q]], want, rtol=tol, atol=tol * norm / np.sqrt(a.size)), (mode, q)
        assert abs(np.linalg.norm(a) - norm) <= tol * norm, (mode, q)
