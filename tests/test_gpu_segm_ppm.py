"""semantic.ppm (sdn_segm_ppm_pool / _fill / _fill_bwd / _pool_bwd, csrc/segm_ppm.hip) against torch's own adaptive_avg_pool2d,
interpolate(bilinear, align_corners=False), cat and autograd in float64 on the CPU (tests/segm_ppm_util.py), which the fixture
tests/golden/segm_ppm_golden.npz pins to the reference's PPMBilinearDeepsup (tests/golden/make_segm_ppm_golden.py).

The numeric gate is the sibling tests' (GATE = 1e-6, relative 2-norm against float64) for the pooled tensors, the branch channels
of the concatenated tensor, grad_conv5 and the branch gradients of every case.  torch's own fp32 CPU run on the same draws sits
at 2.3e-8 to 6.1e-7, and at 1.7e-6 on the branch gradients of `wide` (an fp32 sum of 2028 terms of either sign); the fixture
holds these figures and the tests print them beside the device's.  The first C channels of the concatenated tensor, the
run-to-run bits, the channels_last bits, the None gradients and the reach of a NaN / an Inf are exact.  The module-level tests
gate eval() at GATE and train() at max(GATE, 4 x torch's fp32 CPU error of the fixture) per quantity: BatchNorm over the two
samples of a 1 x 1 branch amplifies rounding (torch alone: 2.6e-6 on grad_conv5).

The branch modules are the caller's, and so is their BatchNorm.  In train() the comparisons run with torch's native batch-norm
kernels (torch.backends.cudnn.flags(enabled=False)): MIOpen's fp32 batch norm over the two samples of the 1 x 1 branch is, by
itself, outside that gate -- measured once on an MI355X on the UNPATCHED stand-in decoder (torch's own pool / upsample / cat):
cat 2.1e-6, grad_conv5 5.1e-5, grad_w0 5.1e-5 against float64 with MIOpen, 3.0e-7, 1.2e-6, 9.3e-7 with the native kernels (the
CPU, whose fp32 batch norm accumulates in double: 3.7e-7, 2.6e-6, 1.9e-6).  Through ppm_concat the same run gave 3.0e-6, 1.3e-4,
1.3e-4 with MIOpen and 1.9e-7, 9.2e-7, 6.6e-7 with the native kernels; the pooled tensors that enter the branches were at 2.4e-8
(torch on the GPU: 5e-8 to 1e-7).  eval() runs with the default backend."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import segm_ppm_util as u

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-6


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty that fills what it returns: NaN for floats, 99 for integers -- whatever a kernel leaves unwritten shows"""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poison(t):
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(99)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: poison(real_empty(*a, **k)))
    monkeypatch.setattr(torch, 'empty_like', lambda *a, **k: poison(real_empty_like(*a, **k)))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def run_device(case, grad_x=True, grad_y=None, use_cat=True, use_gp=True, channels_last=False):
    """pool, fill and the backward pass of total = sum(go * cat) + sum_k sum(gp_k * p_k) on the device; tensors stay there"""
    from semantic import ppm
    grad_y = [True] * len(case['ys']) if grad_y is None else grad_y
    x = torch.as_tensor(case['conv5']).to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(grad_x)
    ys = [torch.as_tensor(y).to(DEV).requires_grad_(g) for y, g in zip(case['ys'], grad_y)]
    res = ppm.ppm_pool(x, case['scales'], case['K'])
    cat, ps = res[0], list(res[1:])
    assert len(ps) == len(case['scales']) and all(p.is_contiguous() for p in ps)
    at = cat.data_ptr()
    total = 0.0
    if use_cat:
        out = ppm.ppm_fill(cat, case['C'], *ys)
        assert out.data_ptr() == at and out.shape == cat.shape
        total = total + (torch.as_tensor(case['go']).to(DEV) * out).sum()
    else:
        out = cat
    if use_gp:
        for gp, p in zip(case['gps'], ps):
            total = total + (torch.as_tensor(gp).to(DEV) * p).sum()
    if total.requires_grad:
        total.backward()
    return dict(x=x, pooled=[p.detach() for p in ps], cat=out.detach(), grad_conv5=x.grad, grad_y=[y.grad for y in ys])


def to_numpy(res):
    return dict(pooled=[p.cpu().numpy() for p in res['pooled']], cat=res['cat'].cpu().numpy(), grad_conv5=res['grad_conv5'].cpu().numpy(),
                grad_y=[g.cpu().numpy() for g in res['grad_y']])


_done = {}


def case(name):
    """inputs, float64 truth and the device's answer of a case, computed once and shared (read-only)"""
    if name not in _done:
        c = u.draw_case(name)
        _done[name] = dict(case=c, ref=u.reference(c), res=run_device(c))
    return _done[name]


@pytest.mark.parametrize('name', list(u.CASES))
def test_pool_fill_and_gradients_match_the_float64_reference(gold, poisoned_empty, name):
    _done.pop(name, None)            # this run's buffers start as NaN
    d = case(name)
    c, ref, res = d['case'], d['ref'], d['res']
    C = c['C']
    B, _, h, w = c['conv5'].shape
    assert res['cat'].shape == (B, C + sum(c['K']), h, w) and res['cat'].is_contiguous()
    for p, s in zip(res['pooled'], c['scales']):
        assert p.shape == (B, C, s, s) and p.dtype == torch.float32
    # the pooled tensors are consecutive segments of one buffer
    ptrs = [p.data_ptr() for p in res['pooled']]
    assert all(b - a == 4 * B * C * s * s for a, b, s in zip(ptrs, ptrs[1:], c['scales']))
    # the copy: bit for bit
    assert torch.equal(bits(res['cat'][:, :C]), bits(torch.as_tensor(c['conv5']).to(DEV)))
    # every element is written
    for t in [res['cat'], res['grad_conv5']] + res['pooled'] + res['grad_y']:
        assert t.dtype == torch.float32 and not torch.isnan(t).any()
    assert res['grad_conv5'].shape == res['x'].shape and all(g.shape == y.shape for g, y in zip(res['grad_y'], c['ys']))
    e = u.errors(to_numpy(res), ref, C)
    for q in u.QUANTITIES:
        print('%s %s: device rel 2-norm %.3g, torch fp32 on the CPU %.3g' % (name, q, e[q], float(gold['op32/%s/%s' % (name, q)])))
    for q in u.QUANTITIES:
        assert e[q] <= GATE, (name, q, e[q])


def test_an_identity_upsample_copies_the_branch():
    """s = h = w would be the identity; at 6 x 12 the rows are: every output row takes one input row with weight 1"""
    d = case('even')
    y = torch.as_tensor(d['case']['ys'][3]).to(DEV)                   # [B, 4, 6, 6] to 6 x 12
    got = d['res']['cat'][:, d['case']['C'] + 12:]
    want = F.interpolate(y, size=(6, 12), mode='bilinear', align_corners=False)
    assert torch.equal(got[:, :, :, 0], y[:, :, :, 0])              # column 0 sits on tap 0 with weight 1
    # against torch on the GPU: an ulp of the source position (below 8: 2^-21) between a fused and an unfused evaluation of the
    # rule, times a tap difference of at most the largest value, plus the roundings of the three products and sums
    assert float((got - want).abs().max()) <= (2.0 ** -21 + 2.0 ** -22) * float(want.abs().max())


@pytest.mark.parametrize('name', ['odd', 'wide', 'tiles1'])
def test_two_runs_are_bit_identical(name):
    d = case(name)
    again = run_device(d['case'])
    for k in ('cat', 'grad_conv5'):
        assert torch.equal(bits(again[k]), bits(d['res'][k])), k
    for k in ('pooled', 'grad_y'):
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again[k], d['res'][k])), k


def test_gradients_are_computed_only_where_asked():
    d = case('mixed')
    c, full = d['case'], d['res']
    only_x = run_device(c, grad_x=True, grad_y=[False] * 4)
    assert all(g is None for g in only_x['grad_y']) and torch.equal(bits(only_x['grad_conv5']), bits(full['grad_conv5']))
    only_b2 = run_device(c, grad_x=False, grad_y=[False, False, True, False])
    assert only_b2['grad_conv5'] is None and [g is None for g in only_b2['grad_y']] == [True, True, False, True]
    assert torch.equal(bits(only_b2['grad_y'][2]), bits(full['grad_y'][2]))
    nothing = run_device(c, grad_x=False, grad_y=[False] * 4)
    assert nothing['grad_conv5'] is None and torch.equal(bits(nothing['cat']), bits(full['cat']))


def test_the_pooled_tensors_or_the_concatenation_alone_carry_the_gradient():
    """pool_bwd with no grad_p at all, and with no grad_cat: against float64 with the unused upstream gradient zeroed"""
    d = case('odd')
    c = d['case']
    no_gp = dict(c, gps=[np.zeros_like(g) for g in c['gps']])
    res = run_device(c, use_gp=False)
    e = u.rel(res['grad_conv5'].cpu().numpy(), u.reference(no_gp)['grad_conv5'])
    print('grad_conv5 through cat alone: rel 2-norm %.3g' % e)
    assert e <= GATE and torch.equal(bits(res['grad_conv5']), bits(torch.as_tensor(c['go'][:, :c['C']]).to(DEV)))
    no_go = dict(c, go=np.zeros_like(c['go']))
    res = run_device(c, use_cat=False)
    e = u.rel(res['grad_conv5'].cpu().numpy(), u.reference(no_go)['grad_conv5'])
    print('grad_conv5 through the pooled tensors alone: rel 2-norm %.3g' % e)
    assert e <= GATE and all(g is None for g in res['grad_y'])


def test_a_channels_last_conv5_gives_the_same_bits():
    d = case('odd')
    res = run_device(d['case'], channels_last=True)
    assert not res['x'].is_contiguous()
    assert torch.equal(bits(res['cat']), bits(d['res']['cat'])) and torch.equal(bits(res['grad_conv5']), bits(d['res']['grad_conv5']))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(res['pooled'], d['res']['pooled']))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(res['grad_y'], d['res']['grad_y']))


def test_a_nan_and_an_inf_reach_exactly_the_bins_that_cover_them():
    from semantic import ppm
    c = dict(case('odd')['case'])
    x = c['conv5'].copy()
    x[0, 1, 3, 5] = np.nan
    x[1, 2, 6, 12] = np.inf
    c['conv5'] = x
    res = run_device(c, grad_x=False, grad_y=[False] * 4)
    assert torch.equal(bits(res['cat'][:, :c['C']]), bits(torch.as_tensor(x).to(DEV)))      # the NaN's bits included
    assert torch.isfinite(res['cat'][:, c['C']:]).all()
    h, w = x.shape[2:]
    for p, s in zip(res['pooled'], c['scales']):
        p = p.cpu().numpy()
        want_nan, want_inf = np.zeros(p.shape, bool), np.zeros(p.shape, bool)
        for i, (r0, r1) in enumerate(ppm.ppm_bins(h, s)):
            for j, (c0, c1) in enumerate(ppm.ppm_bins(w, s)):
                want_nan[0, 1, i, j] = r0 <= 3 < r1 and c0 <= 5 < c1
                want_inf[1, 2, i, j] = r0 <= 6 < r1 and c0 <= 12 < c1
        assert want_nan.sum() >= 1 and want_inf.sum() >= 1
        assert np.array_equal(np.isnan(p), want_nan) and np.array_equal(np.isposinf(p), want_inf), s
        assert np.isfinite(p[~want_nan & ~want_inf]).all()


# ---- module level: the stand-in decoder with the fixture's weights -------------------------------------------------------------------
def branch_backend(mode):
    """the batch-norm backend of the caller's branch modules: the default in eval(), torch's native kernels in train() -- the
    module docstring has the figures"""
    return torch.backends.cudnn.flags(enabled=mode != 'train')


def fresh_decoder(gold, mode, **kw):
    torch.manual_seed(u.MOD_SEED[mode])
    dec = u.Decoder(**kw)
    u.load_ppm_state(dec, u.fixture_state(gold))
    return dec.to(DEV).train(mode == 'train')


def gates(gold, mode):
    return {q: (GATE if mode == 'eval' else max(GATE, 4.0 * float(gold['err32/%s/%s' % (mode, q)]))) for q in u.MOD_QUANTITIES}


_truth = {}


def module_truth(gold, mode):
    if mode not in _truth:
        _truth[mode] = u.module_reference(mode, state=u.fixture_state(gold))
        u.check_against_fixture(gold, mode, _truth[mode])
    return _truth[mode]


def compare_module(gold, mode, what, got):
    want, gate = module_truth(gold, mode), gates(gold, mode)
    e = {q: u.rel(got[q], want[q]) for q in u.MOD_QUANTITIES}
    for q in u.MOD_QUANTITIES:
        print('%s %s %s: device rel 2-norm %.3g, torch fp32 on the CPU %.3g, gate %.3g'
              % (mode, what, q, e[q], float(gold['err32/%s/%s' % (mode, q)]), gate[q]))
    for q in u.MOD_QUANTITIES:
        assert e[q] <= gate[q], (mode, what, q, e[q], gate[q])


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_ppm_concat_matches_the_fixture(gold, mode):
    from semantic import ppm
    dec = fresh_decoder(gold, mode)
    conv5, go = u.draw_module_case(mode)
    with branch_backend(mode):
        got = u.module_results(dec, lambda x: ppm.ppm_concat(dec, x), conv5, go)
    assert np.array_equal(got['cat'][:, :u.MOD_FC], conv5.astype(np.float64))
    compare_module(gold, mode, 'ppm_concat', got)


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_the_patched_forward_matches_the_fixture(gold, mode):
    """what reaches conv_last inside the installed forward, taken with a forward pre-hook as the fixture's generator does"""
    from semantic import ppm
    dec = fresh_decoder(gold, mode)
    keys = list(dec.state_dict())
    conv5, go = u.draw_module_case(mode)
    grabbed = []
    hook = dec.conv_last.register_forward_pre_hook(lambda mod, inp: grabbed.append(inp[0]))

    def concat(x):
        out = dec([x])
        assert len(grabbed) == 1 and out.shape == (x.shape[0], u.MOD_CLASSES, u.MOD_H, u.MOD_W)
        return grabbed[0]
    with ppm.use_device_ppm(dec), branch_backend(mode):
        got = u.module_results(dec, concat, conv5, go)
    hook.remove()
    assert 'forward' not in dec.__dict__ and list(dec.state_dict()) == keys
    compare_module(gold, mode, 'patched forward', got)


def test_the_patched_decoder_returns_what_the_unpatched_one_returns(gold):
    """eval(): the use_softmax branch with a segSize, and the deep-supervision pair; the same GPU inputs, the eval() gate"""
    from semantic import ppm
    conv5 = torch.as_tensor(u.draw_module_case('eval')[0]).to(DEV)
    conv4 = torch.randn(1, u.MOD_FC // 2, 2 * u.MOD_H, 2 * u.MOD_W, generator=torch.Generator().manual_seed(5301)).to(DEV)
    with torch.no_grad():
        dec = fresh_decoder(gold, 'eval', use_softmax=True)
        want = dec([conv4, conv5], segSize=(56, 104))
        with ppm.use_device_ppm(dec):
            got = dec([conv4, conv5], segSize=(56, 104))
        assert got.shape == want.shape == (1, u.MOD_CLASSES, 56, 104)
        e = u.rel(got.cpu().numpy(), want.cpu().numpy())
        print('use_softmax at (56, 104): patched against unpatched rel 2-norm %.3g' % e)
        assert e <= GATE
        dec = fresh_decoder(gold, 'eval', deepsup=True)
        want = dec([conv4, conv5])
        with ppm.use_device_ppm(dec):
            got = dec([conv4, conv5])
        assert isinstance(got, tuple) and len(got) == len(want) == 2 and got[0].shape == want[0].shape
        e = u.rel(got[0].cpu().numpy(), want[0].cpu().numpy())
        print('deepsup pair: main head patched against unpatched rel 2-norm %.3g' % e)
        assert e <= GATE and u.rel(got[1].cpu().numpy(), want[1].cpu().numpy()) <= GATE


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv4, self.conv5 = nn.Conv2d(3, 8, 1), nn.Conv2d(3, 16, 1)

    def forward(self, x, return_feature_maps=False):
        # conv4 and conv5 share their size, as in the reference's dilated encoders
        return [F.avg_pool2d(torch.tanh(self.conv4(x)), 8), F.avg_pool2d(torch.tanh(self.conv5(x)), 8)]


class _Module(nn.Module):
    """stands in for SegmentationModule: the same attributes and call forms (the precedent: tests/test_gpu_segm_loss.py)"""

    def __init__(self):
        super().__init__()
        self.encoder, self.decoder = _Encoder(), u.Decoder(branch=4, deepsup=True)
        self.crit = nn.NLLLoss(ignore_index=-1)
        self.deep_sup_scale = 0.4

    def forward(self, feed_dict, *, segSize=None):
        feats = self.encoder(feed_dict['img_data'], return_feature_maps=True)
        if segSize is not None:
            pred = self.decoder(feats, segSize=segSize)
            return pred[0] if isinstance(pred, tuple) else pred
        pred, pred_deepsup = self.decoder(feats)
        loss = self.crit(pred, feed_dict['seg_label']) + self.crit(pred_deepsup, feed_dict['seg_label']) * self.deep_sup_scale
        return loss, loss.detach()


def test_predict_and_train_forward_run_through_a_patched_decoder():
    from semantic import ppm, segm_tail, train_loss
    torch.manual_seed(5302)
    m = _Module().to(DEV).eval()
    patched = copy.deepcopy(m)
    handle = ppm.use_device_ppm(patched.decoder)
    g = torch.Generator().manual_seed(5303)
    img = torch.randn(2, 3, 56, 104, generator=g).to(DEV)
    feed = {'img_data': img, 'seg_label': torch.randint(-1, u.MOD_CLASSES, (2, 7, 13), generator=g).to(DEV)}
    res = {}
    for name, mod in (('plain', m), ('patched', patched)):
        loss, acc = train_loss.train_forward(mod, feed)
        loss.backward()
        labels, probs = segm_tail.predict(mod, [img, img[:, :, ::2, ::2].contiguous()], (56, 104), return_probs=True)
        res[name] = dict(loss=float(loss.detach()), gw=mod.decoder.ppm[3][1].weight.grad.cpu().numpy(), ge=mod.encoder.conv5.weight.grad.cpu().numpy(),
                         labels=labels.cpu().numpy(), probs=probs.cpu().numpy())
        assert not mod.decoder.conv_last._forward_hooks
    a, b = res['plain'], res['patched']
    e = {'loss': abs(a['loss'] - b['loss']) / abs(a['loss']), 'grad ppm[3] weight': u.rel(b['gw'], a['gw']),
         'grad encoder weight': u.rel(b['ge'], a['ge']), 'probs': u.rel(b['probs'], a['probs'])}
    for k, v in e.items():
        print('patched against unpatched, %s: rel %.3g' % (k, v))
    assert all(v <= GATE for v in e.values()), e
    assert b['labels'].shape == (2, 1, 56, 104) and b['labels'].dtype == np.uint8
    top = np.sort(a['probs'], axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-5                      # away from a tie the label cannot change
    assert clear.mean() > 0.99 and np.array_equal(a['labels'][:, 0][clear], b['labels'][:, 0][clear])
    handle.remove()
    assert 'forward' not in patched.decoder.__dict__
