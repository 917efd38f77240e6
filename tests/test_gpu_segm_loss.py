"""semantic.train_loss (sdn_segm_loss_fwd / _bwd, csrc/segm_loss.hip) against the reference's expressions in float64 on the CPU
(tests/segm_loss_util.py: semantic/models.py:15-21, 39-44, the decoders' log_softmax, nn.NLLLoss(ignore_index=-1)), which the
fixture tests/golden/segm_loss_golden.npz pins to the reference's own pixel_acc and torch's NLLLoss
(tests/golden/make_segm_loss_golden.py).

The numeric gate is the sibling loss's (tests/test_gpu_train_losses.py, GATE = 1e-6): every finite loss within 1e-6 relative of
the float64 value, every gradient within 1e-6 of the float64 gradient in relative 2-norm; torch's own fp32 CPU run sits at 2e-9
to 4e-8 (losses) and 7e-8 to 1e-7 (gradients) on these cases.  The integers, acc, the NaN of an all-ignored batch, every zero
and the run-to-run bits are exact."""
import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import segm_loss_util as u

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-6
LOSSES = ('loss', 'loss_main', 'loss_deepsup')


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


def val(t):
    return float(t.detach())


def total_of(res):
    return sum(u.WEIGHTS[k] * res[k] for k in ('loss', 'acc', 'loss_main', 'loss_deepsup'))


def run_device(scores, deep, label, scale=u.SCALE, grad=(True, True)):
    """(the dict of segm_losses, gradient of the main head's scores, of the deepsup head's) for sum(w_k out_k)"""
    from semantic import train_loss
    s0 = torch.as_tensor(scores).to(DEV).requires_grad_(grad[0])
    s1 = torch.as_tensor(deep).to(DEV).requires_grad_(grad[1]) if deep is not None else None
    res = train_loss.segm_losses(s0, torch.as_tensor(label).to(DEV), s1, scale if deep is not None else None)
    total_of(res).backward()
    return res, s0.grad, (s1.grad if s1 is not None else None)


_done = {}


def case(name):
    """inputs, float64 truth and the device's answer of a fixture case, computed once and shared (read-only)"""
    if name not in _done:
        scores, deep, label = u.draw_case(name)
        ref = u.reference(scores, deep, label)
        res, g0, g1 = run_device(scores, deep, label)
        _done[name] = dict(scores=scores, deep=deep, label=label, ref=ref, res=res, g0=g0, g1=g1)
    return _done[name]


def compare(what, res, g0, g1, ref, label):
    """prints every figure, then asserts the gate and the exact expectations"""
    C_valid = (torch.as_tensor(label) >= 0) & (torch.as_tensor(label) < ref['grad'].shape[1])
    for k in LOSSES:
        got, want = val(res[k]), ref[k]
        print('%s %s: device %.9g fp64 %.12g rel %.3g' % (what, k, got, want, abs(got - want) / abs(want) if want else abs(got)))
    rels = {}
    for k, g, rg in (('grad', g0, ref['grad']), ('grad_deepsup', g1, ref['grad_deepsup'])):
        if rg is not None and np.linalg.norm(rg) > 0:
            rels[k] = float(np.linalg.norm(g.cpu().double().numpy() - rg) / np.linalg.norm(rg))
            print('%s %s: rel 2-norm %.3g' % (what, k, rels[k]))
    for k in LOSSES:
        got, want = val(res[k]), ref[k]
        assert res[k].dim() == 0 and res[k].dtype == torch.float32
        if np.isnan(want):
            assert np.isnan(got), (what, k, got)
        else:
            assert abs(got - want) <= GATE * abs(want), (what, k, got, want)
    for k in ('acc_sum', 'pixel_sum', 'bad'):
        assert res[k].dim() == 0 and res[k].dtype == torch.int64 and int(res[k]) == ref[k], (what, k, int(res[k]), ref[k])
    assert res['acc'].detach().cpu().numpy().tobytes() == u.acc_fp32(ref['acc_sum'], ref['pixel_sum']).tobytes() == ref['acc'].tobytes(), what
    for k, g, rg in (('grad', g0, ref['grad']), ('grad_deepsup', g1, ref['grad_deepsup'])):
        if rg is None:
            assert g is None, (what, k)
            continue
        assert g.shape == rg.shape and g.dtype == torch.float32 and not torch.isnan(g).any(), (what, k)
        # ignored pixels: exact zeros, written by the kernel
        assert not g.cpu().permute(0, 2, 3, 1)[~C_valid].any(), (what, k)
        if k in rels:
            assert rels[k] <= GATE, (what, k, rels[k])
        else:
            assert not g.any(), (what, k)


def check_against_fixture(gold, name, ref):
    """the float64 values the device is held against are the fixture's"""
    p = name + '/'
    for k in LOSSES:
        want = float(gold[p + k])
        assert (np.isnan(want) and np.isnan(ref[k])) or abs(ref[k] - want) <= 1e-13 * abs(want), (name, k)
    for k in ('acc_sum', 'pixel_sum', 'bad'):
        assert ref[k] == int(gold[p + k])
    assert ref['acc'].tobytes() == gold[p + 'acc'].tobytes()
    for k in ('grad', 'grad_deepsup'):
        if ref[k] is None:
            continue
        if name in u.STORED_WHOLE:
            assert np.allclose(ref[k], gold[p + k], rtol=1e-12, atol=1e-18)
        else:
            assert np.allclose(ref[k].reshape(-1)[::u.SAMPLE_STRIDE], gold[p + k + '_sample'], rtol=1e-12, atol=1e-18)
            assert abs(np.linalg.norm(ref[k]) - float(gold[p + k + '_norm'])) <= 1e-12 * float(gold[p + k + '_norm'])


@pytest.mark.parametrize('name', list(u.CASES))
def test_losses_counts_and_gradients_match_the_float64_reference(gold, poisoned_empty, name):
    _done.pop(name, None)            # this run's buffers start as NaN / 99
    c = case(name)
    check_against_fixture(gold, name, c['ref'])
    res = c['res']
    assert list(res) == ['loss', 'acc', 'loss_main', 'loss_deepsup', 'acc_sum', 'pixel_sum', 'bad']
    # views of one [4] and one [3] tensor
    assert all(res[k]._base is res['loss']._base and res['loss']._base.shape == (4,) for k in ('acc',) + LOSSES)
    assert all(res[k]._base is res['bad']._base and res['bad']._base.shape == (3,) for k in ('acc_sum', 'pixel_sum'))
    assert not res['bad']._base.requires_grad and res['loss'].requires_grad
    compare(name, res, c['g0'], c['g1'], c['ref'], c['label'])


def test_an_all_ignored_batch_gives_nan_zero_accuracy_and_zero_gradients():
    c = case('ignored')
    assert all(np.isnan(val(c['res'][k])) for k in LOSSES)
    assert val(c['res']['acc']) == 0.0 and int(c['res']['pixel_sum']) == 0 and int(c['res']['acc_sum']) == 0
    assert not c['g0'].any() and not c['g1'].any() and not torch.isnan(c['g0']).any() and not torch.isnan(c['g1']).any()


def test_one_class_gives_exact_zeros():
    c = case('c1')
    assert all(val(c['res'][k]) == 0.0 for k in LOSSES) and val(c['res']['acc']) == 1.0
    assert not c['g0'].any() and not c['g1'].any()


def test_without_the_deepsup_head_the_loss_is_the_main_loss():
    a, b = case('blocks'), case('blocks_nodeep')
    assert torch.equal(b['res']['loss'], b['res']['loss_main']) and val(b['res']['loss_deepsup']) == 0.0
    assert torch.equal(a['res']['loss_main'], b['res']['loss_main']) and torch.equal(a['res']['acc'], b['res']['acc'])
    assert b['g1'] is None and int(b['res']['bad']) == int(a['res']['bad']) > 0
    # d total / d scores: 0.7 + 1.3 on the main head in both variants
    assert torch.equal(a['g0'], b['g0'])


@pytest.mark.parametrize('name', ['blocks', 'maxc'])
def test_two_runs_are_bit_identical(name):
    c = case(name)
    res, g0, g1 = run_device(c['scores'], c['deep'], c['label'])
    for k in c['res']:
        assert torch.equal(res[k], c['res'][k]), k
    assert torch.equal(g0, c['g0']) and torch.equal(g1, c['g1'])


def test_a_head_without_gradient_leaves_the_other():
    c = case('blocks')
    res, g0, g1 = run_device(c['scores'], c['deep'], c['label'], grad=(True, False))
    assert g1 is None and torch.equal(g0, c['g0']) and torch.equal(res['loss'], c['res']['loss'])
    res, g0, g1 = run_device(c['scores'], c['deep'], c['label'], grad=(False, True))
    assert g0 is None and torch.equal(g1, c['g1'])


def test_the_gradient_slots_and_the_scale_are_where_they_belong():
    """each output alone: loss reaches both heads (the deepsup head times the scale), loss_main and loss_deepsup one head each,
    acc none"""
    from semantic import train_loss
    c = case('small')
    lab = torch.as_tensor(c['label']).to(DEV)
    grads = {}
    for k in ('loss', 'acc', 'loss_main', 'loss_deepsup'):
        s0 = torch.as_tensor(c['scores']).to(DEV).requires_grad_()
        s1 = torch.as_tensor(c['deep']).to(DEV).requires_grad_()
        train_loss.segm_losses(s0, lab, s1, 0.25)[k].backward()
        grads[k] = (s0.grad, s1.grad)
    assert not grads['acc'][0].any() and not grads['acc'][1].any()
    assert grads['loss_main'][0].any() and not grads['loss_main'][1].any()
    assert not grads['loss_deepsup'][0].any() and grads['loss_deepsup'][1].any()
    assert torch.equal(grads['loss'][0], grads['loss_main'][0])
    assert torch.equal(grads['loss'][1], grads['loss_deepsup'][1] * 0.25)   # 0.25: the product is exact


def test_non_contiguous_scores_give_the_same_numbers():
    from semantic import train_loss
    c = case('blocks')
    B, C, h, w = c['scores'].shape
    wide = torch.zeros(B, C, h, w + 5, device=DEV)
    wide[..., 2:w + 2] = torch.as_tensor(c['scores']).to(DEV)
    wide.requires_grad_()
    view = wide[..., 2:w + 2]
    assert not view.is_contiguous()
    s1 = torch.as_tensor(c['deep']).to(DEV).requires_grad_()
    res = train_loss.segm_losses(view, torch.as_tensor(c['label']).to(DEV), s1, u.SCALE)
    total_of(res).backward()
    for k in c['res']:
        assert torch.equal(res[k], c['res'][k]), k
    assert torch.equal(wide.grad[..., 2:w + 2], c['g0']) and not wide.grad[..., :2].any() and not wide.grad[..., w + 2:].any()


# ---- the C entry points on guarded buffers -------------------------------------------------------------------------------------------
CANARY = -12345.0
PAD = 64   # elements on either side: the guarded part stays 256-byte aligned


def guarded(n, dtype, canary):
    buf = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
    buf[PAD:PAD + n] = float('nan') if dtype.is_floating_point else 99
    return buf, buf[PAD:PAD + n]


def borders_intact(buf, canary):
    return bool((buf[:PAD] == canary).all()) and bool((buf[-PAD:] == canary).all())


@pytest.mark.parametrize('name,shift', [('blocks', 0), ('blocks', 1), ('maxc', 0), ('small', 0)])
def test_nothing_is_written_outside_the_outputs(name, shift):
    """out, counts, lse and both gradients inside canary borders, the outputs NaN / 99 before the call.  shift 1 moves both score
    tensors off their 16-byte alignment: the same case (h w % 4 == 0) then takes the scalar path."""
    import sdn_hip
    from sdn_hip import ops
    c = case(name)
    B, C, h, w = c['scores'].shape
    n = B * C * h * w
    L = sdn_hip.lib()
    hold = [torch.zeros(n + 4, device=DEV) for _ in range(2)]
    s0, s1 = hold[0][shift:shift + n], hold[1][shift:shift + n]
    s0.copy_(torch.as_tensor(c['scores']).reshape(-1))
    s1.copy_(torch.as_tensor(c['deep']).reshape(-1))
    assert (s0.data_ptr() % 16 == 0) == (shift == 0)
    lab = torch.as_tensor(c['label']).to(DEV)
    nblk = B * (-(-h * w // ops.SEGM_LOSS_PIXELS))
    scratch_buf, scratch = guarded(nblk * ops.SEGM_LOSS_PART_BYTES, torch.uint8, 0xA5)
    lse_buf, lse = guarded(2 * B * h * w, torch.float32, CANARY)
    out_buf, out = guarded(4, torch.float32, CANARY)
    cnt_buf, cnt = guarded(3, torch.int64, -777)
    g0_buf, g0 = guarded(n, torch.float32, CANARY)
    g1_buf, g1 = guarded(n, torch.float32, CANARY)
    p = lambda t: t.data_ptr()
    rc = L.sdn_segm_loss_fwd(p(s0), p(s1), p(lab), B, C, h, w, u.SCALE, p(scratch), scratch.numel(), p(lse), p(out), p(cnt), sdn_hip.stream())
    assert rc == 0, L.sdn_last_error()
    gout = torch.tensor([u.WEIGHTS[k] for k in ('loss', 'acc', 'loss_main', 'loss_deepsup')], dtype=torch.float32, device=DEV)
    rc = L.sdn_segm_loss_bwd(p(s0), p(s1), p(lab), B, C, h, w, u.SCALE, p(lse), p(cnt), p(gout), p(g0), p(g1), sdn_hip.stream())
    assert rc == 0, L.sdn_last_error()
    torch.cuda.synchronize()
    assert borders_intact(scratch_buf, 0xA5) and borders_intact(lse_buf, CANARY) and borders_intact(out_buf, CANARY)
    assert borders_intact(cnt_buf, -777) and borders_intact(g0_buf, CANARY) and borders_intact(g1_buf, CANARY)
    assert not torch.isnan(lse).any() and not torch.isnan(g0).any() and not torch.isnan(g1).any() and not torch.isnan(out).any()
    # the same numbers as through the binding; per element the two load paths run the same operations
    res = c['res']
    assert [int(v) for v in cnt] == [int(res['acc_sum']), int(res['pixel_sum']), int(res['bad'])]
    assert torch.equal(g0.view(B, C, h, w), c['g0']) and torch.equal(g1.view(B, C, h, w), c['g1'])
    assert out[1] == res['acc']
    for i, k in ((0, 'loss'), (2, 'loss_main'), (3, 'loss_deepsup')):
        if shift == 0:
            assert out[i] == res[k], k
        else:   # another order of the fp64 partial sums
            assert abs(val(out[i]) - c['ref'][k]) <= GATE * abs(c['ref'][k]), k


def test_the_workload_size():
    """(2, 14, 48, 156): the reference's default classes at 1 / 8 of its default crop; drawn here, checked against the same
    float64 expressions"""
    rs = np.random.RandomState(4201)
    shape = (2, 14, 48, 156)
    scores, deep = u.draw_scores(rs, shape), u.draw_scores(rs, shape)
    label = rs.randint(-1, 14, (2, 48, 156)).astype(np.int64)
    label = np.where(rs.rand(2, 48, 156) < 0.6, scores.argmax(axis=1), label)
    label[1, 40:, :] = -1     # the padding of the smaller item
    ref = u.reference(scores, deep, label)
    res, g0, g1 = run_device(scores, deep, label)
    compare('workload', res, g0, g1, ref, label)
    assert int(res['bad']) == 0 and 0 < int(res['acc_sum']) < int(res['pixel_sum']) < label.size


def strict_argmax(x):
    """the device's rule on one pixel's scores: a scan from class 0 with a strict >"""
    best, top = 0, x[0]
    for c in range(1, len(x)):
        if x[c] > top:
            best, top = c, x[c]
    return best


def test_a_nan_score_makes_the_loss_nan_and_never_wins_the_prediction():
    """Differs from torch.max, which returns the NaN's class: documented in semantic.train_loss.segm_losses"""
    c = case('small')
    scores, label = c['scores'].copy(), c['label'].copy()
    scores[0, 3, 2, 4] = np.nan          # a NaN in class 3: the best of the others wins
    scores[1, 0, 1, 1] = np.nan          # a NaN in class 0: nothing is greater than NaN, class 0 stays
    want_a, want_b = strict_argmax(scores[0, :, 2, 4]), strict_argmax(scores[1, :, 1, 1])
    assert want_a not in (0, 3) and want_b == 0
    label[0, 2, 4], label[1, 1, 1] = want_a, want_b      # both pixels valid, both hits under the strict rule
    preds = np.stack([[[strict_argmax(scores[b, :, y, x]) for x in range(7)] for y in range(5)] for b in range(2)])
    valid = label >= 0
    res, g0, _ = run_device(scores, c['deep'], label)
    assert np.isnan(val(res['loss'])) and np.isnan(val(res['loss_main'])) and np.isfinite(val(res['loss_deepsup']))
    assert int(res['pixel_sum']) == int(valid.sum()) and int(res['acc_sum']) == int((valid & (preds == label)).sum())
    t_preds = torch.max(torch.as_tensor(scores), dim=1)[1].numpy()
    assert t_preds[0, 2, 4] == 3 and int((valid & (t_preds == label)).sum()) == int(res['acc_sum']) - 1
    # the NaN stays in its pixel's gradient
    nan_px = torch.isnan(g0).any(dim=1).cpu().numpy()
    assert nan_px[0, 2, 4] and nan_px[1, 1, 1] and int(nan_px.sum()) == 2


# ---- train_forward ------------------------------------------------------------------------------------------------------------------
class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, 1)

    def forward(self, x, return_feature_maps=False):
        return [F.avg_pool2d(torch.tanh(self.conv(x)), 8)]


class _Decoder(nn.Module):
    """1 x 1 heads, no dropout, log_softmax as the reference's decoders return it in training"""

    def __init__(self, deepsup=True, twice=False):
        super().__init__()
        self.conv_last = nn.Conv2d(8, 14, 1)
        if deepsup:
            self.conv_last_deepsup = nn.Conv2d(8, 14, 1)
        self.twice = twice

    def forward(self, conv_out, segSize=None):
        x = self.conv_last(conv_out[-1])
        if self.twice:
            x = x + self.conv_last(conv_out[-1])
        x = F.log_softmax(x, dim=1)
        if hasattr(self, 'conv_last_deepsup'):
            return x, F.log_softmax(self.conv_last_deepsup(conv_out[-1]), dim=1)
        return x


class _Module(nn.Module):
    """stands in for SegmentationModule: the same attributes, the same return value in training"""

    def __init__(self, deep_sup_scale, **kw):
        super().__init__()
        self.encoder, self.decoder = _Encoder(), _Decoder(**kw)
        self.crit = nn.NLLLoss(ignore_index=-1)
        self.deep_sup_scale = deep_sup_scale

    def forward(self, feed_dict, *, segSize=None):
        pred = self.decoder(self.encoder(feed_dict['img_data'], return_feature_maps=self.deep_sup_scale is not None))
        if self.deep_sup_scale is not None:
            pred, pred_deepsup = pred
        elif isinstance(pred, tuple):
            pred = pred[0]
        loss = self.crit(pred, feed_dict['seg_label'])
        if self.deep_sup_scale is not None:
            loss = loss + self.crit(pred_deepsup, feed_dict['seg_label']) * self.deep_sup_scale
        return loss, loss.detach()


@pytest.mark.parametrize('scale', [0.4, None])
def test_train_forward_equals_segm_losses_on_the_hooked_scores(scale):
    from semantic import train_loss
    torch.manual_seed(7)
    m = _Module(scale).to(DEV).train()
    feed = {'img_data': torch.randn(2, 3, 40, 56, device=DEV), 'seg_label': torch.as_tensor(case('small')['label']).to(DEV)}
    loss, acc = train_loss.train_forward(m, feed)
    assert loss.dim() == 0 and acc.dim() == 0 and loss.requires_grad
    loss.backward()
    got = {k: (p.grad.clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    assert not m.decoder.conv_last._forward_hooks          # the hooks are gone
    m.zero_grad()
    feat = m.encoder(feed['img_data'], return_feature_maps=True)
    s = m.decoder.conv_last(feat[-1])
    sd = m.decoder.conv_last_deepsup(feat[-1]) if scale is not None else None
    res = train_loss.segm_losses(s, feed['seg_label'], sd, scale)
    assert torch.equal(loss, res['loss']) and torch.equal(acc, res['acc'])
    res['loss'].backward()
    for k, p in m.named_parameters():
        if scale is None and 'deepsup' in k:
            assert got[k] is None or not got[k].any()
            continue
        rel = float((got[k] - p.grad).norm() / p.grad.norm())
        print('train_forward d/d%s: rel 2-norm against the explicit graph %.3g' % (k, rel))
        assert rel <= GATE, (k, rel)
    # and the loss is the float64 one of the same scores
    ref = u.reference(s.detach().cpu().numpy(), sd.detach().cpu().numpy() if sd is not None else None, feed['seg_label'].cpu().numpy(),
                      scale=scale if scale is not None else 0.0)
    assert abs(val(loss) - ref['loss']) <= GATE * abs(ref['loss'])


def test_train_forward_refuses_what_it_cannot_hook():
    from semantic import train_loss
    feed = {'img_data': torch.randn(2, 3, 40, 56, device=DEV), 'seg_label': torch.as_tensor(case('small')['label']).to(DEV)}
    m = _Module(0.4, deepsup=False).to(DEV)
    with pytest.raises(ValueError, match='conv_last_deepsup not found'):
        train_loss.train_forward(m, feed)
    assert not m.decoder.conv_last._forward_hooks
    m = _Module(None, deepsup=False, twice=True).to(DEV)
    with pytest.raises(RuntimeError, match='ran 2 times'):
        train_loss.train_forward(m, feed)
    assert not m.decoder.conv_last._forward_hooks


def test_the_labels_of_segm_train_batch_go_in_as_they_are():
    import segm_train_util as tu
    from semantic import train_items, train_loss
    frames, scenes, tables = tu.small_inputs()
    flips, jitters = tu.small_case(20, False)
    cfg = tu.SMALL
    batch = train_items.segm_train_batch(torch.from_numpy(frames).to(DEV), torch.from_numpy(scenes).to(DEV), tables, 20, flips, jitters,
                                         cfg['img_max_size'], cfg['padding_constant'], cfg['segm_downsampling_rate'], cfg['frame_size'])
    lab = batch['seg_label']
    assert lab.dtype == torch.int64 and lab.is_contiguous() and tuple(lab.shape) == (3, 3, 9)
    rs = np.random.RandomState(4301)
    scores = u.draw_scores(rs, (3, 14, 3, 9))
    s0 = torch.as_tensor(scores).to(DEV).requires_grad_()
    res = train_loss.segm_losses(s0, lab)
    fn = res['loss'].grad_fn.next_functions[0][0]            # the select's input: SegmLossFn's node
    saved = [t for t in fn.saved_tensors if t is not None and t.dtype == torch.int64 and t.dim() == 3]
    assert len(saved) == 1 and saved[0].data_ptr() == lab.data_ptr()          # no cast, no copy
    ref = u.reference(scores, None, lab.cpu().numpy(), scale=0.0)
    assert ref['pixel_sum'] > 0 and abs(val(res['loss']) - ref['loss']) <= GATE * abs(ref['loss'])
    assert [int(res[k]) for k in ('acc_sum', 'pixel_sum', 'bad')] == [ref['acc_sum'], ref['pixel_sum'], ref['bad']]
