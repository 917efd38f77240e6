"""maskrcnn.losses (sdn_mrcnn_loss_fwd / _bwd, csrc/mrcnn_loss.hip) against the reference's compute_losses in float64: the
fixture tests/golden/mrcnn_loss_golden.npz holds what the reference's own functions gave (tests/golden/make_mrcnn_loss_golden.py),
tests/mrcnn_loss_util.py restates them in numpy for the inputs the fixture does not cover.

The numeric gate is the sibling loss's (tests/test_gpu_segm_loss.py, 1e-6 of the float64 run): absolute for the six losses; for
the gradients per element, relative to max(|ref|, 1 / n) with n the element count of that loss's mean, so that the saturated
binary-cross-entropy elements (about 1e12 / n) do not set the scale for the rest.  torch's own float32 CPU run sits at 7e-8 to
3e-7 in that measure on the fixture's cases (the fixture records it per case, with the gate).  The counts, the NaN of an empty
selection, every zero outside a selection and the run-to-run bits are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mrcnn_loss_util as u
from maskrcnn import losses   # the feature itself: without it this module does not import

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


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
    return sum(w * res[k] for w, k in zip(u.WEIGHTS, u.LOSSES))


def device_inputs(c, grad=(True,) * 5):
    t = {k: torch.as_tensor(c[k]).to(DEV) for k in u.INPUTS}
    for k, g in zip(u.PREDICTIONS, grad):
        if g and t[k].numel():
            t[k].requires_grad_()
    return t


def run_device(c, grad=(True,) * 5):
    """(the dict of mrcnn_losses, {prediction: gradient of sum(w_k out_k) or None})"""
    t = device_inputs(c, grad)
    res = losses.mrcnn_losses(*[t[k] for k in u.INPUTS])
    if any(t[k].requires_grad for k in u.PREDICTIONS):
        total_of(res).backward()
    return res, {k: t[k].grad for k in u.PREDICTIONS}


_done = {}


def case(name):
    """inputs, float64 truth and the device's answer of a fixture case, computed once and shared (read-only)"""
    if name not in _done:
        c = u.draw_case(name)
        res, grads = run_device(c)
        _done[name] = dict(c=c, ref=u.reference(c), res=res, grads=grads)
    return _done[name]


def compare(what, res, grads, ref, gate=u.GATE):
    """prints every figure, then asserts the gate and the exact expectations"""
    for k in u.LOSSES:
        print('%s %s: device %.9g fp64 %.12g abs %.3g' % (what, k, val(res[k]), ref[k], abs(val(res[k]) - ref[k])))
    errs = {}
    for k in u.PREDICTIONS:
        if ref['grad'][k] is not None and grads[k] is not None:
            errs[k] = u.grad_error(grads[k].cpu().numpy(), ref['grad'][k], ref['n'][k])
            print('%s d %s: worst element %.3g of max(|ref|, 1 / %d)' % (what, k, errs[k], ref['n'][k]))
    for k in u.LOSSES:
        got, want = val(res[k]), ref[k]
        assert res[k].dim() == 0 and res[k].dtype == torch.float32
        if np.isnan(want):
            assert np.isnan(got), (what, k, got)
        else:
            assert abs(got - want) <= gate, (what, k, got, want)
    for k in u.COUNTS:
        assert res[k].dim() == 0 and res[k].dtype == torch.int64 and int(res[k]) == ref[k], (what, k, int(res[k]), ref[k])
    for k in u.PREDICTIONS:
        g, rg = grads[k], ref['grad'][k]
        if rg is None or g is None:
            assert g is None, (what, k)
            continue
        assert g.shape == rg.shape and g.dtype == torch.float32 and not torch.isnan(g).any(), (what, k)
        # outside the selection: +0.0, written by the kernel
        outside = g.cpu()[torch.as_tensor(~ref['selected'][k])]
        assert not outside.any() and not torch.signbit(outside).any(), (what, k)
        assert errs[k] <= gate, (what, k, errs[k])


@pytest.mark.parametrize('name', list(u.CASES))
def test_losses_counts_and_gradients_match_the_references_float64_run(gold, poisoned_empty, name):
    _done.pop(name, None)            # this run's buffers start as NaN / 99
    c = case(name)
    p = name + '/'
    ref, res = c['ref'], c['res']
    # the float64 values the device is held against are the fixture's
    for k in u.LOSSES:
        want = float(gold[p + k])
        assert (np.isnan(want) and np.isnan(ref[k])) or abs(ref[k] - want) <= 1e-13 * max(abs(want), 1.0), (name, k)
    for k in u.COUNTS:
        assert ref[k] == int(gold[p + k])
    for k in u.PREDICTIONS:
        if ref['grad'][k] is not None:
            want = u.dense(gold[p + 'grad_idx_' + k], gold[p + 'grad_val_' + k], ref['grad'][k].shape)
            assert np.allclose(ref['grad'][k], want, rtol=1e-11, atol=1e-300), (name, k)
    assert list(res) == list(u.LOSSES) + list(u.COUNTS)
    # views of one [6] and one [4] tensor
    assert all(res[k]._base is res['loss']._base and res['loss']._base.shape == (6,) for k in u.LOSSES)
    assert all(res[k]._base is res['bad']._base and res['bad']._base.shape == (4,) for k in u.COUNTS)
    assert not res['bad']._base.requires_grad and res['loss'].requires_grad
    compare(name, res, c['grads'], ref, float(gold[p + 'gate']))


def test_empty_selections_give_nan_and_exact_zero_gradients():
    c = case('novalid')
    res, g = c['res'], c['grads']
    assert all(np.isnan(val(res[k])) for k in ('rpn_class_loss', 'rpn_bbox_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss', 'loss'))
    assert np.isfinite(val(res['mrcnn_class_loss'])) and g['mrcnn_class_logits'].any()
    for k in ('rpn_class_logits', 'rpn_pred_bbox', 'mrcnn_bbox', 'mrcnn_mask'):
        assert not g[k].any() and not torch.isnan(g[k]).any(), k
    c = case('nopos')
    assert np.isnan(val(c['res']['rpn_bbox_loss'])) and not c['grads']['rpn_pred_bbox'].any() and c['grads']['rpn_class_logits'].any()


@pytest.mark.parametrize('name', ['chunks', 'exact', 'nopos'])
def test_two_runs_are_bit_identical(name):
    c = case(name)
    res, grads = run_device(c['c'])
    for k in c['res']:
        assert torch.equal(res[k], c['res'][k]) or (np.isnan(val(res[k])) and np.isnan(val(c['res'][k]))), k
    for k in u.PREDICTIONS:
        assert torch.equal(grads[k], c['grads'][k]), k


def test_no_roi_gives_zero_head_losses_and_leaves_the_rpn_alone():
    """R = 0, also as the tensors predict(..., mode='training') returns when no RoI was sampled (model.py:1803-1812)"""
    e = case('empty')
    assert [val(e['res'][k]) for k in u.LOSSES[2:5]] == [0.0, 0.0, 0.0] and int(e['res']['n_roi_pos']) == 0
    assert all(e['grads'][k] is None for k in u.PREDICTIONS[2:]) and e['grads']['rpn_pred_bbox'].any()
    # the RPN half of `chunks` with predict's empty tensors: the same RPN losses and gradients, bit for bit
    full = case('chunks')
    t = device_inputs(full['c'])
    heads = [torch.IntTensor().to(DEV), torch.FloatTensor().to(DEV), torch.FloatTensor().to(DEV), torch.FloatTensor().to(DEV),
             torch.FloatTensor().to(DEV), torch.FloatTensor().to(DEV)]
    heads[1].requires_grad_()
    res = losses.mrcnn_losses(*([t[k] for k in u.INPUTS[:4]] + heads))
    total_of(res).backward()
    for k in ('rpn_class_loss', 'rpn_bbox_loss', 'n_rpn_valid', 'n_rpn_pos'):
        assert torch.equal(res[k], full['res'][k]), k
    assert [val(res[k]) for k in u.LOSSES[2:5]] == [0.0, 0.0, 0.0] and int(res['bad']) == 0
    assert abs(val(res['loss']) - (full['ref']['rpn_class_loss'] + full['ref']['rpn_bbox_loss'])) <= u.GATE
    for k in u.PREDICTIONS[:2]:
        assert torch.equal(t[k].grad, full['grads'][k]), k
    assert heads[1].grad is None
    out = losses.compute_losses(*([t[k] for k in u.INPUTS[:4]] + heads))
    assert len(out) == 5 and val(sum(out)) == val(out[0] + out[1])


def test_an_input_without_gradient_leaves_the_others():
    c = case('chunks')
    for grad in ((False, True, False, False, True), (False, False, True, False, False), (True, False, False, True, False)):
        res, grads = run_device(c['c'], grad)
        assert torch.equal(res['loss'], c['res']['loss'])
        for k, g in zip(u.PREDICTIONS, grad):
            assert (grads[k] is None) if not g else torch.equal(grads[k], c['grads'][k]), (grad, k)
    res, grads = run_device(c['c'], (False,) * 5)
    assert not res['loss'].requires_grad and torch.equal(res['loss'], c['res']['loss'])


def test_the_gradient_slots_are_where_they_belong():
    """each output alone reaches its own input; `loss` reaches all five with weight one"""
    c = case('chunks')
    alone = {}
    for k in u.LOSSES:
        t = device_inputs(c['c'])
        losses.mrcnn_losses(*[t[i] for i in u.INPUTS])[k].backward()
        alone[k] = {p: t[p].grad for p in u.PREDICTIONS}
    for k, own in zip(u.LOSSES[:5], u.PREDICTIONS):
        for p in u.PREDICTIONS:
            assert alone[k][p].any() == (p == own), (k, p)
        assert torch.equal(alone['loss'][own], alone[k][own]), k


def test_what_the_reference_leaves_undefined_is_left_out_and_counted():
    c = case('chunks')['c']
    d = {k: v.copy() for k, v in c.items()}
    d['rpn_match'][0, 10, 0], d['rpn_match'][0, 2000, 0] = 2, -7
    res, grads = run_device(d)
    ref = u.reference(d)
    assert int(res['bad']) == 2 == ref['bad']
    compare('bad match', res, grads, ref)
    d = {k: v.copy() for k, v in c.items()}
    d['rpn_bbox'] = np.ascontiguousarray(c['rpn_bbox'][:, :10])
    res, grads = run_device(d)
    ref = u.reference(d)
    assert int(res['n_rpn_pos']) == 10 and int(res['bad']) == ref['bad'] > 0 and int(res['n_rpn_valid']) == int(case('chunks')['res']['n_rpn_valid'])
    compare('rank >= T', res, grads, ref)
    d = {k: v.copy() for k, v in c.items()}
    d['target_class_ids'][2], d['target_class_ids'][5] = 3, -1
    res, grads = run_device(d)
    ref = u.reference(d)
    assert int(res['bad']) == 2 == ref['bad']
    compare('bad class id', res, grads, ref)
    assert not grads['mrcnn_class_logits'][2].any() and not grads['mrcnn_mask'][5].any() and not grads['mrcnn_bbox'][2].any()


def test_a_probability_outside_the_unit_interval_gives_nan_in_that_loss_only():
    c = case('chunks')['c']
    d = {k: v.copy() for k, v in c.items()}
    d['mrcnn_mask'][0, c['target_class_ids'][0], 3, 3] = 1.5
    res, _ = run_device(d, (False,) * 5)
    assert np.isnan(val(res['mrcnn_mask_loss'])) and np.isnan(val(res['loss']))
    assert all(torch.equal(res[k], case('chunks')['res'][k]) for k in u.LOSSES[:4])


def test_compute_losses_is_the_references_list_and_strides_do_not_matter():
    full = case('chunks')
    c = full['c']
    t = device_inputs(c)
    out = losses.compute_losses(*[t[k] for k in u.INPUTS])
    assert isinstance(out, list) and len(out) == 5
    for o, k in zip(out, u.LOSSES):
        assert o.dim() == 0 and torch.equal(o, full['res'][k]), k
    loss = out[0] + out[1] + out[2] + out[3] + out[4]          # model.py:1955
    # five fp32 values added in fp32, as the reference does.  Every term is below 4 and a correctly rounded fp64 value (half a
    # unit in the last place: 2^-23 = 1.2e-7 at most); each of the four additions rounds a partial sum below 8 by at most 2^-22 =
    # 2.4e-7
    assert all(full['ref'][k] < 4 for k in u.LOSSES[:5]) and full['ref']['loss'] < 8
    assert abs(val(loss) - full['ref']['loss']) <= 5 * 1.2e-7 + 4 * 2.4e-7
    loss.backward()
    assert all(t[k].grad is not None and t[k].grad.any() for k in u.PREDICTIONS)
    # non-contiguous views: the box predictions inside a wider row, the masks in the network's [R, h, w, C] layout
    A, R, C = c['rpn_pred_bbox'].shape[1], c['mrcnn_mask'].shape[0], c['mrcnn_mask'].shape[1]
    t = device_inputs(c)
    wide = torch.zeros(1, A, 6, device=DEV)
    wide[..., 1:5] = t['rpn_pred_bbox'].detach()
    wide.requires_grad_()
    nhwc = t['mrcnn_mask'].detach().permute(0, 2, 3, 1).contiguous().requires_grad_()
    args = dict(t)
    args['rpn_pred_bbox'], args['mrcnn_mask'] = wide[..., 1:5], nhwc.permute(0, 3, 1, 2)
    assert not args['rpn_pred_bbox'].is_contiguous() and not args['mrcnn_mask'].is_contiguous()
    res = losses.mrcnn_losses(*[args[k] for k in u.INPUTS])
    total_of(res).backward()
    for k in full['res']:
        assert torch.equal(res[k], full['res'][k]), k
    assert torch.equal(wide.grad[..., 1:5], full['grads']['rpn_pred_bbox']) and not wide.grad[..., 0].any() and not wide.grad[..., 5].any()
    assert torch.equal(nhwc.grad.permute(0, 3, 1, 2), full['grads']['mrcnn_mask'])
    assert torch.equal(t['mrcnn_bbox'].grad, full['grads']['mrcnn_bbox'])


def reference_form(t):
    """the reference's expressions for the RPN class loss (model.py:1013-1027)"""
    rpn_match = t['rpn_match'].squeeze(2)
    anchor_class = (rpn_match == 1).long()
    indices = torch.nonzero(rpn_match != 0)
    logits = t['rpn_class_logits'][indices.data[:, 0], indices.data[:, 1], :]
    anchor_class = anchor_class[indices.data[:, 0], indices.data[:, 1]]
    return F.cross_entropy(logits, anchor_class)


def test_no_host_wait_forward_and_backward(monkeypatch):
    """torch.cuda.set_sync_debug_mode('error') raises on a synchronising call; .cpu() / .item() / .tolist() / .numpy() on a tensor
    are made to raise for the duration as well.  The reference's own expressions do raise there: the probe works."""
    full = case('chunks')          # everything is loaded and compiled before the probe is set
    t = device_inputs(full['c'])
    e = device_inputs(case('empty')['c'])
    weights = torch.tensor(u.WEIGHTS, device=DEV)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('device-to-host copy')
    was = torch.cuda.get_sync_debug_mode()
    with monkeypatch.context() as mp:
        for name in ('cpu', 'item', 'tolist', 'numpy'):
            mp.setattr(torch.Tensor, name, refuse)
        torch.cuda.set_sync_debug_mode('error')
        try:
            res = losses.mrcnn_losses(*[t[k] for k in u.INPUTS])
            (res['loss']._base * weights).sum().backward()
            out = losses.compute_losses(*[e[k] for k in u.INPUTS])
            sum(out).backward()
            with pytest.raises(RuntimeError):
                reference_form(t)
        finally:
            torch.cuda.set_sync_debug_mode(was)
    assert torch.equal(res['loss'], full['res']['loss'])
    for k in u.PREDICTIONS:
        assert u.grad_error(t[k].grad.cpu().numpy(), full['ref']['grad'][k], full['ref']['n'][k]) <= u.GATE, k
    assert abs(val(reference_form(t)) - full['ref']['rpn_class_loss']) <= u.GATE       # and outside the probe they are the same loss


# ---- the C entry points on guarded buffers -------------------------------------------------------------------------------------------
CANARY = -12345.0
PAD = 64   # elements on either side


def guarded(n, dtype, canary):
    buf = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
    buf[PAD:PAD + n] = float('nan') if dtype.is_floating_point else 99
    return buf, buf[PAD:PAD + n]


def borders_intact(buf, canary):
    return bool((buf[:PAD] == canary).all()) and bool((buf[-PAD:] == canary).all())


def shifted(a, shift):
    """a device copy of the numpy array whose first element sits `shift` elements behind a 256-byte boundary"""
    hold = torch.zeros(a.size + 8, dtype=torch.as_tensor(a).dtype, device=DEV)
    view = hold[shift:shift + a.size]
    view.copy_(torch.as_tensor(a).reshape(-1))
    return view


@pytest.mark.parametrize('name,shift', [('chunks', 0), ('chunks', 1), ('exact', 0), ('exact', 1), ('nopos', 0), ('empty', 0)])
def test_nothing_is_written_outside_the_outputs(name, shift):
    """workspace, saved, out, counts and the five gradients inside canary borders, the outputs NaN / 99 before the call.  shift 1
    moves every input and gradient off its 16-byte alignment: the same case then takes the scalar loads and stores."""
    import sdn_hip
    from sdn_hip import ops
    full = case(name)
    c = full['c']
    A, T, R = c['rpn_match'].shape[1], c['rpn_bbox'].shape[1], c['target_class_ids'].shape[0]
    C, h, w = c['mrcnn_mask'].shape[1:] if R else (0, 0, 0)
    L = sdn_hip.lib()
    t = {k: (shifted(c[k], shift) if c[k].size else None) for k in u.INPUTS}
    assert (t['rpn_pred_bbox'].data_ptr() % 16 == 0) == (shift == 0)
    flags = [int(c[k].dtype == np.int64) for k in ('rpn_match', 'target_class_ids')]
    wbytes, sbytes = ops.mrcnn_loss_bytes(A, R)
    work_buf, work = guarded(wbytes, torch.uint8, 0xA5)
    saved_buf, saved = guarded(sbytes, torch.uint8, 0xA5)
    out_buf, out = guarded(6, torch.float32, CANARY)
    cnt_buf, cnt = guarded(4, torch.int64, -777)
    grads = {}
    for k in u.PREDICTIONS:
        if c[k].size:
            buf, g = guarded(c[k].size + shift, torch.float32, CANARY)
            grads[k] = (buf, g[shift:])
            buf[PAD:PAD + shift] = CANARY
    p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    inputs = [p(t['rpn_match']), flags[0], p(t['rpn_bbox']), p(t['rpn_class_logits']), p(t['rpn_pred_bbox']), 1, A, T,
              p(t['target_class_ids']), flags[1], p(t['mrcnn_class_logits']), p(t['target_deltas']), p(t['mrcnn_bbox']),
              p(t['target_mask']), p(t['mrcnn_mask']), R, C, h, w]
    rc = L.sdn_mrcnn_loss_fwd(*(inputs + [p(work), wbytes, p(saved), sbytes, p(out), p(cnt), sdn_hip.stream()]))
    assert rc == 0, L.sdn_last_error()
    gout = torch.tensor(u.WEIGHTS, dtype=torch.float32, device=DEV)
    gp = [p(grads[k][1]) if k in grads else None for k in u.PREDICTIONS]
    rc = L.sdn_mrcnn_loss_bwd(*(inputs + [p(saved), sbytes, p(gout)] + gp + [sdn_hip.stream()]))
    assert rc == 0, L.sdn_last_error()
    torch.cuda.synchronize()
    assert borders_intact(work_buf, 0xA5) and borders_intact(saved_buf, 0xA5) and borders_intact(out_buf, CANARY) and borders_intact(cnt_buf, -777)
    for k, (buf, g) in grads.items():
        assert borders_intact(buf, CANARY) and bool((buf[PAD:PAD + shift] == CANARY).all()), k
        # every element written, and the same numbers as through the binding: per element both load paths run the same operations
        assert torch.equal(g.view(full['grads'][k].shape), full['grads'][k]), k
    res = full['res']
    assert [int(v) for v in cnt] == [int(res[k]) for k in u.COUNTS]
    for i, k in enumerate(u.LOSSES):
        got, want = val(out[i]), val(res[k])
        if np.isnan(want):
            assert np.isnan(got), k
        elif shift == 0 or k in u.LOSSES[:4]:
            assert got == want, k
        else:   # the mask planes' scalar path sums in another order
            assert abs(got - full['ref'][k]) <= u.GATE, k


def test_the_references_full_shapes():
    """A = 261 888 anchors (256 chunks), T = 256, R = 200, C = 3, 28 x 28: drawn here, checked against the float64 restatement"""
    c = u.draw(seed=5201, A=261888, T=256, pos=200, valid=0.3, R=200, C=3, h=28, w=28, ids='mixed', dtype=np.int32)
    ref = u.reference(c)
    res, grads = run_device(c)
    compare('full size', res, grads, ref)
    assert int(res['n_rpn_pos']) == 200 and int(res['bad']) == 0 and 0 < int(res['n_roi_pos']) < 200
    assert int(res['n_rpn_valid']) > 70000
