"""maskrcnn.rpn_targets (sdn_rpn_targets, csrc/rpn_targets.hip) against the reference's build_rpn_targets: the fixture
tests/golden/rpn_targets_golden.npz holds what the reference's own functions gave, its np.random.choice being the order of the
sampling keys (tests/golden/make_rpn_targets_golden.py); tests/rpn_targets_util.py restates them in numpy.

rpn_match, rows, the counts, dy, dx and all padding must equal the fixture bit for bit: they come from IEEE float64 operations in the
reference's order and one rounding to float32.  dh and dw pass through log: a device log may differ from numpy's in the last bit of
the double, which moves the float32 rounding by at most one step, so they must be equal or adjacent float32 values, infinities
equal."""
import numpy as np
import pytest
import torch

import rpn_targets_util as u
from maskrcnn import losses
from maskrcnn import rpn_targets as rt   # the feature itself: without it this module does not import
from sdn_hip import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty that fills what it returns: NaN for floats, 99 for integers -- whatever a kernel leaves unwritten shows"""
    real_empty = torch.empty

    def poison(t):
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(99)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: poison(real_empty(*a, **k)))


class Config(object):
    RPN_TRAIN_ANCHORS_PER_IMAGE = u.T
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)


def device_inputs(c):
    return [torch.from_numpy(np.ascontiguousarray(c[k]).copy()).to(DEV) for k in ('anchors', 'gt_class_ids', 'gt_boxes', 'keys')]


def device_count(c):
    return None if c['gt_count'] is None else torch.tensor([c['gt_count']], dtype=torch.int32, device=DEV)


def run(c, ids_dtype=None, boxes_dtype=None):
    anchors, ids, boxes, keys = device_inputs(c)
    if ids_dtype is not None:
        ids = ids.to(ids_dtype)
    if boxes_dtype is not None:
        boxes = boxes.to(boxes_dtype)
    out = ops.rpn_targets(anchors, ids, boxes, keys, c['T'], c['std_dev'], gt_count=device_count(c))
    return {k: v.cpu().numpy() for k, v in zip(('rpn_match', 'rpn_bbox', 'rows', 'counts'), out)}


def compare(d, gold, name):
    c = u.draw_case(name)
    p = name + '/'
    A, T = c['A'], c['T']
    want_match = u.unpack_labels(gold[p + 'match_at'], gold[p + 'match_values'], A)
    want_bbox, want_rows, want_counts = gold[p + 'rpn_bbox'], gold[p + 'rows'], gold[p + 'counts']
    assert d['rpn_match'].dtype == np.int32 and d['rpn_match'].shape == (A,)
    assert d['rpn_bbox'].dtype == np.float32 and d['rpn_bbox'].shape == (T, 4)
    assert d['rows'].dtype == np.int32 and d['rows'].shape == (T,) and d['counts'].dtype == np.int32 and d['counts'].shape == (2,)
    n_pos = int(want_counts[0])
    print('%s: counts %s (the fixture %s); %d labels differ; %d rows differ' % (name, d['counts'].tolist(), want_counts.tolist(),
                                                                               int((d['rpn_match'] != want_match).sum()), int((d['rows'] != want_rows).sum())))
    assert d['counts'].tobytes() == want_counts.tobytes()
    assert d['rpn_match'].tobytes() == want_match.tobytes()
    assert d['rows'].tobytes() == want_rows.tobytes()
    got = d['rpn_bbox']
    assert got[:, :2].tobytes() == want_bbox[:, :2].tobytes()                              # dy, dx
    assert got[n_pos:].tobytes() == np.zeros((T - n_pos, 4), np.float32).tobytes()         # +0.0 behind n_pos
    ok, adjacent = u.adjacent_or_equal(got[:n_pos, 2:], want_bbox[:n_pos, 2:])
    print('%s: dh, dw: %d of %d values are the adjacent float32, the others equal' % (name, adjacent, 2 * n_pos))
    assert ok
    return adjacent


@pytest.mark.parametrize('name', list(u.CASES))
def test_every_output_is_the_references(gold, poisoned_empty, name):
    compare(run(u.draw_case(name)), gold, name)


def test_other_dtypes_of_ids_and_boxes_give_the_same(gold, poisoned_empty):
    compare(run(u.draw_case('crowd_mixed'), torch.int64, torch.int32), gold, 'crowd_mixed')
    compare(run(u.draw_case('int_boxes_int64_ids'), torch.int32, torch.float32), gold, 'int_boxes_int64_ids')


@pytest.mark.parametrize('name', ['plain', 'many_positive', 'no_box'])
def test_the_reference_form_is_the_padded_form(gold, name):
    c = u.draw_case(name)
    anchors, ids, boxes, keys = device_inputs(c)
    match, bbox, rows, counts = rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=keys)
    a_match, a_bbox = rt.build_rpn_targets((c['side'], c['side'], 3), anchors, ids, boxes, Config, keys=keys)
    assert match.shape == (1, c['A'], 1) and match.dtype == torch.int32 and bbox.shape == (1, c['T'], 4) and bbox.dtype == torch.float32
    assert rows.shape == (c['T'],) and counts.shape == (2,)
    assert a_match.shape == (c['A'],) and a_bbox.shape == (c['T'], 4)
    assert torch.equal(a_match, match[0, :, 0]) and a_bbox.cpu().numpy().tobytes() == bbox[0].cpu().numpy().tobytes()
    assert not a_bbox.requires_grad and counts.cpu().numpy().tobytes() == gold[name + '/counts'].tobytes()


@pytest.mark.parametrize('name', ['ties', 'full'])
def test_two_calls_give_the_same_bits(name):
    c = u.draw_case(name)
    a, b = run(c), run(c)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_keys_drawn_on_the_device_give_a_valid_sample():
    c = u.draw_case('side256')
    anchors, ids, boxes, _keys = device_inputs(c)
    torch.manual_seed(5)
    match, bbox, rows, counts = rt.rpn_targets_padded(anchors, ids, boxes, Config)   # keys=None
    match, rows, counts = match[0, :, 0].cpu().numpy(), rows.cpu().numpy(), counts.cpu().numpy()
    mine = u.contract(c)
    before, T = mine['before'], c['T']
    n_pos, n_neg = int(counts[0]), int(counts[1])
    assert 0 < n_pos <= T // 2 and n_pos + n_neg <= T
    assert n_pos == min(int((before == 1).sum()), T // 2) and n_neg == min(int((before == -1).sum()), T - n_pos)
    assert int((match == 1).sum()) == n_pos and int((match == -1).sum()) == n_neg
    assert (before[match == 1] == 1).all() and (before[match == -1] == -1).all()       # every kept anchor was a candidate
    assert np.array_equal(rows[:n_pos], np.nonzero(match == 1)[0]) and (rows[n_pos:] == -1).all()
    want = u.deltas(c['anchors'][rows[:n_pos]], c['gt_boxes'].astype(np.float64)[mine['argmax'][rows[:n_pos]]], c['std_dev']).astype(np.float32)
    got = bbox[0].cpu().numpy()
    assert got[:n_pos, :2].tobytes() == want[:, :2].tobytes() and u.adjacent_or_equal(got[:n_pos, 2:], want[:, 2:])[0]
    assert not np.array_equal(match, mine['rpn_match'])                                 # and not the fixture's keys


def _rpn_losses(rpn_match, rpn_bbox, logits, pred):
    logits, pred = logits.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    C = 4
    empty = [torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, C, device=DEV), torch.zeros(0, 4, device=DEV),
             torch.zeros(0, C, 4, device=DEV), torch.zeros(0, 7, 7, device=DEV), torch.zeros(0, C, 7, 7, device=DEV)]
    res = losses.mrcnn_losses(rpn_match, rpn_bbox, logits, pred, *empty)
    (res['rpn_class_loss'] + res['rpn_bbox_loss']).backward()
    return res, logits.grad, pred.grad


def test_the_padded_targets_feed_the_losses(gold):
    """rpn_targets_padded's first two results ARE the rpn_match and rpn_bbox arguments of mrcnn_losses: the two RPN losses and their
    gradients are those of the fixture's targets"""
    name = 'plain'
    c = u.draw_case(name)
    anchors, ids, boxes, keys = device_inputs(c)
    match, bbox, _rows, counts = rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=keys)
    A, T = c['A'], c['T']
    g = torch.Generator(device='cpu').manual_seed(17)
    logits, pred = torch.randn(1, A, 2, generator=g).to(DEV), torch.randn(1, A, 4, generator=g).to(DEV)
    want_match = torch.from_numpy(u.unpack_labels(gold[name + '/match_at'], gold[name + '/match_values'], A)).to(DEV).view(1, A, 1)
    want_bbox = torch.from_numpy(gold[name + '/rpn_bbox']).to(DEV).view(1, T, 4)
    mine, ref = _rpn_losses(match, bbox, logits, pred), _rpn_losses(want_match, want_bbox, logits, pred)
    for k in ('rpn_class_loss', 'rpn_bbox_loss'):
        a, b = float(mine[0][k].detach()), float(ref[0][k].detach())
        print('%s: from the device targets %.9g, from the fixture %.9g' % (k, a, b))
        assert np.isfinite(a) and a == b, k
    assert int(mine[0]['n_rpn_pos']) == int(counts[0]) == int(gold[name + '/counts'][0]) > 0 and int(mine[0]['bad']) == 0
    assert int(mine[0]['n_rpn_valid']) == int(counts.sum())
    for a, b in zip(mine[1:], ref[1:]):
        assert a.abs().sum() > 0 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_a_captured_call_replayed_with_new_keys_equals_the_eager_result():
    c = u.draw_case('many_positive')
    anchors, ids, boxes, keys = device_inputs(c)
    static_keys = keys.clone()
    rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=static_keys)   # warm up: the library is loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=static_keys)
    new_keys = torch.rand(2, c['A'], generator=torch.Generator().manual_seed(3)).to(DEV)
    static_keys.copy_(new_keys)
    graph.replay()
    torch.cuda.synchronize()
    eager = rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=new_keys)
    first = rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=keys)
    for a, b in zip(captured, eager):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert not torch.equal(eager[0], first[0])
