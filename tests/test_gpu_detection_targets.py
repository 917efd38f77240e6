"""maskrcnn.detection_targets (sdn_detection_targets, csrc/detection_targets.hip) against the reference's detection_target_layer: the
fixture tests/golden/detection_targets_golden.npz holds what the reference's own functions gave on its own crop_and_resize.c, its
randperm being the order of the sampling keys (tests/golden/make_detection_targets_golden.py); tests/detection_targets_util.py restates
them in numpy.

rows, assign, the counts, rois, class ids, masks, dy, dx and all padding must equal the fixture bit for bit: they come from IEEE
operations in the reference's order alone (the masks' samples lie at least 0.01 from 0.5, asserted by the generator).  dh and dw pass
through logf and must lie within the gate stored per case -- four times the reference's own |fp32 - fp64| -- or within 2^-22 of the
value."""
import numpy as np
import pytest
import torch

import detection_targets_util as u
from maskrcnn import detection_targets as dt   # the feature itself: without it this module does not import
from maskrcnn import losses
from sdn_hip import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = 2.0 ** -22


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
    BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, c):
        self.TRAIN_ROIS_PER_IMAGE, self.ROI_POSITIVE_RATIO = c['R'], c['ratio']
        self.USE_MINI_MASK, self.MASK_SHAPE = c['mini'], list(c['shape'])


def device_inputs(c, ids_dtype=None):
    t = [torch.from_numpy(c[k].copy()).to(DEV) for k in u.INPUTS]
    if ids_dtype is not None:
        t[1] = t[1].to(ids_dtype)
    return t


def device_count(c):
    return None if c['roi_count'] is None else torch.tensor([c['roi_count']], dtype=torch.int32, device=DEV)


def run(c, ids_dtype=None):
    proposals, ids, boxes, masks, keys = device_inputs(c, ids_dtype)
    out = ops.detection_targets(proposals, ids, boxes, masks, keys, c['R'], c['ratio'], c['std_dev'], c['shape'], use_mini_mask=c['mini'],
                                roi_count=device_count(c))
    return {k: v.cpu().numpy() for k, v in zip(u.OUTPUTS, out)}


def compare(d, gold, name):
    c = u.draw_case(name)
    p = name + '/'
    want = {k: gold[p + k] for k in u.OUTPUTS if k != 'target_mask'}
    want['target_mask'] = u.unpack_masks(gold[p + 'target_mask_bits'], (c['R'],) + tuple(c['shape']))
    for k in u.OUTPUTS:
        assert d[k].dtype == want[k].dtype and d[k].shape == want[k].shape, k
    n, P = int(want['count'][0]), int(want['n_pos'][0])
    print('%s: count %d (the fixture %d), positives %d (%d)' % (name, int(d['count'][0]), n, int(d['n_pos'][0]), P))
    for k in ('count', 'n_pos', 'rows', 'assign', 'rois', 'target_class_ids', 'target_mask'):
        bad = int((d[k] != want[k]).sum()) if d[k].dtype.kind != 'f' else int((d[k].view(np.uint32) != want[k].view(np.uint32)).sum())
        print('%s %s: %d of %d elements differ' % (name, k, bad, d[k].size))
        assert d[k].tobytes() == want[k].tobytes(), k
    got, ref = d['target_deltas'], want['target_deltas']
    assert got[:, :2].tobytes() == ref[:, :2].tobytes()                       # dy, dx
    assert got[P:].tobytes() == np.zeros((c['R'] - P, 4), np.float32).tobytes()   # +0.0 for negatives and behind count
    gate = float(gold[p + 'gate'])
    err = np.abs(got[:P, 2:].astype(np.float64) - ref[:P, 2:])
    tol = np.maximum(gate, REL * np.abs(ref[:P, 2:].astype(np.float64)))
    print('%s: dh, dw differ by at most %.3e; gate %.3e' % (name, float(err.max()) if P else 0.0, gate))
    assert (err <= tol).all()


@pytest.mark.parametrize('name', list(u.CASES))
def test_every_output_is_the_references(gold, poisoned_empty, name):
    compare(run(u.draw_case(name)), gold, name)


def test_int64_class_ids_give_the_same(gold, poisoned_empty):
    for name in ('crowd_with_zero_id', 'zero_id_no_crowd'):
        compare(run(u.draw_case(name), torch.int64), gold, name)


@pytest.mark.parametrize('name', ['few_positive', 'none_positive', 'no_negative', 'full_mask'])
def test_the_reference_form_is_the_padded_form_cut_at_count(gold, name):
    c = u.draw_case(name)
    proposals, ids, boxes, masks, keys = device_inputs(c)
    cfg = Config(c)
    rois, cls, deltas, mask, count, n_pos = dt.detection_targets_padded(proposals[None], ids[None], boxes[None], masks[None], cfg, keys=keys)
    a = dt.detection_target_layer(proposals[None], ids[None], boxes[None], masks[None], cfg, keys=keys)
    n = int(gold[name + '/count'][0])
    assert int(count.item()) == n and int(n_pos.item()) == int(gold[name + '/n_pos'][0])
    assert rois.shape == (1, c['R'], 4) and cls.dtype == torch.int32 and mask.shape == (c['R'],) + tuple(c['shape'])
    assert [tuple(t.shape) for t in a] == [(n, 4), (n,), (n, 4), (n,) + tuple(c['shape'])]
    for x, y in zip(a, (rois[0], cls, deltas, mask)):
        assert torch.equal(x, y[:n]) and not x.requires_grad
    assert rois[0].cpu().numpy().tobytes() == gold[name + '/rois'].tobytes()


def test_keys_drawn_on_the_device_give_a_valid_sample():
    c = u.draw_case('real')
    proposals, ids, boxes, masks, _keys = device_inputs(c)
    torch.manual_seed(5)
    out = ops.detection_targets(proposals, ids, boxes, masks, torch.rand(2, c['N'], device=DEV), c['R'], c['ratio'], c['std_dev'], c['shape'])
    d = {k: v.cpu().numpy() for k, v in zip(u.OUTPUTS, out)}
    rois, cls, deltas, mask, count, n_pos = dt.detection_targets_padded(proposals, ids, boxes, masks, Config(c))   # keys=None
    n, P = int(count.item()), int(n_pos.item())
    assert 0 < P <= int(c['R'] * c['ratio']) and P <= n <= c['R']
    positive, negative, assign, _gt = u.classes_of(c)   # float32 IoU, the device's own arithmetic
    rows, cnt, npos = d['rows'], int(d['count'][0]), int(d['n_pos'][0])
    assert positive[rows[:npos]].all() and negative[rows[npos:cnt]].all() and (rows[cnt:] == -1).all()
    assert len(set(rows[:cnt].tolist())) == cnt and np.array_equal(d['assign'][:npos], assign[rows[:npos]])
    # the padded form's own draw: every roi is a proposal of the right class
    got = rois[0, :n].cpu().numpy()
    index = {r.tobytes(): i for i, r in enumerate(c['proposals'])}
    rows = np.array([index[r.tobytes()] for r in got])
    assert positive[rows[:P]].all() and negative[rows[P:]].all() and (cls[n:].cpu().numpy() == -1).all()
    assert not np.array_equal(rows, u.contract(c)['rows'][:n])     # and not the fixture's keys


def test_the_padded_targets_compose_with_the_losses(gold):
    """class id -1 behind count is what mrcnn_losses leaves out: the padded targets give the unpadded targets' head losses"""
    c = u.draw_case('few_positive')
    proposals, ids, boxes, masks, keys = device_inputs(c)
    cfg = Config(c)
    _rois, cls, deltas, mask, count, _n_pos = dt.detection_targets_padded(proposals, ids, boxes, masks, cfg, keys=keys)
    R, n, C = c['R'], int(count.item()), 8
    H, W = c['shape']
    assert 0 < n < R
    g = torch.Generator(device='cpu').manual_seed(11)
    A = 32
    rpn_match = torch.randint(-1, 2, (1, A, 1), generator=g).to(DEV)
    rpn_bbox, rpn_logits, rpn_pred = torch.randn(1, A, 4, generator=g).to(DEV), torch.randn(1, A, 2, generator=g).to(DEV), torch.randn(1, A, 4, generator=g).to(DEV)
    logits, bbox = torch.randn(R, C, generator=g).to(DEV), torch.randn(R, C, 4, generator=g).to(DEV)
    probs = torch.rand(R, C, H, W, generator=g).mul(0.98).add(0.01).to(DEV)
    padded = losses.mrcnn_losses(rpn_match, rpn_bbox, rpn_logits, rpn_pred, cls, logits, deltas, bbox, mask, probs)
    cut = losses.mrcnn_losses(rpn_match, rpn_bbox, rpn_logits, rpn_pred, cls[:n], logits[:n], deltas[:n], bbox[:n], mask[:n], probs[:n])
    for k in ('mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss'):
        a, b = float(padded[k]), float(cut[k])
        print('%s: padded %.9g, cut at count %.9g' % (k, a, b))
        assert np.isfinite(a) and a == b, k
    assert int(padded['bad']) == R - n and int(cut['bad']) == 0 and int(padded['n_roi_pos']) == int(cut['n_roi_pos']) > 0


def test_a_captured_call_replayed_with_new_keys_equals_the_eager_result():
    c = u.draw_case('n1025')
    proposals, ids, boxes, masks, keys = device_inputs(c)
    cfg = Config(c)
    static_keys = keys.clone()
    dt.detection_targets_padded(proposals, ids, boxes, masks, cfg, keys=static_keys)   # warm up: the library is loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = dt.detection_targets_padded(proposals, ids, boxes, masks, cfg, keys=static_keys)
    new_keys = torch.rand(2, c['N'], generator=torch.Generator().manual_seed(3)).to(DEV)
    static_keys.copy_(new_keys)
    graph.replay()
    torch.cuda.synchronize()
    eager = dt.detection_targets_padded(proposals, ids, boxes, masks, cfg, keys=new_keys)
    first = dt.detection_targets_padded(proposals, ids, boxes, masks, cfg, keys=keys)
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
    assert not torch.equal(eager[0], first[0])
