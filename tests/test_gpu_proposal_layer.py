"""maskrcnn.proposals (sdn_proposal_layer, csrc/proposal_layer.hip) against the reference's proposal_layer: the fixture
tests/golden/proposal_layer_golden.npz holds what the reference's own functions gave on its own nms.c
(tests/golden/make_proposal_layer_golden.py), tests/proposal_layer_util.py restates them in numpy.

Selection, order, the kept positions and their count are exact.  The decoded boxes must lie within the fixture's gate of the float64
boxes, in pixels: four times the distance of the reference's own float32 run, at least 2^-23 of the image's longer side (device and
host exp may each be one ulp off, and two roundings follow); where exp is exact (`noexp`) the bits are equal.  rois is checked bit for
bit against the division of the device's own boxes.  No stored case has a pair of boxes whose IoU lies within 1e-5 of the threshold,
so the last bit of exp cannot change what is kept; and without any margin, keep must equal this project's pth_nms on the device's own
boxes and scores."""
import numpy as np
import pytest
import torch

import proposal_layer_util as u
from maskrcnn import proposals   # the feature itself: without it this module does not import
from maskrcnn.nms.pth_nms import pth_nms
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
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, image):
        self.IMAGE_SHAPE = np.array([image[0], image[1], 3])


def device_inputs(c, batch=True):
    lift = (lambda t: t[None]) if batch else (lambda t: t)
    return [lift(torch.from_numpy(c['probs'].copy())).to(DEV), lift(torch.from_numpy(c['deltas'].copy())).to(DEV)], \
        torch.from_numpy(c['anchors'].copy()).to(DEV)


def run(c, strict=True, batch=False):
    (probs, deltas), anchors = device_inputs(c, batch)
    H, W = c['image']
    out = ops.proposal_layer(probs, deltas, anchors, c['std_dev'], H, W, c['P'], c['thr'], pre_nms_limit=c['limit'], strict=strict)
    return dict(zip(('order', 'boxes_px', 'keep', 'count', 'rois'), out))


_done = {}


def case(name):
    """the device's answer to a fixture case, computed once and shared (read-only), as numpy"""
    if name not in _done:
        d = run(u.draw_case(name))
        _done[name] = {k: v.cpu().numpy() for k, v in d.items()}
        for v in _done[name].values():
            v.setflags(write=False)
    return _done[name]


@pytest.mark.parametrize('name', list(u.CASES))
def test_selection_and_kept_positions_are_the_references(gold, name):
    c, d = u.draw_case(name), case(name)
    p = name + '/'
    assert d['order'].dtype == np.int32 and d['order'].shape == (c['K'],) and np.array_equal(d['order'], gold[p + 'order'])
    assert d['keep'].dtype == np.int32 and d['keep'].shape == (c['P'],) and d['count'].dtype == np.int32 and d['count'].shape == (1,)
    if name in u.DECODE_ONLY:
        return
    n = int(d['count'][0])
    assert n == int(gold[p + 'count']) and np.array_equal(d['keep'][:n], gold[p + 'keep'])


@pytest.mark.parametrize('name', list(u.CASES))
def test_boxes_are_within_the_fixtures_gate_of_float64(gold, name):
    c, d = u.draw_case(name), case(name)
    p = name + '/'
    want = gold[p + 'boxes_px64'] if name in u.STORED_WHOLE else u.contract(c, np.float64)['boxes']
    ref32 = gold[p + 'boxes_px32'] if name in u.STORED_WHOLE else u.contract(c, np.float32)['boxes']
    got, gate = d['boxes_px'], float(gold[p + 'gate'])
    assert got.dtype == np.float32 and got.shape == want.shape == (c['K'], 4)
    assert np.array_equal(np.isnan(got), np.isnan(ref32)) and np.array_equal(np.isnan(got), np.isnan(want))
    assert not np.isinf(got).any() and not np.isinf(ref32).any()                      # the clamp leaves no infinity
    ok = ~np.isnan(want)
    err = float(np.abs(got.astype(np.float64) - want)[ok].max())
    print('%s: %.3e px from the float64 boxes; the reference\'s float32 run %.3e; gate %.3e; %d of %d coordinates differ from the float32 run'
          % (name, err, float(gold[p + 'fp32_error']), gate, int((got[ok] != ref32[ok]).sum()), int(ok.sum())))
    assert err <= gate
    if name in ('noexp', 'tie_iou'):                                                  # exp(0) is exact: the reference's bits
        assert got.tobytes() == ref32.tobytes() and u.checksum(got) == int(gold[p + 'crc_boxes32'])
        assert d['rois'][:int(d['count'][0])].tobytes() == gold[p + 'rois32'].tobytes()


@pytest.mark.parametrize('name', list(u.CASES))
def test_rois_are_the_division_of_the_devices_own_boxes_and_the_padding_is_written(name, poisoned_empty):
    c = u.draw_case(name)
    d = {k: v.cpu().numpy() for k, v in run(c).items()}           # a fresh run into poisoned buffers
    n = int(d['count'][0])
    assert 0 < n <= c['P'] and d['rois'].dtype == np.float32 and d['rois'].shape == (c['P'], 4)
    keep = d['keep'][:n]
    assert (keep >= 0).all() and (keep < c['K']).all() and (np.diff(keep) > 0).all() and keep[0] == 0
    H, W = c['image']
    with np.errstate(all='ignore'):
        want = d['boxes_px'][keep] / np.asarray([H, W, H, W], np.float32)              # one IEEE division per coordinate
    assert d['rois'][:n].tobytes() == want.tobytes()
    assert (d['keep'][n:] == -1).all() and d['rois'][n:].tobytes() == np.zeros((c['P'] - n, 4), np.float32).tobytes()     # +0.0
    assert not (d['order'] == 99).all() and sorted(d['order'].tolist()) == sorted(set(d['order'].tolist()))
    for k in d:
        assert d[k].tobytes() == case(name)[k].tobytes(), k                             # two runs are bit-identical


@pytest.mark.parametrize('strict', [True, False])
@pytest.mark.parametrize('name', list(u.CASES))
def test_keep_is_this_projects_nms_on_the_devices_own_boxes(name, strict):
    """no margin needed: the same boxes and scores through sdn_nms, cut to P"""
    c = u.draw_case(name)
    d = run(c, strict=strict) if not strict else {k: torch.from_numpy(v.copy()).to(DEV) for k, v in case(name).items()}
    scores = torch.from_numpy(c['probs'][:, 1].copy()).to(DEV)[d['order'].long()]
    # pth_nms sorts by score itself: hand it a strictly descending stand-in, so that equal and NaN scores keep the device's order
    rank = torch.arange(c['K'], 0, -1, dtype=torch.float32, device=DEV)
    keep = pth_nms(torch.cat([d['boxes_px'], rank[:, None]], 1), c['thr'], strict=strict)[:c['P']]
    n = int(d['count'].item())
    assert n == len(keep) and torch.equal(d['keep'][:n].long(), keep)
    if name not in u.TIES and not torch.isnan(scores).any():
        same = pth_nms(torch.cat([d['boxes_px'], scores[:, None]], 1), c['thr'], strict=strict)[:c['P']]
        assert torch.equal(same, keep)


def test_an_iou_on_the_threshold_is_kept_by_the_strict_rule_only(gold):
    c = u.draw_case('tie_iou')
    tight, loose = case('tie_iou'), {k: v.cpu().numpy() for k, v in run(c, strict=False).items()}
    assert np.array_equal(tight['keep'][:int(tight['count'][0])], gold['tie_iou/keep']) and 1 in tight['keep']
    assert np.array_equal(loose['keep'][:int(loose['count'][0])], gold['tie_iou/keep_loose']) and 1 not in loose['keep']
    assert int(tight['count'][0]) == int(loose['count'][0]) + 1 and tight['boxes_px'].tobytes() == loose['boxes_px'].tobytes()


@pytest.mark.parametrize('name', ['short', 'rect', 'padded', 'objects'])
def test_the_drop_in_form_is_the_padded_form_cut_to_count(gold, name):
    c, d = u.draw_case(name), case(name)
    inputs, anchors = device_inputs(c)
    held, shapes = list(inputs), [t.shape for t in inputs]
    cfg = Config(c['image'])
    n = int(d['count'][0])
    if c['limit'] == 6000:         # the reference's fixed limit: the drop-in form has no other
        out = proposals.proposal_layer(inputs, c['P'], c['thr'], anchors, cfg)
        assert out.shape == (1, n, 4) and out.dtype == torch.float32 and not out.requires_grad
        assert out[0].cpu().numpy().tobytes() == d['rois'][:n].tobytes()
    rois, count = proposals.proposals_padded(inputs, c['P'], c['thr'], anchors, cfg, pre_nms_limit=c['limit'])
    assert rois.shape == (1, c['P'], 4) and int(count.item()) == n and rois[0].cpu().numpy().tobytes() == d['rois'].tobytes()
    assert all(a is b for a, b in zip(inputs, held)) and [t.shape for t in inputs] == shapes            # `inputs` is not changed
    # without the batch axis, and with inputs that ask for a gradient: nothing comes back differentiable
    (probs, deltas), _ = device_inputs(c, batch=False)
    rois2, _ = proposals.proposals_padded([probs.requires_grad_(), deltas.requires_grad_()], c['P'], c['thr'], anchors, cfg, pre_nms_limit=c['limit'])
    assert torch.equal(rois2, rois) and not rois2.requires_grad


def test_nothing_waits_for_the_device_and_a_side_stream_gives_the_same_bits():
    c, d = u.draw_case('objects'), case('objects')
    inputs, anchors = device_inputs(c)
    cfg = Config(c['image'])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')       # torch raises on anything that makes the host wait for the stream
    try:
        rois, count = proposals.proposals_padded(inputs, c['P'], c['thr'], anchors, cfg, pre_nms_limit=c['limit'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert rois[0].cpu().numpy().tobytes() == d['rois'].tobytes() and int(count.item()) == int(d['count'][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rois2, count2 = proposals.proposals_padded(inputs, c['P'], c['thr'], anchors, cfg, pre_nms_limit=c['limit'])
    side.synchronize()
    assert torch.equal(rois2, rois) and torch.equal(count2, count)


def test_tensors_the_kernels_cannot_take_are_refused():
    c = u.draw_case('short')
    (probs, deltas), anchors = device_inputs(c, batch=False)
    args = (c['std_dev'], 128, 128, 5, 0.7)
    with pytest.raises(TypeError, match='rpn_probs must be torch.float32'):
        ops.proposal_layer(probs.double(), deltas, anchors, *args)
    with pytest.raises(ValueError, match='rpn_bbox must be contiguous'):
        ops.proposal_layer(probs, deltas.t().contiguous().t(), anchors, *args)
    with pytest.raises(NotImplementedError, match='anchors is on cpu'):
        ops.proposal_layer(probs, deltas, anchors.cpu(), *args)
    with pytest.raises(ValueError, match=r'model\.py:358'):
        ops.proposal_layer(torch.stack([probs, probs]), deltas, anchors, *args)
    # the largest K and P the sorting workgroup takes, more anchors than that
    A = u.MAX_PRE_NMS + 500
    g = torch.Generator(device='cpu').manual_seed(5)
    scores = torch.rand(A, generator=g)
    big = dict(probs=torch.stack([1 - scores, scores], 1).numpy(), deltas=torch.randn(A, 4, generator=g).numpy(),
               anchors=u._random_anchors(np.random.RandomState(5), A, 512, 512), std_dev=u.STD_DEV, image=(512, 512), A=A, K=u.MAX_PRE_NMS,
               P=u.MAX_PRE_NMS, thr=0.5, limit=u.MAX_PRE_NMS)
    d = {k: v.cpu().numpy() for k, v in run(big).items()}
    assert np.array_equal(d['order'], u.select(big['probs'][:, 1], u.MAX_PRE_NMS))
    want = u.decode(big['anchors'][d['order']], big['deltas'][d['order']], u.STD_DEV, 512, 512, np.float64)
    # before the clamp every intermediate stays below 2048 px (sides of at most 307 px scaled by e^(0.2 * 5), centres inside the image):
    # eight roundings of half an ulp of 2048, the one ulp of exp among them
    assert np.abs(d['boxes_px'] - want).max() <= 8 * 2.0 ** -24 * 2048
    keep = u.nms(d['boxes_px'], 0.5, True, u.MAX_PRE_NMS)           # on the device's own boxes: no margin was arranged here
    assert int(d['count'][0]) == len(keep) and np.array_equal(d['keep'][:len(keep)], keep) and (d['keep'][len(keep):] == -1).all()


def test_sdn_nms_still_gives_what_it_gave(gold):
    """raster_boxes.hip now takes its pair test from nms_mask.h: an old case of tests/test_gpu_maskrcnn_ops.py's kind, against the CPU
    restatement, and the proposal layer's own boxes through both paths"""
    rs = np.random.RandomState(11)
    n = 300
    y1, x1 = rs.uniform(0, 200, n), rs.uniform(0, 200, n)
    dets = np.stack([y1, x1, y1 + rs.uniform(5, 80, n), x1 + rs.uniform(5, 80, n), rs.permutation(n) / n], 1).astype(np.float32)
    order = np.argsort(-dets[:, 4], kind='stable')
    for strict in (True, False):
        want = order[u.nms(dets[order, :4], 0.5, strict)]
        got = pth_nms(torch.from_numpy(dets).to(DEV), 0.5, strict=strict).cpu().numpy()
        assert np.array_equal(got, want), strict
    b = torch.from_numpy(gold['objects/boxes_px32']).to(DEV)
    rank = torch.arange(len(b), 0, -1, dtype=torch.float32, device=DEV)
    got = pth_nms(torch.cat([b, rank[:, None]], 1), 0.7).cpu().numpy()
    assert np.array_equal(got[:len(gold['objects/keep'])], gold['objects/keep'])
