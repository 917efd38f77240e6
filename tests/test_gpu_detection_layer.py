"""maskrcnn.detection_layer (sdn_detection_layer, csrc/detection_layer.hip) against the reference's refine_detections: the fixture
tests/golden/detection_layer_golden.npz holds what the reference's own functions gave on its own nms.c
(tests/golden/make_detection_layer_golden.py), tests/detection_layer_util.py restates them in numpy.

All seven outputs must equal the fixture bit for bit.  That is exact, not approximate: scores are gathered, boxes are whole pixels
after rounding, and the only operation that may differ from the reference's CPU run, expf, can show only by moving a coordinate
across k + 0.5 -- the fixture's generator asserted that every coordinate lies further from a half than four times the reference's own
float32 error (`halves` is exact by construction).  `overflow` (NaN boxes) compares the three per-row outputs, NaNs equal to each
other.  Without any margin, keep must equal per-class pth_nms of this project followed by the final sort, on the device's own
boxes, class ids and scores."""
import numpy as np
import pytest
import torch

import detection_layer_util as u
from maskrcnn import detection_layer   # the feature itself: without it this module does not import
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

    def __init__(self, c):
        self.IMAGE_SHAPE = np.array([c['image'][0], c['image'][1], 3])
        self.DETECTION_MIN_CONFIDENCE = c['conf']
        self.DETECTION_NMS_THRESHOLD = c['thr']
        self.DETECTION_MAX_INSTANCES = c['D']


def device_inputs(c):
    return [torch.from_numpy(c[k].copy()).to(DEV) for k in ('rois', 'probs', 'deltas')]


def device_count(c):
    return None if c['roi_count'] is None else torch.tensor([c['roi_count']], dtype=torch.int32, device=DEV)


def run(c, strict=True):
    rois, probs, deltas = device_inputs(c)
    H, W = c['image']
    out = ops.detection_layer(rois, probs, deltas, c['window'], c['std_dev'], H, W, c['conf'], c['thr'], c['D'], roi_count=device_count(c),
                              strict=strict)
    return dict(zip(u.OUTPUTS, out))


_done = {}


def case(name):
    """the device's answer to a fixture case, computed once and shared (read-only), as numpy"""
    if name not in _done:
        _done[name] = {k: v.cpu().numpy() for k, v in run(u.draw_case(name)).items()}
        for v in _done[name].values():
            v.setflags(write=False)
    return _done[name]


def same(a, b):
    """equal bits, any NaN counting as equal to any NaN"""
    nan = np.isnan(a) if a.dtype.kind == 'f' else np.zeros(a.shape, bool)
    other = np.isnan(b) if b.dtype.kind == 'f' else np.zeros(b.shape, bool)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, other) and a[~nan].tobytes() == b[~nan].tobytes()


@pytest.mark.parametrize('name', list(u.CASES))
def test_all_seven_outputs_are_the_references_bits(gold, name):
    d = case(name)
    p = name + '/'
    for k in u.OUTPUTS:
        assert d[k].dtype == gold[p + k].dtype and d[k].shape == gold[p + k].shape, k
    for k in ('class_ids', 'scores', 'boxes_px'):
        bad = int((~((d[k] == gold[p + k]) | (d[k] != d[k]))).sum())
        print('%s %s: %d of %d elements differ' % (name, k, bad, d[k].size))
        assert same(d[k], gold[p + k]), k
    if name in u.ROWS_ONLY:
        return
    print('%s: count %d, the fixture %d; gate %.2e px, nearest half %.2e px' % (name, int(d['count'][0]), int(gold[p + 'count'][0]),
                                                                             float(gold[p + 'gate']), float(gold[p + 'half_distance'])))
    for k in ('keep', 'count', 'detections', 'boxes_norm'):
        assert d[k].tobytes() == gold[p + k].tobytes(), k


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_loose_rule_keeps_the_fixtures_rows(gold, name):
    if name in u.ROWS_ONLY:
        return
    d = {k: v.cpu().numpy() for k, v in run(u.draw_case(name), strict=False).items()}
    p = name + '/'
    assert np.array_equal(d['keep'], gold[p + 'keep_loose']) and np.array_equal(d['count'], gold[p + 'count_loose'])
    assert d['boxes_px'].tobytes() == case(name)['boxes_px'].tobytes()
    if name == 'tie_iou':
        assert int(d['count'][0]) + 1 == int(case(name)['count'][0]) and 1 in case(name)['keep'] and 1 not in d['keep']


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_padding_is_written_norm_is_the_division_and_two_runs_agree(name, poisoned_empty):
    c = u.draw_case(name)
    d = {k: v.cpu().numpy() for k, v in run(c).items()}           # a fresh run into poisoned buffers
    n, D = int(d['count'][0]), c['D']
    assert 0 <= n <= D
    if name not in u.ROWS_ONLY:                                   # no poison survives: the only NaNs are the scores of rows that hold one
        for k in ('boxes_px', 'detections', 'boxes_norm'):
            assert not np.isnan(d[k]).any(), k
    assert (d['class_ids'] >= 0).all() and (d['class_ids'] < c['C']).all()
    assert np.isnan(d['scores']).sum() == np.isnan(c['probs']).any(1).sum()
    assert (d['keep'][n:] == -1).all() and (d['keep'][:n] >= 0).all() and (d['keep'][:n] < c['N']).all()
    assert d['detections'][n:].tobytes() == np.zeros((D - n, 6), np.float32).tobytes()             # +0.0
    assert d['boxes_norm'][n:].tobytes() == np.zeros((D - n, 4), np.float32).tobytes()
    keep = d['keep'][:n]
    assert d['detections'][:n, :4].tobytes() == d['boxes_px'][keep].tobytes()
    assert np.array_equal(d['detections'][:n, 4], d['class_ids'][keep].astype(np.float32)) and (d['detections'][:n, 4] > 0).all()
    assert d['detections'][:n, 5].tobytes() == d['scores'][keep].tobytes()
    H, W = c['image']
    with np.errstate(all='ignore'):
        want = d['detections'][:n, :4] / np.asarray([H, W, H, W], np.float32)                      # one IEEE division per coordinate
    assert same(d['boxes_norm'][:n], want)
    for k in d:
        assert d[k].tobytes() == case(name)[k].tobytes(), k                                        # two runs are bit-identical


@pytest.mark.parametrize('strict', [True, False])
@pytest.mark.parametrize('name', list(u.CASES))
def test_keep_is_per_class_pth_nms_and_the_final_sort_on_the_devices_own_rows(name, strict):
    """no margin needed: :798-829 on the device's own boxes_px, class_ids and scores, with this project's pth_nms per class"""
    c = u.draw_case(name)
    d = run(c, strict=strict)
    class_ids, scores, boxes = d['class_ids'].long(), d['scores'], d['boxes_px']
    limit = c['N'] if c['roi_count'] is None else c['roi_count']
    valid = (torch.arange(c['N'], device=DEV) < limit) & (class_ids > 0)
    if c['conf']:
        valid = valid & (scores >= c['conf'])
    rows = torch.nonzero(valid)[:, 0]
    kept = []
    for class_id in torch.unique(class_ids[rows]).tolist():
        ixs = rows[class_ids[rows] == class_id]
        # pth_nms sorts by score itself: hand it a strictly descending stand-in, so that equal and NaN scores keep the contract's order
        order = torch.from_numpy(u._descending(scores[ixs].cpu().numpy())).to(DEV)
        rank = torch.arange(len(ixs), 0, -1, dtype=torch.float32, device=DEV)
        k = pth_nms(torch.cat([boxes[ixs[order]], rank[:, None]], 1), c['thr'], strict=strict)
        kept.append(ixs[order[k]])
    n = int(d['count'].item())
    if not kept:
        assert n == 0
        return
    kept = torch.cat(kept).sort()[0].cpu().numpy()
    want = kept[u._descending(scores.cpu().numpy()[kept])][:c['D']]
    assert n == len(want) and np.array_equal(d['keep'][:n].cpu().numpy(), want)


@pytest.mark.parametrize('name', ['few', 'real_c3', 'window', 'all_background'])
def test_the_drop_in_forms_return_the_prefix(name):
    c, d = u.draw_case(name), case(name)
    rois, probs, deltas = device_inputs(c)
    cfg = Config(c)
    n = int(d['count'][0])
    out = detection_layer.refine_detections(rois, probs, deltas, c['window'], cfg)
    assert out.shape == (n, 6) and out.dtype == torch.float32 and not out.requires_grad
    assert out.cpu().numpy().tobytes() == d['detections'][:n].tobytes()
    meta = np.zeros((1, 8 + c['C']))
    meta[0, 1:4] = (c['image'][0], c['image'][1], 3)
    meta[0, 4:8] = c['window']
    for m in (meta, torch.from_numpy(meta)):
        out2 = detection_layer.detection_layer(cfg, rois[None], probs, deltas, m)
        assert torch.equal(out2, out)
    det, norm, count = detection_layer.detections_padded(rois[None], probs.requires_grad_(), deltas.requires_grad_(), c['window'], cfg)
    assert det.shape == (c['D'], 6) and norm.shape == (1, c['D'], 4) and int(count.item()) == n
    assert det.cpu().numpy().tobytes() == d['detections'].tobytes() and norm[0].cpu().numpy().tobytes() == d['boxes_norm'].tobytes()
    assert not det.requires_grad and not norm.requires_grad


def test_the_count_of_the_proposals_is_handed_through_unread():
    c, d = u.draw_case('roi_count'), case('roi_count')
    rois, probs, deltas = device_inputs(c)
    det, _norm, count = detection_layer.detections_padded(rois, probs, deltas, c['window'], Config(c), roi_count=device_count(c))
    n = int(count.item())
    assert n == int(d['count'][0]) and det.cpu().numpy().tobytes() == d['detections'].tobytes() and d['keep'][:n].max() < c['roi_count']
    # without the count the confident rows behind it are detections
    every = detection_layer.detections_padded(rois, probs, deltas, c['window'], Config(c))
    assert not torch.equal(every[0], det)
    # a count beyond N means all rows; a negative one none
    for value, like in ((10 ** 6, every), (-5, None)):
        got = detection_layer.detections_padded(rois, probs, deltas, c['window'], Config(c),
                                                roi_count=torch.tensor([value], dtype=torch.int32, device=DEV))
        if like is None:
            assert int(got[2].item()) == 0 and not got[0].any()
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, like))


def test_nothing_waits_for_the_device_and_a_side_stream_gives_the_same_bits():
    c, d = u.draw_case('real_c81'), case('real_c81')
    rois, probs, deltas = device_inputs(c)
    cfg = Config(c)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')       # torch raises on anything that makes the host wait for the stream
    try:
        det, norm, count = detection_layer.detections_padded(rois, probs, deltas, c['window'], cfg)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert det.cpu().numpy().tobytes() == d['detections'].tobytes() and int(count.item()) == int(d['count'][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        det2, norm2, count2 = detection_layer.detections_padded(rois, probs, deltas, c['window'], cfg)
    side.synchronize()
    assert torch.equal(det2, det) and torch.equal(norm2, norm) and torch.equal(count2, count)


def test_tensors_the_kernels_cannot_take_are_refused_and_the_largest_sizes_run():
    c = u.draw_case('few')
    rois, probs, deltas = device_inputs(c)
    tail = (c['window'], c['std_dev'], 256, 256, 0.7, 0.3, 100)
    with pytest.raises(TypeError, match='probs must be torch.float32'):
        ops.detection_layer(rois, probs.double(), deltas, *tail)
    with pytest.raises(ValueError, match='deltas must be contiguous'):
        ops.detection_layer(rois, probs, deltas.transpose(1, 2).contiguous().transpose(1, 2), *tail)
    with pytest.raises(NotImplementedError, match='probs is on cpu'):
        ops.detection_layer(rois, probs.cpu(), deltas, *tail)
    with pytest.raises(NotImplementedError, match='roi_count is on cpu'):
        ops.detection_layer(rois, probs, deltas, *tail, roi_count=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='N = 8193'):
        ops.detection_layer(torch.zeros(8193, 4, device=DEV), torch.zeros(8193, 2, device=DEV), torch.zeros(8193, 2, 4, device=DEV), *tail)
    with pytest.raises(ValueError, match='max_instances 8193'):
        ops.detection_layer(rois, probs, deltas, *tail[:-1], 8193)
    with pytest.raises(TypeError, match='window must be four host numbers'):
        ops.detection_layer(rois, probs, deltas, torch.tensor(c['window'], device=DEV), *tail[1:])
    # the largest N and D the sorting workgroup and the scan take: every row valid, a grid of boxes that overlap their neighbours
    N = u.MAX_ROIS
    rs = np.random.RandomState(5)
    gy, gx = np.divmod(np.arange(N), 128)
    big = dict(name='big', N=N, C=3, D=u.MAX_INSTANCES, image=(1024, 1024), window=(0, 0, 1024, 1024), std_dev=u.STD_DEV, conf=0.0, thr=0.3,
               roi_count=None, rois=(np.stack([gy * 8, gx * 8, gy * 8 + 20, gx * 8 + 20], 1) / 1024.0).astype(np.float32),
               probs=u._probs(rs, N, 3, rs.randint(1, 3, N), rs.uniform(0.5, 0.999, N)).astype(np.float32),
               deltas=rs.normal(0, 0.5, (N, 3, 4)).astype(np.float32))
    d = {k: v.cpu().numpy() for k, v in run(big).items()}
    class_ids, scores, _pre, valid = u.rows_of(big)
    assert np.array_equal(d['class_ids'], class_ids) and d['scores'].tobytes() == scores.tobytes() and valid.all()
    keep = u.keep_global(d['class_ids'], d['scores'], d['boxes_px'], valid, 0.3, N, True)          # on the device's own boxes: no margin here
    n = int(d['count'][0])
    assert 128 < n == len(keep) < N and np.array_equal(d['keep'][:n], keep) and (d['keep'][n:] == -1).all()


@pytest.mark.parametrize('C', [1, 2, 7, 8, 9, 17, 81, 200])
def test_the_arg_max_is_torch_max_on_the_cpu_with_ties_and_nans_in_every_lane(C):
    """k_det_rows splits a row's classes over eight lanes and combines their candidates: rows of few distinct values (ties within a
    lane, across lanes, with class 0), NaNs of either sign before and behind the maximum, whole rows of -inf and of NaN -- against
    the reference's own operation, torch.max(dim=1) on the CPU (model.py:760)"""
    rs = np.random.RandomState(100 + C)
    N = 130
    probs = (rs.randint(0, 4, (N, C)) / 4.0).astype(np.float32)
    probs[rs.uniform(0, 1, (N, C)) < 0.04] = np.nan
    probs[rs.uniform(0, 1, (N, C)) < 0.02] = -np.nan
    probs[5::16] = rs.uniform(0, 1, probs[5::16].shape).astype(np.float32)        # distinct values
    probs[3] = -np.inf
    probs[4] = np.nan
    probs[6] = -0.0
    probs[6, C // 2] = 0.0                                                       # equal to -0.0: the first index still wins
    want_scores, want_ids = torch.max(torch.from_numpy(probs), dim=1)
    out = ops.detection_layer(torch.rand(N, 4, device=DEV), torch.from_numpy(probs).to(DEV), torch.zeros(N, C, 4, device=DEV), (0, 0, 64, 64),
                              u.STD_DEV, 64, 64, 0.0, 0.3, 10)
    class_ids, scores = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.array_equal(class_ids, want_ids.numpy().astype(np.int32))
    assert same(scores, want_scores.numpy()) and np.array_equal(np.signbit(scores[6:7]), np.signbit(want_scores.numpy()[6:7]))
