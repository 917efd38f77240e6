"""The proposal layer without a GPU: the numpy restatement of tests/proposal_layer_util.py against the fixture
tests/golden/proposal_layer_golden.npz (the reference's own functions on its own nms.c, run by
tests/golden/make_proposal_layer_golden.py), the conditions the stored cases must meet (no IoU near the threshold, distinct scores),
the entry points' names in header, binding and library, the build list, the constants the Python side mirrors, the argument checks of
sdn_proposal_layer / _workspace_bytes and of the wrappers, all of which run before any launch, and the check header under ASan and
UBSan in a stand-alone host program."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import host_checks
import makefile_rules
import proposal_layer_util as u
from maskrcnn import proposals   # the feature itself: without it this module does not import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_proposal_layer_workspace_bytes', 'sdn_proposal_layer')


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_gives_the_fixtures_numbers(gold, name):
    c = u.draw_case(name)
    p = name + '/'
    assert (int(gold[p + 'crc_probs']), int(gold[p + 'crc_deltas']), int(gold[p + 'crc_anchors'])) == \
        (u.checksum(c['probs']), u.checksum(c['deltas']), u.checksum(c['anchors']))
    r = u.contract(c, np.float32)
    assert r['order'].dtype == np.int32 and np.array_equal(r['order'], gold[p + 'order']) and len(r['order']) == c['K'] == min(c['limit'], c['A'])
    # selection is torch's stable descending sort, NaN and all
    want = torch.sort(torch.from_numpy(c['probs'][:, 1].copy()), descending=True, stable=True)[1][:c['K']].numpy()
    assert np.array_equal(r['order'], want)
    assert np.array_equal(r['keep'], gold[p + 'keep']) and len(r['keep']) == int(gold[p + 'count']) <= c['P']
    assert np.array_equal(u.contract(c, np.float32, strict=False)['keep'], gold[p + 'keep_loose'])
    b64 = u.contract(c, np.float64)['boxes']
    gate = float(gold[p + 'gate'])
    assert gate == max(4 * float(gold[p + 'fp32_error']), 2.0 ** -23 * max(c['image']))
    if name in u.STORED_WHOLE:
        ref32, ref64 = gold[p + 'boxes_px32'], gold[p + 'boxes_px64']
        assert ref32.dtype == np.float32 and ref64.dtype == np.float64 and ref32.shape == ref64.shape == (c['K'], 4)
        assert np.array_equal(np.isnan(ref32), np.isnan(ref64)) and np.array_equal(np.isnan(r['boxes']), np.isnan(ref32))
        ok = ~np.isnan(ref64)
        assert not np.isinf(ref32).any() and np.allclose(b64[ok], ref64[ok], rtol=1e-12, atol=1e-9)
        # this machine's exp may differ from the generator's in the last bit: inside the gate, and equal bits where exp is exact
        assert np.abs(r['boxes'].astype(np.float64) - ref64)[ok].max() <= gate
        assert np.allclose(np.abs(ref32.astype(np.float64) - ref64)[ok].max(), gold[p + 'fp32_error'], rtol=1e-9, atol=0)
        if name in ('noexp', 'tie_iou'):
            assert r['boxes'].tobytes() == ref32.tobytes() and u.checksum(r['boxes']) == int(gold[p + 'crc_boxes32'])
            assert r['rois'].tobytes() == gold[p + 'rois32'].tobytes() and u.checksum(r['rois']) == int(gold[p + 'crc_rois32'])
        if name not in u.DECODE_ONLY:
            H, W = c['image']
            assert gold[p + 'rois32'].tobytes() == (ref32[gold[p + 'keep']] / np.asarray([H, W, H, W], np.float32)).tobytes()


def test_no_stored_case_sits_near_the_threshold_and_the_scores_are_distinct(gold):
    assert os.path.getsize(u.GOLD) < 400 * 1024
    for name in u.CASES:
        c = u.draw_case(name)
        boxes = gold[name + '/boxes_px32'] if name in u.STORED_WHOLE else u.contract(c)['boxes']
        if name != 'tie_iou' and name not in u.DECODE_ONLY:
            assert not u.near_pairs(boxes, c['thr']), name
            assert u.min_margin(boxes, c['thr']) >= u.MARGIN, name
            assert np.array_equal(gold[name + '/keep'], gold[name + '/keep_loose']), name       # `>` and `>=` keep the same boxes
        if name not in u.TIES:
            s = c['probs'][:, 1]
            top = s[u.select(s, min(c['K'] + 1, c['A']))]
            assert len(set(top.tolist())) == len(top), name
    # what the margin function flags: a pair on the threshold
    c = u.draw_case('tie_iou')
    boxes = gold['tie_iou/boxes_px32']
    assert u.near_pairs(boxes, c['thr']) == [1] and u.min_margin(boxes, c['thr']) == 0.0
    assert len(gold['tie_iou/keep']) == len(gold['tie_iou/keep_loose']) + 1 and 1 in gold['tie_iou/keep'] and 1 not in gold['tie_iou/keep_loose']


def test_the_fixture_holds_what_the_cases_are_there_for(gold):
    k = u.CASES
    assert u.draw_case('single')['A'] == 1 and u.draw_case('short')['A'] == 37 < k['short']['limit']
    assert (k['exactK']['A'], k['K+1']['A']) == (100, 101) and k['exactK']['limit'] == k['K+1']['limit'] == 100
    assert (k['chunks1025']['A'], k['chunks2049']['A']) == (u.CHUNK + 1, 2 * u.CHUNK + 1)
    assert [u.draw_case(n)['K'] for n in ('k63', 'k64', 'k65')] == [63, 64, 65]
    assert int(gold['onebox/count']) == 1 and int(gold['disjoint/count']) == k['disjoint']['P'] < len(u.nms(gold['disjoint/boxes_px32'], 0.7, True)) == 128
    assert int(gold['padded/count']) < k['padded']['P'] and int(gold['full/count']) < k['full']['P']
    assert not u.draw_case('noexp')['deltas'][:, 2:].any()
    assert k['rect']['image'] == (320, 480)
    b = gold['clip/boxes_px32']
    assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == 200).any() and (b[:, 3] == 200).any()
    assert np.isnan(gold['overflow/boxes_px32']).any() and not np.isinf(gold['overflow/boxes_px32']).any()
    assert np.array_equal(gold['ties_all/order'], np.arange(1000))
    c = u.draw_case('ties_straddle')
    s = c['probs'][:, 1]
    tied = np.nonzero(s == s[gold['ties_straddle/order'][-1]])[0]
    taken = np.intersect1d(tied, gold['ties_straddle/order'])
    assert len(tied) >= 300 and 0 < len(taken) < len(tied) and np.array_equal(taken, tied[:len(taken)])       # the lowest indices of the run
    assert len(set((tied // u.CHUNK).tolist())) == 4                                                                # in every chunk
    c = u.draw_case('ties_special')
    s = c['probs'][:, 1][gold['ties_special/order']]
    assert np.isnan(s[:3]).all() and np.isinf(s[3:5]).all() and (s[5:7] == 1.0).all() and np.isneginf(c['probs'][:, 1]).any()
    assert u.draw_case('objects')['A'] == 16368 and u.draw_case('full')['A'] == 261888 and u.draw_case('full')['K'] == 6000
    assert int(gold['objects/count']) < u.draw_case('objects')['K'] / 3                                             # heavy suppression
    assert u.pyramid_anchors(1024).shape == (261888, 4)


def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    clause = 'still 20: sdn_proposal_layer_workspace_bytes, sdn_proposal_layer added'
    assert clause in history[at - 3000:at]
    assert history.index('sdn_pyramid_roi_align_bwd added') < history.index(clause) < at
    assert 'model.py:344-407' in history and ':307-328' in history and ':331-341' in history and 'Nothing is differentiable' in history
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernels_are_built_without_fma_contraction_and_share_the_nms_pair_test():
    csrc = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
    makefile_rules.assert_built_exactly('proposal_layer.hip')
    makefile_rules.assert_built_exactly('raster_boxes.hip')
    shared = open(os.path.join(csrc, 'nms_mask.h')).read()
    assert len(re.findall(r'bool suppresses\(', shared)) == 1 and len(re.findall(r'void nms_mask_block\(', shared)) == 1
    for f in ('raster_boxes.hip', 'proposal_layer.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "nms_mask.h"' in text and 'nms_mask_block(' in text and not re.search(r'bool suppresses\(', text), f
    text = open(os.path.join(csrc, 'proposal_layer.hip')).read()
    assert '#include "proposal_layer_check.h"' in text and '#include "rank_select.h"' in text and 'ids_find(' in text
    assert 'expf(' in text and not re.search(r'__(expf|fdividef|frcp_r[a-z]|fdiv_r[a-z])\b', text)
    assert not re.search(r'\bf(min|max)f\(', text)                  # they drop NaN: the clamp compares
    assert 'hipLaunchCooperativeKernel' not in text and 'hipMemcpy' not in text and 'Synchronize' not in text


def test_the_constants_are_mirrored_and_the_workspace_comes_from_the_library():
    from sdn_hip import ops
    const = lambda k: host_checks.constexpr_int('proposal_layer_check.h', k)   # noqa: E731
    assert const('PROP_MAX_PRE_NMS') == ops.PROPOSAL_MAX_PRE_NMS == u.MAX_PRE_NMS == 8192
    assert const('PROP_MAX_ANCHORS') == ops.PROPOSAL_MAX_ANCHORS == u.MAX_ANCHORS == 1 << 24
    assert const('PROP_CHUNK') == ops.PROPOSAL_CHUNK == u.CHUNK == 4 * const('PROP_THREADS') and const('PROP_THREADS') % 64 == 0
    assert const('PROP_MAX_PRE_NMS') * 8 <= 64 * 1024 and const('PROP_SORT_THREADS') <= 1024
    assert list(inspect.signature(proposals.proposals_padded).parameters)[:5] == list(inspect.signature(proposals.proposal_layer).parameters)
    assert inspect.signature(ops.proposal_layer).parameters['pre_nms_limit'].default == 6000      # model.py:374

    def want(A, K, P):
        r16 = lambda n: (n + 15) // 16 * 16   # noqa: E731
        return r16(4 * const('PROP_HEAD_INTS')) + r16(4 * ((A + u.CHUNK - 1) // u.CHUNK)) + r16(8 * K) + r16(4 * K) + r16(8 * K * ((K + 63) // 64))
    for A, K, P in ((1, 1, 1), (37, 37, 10), (1025, 300, 50), (261888, 6000, 2000), ((1 << 24) - 1, 8192, 8192)):
        assert ops.proposal_workspace_bytes(A, K, P) == want(A, K, P), (A, K, P)


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _call(probs=FAKE, bbox=FAKE, anchors=FAKE, A=1000, std=(0.1, 0.1, 0.2, 0.2), height=256, width=256, K=100, P=20, order=FAKE, boxes=FAKE,
          keep=FAKE, count=FAKE, rois=FAKE, ws=FAKE, ws_bytes=1 << 26):
    import sdn_hip
    L = sdn_hip.lib()
    s = None if std is None else (ctypes.c_float * 4)(*std)
    rc = L.sdn_proposal_layer(probs, bbox, anchors, A, s, height, width, K, P, 0.7, 1, order, boxes, keep, count, rois, ws, ws_bytes, None)
    return rc, L.sdn_last_error().decode()


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    for kw, reason in ((dict(A=0), 'A 0 (no anchors)'), (dict(A=-1), 'A -1'), (dict(A=1 << 24), 'fewer than 2^24'), (dict(A=0x7fffffff), 'fewer than 2^24'),
                       (dict(K=0), 'K 0; 1 to 8192'), (dict(K=8193, A=100000), 'K 8193; 1 to 8192'), (dict(K=1001), 'K 1001 exceeds A 1000'),
                       (dict(P=0), 'P 0; 1 to 8192'), (dict(P=-3), 'P -3'), (dict(P=8193), 'P 8193'),
                       (dict(height=0), 'image 0 x 256'), (dict(width=-2), 'image 256 x -2'), (dict(std=None), 'std_dev is NULL'),
                       (dict(probs=None), 'rpn_probs, rpn_bbox or anchors is NULL'), (dict(bbox=None), 'rpn_probs, rpn_bbox or anchors is NULL'),
                       (dict(anchors=None), 'rpn_probs, rpn_bbox or anchors is NULL'),
                       (dict(order=None), 'count or rois is NULL'), (dict(boxes=None), 'count or rois is NULL'), (dict(keep=None), 'count or rois is NULL'),
                       (dict(count=None), 'count or rois is NULL'), (dict(rois=None), 'count or rois is NULL'),
                       (dict(ws=None), 'workspace is NULL'), (dict(ws_bytes=0), 'workspace 0 <'),
                       (dict(probs=FAKE + 2), 'aligned to 4 bytes'), (dict(anchors=FAKE + 1), 'aligned to 4 bytes'), (dict(keep=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(boxes=FAKE + 4), 'aligned to 16 bytes'), (dict(rois=FAKE + 8), 'aligned to 16 bytes'), (dict(ws=FAKE + 4), 'aligned to 16 bytes')):
        rc, msg = _call(**kw)
        assert rc == -1 and msg.startswith('sdn_proposal_layer: ') and reason in msg, (kw, msg)
    from sdn_hip import ops
    need = ops.proposal_workspace_bytes(1000, 100, 20)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == -1 and 'workspace %d < %d bytes' % (need - 1, need) in msg


def test_the_workspace_query_checks_its_arguments():
    import sdn_hip
    L = sdn_hip.lib()
    n = ctypes.c_size_t(0)
    assert L.sdn_proposal_layer_workspace_bytes(1000, 100, 20, ctypes.byref(n)) == 0 and n.value > 0
    assert L.sdn_proposal_layer_workspace_bytes(1000, 100, 20, None) == -1
    for A, K, P in ((0, 1, 1), (1 << 24, 1, 1), (10, 11, 1), (10, 0, 1), (100000, 8193, 1), (10, 5, 0), (10, 5, 8193)):
        assert L.sdn_proposal_layer_workspace_bytes(A, K, P, ctypes.byref(n)) == -1, (A, K, P)
        assert L.sdn_last_error().decode().startswith('sdn_proposal_layer_workspace_bytes: ')


class Config(object):
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, image):
        self.IMAGE_SHAPE = np.array([image[0], image[1], 3])


def _cpu_inputs(name='short', batch=True):
    c = u.draw_case(name)
    lift = (lambda t: t[None]) if batch else (lambda t: t)
    return [lift(torch.from_numpy(c['probs'].copy())), lift(torch.from_numpy(c['deltas'].copy()))], torch.from_numpy(c['anchors'].copy()), c


def test_the_wrappers_refuse_what_the_reference_cannot_mean():
    from sdn_hip import ops
    inputs, anchors, c = _cpu_inputs()
    cfg = Config(c['image'])
    held = list(inputs)
    for fn in (proposals.proposal_layer, proposals.proposals_padded):
        with pytest.raises(NotImplementedError, match='rpn_probs is on cpu'):
            fn(inputs, c['P'], c['thr'], anchors, cfg)                 # well-formed, but not on the GPU: there is no torch form
    assert all(a is b for a, b in zip(inputs, held)) and inputs[0].dim() == 3 and inputs[1].dim() == 3     # `inputs` is not changed
    with pytest.raises(NotImplementedError):
        proposals.proposal_layer(_cpu_inputs(batch=False)[0], c['P'], c['thr'], anchors, cfg)
    with pytest.raises(ValueError, match=r'rpn_probs has batch 2; only 1 is supported.*model\.py:358'):
        proposals.proposal_layer([torch.cat([inputs[0]] * 2), inputs[1]], c['P'], c['thr'], anchors, cfg)
    with pytest.raises(ValueError, match=r'rpn_bbox has batch 3.*model\.py:358'):
        proposals.proposal_layer([inputs[0], torch.cat([inputs[1]] * 3)], c['P'], c['thr'], anchors, cfg)
    with pytest.raises(ValueError, match='got 3 entries'):
        proposals.proposal_layer(inputs + inputs[:1], c['P'], c['thr'], anchors, cfg)
    with pytest.raises(ValueError, match='config is needed'):
        proposals.proposal_layer(inputs, c['P'], c['thr'], anchors)
    probs, deltas = inputs[0][0], inputs[1][0]
    args = (u.STD_DEV, 128, 128)
    with pytest.raises(ValueError, match='no anchors'):
        ops.proposal_layer(probs[:0], deltas[:0], anchors[:0], *args, 5, 0.7)
    with pytest.raises(ValueError, match='rpn_probs has 36 rows, rpn_bbox 37, anchors 37'):
        ops.proposal_layer(probs[:36], deltas, anchors, *args, 5, 0.7)
    with pytest.raises(ValueError, match='rpn_probs has 37 rows, rpn_bbox 37, anchors 30'):
        ops.proposal_layer(probs, deltas, anchors[:30], *args, 5, 0.7)
    with pytest.raises(ValueError, match='fewer than 2\\^24'):
        big = torch.empty(1, 1).expand(1 << 24, 4)                     # a shape only: one float behind it
        ops.proposal_layer(torch.empty(1, 1).expand(1 << 24, 2), big, big, *args, 5, 0.7)
    with pytest.raises(ValueError, match='proposal_count 0'):
        ops.proposal_layer(probs, deltas, anchors, *args, 0, 0.7)
    with pytest.raises(ValueError, match='proposal_count 11 exceeds pre_nms_limit 10'):
        ops.proposal_layer(probs, deltas, anchors, *args, 11, 0.7, pre_nms_limit=10)
    with pytest.raises(ValueError, match='proposal_count 6001 exceeds pre_nms_limit 6000'):
        proposals.proposal_layer(inputs, 6001, c['thr'], anchors, cfg)
    for limit in (0, 8193):
        with pytest.raises(ValueError, match='pre_nms_limit %d; 1 to 8192' % limit):
            ops.proposal_layer(probs, deltas, anchors, *args, 1, 0.7, pre_nms_limit=limit)
    with pytest.raises(ValueError, match=r'rpn_probs must be fp32 \[A, 2\]'):
        ops.proposal_layer(deltas, deltas, anchors, *args, 5, 0.7)
    with pytest.raises(ValueError, match=r'anchors must be fp32 \[A, 4\]'):
        ops.proposal_layer(probs, deltas, anchors[None], *args, 5, 0.7)
    with pytest.raises(ValueError, match='four values'):
        ops.proposal_layer(probs, deltas, anchors, (0.1, 0.2), 128, 128, 5, 0.7)
    with pytest.raises(ValueError, match='image 0 x 128'):
        ops.proposal_layer(probs, deltas, anchors, u.STD_DEV, 0, 128, 5, 0.7)
    with pytest.raises(TypeError, match='rpn_bbox must be torch.float32'):
        ops.proposal_layer(probs, deltas.double(), anchors, *args, 5, 0.7)
    with pytest.raises(TypeError, match='anchors must be torch.float32'):
        ops.proposal_layer(probs, deltas, anchors.half(), *args, 5, 0.7)
    with pytest.raises(TypeError, match='rpn_probs must be a torch.Tensor'):
        ops.proposal_layer(probs.numpy(), deltas, anchors, *args, 5, 0.7)
    with pytest.raises(ValueError, match='rpn_probs must be contiguous'):
        ops.proposal_layer(torch.cat([probs, probs], 1)[:, 1:3], deltas, anchors, *args, 5, 0.7)
    with pytest.raises(ValueError, match='anchors must be contiguous'):
        ops.proposal_layer(probs, deltas, anchors.t().contiguous().t(), *args, 5, 0.7)
    with pytest.raises(NotImplementedError, match='rpn_probs is on cpu; the proposal layer only runs on the GPU'):
        ops.proposal_layer(probs, deltas, anchors, *args, 5, 0.7)


def test_the_public_names_and_the_docstrings():
    assert list(inspect.signature(proposals.proposal_layer).parameters) == ['inputs', 'proposal_count', 'nms_threshold', 'anchors', 'config']   # model.py:344
    assert inspect.signature(proposals.proposal_layer).parameters['config'].default is None
    from sdn_hip import ops
    assert list(inspect.signature(ops.proposal_layer).parameters) == ['rpn_probs', 'rpn_bbox', 'anchors', 'std_dev', 'height', 'width', 'proposal_count',
                                                                      'nms_threshold', 'pre_nms_limit', 'strict']
    assert inspect.signature(ops.proposal_layer).parameters['strict'].default is True
    doc = ' '.join(proposals.proposal_layer.__doc__.split())
    assert 'model.py:344-407' in doc and 'is not changed' in doc and 'only host wait' in doc and 'no gradient' in doc
    for d in (ops.proposal_layer.__doc__, proposals.proposals_padded.__doc__, proposals.__doc__):
        assert 'No result carries a gradient' in ' '.join(d.split()) and ':473' in ops.proposal_layer.__doc__ and ':473' in proposals.__doc__


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_image_network_layout_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/proposal_layer_check.cpp: a stand-alone program with its own main that includes only csrc/proposal_layer_check.h; host
    code on the CPU, never loaded into Python"""
    rc, out = host_checks.run_check_program('proposal_layer_check', ['proposal_layer_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out and b'the validators' in out
