"""The detection layer's host half (no GPU): the numpy restatements of tests/detection_layer_util.py against the fixture
tests/golden/detection_layer_golden.npz (what the reference's own functions gave on its own nms.c,
tests/golden/make_detection_layer_golden.py) and against each other, the fixture's margins, the C entry points' refusals (they run on
the arguments alone, before any launch), the python layers' argument errors, the composition with detections.unmold_boxes, and
tools/detection_layer_check.cpp under ASan and UBSan."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import detection_layer_util as u
import host_checks
import makefile_rules
from maskrcnn import detection_layer as dl   # the feature itself: without it this module does not import
from maskrcnn import detections as det

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_detection_layer_workspace_bytes', 'sdn_detection_layer')


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


def same(a, b):
    """equal bits, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) if a.dtype.kind == 'f' else np.zeros(a.shape, bool)
    other = np.isnan(b) if b.dtype.kind == 'f' else np.zeros(b.shape, bool)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, other) and a[~nan].tobytes() == b[~nan].tobytes()


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_gives_the_fixtures_numbers(gold, name):
    c = u.draw_case(name)
    p = name + '/'
    for k in ('rois', 'probs', 'deltas'):
        assert u.checksum(c[k]) == int(gold[p + 'crc_' + k]), k                   # the draw is the generator's draw
    mine, loose = u.contract(c, np.float32, strict=True), u.contract(c, np.float32, strict=False)
    for k in u.OUTPUTS:
        assert same(mine[k], gold[p + k]), k
    assert np.array_equal(loose['keep'], gold[p + 'keep_loose']) and np.array_equal(loose['count'], gold[p + 'count_loose'])
    assert mine['class_ids'].dtype == np.int32 and mine['keep'].dtype == np.int32 and mine['count'].shape == (1,)
    assert mine['detections'].shape == (c['D'], 6) and mine['boxes_norm'].shape == (c['D'], 4) and mine['boxes_px'].shape == (c['N'], 4)
    n = int(mine['count'][0])
    assert (mine['keep'][n:] == -1).all() and mine['detections'][n:].tobytes() == np.zeros((c['D'] - n, 6), np.float32).tobytes()


@pytest.mark.parametrize('strict', [True, False])
@pytest.mark.parametrize('name', list(u.CASES))
def test_one_global_order_with_the_class_test_is_the_loop_over_classes(name, strict):
    """the proof of csrc/detection_layer.hip's header: the kernel's way gives the reference's way, on every case"""
    c = u.draw_case(name)
    a, b = u.contract(c, np.float32, strict), u.contract_global(c, np.float32, strict)
    for k in u.OUTPUTS:
        assert same(a[k], b[k]), k


def test_the_two_forms_agree_on_dense_random_scenes_with_many_classes_and_ties():
    """beyond the stored cases: heavy overlap, few score values, every D from 1 to more than survive"""
    rs = np.random.RandomState(31)
    for trial in range(30):
        N, C = int(rs.randint(2, 90)), int(rs.randint(2, 6))
        y1, x1 = rs.randint(0, 40, N), rs.randint(0, 40, N)
        boxes = np.stack([y1, x1, y1 + rs.randint(4, 30, N), x1 + rs.randint(4, 30, N)], 1).astype(np.float32)
        class_ids = rs.randint(0, C, N).astype(np.int32)
        scores = (rs.randint(1, 12, N) / 12.0).astype(np.float32)
        valid = (class_ids > 0) & (rs.uniform(0, 1, N) < 0.8)
        for D in (1, 3, N):
            for strict in (True, False):
                a = u.keep_per_class(class_ids, scores, boxes, valid, 0.3, D, strict)
                b = u.keep_global(class_ids, scores, boxes, valid, 0.3, D, strict)
                assert np.array_equal(a, b), (trial, D, strict)


def test_the_fixtures_margins_hold_and_nothing_was_widened(gold):
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        pre32, pre64 = u.rows_of(c, np.float32)[2], u.rows_of(c, np.float64)[2]
        finite = np.isfinite(pre64)
        err = float(np.abs(pre32.astype(np.float64) - pre64)[finite].max())
        gate, dist = float(gold[p + 'gate']), float(gold[p + 'half_distance'])
        assert err == float(gold[p + 'fp32_error']) and gate == max(4 * err, 2.0 ** -23 * max(c['image'])) and dist == u.half_distance(pre64), name
        if name in u.ON_HALVES:
            assert err == 0.0 and dist == 0.0
        else:
            assert dist > gate, (name, dist, gate)
        if name in u.ROWS_ONLY:
            continue
        class_ids, _scores, _pre, valid = u.rows_of(c)
        assert u.pairs_on_threshold(class_ids, gold[p + 'boxes_px'], valid, c['thr']) == (1 if name == 'tie_iou' else 0), name
        if name != 'tie_iou':
            assert np.array_equal(gold[p + 'keep'], gold[p + 'keep_loose']), name


def test_the_fixture_holds_what_the_cases_are_there_for(gold):
    count = {name: int(gold[name + '/count'][0]) for name in u.CASES}
    assert count['one'] == 1 and count['cross_class'] == 6 and count['same_class'] == 1
    assert count['all_background'] == count['C1'] == count['below_conf'] == 0 and count['no_min_conf'] > 0
    assert [int(gold['words%d/valid' % n]) for n in (63, 64, 65)] == [63, 64, 65]
    assert count['top_d'] == 5 and int(gold['top_d/valid']) > 100 and 0 < count['few'] < 100 and count['D1'] == 1
    assert gold['roi_count/keep'].max() < 100 and (gold['roi_count/class_ids'][100:] > 0).all()
    assert count['tie_iou'] == int(gold['tie_iou/count_loose'][0]) + 1
    for name in ('real_c3', 'real_c81'):
        assert gold[name + '/class_ids'].shape == (1000,) and 250 <= int(gold[name + '/valid']) <= 450 and gold[name + '/detections'].shape == (100, 6)
    assert np.isnan(gold['nan_row/scores']).any() and np.isnan(gold['overflow/boxes_px']).any()
    assert os.path.getsize(u.GOLD) < 400 * 1024


def test_unmold_boxes_reads_the_padded_detections_as_the_unpadded_ones(gold):
    c = u.draw_case('few')
    padded = gold['few/detections']
    n = int(gold['few/count'][0])
    assert 0 < n < c['D'] and (padded[n:] == 0).all() and (padded[:n, 4] > 0).all()
    a = det.unmold_boxes(padded, (375, 1242, 3), c['window'])
    b = det.unmold_boxes(padded[:n].copy(), (375, 1242, 3), c['window'])
    assert len(a) == len(b) == 4 and len(a[0]) > 0
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    clause = 'still 20: sdn_detection_layer_workspace_bytes, sdn_detection_layer added'
    assert history.index('sdn_proposal_layer added') < history.index(clause) < at
    assert 'model.py:744-837' in history and ':731-741' in history
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernels_are_built_without_fma_contraction_and_share_the_pair_test_and_the_clamp():
    csrc = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    makefile_rules.assert_built_exactly('detection_layer.hip')
    assert '-ffp-contract=off' in re.search(r'^EXACT\s*:=\s*(.*)$', mk, flags=re.M).group(1) and '-fno-slp-vectorize' in mk
    text = open(os.path.join(csrc, 'detection_layer.hip')).read()
    for h in ('nms_mask.h', 'prop_device.h', 'detection_layer_check.h'):
        assert '#include "%s"' % h in text
    assert 'suppresses(' in text and not re.search(r'bool suppresses\(', text) and 'prop_clamp(' in text and 'prop_sort_keys(' in text
    assert 'rintf(' in text and not re.search(r'\broundf\(', text)                 # half to even
    assert 'expf(' in text and not re.search(r'__(expf|fdividef|frcp_r[a-z]|fdiv_r[a-z])\b', text)
    assert not re.search(r'\bf(min|max)f\(', text)                                 # they drop NaN: the clamp compares
    assert 'atomic' not in text.split('namespace sdn {')[1]                        # no atomics at all
    assert 'hipLaunchCooperativeKernel' not in text and 'hipMemcpy' not in text and 'Synchronize' not in text
    shared = open(os.path.join(csrc, 'prop_device.h')).read()
    prop = open(os.path.join(csrc, 'proposal_layer.hip')).read()
    for fn in ('prop_clamp', 'prop_uniform64', 'prop_lane64', 'prop_sort_keys', 'prop_apply_deltas'):
        assert len(re.findall(r'\b%s\(' % fn, shared)) == 1 and '#include "prop_device.h"' in prop
    for f in (text, prop):                                                         # the decode and the sort are calls, not copies
        assert len(re.findall(r'\bprop_apply_deltas\(', f)) == 1 and len(re.findall(r'\bprop_sort_keys\(', f)) == 1
    # apply_box_deltas lives in the shared header: the same intrinsics are pinned there
    assert len(re.findall(r'\bexpf\(', shared)) == 2 and '#include "proposal_layer_check.h"' in shared
    for word in ('__expf', '__fdividef', 'fmaf', 'fminf', 'fmaxf', '__frcp_r', '__fdiv_r', 'atomic'):
        assert word not in shared, word
    assert len(re.findall(r'\bprop_bitonic_pair\(', shared)) == 1                 # the one device caller
    for f in os.listdir(csrc):
        if f.endswith('.hip'):
            assert 'prop_bitonic_pair(' not in open(os.path.join(csrc, f)).read(), f
    scan = open(os.path.join(csrc, 'nms_mask.h')).read()
    assert len(re.findall(r'\bnms_scan_words\(', scan)) == 1 and re.search(r'\bint nms_scan_words\(', scan) and '#include "prop_device.h"' in scan
    assert len(re.findall(r'\bNMS_SCAN_ROWS = 16;', scan)) == 1
    for f in (text, prop):
        assert len(re.findall(r'\bnms_scan_words\(', f)) == 1 and not re.search(r'\b(PROP|DET)_SCAN_ROWS\b', f)


def test_the_constants_are_mirrored_and_the_workspace_comes_from_the_library():
    from sdn_hip import ops
    hdr = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'detection_layer_check.h')).read()
    assert 'DET_MAX_ROIS = PROP_MAX_PRE_NMS' in hdr and 'DET_MAX_INSTANCES = PROP_MAX_PRE_NMS' in hdr
    assert ops.DETECTION_MAX_ROIS == u.MAX_ROIS == ops.PROPOSAL_MAX_PRE_NMS == 8192 and ops.DETECTION_MAX_INSTANCES == u.MAX_INSTANCES == 8192
    head = host_checks.constexpr_int('detection_layer_check.h', 'DET_HEAD_INTS')

    def want(N):
        r16 = lambda n: (n + 15) // 16 * 16   # noqa: E731
        return r16(4 * head) + r16(8 * N) + r16(16 * N) + 3 * r16(4 * N) + r16(8 * N * ((N + 63) // 64))
    for N, C, D in ((1, 1, 1), (63, 3, 30), (65, 3, 30), (1000, 81, 100), (8192, 2, 8192)):
        assert ops.detection_workspace_bytes(N, C, D) == want(N), (N, C, D)


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _call(rois=FAKE, probs=FAKE, deltas=FAKE, N=1000, C=3, window=(0, 0, 256, 256), std=(0.1, 0.1, 0.2, 0.2), height=256, width=256, D=100,
          roi_count=None, class_ids=FAKE, scores=FAKE, boxes=FAKE, keep=FAKE, count=FAKE, detections=FAKE, norm=FAKE, ws=FAKE, ws_bytes=1 << 26):
    import sdn_hip
    L = sdn_hip.lib()
    s = None if std is None else (ctypes.c_float * 4)(*std)
    w = None if window is None else (ctypes.c_float * 4)(*window)
    rc = L.sdn_detection_layer(rois, probs, deltas, N, C, w, s, height, width, 0.7, 0.3, D, 1, roi_count, class_ids, scores, boxes, keep, count,
                               detections, norm, ws, ws_bytes, None)
    return rc, L.sdn_last_error().decode()


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    null_out = 'keep, count, detections or boxes_norm is NULL'
    for kw, reason in ((dict(N=0), 'N 0; 1 to 8192'), (dict(N=-1), 'N -1'), (dict(N=8193), 'N 8193; 1 to 8192'), (dict(C=0), 'C 0 (no classes)'),
                       (dict(D=0), 'D 0; 1 to 8192'), (dict(D=-3), 'D -3'), (dict(D=8193), 'D 8193'),
                       (dict(height=0), 'image 0 x 256'), (dict(width=-2), 'image 256 x -2'), (dict(std=None), 'std_dev is NULL'),
                       (dict(window=None), 'window is NULL'),
                       (dict(rois=None), 'rois, probs or deltas is NULL'), (dict(probs=None), 'rois, probs or deltas is NULL'),
                       (dict(deltas=None), 'rois, probs or deltas is NULL'),
                       (dict(class_ids=None), 'class_ids, scores or boxes_px is NULL'), (dict(scores=None), 'class_ids, scores or boxes_px is NULL'),
                       (dict(boxes=None), 'class_ids, scores or boxes_px is NULL'),
                       (dict(keep=None), null_out), (dict(count=None), null_out), (dict(detections=None), null_out), (dict(norm=None), null_out),
                       (dict(ws=None), 'workspace is NULL'), (dict(ws_bytes=0), 'workspace 0 <'),
                       (dict(probs=FAKE + 2), 'aligned to 4 bytes'), (dict(roi_count=FAKE + 1), 'roi_count must be aligned to 4 bytes'),
                       (dict(keep=FAKE + 2), 'aligned to 4 bytes'), (dict(detections=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(boxes=FAKE + 4), 'aligned to 16 bytes'), (dict(norm=FAKE + 8), 'aligned to 16 bytes'), (dict(ws=FAKE + 4), 'aligned to 16 bytes')):
        rc, msg = _call(**kw)
        assert rc == -1 and msg.startswith('sdn_detection_layer: ') and reason in msg, (kw, msg)
    from sdn_hip import ops
    need = ops.detection_workspace_bytes(1000, 3, 100)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == -1 and 'workspace %d < %d bytes' % (need - 1, need) in msg


def test_the_workspace_query_checks_its_arguments():
    import sdn_hip
    L = sdn_hip.lib()
    n = ctypes.c_size_t(0)
    assert L.sdn_detection_layer_workspace_bytes(1000, 81, 100, ctypes.byref(n)) == 0 and n.value > 0
    assert L.sdn_detection_layer_workspace_bytes(1000, 81, 100, None) == -1
    for N, C, D in ((0, 1, 1), (8193, 1, 1), (10, 0, 1), (10, 3, 0), (10, 3, 8193)):
        assert L.sdn_detection_layer_workspace_bytes(N, C, D, ctypes.byref(n)) == -1, (N, C, D)
        assert L.sdn_last_error().decode().startswith('sdn_detection_layer_workspace_bytes: ')


class Config(object):
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, c):
        self.IMAGE_SHAPE = np.array([c['image'][0], c['image'][1], 3])
        self.DETECTION_MIN_CONFIDENCE = c['conf']
        self.DETECTION_NMS_THRESHOLD = c['thr']
        self.DETECTION_MAX_INSTANCES = c['D']


def _cpu_inputs(name='few'):
    c = u.draw_case(name)
    return [torch.from_numpy(c[k].copy()) for k in ('rois', 'probs', 'deltas')], c


def test_the_wrappers_refuse_what_the_kernels_cannot_take():
    from sdn_hip import ops
    (rois, probs, deltas), c = _cpu_inputs()
    cfg = Config(c)
    tail = (c['window'], c['std_dev'], 256, 256, 0.7, 0.3, 100)
    # there is no torch form: CPU tensors are an error in every layer
    with pytest.raises(NotImplementedError, match='rois is on cpu; the detection layer only runs on the GPU'):
        ops.detection_layer(rois, probs, deltas, *tail)
    with pytest.raises(NotImplementedError, match='rois is on cpu'):
        dl.detections_padded(rois[None], probs, deltas, c['window'], cfg)
    with pytest.raises(NotImplementedError):
        dl.refine_detections(rois, probs, deltas, c['window'], cfg)
    meta = np.zeros((1, 8 + c['C']))
    meta[0, 4:8] = c['window']
    with pytest.raises(NotImplementedError):
        dl.detection_layer(cfg, rois[None], probs, deltas, meta)
    with pytest.raises(NotImplementedError):
        dl.detection_layer(cfg, rois[None], probs, deltas, torch.from_numpy(meta))
    with pytest.raises(ValueError, match=r'image_meta must be \[1, 8 \+ classes\]'):
        dl.detection_layer(cfg, rois[None], probs, deltas, meta[0])
    with pytest.raises(ValueError, match=r'rois has batch 2; only 1 is supported.*model\.py:848'):
        dl.detections_padded(torch.stack([rois, rois]), probs, deltas, c['window'], cfg)
    with pytest.raises(ValueError, match='config is needed'):
        dl.detections_padded(rois, probs, deltas, c['window'], None)
    # shapes and sizes
    with pytest.raises(ValueError, match=r'rois must be fp32 \[N, 4\]'):
        ops.detection_layer(rois[:, :3], probs, deltas, *tail)
    with pytest.raises(ValueError, match=r'probs must be fp32 \[N, C\] with N = 150'):
        ops.detection_layer(rois, probs[:-1], deltas, *tail)
    with pytest.raises(ValueError, match=r'deltas must be fp32 \[N, C, 4\] = \(150, 4, 4\)'):
        ops.detection_layer(rois, probs, deltas[:, :3], *tail)
    with pytest.raises(ValueError, match='N = 0; 1 to 8192'):
        ops.detection_layer(rois[:0], probs[:0], deltas[:0], *tail)
    with pytest.raises(ValueError, match='N = 8193; 1 to 8192'):
        ops.detection_layer(torch.zeros(8193, 4), torch.zeros(8193, 2), torch.zeros(8193, 2, 4), *tail)
    with pytest.raises(ValueError, match='no classes'):
        ops.detection_layer(rois, probs[:, :0], deltas[:, :0], *tail)
    for D in (0, 8193):
        with pytest.raises(ValueError, match='max_instances %d; 1 to 8192' % D):
            ops.detection_layer(rois, probs, deltas, *tail[:-1], D)
    with pytest.raises(ValueError, match='image 0 x 256'):
        ops.detection_layer(rois, probs, deltas, c['window'], c['std_dev'], 0, 256, 0.7, 0.3, 100)
    with pytest.raises(ValueError, match='window must hold four values'):
        ops.detection_layer(rois, probs, deltas, (0, 0, 256), *tail[1:])
    with pytest.raises(ValueError, match='std_dev must hold four values'):
        ops.detection_layer(rois, probs, deltas, c['window'], (0.1, 0.2), *tail[2:])
    with pytest.raises(ValueError, match='roi_count must hold one element'):
        ops.detection_layer(rois, probs, deltas, *tail, roi_count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='deltas must be contiguous'):
        ops.detection_layer(rois, probs, deltas.transpose(1, 2).contiguous().transpose(1, 2), *tail)
    with pytest.raises(ValueError, match='rois must be contiguous'):
        ops.detection_layer(rois.t().contiguous().t(), probs, deltas, *tail)
    # types
    with pytest.raises(TypeError, match='probs must be torch.float32'):
        ops.detection_layer(rois, probs.double(), deltas, *tail)
    with pytest.raises(TypeError, match='deltas must be torch.float32'):
        ops.detection_layer(rois, probs, deltas.half(), *tail)
    with pytest.raises(TypeError, match='rois must be a torch.Tensor'):
        ops.detection_layer(rois.numpy(), probs, deltas, *tail)
    with pytest.raises(TypeError, match='roi_count must be torch.int32'):
        ops.detection_layer(rois, probs, deltas, *tail, roi_count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match='roi_count must be None or an int32'):
        ops.detection_layer(rois, probs, deltas, *tail, roi_count=100)
    with pytest.raises(NotImplementedError, match='rois is on cpu'):
        ops.detection_layer(rois, probs, deltas, *tail, roi_count=torch.zeros(1, dtype=torch.int32))


def test_the_public_names_and_the_docstrings():
    assert list(inspect.signature(dl.refine_detections).parameters) == ['rois', 'probs', 'deltas', 'window', 'config']                  # model.py:744
    assert list(inspect.signature(dl.detection_layer).parameters) == ['config', 'rois', 'mrcnn_class', 'mrcnn_bbox', 'image_meta']     # model.py:840
    assert list(inspect.signature(dl.detections_padded).parameters) == ['rois', 'probs', 'deltas', 'window', 'config', 'roi_count', 'strict']
    assert inspect.signature(dl.detections_padded).parameters['roi_count'].default is None
    assert inspect.signature(dl.detections_padded).parameters['strict'].default is True
    from sdn_hip import ops
    assert list(inspect.signature(ops.detection_layer).parameters) == ['rois', 'probs', 'deltas', 'window', 'std_dev', 'height', 'width', 'min_confidence',
                                                                       'nms_threshold', 'max_instances', 'roi_count', 'strict']
    doc = ' '.join(dl.refine_detections.__doc__.split())
    assert 'model.py:744-837' in doc and 'only host wait' in doc
    for d in (ops.detection_layer.__doc__, dl.__doc__):
        assert 'No result carries a gradient' in ' '.join(d.split())


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_layout_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/detection_layer_check.cpp: a stand-alone program with its own main that includes only csrc/detection_layer_check.h; host
    code on the CPU, never loaded into Python"""
    rc, out = host_checks.run_check_program('detection_layer_check', ['detection_layer_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out and b'the validators' in out
