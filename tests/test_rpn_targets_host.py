"""The RPN targets' host half (no GPU): the numpy restatement of tests/rpn_targets_util.py against the fixture
tests/golden/rpn_targets_golden.npz (what the reference's own build_rpn_targets gave, tests/golden/make_rpn_targets_golden.py), the
branches the cases are there for, generate_pyramid_anchors against the stored table and checksums, the sampling's distribution, the C
entry points' refusals (they run on the arguments alone, before any launch), the python layers' argument errors, the build's flags
and tools/rpn_targets_check.cpp under ASan and UBSan."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import host_checks
import makefile_rules
import rpn_targets_util as u
from maskrcnn import rpn_targets as rt   # the feature itself: without it this module does not import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_rpn_targets_workspace_bytes', 'sdn_rpn_targets')


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture(scope='module')
def results():
    """the contract's outputs, computed once per case and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = u.contract(u.draw_case(name))
        return cache[name]
    return get


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    """tools/rpn_targets_check.cpp built with ASan and UBSan and run once as a child process: (return code, output)"""
    rc, out = host_checks.run_check_program('rpn_targets_check', ['rpn_targets_check.h'], tmp_path_factory.mktemp('rt'))
    return rc, out.decode()


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_gives_the_fixtures_numbers(gold, results, name):
    c, mine = u.draw_case(name), results(name)
    p = name + '/'
    for k in u.INPUTS:
        assert u.checksum(c[k]) == int(gold[p + 'crc_' + k]), k                   # the draw is the generator's draw
    assert mine['rpn_match'].dtype == np.int32 and mine['rpn_match'].shape == (c['A'],)
    assert np.array_equal(mine['rpn_match'], u.unpack_labels(gold[p + 'match_at'], gold[p + 'match_values'], c['A']))
    for k in ('rows', 'counts'):
        assert mine[k].dtype == gold[p + k].dtype == np.int32 and mine[k].tobytes() == gold[p + k].tobytes(), k
    n_pos = int(mine['counts'][0])
    # dy, dx are IEEE operations; dh, dw pass through this machine's log, whose last bit may differ between numpy builds
    for k, dtype in (('rpn_bbox64', np.float64), ('rpn_bbox', np.float32)):
        got, ref = mine[k], gold[p + k]
        assert got.dtype == ref.dtype == dtype and got.shape == ref.shape == (c['T'], 4)
        assert got[:, :2].tobytes() == ref[:, :2].tobytes() and got[n_pos:].tobytes() == np.zeros((c['T'] - n_pos, 4), dtype).tobytes()
    ok, adjacent = u.adjacent_or_equal(mine['rpn_bbox'][:, 2:], gold[p + 'rpn_bbox'][:, 2:])
    assert ok, adjacent
    assert gold[p + 'rpn_bbox'].tobytes() == gold[p + 'rpn_bbox64'].astype(np.float32).tobytes()   # :1404
    assert (mine['rows'][n_pos:] == -1).all() and np.array_equal(mine['rows'][:n_pos], np.nonzero(mine['rpn_match'] == 1)[0])


@pytest.mark.parametrize('name', list(u.CASES))
def test_every_case_reaches_the_branch_it_names(results, name):
    u.check_case(name, u.draw_case(name), results(name))


def test_the_case_list_is_the_issues():
    assert list(u.CASES) == ['plain', 'many_positive', 'few_negative', 'crowd_mixed', 'zero_id_no_crowd', 'unmatched_box', 'zero_box',
                             'zero_height_box', 'ties', 'thresholds', 'thresholds_low', 'gt_count', 'no_box', 'int_boxes_int64_ids',
                             'side256', 'full']
    assert u.draw_case('int_boxes_int64_ids')['gt_boxes'].dtype == np.int32 and u.draw_case('int_boxes_int64_ids')['gt_class_ids'].dtype == np.int64
    assert u.draw_case('plain')['gt_boxes'].dtype == np.float32 and u.draw_case('plain')['gt_class_ids'].dtype == np.int32
    assert u.T == 256 and os.path.getsize(u.GOLD) < 400 * 1024
    for name in u.CASES:   # integer pixels before gt_count: widening to float64 first is what the reference computes
        c = u.draw_case(name)
        n = c['G'] if c['gt_count'] is None else c['gt_count']
        b = c['gt_boxes'][:n].astype(np.float64)
        assert (b == np.rint(b)).all() and np.abs(b).max() <= 1024, name


def test_the_threshold_quotients_are_the_thresholds():
    # IoU of (24, 32, 60, 64) and of (0, 28, 54, 62) with the anchor (32, 32, 64, 64), as compute_iou computes them
    a = np.array([u.THRESHOLD_ANCHOR])
    for box, inter, union, want in (((24, 32, 60, 64), 896.0, 1280.0, 0.7), ((0, 28, 54, 62), 660.0, 2200.0, 0.3)):
        b = np.array(box, np.float64)
        iou = u.iou_column(b, a, (b[2] - b[0]) * (b[3] - b[1]), np.array([1024.0]))[0]
        assert iou == inter / union == want
    assert u.anchor_index(128, u.THRESHOLD_ANCHOR) >= 0


def test_generate_pyramid_anchors_is_the_references_bit_for_bit(gold):
    a = u.anchors(128)
    assert a.dtype == np.float64 and a.shape == (4092, 4) and a.tobytes() == gold['anchors128'].tobytes()
    for side, count in ((128, 4092), (256, 16368), (1024, 261888)):
        got = rt.generate_pyramid_anchors(u.SCALES, u.RATIOS, u.backbone_shapes(side), u.STRIDES, u.ANCHOR_STRIDE)
        assert got.shape == (count, 4) and np.array_equal(u.sha256(got), gold['anchors%d_sha256' % side]), side
    # another anchor stride and a rectangular level: the order is cell-major with the ratios inside a cell
    got = rt.generate_pyramid_anchors((8, 16), [0.5, 1, 2], [[4, 6], [2, 3]], [4, 8], 2)
    assert got.shape == ((2 * 3 + 1 * 2) * 3, 4)
    assert np.array_equal(got[0], [-8 / np.sqrt(0.5) / 2, -8 * np.sqrt(0.5) / 2, 8 / np.sqrt(0.5) / 2, 8 * np.sqrt(0.5) / 2])
    assert np.array_equal(got[4], [0 - 4, 8 - 4, 0 + 4, 8 + 4])   # second cell (y 0, x 2 * 4), ratio 1
    assert list(inspect.signature(rt.generate_pyramid_anchors).parameters) == ['scales', 'ratios', 'feature_shapes', 'feature_strides', 'anchor_stride']


def test_the_sampling_is_choice_in_distribution():
    """12 candidates, 5 stay: with uniform keys every candidate stays with probability 5 / 12 and every pair with 5 * 4 / (12 * 11).
    20 000 seeded draws; the bounds are five standard deviations of the binomial counts, so a correct sampler passes for certain
    (the draws are seeded) and one that favours an anchor by a few percent does not."""
    rs = np.random.RandomState(11)
    ids = np.array([3, 4, 9, 20, 21, 22, 40, 41, 50, 63, 64, 99])
    trials, n, k = 20000, 12, 5
    single, pair = np.zeros(100), np.zeros((100, 100))
    for _ in range(trials):
        keys = rs.uniform(0, 1, 100).astype(np.float32)
        stay = u.keep_smallest(ids, keys, k)
        assert len(stay) == k and np.isin(stay, ids).all() and (np.diff(stay) > 0).all()
        single[stay] += 1
        pair[np.ix_(stay, stay)] += 1
    p1, p2 = k / n, k * (k - 1) / (n * (n - 1))
    for p, counts in ((p1, single[ids]), (p2, pair[np.ix_(ids, ids)][~np.eye(n, dtype=bool)])):
        bound = 5 * np.sqrt(trials * p * (1 - p))
        assert np.abs(counts - trials * p).max() <= bound, (np.abs(counts - trials * p).max(), bound)
    # equal keys keep the lower anchor; the order is the image's, a negative NaN first and a positive NaN last
    keys = np.zeros(100, np.float32)
    assert np.array_equal(u.keep_smallest(ids, keys, 5), ids[:5])
    keys[[99, 64]] = [-np.nan, np.nan]
    keys[3] = 0.5
    assert np.array_equal(u.keep_smallest(ids, keys, 10), [4, 9, 20, 21, 22, 40, 41, 50, 63, 99])


def test_adjacent_or_equal_is_one_step_of_float32():
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    inf = np.float32(np.inf)
    assert u.adjacent_or_equal([one, -one, -inf, 0.0], [up, -down, -inf, 0.0]) == (True, 2)
    assert u.adjacent_or_equal([one], [np.nextafter(up, np.float32(2))]) == (False, 0)
    assert not u.adjacent_or_equal([np.finfo(np.float32).max], [inf])[0] and not u.adjacent_or_equal([-inf], [inf])[0]
    assert not u.adjacent_or_equal([np.float32(1e-45)], [np.float32(-1e-45)])[0] and not u.adjacent_or_equal([0.0], [-0.0])[0]


def test_the_check_program_walks_clean_under_asan_and_ubsan(check_program):
    """a stand-alone program with its own main that includes only csrc/rpn_targets_check.h; host code on the CPU, never loaded into
    Python"""
    rc, out = check_program
    text = open(os.path.join(ROOT, 'tools', 'rpn_targets_check.cpp')).read()
    assert re.findall(r'#include "([^"]+)"', text) == ['rpn_targets_check.h'] and 'int main()' in text and 'hip' not in text.lower()
    print(out)
    assert rc == 0 and ' 0 failures' in out and 'the validators: walked' in out
    from sdn_hip import ops
    (total,) = [int(line.split()[-1]) for line in out.splitlines() if line.startswith('workspace 261888 100 256 ')]
    assert ops.rpn_targets_workspace_bytes(261888, 100, 256) == total


# ---- header, binding, library, build -------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    clause = 'still 20: sdn_rpn_targets_workspace_bytes, sdn_rpn_targets added'
    assert history.index('sdn_detection_targets added') < history.index(clause) < at
    assert 'model.py:1214-1322' in history and 'utils.py:52-89' in history
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernels_are_built_exactly_and_use_no_shortcut():
    csrc = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    makefile_rules.assert_built_exactly('rpn_targets.hip')
    assert '-ffp-contract=off' in re.search(r'^EXACT\s*:=\s*(.*)$', mk, flags=re.M).group(1) and 'fast-math' not in mk
    text = open(os.path.join(csrc, 'rpn_targets.hip')).read()
    for h in ('rank_select.h', 'rpn_targets_check.h'):
        assert '#include "%s"' % h in text
    code = text.split('namespace sdn {')[1]
    assert 'ids_find(' in code and 'rt_argmax_takes(' in code and 'rt_image(' in code and 'rt_positives_kept(' in code
    assert not re.search(r'\bfloat\b(?!4)', code.split('struct RtArgs')[0])          # the arithmetic is double
    assert ' log(' in code and not re.search(r'\b(logf|__logf|__expf|__fdividef|__frcp_r[a-z]|__drcp_r[a-z]|__ddiv_r[a-z]|__fma_r[a-z])\b', code)
    assert not re.search(r'\bf(min|max|ma)f?\(', code)                               # fmin / fmax drop NaN, fma contracts
    assert set(re.findall(r'\batomic\w+', code)) == {'atomicAdd'}                    # integer counters only:
    for m in re.finditer(r'atomicAdd\(&(\w+)', code):                                # every target is an int histogram or counter
        assert m.group(1) in ('s_hist', 'R', 's_count', 's_before'), m.group(1)
    assert re.search(r'int32_t\* hist;', code) and 'atomicAdd(&R.hist[' in code and 'atomicAdd(&R.' not in code.replace('atomicAdd(&R.hist[', '')
    for word in ('hipLaunchCooperativeKernel', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipMalloc'):
        assert word not in text
    assert '0.3' in code and '0.7' in code and '0.001' in code and '0.3f' not in code and '0.7f' not in code
    hdr = open(os.path.join(csrc, 'rpn_targets_check.h')).read()
    assert re.findall(r'#include [<"]([^>"]+)[>"]', hdr) == ['cstring', 'detection_targets_check.h']   # plain C++: no HIP header


def test_the_constants_are_mirrored_and_the_workspace_comes_from_the_library():
    from sdn_hip import ops
    hdr = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'rpn_targets_check.h')).read()
    assert 'RT_MAX_ANCHORS = (1 << 24) - 1' in hdr and 'RT_MAX_BOXES = DT_MAX_BOXES' in hdr and 'RT_MAX_TARGETS = 8192' in hdr
    assert 'RT_CHUNK = RT_THREADS * RT_PER_LANE' in hdr and 'RT_THREADS = 256' in hdr and 'RT_PER_LANE = 4' in hdr and u.CHUNK == 1024
    assert (ops.RPN_TARGETS_MAX_ANCHORS, ops.RPN_TARGETS_MAX_BOXES, ops.RPN_TARGETS_MAX_PER_IMAGE) == \
        (u.MAX_ANCHORS, u.MAX_BOXES, u.MAX_TARGETS) == ((1 << 24) - 1, 128, 8192)
    small, large = ops.rpn_targets_workspace_bytes(4092, 8, 256), ops.rpn_targets_workspace_bytes(261888, 100, 256)
    assert small % 16 == 0 and large % 16 == 0 and 4092 < small < large < 1 << 20      # far from an [A, G] matrix of 210 MB


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _call(anchors=FAKE, ids=FAKE, boxes=FAKE, keys=FAKE, A=261888, G=100, ids64=0, boxes32=0, gt_count=None, T=256, std=(0.1, 0.1, 0.2, 0.2),
          match=FAKE, bbox=FAKE, rows=FAKE, counts=FAKE, ws=FAKE, ws_bytes=1 << 24):
    import sdn_hip
    L = sdn_hip.lib()
    s = None if std is None else (ctypes.c_double * 4)(*std)
    rc = L.sdn_rpn_targets(anchors, ids, boxes, keys, A, G, ids64, boxes32, gt_count, T, s, match, bbox, rows, counts, ws, ws_bytes, None)
    return rc, L.sdn_last_error().decode()


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    null_in, null_out = 'anchors, gt_class_ids, gt_boxes or keys is NULL', 'rpn_match, rpn_bbox, rows or counts is NULL'
    for kw, reason in ((dict(A=0), 'A 0; 1 to 16777215'), (dict(A=1 << 24), 'A 16777216; 1 to 16777215'), (dict(G=0), 'G 0; 1 to 128'),
                       (dict(G=129), 'G 129; 1 to 128'), (dict(T=1), 'T 1; 2 to 8192'), (dict(T=8193), 'T 8193; 2 to 8192'),
                       (dict(std=None), 'std_dev is NULL'), (dict(std=(0.1, 0.1, 0.0, 0.2)), 'std_dev[2] is 0'),
                       (dict(std=(0.1, float('nan'), 0.2, 0.2)), 'std_dev[1]'),
                       (dict(anchors=None), null_in), (dict(ids=None), null_in), (dict(boxes=None), null_in), (dict(keys=None), null_in),
                       (dict(match=None), null_out), (dict(bbox=None), null_out), (dict(rows=None), null_out), (dict(counts=None), null_out),
                       (dict(ws=None), 'workspace is NULL'), (dict(ws_bytes=0), 'workspace 0 < 580752 bytes'),
                       (dict(ws_bytes=580751), 'workspace 580751 < 580752 bytes'),
                       (dict(anchors=FAKE + 8), 'anchors must be aligned to 16 bytes'), (dict(keys=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(boxes=FAKE + 1), 'aligned to 4 bytes'), (dict(ids=FAKE + 2), 'gt_class_ids must be aligned to 4 bytes'),
                       (dict(ids=FAKE + 4, ids64=1), 'gt_class_ids must be aligned to 8 bytes'),
                       (dict(gt_count=FAKE + 1), 'gt_count must be aligned to 4 bytes'), (dict(match=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(rows=FAKE + 2), 'aligned to 4 bytes'), (dict(counts=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(bbox=FAKE + 4), 'aligned to 16 bytes'), (dict(ws=FAKE + 4), 'aligned to 16 bytes')):
        rc, msg = _call(**kw)
        assert rc == -1 and msg.startswith('sdn_rpn_targets: ') and reason in msg, (kw, msg)


def test_the_workspace_query_checks_its_arguments():
    import sdn_hip
    L = sdn_hip.lib()
    n = ctypes.c_size_t(0)
    assert L.sdn_rpn_targets_workspace_bytes(261888, 100, 256, ctypes.byref(n)) == 0 and n.value == 580752
    assert L.sdn_rpn_targets_workspace_bytes(261888, 100, 256, None) == -1
    for args in ((0, 24, 256), (1 << 24, 24, 256), (10, 0, 256), (10, 129, 256), (10, 3, 1), (10, 3, 8193), (-5, 3, 256)):
        assert L.sdn_rpn_targets_workspace_bytes(*args, ctypes.byref(n)) == -1, args
        assert L.sdn_last_error().decode().startswith('sdn_rpn_targets_workspace_bytes: ')


# ---- the python layers ---------------------------------------------------------------------------------------------------------------------
class Config(object):
    RPN_TRAIN_ANCHORS_PER_IMAGE = u.T
    RPN_BBOX_STD_DEV = np.array(u.STD_DEV)


def _cpu_inputs(name='plain'):
    c = u.draw_case(name)
    return [torch.from_numpy(c[k].copy()) for k in ('anchors', 'gt_class_ids', 'gt_boxes', 'keys')], c


def test_the_wrappers_refuse_what_the_kernels_cannot_take():
    from sdn_hip import ops
    (anchors, ids, boxes, keys), c = _cpu_inputs()
    tail = (u.T, u.STD_DEV)
    A, G = c['A'], c['G']
    # there is no torch form: CPU tensors are an error in every layer
    with pytest.raises(NotImplementedError, match='anchors is on cpu; the RPN targets only run on the GPU'):
        ops.rpn_targets(anchors, ids, boxes, keys, *tail)
    with pytest.raises(NotImplementedError, match='anchors is on cpu'):
        rt.rpn_targets_padded(anchors, ids, boxes, Config, keys=keys)
    with pytest.raises(NotImplementedError):
        rt.build_rpn_targets((128, 128, 3), anchors, ids, boxes, Config, keys=keys)
    with pytest.raises(TypeError, match='keys must be a torch.Tensor'):
        rt.build_rpn_targets((128, 128, 3), anchors, ids, boxes, Config)              # keys=None is only drawn on the device
    with pytest.raises(ValueError, match='config is needed'):
        rt.rpn_targets_padded(anchors, ids, boxes, None, keys=keys)
    # shapes and sizes
    with pytest.raises(ValueError, match=r'anchors must be fp64 \[A, 4\]'):
        ops.rpn_targets(anchors[:, :3], ids, boxes, keys, *tail)
    with pytest.raises(ValueError, match='A = 0; 1 to 16777215'):
        ops.rpn_targets(anchors[:0], ids, boxes, keys[:, :0], *tail)
    with pytest.raises(ValueError, match='G = 0; 1 to 128'):
        ops.rpn_targets(anchors, ids[:0], boxes[:0], keys, *tail)
    with pytest.raises(ValueError, match='G = 129; 1 to 128'):
        ops.rpn_targets(anchors, torch.ones(129, dtype=torch.int32), torch.zeros(129, 4), keys, *tail)
    with pytest.raises(ValueError, match=r'gt_class_ids must be \[G\]'):
        ops.rpn_targets(anchors, ids[None], boxes, keys, *tail)
    with pytest.raises(ValueError, match=r'gt_boxes must be \[G, 4\] = \(%d, 4\)' % G):
        ops.rpn_targets(anchors, ids, boxes[:-1], keys, *tail)
    for bad in (keys[0], keys[:, :-1], keys.t(), torch.zeros(3, A)):
        with pytest.raises(ValueError, match=r'keys must be fp32 \[2, A\] = \(2, %d\)' % A):
            ops.rpn_targets(anchors, ids, boxes, bad, *tail)
    for T in (1, 8193):
        with pytest.raises(ValueError, match='anchors_per_image %d; 2 to 8192' % T):
            ops.rpn_targets(anchors, ids, boxes, keys, T, u.STD_DEV)
    with pytest.raises(ValueError, match='std_dev must hold four values'):
        ops.rpn_targets(anchors, ids, boxes, keys, u.T, (0.1, 0.2))
    with pytest.raises(ValueError, match='std_dev must be positive'):
        ops.rpn_targets(anchors, ids, boxes, keys, u.T, (0.1, 0.1, 0.0, 0.2))
    with pytest.raises(ValueError, match='gt_count must hold one element'):
        ops.rpn_targets(anchors, ids, boxes, keys, *tail, gt_count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='anchors must be contiguous'):
        ops.rpn_targets(anchors.t().contiguous().t(), ids, boxes, keys, *tail)
    # types
    with pytest.raises(TypeError, match='anchors must be torch.float64'):
        ops.rpn_targets(anchors.float(), ids, boxes, keys, *tail)
    with pytest.raises(TypeError, match='keys must be torch.float32'):
        ops.rpn_targets(anchors, ids, boxes, keys.double(), *tail)
    with pytest.raises(TypeError, match='gt_class_ids must be torch.int32 or torch.int64'):
        ops.rpn_targets(anchors, ids.float(), boxes, keys, *tail)
    with pytest.raises(TypeError, match='gt_boxes must be torch.float32 or torch.int32'):
        ops.rpn_targets(anchors, ids, boxes.double(), keys, *tail)
    with pytest.raises(TypeError, match='gt_boxes must be a torch.Tensor'):
        ops.rpn_targets(anchors, ids, boxes.numpy(), keys, *tail)
    with pytest.raises(TypeError, match='gt_count must be torch.int32'):
        ops.rpn_targets(anchors, ids, boxes, keys, *tail, gt_count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match='gt_count must be None or an int32'):
        ops.rpn_targets(anchors, ids, boxes, keys, *tail, gt_count=6)
    with pytest.raises(NotImplementedError, match='anchors is on cpu'):
        ops.rpn_targets(anchors, ids.long(), boxes.int(), keys, *tail, gt_count=torch.zeros(1, dtype=torch.int32))


def test_the_public_names_and_the_docstrings():
    assert list(inspect.signature(rt.build_rpn_targets).parameters) == ['image_shape', 'anchors', 'gt_class_ids', 'gt_boxes', 'config', 'keys']   # model.py:1214
    assert list(inspect.signature(rt.rpn_targets_padded).parameters) == ['anchors', 'gt_class_ids', 'gt_boxes', 'config', 'keys', 'gt_count']
    for fn in (rt.build_rpn_targets, rt.rpn_targets_padded):
        assert inspect.signature(fn).parameters['keys'].default is None
    assert inspect.signature(rt.rpn_targets_padded).parameters['gt_count'].default is None
    from sdn_hip import ops
    assert list(inspect.signature(ops.rpn_targets).parameters) == ['anchors', 'gt_class_ids', 'gt_boxes', 'keys', 'anchors_per_image', 'std_dev',
                                                                   'gt_count']
    doc = ' '.join(rt.__doc__.split())
    assert 'model.py:1214-1322' in doc and 'utils.py:52-89' in doc and 'every anchor\'s maximum counts as 0' in doc
    for d in (ops.rpn_targets.__doc__, rt.__doc__):
        assert 'No result carries a gradient' in ' '.join(d.split())
    from maskrcnn import losses
    text = ' '.join(losses.__doc__.split())
    assert 'maskrcnn.rpn_targets' in text and 'rpn_targets_padded' in text
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'csrc/rpn_targets.hip' in readme and 'profiles/rpn_targets.md' in readme
    assert 'rpn_targets' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'rpn_targets' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
