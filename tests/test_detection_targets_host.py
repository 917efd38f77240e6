"""The detection targets' host half (no GPU): the numpy restatement of tests/detection_targets_util.py against the fixture
tests/golden/detection_targets_golden.npz (what the reference's own functions gave on its own crop_and_resize.c,
tests/golden/make_detection_targets_golden.py), the fixture's margins, the negative count of the check header against Python's
expression, the C entry points' refusals (they run on the arguments alone, before any launch), the python layers' argument errors,
the build's flags and tools/detection_targets_check.cpp under ASan and UBSan."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import detection_targets_util as u
import host_checks
import makefile_rules
from maskrcnn import detection_targets as dt   # the feature itself: without it this module does not import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_detection_targets_workspace_bytes', 'sdn_detection_targets')
RATIOS = (0.33, 0.25, 0.5, 0.1, 1.0)


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    """tools/detection_targets_check.cpp built with ASan and UBSan and run once as a child process: (return code, output)"""
    rc, out = host_checks.run_check_program('detection_targets_check', ['detection_targets_check.h'], tmp_path_factory.mktemp('dt'))
    return rc, out.decode()


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_gives_the_fixtures_numbers(gold, name):
    c = u.draw_case(name)
    p = name + '/'
    for k in u.INPUTS:
        assert u.checksum(c[k]) == int(gold[p + 'crc_' + k]), k                   # the draw is the generator's draw
    mine = u.contract(c, np.float32)
    R, (H, W) = c['R'], c['shape']
    for k in u.OUTPUTS:
        if k not in ('target_mask', 'target_deltas'):
            assert mine[k].dtype == gold[p + k].dtype and mine[k].tobytes() == gold[p + k].tobytes(), k
    # dy, dx are IEEE operations; dh, dw pass through this machine's log, whose last bit differs between CPUs: the fixture's gate
    got, ref = mine['target_deltas'], gold[p + 'target_deltas']
    assert got.dtype == ref.dtype and got[:, :2].tobytes() == ref[:, :2].tobytes()
    err = np.abs(got[:, 2:].astype(np.float64) - ref[:, 2:])
    assert (err <= np.maximum(float(gold[p + 'gate']), 2.0 ** -22 * np.abs(ref[:, 2:].astype(np.float64)))).all(), float(err.max())
    assert mine['target_mask'].tobytes() == u.unpack_masks(gold[p + 'target_mask_bits'], (R, H, W)).tobytes()
    assert mine['rois'].shape == (R, 4) and mine['target_deltas'].shape == (R, 4) and mine['target_mask'].shape == (R, H, W)
    assert all(mine[k].dtype == np.int32 for k in ('target_class_ids', 'rows', 'assign', 'count', 'n_pos'))
    n, P = int(mine['count'][0]), int(mine['n_pos'][0])
    assert 0 <= P <= min(n, int(R * c['ratio'])) and n <= R
    assert (mine['rows'][n:] == -1).all() and (mine['target_class_ids'][n:] == -1).all() and (mine['target_class_ids'][P:n] == 0).all()
    assert (mine['assign'][P:] == -1).all() and (mine['assign'][:P] >= 0).all()
    for k in ('rois', 'target_deltas', 'target_mask'):
        tail = mine[k][P:] if k != 'rois' else mine[k][n:]
        assert tail.tobytes() == np.zeros(tail.shape, np.float32).tobytes(), k    # +0.0, not -0.0


def test_the_fixtures_margins_hold_and_nothing_was_widened(gold):
    for name in u.CASES:
        c = u.draw_case(name)
        p = name + '/'
        mine, exact = u.contract(c, np.float32), u.contract(c, np.float64)
        P = int(mine['n_pos'][0])
        mask_err = float(np.abs(mine['pre_round'].astype(np.float64) - exact['pre_round']).max()) if P else 0.0
        dist = u.half_distance(exact['pre_round'])
        assert mask_err == float(gold[p + 'mask_error']) and dist == float(gold[p + 'half_distance']), name
        assert dist > 4 * mask_err and (name in u.EXPLICIT or dist >= u.DRAW_GATE), (name, dist, mask_err)
        gate, log_err = float(gold[p + 'gate']), float(gold[p + 'log_error'])
        assert gate == 4 * log_err and gate < 1e-5, (name, gate)                  # four times the reference's own error, as measured
        # the restatement's float32 deltas lie inside the gate of its float64 ones: the gate is of the right order
        if P:
            d = np.abs(mine['target_deltas'][:P].astype(np.float64) - exact['target_deltas'][:P])
            assert d[:, 2:].max() <= gate and d.max() < 1e-4, name


def test_the_fixture_holds_what_the_cases_are_there_for(gold):
    cnt = {k: int(gold[k + '/count'][0]) for k in u.CASES}
    pos = {k: int(gold[k + '/n_pos'][0]) for k in u.CASES}
    assert [u.CASES[k]['N'] for k in ('n1', 'n63', 'n64', 'n65', 'n1025', 'n8192')] == [1, 63, 64, 65, 1025, 8192]
    assert {u.CASES[k]['G'] for k in u.CASES} >= {1, 7, 100, 128}
    assert cnt['n1'] == 1 and all(pos[k] == 4 and cnt[k] == 8 for k in ('n63', 'n64', 'n65'))
    assert all(pos[k] == 66 and cnt[k] == 200 for k in ('n1025', 'n8192', 'g100', 'real')) and gold['n1025/rows'][0] == 1024
    assert pos['r1100'] == 550 and cnt['r1100'] == 1100 and pos['ratio_one'] == cnt['ratio_one'] == 32
    assert cnt['none_positive'] == 0 and cnt['only_crowd'] == 0 and cnt['no_negative'] == pos['no_negative'] == 21
    assert 0 < pos['few_positive'] < 21 and cnt['few_positive'] == pos['few_positive'] + u.negative_count(0.33, pos['few_positive']) < 64
    assert pos['few_negative'] == 21 and cnt['few_negative'] < 21 + 42
    z = gold['zero_id_no_crowd/target_class_ids'][:pos['zero_id_no_crowd']]
    assert (z == 0).any() and (z > 0).any()
    assert pos['iou_half'] == 2 and sorted(gold['iou_half/rows'][:2]) == [0, 1]
    t = gold['tie_argmax/assign'][:pos['tie_argmax']]
    assert (t == 0).any() and not (t == 1).any()
    assert gold['roi_count/rows'].max() < 100
    c = u.draw_case('real')
    assert (c['N'], c['G'], c['R'], c['mask'], c['shape']) == (2000, 24, 200, (56, 56), (28, 28))
    assert os.path.getsize(u.GOLD) < 400 * 1024


def test_the_order_of_the_keys_is_their_stable_argsort():
    rs = np.random.RandomState(3)
    keys = np.concatenate([rs.uniform(0, 1, 200), [0.0, -0.0, 0.25, 0.25, 1.0, -1.0, np.inf, -np.inf]]).astype(np.float32)
    rows = np.sort(rs.permutation(len(keys))[:150])
    finite_order = rows[np.argsort(keys[rows] + np.float32(0), kind='stable')]
    mine = u.key_order(keys, rows)
    assert np.array_equal(keys[mine], keys[finite_order])                          # the same keys in the same order ...
    same = keys[mine][1:] == keys[mine][:-1]
    zero_pair = same & (keys[mine][1:] == 0)
    assert (mine[1:][same & ~zero_pair] > mine[:-1][same & ~zero_pair]).all()     # ... equal keys lower row first; -0.0 before +0.0


# ---- the negative count ------------------------------------------------------------------------------------------------------------------
def test_the_negative_count_of_the_header_is_pythons_for_every_p(check_program):
    rc, out = check_program
    table = {}
    for line in out.splitlines():
        if line.startswith('negative_count '):
            _tag, ratio, P, n = line.split()
            table[(float(ratio), int(P))] = int(n)
    assert len(table) == len(RATIOS) * 513
    for ratio in RATIOS:
        cap_max = 0
        for P in range(513):
            r = 1.0 / ratio
            want = int(r * P - P)
            assert table[(ratio, P)] == want == u.negative_count(ratio, P), (ratio, P)
        # the clamp to R - P is idle: for every R the count at P <= int(R * ratio) fits
        for R in range(1, 1025):
            cap = int(R * ratio)
            cap_max = max(cap_max, cap)
            for P in (cap, max(cap - 1, 0), cap // 2):
                assert u.negative_count(ratio, P) <= R - P, (ratio, R, P)
        assert cap_max <= 1024
    assert u.negative_count(0.33, 66) == 134
    assert 'the clamp to R - P is idle' not in out   # only failures are printed


def test_the_check_program_walks_clean_under_asan_and_ubsan(check_program):
    """a stand-alone program with its own main that includes only csrc/detection_targets_check.h; host code on the CPU, never loaded
    into Python"""
    rc, out = check_program
    text = open(os.path.join(ROOT, 'tools', 'detection_targets_check.cpp')).read()
    assert re.findall(r'#include "([^"]+)"', text) == ['detection_targets_check.h'] and 'int main()' in text and 'hip' not in text.lower()
    print('\n'.join(line for line in out.splitlines() if not line.startswith('negative_count ')))
    assert rc == 0 and ' 0 failures' in out and 'the validators' in out


# ---- header, binding, library, build -------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    clause = 'still 20: sdn_detection_targets_workspace_bytes, sdn_detection_targets added'
    assert history.index('sdn_detection_layer added') < history.index(clause) < at
    assert 'model.py:545-724' in history and 'utils.py:92-113' in history
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernels_are_built_exactly_and_use_no_shortcut():
    csrc = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    makefile_rules.assert_built_exactly('detection_targets.hip')
    assert '-ffp-contract=off' in re.search(r'^EXACT\s*:=\s*(.*)$', mk, flags=re.M).group(1) and '-fno-slp-vectorize' in mk
    assert '-fhip-fp32-correctly-rounded-divide-sqrt' in mk
    text = open(os.path.join(csrc, 'detection_targets.hip')).read()
    for h in ('crop_sample.h', 'detection_targets_check.h', 'prop_device.h'):
        assert '#include "%s"' % h in text
    assert 'prop_sort_keys(' in text and 'prop_bitonic_pair(' not in text and 'det_argmax_takes(' in text and 'axis_in(' in text and 'axis_inside(' in text
    assert 'dt_negatives_taken(' in text and 'dt_positive_cap(' in text
    assert 'rintf(' in text and not re.search(r'\broundf\(', text)                 # half to even
    assert 'logf(' in text and not re.search(r'__(logf|expf|fdividef|frcp_r[a-z]|fdiv_r[a-z]|fmaf_r[a-z])\b', text)
    assert not re.search(r'\bf(min|max|ma)f?\(', text)                             # fminf / fmaxf drop NaN, fma contracts
    assert 'atomic' not in text.split('namespace sdn {')[1]                        # no atomics at all
    for word in ('hipLaunchCooperativeKernel', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert word not in text
    assert len(re.findall(r'hipLaunchKernelGGL\(', text)) == 2                     # two dependent launches
    hdr = open(os.path.join(csrc, 'detection_targets_check.h')).read()
    body = hdr[hdr.index('SDN_HD int dt_negative_count'):]
    body = body[:body.index('}')]
    assert 'double' in body and 'float' not in body and re.search(r'r \* \(double\)P;\s*return \(int\)\(product - \(double\)P\);', body)


def test_the_constants_are_mirrored_and_the_workspace_comes_from_the_library():
    from sdn_hip import ops
    hdr = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'detection_targets_check.h')).read()
    assert 'DT_MAX_ROIS = PROP_MAX_PRE_NMS' in hdr and 'DT_MAX_TARGETS = PROP_MAX_PRE_NMS' in hdr
    assert 'DT_MAX_BOXES = 128' in hdr and 'DT_MAX_MASK_SIDE = 64' in hdr
    assert (ops.TARGETS_MAX_ROIS, ops.TARGETS_MAX_PER_IMAGE, ops.TARGETS_MAX_BOXES, ops.TARGETS_MAX_MASK_SIDE) == \
        (u.MAX_ROIS, u.MAX_TARGETS, u.MAX_BOXES, u.MAX_MASK_SIDE) == (8192, 8192, 128, 64)
    for R in (1, 3, 200, 8192):
        assert ops.detection_targets_workspace_bytes(2000, 24, 56, 56, R, 28, 28) == 16 * R


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _call(proposals=FAKE, ids=FAKE, boxes=FAKE, masks=FAKE, keys=FAKE, N=2000, G=24, mh=56, mw=56, ids64=0, roi_count=None, R=200, ratio=0.33,
          std=(0.1, 0.1, 0.2, 0.2), H=28, W=28, mini=1, rois=FAKE, cls=FAKE, deltas=FAKE, mask=FAKE, rows=FAKE, assign=FAKE, count=FAKE,
          n_pos=FAKE, ws=FAKE, ws_bytes=1 << 20):
    import sdn_hip
    L = sdn_hip.lib()
    s = None if std is None else (ctypes.c_float * 4)(*std)
    rc = L.sdn_detection_targets(proposals, ids, boxes, masks, keys, N, G, mh, mw, ids64, roi_count, R, ratio, s, H, W, mini, rois, cls, deltas,
                                 mask, rows, assign, count, n_pos, ws, ws_bytes, None)
    return rc, L.sdn_last_error().decode()


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    null_in = 'proposals, gt_class_ids, gt_boxes, gt_masks or keys is NULL'
    null_out = 'rois, target_class_ids, target_deltas or target_mask is NULL'
    null_idx = 'rows, assign, count or n_pos is NULL'
    for kw, reason in ((dict(N=0), 'N 0; 1 to 8192'), (dict(N=8193), 'N 8193; 1 to 8192'), (dict(G=0), 'G 0; 1 to 128'), (dict(G=129), 'G 129'),
                       (dict(mh=0), 'masks 0 x 56'), (dict(mw=-3), 'masks 56 x -3'), (dict(R=0), 'R 0; 1 to 8192'), (dict(R=8193), 'R 8193'),
                       (dict(H=0), 'mask shape 0 x 28'), (dict(W=65), 'mask shape 28 x 65'), (dict(ratio=0.0), 'positive ratio 0'),
                       (dict(ratio=1.25), 'positive ratio 1.25'), (dict(ratio=float('nan')), 'positive ratio'), (dict(std=None), 'std_dev is NULL'),
                       (dict(std=(0.1, 0.1, 0.0, 0.2)), 'std_dev[2] is 0'),
                       (dict(proposals=None), null_in), (dict(ids=None), null_in), (dict(boxes=None), null_in), (dict(masks=None), null_in),
                       (dict(keys=None), null_in), (dict(rois=None), null_out), (dict(cls=None), null_out), (dict(deltas=None), null_out),
                       (dict(mask=None), null_out), (dict(rows=None), null_idx), (dict(assign=None), null_idx), (dict(count=None), null_idx),
                       (dict(n_pos=None), null_idx), (dict(ws=None), 'workspace is NULL'), (dict(ws_bytes=0), 'workspace 0 < 3200 bytes'),
                       (dict(ws_bytes=3199), 'workspace 3199 < 3200 bytes'),
                       (dict(keys=FAKE + 2), 'aligned to 4 bytes'), (dict(ids=FAKE + 2), 'gt_class_ids must be aligned to 4 bytes'),
                       (dict(ids=FAKE + 4, ids64=1), 'gt_class_ids must be aligned to 8 bytes'),
                       (dict(roi_count=FAKE + 1), 'roi_count must be aligned to 4 bytes'), (dict(assign=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(rois=FAKE + 4), 'aligned to 16 bytes'), (dict(deltas=FAKE + 8), 'aligned to 16 bytes'), (dict(ws=FAKE + 4), 'aligned to 16 bytes')):
        rc, msg = _call(**kw)
        assert rc == -1 and msg.startswith('sdn_detection_targets: ') and reason in msg, (kw, msg)


def test_the_workspace_query_checks_its_arguments():
    import sdn_hip
    L = sdn_hip.lib()
    n = ctypes.c_size_t(0)
    assert L.sdn_detection_targets_workspace_bytes(2000, 24, 56, 56, 200, 28, 28, ctypes.byref(n)) == 0 and n.value == 3200
    assert L.sdn_detection_targets_workspace_bytes(2000, 24, 56, 56, 200, 28, 28, None) == -1
    for args in ((0, 24, 56, 56, 200, 28, 28), (8193, 24, 56, 56, 200, 28, 28), (10, 0, 56, 56, 200, 28, 28), (10, 129, 56, 56, 200, 28, 28),
                 (10, 3, 0, 56, 200, 28, 28), (10, 3, 56, 56, 0, 28, 28), (10, 3, 56, 56, 8193, 28, 28), (10, 3, 56, 56, 200, 65, 28),
                 (10, 3, 56, 56, 200, 28, 0)):
        assert L.sdn_detection_targets_workspace_bytes(*args, ctypes.byref(n)) == -1, args
        assert L.sdn_last_error().decode().startswith('sdn_detection_targets_workspace_bytes: ')


# ---- the python layers ---------------------------------------------------------------------------------------------------------------------
class Config(object):
    BBOX_STD_DEV = np.array(u.STD_DEV)

    def __init__(self, c):
        self.TRAIN_ROIS_PER_IMAGE, self.ROI_POSITIVE_RATIO = c['R'], c['ratio']
        self.USE_MINI_MASK, self.MASK_SHAPE = c['mini'], list(c['shape'])


def _cpu_inputs(name='few_positive'):
    c = u.draw_case(name)
    return [torch.from_numpy(c[k].copy()) for k in u.INPUTS], c


def test_the_wrappers_refuse_what_the_kernels_cannot_take():
    from sdn_hip import ops
    (proposals, ids, boxes, masks, keys), c = _cpu_inputs()
    cfg = Config(c)
    tail = (c['R'], c['ratio'], c['std_dev'], c['shape'])
    # there is no torch form: CPU tensors are an error in every layer
    with pytest.raises(NotImplementedError, match='proposals is on cpu; the detection targets only run on the GPU'):
        ops.detection_targets(proposals, ids, boxes, masks, keys, *tail)
    with pytest.raises(NotImplementedError, match='proposals is on cpu'):
        dt.detection_targets_padded(proposals[None], ids[None], boxes[None], masks[None], cfg, keys=keys)
    with pytest.raises(NotImplementedError):
        dt.detection_target_layer(proposals[None], ids[None], boxes[None], masks[None], cfg, keys=keys)
    with pytest.raises(TypeError, match='keys must be a torch.Tensor'):
        dt.detection_target_layer(proposals, ids, boxes, masks, cfg)              # keys=None is only drawn on the device
    with pytest.raises(ValueError, match=r'proposals has batch 2; only 1 is supported.*model\.py:570'):
        dt.detection_targets_padded(torch.stack([proposals, proposals]), ids, boxes, masks, cfg, keys=keys)
    with pytest.raises(ValueError, match='config is needed'):
        dt.detection_targets_padded(proposals, ids, boxes, masks, None, keys=keys)
    # shapes and sizes
    with pytest.raises(ValueError, match=r'proposals must be fp32 \[N, 4\]'):
        ops.detection_targets(proposals[:, :3], ids, boxes, masks, keys, *tail)
    with pytest.raises(ValueError, match='N = 0; 1 to 8192'):
        ops.detection_targets(proposals[:0], ids, boxes, masks, keys[:, :0], *tail)
    with pytest.raises(ValueError, match='N = 8193; 1 to 8192'):
        ops.detection_targets(torch.zeros(8193, 4), ids, boxes, masks, torch.zeros(2, 8193), *tail)
    with pytest.raises(ValueError, match='G = 0; 1 to 128'):
        ops.detection_targets(proposals, ids[:0], boxes[:0], masks[:0], keys, *tail)
    with pytest.raises(ValueError, match='G = 129; 1 to 128'):
        ops.detection_targets(proposals, torch.ones(129, dtype=torch.int32), torch.zeros(129, 4), torch.zeros(129, 4, 4), keys, *tail)
    with pytest.raises(ValueError, match=r'gt_class_ids must be \[G\]'):
        ops.detection_targets(proposals, ids[None], boxes, masks, keys, *tail)
    with pytest.raises(ValueError, match=r'gt_boxes must be fp32 \[G, 4\] = \(7, 4\)'):
        ops.detection_targets(proposals, ids, boxes[:-1], masks, keys, *tail)
    with pytest.raises(ValueError, match=r'gt_masks must be fp32 \[G, mh, mw\] with G = 7'):
        ops.detection_targets(proposals, ids, boxes, masks[:-1], keys, *tail)
    for bad in (keys[0], keys[:, :-1], keys.t(), torch.zeros(3, c['N'])):
        with pytest.raises(ValueError, match=r'keys must be fp32 \[2, N\] = \(2, 200\)'):
            ops.detection_targets(proposals, ids, boxes, masks, bad, *tail)
    for R in (0, 8193):
        with pytest.raises(ValueError, match='rois_per_image %d; 1 to 8192' % R):
            ops.detection_targets(proposals, ids, boxes, masks, keys, R, *tail[1:])
    for ratio in (0.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match=r'positive_ratio .*; it must lie in \(0, 1\]'):
            ops.detection_targets(proposals, ids, boxes, masks, keys, c['R'], ratio, *tail[2:])
    with pytest.raises(ValueError, match='std_dev must hold four values'):
        ops.detection_targets(proposals, ids, boxes, masks, keys, c['R'], c['ratio'], (0.1, 0.2), c['shape'])
    with pytest.raises(ValueError, match='std_dev must be positive'):
        ops.detection_targets(proposals, ids, boxes, masks, keys, c['R'], c['ratio'], (0.1, 0.1, 0.0, 0.2), c['shape'])
    for shape in ((0, 14), (14, 65), (14,), (14, 14, 1)):
        with pytest.raises(ValueError, match='mask_shape .*; two sides of 1 to 64'):
            ops.detection_targets(proposals, ids, boxes, masks, keys, c['R'], c['ratio'], c['std_dev'], shape)
    with pytest.raises(ValueError, match='roi_count must hold one element'):
        ops.detection_targets(proposals, ids, boxes, masks, keys, *tail, roi_count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='gt_masks must be contiguous'):
        ops.detection_targets(proposals, ids, boxes, masks.transpose(1, 2).contiguous().transpose(1, 2), keys, *tail)
    with pytest.raises(ValueError, match='proposals must be contiguous'):
        ops.detection_targets(proposals.t().contiguous().t(), ids, boxes, masks, keys, *tail)
    # types
    with pytest.raises(TypeError, match='proposals must be torch.float32'):
        ops.detection_targets(proposals.double(), ids, boxes, masks, keys, *tail)
    with pytest.raises(TypeError, match='gt_masks must be torch.float32'):
        ops.detection_targets(proposals, ids, boxes, masks.bool(), keys, *tail)
    with pytest.raises(TypeError, match='keys must be torch.float32'):
        ops.detection_targets(proposals, ids, boxes, masks, keys.double(), *tail)
    with pytest.raises(TypeError, match='gt_class_ids must be torch.int32 or torch.int64'):
        ops.detection_targets(proposals, ids.float(), boxes, masks, keys, *tail)
    with pytest.raises(TypeError, match='gt_boxes must be a torch.Tensor'):
        ops.detection_targets(proposals, ids, boxes.numpy(), masks, keys, *tail)
    with pytest.raises(TypeError, match='roi_count must be torch.int32'):
        ops.detection_targets(proposals, ids, boxes, masks, keys, *tail, roi_count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match='roi_count must be None or an int32'):
        ops.detection_targets(proposals, ids, boxes, masks, keys, *tail, roi_count=100)
    with pytest.raises(NotImplementedError, match='proposals is on cpu'):
        ops.detection_targets(proposals, ids.long(), boxes, masks, keys, *tail, roi_count=torch.zeros(1, dtype=torch.int32))


def test_the_public_names_and_the_docstrings():
    assert list(inspect.signature(dt.detection_target_layer).parameters) == ['proposals', 'gt_class_ids', 'gt_boxes', 'gt_masks', 'config', 'keys']   # model.py:545
    assert list(inspect.signature(dt.detection_targets_padded).parameters) == ['proposals', 'gt_class_ids', 'gt_boxes', 'gt_masks', 'config', 'keys',
                                                                               'roi_count']
    for fn in (dt.detection_target_layer, dt.detection_targets_padded):
        assert inspect.signature(fn).parameters['keys'].default is None
    assert inspect.signature(dt.detection_targets_padded).parameters['roi_count'].default is None
    from sdn_hip import ops
    assert list(inspect.signature(ops.detection_targets).parameters) == ['proposals', 'gt_class_ids', 'gt_boxes', 'gt_masks', 'keys', 'rois_per_image',
                                                                         'positive_ratio', 'std_dev', 'mask_shape', 'use_mini_mask', 'roi_count']
    doc = ' '.join(dt.detection_target_layer.__doc__.split())
    assert 'model.py:545-724' in doc and 'only host wait' in doc and ':1803' in doc
    for d in (ops.detection_targets.__doc__, dt.__doc__):
        assert 'No result carries a gradient' in ' '.join(d.split())
    from maskrcnn import losses
    text = ' '.join(losses.__doc__.split())
    assert 'detection_target_layer' in text and 'maskrcnn.detection_targets' in text and 'build_rpn_targets stay the caller' in text
