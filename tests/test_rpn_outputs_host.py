"""The host half (no GPU) of the fused RPN outputs and of maskrcnn.predict: the entry points in header, binding and library, the
mirrored constants, the C entry points' refusals (they run on the arguments alone, before any launch), the python layers' argument
errors, tools/rpn_outputs_check.cpp under ASan and UBSan, the torch restatement's index map against explicit loops, and the
conditions the stand-in network's fixture (tests/predict_util.py) must meet, checked with the numpy restatements of the decision
layers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import detection_layer_util as dlu
import host_checks
import makefile_rules
import predict_util as u
import proposal_layer_util as plu
from maskrcnn import predict as pr          # the feature itself: without it this module does not import
from sdn_hip import ops
from sdn_hip.ops import rpn_outputs         # noqa: F401  (likewise)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_rpn_outputs_fwd', 'sdn_rpn_outputs_bwd')
CSRC = os.path.join(ROOT, '3d-sdn_amd', 'csrc')


def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    assert history.index('sdn_training_item added') < history.index('sdn_rpn_outputs_fwd, sdn_rpn_outputs_bwd added') < at
    for line in ('model.py:896-911', ':897-899', ':909-911', ':1729-1740'):       # the reference lines the entry points replace
        assert line in history, line
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernel_file_is_built_like_its_neighbours_and_uses_no_atomics():
    makefile_rules.assert_built_exactly('rpn_outputs.hip')
    text = open(os.path.join(CSRC, 'rpn_outputs.hip')).read()
    assert '#include "rpn_outputs_check.h"' in text
    code = text.split('namespace sdn {')[1]
    assert 'atomic' not in code and 'hipMemset' not in code and 'hipMemcpy' not in code and 'Synchronize' not in code
    assert len(re.findall(r'\bexpf\(', code)) == 2 and not re.search(r'__(expf|fdividef|frcp_r[a-z]|fdiv_r[a-z])\b', code)
    assert not re.search(r'\bf(min|max)f\(', code)                                 # they drop a NaN: the maximum is a comparison
    assert len(re.findall(r'hipLaunchKernelGGL\(', text)) == 2                     # one launch each way


def test_the_constants_are_mirrored():
    const = lambda name: host_checks.constexpr_int('rpn_outputs_check.h', name)   # noqa: E731
    assert ops.RPN_OUTPUTS_MAX_LEVELS == const('RPO_MAX_LEVELS') == 8 and ops.RPN_OUTPUTS_MAX_K == const('RPO_MAX_K') == 16
    assert ops.RPN_OUTPUTS_TILE == const('RPO_TILE') == 64 and ops.RPN_OUTPUTS_MAX_BATCH == const('RPO_MAX_BATCH') == 65535


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _ptrs(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


def _ints(values):
    return None if values is None else (ctypes.c_int * len(values))(*values)


H5, W5 = (32, 16, 8, 4, 2), (32, 16, 8, 4, 2)


def _fwd(cls=(FAKE,) * 5, box=(FAKE,) * 5, H=H5, W=W5, L=5, k=3, B=1, logits=FAKE, probs=FAKE, bbox=FAKE):
    import sdn_hip
    lib = sdn_hip.lib()
    rc = lib.sdn_rpn_outputs_fwd(_ptrs(cls), _ptrs(box), _ints(H), _ints(W), L, k, B, logits, probs, bbox, None)
    return rc, lib.sdn_last_error().decode()


def _bwd(g_logits=FAKE, g_probs=FAKE, g_bbox=FAKE, probs=FAKE, H=H5, W=W5, L=5, k=3, B=1, g_cls=(FAKE,) * 5, g_box=(FAKE,) * 5):
    import sdn_hip
    lib = sdn_hip.lib()
    rc = lib.sdn_rpn_outputs_bwd(g_logits, g_probs, g_bbox, probs, _ints(H), _ints(W), L, k, B, _ptrs(g_cls), _ptrs(g_box), None)
    return rc, lib.sdn_last_error().decode()


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    hole, bent = (FAKE, FAKE, None, FAKE, FAKE), (FAKE, FAKE, FAKE, FAKE + 2, FAKE)
    null_out = 'rpn_class_logits, rpn_probs or rpn_bbox is NULL'
    for kw, reason in ((dict(L=0), 'L 0; 1 to 8 levels'), (dict(L=9), 'L 9; 1 to 8'), (dict(L=-2), 'L -2'), (dict(k=0), 'k 0; 1 to 16 anchors'),
                       (dict(k=17), 'k 17; 1 to 16'), (dict(B=0), 'B 0; 1 to 65535'), (dict(B=65536), 'B 65536'),
                       (dict(H=None), 'H or W is NULL'), (dict(W=None), 'H or W is NULL'), (dict(H=(32, 0, 8, 4, 2)), 'level 1 is 0 x 16'),
                       (dict(W=(32, 16, 8, 4, -1)), 'level 4 is 2 x -1'),
                       (dict(H=(1 << 16,), W=(1 << 16,), L=1, k=1), 'H * W = 4294967296 must stay below 2^31'),
                       (dict(H=(1 << 14,), W=(1 << 14,), L=1, k=2), 'B * A * 4 = 2147483648 must stay below 2^31'),
                       (dict(H=(1 << 14,), W=(1 << 14,), L=1, k=1, B=2), 'must stay below 2^31'),
                       (dict(cls=None), 'class_maps is NULL'), (dict(box=None), 'bbox_maps is NULL'), (dict(cls=hole), 'class_maps[2] is NULL'),
                       (dict(box=hole), 'bbox_maps[2] is NULL'), (dict(cls=bent), 'class_maps[3] must be aligned to 4 bytes'),
                       (dict(box=bent), 'bbox_maps[3] must be aligned to 4 bytes'),
                       (dict(logits=None), null_out), (dict(probs=None), null_out), (dict(bbox=None), null_out),
                       (dict(logits=FAKE + 4), 'aligned to 16 bytes'), (dict(probs=FAKE + 8), 'aligned to 16 bytes'),
                       (dict(bbox=FAKE + 4), 'aligned to 16 bytes')):
        rc, msg = _fwd(**kw)
        assert rc == -1 and msg.startswith('sdn_rpn_outputs_fwd: ') and reason in msg, (kw, msg)
    for kw, reason in ((dict(L=9), 'L 9'), (dict(k=0), 'k 0'), (dict(B=0), 'B 0'), (dict(H=None), 'H or W is NULL'),
                       (dict(probs=None), 'rpn_probs is NULL although grad_probs is given'),
                       (dict(g_logits=FAKE + 2), 'aligned to 4 bytes'), (dict(g_probs=FAKE + 1), 'aligned to 4 bytes'),
                       (dict(g_bbox=FAKE + 2), 'aligned to 4 bytes'), (dict(probs=FAKE + 2), 'aligned to 4 bytes'),
                       (dict(g_cls=None), 'grad_class_maps is NULL'), (dict(g_box=None), 'grad_bbox_maps is NULL'),
                       (dict(g_cls=hole), 'grad_class_maps[2] is NULL'), (dict(g_box=bent), 'grad_bbox_maps[3] must be aligned to 4 bytes')):
        rc, msg = _bwd(**kw)
        assert rc == -1 and msg.startswith('sdn_rpn_outputs_bwd: ') and reason in msg, (kw, msg)


def test_the_wrappers_refuse_what_the_kernels_cannot_take():
    cls, box = u.draw_maps([(4, 6), (2, 3)], 3, 1, seed=1)
    # there is no torch form: CPU tensors are an error in every layer
    with pytest.raises(NotImplementedError, match=r'class_maps\[0\] is on cpu; the RPN output kernels only run on the GPU'):
        ops.rpn_outputs(cls, box)
    with pytest.raises(NotImplementedError):
        pr.rpn_outputs(cls, box)
    # types
    with pytest.raises(TypeError, match=r'bbox_maps\[1\] must be torch.float32'):
        ops.rpn_outputs(cls, [box[0], box[1].double()])
    with pytest.raises(TypeError, match=r'class_maps\[0\] must be torch.float32'):
        ops.rpn_outputs([cls[0].half(), cls[1]], box)
    with pytest.raises(TypeError, match=r'class_maps\[1\] must be a torch.Tensor'):
        ops.rpn_outputs([cls[0], cls[1].numpy()], box)
    with pytest.raises(TypeError, match='sequences of tensors'):
        ops.rpn_outputs(3, box)
    # shapes and sizes
    with pytest.raises(ValueError, match='2 class maps and 1 box maps'):
        ops.rpn_outputs(cls, box[:1])
    with pytest.raises(ValueError, match='0 class maps and 0 box maps; 1 to 8 levels'):
        ops.rpn_outputs([], [])
    with pytest.raises(ValueError, match='9 class maps'):
        ops.rpn_outputs([cls[0]] * 9, [box[0]] * 9)
    with pytest.raises(ValueError, match=r'class_maps\[0\] must be fp32 \[B, channels, H, W\]'):
        ops.rpn_outputs([cls[0][0], cls[1]], box)
    with pytest.raises(ValueError, match='without an empty axis'):
        ops.rpn_outputs([cls[0][:, :, :0], cls[1]], box)
    with pytest.raises(ValueError, match=r'class_maps\[0\] has 5 channels; 2k with k = 1 to 16'):
        ops.rpn_outputs([cls[0][:, :5].contiguous(), cls[1]], box)
    with pytest.raises(ValueError, match='has 34 channels'):
        ops.rpn_outputs([torch.zeros(1, 34, 2, 2)], [torch.zeros(1, 68, 2, 2)])
    with pytest.raises(ValueError, match=r'class_maps\[1\] must be \[1, 6, H, W\]'):
        ops.rpn_outputs([cls[0], cls[1][:, :4].contiguous()], box)
    with pytest.raises(ValueError, match=r'bbox_maps\[1\] must be \[1, 12, 2, 3\]'):
        ops.rpn_outputs(cls, [box[0], box[0]])
    with pytest.raises(ValueError, match=r'bbox_maps\[0\] must be \[1, 12, 4, 6\]'):
        ops.rpn_outputs(cls, [torch.cat([box[0], box[0]]), box[1]])
    with pytest.raises(ValueError, match=r'class_maps\[0\] must be contiguous'):
        ops.rpn_outputs([cls[0].transpose(2, 3).contiguous().transpose(2, 3), cls[1]], box)
    with pytest.raises(ValueError, match=r'must stay below 2\^31'):
        big = torch.zeros(1).expand(1, 2, 1 << 14, 1 << 15)
        ops.rpn_outputs([big], [torch.zeros(1).expand(1, 4, 1 << 14, 1 << 15)])


def test_predict_refuses_a_batch_and_a_cpu_model():
    model = u.StandIn()
    frame = u.painted_frame()
    with pytest.raises(ValueError, match=r'batch 2; only 1 is supported.*model\.py:358'):
        pr.predict_padded(model, [torch.cat([u.molded(frame)] * 2), u.image_metas()], 'inference')
    with pytest.raises(NotImplementedError, match='molded_images is on cpu; predict only runs on the GPU'):
        pr.predict_padded(model, [u.molded(frame), u.image_metas()], 'inference')
    with pytest.raises(NotImplementedError):
        pr.predict(model, u.training_input(frame, 'cpu'), 'training')
    with pytest.raises(NotImplementedError, match='model.anchors must be on the device'):
        pr.use_device_predict(model)
    with pytest.raises(NotImplementedError):
        pr.detect(model, [torch.from_numpy(frame)])
    with pytest.raises(TypeError, match='must be an nn.Module'):
        pr.use_device_predict(object())
    with pytest.raises(ValueError, match='has no attribute fpn'):
        pr.use_device_predict(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match='molded_images must be a torch.Tensor'):
        pr.predict_padded(model, [frame, u.image_metas()], 'inference')


def test_the_public_names_and_the_docstrings():
    assert list(inspect.signature(pr.predict).parameters)[:3] == ['model', 'input', 'mode']            # model.py:1705
    assert list(inspect.signature(pr.predict_padded).parameters) == ['model', 'input', 'mode', 'keys']
    assert list(inspect.signature(pr.rpn_forward).parameters) == ['rpn', 'feature_maps']
    assert list(inspect.signature(pr.classifier_head).parameters) == ['classifier', 'maps', 'rois']
    assert list(inspect.signature(pr.mask_head).parameters) == ['mask', 'maps', 'rois']
    assert list(inspect.signature(pr.detect).parameters) == ['model', 'frames_u8']
    assert list(inspect.signature(ops.rpn_outputs).parameters) == ['class_maps', 'bbox_maps']
    doc = ' '.join(pr.__doc__.split())
    for words in ('Out of scope', 'fusing the two 1 x 1 convs', 'half precision', 'generate_inst_map', "train_epoch's optimizer loop",
                  'the id selection of load_mask', 'gt_boxes / scale', 'model.py:1705-1821'):
        assert words in doc, words


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_table_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/rpn_outputs_check.cpp: a stand-alone program with its own main that includes only csrc/rpn_outputs_check.h; host code on
    the CPU, never loaded into Python"""
    # the header stands alone: no other operation's header, only the macros every check header shares (plain C++ as well)
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, 'rpn_outputs_check.h')).read()) == ['check_common.h']
    assert not re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, 'check_common.h')).read())
    rc, out = host_checks.run_check_program('rpn_outputs_check', ['rpn_outputs_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out and b'the validators' in out


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_restatements_index_map_is_the_explicit_loop():
    """two levels, k = 3, batch 2: permute / view / cat put every map element where include/sdn_hip.h says"""
    cls, box = u.draw_maps([(3, 5), (2, 3)], 3, 2, seed=4)
    logits, probs, boxes = u.rpn_tail(cls, box)
    want_logits, _none, want_boxes = u.index_loop([c.numpy() for c in cls], [b.numpy() for b in box])
    assert logits.shape == (2, 3 * (15 + 6), 2) and boxes.shape == (2, 3 * (15 + 6), 4)
    assert logits.numpy().tobytes() == want_logits.tobytes() and boxes.numpy().tobytes() == want_boxes.tobytes()
    x = want_logits.astype(np.float64)
    e = np.exp(x - x.max(axis=2, keepdims=True))
    assert np.abs(probs.numpy() - e / e.sum(axis=2, keepdims=True)).max() < 2.0 ** -22
    cls64, box64 = [c.double() for c in cls], [b.double() for b in box]
    assert u.rpn_tail(cls64, box64)[1].dtype == torch.float64
    # the second level starts at anchor k * H_0 * W_0; anchor (y * W + x) * k + a, component j, is channel a * 2 + j (boxes: a * 4 + j)
    assert logits[1, 45 + (1 * 3 + 2) * 3 + 1, 1] == cls[1][1, 1 * 2 + 1, 1, 2] and boxes[0, (2 * 5 + 4) * 3 + 2, 3] == box[0][0, 2 * 4 + 3, 2, 4]


# ---- the stand-in's fixture -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def chain():
    return u.cpu_chain(u.StandIn(), u.painted_frame())


def test_the_stand_in_has_the_reference_s_names_and_its_anchors_are_the_librarys():
    model = u.StandIn()
    assert model.anchors.shape == (3 * (1024 + 256 + 64 + 16 + 4), 4) and model.anchors.dtype == torch.float32
    for name in ('fpn', 'rpn', 'classifier', 'mask', 'anchors', 'config'):
        assert hasattr(model, name)
    for name in ('padding', 'conv_shared', 'relu', 'conv_class', 'conv_bbox'):
        assert hasattr(model.rpn, name)
    anchors = u.anchors64()
    for box in u.GT_BOXES:                                   # every ground-truth box IS an anchor
        assert (anchors == box.astype(np.float64)).all(axis=1).sum() == 1
    assert len(model.state_dict()) > 40 and 'anchors' not in model.state_dict()


def test_the_fixture_makes_the_decision_layers_work(chain):
    cfg = u.config()
    for mode, P in (('training', cfg.POST_NMS_ROIS_TRAINING), ('inference', cfg.POST_NMS_ROIS_INFERENCE)):
        c, got = chain[mode + '_proposals']
        assert len(got['keep']) == P and c['K'] == c['anchors'].shape[0] == 4092
        assert got['keep'][-1] > P                                                  # the NMS suppressed some boxes on the way
        assert plu.near_pairs(got['boxes'], c['thr']) == []                         # no pair within 1e-5 of the RPN's NMS threshold
        best = got['boxes'][got['keep'][:3]]
        for box in u.GT_BOXES:                                                      # the three best proposals are the painted squares
            assert np.abs(best - box).max(axis=1).min() < 1.0
    t, (pos, neg, assign) = chain['targets']
    assert len(pos) >= 2 and len(neg) >= 1 and len(pos) < len(pos) + len(neg) < t['R']     # n_pos < count < R: padding behind the count
    assert len(set(assign.tolist())) >= 2
    d, got = chain['detections']
    n = int(got['count'][0])
    assert n >= 2 and set(got['detections'][:n, 4].astype(int).tolist()) == {1, 2}
    assert (got['detections'][:n, 5] >= np.float32(cfg.DETECTION_MIN_CONFIDENCE)).all()
    class_ids, _scores, pre, valid = dlu.rows_of(d)
    boxes32 = np.rint(pre)
    assert valid.sum() > n                                                          # the per-class NMS suppressed some rows
    rows = np.nonzero(valid)[0]
    for cls in (1, 2):                                                              # no same-class pair within 1e-5 of the threshold
        mine = rows[class_ids[rows] == cls]
        assert plu.near_pairs(boxes32[mine], d['thr']) == [], cls
    for box in u.GT_BOXES:
        assert np.abs(got['detections'][:n, :4] - box).max(axis=1).min() <= 2.0


def test_a_frame_without_squares_has_no_positive():
    out = u.cpu_chain(u.StandIn(), u.painted_frame(squares=()))
    _t, (pos, neg, _assign) = out['targets']
    assert len(pos) == 0 and len(neg) == 0
