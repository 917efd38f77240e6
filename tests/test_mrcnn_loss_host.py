"""The Mask R-CNN training losses without a GPU: the float64 restatement of tests/mrcnn_loss_util.py against the fixture
tests/golden/mrcnn_loss_golden.npz (the reference's own functions, run by tests/golden/make_mrcnn_loss_golden.py), the entry
points' names in header, binding and library, the build list, the constants the Python side mirrors, the argument checks of
sdn_mrcnn_loss_fwd / _bwd and of the binding, all of which run before any launch, and the header's arithmetic under ASan and UBSan
in a stand-alone host program."""
import ctypes
import os

import numpy as np
import pytest
import torch

import host_checks
import makefile_rules
import mrcnn_loss_util as u
from maskrcnn import losses   # the feature itself: without it this module does not import

NAMES = ('sdn_mrcnn_loss_workspace_bytes', 'sdn_mrcnn_loss_fwd', 'sdn_mrcnn_loss_bwd')


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_restatement_gives_the_references_numbers(gold, name):
    c = u.draw_case(name)
    p = name + '/'
    for k in u.INPUTS:
        assert int(gold[p + 'crc_' + k]) == u.checksum(c[k]), k
        if name in u.STORED_WHOLE:
            assert gold[p + k].dtype == c[k].dtype and np.array_equal(gold[p + k], c[k]), k
    r = u.reference(c)
    for k in u.LOSSES:
        want = float(gold[p + k])
        assert (np.isnan(want) and np.isnan(r[k])) or abs(r[k] - want) <= 1e-13 * max(abs(want), 1.0), (k, r[k], want)
    for k in u.COUNTS:
        assert r[k] == int(gold[p + k]), k
    for k in u.PREDICTIONS:
        g = r['grad'][k]
        if g is None:
            assert p + 'grad_idx_' + k not in gold.files
            continue
        want = u.dense(gold[p + 'grad_idx_' + k], gold[p + 'grad_val_' + k], g.shape)
        assert np.allclose(g, want, rtol=1e-11, atol=1e-300), k
        assert not want[~r['selected'][k]].any(), k       # exact zeros outside the selection


def test_the_fixture_holds_what_the_cases_are_there_for(gold):
    assert os.path.getsize(u.GOLD) < 400 * 1024
    assert np.array_equal(gold['weights'], u.WEIGHTS) and len(set(u.WEIGHTS)) == 6
    assert all(float(np.float32(w)) == w for w in u.WEIGHTS)
    for name in u.CASES:
        # the gate: the sibling's 1e-6, or four times what torch's own float32 run is off where that is more
        err, gate = float(gold[name + '/fp32_error']), float(gold[name + '/gate'])
        assert gate == (u.GATE if err <= u.GATE else 4 * err), name
    ch = u.draw_case('chunks')
    m = ch['rpn_match'].reshape(-1)
    assert len(m) % 4 and len(m) > 4 * u.CHUNK and m[0] == 1 and m[-1] == 1 and m.dtype == np.int32
    assert all(m[e - 1] == 1 and m[e] == 1 for e in (u.QUAD, u.STEP, u.CHUNK, 2 * u.CHUNK, 4 * u.CHUNK))
    ex = u.draw_case('exact')
    assert int(gold['exact/n_rpn_pos']) == ex['rpn_bbox'].shape[1] == int((ex['rpn_match'] == 1).sum())
    assert ex['rpn_match'].dtype == np.int64 and ex['target_class_ids'].dtype == np.int64
    assert {u.CASES[n]['R'] for n in u.CASES} >= {0, 1, 13, 200} and {u.CASES[n]['C'] for n in u.CASES} >= {2, 3, 81}
    assert {(u.CASES[n]['h'], u.CASES[n]['w']) for n in u.CASES} >= {(28, 28), (5, 7)}
    assert np.isnan(gold['nopos/rpn_bbox_loss']) and np.isnan(gold['novalid/rpn_class_loss']) and np.isnan(gold['novalid/mrcnn_mask_loss'])
    assert int(gold['novalid/n_roi_pos']) == 0 and int(gold['novalid/n_rpn_valid']) == 0
    assert [float(gold['empty/' + k]) for k in u.LOSSES[2:5]] == [0.0, 0.0, 0.0]
    # the saturated probabilities: 1 / floor on two of the four planted elements, exact 0 on the others
    ids = ch['target_class_ids']
    g = u.dense(gold['chunks/grad_idx_mrcnn_mask'], gold['chunks/grad_val_mrcnn_mask'], ch['mrcnn_mask'].shape)[0, ids[0], 0, :4]
    assert g[0] == 0.0 and g[3] == 0.0 and g[1] > 1e6 and g[2] < -1e6


def test_what_the_reference_leaves_undefined_is_left_out_and_counted():
    c = u.draw_case('chunks')
    base = u.reference(c)
    d = {k: v.copy() for k, v in c.items()}
    d['rpn_match'][0, 10, 0], d['rpn_match'][0, 2000, 0] = 2, -7       # both neutral before
    assert c['rpn_match'][0, 10, 0] == 0 and c['rpn_match'][0, 2000, 0] == 0
    r = u.reference(d)
    assert r['bad'] == 2 and all(r[k] == base[k] for k in u.LOSSES)
    d = {k: v.copy() for k, v in c.items()}
    d['rpn_bbox'] = c['rpn_bbox'][:, :10]
    r = u.reference(d)
    assert r['bad'] == base['n_rpn_pos'] - 10 and r['n_rpn_pos'] == 10 and r['rpn_class_loss'] == base['rpn_class_loss']
    d = {k: v.copy() for k, v in c.items()}
    d['target_class_ids'][2], d['target_class_ids'][5] = 3, -1
    r = u.reference(d)
    keep = np.ones(13, bool)
    keep[[2, 5]] = False
    e = {k: (v[keep] if k in u.INPUTS[4:] else v) for k, v in c.items()}
    rr = u.reference(e)
    assert r['bad'] == 2 and all(r[k] == rr[k] for k in u.LOSSES) and r['n_roi_pos'] == rr['n_roi_pos']


def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    assert all(name in history[at - 3000:at] for name in NAMES)
    assert 'still 20: sdn_mrcnn_loss_workspace_bytes, sdn_mrcnn_loss_fwd, sdn_mrcnn_loss_bwd added' in history
    assert 'model.py:1004-1147' in history and ':1955' in history
    host_checks.stale_library_is_refused(NAMES)


def test_the_kernels_are_built_without_fma_contraction():
    makefile_rules.assert_built_exactly('mrcnn_loss.hip')


def test_the_constants_are_mirrored_and_the_sizes_come_from_the_library():
    from sdn_hip import ops
    const = lambda k: host_checks.constexpr_int('mrcnn_loss_check.h', k)   # noqa: E731
    assert const('MRL_THREADS') == 64 and const('MRL_QUAD') == u.QUAD and const('MRL_STEPS') * u.STEP == u.CHUNK == ops.MRCNN_LOSS_CHUNK
    assert const('MRL_MAX_CLASSES') == ops.MRCNN_MAX_CLASSES == 128 and const('MRL_MAX_ANCHORS') == ops.MRCNN_MAX_ANCHORS
    wb, sb = ops.mrcnn_loss_bytes(5003, 13)
    assert wb == (5 + 13) * const('MRL_PART_BYTES') + 5 * 4 + 4 and sb == 16 + 13 * 8 + 5 * 4 + 4     # rounded up to 8 / to 16
    wb, sb = ops.mrcnn_loss_bytes(261888, 200)
    assert wb == (256 + 200) * 40 + 256 * 4 and sb == 16 + 200 * 8 + 256 * 4
    import sdn_hip
    n = ctypes.c_size_t()
    assert sdn_hip.lib().sdn_mrcnn_loss_workspace_bytes(0, 1, ctypes.byref(n), ctypes.byref(n)) == -1
    assert sdn_hip.lib().sdn_mrcnn_loss_workspace_bytes(5, 1, None, ctypes.byref(n)) == -1


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _inputs(batch=1, A=100, T=8, R=2, C=3, h=5, w=7, match=FAKE, pred=FAKE, ids=FAKE, mask=FAKE, ids_i64=1):
    return [match, 0, FAKE, FAKE, pred, batch, A, T, ids, ids_i64, FAKE, FAKE, FAKE, FAKE, mask, R, C, h, w]


def _fwd(work_bytes=1 << 30, saved_bytes=1 << 30, out=FAKE, counts=FAKE, **kw):
    import sdn_hip
    L = sdn_hip.lib()
    rc = L.sdn_mrcnn_loss_fwd(*(_inputs(**kw) + [FAKE, work_bytes, FAKE, saved_bytes, out, counts, None]))
    return rc, L.sdn_last_error().decode()


def _bwd(saved_bytes=1 << 30, grads=(FAKE,) * 5, gout=FAKE, **kw):
    import sdn_hip
    L = sdn_hip.lib()
    rc = L.sdn_mrcnn_loss_bwd(*(_inputs(**kw) + [FAKE, saved_bytes, gout] + list(grads) + [None]))
    return rc, L.sdn_last_error().decode()


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_the_entry_points_refuse_bad_arguments_before_any_launch(call):
    rc, msg = call(batch=2)
    assert rc == -1 and 'batch 2' in msg and 'model.py:1053' in msg
    rc, msg = call(C=1)
    assert rc == -1 and '1 classes; 2 to 128' in msg
    rc, msg = call(C=129)
    assert rc == -1 and '129 classes; 2 to 128' in msg
    rc, msg = call(match=None)
    assert rc == -1 and 'rpn_match is NULL' in msg
    rc, msg = call(pred=None)
    assert rc == -1 and 'is NULL' in msg
    rc, msg = call(mask=None)
    assert rc == -1 and 'head tensor is NULL' in msg
    rc, msg = call(ids=FAKE + 4)
    assert rc == -1 and 'aligned to its element size' in msg
    assert call(ids=FAKE + 4, ids_i64=0)[1].find('element size') < 0        # an int32 tensor may sit there
    rc, msg = call(pred=FAKE + 2)
    assert rc == -1 and 'aligned to 4' in msg
    rc, msg = call(R=4, C=128, h=2048, w=2048)                                # exactly 2^31
    assert rc == -1 and 'below 2^31' in msg
    rc, msg = call(R=0x7fffffff, C=128, h=0x7fffffff, w=0x7fffffff)           # the check itself must not overflow
    assert rc == -1 and 'below 2^31' in msg
    rc, msg = call(A=(1 << 24) + 1)
    assert rc == -1 and 'anchors; at most' in msg
    for bad in (dict(A=0), dict(T=0), dict(R=-1), dict(h=0), dict(w=-3)):
        rc, msg = call(**bad)
        assert rc == -1 and 'bad sizes' in msg, bad


def test_the_forward_entry_point_checks_its_buffers():
    rc, msg = _fwd(out=None)
    assert rc == -1 and 'NULL' in msg
    rc, msg = _fwd(counts=FAKE + 4)
    assert rc == -1 and 'aligned to 8' in msg
    rc, msg = _fwd(A=5003, R=13, work_bytes=743)
    assert rc == -1 and 'workspace of 743 bytes; 744 are needed' in msg
    rc, msg = _fwd(A=5003, R=13, saved_bytes=143)
    assert rc == -1 and 'saved of 143 bytes; 144 are needed' in msg


def test_the_backward_entry_point_checks_its_buffers():
    rc, msg = _bwd(grads=(None,) * 5)
    assert rc == -1 and 'no gradient asked for' in msg
    rc, msg = _bwd(R=0, grads=(FAKE, FAKE, None, None, FAKE))
    assert rc == -1 and 'head gradient with R = 0' in msg
    rc, msg = _bwd(gout=None)
    assert rc == -1 and 'NULL' in msg
    rc, msg = _bwd(A=5003, R=13, saved_bytes=143)
    assert rc == -1 and 'saved of 143 bytes' in msg


def _cpu_case():
    return [torch.as_tensor(v) for v in u.draw_case('novalid').values()]


def test_cpu_tensors_and_bad_arguments_raise():
    from sdn_hip import ops
    args = _cpu_case()
    for fn in (losses.mrcnn_losses, losses.compute_losses, ops.mrcnn_loss):
        with pytest.raises(NotImplementedError):
            fn(*args)
    empty = [torch.as_tensor(v) for v in u.draw_case('empty').values()]
    with pytest.raises(NotImplementedError):
        losses.compute_losses(*empty)                      # R = 0 goes the same way

    def swapped(i, t):
        return [t if j == i else a for j, a in enumerate(args)]
    with pytest.raises(TypeError, match='rpn_match must be torch.int32 or torch.int64'):
        losses.mrcnn_losses(*swapped(0, args[0].float()))
    with pytest.raises(TypeError, match='mrcnn_mask must be torch.float32'):
        losses.mrcnn_losses(*swapped(9, args[9].double()))
    with pytest.raises(TypeError, match='must be a torch.Tensor'):
        losses.mrcnn_losses(*swapped(3, args[3].numpy()))
    with pytest.raises(ValueError, match=r'model\.py:1053'):
        losses.mrcnn_losses(*[torch.cat([a, a]) if i < 4 else a for i, a in enumerate(args)])
    with pytest.raises(ValueError, match=r'rpn_match must be \[1, 300, 1\]'):
        losses.mrcnn_losses(*swapped(0, args[0][:, :299]))
    with pytest.raises(ValueError, match='rpn_pred_bbox must be'):
        losses.mrcnn_losses(*swapped(3, args[3][:, :, :3]))
    with pytest.raises(ValueError, match=r'rpn_bbox must be fp32 \[1, T, 4\]'):
        losses.mrcnn_losses(*swapped(1, args[1][0]))
    with pytest.raises(ValueError, match='mrcnn_bbox must be'):
        losses.mrcnn_losses(*swapped(7, args[7][:, :2]))
    with pytest.raises(ValueError, match='target_mask must be'):
        losses.mrcnn_losses(*swapped(8, args[8][:, :4]))
    with pytest.raises(ValueError, match='2 to 128 classes'):
        losses.mrcnn_losses(*swapped(9, torch.zeros(13, 1, 5, 7)))
    with pytest.raises(ValueError, match=r'target_class_ids must be \[R\]'):
        losses.mrcnn_losses(*swapped(4, args[4].reshape(1, 13)))


def test_the_public_names_and_the_docstring():
    assert losses.LOSS_KEYS == u.LOSSES and losses.COUNT_KEYS == u.COUNTS
    import inspect
    assert list(inspect.signature(losses.compute_losses).parameters) == list(u.INPUTS)
    assert list(inspect.signature(losses.mrcnn_losses).parameters) == list(u.INPUTS)
    doc = losses.mrcnn_losses.__doc__
    assert 'NaN' in doc and ':1070, 1088, 1118' in doc and ':1053' in doc


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_arithmetic_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/mrcnn_loss_check.cpp: a stand-alone program with its own main that includes only csrc/mrcnn_loss_check.h; host code on
    the CPU, never loaded into Python"""
    rc, out = host_checks.run_check_program('mrcnn_loss_check', ['mrcnn_loss_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out
