"""The semantic training loss without a GPU: the fixture tests/golden/segm_loss_golden.npz against its seeds and against the
float64 expressions of tests/segm_loss_util.py, the ABI revision, the build list, and the argument checks of sdn_segm_loss_fwd /
_bwd and of the binding, all of which run before any launch."""
import os

import numpy as np
import pytest
import torch

import host_checks
import makefile_rules
import segm_loss_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_fixture_regenerates_from_its_seeds(gold, name):
    scores, deep, label = u.draw_case(name)
    p = name + '/'
    assert np.array_equal(gold[p + 'scores8'].astype(np.float32) / 8, scores)
    assert (p + 'deepsup8' in gold.files) == (deep is not None)
    if deep is not None:
        assert np.array_equal(gold[p + 'deepsup8'].astype(np.float32) / 8, deep)
    assert gold[p + 'seg_label'].dtype == np.int64 and np.array_equal(gold[p + 'seg_label'], label)
    r = u.reference(scores, deep, label)
    for k in ('loss', 'loss_main', 'loss_deepsup'):
        want = float(gold[p + k])
        assert (np.isnan(want) and np.isnan(r[k])) or abs(r[k] - want) <= 1e-13 * abs(want), (k, r[k], want)
    assert r['acc'].tobytes() == gold[p + 'acc'].tobytes() == u.acc_fp32(r['acc_sum'], r['pixel_sum']).tobytes()
    for k in ('acc_sum', 'pixel_sum', 'bad'):
        assert r[k] == int(gold[p + k]), k
    for k in ('grad', 'grad_deepsup'):
        g = r[k]
        if g is None:
            assert not any(f.startswith(p + k) for f in gold.files)
        elif name in u.STORED_WHOLE:
            assert np.allclose(g, gold[p + k], rtol=1e-12, atol=1e-18)
        else:
            assert np.allclose(g.reshape(-1)[::u.SAMPLE_STRIDE], gold[p + k + '_sample'], rtol=1e-12, atol=1e-18)
            assert abs(np.linalg.norm(g) - float(gold[p + k + '_norm'])) <= 1e-12 * float(gold[p + k + '_norm'])


def test_the_fixture_holds_what_the_cases_are_there_for(gold):
    assert os.path.getsize(u.GOLD) < 300 * 1024
    assert np.array_equal(gold['weights'], [u.WEIGHTS[k] for k in ('loss', 'acc', 'loss_main', 'loss_deepsup')])
    assert len(set(u.WEIGHTS.values())) == 4 and float(gold['scale']) == u.SCALE
    lab = gold['blocks/seg_label']
    assert (lab[1] == -1).all() and (lab == 14).any() and (lab == -2).any() and int(gold['blocks/bad']) > 0
    assert int(gold['blocks/bad']) == int(((lab < -1) | (lab >= 14)).sum())
    assert np.isnan(gold['ignored/loss']) and float(gold['ignored/acc']) == 0.0 and int(gold['ignored/pixel_sum']) == 0
    assert not gold['ignored/grad'].any() and not gold['ignored/grad_deepsup'].any()
    assert float(gold['c1/loss']) == 0.0 and not gold['c1/grad'].any() and not gold['c1/grad_deepsup'].any()
    for name, (_, (B, C, h, w), _, _) in u.CASES.items():
        if C >= 2:
            gap = u.top_two_gap(gold[name + '/scores8'].astype(np.float32) / 8)
            assert (gap == 0).any() and ((gap == 0) | (gap >= 0.125)).all(), name
    # the vector path with more than one workgroup per item, and the scalar path with more than one
    assert (12 * 40) % 4 == 0 and 12 * 40 > u.BLOCK_PIXELS and (9 * 65) % 4 and 9 * 65 > u.BLOCK_PIXELS


def test_the_abi_revision_is_20_everywhere():
    assert '20: sdn_segm_loss_fwd' in host_checks.entry_points(('sdn_segm_loss_fwd', 'sdn_segm_loss_bwd'))


def test_the_kernels_are_built_without_fma_contraction():
    makefile_rules.assert_built_exactly('segm_loss.hip')


def test_the_block_constant_is_mirrored():
    from sdn_hip import ops
    hdr = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'segm_loss_check.h')).read()
    assert host_checks.constexpr_int('segm_loss_check.h', 'SGL_PIXELS') == ops.SEGM_LOSS_PIXELS == u.BLOCK_PIXELS
    assert host_checks.constexpr_int('segm_loss_check.h', 'SGL_PART_BYTES') == ops.SEGM_LOSS_PART_BYTES
    assert 'segm_tail_check.h' in hdr and 'SEG_MAX_CLASSES' in hdr and ops.SEGM_MAX_CLASSES == 32   # one class limit, reused


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first


def _fwd(B=2, C=14, h=5, w=7, scores=FAKE, label=FAKE, scratch_bytes=1 << 30, out=FAKE):
    import sdn_hip
    L = sdn_hip.lib()
    rc = L.sdn_segm_loss_fwd(scores, FAKE, label, B, C, h, w, 0.4, FAKE, scratch_bytes, FAKE, out, FAKE, None)
    return rc, L.sdn_last_error().decode()


def _bwd(B=2, C=14, h=5, w=7, label=FAKE, g0=FAKE, g1=FAKE, scores=FAKE):
    import sdn_hip
    L = sdn_hip.lib()
    rc = L.sdn_segm_loss_bwd(scores, FAKE, label, B, C, h, w, 0.4, FAKE, FAKE, FAKE, g0, g1, None)
    return rc, L.sdn_last_error().decode()


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_the_entry_points_refuse_bad_arguments_before_any_launch(call):
    rc, msg = call(C=0)
    assert rc == -1 and '0 classes; 1 to 32' in msg
    rc, msg = call(C=33)
    assert rc == -1 and '33 classes; 1 to 32' in msg
    rc, msg = call(label=None)
    assert rc == -1 and 'seg_label is NULL' in msg
    rc, msg = call(B=4, C=32, h=4096, w=4096)                  # exactly 2^31
    assert rc == -1 and 'below 2^31' in msg
    rc, msg = call(B=1, C=1, h=65536, w=32768)                 # h * w alone reaches 2^31
    assert rc == -1 and 'below 2^31' in msg
    rc, msg = call(B=0x7fffffff, C=32, h=0x7fffffff, w=0x7fffffff)   # the check itself must not overflow
    assert rc == -1 and 'below 2^31' in msg
    for bad in (dict(B=0), dict(h=0), dict(w=-3)):
        rc, msg = call(**bad)
        assert rc == -1 and 'bad sizes' in msg


def test_the_forward_entry_point_checks_its_buffers():
    rc, msg = _fwd(scores=None)
    assert rc == -1 and 'scores is NULL' in msg
    rc, msg = _fwd(out=None)
    assert rc == -1 and 'NULL' in msg
    rc, msg = _fwd(B=3, h=12, w=40, scratch_bytes=3 * 2 * 32 - 1)   # 480 pixels: two workgroups per item
    assert rc == -1 and 'scratch of 191 bytes; 192 are needed' in msg
    rc, msg = _fwd(label=FAKE + 4)
    assert rc == -1 and 'aligned to 8' in msg


def test_the_backward_entry_point_checks_its_buffers():
    rc, msg = _bwd(g0=None, g1=None)
    assert rc == -1 and 'no gradient asked for' in msg
    rc, msg = _bwd(scores=None)
    assert rc == -1 and 'grad_scores without scores' in msg


def test_cpu_tensors_and_bad_arguments_raise():
    import semantic
    from sdn_hip import ops
    from semantic import train_loss
    assert semantic.segm_losses is train_loss.segm_losses and semantic.train_forward is train_loss.train_forward
    scores = torch.zeros(2, 14, 5, 7)
    label = torch.zeros(2, 5, 7, dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        train_loss.segm_losses(scores, label)
    with pytest.raises(NotImplementedError):
        ops.segm_loss(scores, scores, label, 0.4)
    with pytest.raises(TypeError):
        ops.segm_loss(scores.numpy(), None, label, 0.4)
    with pytest.raises(ValueError, match='deep_sup_scale'):
        train_loss.segm_losses(scores, label, scores_deepsup=scores)
    # a wrong dtype or shape is refused whatever the device
    for bad_label in (label.int(), label.float()):
        with pytest.raises(TypeError, match='seg_label must be torch.int64'):
            train_loss.segm_losses(scores, bad_label)
    with pytest.raises(TypeError, match='scores must be torch.float32'):
        train_loss.segm_losses(scores.double(), label)
    with pytest.raises(ValueError, match='seg_label must be int64'):
        train_loss.segm_losses(scores, label[:, :4])
    with pytest.raises(ValueError, match='scores_deepsup is'):
        train_loss.segm_losses(scores, label, scores[:, :13], 0.4)
    with pytest.raises(ValueError, match=r'\[B, C, h, w\]'):
        train_loss.segm_losses(scores[0], label)
    with pytest.raises(ValueError, match='1 to 32 classes'):
        train_loss.segm_losses(torch.zeros(2, 33, 5, 7), label)

    class NoDecoder(torch.nn.Module):
        deep_sup_scale = None

    with pytest.raises(ValueError, match='decoder'):
        train_loss.train_forward(NoDecoder(), {})
