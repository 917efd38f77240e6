"""The host side of derender3d.losses.step_losses: what it refuses before any launch, its keys per mode, and the scratch size the
library reports.  No GPU is needed."""
import ctypes
import os

import pytest
import torch

import sdn_hip
from derender3d import TargetType
from derender3d import losses as L


def tensors(B=3, R=40, S=32):
    blob = {'_theta_deltas': torch.zeros(B, 2), '_translation2ds': torch.zeros(B, 2), '_log_scales': torch.zeros(B, 3),
            '_log_depths': torch.zeros(B, 1), '_class_log_probs': torch.zeros(B), '_masks': torch.zeros(B, 1, R, R),
            '_ffd_coeffs': torch.zeros(B, 8, 21), '_normals': [], '_depth_maps': []}
    batch = {'thetas': torch.zeros(B, 1), 'translation2ds': torch.zeros(B, 2), 'log_scales': torch.zeros(B, 3),
             'log_depths': torch.zeros(B, 1), 'masks': torch.zeros(B, 1, S, S), 'ignores': torch.zeros(B, 1, S, S),
             'targets': torch.full((B,), 3, dtype=torch.int64)}
    return blob, batch


def test_cpu_tensors_raise_not_implemented():
    blob, batch = tensors()
    for mode in (TargetType.pretrain, TargetType.finetune, TargetType.full, TargetType.extend):
        with pytest.raises(NotImplementedError):
            L.step_losses(blob, batch, mode)


def test_shapes_and_dtypes_are_checked_before_the_device():
    blob, batch = tensors()
    assert L.check_step_shapes(blob, batch, TargetType.extend) == (3, 40, 32)
    assert L.check_step_shapes(blob, batch, TargetType.pretrain) == (3, None, None)
    assert L.check_step_shapes(dict(blob, _masks=torch.zeros(3, 1, 32, 32)), batch, TargetType.extend) == (3, 32, 32)   # p = 0
    assert L.check_step_shapes(blob, dict(batch, targets=batch['targets'].to(torch.uint8)), TargetType.extend) == (3, 40, 32)
    bad = [
        (dict(blob, _masks=torch.zeros(3, 1, 35, 35)), batch),                    # R - S odd
        (dict(blob, _masks=torch.zeros(3, 1, 30, 30)), batch),                    # R < S
        (blob, dict(batch, masks=torch.zeros(3, 1, 32, 33))),                     # a mask that is not square
        (blob, dict(batch, ignores=torch.zeros(3, 1, 32, 33))),
        (dict(blob, _log_scales=torch.zeros(3, 3, dtype=torch.float64)), batch),  # float64 predictions
        (dict(blob, _masks=torch.zeros(3, 1, 40, 40, dtype=torch.float64)), batch),
        (dict(blob, _theta_deltas=torch.zeros(3, 3)), batch),
        (dict(blob, _class_log_probs=torch.zeros(3, 1)), batch),
        (dict(blob, _masks=torch.zeros(2, 1, 40, 40)), batch),
        (dict(blob, _ffd_coeffs=torch.zeros(0)), batch),
        (blob, dict(batch, targets=torch.zeros(3))),                              # float targets
        (blob, dict(batch, targets=torch.zeros(3, 1, dtype=torch.int64))),
        (blob, {k: v for k, v in batch.items() if k != 'thetas'}),
        ({k: v for k, v in blob.items() if k != '_masks'}, batch),
    ]
    for b, t in bad:
        with pytest.raises(ValueError):
            L.check_step_shapes(b, t, TargetType.extend)
        with pytest.raises(ValueError):       # the same through the public function, on CPU tensors: refused before the device is asked for
            L.step_losses(b, t, TargetType.extend)


def test_a_mode_only_needs_the_entries_of_its_groups():
    blob, batch = tensors()
    no_maps = {k: v for k, v in batch.items() if k not in ('masks', 'ignores')}
    assert L.check_step_shapes(blob, no_maps, TargetType.pretrain)[0] == 3
    with pytest.raises(ValueError):
        L.check_step_shapes(blob, no_maps, TargetType.full)
    only_maps = {k: batch[k] for k in ('masks', 'ignores', 'targets')}
    assert L.check_step_shapes(blob, only_maps, TargetType.finetune) == (3, 40, 32)
    with pytest.raises(ValueError):
        L.check_step_shapes(blob, only_maps, TargetType.full)


def test_keys_per_mode_in_the_reference_order():
    geometry = ('theta_delta_loss', 'translation2d_loss', 'scale_loss', 'depth_loss')
    reproject = ('class_reward', 'mask_loss', 'ffd_coeff_reg')
    assert L.step_loss_keys(TargetType.pretrain) == geometry
    assert L.step_loss_keys(TargetType.finetune) == reproject
    assert L.step_loss_keys(TargetType.full) == L.step_loss_keys(TargetType.extend) == geometry + reproject
    assert L.step_loss_keys(TargetType.normal | TargetType.depth) == ()


@pytest.mark.skipif(not os.path.exists(sdn_hip.LIB_PATH), reason='libsdn_hip.so is not built')
def test_the_scratch_size_comes_from_the_library_and_follows_the_batch():
    small, large = sdn_hip.train_losses_scratch(4, 384, 1000), sdn_hip.train_losses_scratch(64, 384, 1000)
    assert 0 < small < large and small % 8 == 0 and large % 8 == 0
    assert sdn_hip.train_losses_scratch(64, 384, 10 ** 7) == large == sdn_hip.train_losses_scratch(64, 384, 0)
    assert sdn_hip.train_losses_scratch(64, 384, 0) >= 8 * (2 + 64 + 2 * 64)      # n_g, n_r, m_i and a partial pair per item at least
    n = ctypes.c_size_t(0)
    assert sdn_hip.lib().sdn_train_losses_scratch(0, 384, 0, ctypes.byref(n)) == -1
    assert sdn_hip.lib().sdn_train_losses_scratch(4, 384, 0, None) == -1


@pytest.mark.skipif(not os.path.exists(sdn_hip.LIB_PATH), reason='libsdn_hip.so is not built')
def test_the_library_validates_before_it_launches():
    """every call below is refused on the host (fake non-null pointers are never dereferenced)"""
    lib = sdn_hip.lib()
    fake = 4096
    args = lambda R, S, mode, scratch=fake: ([fake] * 7 + [168] + [fake] * 7 + [2, R, S, mode, 0.1, 1.0, scratch, fake, None])
    assert lib.sdn_train_losses_fwd(*args(35, 32, 3)) == -1 and b'must be even' in lib.sdn_last_error()
    assert lib.sdn_train_losses_fwd(*args(30, 32, 2)) == -1 and b'must be even' in lib.sdn_last_error()
    assert lib.sdn_train_losses_fwd(*args(40, 32, 3, scratch=None)) == -1
    a = args(40, 32, 3)
    a[0] = None
    assert lib.sdn_train_losses_fwd(*a) == -1 and b'geometry' in lib.sdn_last_error()
    a = args(40, 32, 3)
    a[12] = None
    assert lib.sdn_train_losses_fwd(*a) == -1 and b'reprojection' in lib.sdn_last_error()
    bwd = [fake] * 6 + [168] + [fake] * 7 + [2, 35, 32, 3, 0.1, 1.0, fake, fake] + [fake] * 7 + [None]
    assert lib.sdn_train_losses_bwd(*bwd) == -1 and b'must be even' in lib.sdn_last_error()
    bwd[15] = 40
    bwd[22:29] = [None] * 7
    assert lib.sdn_train_losses_bwd(*bwd) == -1 and b'no gradient' in lib.sdn_last_error()
