"""Losses of the geometric branch: the test-time optimisation (geometric/scripts/main.py:422-456) and the training step
(BaseNet.step_batch, main.py:114-154).

The reference writes the loss inline in its optimisation loop (main.py:445-451):

    loss = torch.nn.functional.mse_loss(_masks, masks_padded, reduce=False) + 100 * torch.mean(_blob['_ffd_coeffs'] ** 2)
    if image_ignores is not None:
        loss = loss * (1 - ignores_padded)
    loss = torch.mean(loss)

`silhouette_ffd_loss` is that expression as one fused HIP op (sdn_silhouette_loss_fwd / _bwd, csrc/fast_loss.hip): the loop
runs it once per iteration around a 0.9 ms frame step, where a dozen 3-9 us element-wise launches each way were 15 % of the
step.  GPU tensors only (no CPU fallback).

`step_losses` is the body of BaseNet.step_batch after the model call: the loss dict of a training step from the model's blob
and the batch, as one fused HIP op (sdn_train_losses_fwd / _bwd, csrc/train_loss.hip)."""
import torch

from . import TargetType

GEOMETRY_LOSSES = ('theta_delta_loss', 'translation2d_loss', 'scale_loss', 'depth_loss')
REPROJECT_LOSSES = ('class_reward', 'mask_loss', 'ffd_coeff_reg')
_GEOMETRY_COLUMNS = (('_theta_deltas', 'thetas', 2, 1), ('_translation2ds', 'translation2ds', 2, 2), ('_log_scales', 'log_scales', 3, 3),
                     ('_log_depths', 'log_depths', 1, 1))


def silhouette_ffd_loss(masks, masks_target, ffd_coeffs, ignores=None):
    """masks, masks_target (and ignores) [n, 1, R, R] float32 CUDA; ffd_coeffs any shape.  Returns the scalar loss;
    differentiable wrt masks and ffd_coeffs."""
    from sdn_hip import ops
    if not masks.is_cuda:
        raise NotImplementedError('silhouette_ffd_loss runs on the GPU only (got %s)' % masks.device)
    return ops.SilhouetteLossFn.apply(masks, masks_target, ffd_coeffs, ignores)


def step_loss_keys(mode):
    """the keys of step_losses' dict for `mode`, in the reference's order"""
    return (GEOMETRY_LOSSES if mode & TargetType.geometry else ()) + (REPROJECT_LOSSES if mode & TargetType.reproject else ())


def _entry(mapping, key, what):
    try:
        return mapping[key]
    except KeyError:
        raise ValueError('%s has no %r, which this mode needs' % (what, key))


def _float32(t, name, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError('%s must be a float32 tensor, got %s' % (name, getattr(t, 'dtype', type(t))))
    if shape is not None and tuple(t.shape) != shape:
        raise ValueError('%s must be %s, got %s' % (name, list(shape), list(t.shape)))
    return t


def check_step_shapes(blob, batch, mode):
    """ValueError unless blob and batch hold what step_losses needs for `mode`, with the dtypes and shapes of
    Derenderer3d.forward and train_batch.  Looks at shapes and dtypes only: no device is needed.  Returns (B, R, S); R and S
    are None without the reprojection terms."""
    targets = _entry(batch, 'targets', 'batch')
    if not isinstance(targets, torch.Tensor) or targets.dim() != 1 or targets.shape[0] < 1 or targets.dtype not in (torch.int64, torch.uint8):
        raise ValueError('targets must be an int64 or uint8 tensor [B], got %s %s' %
                         (getattr(targets, 'dtype', type(targets)), list(getattr(targets, 'shape', ()))))
    B = int(targets.shape[0])
    R = S = None
    if mode & TargetType.geometry:
        for pred, given, cols, given_cols in _GEOMETRY_COLUMNS:
            _float32(_entry(blob, pred, 'blob'), pred, (B, cols))
            _float32(_entry(batch, given, 'batch'), given, (B, given_cols))
    if mode & TargetType.reproject:
        _float32(_entry(blob, '_class_log_probs', 'blob'), '_class_log_probs', (B,))
        ffd = _float32(_entry(blob, '_ffd_coeffs', 'blob'), '_ffd_coeffs', None)
        if ffd.numel() < 1:
            raise ValueError('_ffd_coeffs is empty')
        rendered = _float32(_entry(blob, '_masks', 'blob'), '_masks', None)
        if rendered.dim() != 4 or rendered.shape[0] != B or rendered.shape[1] != 1 or rendered.shape[2] != rendered.shape[3]:
            raise ValueError('_masks must be [%d, 1, R, R], got %s' % (B, list(rendered.shape)))
        R = int(rendered.shape[3])
        masks = _float32(_entry(batch, 'masks', 'batch'), 'masks', None)
        if masks.dim() != 4 or masks.shape[0] != B or masks.shape[1] != 1 or masks.shape[2] != masks.shape[3]:
            raise ValueError('masks must be [%d, 1, S, S], got %s' % (B, list(masks.shape)))
        S = int(masks.shape[3])
        _float32(_entry(batch, 'ignores', 'batch'), 'ignores', (B, 1, S, S))
        if R < S or (R - S) % 2:
            raise ValueError('the render size %d minus the mask size %d must be even and not negative: pad_like pads (R - S) // 2 on '
                             'both sides' % (R, S))
    return B, R, S


def step_losses(blob, batch, mode, mask_weight=0.1, ffd_coeff_reg=1.0):
    """The loss dict of BaseNet.step_batch (main.py:118-154) for the blob `Derenderer3d.forward` returned and the batch
    `train_items.train_batch` returned (or any mapping with those keys), with FLAGS.mode, .mask_weight, .ffd_coeff_reg as arguments.

    mode & TargetType.geometry: theta_delta_loss, translation2d_loss, scale_loss, depth_loss over the items whose `targets` hold
    the geometry bit; mode & TargetType.reproject: class_reward, mask_loss over the items whose targets hold the reproject bit,
    and ffd_coeff_reg over all items -- the reference's keys in its order, only the groups `mode` selects; the batch entries of
    the other group may be absent.  A loss whose selection is empty is exactly 0 and sends no gradient (the torch.tensor(0.0)
    branch of BaseNet.partial).  targets: int64 [B] (train_batch) or uint8 [B].

    Every value is a 0-dim view of one [7] tensor, so `sum(loss_dict.values()).backward()` is one backward launch.  The items are
    selected on the device: nothing here waits for it.  A NaN propagates into the loss that met it; the reference's
    `pdb.set_trace()` on a NaN (main.py:105-107) is not reproduced.

    ValueError for a missing entry, a wrong dtype or shape, or a render size that differs from the mask size by an odd or negative
    amount, before anything is launched.  GPU tensors only: NotImplementedError for CPU tensors."""
    from sdn_hip import ops
    mode = int(mode)
    check_step_shapes(blob, batch, mode)
    geometry, reproject = bool(mode & TargetType.geometry), bool(mode & TargetType.reproject)
    args = ([blob[k] if geometry else None for k in ('_theta_deltas', '_translation2ds', '_log_scales', '_log_depths')] +
            [blob[k] if reproject else None for k in ('_class_log_probs', '_masks', '_ffd_coeffs')] +
            [batch[k] if geometry else None for k in ('thetas', 'translation2ds', 'log_scales', 'log_depths')] +
            [batch[k] if reproject else None for k in ('masks', 'ignores')])
    targets = batch['targets']
    for t in args + [targets]:
        if t is not None and not t.is_cuda:
            raise NotImplementedError('step_losses runs on the GPU only (got a tensor on %s)' % t.device)
    if not (geometry or reproject):
        return {}
    if targets.dtype != torch.int64:
        targets = targets.long()
    out = ops.TrainLossesFn.apply(mode, float(mask_weight), float(ffd_coeff_reg), *args, targets)
    slots = out.unbind(0)
    names = GEOMETRY_LOSSES + REPROJECT_LOSSES
    return {k: slots[names.index(k)] for k in step_loss_keys(mode)}
