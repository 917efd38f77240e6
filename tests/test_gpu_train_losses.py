"""derender3d.losses.step_losses (sdn_train_losses_fwd / _bwd, csrc/train_loss.hip) against the reference's own expressions
(geometric/scripts/main.py:97-154 with Transforms.pad_like, derender3d/datasets.py:29-33, `// 2` on both sides) evaluated in
float64 on the CPU with autograd.  Predictions and batch entries are drawn independently, so no difference cancels and a relative
gate means something.  The gate is the sibling loss's (tests/test_gpu_derender3d.py:265-268): every loss within 1e-6 relative of
the fp64 value, every gradient within 1e-6 of the fp64 gradient in relative 2-norm."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from derender3d import TargetType
from derender3d import losses as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GATE = 1e-6
PRED_KEYS = ('_theta_deltas', '_translation2ds', '_log_scales', '_log_depths', '_class_log_probs', '_masks', '_ffd_coeffs')
HEAD_KEYS = PRED_KEYS[:4]
ALL_KEYS = L.GEOMETRY_LOSSES + L.REPROJECT_LOSSES
WEIGHTS = dict(zip(ALL_KEYS, (0.7, 1.3, 0.45, 2.1, 1.7, 0.9, 3.2)))   # seven distinct weights: a swapped grad_out slot shows


def reference_losses(blob, batch, mode, mask_weight, ffd_coeff_reg):
    """main.py:97-154, statement for statement, on whatever tensors it is handed (here: float64, CPU)"""
    def partial(f, m):
        def _f(*args, **kwargs):
            index = torch.nonzero(m)
            if index.numel():
                index = index.squeeze(dim=1)
                v = f(*[arg[index] for arg in args], **kwargs)
                if torch.isnan(v).any():        # the reference stops in pdb here (:105-107)
                    raise FloatingPointError('nan')
                return v
            return torch.tensor(0.0, dtype=args[0].dtype, device=m.device)
        return _f

    def pad_like(image, _image, mode='constant', value=0):
        pad_size_2 = _image.shape[2] - image.shape[2]
        pad_size_3 = _image.shape[3] - image.shape[3]
        pad = (pad_size_3 // 2, pad_size_3 // 2, pad_size_2 // 2, pad_size_2 // 2)
        return F.pad(image, pad, mode=mode, value=value) if mode == 'constant' else F.pad(image, pad, mode=mode)

    targets = batch['targets']
    loss_dict = {}
    if mode & TargetType.geometry:
        is_geometry = targets & TargetType.pretrain
        mse_loss = partial(F.mse_loss, is_geometry)
        theta_deltas = torch.cat([torch.cos(batch['thetas']), torch.sin(batch['thetas'])], dim=1)
        loss_dict.update({
            'theta_delta_loss': mse_loss(blob['_theta_deltas'], theta_deltas),
            'translation2d_loss': mse_loss(blob['_translation2ds'], batch['translation2ds']),
            'scale_loss': mse_loss(blob['_log_scales'], batch['log_scales']),
            'depth_loss': mse_loss(blob['_log_depths'], batch['log_depths']),
        })
    if mode & TargetType.reproject:
        is_reproject = targets & TargetType.finetune
        mean = partial(torch.mean, is_reproject)
        masks = pad_like(batch['masks'], blob['_masks'])
        ignores = pad_like(batch['ignores'], blob['_masks'], mode='replicate')
        mask_losses = (1 - ignores) * F.mse_loss(blob['_masks'], masks, reduction='none')
        mask_losses = mask_weight * mask_losses.mean(dim=3).mean(dim=2).mean(dim=1)
        loss_dict.update({
            'class_reward': mean(blob['_class_log_probs'] * mask_losses.detach()),
            'mask_loss': mean(mask_losses),
            'ffd_coeff_reg': ffd_coeff_reg * torch.mean(blob['_ffd_coeffs'] ** 2),
        })
    return loss_dict


def draw(B, R, S, targets, seed):
    """(blob, batch) in float32 on the CPU.  The ignore maps hold what train_batch produces, multiples of 1 / 255 with 254 / 255
    and 0 among them, and differ along their border, so replicate padding cannot pass for constant padding."""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32))
    blob = {
        '_theta_deltas': f(rng.normal(size=(B, 2))),
        '_translation2ds': f(rng.normal(size=(B, 2)) * 0.3),
        '_log_scales': f(rng.normal(size=(B, 3))),
        '_log_depths': f(rng.normal(size=(B, 1)) + 2.0),
        '_class_log_probs': f(np.log(rng.uniform(0.05, 0.9, size=B))),
        '_masks': f(rng.uniform(0, 1, size=(B, 1, R, R))),
        '_ffd_coeffs': f(rng.normal(size=(B, 8, 21)) * 0.1),
    }
    ignores = rng.choice(np.asarray([0, 0, 0, 1, 37, 128, 254, 255]), size=(B, 1, S, S))
    ignores[:, :, 0, :] = np.arange(S) % 7 * 36            # the border rows and columns vary pixel by pixel
    ignores[:, :, S - 1, :] = (np.arange(S) * 5 + 2) % 255
    ignores[:, :, :, 0] = (np.arange(S) * 11 + 1) % 255
    ignores[:, :, :, S - 1] = 254 - np.arange(S) % 5 * 50
    ignores[:, :, 0, 0], ignores[:, :, S - 1, S - 1] = 254, 0
    batch = {
        'thetas': f(rng.uniform(-np.pi, np.pi, size=(B, 1))),
        'translation2ds': f(rng.normal(size=(B, 2)) * 0.3),
        'log_scales': f(rng.normal(size=(B, 3))),
        'log_depths': f(rng.normal(size=(B, 1)) + 2.0),
        'masks': f(rng.integers(0, 256, size=(B, 1, S, S))) / np.float32(255),
        'ignores': f(ignores) / np.float32(255),
        'targets': torch.tensor(targets, dtype=torch.int64),
    }
    return blob, batch


def weighted(loss_dict):
    return sum(WEIGHTS[k] * v for k, v in loss_dict.items())


def run_reference(blob, batch, mode, mask_weight=0.1, ffd_coeff_reg=1.0):
    """the fp64 losses and the fp64 gradients of sum(w_k loss_k)"""
    b64 = {k: v.double().requires_grad_() for k, v in blob.items()}
    t64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in batch.items()}
    ref = reference_losses(b64, t64, mode, mask_weight, ffd_coeff_reg)
    total = weighted(ref)
    if total.requires_grad:
        total.backward()
    return {k: float(v.detach()) for k, v in ref.items()}, {k: v.grad for k, v in b64.items()}


def run_device(blob, batch, mode, no_grad=(), **kw):
    """the device losses and gradients of sum(w_k loss_k); `no_grad`: predictions that ask for none"""
    bd = {k: v.to(DEV).requires_grad_(k not in no_grad) for k, v in blob.items()}
    td = {k: v.to(DEV) for k, v in batch.items()}
    got = L.step_losses(bd, td, mode, **kw)
    total = weighted(got)
    if total.requires_grad:
        total.backward()
    return got, {k: v.grad for k, v in bd.items()}, bd, td


def compare(got, grads, ref, ref_grads, what):
    assert list(got) == list(ref), what
    for k in ref:
        g = float(got[k].detach())
        print('%s %s: device %.9g fp64 %.12g rel %.3g' % (what, k, g, ref[k], abs(g - ref[k]) / abs(ref[k]) if ref[k] else abs(g)))
    for k in ref:
        assert got[k].dim() == 0 and abs(float(got[k].detach()) - ref[k]) <= GATE * abs(ref[k]), (what, k, float(got[k].detach()), ref[k])
    for k, rg in ref_grads.items():
        g = grads[k]
        if rg is None or float(rg.norm()) == 0.0:
            assert g is None or not g.any(), (what, k)
            continue
        rel = float((g.detach().cpu().double() - rg).norm() / rg.norm())
        print('%s d/d%s: rel 2-norm %.3g' % (what, k, rel))
        assert g.shape == rg.shape and rel <= GATE, (what, k, rel)


CASES = {
    'main': (5, 40, 32, [3, 2, 1, 3, 2]),            # p = 4, 16-byte loads everywhere; 400 float4 per item: the tail of a block runs
    'p0': (5, 32, 32, [3, 2, 1, 3, 2]),              # no padding
    'p3': (5, 38, 32, [3, 2, 1, 3, 2]),              # R % 4 != 0: the scalar path
    'p8': (5, 48, 32, [3, 2, 1, 3, 2]),              # p = 8, 16-byte loads
    'p2': (3, 36, 32, [2, 3, 1]),                    # R % 4 == 0, p % 4 != 0: 16-byte loads of _masks, scalar loads of the maps
    'chunks': (3, 96, 64, [3, 1, 2]),                # 9216 floats per item: three row chunks of 42, 42 and 12 rows per item
    'chunks_scalar': (2, 90, 64, [2, 3]),            # the same on the scalar path (p = 13)
    'all2': (4, 40, 32, [2, 2, 2, 2]),
    'all1': (4, 40, 32, [1, 1, 1, 1]),
    'b1': (1, 40, 32, [3]),
}
_done = {}


def case(name):
    """inputs, fp64 truth and the device's answer of a case in mode `extend`, computed once and shared (read-only)"""
    if name not in _done:
        B, R, S, targets = CASES[name]
        blob, batch = draw(B, R, S, targets, seed=100 + sorted(CASES).index(name))
        ref, ref_grads = run_reference(blob, batch, TargetType.extend)
        got, grads, bd, td = run_device(blob, batch, TargetType.extend)
        _done[name] = dict(blob=blob, batch=batch, ref=ref, ref_grads=ref_grads, got=got, grads=grads, bd=bd, td=td)
    return _done[name]


@pytest.mark.parametrize('name', ['main', 'p0', 'p3', 'p8', 'p2', 'chunks', 'chunks_scalar', 'b1'])
def test_losses_and_gradients_match_the_fp64_reference(name):
    c = case(name)
    assert list(c['got']) == list(ALL_KEYS)
    compare(c['got'], c['grads'], c['ref'], c['ref_grads'], name)


def test_unselected_rows_get_exact_zeros():
    c = case('main')
    targets = c['batch']['targets']
    off_r, off_g = (targets & 2) == 0, (targets & 1) == 0
    assert off_r.any() and off_g.any()
    assert not c['grads']['_masks'].cpu()[off_r].any() and c['grads']['_masks'].cpu()[~off_r].any()
    assert not c['grads']['_class_log_probs'].cpu()[off_r].any()
    for k in HEAD_KEYS:
        assert not c['grads'][k].cpu()[off_g].any() and c['grads'][k].cpu()[~off_g].all(), k


def test_no_geometry_item_gives_exact_zeros_and_no_head_gradient():
    c = case('all2')
    compare(c['got'], c['grads'], c['ref'], c['ref_grads'], 'all2')
    for k in L.GEOMETRY_LOSSES:
        assert float(c['got'][k].detach()) == 0.0 and c['ref'][k] == 0.0
    for k in HEAD_KEYS:
        assert c['grads'][k] is None or not c['grads'][k].any()


def test_no_reproject_item_gives_exact_zeros_without_dividing_by_the_empty_count():
    c = case('all1')
    compare(c['got'], c['grads'], c['ref'], c['ref_grads'], 'all1')
    assert float(c['got']['mask_loss'].detach()) == 0.0 and float(c['got']['class_reward'].detach()) == 0.0
    gm = c['grads']['_masks']
    assert gm is not None and not torch.isnan(gm).any() and not gm.any()
    assert not c['grads']['_class_log_probs'].any()
    assert float(c['got']['ffd_coeff_reg'].detach()) > 0 and c['grads']['_ffd_coeffs'].any()


def test_pretrain_has_the_geometry_keys_and_needs_no_masks():
    c = case('main')
    batch = {k: v for k, v in c['batch'].items() if k not in ('masks', 'ignores')}
    ref, ref_grads = run_reference(c['blob'], batch, TargetType.pretrain)
    got, grads, _, _ = run_device(c['blob'], batch, TargetType.pretrain)
    assert list(got) == list(L.GEOMETRY_LOSSES)
    compare(got, grads, ref, ref_grads, 'pretrain')


def test_finetune_has_the_reproject_keys_and_needs_no_geometry_entries():
    c = case('main')
    batch = {k: c['batch'][k] for k in ('masks', 'ignores', 'targets')}
    blob = {k: c['blob'][k] for k in ('_class_log_probs', '_masks', '_ffd_coeffs')}
    ref, ref_grads = run_reference(blob, batch, TargetType.finetune)
    got, grads, _, _ = run_device(blob, batch, TargetType.finetune)
    assert list(got) == list(L.REPROJECT_LOSSES)
    compare(got, grads, ref, ref_grads, 'finetune')


def test_other_weights_and_uint8_targets():
    c = case('main')
    batch = dict(c['batch'], targets=c['batch']['targets'].to(torch.uint8))
    ref, ref_grads = run_reference(c['blob'], dict(batch, targets=c['batch']['targets']), TargetType.full, 0.37, 2.5)
    got, grads, _, _ = run_device(c['blob'], batch, TargetType.full, mask_weight=0.37, ffd_coeff_reg=2.5)
    compare(got, grads, ref, ref_grads, 'weights')


def test_class_reward_sends_its_gradient_to_the_log_probs_only():
    c = case('main')
    bd = {k: v.to(DEV).requires_grad_() for k, v in c['blob'].items()}
    got = L.step_losses(bd, c['td'], TargetType.extend)
    got['class_reward'].backward()
    assert bd['_masks'].grad is None or not bd['_masks'].grad.any()
    # d class_reward / d log p_i = m_i / n_r on the selected rows, from the fp64 masked reprojection term
    b64 = {k: v.double() for k, v in c['blob'].items()}
    t64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in c['batch'].items()}
    logp = b64['_class_log_probs'].requires_grad_()
    reference_losses(b64, t64, TargetType.extend, 0.1, 1.0)['class_reward'].backward()
    sel = (c['batch']['targets'] & 2) != 0
    g = bd['_class_log_probs'].grad.cpu().double()
    assert not g[~sel].any() and float((g - logp.grad).norm() / logp.grad.norm()) <= GATE


def test_masks_without_gradient_leave_the_other_gradients():
    c = case('main')
    got, grads, _, _ = run_device(c['blob'], c['batch'], TargetType.extend, no_grad=('_masks',))
    assert grads['_masks'] is None
    ref_grads = dict(c['ref_grads'], _masks=None)
    compare(got, grads, c['ref'], ref_grads, 'no _masks gradient')
    for k in PRED_KEYS:
        if k != '_masks':
            assert torch.equal(grads[k], c['grads'][k]), k


def test_a_non_contiguous_rendered_mask_gives_the_same_numbers():
    c = case('main')
    B, R = c['blob']['_masks'].shape[0], c['blob']['_masks'].shape[-1]
    wide = torch.zeros(B, 1, R, R + 5, device=DEV)
    wide[..., 2:R + 2] = c['blob']['_masks'].to(DEV)
    wide.requires_grad_()
    bd = {k: v.detach().clone().requires_grad_() for k, v in c['bd'].items()}
    bd['_masks'] = wide[..., 2:R + 2]
    assert not bd['_masks'].is_contiguous()
    got = L.step_losses(bd, c['td'], TargetType.extend)
    weighted(got).backward()
    for k in ALL_KEYS:
        assert torch.equal(got[k], c['got'][k]), k
    assert torch.equal(wide.grad[..., 2:R + 2], c['grads']['_masks']) and not wide.grad[..., :2].any()


def test_two_runs_are_bit_identical():
    c = case('chunks')
    got, grads, _, _ = run_device(c['blob'], c['batch'], TargetType.extend)
    for k in ALL_KEYS:
        assert torch.equal(got[k], c['got'][k]), k
    for k in PRED_KEYS:
        assert torch.equal(grads[k], c['grads'][k]), k


def test_bad_shapes_are_refused_on_the_host_and_a_valid_call_still_succeeds():
    c = case('main')
    bd, td = c['bd'], c['td']
    B, S = td['masks'].shape[0], td['masks'].shape[-1]
    bad = [
        (dict(bd, _masks=torch.zeros(B, 1, S + 3, S + 3, device=DEV)), td),                                   # R - S odd
        (dict(bd, _masks=torch.zeros(B, 1, S - 2, S - 2, device=DEV)), td),                                   # R < S
        (bd, dict(td, masks=torch.zeros(B, 1, S, S + 1, device=DEV))),                                        # not square
        (dict(bd, _log_scales=bd['_log_scales'].detach().double()), td),                                      # float64 prediction
        (dict(bd, _masks=bd['_masks'].detach().double()), td),
    ]
    for blob, batch in bad:
        with pytest.raises(ValueError):
            L.step_losses(blob, batch, TargetType.extend)
        again = L.step_losses(bd, td, TargetType.extend)
        for k in ALL_KEYS:
            assert torch.equal(again[k], c['got'][k]), k
    with pytest.raises(NotImplementedError):
        L.step_losses(dict(bd, _masks=c['blob']['_masks']), td, TargetType.extend)


def test_the_library_refuses_an_odd_difference_itself():
    import sdn_hip
    c = case('main')
    bd, td = c['bd'], c['td']
    B = td['targets'].shape[0]
    scratch = torch.empty(sdn_hip.train_losses_scratch(B, 39, 8), dtype=torch.uint8, device=DEV)
    out = torch.empty(7, device=DEV)
    p = lambda t: t.data_ptr()
    for R, S in ((39, 32), (30, 32)):
        rc = sdn_hip.lib().sdn_train_losses_fwd(None, None, None, None, p(bd['_class_log_probs']), p(bd['_masks']), p(bd['_ffd_coeffs']), 8,
                                                None, None, None, None, p(td['masks']), p(td['ignores']), p(td['targets']), B, R, S, 2, 0.1, 1.0,
                                                p(scratch), p(out), None)
        assert rc == -1 and b'must be even' in sdn_hip.lib().sdn_last_error()


def test_a_training_step_on_the_fixture():
    """train_batch -> Derenderer3d in .train() -> step_losses -> backward -> one Adam step, on the fixture of tests/golden that
    geo_train_util loads; the losses against the fp64 evaluation of the same blob and batch tensors copied to the CPU"""
    import geo_train_util as u
    from derender3d import train_items as ti
    from test_gpu_dropin import _geometric_model
    frames, scenes, items, jitter, rois = u.batch_items(u.golden(), 't')
    batch = ti.train_batch(torch.tensor(frames).to(DEV), torch.tensor(np.ascontiguousarray(scenes)).to(DEV), items, True, jitter=jitter,
                           rois=rois)
    assert batch['masks'].shape[-1] == 256 and batch['images'].shape[-1] == 224
    net, _ = _geometric_model(render_size=384)      # the training size: p = 64
    net = net.to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-3)
    opt.zero_grad()
    blob = net(batch['images'], batch['roi_norms'], batch['focals'])
    got = L.step_losses(blob, batch, TargetType.extend)
    assert list(got) == list(ALL_KEYS)
    sum(got.values()).backward()
    opt.step()
    b64 = {k: blob[k].detach().cpu().double() for k in PRED_KEYS}
    t64 = {k: (v.cpu().double() if v.dtype == torch.float32 else v.cpu()) for k, v in batch.items()}
    ref = reference_losses(b64, t64, TargetType.extend, 0.1, 1.0)
    for k in ALL_KEYS:
        g, r = float(got[k].detach()), float(ref[k])
        print('fixture %s: device %.9g fp64 %.12g' % (k, g, r))
        assert np.isfinite(g) and abs(g - r) <= GATE * abs(r), (k, g, r)
    assert float(net.derenderer._fc3.weight.grad.abs().max()) > 0
    assert torch.isfinite(net.derenderer.net.conv1.weight.grad).all()
