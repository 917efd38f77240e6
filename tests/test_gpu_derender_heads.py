"""sdn_hip.ops.derender_heads and derender3d.models.heads on the GPU against the float64 restatement (tests/derender_heads_util.py).

Gate (derender_heads_util.gate): every output group and every gradient lies within 1e-6 of that group's largest float64 magnitude, or,
where the float32 restatement's own distance from float64 is larger, within 4 x that distance.  Every figure is printed before it is
asserted.  The references are computed once per case on the CPU and shared."""
import pytest
import torch

import derender_heads_util as u
from derender3d.models import heads as model_heads      # the feature itself: without it this module does not import
from sdn_hip import ops
from sdn_hip.ops import derender_heads

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = 'cuda:0'
GATED = [name for name in u.CASES if name != 'zero_row']
GRADS = ('pooled',) + u.PARAMS


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def poisoned():
    """fill the allocator's free blocks with a pattern torch.empty would hand back"""
    junk = [torch.full((n,), float('nan'), device=DEV) for n in (1 << 12, 1 << 16, 1 << 20)]
    del junk


def on_device(name, requires_grad=False):
    pooled, roi_norms, params = u.draw(name)
    return (pooled.to(DEV).requires_grad_(requires_grad), roi_norms.to(DEV),
            [p.to(DEV).requires_grad_(requires_grad) for p in params])


def call(pooled, rois, params, classes):
    return derender_heads(pooled, rois, params[0:2], params[2:4], params[4:6], params[6:8], classes)


def within(what, got, want64, want32):
    distance, bound, own, scale = u.gate(got, want64, want32)
    print('%s: %.3e from float64 (largest magnitude %.3e, float32 restatement %.3e, gate %.3e)' % (what, distance, scale, own, bound))
    assert not torch.isnan(got).any(), what
    assert distance <= bound, what


@pytest.mark.parametrize('name', GATED)
def test_forward_meets_the_gate_and_the_roi_vectors_are_torchs(name):
    ref = u.reference(name)
    pooled, roi_norms, params = on_device(name)
    classes = u.widths(name)[2]
    poisoned()
    blob = call(pooled, roi_norms, params, classes)
    assert list(blob) == list(u.KEYS) + ['_mroi_norms', '_droi_norms']
    for k in u.KEYS:
        assert blob[k].shape == ref['out64'][k].shape and blob[k].is_contiguous(), k
        within('%s %s' % (name, k), blob[k], ref['out64'][k], ref['out32'][k])
    top_left, bottom_right = roi_norms[:, 0:2], roi_norms[:, 2:4]
    assert bits(blob['_mroi_norms']) == bits((bottom_right + top_left) / 2.0) and bits(blob['_droi_norms']) == bits(bottom_right - top_left)
    # the pair form gives the same bits, and so does a second run
    pair = call(pooled, (blob['_mroi_norms'], blob['_droi_norms']), params, classes)
    again = call(pooled, roi_norms, params, classes)
    assert list(pair) == list(u.KEYS)
    for k in u.KEYS:
        assert bits(pair[k]) == bits(blob[k]) and bits(again[k]) == bits(blob[k]), k
    sums = blob['_class_probs'].sum(dim=1)
    assert float((sums - 1).abs().max()) <= 1e-6 and float(blob['_class_probs'].min()) >= 0.0


def run_backward(name, subset, pooled_grad=True, frozen=()):
    pooled, roi_norms, params = on_device(name, requires_grad=True)
    pooled.requires_grad_(pooled_grad)
    for i in frozen:
        params[i].requires_grad_(False)
    g = u.out_grads(name)
    poisoned()
    blob = call(pooled, roi_norms, params, u.widths(name)[2])
    torch.autograd.backward([blob[k] for k in subset], [g[k].to(DEV) for k in subset])
    return dict(zip(GRADS, [pooled.grad] + [p.grad for p in params]))


@pytest.mark.parametrize('name', GATED)
def test_backward_of_all_six_meets_the_gate_and_repeats(name):
    ref = u.reference(name)
    got = run_backward(name, u.KEYS)
    for k in GRADS:
        assert got[k].shape == ref['grad64'][k].shape, k
        within('%s d %s' % (name, k), got[k], ref['grad64'][k], ref['grad32'][k])
    again = run_backward(name, u.KEYS)
    assert all(bits(got[k]) == bits(again[k]) for k in GRADS)


@pytest.mark.parametrize('name', ['real_17', 'odd'])
@pytest.mark.parametrize('subset', [('_ffd_coeffs',), ('_class_probs',), ('_theta_deltas', '_log_depths')])
def test_gradient_subsets_meet_the_gate(name, subset):
    ref = u.reference(name, subset)
    got = run_backward(name, subset)
    for k in GRADS:
        within('%s %s d %s' % (name, '+'.join(subset), k), got[k], ref['grad64'][k], ref['grad32'][k])


@pytest.mark.parametrize('name', ['real_17', 'odd'])
def test_a_gradient_not_asked_for_is_none_and_the_others_stay(name):
    ref = u.reference(name)
    full = run_backward(name, u.KEYS)
    got = run_backward(name, u.KEYS, pooled_grad=False)
    assert got['pooled'] is None
    assert all(bits(got[k]) == bits(full[k]) for k in u.PARAMS)
    got = run_backward(name, u.KEYS, frozen=(2, 3))                  # fc1 frozen
    assert got['fc1.weight'] is None and got['fc1.bias'] is None
    for k in GRADS:
        if not k.startswith('fc1.'):
            assert bits(got[k]) == bits(full[k]), k
            within('%s, fc1 frozen, d %s' % (name, k), got[k], ref['grad64'][k], ref['grad32'][k])
    got = run_backward(name, u.KEYS, pooled_grad=False, frozen=(0, 1, 2, 3))   # the backbone detached, net.fc and fc1 frozen
    assert [k for k in GRADS if got[k] is None] == ['pooled', 'fc.weight', 'fc.bias', 'fc1.weight', 'fc1.bias']
    assert all(bits(got[k]) == bits(full[k]) for k in ('fc2.weight', 'fc2.bias', 'fc3.weight', 'fc3.bias'))


def test_every_row_of_a_batch_is_the_row_computed_alone():
    pooled, roi_norms, params = on_device('real_17')
    batch = call(pooled, roi_norms, params, 8)
    for r in range(17):
        alone = call(pooled[r:r + 1].contiguous(), roi_norms[r:r + 1].contiguous(), params, 8)
        for k in list(u.KEYS) + ['_mroi_norms', '_droi_norms']:
            assert bits(alone[k][0]) == bits(batch[k][r]), (r, k)


def test_a_nan_feature_row_leaves_the_other_rows_alone():
    pooled, roi_norms, params = on_device('real_17')
    clean = call(pooled, roi_norms, params, 8)
    dirty = pooled.clone()
    dirty[5, 100] = float('nan')
    got = call(dirty, roi_norms, params, 8)
    others = [r for r in range(17) if r != 5]
    for k in u.KEYS:
        assert bits(got[k][others]) == bits(clean[k][others]), k
    assert torch.isnan(got['_ffd_coeffs'][5]).all() and torch.isnan(got['_class_probs'][5]).all()


def test_the_zero_pose_pair_gives_nan_in_its_two_outputs_only():
    ref = u.reference('zero_row')
    pooled, roi_norms, params = on_device('zero_row')
    blob = call(pooled, roi_norms, params, 3)
    nan = torch.isnan(blob['_theta_deltas'].cpu())
    want = torch.zeros(5, 2, dtype=torch.bool)
    want[u.ZERO_ROW] = True
    assert torch.equal(nan, want) and torch.equal(torch.isnan(ref['out64']['_theta_deltas']), want)
    rows = [r for r in range(5) if r != u.ZERO_ROW]
    within('zero_row _theta_deltas', blob['_theta_deltas'][rows], ref['out64']['_theta_deltas'][rows], ref['out32']['_theta_deltas'][rows])
    for k in u.KEYS[1:]:
        within('zero_row ' + k, blob[k], ref['out64'][k], ref['out32'][k])


def test_logits_of_plus_and_minus_1e4_give_finite_probabilities():
    pooled, roi_norms, params = on_device('real_16')
    params[7] = params[7].clone()
    params[7][8:16] = torch.tensor([1e4, -1e4, 1e4, -1e4, -1e4, 1e4, -1e4, 1e4], device=DEV)
    probs = call(pooled, roi_norms, params, 8)['_class_probs']
    assert torch.isfinite(probs).all()
    print('sums of the probabilities: within %.3e of 1' % float((probs.sum(dim=1) - 1).abs().max()))
    assert float((probs.sum(dim=1) - 1).abs().max()) <= 1e-6
    assert float(probs[:, [1, 3, 4, 6]].max()) == 0.0 and float(probs[:, [0, 2, 5, 7]].min()) > 0.0


def test_the_plain_slices_are_the_kernels_own_row():
    """the C entry point's optional `row` output: _fc3's own result, of which four output groups are copies"""
    name = 'odd'
    f, hd, classes, coeffs, O, n = u.widths(name)
    pooled, roi_norms, params = on_device(name)
    blob = call(pooled, roi_norms, params, classes)
    out, row = torch.empty(n * O, device=DEV), torch.full((n, O), float('nan'), device=DEV)
    saved, centre, extent = torch.empty(n * (3 * hd + 1), device=DEV), torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
    import sdn_hip
    p = sdn_hip.ptr
    sdn_hip.check(sdn_hip.lib().sdn_derender_heads_fwd(p(pooled), p(roi_norms), None, None, *[p(t) for t in params], n, f, hd, classes, coeffs,
                                                       p(out), p(centre), p(extent), p(row), p(saved), sdn_hip.stream()))
    assert bits(row[:, 2:4]) == bits(blob['_translation2ds']) and bits(row[:, 4:7]) == bits(blob['_log_scales'])
    assert bits(row[:, 7:8]) == bits(blob['_log_depths']) and bits(row[:, 8 + classes:]) == bits(blob['_ffd_coeffs'].reshape(n, -1))
    assert not torch.isnan(row).any()
    ref = u.reference(name)
    within('odd row', row, ref['keep64']['row'], ref['keep32']['row'])
    norm = torch.norm(row[:, 0:2].double(), dim=1)                          # the saved norm, the last n floats of `saved`
    assert float((saved[3 * n * hd:].double() - norm).abs().max()) <= 1e-6 * float(norm.max())


def test_a_captured_forward_replays_on_new_features():
    pooled, roi_norms, params = on_device('real_16')
    other = torch.rand(16, 512, generator=torch.Generator().manual_seed(77)).to(DEV)
    static = pooled.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call(static, roi_norms, params, 8)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call(static, roi_norms, params, 8)
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in captured.items()}
    eager = call(other, roi_norms, params, 8)
    first = call(pooled, roi_norms, params, 8)
    for k in eager:
        assert bits(replayed[k]) == bits(eager[k]), k
    assert bits(first['_ffd_coeffs']) != bits(eager['_ffd_coeffs'])          # the replay did read the new contents


def test_an_empty_batch_returns_empty_tensors():
    _pooled, _roi, params = on_device('odd')
    blob = call(torch.empty(0, 36, device=DEV), torch.empty(0, 4, device=DEV), params, 3)
    assert blob['_ffd_coeffs'].shape == (0, 3, 24) and blob['_class_probs'].shape == (0, 3) and blob['_mroi_norms'].shape == (0, 2)


# ---- module level ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def module():
    from derender3d.models.derenderer import Derenderer
    torch.manual_seed(11)
    model = Derenderer(num_classes=3, grid_size=2).to(DEV).eval()
    g = torch.Generator().manual_seed(12)
    images = torch.rand(5, 3, 64, 64, generator=g).to(DEV)
    top_left = -torch.rand(5, 2, generator=g) * 0.5
    roi_norms = torch.cat((top_left, top_left + 0.1 + torch.rand(5, 2, generator=g) * 0.5), dim=1).to(DEV)
    return model, images, roi_norms


def test_the_module_switch_keeps_keys_shapes_and_parameters_and_meets_the_gate(module):
    model, images, roi_norms = module
    centre, extent = (roi_norms[:, 2:4] + roi_norms[:, 0:2]) / 2.0, roi_norms[:, 2:4] - roi_norms[:, 0:2]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        features = model.net.pooled(images)
        assert features.shape == (5, 512)
        # the three calls below see these very features: the backbone's split-K sums may differ in the last bit from run to run, and
        # this test is about what stands behind the pooling
        model.net.__dict__['pooled'] = lambda x: features
        try:
            model(images, centre, extent)
            off = model(images, centre, extent)
            with model_heads.use_device_heads(model):
                assert model.__dict__['_device_heads'] is True
                on = model(images, centre, extent)
            after = model(images, centre, extent)
        finally:
            del model.net.__dict__['pooled']
    assert '_device_heads' not in model.__dict__
    assert list(on) == list(off) and all(on[k].shape == off[k].shape for k in off)
    assert all(bits(after[k]) == bits(off[k]) for k in off)                  # remove() restores today's bits
    now = model.state_dict()
    assert list(now) == list(before) and all(bits(now[k]) == bits(before[k]) for k in before)
    params = [now[k].cpu() for k in ('net.fc.weight', 'net.fc.bias', 'fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', '_fc3.weight', '_fc3.bias')]
    want32 = u.heads(features.cpu(), (centre.cpu(), extent.cpu()), params, 3)
    want64 = u.heads(features.cpu().double(), (centre.cpu().double(), extent.cpu().double()), [p.double() for p in params], 3)
    for k in u.KEYS:
        within('module ' + k, on[k], want64[k], want32[k])


def test_a_training_step_through_the_switch_reaches_every_parameter(module):
    from derender3d import TargetType, losses
    model, images, roi_norms = module
    centre, extent = (roi_norms[:, 2:4] + roi_norms[:, 0:2]) / 2.0, roi_norms[:, 2:4] - roi_norms[:, 0:2]
    g = torch.Generator().manual_seed(13)
    batch = {'targets': torch.full((5,), int(TargetType.geometry), dtype=torch.int64, device=DEV),
             'thetas': (torch.rand(5, 1, generator=g) * 6 - 3).to(DEV), 'translation2ds': torch.rand(5, 2, generator=g).to(DEV),
             'log_scales': torch.rand(5, 3, generator=g).to(DEV), 'log_depths': torch.rand(5, 1, generator=g).to(DEV)}
    model.train()
    try:
        model.zero_grad()
        with model_heads.use_device_heads(model):
            blob = model(images, centre, extent)
            loss = sum(losses.step_losses(blob, batch, TargetType.geometry).values()) + blob['_ffd_coeffs'].square().mean() + \
                blob['_class_probs'][:, 0].mean()
            loss.backward()
        assert torch.isfinite(loss)
        for name, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert float(model.net.conv1.weight.grad.abs().max()) > 0 and float(model._fc3.weight.grad.abs().max()) > 0
    finally:
        model.eval()
        model.zero_grad()
