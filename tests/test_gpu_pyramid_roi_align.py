"""maskrcnn.pyramid (sdn_pyramid_roi_align_fwd / _bwd, csrc/pyramid_roi_align.hip) against the reference's pyramid_roi_align: the
fixture tests/golden/pyramid_roi_align_golden.npz holds what the reference's own functions gave on its own C crop
(tests/golden/make_pyramid_roi_align_golden.py), tests/pyramid_roi_align_util.py restates them in numpy.

Levels and the pooled values are exact: equal integers, equal bits.  The map gradients are sums of fp32 atomic adds in no fixed
order; per level map they must lie within the fixture's gate of the float64 gradients, relative to that map's largest float64
gradient magnitude: 1e-6, or four times the distance of the reference's own serial float32 sum where that is more (the R = 1000
case, where a pixel of the 3 x 3 map collects thousands of terms).  A level no box was routed to has a gradient of exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

import pyramid_roi_align_util as u
from maskrcnn import pyramid   # the feature itself: without it this module does not import
from maskrcnn.roialign.roi_align.crop_and_resize import CropAndResizeFunction

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty that fills what it returns: NaN for floats, 99 for integers -- whatever a kernel leaves unwritten shows"""
    real_empty = torch.empty

    def poison(t):
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(99)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: poison(real_empty(*a, **k)))


def device_inputs(c, batch=True, grad=True):
    lift = (lambda t: t[None]) if batch else (lambda t: t)
    boxes = lift(torch.from_numpy(c['boxes'].copy())).to(DEV)
    maps = [lift(torch.from_numpy(m.copy())).to(DEV).requires_grad_(grad) for m in c['maps']]
    return [boxes] + maps


_done = {}


def case(name):
    """the device's answer to a fixture case, computed once and shared (read-only): pooled, levels and the four gradients as numpy"""
    if name not in _done:
        c = u.draw_case(name)
        inputs = device_inputs(c)
        keep = list(inputs)
        pooled, levels = pyramid.pyramid_levels(inputs, c['pool'], u.IMAGE_SHAPE)
        assert all(a is b for a, b in zip(inputs, keep))
        pooled.backward(torch.from_numpy(c['grads'].copy()).to(DEV))
        grads = [m.grad for m in inputs[1:]]
        assert all(g.shape == m.shape for g, m in zip(grads, inputs[1:]))
        _done[name] = dict(pooled=pooled.detach().cpu().numpy(), levels=levels.cpu().numpy(), grads=[g[0].cpu().numpy() for g in grads])
    return _done[name]


@pytest.mark.parametrize('name', list(u.CASES))
def test_levels_and_pooled_values_are_the_references(gold, name):
    c, d = u.draw_case(name), case(name)
    p = name + '/'
    assert d['levels'].dtype == np.int32 and np.array_equal(d['levels'], gold[p + 'levels'])
    assert d['pooled'].dtype == np.float32 and d['pooled'].shape == (c['R'], c['C'], c['pool'], c['pool'])
    assert u.checksum(d['pooled']) == int(gold[p + 'crc_pooled'])
    want = gold[p + 'pooled'] if name in u.STORED_WHOLE else u.forward(c, np.float32)
    assert d['pooled'].tobytes() == want.tobytes()                       # bit for bit, in box order


@pytest.mark.parametrize('name', list(u.CASES))
def test_map_gradients_are_within_the_fixtures_gate_of_float64(gold, name):
    d = case(name)
    p = name + '/'
    want = [gold[p + 'grad64_%d' % l] for l in range(u.LEVELS)]
    err, gate = u.grad_error(d['grads'], want), gold[p + 'gate']
    print('%s: distance from the float64 gradients per level %s; the reference\'s float32 run %s; gate %s'
          % (name, ' '.join('%.3g' % e for e in err), ' '.join('%.3g' % e for e in gold[p + 'fp32_error']), ' '.join('%.3g' % g for g in gate)))
    assert all(g.dtype == np.float32 and g.shape == w.shape for g, w in zip(d['grads'], want))
    assert (err <= gate).all(), (err, gate)
    for l in range(u.LEVELS):
        if not (gold[p + 'levels'] == l + 2).any():
            assert not d['grads'][l].any() and not np.signbit(d['grads'][l]).any(), l          # exact +0.0
        else:
            assert d['grads'][l].any()
        # where no sample reads, no gradient arrives: the zeros of the float64 gradient are zeros here
        assert not d['grads'][l][want[l] == 0].any(), l


def _composition(boxes, maps, pool):
    """the reference's loop (model.py:459-500) on this library's CropAndResizeFunction, levels from the float64 restatement"""
    lv = torch.from_numpy(u.levels_of(u.level_values(boxes.cpu().numpy()))).to(DEV)
    pooled, order = [], []
    for l in range(u.LEVELS):
        ix = torch.nonzero(lv == l + 2)[:, 0]
        if not len(ix):
            continue
        ind = torch.zeros(len(ix), dtype=torch.int32, device=DEV)
        pooled.append(CropAndResizeFunction(pool, pool, 0)(maps[l][None], boxes[ix], ind))
        order.append(ix)
    _, back = torch.sort(torch.cat(order))
    return torch.cat(pooled)[back], lv


@pytest.mark.parametrize('pool,C,R', [(7, 70, 300), (14, 9, 61), (2, 130, 41)])
def test_forward_is_the_per_level_composition_of_crop_and_resize(pool, C, R):
    rs = np.random.RandomState(7000 + pool)
    boxes = np.concatenate([u.draw_boxes(rs, 'mixed', R - R // 3), u.draw_boxes(rs, 'outside', R // 3)])
    maps = [torch.from_numpy(rs.randn(C, h, w).astype(np.float32)).to(DEV) for h, w in ((40, 33), (20, 17), (10, 9), (5, 4))]
    boxes = torch.from_numpy(boxes).to(DEV)
    want, lv = _composition(boxes, maps, pool)
    got, levels = pyramid.pyramid_levels([boxes[None]] + [m[None] for m in maps], pool, u.IMAGE_SHAPE)
    assert torch.equal(levels, lv.to(torch.int32)) and len(set(lv.tolist())) == 4
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))      # the same bits


def test_the_c_abi_writes_inside_its_buffers_only_and_backward_matches_it(gold):
    """outputs inside larger NaN-filled buffers; pooled.sum().backward() against sdn_pyramid_roi_align_bwd on ones"""
    import sdn_hip
    from sdn_hip import ops
    name = 'c67'                                     # C * H * W of P2 is 2010 floats: two floats of padding before P3
    c = u.draw_case(name)
    R, C, pool = c['R'], c['C'], c['pool']
    H, W = [m.shape[1] for m in c['maps']], [m.shape[2] for m in c['maps']]
    offsets, total = ops.pyramid_grad_floats(C, H, W)
    assert offsets[1] - C * H[0] * W[0] == 2
    G = 64                                           # guard floats on both sides: 256 bytes, so the 16-byte alignment stays
    n = R * C * pool * pool
    boxes = torch.from_numpy(c['boxes'].copy()).to(DEV)
    maps = [torch.from_numpy(m.copy()).to(DEV) for m in c['maps']]
    pooled = torch.full((n + 2 * G,), float('nan'), device=DEV)
    levels = torch.full((R + 2 * G,), 99, dtype=torch.int32, device=DEV)
    gbuf = torch.full((total + 2 * G,), float('nan'), device=DEV)
    ones = torch.ones(n, device=DEV)
    L = sdn_hip.lib()
    ints = lambda v: (ctypes.c_int * 4)(*v)   # noqa: E731
    ptrs = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
    sdn_hip.check(L.sdn_pyramid_roi_align_fwd(boxes.data_ptr(), R, ptrs, ints(H), ints(W), C, pool, u.IMAGE_AREA, 0.0, pooled.data_ptr() + 4 * G,
                                              levels.data_ptr() + 4 * G, sdn_hip.stream()))
    sdn_hip.check(L.sdn_pyramid_roi_align_bwd(ones.data_ptr(), boxes.data_ptr(), R, ints(H), ints(W), C, pool, u.IMAGE_AREA,
                                              gbuf.data_ptr() + 4 * G, sdn_hip.stream()))
    torch.cuda.synchronize()
    for buf, size in ((pooled, n), (gbuf, total)):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + size:]).all() and not torch.isnan(buf[G:G + size]).any()
    assert (levels[:G] == 99).all() and (levels[G + R:] == 99).all()
    assert np.array_equal(levels[G:G + R].cpu().numpy(), gold[name + '/levels'])
    assert pooled[G:G + n].cpu().numpy().tobytes() == case(name)['pooled'].tobytes()
    inner = gbuf[G:G + total].cpu().numpy()
    used = np.zeros(total, bool)
    for o, h, w in zip(offsets, H, W):
        used[o:o + C * h * w] = True
    assert not inner[~used].any() and (~used).sum() == total - C * sum(h * w for h, w in zip(H, W))      # the padding is zeroed too
    # autograd on the same boxes and maps, the gradient of pooled.sum()
    inputs = device_inputs(c, batch=False)
    out, _ = ops.pyramid_roi_align(inputs[0], inputs[1:], pool, u.IMAGE_AREA)
    grads = torch.autograd.grad(out.sum(), inputs[1:])
    # four views of one buffer, at the library's offsets
    assert all(grads[l].data_ptr() - grads[0].data_ptr() == 4 * offsets[l] for l in range(u.LEVELS))
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 1
    truth = u.backward(dict(c, grads=np.ones_like(c['grads'])))
    gate = gold[name + '/gate']
    cabi = [inner[o:o + C * h * w].reshape(C, h, w) for o, h, w in zip(offsets, H, W)]
    auto = [g.cpu().numpy() for g in grads]
    e_cabi, e_auto = u.grad_error(cabi, truth), u.grad_error(auto, truth)
    print('ones: C ABI within %s, autograd within %s of float64' % (e_cabi, e_auto))
    # both are atomic sums of the same terms: each within the gate of the float64 gradient, so within twice the gate of each other
    assert (e_cabi <= gate).all() and (e_auto <= gate).all()
    assert (u.grad_error(auto, [np.asarray(g, np.float64) for g in cabi]) <= 2 * gate * 1.001).all()


def test_no_box_gives_an_empty_result_and_zero_gradients(poisoned_empty):
    c = u.draw_case('mixed7')
    inputs = device_inputs(c)
    inputs[0] = inputs[0][:, :0]
    out, levels = pyramid.pyramid_levels(inputs, 7, u.IMAGE_SHAPE)
    assert tuple(out.shape) == (0, c['C'], 7, 7) and out.dtype == torch.float32 and tuple(levels.shape) == (0,) and levels.dtype == torch.int32
    assert tuple(pyramid.pyramid_roi_align(inputs, 14, u.IMAGE_SHAPE).shape) == (0, c['C'], 14, 14)
    out.sum().backward()
    for m in inputs[1:]:
        assert m.grad.shape == m.shape and not m.grad.any() and not torch.isnan(m.grad).any()      # the zero fill ran


def test_maps_with_and_without_the_batch_axis_give_the_same(gold, poisoned_empty):
    name = 'thin'
    c, d = u.draw_case(name), case(name)
    inputs = device_inputs(c, batch=False)
    out = pyramid.pyramid_roi_align(inputs, c['pool'], u.IMAGE_SHAPE)
    assert out.detach().cpu().numpy().tobytes() == d['pooled'].tobytes()
    out.backward(torch.from_numpy(c['grads'].copy()).to(DEV))
    want = [gold[name + '/grad64_%d' % l] for l in range(u.LEVELS)]
    got = [m.grad.cpu().numpy() for m in inputs[1:]]
    assert all(g.shape == w.shape for g, w in zip(got, want))
    assert (u.grad_error(got, want) <= gold[name + '/gate']).all()
    # a mix of both forms, and the boxes without their batch axis
    mixed = [inputs[0], inputs[1].detach()[None], inputs[2].detach(), inputs[3].detach()[None], inputs[4].detach()]
    assert torch.equal(pyramid.pyramid_roi_align(mixed, c['pool'], u.IMAGE_SHAPE), out)


def test_nothing_waits_for_the_device_and_the_boxes_get_no_gradient():
    c = u.draw_case('mixed14')
    inputs = device_inputs(c)
    inputs[0].requires_grad_()                    # the reference detaches the boxes (model.py:473)
    g = torch.from_numpy(c['grads'].copy()).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')       # torch raises on anything that makes the host wait for the stream
    try:
        out, levels = pyramid.pyramid_levels(inputs, c['pool'], u.IMAGE_SHAPE)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert inputs[0].grad is None and not levels.requires_grad and all(m.grad is not None for m in inputs[1:])
    assert out.detach().cpu().numpy().tobytes() == case('mixed14')['pooled'].tobytes()


def test_tensors_the_kernels_cannot_take_are_refused():
    c = u.draw_case('single')
    inputs = device_inputs(c, grad=False)
    with pytest.raises(TypeError, match='P3 must be torch.float32'):
        pyramid.pyramid_roi_align(inputs[:2] + [inputs[2].double()] + inputs[3:], 7, u.IMAGE_SHAPE)
    with pytest.raises(TypeError, match='boxes must be torch.float32'):
        pyramid.pyramid_roi_align([inputs[0].half()] + inputs[1:], 7, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match='P2 must be contiguous'):
        pyramid.pyramid_roi_align([inputs[0], inputs[1].transpose(2, 3).contiguous().transpose(2, 3)] + inputs[2:], 7, u.IMAGE_SHAPE)
    with pytest.raises(NotImplementedError, match='P5 is on cpu'):
        pyramid.pyramid_roi_align(inputs[:4] + [inputs[4].cpu()], 7, u.IMAGE_SHAPE)
    for pool in (0, 33):
        with pytest.raises(ValueError, match='1 to 32 are supported'):
            pyramid.pyramid_roi_align(inputs, pool, u.IMAGE_SHAPE)
    with pytest.raises(ValueError, match='image_area'):
        pyramid.pyramid_roi_align(inputs, 7, (0, 1024, 3))
    # the largest pool the sample table takes
    out = pyramid.pyramid_roi_align(inputs, 32, u.IMAGE_SHAPE)
    want = u.forward(dict(c, pool=32), np.float32)
    assert out.cpu().numpy().tobytes() == want.tobytes()
