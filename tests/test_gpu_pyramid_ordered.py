"""The ordered backward of the pyramid RoIAlign on the device (sdn_pyramid_roi_align_bwd_ordered, csrc/pyramid_roi_align.hip:
k_pra_box_records, k_pra_bwd_ordered), the path PyramidRoiAlignFn.backward takes under SDN_DETERMINISTIC=1 or
torch.use_deterministic_algorithms(True).

Reference: tests/pyramid_ordered_util.py, the entry point's contract in numpy -- the float32 terms of crop_and_resize.c:241-247, added
in float64 to +0.0 per destination, rounded to float32 once.  The gate is equality of bits: tests/test_pyramid_ordered_host.py shows
on every case used here that the float64 sum of these terms does not depend on their order, so whatever fixed order the kernel takes
must give the restatement's bits.  The gradients are compared as int32 views, so that a NaN compares too: the NaN that 0 * inf
and inf - inf generate and the NaN that a NaN gradient passes on have the same pattern on the device as in numpy on the host."""
import ctypes

import numpy as np
import pytest
import torch

import pyramid_ordered_util as o
import pyramid_roi_align_util as u
from sdn_hip import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                # guard floats on both sides: 256 bytes, so the 16-byte alignment stays


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture
def ordered(monkeypatch):
    monkeypatch.setenv('SDN_DETERMINISTIC', '1')
    assert ops.pyramid_backward_path() == 'ordered'


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty that fills what it returns: NaN for floats, 99 for integers -- whatever a kernel leaves unwritten shows"""
    real_empty = torch.empty

    def poison(t):
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(99)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: poison(real_empty(*a, **k)))


def autograd(c):
    """the four gradients through ops.pyramid_roi_align and autograd, on the path the switches select now: numpy arrays"""
    boxes = torch.from_numpy(c['boxes'].copy()).to(DEV)
    maps = [torch.from_numpy(m.copy()).to(DEV).requires_grad_(True) for m in c['maps']]
    pooled, levels = ops.pyramid_roi_align(boxes, maps, c['pool'], u.IMAGE_AREA)
    assert np.array_equal(levels.cpu().numpy(), u.levels(c))
    pooled.backward(torch.from_numpy(c['grads'].copy()).to(DEV))
    return [m.grad.cpu().numpy() for m in maps]


_done = {}


def device_case(name):
    """the ordered path's answer to a case, computed once and shared (read-only); call it under the `ordered` fixture"""
    if name not in _done:
        assert ops.pyramid_backward_path() == 'ordered'
        _done[name] = autograd(o.make_case(name))
    return _done[name]


def c_abi(c, guard=0, ws_guard=0):
    """sdn_pyramid_roi_align_bwd_ordered called directly, into buffers with `guard` NaN floats (workspace: `ws_guard` bytes of 0xAB) on
    both sides: (the whole gradient buffer, the whole workspace, offsets, total, workspace bytes)"""
    import sdn_hip
    R, C, pool = c['R'], c['C'], c['pool']
    H, W = [m.shape[1] for m in c['maps']], [m.shape[2] for m in c['maps']]
    offsets, total = ops.pyramid_grad_floats(C, H, W)
    nbytes = ops.pyramid_ordered_workspace_bytes(R)
    boxes = torch.from_numpy(c['boxes'].copy()).to(DEV)
    g = torch.from_numpy(c['grads'].copy()).to(DEV)
    gbuf = torch.full((total + 2 * guard,), float('nan'), device=DEV)
    ws = torch.full((nbytes + 2 * ws_guard,), 0xAB, dtype=torch.uint8, device=DEV)
    ints = lambda v: (ctypes.c_int * 4)(*v)   # noqa: E731
    sdn_hip.check(sdn_hip.lib().sdn_pyramid_roi_align_bwd_ordered(g.data_ptr(), boxes.data_ptr(), R, ints(H), ints(W), C, pool, u.IMAGE_AREA,
                                                                  gbuf.data_ptr() + 4 * guard, ws.data_ptr() + ws_guard, nbytes, sdn_hip.stream()))
    torch.cuda.synchronize()
    return gbuf.cpu().numpy(), ws.cpu().numpy(), offsets, total, nbytes


def split(inner, c, offsets):
    return [inner[at:at + m.size].reshape(m.shape) for at, m in zip(offsets, c['maps'])]


@pytest.mark.parametrize('name', o.ALL_CASES)
def test_the_gradients_are_the_contracts_bits(gold, ordered, name):
    c, got, want = o.make_case(name), device_case(name), o.ordered_backward(name)
    lv = u.levels(c)
    reached = o.reached(c)
    for l in range(u.LEVELS):
        assert got[l].dtype == np.float32 and got[l].shape == c['maps'][l].shape
        differing = int((o.bits(got[l]) != o.bits(want[l])).sum())
        print('%s P%d: %d of %d elements differ from the contract' % (name, l + 2, differing, got[l].size))
        assert differing == 0, (name, l, differing)
        untouched = got[l][:, ~reached[l]]
        assert not untouched.any() and not np.signbit(untouched).any(), l                      # +0.0, the sign bit clear
        if not (lv == l + 2).any():
            assert not o.bits(got[l]).any(), l                                                  # a level without a box: all +0.0
    if name in u.CASES:
        want64 = [gold[name + '/grad64_%d' % l] for l in range(u.LEVELS)]
        err, gate = u.grad_error(got, want64), gold[name + '/gate']
        assert (err <= gate).all(), (err, gate)


@pytest.mark.parametrize('name', ['chunks', 'big'])
def test_three_runs_and_the_c_abi_give_identical_bytes(ordered, name):
    c = o.make_case(name)
    first = device_case(name)
    for _ in range(2):
        again = autograd(c)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first))
    buf, _ws, offsets, _total, _n = c_abi(c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(split(buf, c, offsets), first))


def test_the_c_abi_writes_every_float_inside_its_buffers_and_nothing_outside(ordered, poisoned_empty):
    name = 'c67'                                     # C * H * W of P2 is 2010 floats: two floats of padding before P3
    c = o.make_case(name)
    buf, ws, offsets, total, nbytes = c_abi(c, guard=GUARD, ws_guard=256)
    assert offsets[1] - c['C'] * c['maps'][0].shape[1] * c['maps'][0].shape[2] == 2
    assert np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + total:]).all() and len(buf) == total + 2 * GUARD      # nothing outside is touched
    inner = buf[GUARD:GUARD + total]
    assert not np.isnan(inner).any()                                                            # every float inside is overwritten
    used = np.zeros(total, bool)
    for at, m in zip(offsets, c['maps']):
        used[at:at + m.size] = True
    assert not used[2010:2012].any() and (~used).sum() == total - sum(m.size for m in c['maps']) == 3          # two floats after P2, one after P4
    assert not o.bits(inner[~used]).any()                                                       # the padding: +0.0
    assert (ws[:256] == 0xAB).all() and (ws[256 + nbytes:] == 0xAB).all() and nbytes == 32 * c['R']
    records = ws[256:256 + nbytes].view(np.int32).reshape(c['R'], 8)
    assert np.array_equal(records[:, 0], u.levels(c) - 2) and not records[:, 5:].any()           # every box of c67 has a sample inside
    want = o.ordered_backward(name)
    assert all((o.bits(a) == o.bits(b)).all() for a, b in zip(split(inner, c, offsets), want))
    # autograd: torch.empty's poison survives in no gradient, and the four are views of one buffer at the library's offsets
    boxes = torch.from_numpy(c['boxes'].copy()).to(DEV)
    maps = [torch.from_numpy(m.copy()).to(DEV).requires_grad_(True) for m in c['maps']]
    out, _ = ops.pyramid_roi_align(boxes, maps, c['pool'], u.IMAGE_AREA)
    grads = torch.autograd.grad(out, maps, torch.from_numpy(c['grads'].copy()).to(DEV))
    assert all(grads[l].data_ptr() - grads[0].data_ptr() == 4 * offsets[l] for l in range(u.LEVELS))
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 1
    assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(grads, split(inner, c, offsets)))


def test_no_box_gives_gradients_of_positive_zeros(ordered, poisoned_empty):
    c = o.make_case('mixed7')
    boxes = torch.from_numpy(c['boxes'][:0].copy()).to(DEV)
    maps = [torch.from_numpy(m.copy()).to(DEV).requires_grad_(True) for m in c['maps']]
    out, levels = ops.pyramid_roi_align(boxes, maps, 7, u.IMAGE_AREA)
    assert tuple(out.shape) == (0, c['C'], 7, 7) and tuple(levels.shape) == (0,)
    out.sum().backward()
    for m in maps:
        assert m.grad.shape == m.shape and not o.bits(m.grad.cpu().numpy()).any()               # all bits clear: +0.0


def test_nothing_waits_for_the_device(ordered):
    c = o.make_case('mixed14')
    device_case('mixed14')                           # the library is loaded and the case is known before the mode is set
    boxes = torch.from_numpy(c['boxes'].copy()).to(DEV)
    maps = [torch.from_numpy(m.copy()).to(DEV).requires_grad_(True) for m in c['maps']]
    g = torch.from_numpy(c['grads'].copy()).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')          # torch raises on anything that makes the host wait for the stream
    try:
        out, _ = ops.pyramid_roi_align(boxes, maps, c['pool'], u.IMAGE_AREA)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert all(m.grad.cpu().numpy().tobytes() == w.tobytes() for m, w in zip(maps, device_case('mixed14')))


def test_a_captured_forward_and_backward_replays_on_new_gradients_and_boxes(ordered):
    c, second = o.make_case('mixed7'), o.make_case('nonfinite')          # the same R and shapes
    rs = np.random.RandomState(77)
    new_boxes = u.draw_boxes(rs, 'mixed', c['R'])
    boxes = torch.from_numpy(c['boxes'].copy()).to(DEV)
    g = torch.from_numpy(c['grads'].copy()).to(DEV)
    maps = [torch.from_numpy(m.copy()).to(DEV).requires_grad_(True) for m in c['maps']]

    def step():
        out, _ = ops.pyramid_roi_align(boxes, maps, c['pool'], u.IMAGE_AREA)
        return torch.autograd.grad(out, maps, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    boxes.copy_(torch.from_numpy(new_boxes).to(DEV))
    g.copy_(torch.from_numpy(second['grads'].copy()).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.cpu().numpy() for t in captured]
    eager = autograd(dict(c, boxes=new_boxes, grads=second['grads']))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(replayed, eager))
    assert any(np.isnan(a).any() or np.isinf(a).any() for a in replayed)                         # the new gradients were read
    want = o.ordered_backward(dict(c, boxes=new_boxes, grads=second['grads']))
    assert all((o.bits(a) == o.bits(b)).all() for a, b in zip(replayed, want))


def test_the_default_is_still_the_atomic_path_and_torchs_switch_selects_the_ordered_one(gold, monkeypatch):
    monkeypatch.delenv('SDN_DETERMINISTIC', raising=False)
    before = torch.are_deterministic_algorithms_enabled()
    c = o.make_case('mixed7')
    try:
        torch.use_deterministic_algorithms(False)
        assert ops.pyramid_backward_path() == 'atomic'
        got = autograd(c)
        want64 = [gold['mixed7/grad64_%d' % l] for l in range(u.LEVELS)]
        assert (u.grad_error(got, want64) <= gold['mixed7/gate']).all()
        torch.use_deterministic_algorithms(True)
        assert ops.pyramid_backward_path() == 'ordered'
        by_torch = autograd(c)
    finally:
        torch.use_deterministic_algorithms(before)
    monkeypatch.setenv('SDN_DETERMINISTIC', '1')
    assert all(a.tobytes() == b.tobytes() for a, b in zip(by_torch, device_case('mixed7')))
    assert all((o.bits(a) == o.bits(b)).all() for a, b in zip(by_torch, o.ordered_backward('mixed7')))
