"""sdn_hip.ops.rpn_outputs on the GPU against the torch expressions of the RPN's tail (tests/predict_util.py: rpn_tail).

Logits and boxes are copies and must be bit-equal.  The probabilities are measured against the float64 softmax of the same logits;
the gate is the larger of 2^-22 (four ulps of 1: exp is the only inexact step) and four times the largest distance of torch's CPU
fp32 softmax from that float64 run.  Backward without grad_probs is a copy and must be bit-equal to autograd through the torch
expressions; with grad_probs it is measured against float64 autograd under the same gate, for incoming gradients in (-1, 1).
Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import predict_util as u
from maskrcnn import predict as pr          # noqa: F401  the feature itself: without it this module does not import
from maskrcnn.proposals import proposals_padded
from sdn_hip.ops import rpn_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = 'cuda:0'
PYRAMID = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]
CASES = {
    'tails': (PYRAMID, 3, 1),             # run tails: 15 and 6 pixels in a 64-pixel tile, 960 = 15 tiles
    'k1_unaligned': (PYRAMID, 1, 1),      # level bases not 16-byte aligned: the 3 x 5 level ends at float 30 of its run
    'k5_odd': (PYRAMID, 5, 1),
    'one_pixel': ([(1, 1)], 3, 1),
    'batch2': (PYRAMID, 3, 2),
    'several_groups': ([(64, 64)], 3, 1),
}
FLOOR = 2.0 ** -22


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def draw(name, requires_grad=False, seed=21):
    levels, k, B = CASES[name]
    cls, box = u.draw_maps(levels, k, B, seed)
    on = lambda ts: [t.to(DEV).requires_grad_(requires_grad) for t in ts]   # noqa: E731
    return cls, box, on(cls), on(box)


def reference(cls, box):
    """(fp32 torch expressions on the CPU, float64 softmax of the same logits, the gate)"""
    want = u.rpn_tail(cls, box)
    exact = u.rpn_tail([c.double() for c in cls], [b.double() for b in box])[1]
    cpu_distance = float((want[1].double() - exact).abs().max())
    return want, exact, cpu_distance, max(FLOOR, 4.0 * cpu_distance)


def poisoned():
    """fill the allocator's free blocks with a pattern torch.empty would hand back"""
    junk = [torch.full((n,), float('nan'), device=DEV) for n in (1 << 12, 1 << 16, 1 << 20)]
    del junk


@pytest.mark.parametrize('name', list(CASES))
def test_forward_copies_bit_for_bit_and_the_probabilities_meet_the_gate(name):
    cls, box, dcls, dbox = draw(name)
    want, exact, cpu_distance, gate = reference(cls, box)
    poisoned()
    logits, probs, bbox = rpn_outputs(dcls, dbox)
    assert logits.shape == want[0].shape and probs.shape == want[1].shape and bbox.shape == want[2].shape
    assert bits(logits) == bits(want[0]) and bits(bbox) == bits(want[2])
    distance = float((probs.cpu().double() - exact).abs().max())
    print('%s: probabilities within %.3e of float64 (torch CPU fp32: %.3e, gate %.3e)' % (name, distance, cpu_distance, gate))
    assert distance <= gate
    assert not torch.isnan(probs).any() and float(probs.min()) >= 0.0 and float(probs.max()) <= 1.0
    again = rpn_outputs(dcls, dbox)
    assert all(bits(a) == bits(b) for a, b in zip(again, (logits, probs, bbox)))       # two runs, the same bits


def test_inputs_that_are_views_at_a_4_byte_offset():
    levels, k = PYRAMID, 3
    cls, box = u.draw_maps(levels, k, 1, seed=22)
    want = u.rpn_tail(cls, box)
    buffer = torch.zeros(sum(t.numel() + 2 for t in cls + box) + 1, device=DEV)
    at, dcls, dbox = 1, [], []                     # every view starts an odd number of floats into the 16-byte aligned buffer
    for c, b in zip(cls, box):
        for t, out in ((c, dcls), (b, dbox)):
            view = buffer[at:at + t.numel()].view(t.shape)
            view.copy_(t)
            out.append(view)
            at += t.numel() + (2 if t.numel() % 2 == 0 else 1)
    assert all(v.data_ptr() % 8 == 4 and v.is_contiguous() for v in dcls + dbox)
    logits, probs, bbox = rpn_outputs(dcls, dbox)
    exact = u.rpn_tail([c.double() for c in cls], [b.double() for b in box])[1]
    assert bits(logits) == bits(want[0]) and bits(bbox) == bits(want[2])
    assert float((probs.cpu().double() - exact).abs().max()) <= max(FLOOR, 4.0 * float((want[1].double() - exact).abs().max()))


def test_non_finite_logits_have_torchs_nan_pattern():
    inf, nan = float('inf'), float('nan')
    rows = [(inf, 0.0), (-inf, -inf), (nan, 0.0), (0.0, nan), (-inf, 0.0), (0.0, inf), (1.0, 2.0)]
    cls = [torch.tensor(rows).t().reshape(1, 2, 1, len(rows)).contiguous()]
    box = [torch.zeros(1, 4, 1, len(rows))]
    want = u.rpn_tail(cls, box)[1][0]
    _logits, probs, _bbox = rpn_outputs([cls[0].to(DEV)], [box[0].to(DEV)])
    got = probs[0].cpu()
    print('torch:', want.tolist(), 'kernel:', got.tolist())
    assert torch.isnan(want[0]).all() and torch.isnan(want[1]).all() and torch.isnan(want[2]).all()   # the issue's three rows
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    finite = ~torch.isnan(want)
    assert float((got[finite].double() - want[finite].double()).abs().max()) <= FLOOR


@pytest.mark.parametrize('name', ['tails', 'k1_unaligned', 'k5_odd', 'one_pixel', 'batch2', 'several_groups'])
def test_backward_without_grad_probs_is_autograd_bit_for_bit(name):
    cls, box, dcls, dbox = draw(name, requires_grad=True)
    ccls, cbox = [c.clone().requires_grad_(True) for c in cls], [b.clone().requires_grad_(True) for b in box]
    want = u.rpn_tail(ccls, cbox)
    g = torch.Generator().manual_seed(23)
    g_logits, g_bbox = torch.randn(want[0].shape, generator=g), torch.randn(want[2].shape, generator=g)
    torch.autograd.backward([want[0], want[2]], [g_logits, g_bbox])
    poisoned()
    logits, _probs, bbox = rpn_outputs(dcls, dbox)
    torch.autograd.backward([logits, bbox], [g_logits.to(DEV), g_bbox.to(DEV)])
    for got, ref in zip(dcls + dbox, ccls + cbox):
        assert got.grad.shape == ref.grad.shape and bits(got.grad) == bits(ref.grad)
    first = [t.grad.clone() for t in dcls + dbox]
    for t in dcls + dbox:
        t.grad = None
    logits, _probs, bbox = rpn_outputs(dcls, dbox)
    torch.autograd.backward([logits, bbox], [g_logits.to(DEV), g_bbox.to(DEV)])
    assert all(bits(t.grad) == bits(f) for t, f in zip(dcls + dbox, first))             # two runs, the same bits


def test_backward_of_one_output_alone_writes_zeros_for_the_others():
    _cls, _box, dcls, dbox = draw('tails', requires_grad=True)
    poisoned()
    _logits, _probs, bbox = rpn_outputs(dcls, dbox)
    bbox.sum().backward()
    assert all(bits(t.grad) == bits(torch.zeros_like(t)) for t in dcls)                 # no poison of torch.empty is left
    assert all(bits(t.grad) == bits(torch.ones_like(t)) for t in dbox)


@pytest.mark.parametrize('name', ['tails', 'k1_unaligned', 'batch2'])
def test_backward_with_grad_probs_meets_the_gate_against_float64(name):
    cls, box, dcls, dbox = draw(name, requires_grad=True)
    c64, b64 = [c.double().requires_grad_(True) for c in cls], [b.double().requires_grad_(True) for b in box]
    c32, b32 = [c.clone().requires_grad_(True) for c in cls], [b.clone().requires_grad_(True) for b in box]
    g = torch.Generator().manual_seed(24)
    B, A = cls[0].shape[0], sum(c.shape[1] // 2 * c.shape[2] * c.shape[3] for c in cls)
    g_logits, g_probs = torch.rand(B, A, 2, generator=g) * 2 - 1, torch.rand(B, A, 2, generator=g) * 2 - 1     # magnitudes below 1
    g_bbox = torch.rand(B, A, 4, generator=g) * 2 - 1
    for maps_c, maps_b, cast in ((c64, b64, torch.float64), (c32, b32, torch.float32)):
        out = u.rpn_tail(maps_c, maps_b)
        torch.autograd.backward(out, [g_logits.to(cast), g_probs.to(cast), g_bbox.to(cast)])
    poisoned()
    out = rpn_outputs(dcls, dbox)
    torch.autograd.backward(list(out), [g_logits.to(DEV), g_probs.to(DEV), g_bbox.to(DEV)])
    # the forward's gate: the incoming gradients lie in (-1, 1), so the class gradient g_logit + p * (g_p - <g_p, p>) has the size of
    # a probability and exp stays the only inexact function
    cpu_distance = max(float((a.grad.double() - b.grad).abs().max()) for a, b in zip(c32, c64))
    gate = max(FLOOR, 4.0 * cpu_distance)
    distance = max(float((a.grad.cpu().double() - b.grad).abs().max()) for a, b in zip(dcls, c64))
    print('%s: class gradients within %.3e of float64 (torch CPU fp32: %.3e, gate %.3e)' % (name, distance, cpu_distance, gate))
    assert distance <= gate
    for got, ref in zip(dbox, b32):
        assert bits(got.grad) == bits(ref.grad)                                         # the boxes' gradient stays a copy


def test_a_captured_rpn_outputs_and_proposal_layer_replays_on_new_maps():
    cfg = u.config()
    anchors = torch.from_numpy(u.anchors64().astype(np.float32)).to(DEV)
    levels = list(u.SHAPES)
    first, second = u.draw_maps(levels, 3, 1, seed=31), u.draw_maps(levels, 3, 1, seed=32)
    static_cls, static_box = [t.to(DEV) for t in first[0]], [t.to(DEV) for t in first[1]]

    def step():
        _logits, probs, bbox = rpn_outputs(static_cls, static_box)
        return proposals_padded([probs, bbox * 0.1], cfg.POST_NMS_ROIS_TRAINING, cfg.RPN_NMS_THRESHOLD, anchors, cfg)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rois, count = step()
    for dst, src in zip(static_cls + static_box, second[0] + second[1]):
        dst.copy_(src.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = (rois.clone(), count.clone())
    eager = step()
    assert bits(replayed[0]) == bits(eager[0]) and bits(replayed[1]) == bits(eager[1]) and int(eager[1]) > 1
    for dst, src in zip(static_cls + static_box, first[0] + first[1]):
        dst.copy_(src.to(DEV))
    other = step()
    assert bits(other[0]) != bits(eager[0])                                             # the replay did read the new contents
