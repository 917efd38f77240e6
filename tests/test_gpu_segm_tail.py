"""The semantic tail on the device (csrc/segm_tail.hip through semantic.segm_tail and the C ABI) against the reference's results
in tests/golden/segm_tail_golden.npz (tests/golden/make_segm_tail_golden.py).

Gates: probabilities within 4 e_ref of the float64 pipeline (e_ref = the reference's own fp32 error against it); labels equal
to argmax(pred64) wherever the top-two margin exceeds 8 e_ref, at most 0.1 % of the pixels inside that band; the tie and NaN
cases, the ground-truth labels, the counts and the summary exact."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'textural'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import segm_tail_util as u  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


def _case(gold, name):
    """(scores on the device, (H, W), pred64, e_ref, labels_ref)"""
    p = name + '/'
    if name == 'c':   # redrawn from the seed; tests/test_segm_tail_host.py holds the digest and the float64 sample
        seed, B, C, seg, sizes = u.CASES['c']
        scores = u.draw_scores(seed, B, C, sizes)
        assert u.digest(scores) == str(gold['c/scores_sha256'])
        pred64 = u.pipeline(scores, seg, torch.float64)
    else:
        scores = [gold[p + 'scores%d' % s] for s in range(int(gold[p + 'n_scales']))]
        seg = tuple(int(v) for v in gold[p + 'seg_size'])
        pred64 = torch.from_numpy(gold[p + 'pred64'])
    return [torch.from_numpy(t).cuda() for t in scores], seg, pred64, float(gold[p + 'e_ref']), gold[p + 'labels_ref']


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_fusion_meets_the_gates_on_the_fixture(gold, name):
    from semantic import segm_tail as st
    scores, seg, pred64, e_ref, _ = _case(gold, name)
    labels, pred = st.fuse_predictions(scores, seg, return_probs=True)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (pred64.shape[0], 1) + tuple(seg) and pred.dtype == torch.float32
    u.check_gates(name, pred.cpu(), labels.cpu(), pred64, e_ref)


@pytest.mark.parametrize('name', ['d', 'd0', 'e'])
def test_ties_and_nan_are_exact(gold, name):
    from semantic import segm_tail as st
    scores, seg, pred64, e_ref, labels_ref = _case(gold, name)
    labels, pred = st.fuse_predictions(scores, seg, return_probs=True)
    assert np.array_equal(labels[:, 0].cpu().numpy(), labels_ref)
    pred = pred.cpu()
    if name == 'e':
        hit = torch.from_numpy(gold['e/nan_pixels'])
        assert torch.equal(torch.isnan(pred).any(dim=1), hit) and torch.equal(torch.isnan(pred).all(dim=1), hit)
        assert bool((labels[:, 0].cpu()[hit] == 0).all())
    ok = ~torch.isnan(pred64)
    assert float((pred.double() - pred64)[ok].abs().max()) <= 4 * max(e_ref, 2.0 ** -24)   # d0: the reference's error is 0
    if name == 'd':
        assert torch.equal(pred[:, 2], pred[:, 5]) and bool((labels == 2).all())
    if name == 'd0':
        assert bool((labels == 0).all())


def test_hot_path_labels_equal_and_runs_are_bit_identical(gold):
    from semantic import segm_tail as st
    for name in ('a', 'c'):
        scores, seg, _, _, _ = _case(gold, name)
        labels, pred = st.fuse_predictions(scores, seg, return_probs=True)
        hot = st.fuse_predictions(scores, seg)
        assert isinstance(hot, torch.Tensor) and torch.equal(hot, labels)
        labels2, pred2 = st.fuse_predictions(scores, seg, return_probs=True)
        assert torch.equal(labels2, labels) and torch.equal(pred2.view(torch.int32), pred.view(torch.int32))


def test_a_canary_border_around_every_output_stays_untouched(gold):
    """Through the C ABI with every output placed inside a larger filled buffer."""
    import sdn_hip
    from sdn_hip import ops
    from semantic import segm_tail as st
    L = sdn_hip.lib()
    PAD = 256   # elements in front of and behind each output
    stream = sdn_hip.stream()

    def framed(n, dtype, fill):
        buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device='cuda')
        return buf, buf[PAD:PAD + n]

    def intact(buf, n, fill):
        return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())

    scores, (H, W), _, _, _ = _case(gold, 'c')
    B, C = scores[0].shape[:2]
    lab_buf, lab = framed(B * H * W, torch.uint8, 201)
    pred_buf, pred = framed(B * C * H * W, torch.float32, -7.5)
    table = ops.segm_scale_table(scores)
    sdn_hip.check(L.sdn_segm_fuse(table.ctypes.data, len(scores), B, C, H, W, lab.data_ptr(), pred.data_ptr(), stream))
    ref_lab, ref_pred = st.fuse_predictions(scores, (H, W), return_probs=True)
    assert intact(lab_buf, B * H * W, 201) and intact(pred_buf, B * C * H * W, -7.5)
    assert torch.equal(lab.view(B, 1, H, W), ref_lab) and torch.equal(pred.view(B, C, H, W), ref_pred)

    scene = torch.from_numpy(gold['eval/scene']).cuda()
    F, h, w = scene.shape[:3]
    t_host = st.color_table(gold['eval/codes'], gold['eval/labels'])
    t_dev = torch.from_numpy(t_host).cuda()
    gt_buf, gt = framed(F * h * w, torch.int16, 12345)
    unk_buf, unk = framed(F, torch.int32, -99)
    sdn_hip.check(L.sdn_segm_labels_from_colors(scene.data_ptr(), F, h, w, t_host.ctypes.data, t_dev.data_ptr(), t_host.size // 2,
                                                gt.data_ptr(), unk.data_ptr(), stream))
    assert intact(gt_buf, F * h * w, 12345) and intact(unk_buf, F, -99)
    assert np.array_equal(gt.view(F, h, w).cpu().numpy(), gold['eval/labels_gt']) and unk.tolist() == [0] * F

    Cn = int(gold['eval/num_class'])
    cols = 3 * Cn + 3
    cnt_buf, cnt = framed(F * cols, torch.int64, -5)
    plab = torch.from_numpy(gold['eval/pred']).cuda()
    sdn_hip.check(L.sdn_segm_confusion(plab.data_ptr(), gt.data_ptr(), F, h, w, Cn, cnt.data_ptr(), stream))
    assert intact(cnt_buf, F * cols, -5)
    assert np.array_equal(cnt.view(F, cols).cpu().numpy(), gold['eval/counts'])


def test_ground_truth_labels_counts_and_summary_equal_the_reference(gold):
    from semantic import segm_tail as st
    C = int(gold['eval/num_class'])
    scene = torch.from_numpy(gold['eval/scene']).cuda()
    gt, unknown = st.labels_from_colors(scene, gold['eval/codes'], gold['eval/labels'])
    assert gt.dtype == torch.int16 and np.array_equal(gt.cpu().numpy(), gold['eval/labels_gt']) and unknown.tolist() == [0, 0, 0, 0]
    pred = torch.from_numpy(gold['eval/pred']).cuda()[:, None].contiguous()
    ev = st.SegmEvaluator(C)
    ev.update(pred, gt)                       # four frames in one launch ...
    assert np.array_equal(ev.counts(), gold['eval/counts'])
    one = st.SegmEvaluator(C)
    for f in range(4):                        # ... and one by one
        one.update(pred[f:f + 1], gt[f:f + 1])
    assert np.array_equal(one.counts(), gold['eval/counts'])
    for s in (ev.summary(), one.summary()):
        assert np.array_equal(s['iou'], gold['eval/iou']) and s['mean_iou'] == float(gold['eval/mean_iou'])
        assert s['accuracy'] == float(gold['eval/accuracy']) and np.array_equal(s['acc_per_frame'], gold['eval/acc_per_frame'])
    # a colour outside the table: -32768, counted, and KeyError from the summary as from the reference's dictionary
    bad = torch.from_numpy(gold['eval/scene_unknown']).cuda()
    gt_bad, unk = st.labels_from_colors(bad, gold['eval/codes'], gold['eval/labels'])   # [H, W, 3]: one frame
    assert np.array_equal(gt_bad[0].cpu().numpy(), gold['eval/labels_gt_unknown']) and unk.tolist() == [int(gold['eval/unknown_count'])]
    ev.update(pred[:1], gt_bad)
    row = ev.counts()[4]
    want = gold['eval/counts'][0].copy()
    assert row[3 * C + 2] == 3 and row[3 * C + 1] <= want[3 * C + 1]
    with pytest.raises(KeyError, match='frame 4'):
        ev.summary()


@pytest.fixture(scope='module')
def full():
    """The VKITTI frame, five scales: seeded smooth scores (tests/segm_tail_util.py says why smooth), the float64 pipeline and
    e_ref from an fp32 torch run, all on the device."""
    seed, B, C, seg, sizes = u.FULL
    scores = [torch.from_numpy(t).cuda() for t in u.draw_smooth_scores(seed, B, C, sizes)]
    pred64 = u.pipeline(scores, seg, torch.float64, 'cuda')
    e_ref = float((u.pipeline(scores, seg, torch.float32, 'cuda').double() - pred64).abs().max())
    return scores, seg, pred64, e_ref


def test_full_size_frame_meets_the_gates(full):
    from semantic import segm_tail as st
    scores, seg, pred64, e_ref = full
    labels, pred = st.fuse_predictions(scores, seg, return_probs=True)
    u.check_gates('full', pred, labels, pred64, e_ref)
    assert torch.equal(st.fuse_predictions(scores, seg), labels)


def test_full_size_labels_and_counts_cross_frame_and_block_borders(full):
    """Two frames of 375 x 1242 (a frame is no multiple of four pixels: quads and waves straddle the frames) against torch."""
    from semantic import segm_tail as st
    scores, (H, W), _, _ = full
    C, B = 14, 2
    g = torch.Generator(device='cuda').manual_seed(5)
    codes = np.random.RandomState(6).randint(0, 256, (40, 3))
    codes = np.unique(codes, axis=0)
    K = len(codes)
    table_labels = np.arange(K) % 17                                   # label - 1 in -1 .. 15: unlabelled and >= C included
    pick = torch.randint(0, K, (B, H, W), device='cuda', generator=g)
    scene = torch.from_numpy(codes.astype(np.uint8)).cuda()[pick]      # [B, H, W, 3]
    scene[1, 374, 1241] = torch.tensor([1, 2, 3], dtype=torch.uint8, device='cuda')   # unknown, the last pixel
    scene[0, 374, 1240] = torch.tensor([1, 2, 3], dtype=torch.uint8, device='cuda')
    assert not (codes == (1, 2, 3)).all(axis=1).any()
    gt, unknown = st.labels_from_colors(scene, codes, table_labels)
    want = (torch.from_numpy(table_labels).cuda()[pick] - 1).to(torch.int16)
    want[1, 374, 1241] = -32768
    want[0, 374, 1240] = -32768
    assert torch.equal(gt, want) and unknown.tolist() == [1, 1]
    labels = st.fuse_predictions(scores, (H, W))
    labels = torch.cat((labels, labels.flip(3)), 0)
    counts = st.SegmEvaluator(C)
    counts.update(labels, gt)
    got = counts.counts()
    p, t = labels[:, 0].long(), gt.long()
    valid = t >= 0
    for b in range(B):
        row = [int(((p[b] == c) & (t[b] == c)).sum()) for c in range(C)] + [int(((p[b] == c) & valid[b]).sum()) for c in range(C)] + \
              [int((t[b] == c).sum()) for c in range(C)] + [int(((p[b] == t[b]) & valid[b]).sum()), int(valid[b].sum()), 1]
        assert got[b].tolist() == row, b


def test_labels_feed_the_textural_assembly_unchanged():
    """fuse_predictions' labels[b] is the uint8 [1, H, W] CUDA label map textural.data.assemble.assemble_item -- and through it
    EditSession(model, opt, params, base_segm_u8, ...) and assemble_batch -- take: same dtype, shape and result as the map
    uploaded from a file."""
    from data import assemble as asm
    from semantic import segm_tail as st
    from test_assemble import CASES, _frame, _opt
    opt = _opt(**CASES[5])
    segm, image, inst, _, _ = _frame(5)
    H, W = segm.shape
    t = lambda a: torch.from_numpy(a if a.ndim == 3 else a[:, :, None]).permute(2, 0, 1).contiguous().cuda()
    onehot = torch.nn.functional.one_hot(torch.from_numpy(segm).cuda().long(), 14).permute(2, 0, 1)[None].float().mul(9.0).contiguous()
    labels = st.fuse_predictions([onehot], (H, W))
    assert labels.dtype == torch.uint8 and tuple(labels[0].shape) == (1, H, W) and labels[0].is_contiguous()
    assert torch.equal(labels[0], t(segm))
    params = {'crop_pos': (3, 5), 'flip': False}
    a = asm.assemble_item(opt, params, labels[0], t(image), inst=t(inst))
    b = asm.assemble_item(opt, params, t(segm), t(image), inst=t(inst))
    for k in ('label', 'inst', 'image'):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
