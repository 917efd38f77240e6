#!/usr/bin/env python3
"""Generate tests/golden/segm_tail_golden.npz: the reference's semantic tail, executed on the CPU.

Imported from the reference as it lies: accuracy, intersectionAndUnion and AverageMeter of semantic/utils.py, and -- where
semantic/models.py imports under this torch -- the `use_softmax` tail of its decoder: a C1Bilinear(use_softmax=True) whose two
conv layers are replaced by identities runs models.py:302-303 (upsample, softmax) on our score maps.  tests/segm_tail_util.py's
`pipeline` (the same torch.nn.functional calls) must equal it bit for bit; where models.py does not import, `pipeline` is used
alone.  The fixture's key `tail` says which happened.  The multi-scale loop is vkitti_test.py:58-72, the ground-truth map
vkitti_dataset.py:208-209, 238 (restated: the dataset class needs cv2 and image files), the summary vkitti_eval.py:83-107.

Per fusion case: the score maps, pred32 / labels_ref (fp32, torch.max on the CPU), pred64 (the same calls in float64),
e_ref = max |pred32 - pred64|.  Case c is too large for a committed file (see tests/segm_tail_util.py): its maps are redrawn from
the seed (SHA-256 stored) and its probabilities stored as a strided sample.  Runs only where the reference exists.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
sys.path.insert(0, os.path.join(REF, 'semantic'))

import segm_tail_util as u   # noqa: E402
from utils import AverageMeter, accuracy, intersectionAndUnion   # noqa: E402  (the reference's semantic/utils.py)

warnings.filterwarnings('ignore')
try:
    import models as ref_models   # the reference's semantic/models.py
    TAIL = 'semantic/models.py C1Bilinear(use_softmax=True), :302-303'
except Exception as e:   # noqa: BLE001
    ref_models = None
    TAIL = 'torch.nn.functional (models.py did not import: %r)' % (e,)


def reference_pred(scores, seg_size, dtype):
    mine = u.pipeline(scores, seg_size, dtype)
    if ref_models is None:
        return mine
    dec = ref_models.C1Bilinear(num_class=scores[0].shape[1], fc_dim=8, use_softmax=True)
    dec.cbr = torch.nn.Sequential()
    dec.conv_last = torch.nn.Sequential()
    pred = torch.zeros_like(mine)
    with torch.no_grad():
        for t in scores:   # vkitti_test.py:61-70
            pred_tmp = dec([torch.as_tensor(t).to(dtype)], segSize=tuple(seg_size))
            pred = pred + pred_tmp / len(scores)
    both_nan = torch.isnan(pred) & torch.isnan(mine)
    assert bool(((pred == mine) | both_nan).all()), 'the restated pipeline differs from the reference decoder tail'
    return pred


def fuse_case(out, name, scores, seg_size, exact=False, store_full=True):
    pred32 = reference_pred(scores, seg_size, torch.float32)
    pred64 = reference_pred(scores, seg_size, torch.float64)
    _, labels_ref = torch.max(pred32, dim=1)   # vkitti_test.py:72
    ok = ~torch.isnan(pred64)
    e_ref = float((pred32.double() - pred64)[ok].abs().max())
    p = name + '/'
    out[p + 'seg_size'] = np.asarray(seg_size, dtype=np.int32)
    out[p + 'n_scales'] = np.int32(len(scores))
    out[p + 'labels_ref'] = labels_ref.numpy().astype(np.uint8)
    out[p + 'e_ref'] = np.float64(e_ref)
    if store_full:
        for s, t in enumerate(scores):
            out[p + 'scores%d' % s] = t
        out[p + 'pred32'] = pred32.numpy()
        out[p + 'pred64'] = pred64.numpy()
    else:
        out[p + 'scores_sha256'] = u.digest(scores)
        out[p + 'pred32_sample'] = pred32.numpy().reshape(-1)[::u.SAMPLE_STRIDE]
        out[p + 'pred64_sample'] = pred64.numpy().reshape(-1)[::u.SAMPLE_STRIDE]
    if not exact:
        arg, margin = u.margins(pred64)
        clear = margin > 8 * e_ref
        band = 1.0 - float(clear.double().mean())
        assert band <= 0.001, 'case %s: %.4f %% of the pixels inside the 8 e_ref band: change the seed' % (name, 100 * band)
        assert bool((labels_ref[clear] == arg[clear]).all()), 'case %s: labels_ref differs from argmax(pred64) outside the band' % name
        out[p + 'band'] = np.float64(band)
    print('case %s: e_ref %.3e, labels %s' % (name, e_ref, np.bincount(labels_ref.numpy().ravel())[:8]))
    return pred32, labels_ref


def eval_frames(out):
    """Four frames of 23 x 31, C = 14: random, one with labels >= C, one without a valid pixel, one small; plus a frame with
    a colour outside the table."""
    C, H, W = 14, 23, 31
    rs = np.random.RandomState(21)
    K = 20
    codes = rs.randint(0, 256, (K, 3)).astype(np.uint8)
    codes[3] = (0, 0, 0)
    codes[4] = (255, 255, 255)
    labels = np.concatenate(([0, 0], np.arange(1, 17), [15, 16])).astype(np.int64)   # label - 1 reaches 14 and 15: >= C
    table_segm = {tuple(int(v) for v in c): int(l) for c, l in zip(codes, labels)}
    assert len(table_segm) == K
    frames, preds = [], []
    for f in range(4):
        if f == 2:
            pick = rs.randint(0, 2, (H, W))                  # labels 0 only: no valid pixel
        elif f == 1:
            pick = rs.randint(0, K, (H, W))                  # everything, labels >= C included
        else:
            pick = rs.randint(0, 16, (H, W))                 # label - 1 in -1 .. 13
        frames.append(codes[pick])
        guess = rs.randint(0, C, (H, W)).astype(np.int64)
        if f == 0:   # a good share of hits
            guess = np.where(rs.rand(H, W) < 0.6, (labels[pick] - 1).clip(0, C - 1), guess)
        preds.append(guess)
    scene = np.stack(frames)                                           # uint8 [4, H, W, 3]
    pred = np.stack(preds)
    gts, rows = [], []
    acc_meter, intersection_meter, union_meter = AverageMeter(), AverageMeter(), AverageMeter()
    accs = []
    for f in range(4):
        segm = np.apply_along_axis(lambda a: table_segm[(a[0], a[1], a[2])], 2, scene[f])   # vkitti_dataset.py:208
        segm = segm.astype(np.uint8)                                                       # :209
        seg_label = segm.astype(np.int64) - 1                                              # :234-238
        acc, pix = accuracy(pred[f], seg_label)                                            # vkitti_eval.py:84-88
        intersection, union = intersectionAndUnion(pred[f], seg_label, C)
        acc_meter.update(acc, pix)
        intersection_meter.update(intersection)
        union_meter.update(union)
        accs.append(acc)
        # the two histograms intersectionAndUnion keeps to itself (utils.py:113-126)
        imPred = (pred[f] + 1) * ((seg_label + 1) > 0)
        area_pred, _ = np.histogram(imPred, bins=C, range=(1, C))
        area_lab, _ = np.histogram(seg_label + 1, bins=C, range=(1, C))
        assert np.array_equal(area_pred + area_lab - intersection, union)
        valid = seg_label >= 0
        rows.append(np.concatenate((intersection, area_pred, area_lab, [(valid * (pred[f] == seg_label)).sum(), pix, 0])))
        gts.append(seg_label.astype(np.int16))
    iou = intersection_meter.sum / (union_meter.sum + 1e-10)   # vkitti_eval.py:101
    out['eval/num_class'] = np.int32(C)
    out['eval/codes'] = codes
    out['eval/labels'] = labels.astype(np.int32)
    out['eval/scene'] = scene
    out['eval/pred'] = pred.astype(np.uint8)
    out['eval/labels_gt'] = np.stack(gts)
    out['eval/counts'] = np.stack(rows).astype(np.int64)
    out['eval/acc_per_frame'] = np.asarray(accs, dtype=np.float64)
    out['eval/iou'] = np.asarray(iou, dtype=np.float64)
    out['eval/mean_iou'] = np.float64(iou.mean())
    out['eval/accuracy'] = np.float64(acc_meter.average())
    assert (np.stack(gts) >= C).any() and rows[2][3 * C + 1] == 0 and rows[0][3 * C] > 0
    # a colour outside the table: the reference raises KeyError; here the pixel gets -32768 and is counted
    bad = scene[0].copy()
    where = [(0, 0), (5, 30), (22, 7)]
    for y, x in where:
        bad[y, x] = (1, 2, 3)
    assert (1, 2, 3) not in table_segm
    try:
        np.apply_along_axis(lambda a: table_segm[(a[0], a[1], a[2])], 2, bad)
        raise AssertionError('the reference did not raise')
    except KeyError:
        pass
    gt_bad = gts[0].copy()
    for y, x in where:
        gt_bad[y, x] = -32768
    out['eval/scene_unknown'] = bad
    out['eval/labels_gt_unknown'] = gt_bad
    out['eval/unknown_count'] = np.int32(len(where))
    print('eval: accuracy %.6f, mean IoU %.6f, valid pixels %s' % (acc_meter.average(), iou.mean(), [int(r[3 * C + 1]) for r in rows]))


def main():
    out = {'tail': TAIL}
    for name in ('a', 'b', 'c'):
        seed, B, C, seg, sizes = u.CASES[name]
        fuse_case(out, name, u.draw_scores(seed, B, C, sizes), seg, store_full=(name != 'c'))
    # d: exact ties.  Channel 5 is a copy of channel 2 and both dominate: label 2 everywhere; all-equal scores: label 0
    d = u.draw_scores(31, 1, 8, [(4, 6), (7, 9)])
    for t in d:
        t[:, 2] += 12.0
        t[:, 5] = t[:, 2]
    _, lab = fuse_case(out, 'd', d, (12, 20), exact=True)
    assert bool((lab == 2).all())
    _, lab = fuse_case(out, 'd0', [np.full((1, 8, 4, 6), 1.5, np.float32), np.full((1, 8, 7, 9), -2.0, np.float32)], (12, 20), exact=True)
    assert bool((lab == 0).all())
    # e: one NaN pixel in one scale
    e = u.draw_scores(32, 1, 6, [(5, 9), (8, 20)])
    e[0][0, 3, 2, 4] = np.nan
    pred32, lab = fuse_case(out, 'e', e, (16, 40), exact=True)
    hit = torch.isnan(pred32).any(dim=1)
    assert 0 < int(hit.sum()) < hit.numel() and bool((lab[hit] == 0).all()), 'torch.max does not give 0 at the NaN pixels'
    clean = [t.copy() for t in e]
    clean[0][0, 3, 2, 4] = 0.0
    _, lab_clean = torch.max(u.pipeline(clean, (16, 40)), dim=1)
    assert bool((lab[~hit] == lab_clean[~hit]).all())
    out['e/nan_pixels'] = hit.numpy()
    eval_frames(out)
    path = os.path.join(HERE, 'segm_tail_golden.npz')
    np.savez_compressed(path, **out)
    print('tail:', TAIL)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
