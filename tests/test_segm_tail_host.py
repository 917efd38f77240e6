"""The semantic tail without a GPU: ABI 18 and its three entry points in the header, the binding and the library; argument
errors through the C ABI; the colour and scale tables; SegmEvaluator's float64 arithmetic on the reference's stored counts; the
fixture's self-consistency (tests/golden/make_segm_tail_golden.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sdn_hip  # noqa: E402
import segm_tail_util as u  # noqa: E402
from sdn_hip import ops  # noqa: E402
from semantic import segm_tail as st  # noqa: E402

NAMES = ('sdn_segm_fuse', 'sdn_segm_labels_from_colors', 'sdn_segm_confusion')


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


def test_header_binding_and_library_agree_on_abi_18_and_the_names():
    header = open(os.path.join(ROOT, 'include', 'sdn_hip.h')).read()
    version = int(re.search(r'#define\s+SDN_ABI_VERSION\s+(\d+)', header).group(1))
    L = sdn_hip.lib()
    assert version == sdn_hip.ABI_VERSION == L.sdn_version() and version >= 18
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % n, code), n
        assert n in sdn_hip.exported_symbols() and hasattr(L, n)
        assert getattr(L, n).argtypes is not None
    mk = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'Makefile')).read()
    assert 'segm_tail.hip' in re.search(r'EXACT_SRC\s*:=(.*)', mk).group(1)   # no FMA contraction, no SLP vectoriser


def _table(rows):
    t = np.zeros((len(rows), 2), dtype=np.uint64)
    for s, (addr, h, w) in enumerate(rows):
        t[s] = (addr, (w << 32) | h)
    return t.view(np.int32).reshape(len(rows), 4)


def test_argument_errors_through_the_c_abi():
    L = sdn_hip.lib()
    fake = ctypes.c_void_p(4096)
    err = lambda: L.sdn_last_error().decode()
    ok = _table([(8192, 5, 7), (8192, 8, 11)])
    fuse = lambda t, S, B, C, H, W, lab=fake, pred=None: L.sdn_segm_fuse(t.ctypes.data if t is not None else None, S, B, C, H, W, lab, pred, None)
    assert fuse(None, 2, 1, 14, 37, 50) == -1 and 'null pointer' in err()
    assert fuse(ok, 2, 1, 14, 37, 50, lab=None) == -1 and 'null pointer' in err()
    assert fuse(ok, 0, 1, 14, 37, 50) == -1 and 'scales' in err()
    assert fuse(np.tile(ok, (5, 1))[:9].copy(), 9, 1, 14, 37, 50) == -1 and 'scales' in err()
    assert fuse(ok, 2, 1, 0, 37, 50) == -1 and 'classes' in err()
    assert fuse(ok, 2, 1, 33, 37, 50) == -1 and 'classes' in err()
    assert fuse(ok, 2, 0, 14, 37, 50) == -1 and 'frames' in err()
    assert fuse(ok, 2, 1, 14, 0, 50) == -1 and 'bad sizes' in err()
    assert fuse(ok, 2, 1, 14, 37, 50, pred=ctypes.c_void_p(4098)) == -1 and 'aligned' in err()
    assert fuse(_table([(0, 5, 7)]), 1, 1, 14, 37, 50) == -1 and 'null address' in err()
    assert fuse(_table([(8194, 5, 7)]), 1, 1, 14, 37, 50) == -1 and 'not aligned' in err()
    assert fuse(_table([(8192, 0, 7)]), 1, 1, 14, 37, 50) == -1 and 'bad sizes' in err()
    assert fuse(_table([(8192, 75, 7)]), 1, 1, 14, 37, 50) == -1 and 'at most twice' in err()

    tab = np.array([5, 70000, 0xffffff, 1, 0, 255], dtype=np.int32)
    col = lambda scene=fake, B=1, H=4, W=4, t=tab, dev=fake, K=3, out=fake, unk=fake: L.sdn_segm_labels_from_colors(
        scene, B, H, W, t.ctypes.data if t is not None else None, dev, K, out, unk, None)
    assert col(scene=None) == -1 and 'null pointer' in err()
    assert col(t=None) == -1 and 'null pointer' in err()
    assert col(unk=None) == -1 and 'null pointer' in err()
    assert col(H=0) == -1 and 'bad sizes' in err()
    assert col(B=0) == -1 and 'bad sizes' in err()
    assert col(out=ctypes.c_void_p(4100)) == -1 and 'aligned' in err()
    assert col(scene=ctypes.c_void_p(4097)) == -1 and 'aligned' in err()
    assert col(K=0) == -1 and 'colour codes' in err()
    assert col(t=np.zeros(2050, np.int32), K=1025) == -1 and 'colour codes' in err()
    assert col(t=np.array([7, 5, 1, 2], np.int32), K=2) == -1 and 'not sorted' in err()
    assert col(t=np.array([5, 5, 1, 2], np.int32), K=2) == -1 and 'not sorted' in err()
    assert col(t=np.array([5, 1 << 24, 1, 2], np.int32), K=2) == -1 and 'a code is' in err()
    assert col(t=np.array([5, 6, 1, 256], np.int32), K=2) == -1 and 'outside 0 .. 255' in err()

    conf = lambda lab=fake, gt=fake, B=1, H=4, W=4, C=14, out=fake: L.sdn_segm_confusion(lab, gt, B, H, W, C, out, None)
    assert conf(lab=None) == -1 and 'null pointer' in err()
    assert conf(out=None) == -1 and 'null pointer' in err()
    assert conf(W=0) == -1 and 'bad sizes' in err()
    assert conf(C=0) == -1 and 'classes' in err()
    assert conf(C=257) == -1 and 'classes' in err()
    assert conf(gt=ctypes.c_void_p(4097)) == -1 and 'aligned' in err()
    assert conf(out=ctypes.c_void_p(4100)) == -1 and 'aligned' in err()


def test_cpu_tensors_raise_like_the_rest_of_the_library():
    with pytest.raises(NotImplementedError):
        st.fuse_predictions([torch.zeros(1, 3, 4, 4)], (8, 8))
    with pytest.raises(NotImplementedError):
        st.labels_from_colors(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), [[0, 0, 0]], [1])
    with pytest.raises(NotImplementedError):
        st.SegmEvaluator(14).update(torch.zeros(1, 1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int16))
    with pytest.raises(ValueError):
        st.fuse_predictions([], (8, 8))
    with pytest.raises(ValueError):
        st.SegmEvaluator(14).summary()


def test_colour_table_is_packed_and_sorted():
    codes = [[255, 0, 0], [0, 0, 1], [0, 1, 0], [255, 0, 0], [7, 7, 7]]
    t = st.color_table(codes, [3, 1, 2, 3, 0])
    assert t.dtype == np.int32 and t.tolist() == [255, 256, 0x010000, 0x070707, 3, 2, 1, 0]   # r | g << 8 | b << 16, a duplicate folded
    with pytest.raises(ValueError, match='two labels'):
        st.color_table(codes, [3, 1, 2, 4, 0])
    with pytest.raises(ValueError):
        st.color_table([[0, 0, 256]], [1])
    with pytest.raises(ValueError):
        st.color_table([[0, 0, 0]], [256])
    with pytest.raises(ValueError):
        st.color_table(np.zeros((0, 3)), np.zeros(0))
    rs = np.random.RandomState(3)
    big = rs.randint(0, 256, (1024, 3))
    big = np.unique(big, axis=0)
    t = st.color_table(big, np.arange(len(big)) % 256)
    K = t.size // 2
    assert K == len(big) and np.all(np.diff(t[:K]) > 0)
    packed = big[:, 0] | (big[:, 1] << 8) | (big[:, 2] << 16)
    for k in (0, 5, K - 1):   # every colour finds its own label
        assert t[K + np.searchsorted(t[:K], packed[k])] == k % 256
    with pytest.raises(ValueError, match='at most'):
        c = np.stack(np.unravel_index(np.arange(1025), (256, 256, 256)), 1)
        st.color_table(c, np.zeros(1025, int))


def test_scale_table_rows():
    a, b = torch.zeros(2, 3, 5, 7), torch.zeros(2, 3, 8, 11)
    t = ops.segm_scale_table([a, b])
    assert t.dtype == np.int32 and t.shape == (2, 4)
    assert t.view(np.uint64)[:, 0].tolist() == [a.data_ptr(), b.data_ptr()]
    assert t[:, 2].tolist() == [5, 8] and t[:, 3].tolist() == [7, 11]


def test_summary_equals_the_reference_numbers_exactly(gold):
    C = int(gold['eval/num_class'])
    s = st.summarize(gold['eval/counts'], C)
    assert np.array_equal(s['iou'], gold['eval/iou']) and s['iou'].dtype == np.float64
    assert s['mean_iou'] == float(gold['eval/mean_iou'])
    assert s['accuracy'] == float(gold['eval/accuracy'])
    assert np.array_equal(s['acc_per_frame'], gold['eval/acc_per_frame'])
    assert s['acc_per_frame'][2] == 0.0   # the frame without a valid pixel: 0 / (0 + 1e-10)
    one = st.summarize(gold['eval/counts'][:1], C)   # AverageMeter after one update: avg is the value itself
    assert one['accuracy'] == float(gold['eval/acc_per_frame'][0])
    bad = gold['eval/counts'].copy()
    bad[1, 3 * C + 2] = 3
    with pytest.raises(KeyError, match='frame 1'):
        st.summarize(bad, C)
    with pytest.raises(ValueError):
        st.summarize(bad[:, :-1], C)


def test_fixture_counts_follow_from_its_labels(gold):
    """An independent count of the stored rows: the masks of utils.py:101-129 written out per class."""
    C = int(gold['eval/num_class'])
    pred, gt, rows = gold['eval/pred'].astype(np.int64), gold['eval/labels_gt'].astype(np.int64), gold['eval/counts']
    assert rows.shape == (4, 3 * C + 3) and (gt >= C).any() and (gt[2] < 0).all()
    for f in range(4):
        valid = gt[f] >= 0
        want = [((pred[f] == c) & (gt[f] == c)).sum() for c in range(C)] + [((pred[f] == c) & valid).sum() for c in range(C)] + \
               [(gt[f] == c).sum() for c in range(C)] + [((pred[f] == gt[f]) & valid).sum(), valid.sum(), 0]
        assert rows[f].tolist() == [int(v) for v in want], f
    t = st.color_table(gold['eval/codes'], gold['eval/labels'])
    K = t.size // 2
    sc = gold['eval/scene'].astype(np.int64)
    packed = sc[..., 0] | (sc[..., 1] << 8) | (sc[..., 2] << 16)
    at = np.searchsorted(t[:K], packed)
    assert np.array_equal(t[:K][at], packed) and np.array_equal(t[K:][at] - 1, gt)
    assert int((gold['eval/labels_gt_unknown'] == -32768).sum()) == int(gold['eval/unknown_count']) == 3


@pytest.mark.parametrize('name', ['a', 'b', 'd', 'd0', 'e'])
def test_fixture_fusion_cases_are_self_consistent(gold, name):
    p = name + '/'
    S = int(gold[p + 'n_scales'])
    scores = [gold[p + 'scores%d' % s] for s in range(S)]
    H, W = gold[p + 'seg_size']
    pred32, pred64 = gold[p + 'pred32'], gold[p + 'pred64']
    assert pred32.dtype == np.float32 and pred64.dtype == np.float64 and pred32.shape == pred64.shape == scores[0].shape[:2] + (H, W)
    if name in u.CASES:
        seed, B, C, seg, sizes = u.CASES[name]
        assert tuple(seg) == (H, W) and all(np.array_equal(a, b) for a, b in zip(scores, u.draw_scores(seed, B, C, sizes)))
    ok = ~np.isnan(pred64)
    assert float(np.abs(pred32.astype(np.float64) - pred64)[ok].max()) == float(gold[p + 'e_ref'])
    # the float64 pipeline run again here (a later torch may differ in the last bits of a float64)
    again = u.pipeline(scores, (H, W), torch.float64).numpy()
    assert np.allclose(again[ok], pred64[ok], rtol=0, atol=1e-13) and np.array_equal(np.isnan(again), ~ok)
    lab = gold[p + 'labels_ref']
    if name in ('a', 'b'):
        arg, margin = u.margins(pred64)
        clear = (margin > 8 * float(gold[p + 'e_ref'])).numpy()
        assert 1.0 - clear.mean() <= 0.001 and np.array_equal(lab[clear], arg.numpy()[clear])
    elif name == 'd':
        assert (lab == 2).all() and np.array_equal(pred32[:, 2], pred32[:, 5])
    elif name == 'd0':
        assert (lab == 0).all()
    else:
        hit = gold['e/nan_pixels']
        assert np.array_equal(hit, np.isnan(pred32).any(axis=1)) and 0 < hit.sum() < hit.size and (lab[hit] == 0).all()


def test_fixture_case_c_is_redrawn_from_its_seed(gold):
    seed, B, C, seg, sizes = u.CASES['c']
    assert (B, C, len(sizes)) == (2, 32, 8) and any(h > seg[0] and w > seg[1] for h, w in sizes)
    scores = u.draw_scores(seed, B, C, sizes)
    assert u.digest(scores) == str(gold['c/scores_sha256'])
    pred64 = u.pipeline(scores, seg, torch.float64)
    pred32 = u.pipeline(scores, seg, torch.float32)
    assert np.allclose(pred64.numpy().reshape(-1)[::u.SAMPLE_STRIDE], gold['c/pred64_sample'], rtol=0, atol=1e-13)
    e_ref = float(gold['c/e_ref'])
    assert abs(float((pred32.double() - pred64).abs().max()) - e_ref) <= 0.25 * e_ref   # this torch's fp32 run, for orientation
    arg, margin = u.margins(pred64)
    clear = margin > 8 * e_ref
    assert 1.0 - float(clear.double().mean()) <= 0.001
    assert np.array_equal(gold['c/labels_ref'][clear.numpy()], arg.numpy()[clear.numpy()])
