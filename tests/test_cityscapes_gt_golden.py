"""CPU: the host half of the Cityscapes ground-truth source (derender3d.scene.percentile95_threshold, the selection) and the
numpy emulation of sdn_scene_id_stats / sdn_scene_id_planes (tests/cityscapes_util.py) against
tests/golden/cityscapes_gt_golden.npz (the reference's statements, executed: tests/golden/make_cityscapes_gt_golden.py).
Exact comparisons throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cityscapes_util as cu  # noqa: E402
from derender3d import scene as sc  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return cu.load()


def test_fixture_is_small_and_holds_the_cases(gold):
    g = gold
    assert os.path.getsize(cu.GOLDEN) < 400000
    assert g['a_scene'].shape == g['b_scene'].shape == (37, 70) and g['c_scene'].shape == (64, 128)
    assert [len(g[t + '_ids']) for t in cu.CASES] == [1, 3, 33] and len(g['c_sels']) == 16
    for t in cu.CASES:
        assert g[t + '_scene'].dtype == g[t + '_disparity'].dtype == np.uint16
        assert {0, 26, 24001, 25999, 27000, 27999} <= set(np.unique(g[t + '_scene']).tolist())
    assert g['b_ids'].tolist() == [26000, 26500, 26999] and g['a_rois'].tolist() == [[0, 0, 37, 70]]
    s = g['c_stats']
    assert sorted(set(s[:8, 5].tolist())) == [0, 1, 2, 11, 21, 22, 41, 54] and g['c_areas'][8] == g['c_areas'][9]
    assert g['b_stats'][:, 6:].tolist() == [[255, 256], [65535, 65535], [0x1FF, 0x200]]


@pytest.mark.parametrize('tag', cu.CASES)
def test_emulation_equals_the_fixture_bit_for_bit(gold, tag):
    g = gold
    scene, disparity = cu.maps(g, tag)
    table = cu.stats_emulated(scene, disparity)
    j = g[tag + '_ids'] - 26000
    assert np.array_equal(table[j], g[tag + '_stats']), np.flatnonzero((table[j] != g[tag + '_stats']).any(axis=1))
    absent = np.setdiff1d(np.arange(1000), j)
    assert (table[absent, 0] == 0).all() and (table[absent, 1:3] == cu.INT_MAX).all() and (table[absent, 3:] == 0).all()
    # the host step: thresholds from (n, lo, hi), all objects, then the selection
    thr = sc.percentile95_threshold(table[j, 5], table[j, 6], table[j, 7])
    assert thr.dtype == np.int32 and np.array_equal(thr, np.floor(g[tag + '_percentiles']).astype(np.int32))
    masks, ignores, cover = cu.planes_emulated(scene, disparity, g[tag + '_ids'], thr)
    assert np.array_equal(masks, cu.planes(g, tag, 'masks')) and np.array_equal(ignores, cu.planes(g, tag, 'ignores'))
    sels, ids, rois, areas, sel_thr = cu.select_emulated(table)
    assert np.array_equal(sels, g[tag + '_sels']) and np.array_equal(ids, g[tag + '_ids'][sels])
    assert np.array_equal(rois, g[tag + '_rois'][sels]) and np.array_equal(areas, g[tag + '_areas'][sels])
    assert np.array_equal(sel_thr, thr[sels])
    for k in range(len(j)):
        assert np.array_equal((cover[k // 32] >> np.uint32(k & 31)) & 1, ignores[k, 0])


def test_the_emulation_ignores_other_categories_and_the_bare_category():
    scene = np.asarray([[26, 25999, 27000, 26000], [26999, 24001, 0, 26999]], np.int32)
    disparity = np.asarray([[5, 6, 7, 8], [9, 10, 11, 0]], np.int32)
    table = cu.stats_emulated(scene, disparity)
    assert np.flatnonzero(table[:, 0]).tolist() == [0, 999]
    assert table[0].tolist() == [1, 0, 3, 1, 4, 1, 8, 8] and table[999].tolist() == [2, 1, 0, 2, 4, 1, 9, 9]


def _values(rng, kind, n):
    if kind == 'narrow':   # a step of 20 between the two ranks: lo + 20 frac((n - 1) 0.95) is an integer in exact arithmetic
        i = cu.integer_rank(n)
        return rng.permutation(np.asarray([1000] * (i + 1) + [1020] * (n - i - 1)))
    if kind == 'constant':
        return np.full(n, 4242)
    return rng.integers(1, 65536, n)


@pytest.mark.parametrize('dtype', [np.uint16, np.int32])
@pytest.mark.parametrize('kind', ['narrow', 'constant', 'full'])
def test_threshold_equals_floor_of_numpy_percentile(kind, dtype):
    """every n in 1 .. 600: (n, lo, hi) -> floor(np.percentile(values, 95)), np.percentile executed here"""
    rng = np.random.default_rng(5)
    ns, los, his, want, integral = [], [], [], [], 0
    for n in range(1, 601):
        a = _values(rng, kind, n).astype(dtype)
        s = np.sort(a.astype(np.int64))
        i = cu.integer_rank(n)
        ns.append(n)
        los.append(s[i])
        his.append(s[min(i + 1, n - 1)])
        p = np.percentile(a, 95)
        want.append(int(np.floor(p)))
        integral += int(p == np.floor(p) and los[-1] != his[-1])
    got = sc.percentile95_threshold(np.asarray(ns), np.asarray(los), np.asarray(his))
    assert got.dtype == np.int32 and got.tolist() == want
    if kind == 'narrow':
        assert integral > 0     # lo != hi with an integral percentile: where one ulp would flip pixels
    assert sc.percentile95_threshold([0, 0], [0, 7], [0, 9]).tolist() == [0, 0]            # nothing left: main.py:778


def test_integer_rank_equals_the_float64_floor():
    n = np.arange(1, 2 ** 22 + 1, dtype=np.int64)
    assert np.array_equal((19 * (n - 1)) // 20, np.floor((n - 1) * np.true_divide(95, 100)).astype(np.int64))
    assert np.array_equal((19 * (n - 1)) // 20, np.floor((n - 1) * 0.95).astype(np.int64))


def test_camera_is_the_reference_s():
    assert (sc.CityscapesCamera.focal, sc.CityscapesCamera.u0, sc.CityscapesCamera.v0) == (2250.0, 925.0, 460.0)


def test_argument_checks_run_before_the_first_launch(gold):
    g = gold
    from derender3d import scene2d
    from sdn_hip import ops
    scene, disparity = (torch.from_numpy(a) for a in cu.maps(g, 'b'))
    image = torch.zeros(3, 37, 70, dtype=torch.uint8)
    planes = torch.zeros(3, 1, 37, 70)
    words = torch.zeros(1, 37, 70, dtype=torch.int32)
    with pytest.raises(ValueError, match='one of them'):
        sc.SceneSession(None, sc.CityscapesCamera, image, [1, 1, 1], planes, g['b_rois'], image_ignores=planes, ignore_cover=words)
    with pytest.raises(ValueError, match='one of them'):
        sc.ignore_crops(None, None, image_ignores=planes, ignore_cover=words)
    # CPU tensors: no fallback
    ids = torch.from_numpy(g['b_ids'])
    for call in (lambda: ops.scene_id_stats(scene, disparity), lambda: ops.scene_id_planes(scene, disparity, ids, ids),
                 lambda: sc.cityscapes_gt_inputs(scene, disparity),
                 lambda: sc.SceneSession.from_cityscapes_gt(None, sc.CityscapesCamera, image, scene, disparity),
                 lambda: scene2d.Scene2D.from_cityscapes_gt(None, scene, disparity)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(TypeError):
        sc.cityscapes_gt_inputs(cu.maps(g, 'b')[0], disparity)


def test_the_launchers_refuse_bad_arguments_without_a_gpu():
    """error paths return codes and set the message; no kernel is launched (fake non-null pointers)"""
    import sdn_hip
    L = sdn_hip.lib()
    fake, n = ctypes.c_void_p(4096), ctypes.c_size_t(0)
    assert L.sdn_scene_id_workspace_bytes(ctypes.byref(n)) == 0 and n.value == 4 * (1000 * 256 + 1000 * 4 + 1000 * 2 * 256)
    assert L.sdn_scene_id_workspace_bytes(None) == -1
    assert L.sdn_scene_id_stats(None, fake, 26, 4, 4, fake, fake, None) == -1 and b'null pointer' in L.sdn_last_error()
    assert L.sdn_scene_id_stats(fake, fake, 26, 0, 4, fake, fake, None) == -1 and b'bad sizes' in L.sdn_last_error()
    assert L.sdn_scene_id_stats(fake, fake, -1, 4, 4, fake, fake, None) == -1 and b'category' in L.sdn_last_error()
    assert L.sdn_scene_id_stats(fake, fake, 26, 4, 4, fake, ctypes.c_void_p(4100), None) == -1 and b'aligned' in L.sdn_last_error()
    assert L.sdn_scene_id_planes(fake, None, fake, fake, 1, 4, 4, fake, fake, None, None) == -1 and b'null pointer' in L.sdn_last_error()
    assert L.sdn_scene_id_planes(fake, fake, fake, fake, 0, 4, 4, fake, fake, None, None) == -1 and b'bad sizes' in L.sdn_last_error()
    assert L.sdn_scene_id_planes(fake, fake, fake, fake, 1, 4, 4, None, None, fake, None) == -1 and b'neither' in L.sdn_last_error()
    assert L.sdn_scene_id_planes(fake, fake, fake, fake, 1, 4, 4, ctypes.c_void_p(4098), None, None, None) == -1
