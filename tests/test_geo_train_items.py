"""derender3d/train_items.py without a GPU: the host restatement of Pillow's colour ops (tests/geo_train_util.py, the statements
csrc/train_items.hip holds for the device) against the installed Pillow, and the module's host half against the fixture the
reference's own VKitti class produced (tests/golden/make_geo_train_golden.py)."""
import random

import numpy as np
import PIL.Image
import PIL.ImageStat
import pytest

import geo_train_util as u
from derender3d import train_items as ti


@pytest.fixture(scope='module')
def g():
    return u.golden()


def fixture_factors(g):
    return sorted({float(v) for v in g['t_factors'].reshape(-1)} | {0.0, 1.0})


def test_blend_equals_pillow_for_every_value_pair(g):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    ia, ib = PIL.Image.fromarray(a, 'L'), PIL.Image.fromarray(b, 'L')
    factors = fixture_factors(g)
    assert any(f > 1 for f in factors) and any(0 < f < 1 for f in factors)
    for f in factors:
        assert np.array_equal(np.asarray(PIL.Image.blend(ia, ib, f)), u.blend(a, b, f)), f


def test_luma_equals_pillow():
    v = np.arange(0, 256, 5, dtype=np.uint8)
    v = np.concatenate([v, np.uint8([1, 2, 127, 128, 254])])
    rgb = np.stack(np.meshgrid(v, v, v, indexing='ij'), axis=-1).reshape(v.size, -1, 3)
    assert np.array_equal(np.asarray(PIL.Image.fromarray(rgb, 'RGB').convert('L')), u.luma(rgb))


def all_colours():
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def test_hsv_conversions_equal_pillow_for_all_colours():
    cube = all_colours()
    ref = np.asarray(PIL.Image.fromarray(cube, 'RGB').convert('HSV'))
    for k in range(0, 4096, 512):
        assert np.array_equal(ref[k:k + 512], u.rgb_to_hsv(cube[k:k + 512])), 'RGB -> HSV, rows from %d' % k
    ref = np.asarray(PIL.Image.fromarray(cube, 'HSV').convert('RGB'))
    for k in range(0, 4096, 512):
        assert np.array_equal(ref[k:k + 512], u.hsv_to_rgb(cube[k:k + 512])), 'HSV -> RGB, rows from %d' % k


def test_draws_follow_the_reference_under_the_recorded_seeds(g):
    drawn = np.flatnonzero(g['t_drawn_roi'] & g['t_drawn_jitter'])
    assert drawn.size >= 4
    for b in drawn:
        random.seed(int(g['t_seeds'][b]))
        assert ti.roi_jitter(g['t_mask_rois'][b].tolist()) == g['t_rois_used'][b].tolist()
        order, factors, shift = ti.jitter_params()
        assert order == u.item_order(g, b) and list(factors) == g['t_factors'][b].tolist() and shift == int(g['t_hue_shift'][b])
    # an item whose colour parameters were prescribed still drew its roi first
    only_roi = np.flatnonzero(g['t_drawn_roi'] & ~g['t_drawn_jitter'])
    assert only_roi.size
    for b in only_roi:
        random.seed(int(g['t_seeds'][b]))
        assert ti.roi_jitter(g['t_mask_rois'][b].tolist()) == g['t_rois_used'][b].tolist()


def test_jitter_params_without_some_ops():
    order, factors, shift = ti.jitter_params(brightness=0, saturation=0, rng=random.Random(3))
    assert sorted(order) == [ti.CONTRAST, ti.HUE] and factors[0] == 1.0 and factors[2] == 1.0 and 0 <= shift <= 255
    assert ti.jitter_params(0, 0, 0, 0) == ([], (1.0, 1.0, 1.0), 0)


def ulps(a, b):
    """distance in float32 steps"""
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, np.int64(-2 ** 31) - i, i) for i in (ia, ib))
    return np.abs(ia - ib)


def check_targets(entries, g, tag, b):
    """exact where the entry is plain arithmetic, within one float32 step where it passes through log / cos / sin (the libm
    behind numpy may differ between machines)"""
    for k in u.TARGET_KEYS:
        want = g['%s_%s' % (tag, k)][b]
        have = np.asarray(entries[k])
        if k == 'targets':
            assert int(have) == int(want)
        elif k in u.LIBM_KEYS:
            assert have.dtype == np.float32 and ulps(have, want).max() <= 1, (k, b, have, want)
        else:
            assert have.dtype == np.float32 and np.array_equal(have, want), (k, b, have, want)


@pytest.mark.parametrize('tag', ['t', 'e'])
def test_vkitti_targets_equal_the_fixture(g, tag):
    _, _, items, _, rois = u.batch_items(g, tag)
    for b, it in enumerate(items):
        entries, nearer = ti.vkitti_targets(it.row(), it.rows, rois[b])
        check_targets(entries, g, tag, b)
        # the recorded libm values reproduce the fixture's entries exactly: cos, sin, log(scale) x 3, log(depth), log(droi) x 2
        m = g[tag + '_libm'][b]
        assert np.array_equal(np.float32([m[0], 0, -m[1], 0]), g[tag + '_rotations'][b])
        assert np.array_equal(np.float32(m[2:5]), g[tag + '_log_scales'][b])
        assert np.array_equal(np.float32([m[5] + m[6] + m[7]]), g[tag + '_log_depths'][b])
        depths = np.sum(np.stack([it.rows['x3d'], -(it.rows['y3d'] - it.rows['h3d'] / 2), -it.rows['z3d']], axis=1) ** 2, axis=1)
        assert nearer.tolist() == np.flatnonzero(depths < depths[it.index]).tolist() and it.index not in nearer


def test_contrast_mean_in_integers_equals_imagestat(g):
    from derender3d import scene as sc
    frames, scenes, items, jitter, rois = u.batch_items(g, 't')
    seen = 0
    for b, it in enumerate(items):
        order, factors, shift = jitter[b]
        if u.CONTRAST not in order:
            continue
        win = sc.crop_windows([rois[b]], scenes.shape[1], scenes.shape[2])[0]
        crop = u.window(np.ascontiguousarray(frames[it.frame].transpose(1, 2, 0)), win, 127)
        crop = u.color_jitter(crop, order[:order.index(u.CONTRAST)], factors, shift)
        grey = PIL.Image.fromarray(crop, 'RGB').convert('L')
        lum = np.asarray(grey).astype(np.int64)
        assert u.contrast_grey(lum.sum(), lum.size) == int(PIL.ImageStat.Stat(grey).mean[0] + 0.5)
        seen += 1
    assert seen >= 24


@pytest.mark.parametrize('tag', ['t', 'e'])
def test_host_restatement_reproduces_the_fixture_crops(g, tag):
    """window + restated colour ops + Pillow's tables = the reference's item, bit for bit: what the device is held to"""
    frames, scenes, items, jitter, rois = u.batch_items(g, tag)
    for b, it in enumerate(items):
        _, nearer = ti.vkitti_targets(it.row(), it.rows, rois[b])
        order, factors, shift = jitter[b]
        image, mask, ignore = u.host_item(np.ascontiguousarray(frames[it.frame].transpose(1, 2, 0)), scenes[it.frame], it.code,
                                          it.codes[nearer], rois[b], order, factors, shift, ti.VKITTI_MEAN, ti.VKITTI_STD)
        assert np.array_equal(image, g[tag + '_images'][b]), b
        assert np.array_equal(mask, g[tag + '_masks'][b]), b
        assert np.array_equal(ignore, g[tag + '_ignores'][b]), b


def test_item_table_refuses_bad_parameters():
    with pytest.raises(ValueError):
        ti.item_table([0], [(1, 2, 3)], [0], [0], [([0, 0], (1, 1, 1), 0)])
    with pytest.raises(ValueError):
        ti.item_table([0], [(1, 2, 3)], [0], [0], [([4], (1, 1, 1), 0)])
    with pytest.raises(ValueError):
        ti.item_table([0], [(1, 2, 3)], [0], [0], [([3], (1, 1, 1), 256)])
    tab = ti.item_table([2], [(1, 2, 3)], [5], [2], [([3, 1], (0.5, 1.5, 1.0), 7)])
    assert tab.shape == (1, ti.ITEM_INTS) and tab[0, :6].tolist() == [2, 1 | 2 << 8 | 3 << 16, 5, 2, 2, 3 | 1 << 4] and tab[0, 9] == 7
    assert tab.view(np.float32)[0, 6:9].tolist() == [0.5, 1.5, 1.0]


def test_cpu_tensors_raise():
    import torch
    with pytest.raises(NotImplementedError):
        ti.train_batch(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), [], False)
