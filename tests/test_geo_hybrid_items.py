"""derender3d/train_items.py's hybrid half without a GPU, against the fixture the reference's own dataset classes and
collate_fn produced (tests/golden/make_geo_hybrid_golden.py)."""
import os
import re

import numpy as np
import pytest

import geo_hybrid_util as h
import geo_train_util as u
from derender3d import scene as sc
from derender3d import train_items as ti
from test_geo_train_items import ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def g():
    return h.golden()


def collated(g, tag):
    """the module's host half on batch `tag` with the fixture's rois: item_entries per item, then collate_entries"""
    keys, items, _, rois, _ = h.host_items(g, tag)
    sizes = [h.frame_arrays(g, keys[it.frame])['rgb'].shape[:2] for it in items]
    entries = [ti.item_entries(it, rois[b], sizes[b][0], sizes[b][1]) for b, it in enumerate(items)]
    for b, it in enumerate(items):
        if isinstance(it, ti.KittiObjectItem):
            assert [int(v) for v in it.row[:4]] == rois[b].tolist()
        mine = set(entries[b]) | {'targets', 'images'} | ({'masks', 'ignores'} if ti.has_maps(it) else set())
        assert mine == set(str(k) for k in g['%s_item%d_keys' % (tag, b)]), (tag, b)      # the keys of the reference's own item
    return ti.collate_entries(items, entries)


@pytest.mark.parametrize('tag', ['vk', 'ko', 'ks', 'cs', 'ce', 'mr', 'mt', 'vc', 'kk'])
def test_host_entries_and_their_collation_equal_the_collated_dict(g, tag):
    """every key of the reference's collated dict but the three crops: the key union, the values, collate's zero rows and the
    int64 targets.  Exact, except one float32 step where a value passes through log / cos / sin"""
    assert tag in h.batch_tags(g)
    host, maps = collated(g, tag)
    want_keys = set(str(k) for k in g[tag + '_keys'])
    assert set(host) | {'images'} | ({'masks', 'ignores'} if maps else set()) == want_keys
    assert host['targets'].dtype == np.int64 and np.array_equal(host['targets'], g[tag + '_targets'])
    for k, have in host.items():
        want = g['%s_%s' % (tag, k)]
        assert have.dtype == want.dtype and have.shape == want.shape, (tag, k)
        if k in u.LIBM_KEYS:
            assert ulps(have, want).max() <= 1, (tag, k, have, want)
        else:
            assert np.array_equal(have, want), (tag, k, have, want)


def test_the_fixture_holds_every_kind_and_the_zero_fill_cases(g):
    kinds = set()
    for tag in h.batch_tags(g):
        kinds |= set(g[tag + '_kind'].tolist())
    assert kinds == {h.VK, h.KO, h.KS, h.CS, h.MR}
    assert g['kk_kind'][0] == h.KO and not g['kk_masks'][0].any() and g['kk_masks'][1].any()       # the shape comes from a later item
    assert g['vc_kind'].tolist().count(h.CS) == 1 and not g['vc_rotations'][g['vc_kind'] == h.CS].any()
    assert 'masks' not in set(g['ko_keys']) and 'rois' not in set(g['ks_keys'])


def test_recorded_libm_values_reproduce_the_kitti_object_entries(g):
    m, kind = g['ko_libm'], g['ko_kind']
    for b in np.flatnonzero(kind == h.KO):
        assert np.array_equal(np.float32(m[b, 2:5]), g['ko_log_scales'][b])
        assert np.array_equal(np.float32([m[b, 5] + m[b, 6] + m[b, 7]]), g['ko_log_depths'][b])


@pytest.mark.parametrize('tag', ['vk', 'ko', 'ks', 'cs', 'ce', 'mr', 'mt', 'vc', 'kk'])
def test_host_emulation_reproduces_the_fixture_crops(g, tag):
    assert tag in h.batch_tags(g)
    keys, items, jitter, rois, is_train = h.host_items(g, tag)
    for b, it in enumerate(items):
        image, mask, ignore = h.host_mixed_item(g, tag, b, it, h.frame_arrays(g, keys[it.frame]), rois[b], jitter[b])
        assert np.array_equal(image, g[tag + '_images'][b]), (tag, b)
        if tag + '_masks' in g:
            zeros = np.zeros((1, 256, 256), np.float32)
            assert np.array_equal(zeros if mask is None else mask, g[tag + '_masks'][b]), (tag, b)
            assert np.array_equal(zeros if ignore is None else ignore, g[tag + '_ignores'][b]), (tag, b)
        else:
            assert mask is None


def test_percentile_threshold_of_the_order_statistics_equals_numpy(g):
    seen = set()
    for key in ('cs000019', 'cs000020'):
        f = h.frame_arrays(g, key)
        for obj in np.unique(f['ids']):
            v = f['disp'][f['ids'] == obj]
            n, lo, hi = h.order_statistics(v)
            want = int(np.floor(np.percentile(v[v != 0], 95))) if n else 0
            assert int(sc.percentile95_threshold([n], [lo], [hi])[0]) == want, (key, obj)
            seen.add('zero' if n == 0 else 'one' if n == 1 else 'tie' if lo == hi else 'bytes' if lo >> 8 != hi >> 8 else 'plain')
    assert seen >= {'zero', 'one', 'tie', 'bytes', 'plain'}


def test_draws_follow_the_reference_under_the_recorded_seeds(g):
    import random
    seen = 0
    for tag in h.batch_tags(g):
        p = tag + '_'
        for b in np.flatnonzero(g[p + 'drawn_roi'] | g[p + 'drawn_jitter']):
            random.seed(int(g[p + 'seeds'][b]))
            if g[p + 'kind'][b] != h.KO and g[p + 'drawn_roi'][b]:
                assert ti.roi_jitter(g[p + 'mask_rois'][b].tolist()) == g[p + 'rois_used'][b].tolist(), (tag, b)
            elif g[p + 'kind'][b] != h.KO:
                continue        # a prescribed roi: the reference's draw for it was not made, the stream differs
            if g[p + 'drawn_jitter'][b]:
                order, factors, shift = ti.jitter_params()
                assert order == u.item_order(g, b, tag) and list(factors) == g[p + 'factors'][b].tolist() and shift == int(g[p + 'hue_shift'][b])
                seen += 1
    assert seen >= 6


def test_hybrid_weights_equal_the_reference_expression():
    lengths, weights = [7, 3], [0.75, 0.25]
    want = np.concatenate([w * np.ones(n) / n for n, w in zip(lengths, weights)], axis=0)
    assert np.array_equal(ti.hybrid_weights(lengths, weights), want)
    assert np.array_equal(ti.hybrid_weights([2, 5]), np.concatenate([np.ones(2) / 2, np.ones(5) / 5]))


def test_abi_numbers_agree_and_the_header_declares_the_new_symbols():
    import sdn_hip
    header = open(os.path.join(ROOT, 'include', 'sdn_hip.h')).read()
    version = int(re.search(r'#define\s+SDN_ABI_VERSION\s+(\d+)', header).group(1))
    assert version == sdn_hip.ABI_VERSION == sdn_hip.lib().sdn_version() >= 17
    for name in ('sdn_train_id_stats_workspace_bytes', 'sdn_train_id_stats', 'sdn_train_crops_mixed'):
        assert re.search(r'\bint\s+%s\(' % name, header), name
        assert name in sdn_hip.exported_symbols() and hasattr(sdn_hip.lib(), name)
    makefile = open(os.path.join(ROOT, '3d-sdn_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'EXACT_SRC\s*:=.*\btrain_hybrid\.hip\b', makefile)


def test_cpu_tensors_raise():
    import torch
    with pytest.raises(NotImplementedError):
        ti.SourceFrame(torch.zeros(3, 8, 8, dtype=torch.uint8))
