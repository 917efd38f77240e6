"""CPU: the constructed inputs of tests/id_select_util.py are what they claim to be, and the three host references of the
order-statistic selects vouch for each other on them.

  * the census conditions: `crowd` overflows the LDS slot table of k_ids_pass_a / k_ids_pass_b in every chunk, `ranks` holds
    exactly the n listed, `bins` holds every kind of object the census tells apart; every case meets its docstring;
  * id_select_util.plain_stats (a sort) equals cityscapes_util.stats_emulated (the kernels' histograms) on every case and on
    the fixture's cases, and geo_hybrid_util.order_statistics column for column;
  * derender3d.scene.percentile95_threshold of plain_stats' (n, lo, hi) equals floor(np.percentile(., 95))."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cityscapes_util as cu  # noqa: E402
import geo_hybrid_util as gh  # noqa: E402
import id_select_util as iu  # noqa: E402


@pytest.fixture(scope='module')
def cases():
    return iu.cases()


@pytest.fixture(scope='module')
def plain(cases):
    return {name: iu.plain_stats(*c) for name, c in cases.items()}


def test_the_case_names_and_types(cases):
    assert tuple(cases) == iu.CASE_NAMES
    for name, (scene, disparity, category) in cases.items():
        assert scene.dtype == disparity.dtype == np.int32 and scene.shape == disparity.shape and scene.ndim == 2, name
        assert scene.size < 10 ** 4 and 0 <= category <= iu.MAX_CATEGORY, name
        assert disparity.min() >= 0 and disparity.max() <= 65535, name            # the launchers' precondition
    again = iu.cases()
    assert all(np.array_equal(a, b) for name in cases for a, b in zip(cases[name][:2], again[name][:2]))      # seeded


def test_crowd_overflows_the_slot_table_in_every_chunk(cases, plain):
    scene, disparity, category = cases['crowd']
    c = iu.census(scene, disparity, category)
    assert scene.shape == (24, 96) and scene.size > iu.ID_CHUNK                   # two chunks
    assert c['fewest_per_chunk'] > iu.ID_SLOTS and c['fewest_per_chunk'] >= 17    # the slot == -1 branches, both passes
    assert c['straddling'] >= 17                                                  # both low-byte histograms, also without a slot
    # what the docstring claims
    assert c['objects'] == 40 and c['fewest_per_chunk'] == c['most_per_chunk'] == 40 and c['fewest_per_run'] >= 37
    assert c['straddling'] >= 35 and plain['crowd'][999, 0] > 0 and plain['crowd'][39, 0] == 0
    zeros = float((disparity == 0).mean())
    assert 0.15 < zeros < 0.25 and (disparity == 65535).sum() >= 1 and (disparity == 65534).sum() >= 1
    # ties among the areas: cityscapes_gt_inputs keeps 16 of 40
    assert len(set(plain['crowd'][:, 0].tolist()) - {0}) < 40


def test_ranks_holds_exactly_the_listed_n(cases, plain):
    scene, disparity, category = cases['ranks']
    c = iu.census(scene, disparity, category)
    assert c['ns'] == set(iu.RANK_NS) and c['objects'] == len(iu.RANK_NS) and scene.shape[1] % 2 == 1
    assert {1, 2, 19, 20, 21, 22, 40, 41, 42} <= c['ns']             # i = 19 (n - 1) / 20 steps at 21 -> 22 and 41 -> 42
    for k, n in enumerate(iu.RANK_NS):
        row = plain['ranks'][7 * k]
        d = disparity[scene == 26000 + 7 * k]
        d = d[d != 0]
        assert row[5] == n and row[0] == n + 1 + k % 4 and len(set(d.tolist())) == n       # pairwise distinct, area != n
        if n > 1:
            assert row[6] < row[7]
        if k % 2:
            assert d.max() - d.min() < 768


def test_bins_holds_every_kind(cases, plain):
    scene, disparity, category = cases['bins']
    c = iu.census(scene, disparity, category)
    for kind in ('n0', 'n1', 'tied', 'same_bin', 'straddling'):
        assert c[kind] >= 1, kind
    assert c['objects'] == len(iu.BINS)
    for obj_id, (what, lo, hi) in iu.BINS.items():
        assert plain['bins'][obj_id - 26000, 6:].tolist() == [lo, hi], what
    t = plain['bins']
    assert t[100:103, 5].tolist() == [5, 7, 30] and t[103, 5] == 40 and t[104, 5] == 21 and t[105, 5] == 41 and t[106, 5] == 20
    assert t[107, 0] == 300 and t[107, 5] == 1 and t[108, 0] == 50 and t[108, 5] == 0
    d = np.sort(disparity[scene == 26103])
    assert (d == 0x5A5A).sum() == 5 and d[-1] == 0x5A5A
    thr = iu.plain_thresholds(scene, disparity, category)
    assert thr[108] == 0 and thr[107] == 4660 and thr[102] == 65535 and thr[106] == 255 + int(np.floor(65280 * 0.05))


def test_edges_of_the_category_counts_only_its_range(cases, plain):
    scene = cases['edges_of_the_category'][0]
    assert set(iu.EDGE_IDS) <= set(np.unique(scene).tolist())
    area = {v: int((scene == v).sum()) for v in iu.EDGE_IDS + (iu.BACKGROUND,)}
    for name, category, inside in (('edges_of_the_category', 26, {26000: 0, 26999: 999}),
                                   ('edges_of_the_category@0', 0, {0: 0, 26: 26, iu.BACKGROUND: 7}),
                                   ('edges_of_the_category@max', iu.MAX_CATEGORY,
                                    {1000 * iu.MAX_CATEGORY: 0, 1000 * iu.MAX_CATEGORY + 999: 999})):
        assert cases[name][2] == category and np.array_equal(cases[name][0], scene)
        t = plain[name]
        assert np.flatnonzero(t[:, 0]).tolist() == sorted(inside.values())
        for v, j in inside.items():
            assert t[j, 0] == area[v]
    assert iu.MAX_CATEGORY == 2147482 and 1000 * iu.MAX_CATEGORY + 999 < iu.INT_MAX


@pytest.mark.parametrize('H,W', iu.SHAPES)
def test_shapes_place_the_objects_on_the_borders(cases, plain, H, W):
    name = 'shapes@%dx%d' % (H, W)
    scene, disparity, category = cases[name]
    t = plain[name]
    assert scene.shape == (H, W)
    assert t[999].tolist() == [1, H - 1, W - 1, H, W, 1, 40000, 40000]              # one pixel, the last
    corners = {(y, x) for y in (0, H - 1) for x in (0, W - 1)} - {(H - 1, W - 1)}
    assert all(scene[y, x] == 26500 for y, x in corners) and t[500, 0] == len(corners)
    assert t[500, 1:3].tolist() == [0, 0]
    if min(H, W) > 1:
        assert t[500, 1:5].tolist() == [0, 0, H, W]
    assert iu.SHAPES[:5] == ((1, 2047), (1, 2048), (1, 2049), (2049, 1), (3, 1))


def test_plain_stats_equals_the_emulation_and_the_order_statistics(cases, plain):
    g = cu.load()
    inputs = dict(cases)
    for tag in cu.CASES:
        inputs['fixture ' + tag] = cu.maps(g, tag) + (26,)
    for name, (scene, disparity, category) in inputs.items():
        want = plain[name] if name in plain else iu.plain_stats(scene, disparity, category)
        got = cu.stats_emulated(scene, disparity, category)
        assert np.array_equal(got, want), '%s: rows %s' % (name, np.flatnonzero((got != want).any(axis=1)))
        for j in np.flatnonzero(want[:, 0]).tolist():
            values = disparity[scene.astype(np.int64) == 1000 * category + j]
            assert tuple(want[j, 5:].tolist()) == gh.order_statistics(values), (name, j)
    for tag in cu.CASES:
        j = g[tag + '_ids'] - 26000
        assert np.array_equal(iu.plain_stats(*cu.maps(g, tag))[j], g[tag + '_stats'])


def test_the_threshold_formula_equals_np_percentile(cases, plain):
    from derender3d import scene as sc
    for name, (scene, disparity, category) in cases.items():
        t = plain[name]
        got = sc.percentile95_threshold(t[:, 5], t[:, 6], t[:, 7])
        want = iu.plain_thresholds(scene, disparity, category)
        assert got.dtype == np.int32 and np.array_equal(got, want), '%s: objects %s' % (name, np.flatnonzero(got != want))


def test_the_item_lists_cover_what_they_claim():
    items = iu.item_cases()
    maps, records = items['single']
    assert len(records) == 1 and len(maps) == 1
    maps, records = items['mixed']
    sizes = [s.size for s, _ in maps]
    assert 1 in sizes and max(sizes) == 72 * 96 and max(sizes) > 3 * iu.ID_CHUNK       # a 1 x 1 frame beside the largest
    assert all(s.dtype == d.dtype == np.int32 and s.shape == d.shape for s, d in maps)
    assert any(not has for _, _, has in records)                                        # an item without a disparity map
    assert any(not (maps[f][0] == v).any() for f, v, _ in records)                      # an absent id
    assert len(set(records)) < len(records)                                             # the same item twice
    assert {f for f, _, _ in records} == set(range(len(maps)))
    for f, v, has in records[:50]:
        row = iu.plain_item_row(maps[f][0], maps[f][1] if has else None, v)
        if 26000 <= v < 27000 and has:
            assert np.array_equal(row, iu.plain_stats(*maps[f])[v - 26000])
