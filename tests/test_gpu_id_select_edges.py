"""GPU: every path of the order-statistic selects -- sdn_scene_id_stats / sdn_scene_id_planes (csrc/scene_ids.hip),
sdn_train_id_stats (csrc/train_hybrid.hip), ids_find (csrc/rank_select.h) -- on the constructed inputs of
tests/id_select_util.py against its plain reference, a sort.  The kernels are integer arithmetic: every comparison is
np.array_equal, there is no tolerance anywhere.

  * ops.scene_id_stats on every case: the whole table, absent rows included; the same bytes on a second call (five on `crowd`,
    where which objects find an LDS slot depends on scheduling); the thresholds of the device table against np.percentile;
  * ops.scene_id_planes at n = 32, 64 and 65, with absent, foreign and duplicate ids and thr = -1, 0, 65534, 65535; on maps
    of 1, 2, 3 and 5 pixels into dirty buffers at every offset inside a 16-byte quad;
  * ops.train_id_stats on the same maps as items, with one workgroup per chunk and with one workgroup per item;
  * derender3d.scene.cityscapes_gt_inputs on `crowd`.
Every input meets the launchers' preconditions; nothing here provokes a device fault."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'),
           os.path.join(ROOT, '3d-sdn_amd', 'textural'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cityscapes_util as cu  # noqa: E402
import id_select_util as iu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    return iu.cases()


@pytest.fixture(scope='module')
def plain(cases):
    """the reference tables, computed once and shared (read-only)"""
    out = {name: iu.plain_stats(*c) for name, c in cases.items()}
    for t in out.values():
        t.setflags(write=False)
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(got, want):
    return 'rows %s differ' % np.flatnonzero((got != want).any(axis=1)).tolist()


@pytest.mark.parametrize('name', iu.CASE_NAMES)
def test_scene_id_stats_equals_the_sort(cases, plain, name):
    from derender3d import scene as sc
    from sdn_hip import ops
    scene, disparity, category = cases[name]
    scene_d, disparity_d = _dev(scene), _dev(disparity)
    table = ops.scene_id_stats(scene_d, disparity_d, category)
    assert table.dtype == torch.int32 and tuple(table.shape) == (1000, 8)
    got = table.cpu().numpy()
    assert np.array_equal(got, plain[name]), _rows(got, plain[name])            # the absent ids too
    for _ in range(4 if name == 'crowd' else 1):
        again = ops.scene_id_stats(scene_d, disparity_d, category).cpu().numpy()
        assert again.tobytes() == got.tobytes(), _rows(again, got)
    thr = sc.percentile95_threshold(got[:, 5], got[:, 6], got[:, 7])
    want = iu.plain_thresholds(scene, disparity, category)
    assert np.array_equal(thr, want), 'objects %s' % np.flatnonzero(thr != want).tolist()


def _id_lists(cases, plain):
    """(case, ids, thr) of the plane tests: n = 32, 64, 65 from `crowd`, its 40 ids repeated, with an absent id and one of
    another category in the list; every id of the edges map, one twice, an absent one and the background"""
    crowd_ids = (np.flatnonzero(plain['crowd'][:, 0]) + 26000).tolist()
    crowd_thr = iu.plain_thresholds(*cases['crowd'])
    out = []
    for n in (32, 64, 65):
        ids = [crowd_ids[k % 40] for k in range(n)]
        ids[1], ids[2], ids[n - 1] = 26500, 24003, crowd_ids[0]
        thr = [(-1, 0, 65534, 65535)[k % 4] if k < 8 or k == n - 1 else int(crowd_thr[ids[k] - 26000]) for k in range(n)]
        out.append(('crowd', ids, thr))
    ids = list(iu.EDGE_IDS) + [26000, 12345, iu.BACKGROUND]
    out.append(('edges_of_the_category', ids, [(-1, 0, 65534, 65535, 30000)[k % 5] for k in range(len(ids))]))
    return out


@pytest.mark.parametrize('which', range(4))
def test_scene_id_planes_at_the_word_edges(cases, plain, which):
    from sdn_hip import ops
    name, ids, thr = _id_lists(cases, plain)[which]
    scene, disparity, _ = cases[name]
    n = len(ids)
    assert n == (32, 64, 65, 14)[which] and len(set(ids)) < n
    ids, thr = np.asarray(ids, np.int32), np.asarray(thr, np.int32)
    masks, cover, ignores = ops.scene_id_planes(_dev(scene), _dev(disparity), _dev(ids), _dev(thr), ignore_planes=True)
    want_m, want_i, want_c = cu.planes_emulated(scene, disparity, ids.tolist(), thr.tolist())
    assert tuple(masks.shape) == tuple(ignores.shape) == (n, 1) + scene.shape and masks.dtype == ignores.dtype == torch.float32
    assert cover.dtype == torch.int32 and tuple(cover.shape) == ((n + 31) // 32,) + scene.shape
    got_m, got_i = masks.cpu().numpy(), ignores.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got_m[k], want_m[k].astype(np.float32)), 'mask %d (id %d)' % (k, ids[k])
        assert np.array_equal(got_i[k], want_i[k].astype(np.float32)), 'ignore %d (thr %d)' % (k, thr[k])
    assert np.array_equal(cover.cpu().numpy().view(np.uint32), want_c)
    # what the emulation must say at the ends of the threshold's range
    for k in np.flatnonzero(thr == -1).tolist():
        assert got_i[k].all()                                        # every pixel, the zeros too
    for k in np.flatnonzero(thr == 65535).tolist():
        assert not got_i[k].any()
    for k in np.flatnonzero(thr == 65534).tolist():
        assert np.array_equal(got_i[k, 0] != 0, disparity == 65535)
    for k in np.flatnonzero(~np.isin(ids, scene)).tolist():
        assert not got_m[k].any()                                    # an absent id: a zero plane
    assert (~np.isin(ids, scene)).any()


@pytest.mark.parametrize('shape', [(1, 1), (1, 2), (3, 1), (1, 5)])
def test_scene_id_planes_on_maps_smaller_than_a_quad(shape):
    """n = 5 output rows of 1, 2, 3 or 5 words each: one 16-byte quad spans up to four rows.  The outputs start 0, 4, 8 and 12
    bytes into the quads of buffers that held 7: every element written, the guard words before and after untouched."""
    from sdn_hip import check, lib, ptr, stream
    H, W = shape
    HW, n = H * W, 5
    rng = np.random.default_rng(17 + HW)
    scene = rng.choice(np.array([26000, 26001, 24003, iu.BACKGROUND], np.int32), (H, W))
    disparity = rng.integers(0, 4, (H, W)).astype(np.int32) * 300
    ids = np.array([26000, 26001, 26001, 24003, 26500], np.int32)
    thr = np.array([-1, 0, 300, 600, 65535], np.int32)
    want_m, want_i, want_c = cu.planes_emulated(scene, disparity, ids.tolist(), thr.tolist())
    scene_d, disparity_d, ids_d, thr_d = _dev(scene), _dev(disparity), _dev(ids), _dev(thr)
    for off in range(4):
        for others in range(4):      # the other two outputs at another offset each
            offs = (off, (off + others) % 4, (off + 2 * others + 1) % 4)
            sizes = (n * HW, n * HW, HW)
            bufs = [torch.full((4 + o + size + 8,), 7.0, device=DEV) for o, size in zip(offs[:2], sizes[:2])]
            bufs.append(torch.full((4 + offs[2] + HW + 8,), 7, dtype=torch.int32, device=DEV))
            assert all(b.data_ptr() % 16 == 0 for b in bufs)
            views = [b[4 + o:4 + o + size] for b, o, size in zip(bufs, offs, sizes)]
            check(lib().sdn_scene_id_planes(ptr(scene_d), ptr(disparity_d), ptr(ids_d), ptr(thr_d), n, H, W, views[0].data_ptr(),
                                            views[2].data_ptr(), views[1].data_ptr(), stream()))
            what = 'offsets %s' % (offs,)
            assert np.array_equal(views[0].cpu().numpy().reshape(n, 1, H, W), want_m.astype(np.float32)), what
            assert np.array_equal(views[1].cpu().numpy().reshape(n, 1, H, W), want_i.astype(np.float32)), what
            assert np.array_equal(views[2].cpu().numpy().view(np.uint32).reshape(1, H, W), want_c), what
            for b, o, size in zip(bufs, offs, sizes):
                assert bool((b[:4 + o] == 7).all()) and bool((b[4 + o + size:] == 7).all()), what


@pytest.fixture(scope='module')
def items():
    """per item case: the maps on the device, the records and the rows of the plain reference, computed once"""
    out = {}
    for name, (maps, records) in iu.item_cases().items():
        dev = [(_dev(s), _dev(d)) for s, d in maps]
        want = np.stack([iu.plain_item_row(maps[f][0], maps[f][1] if has else None, v) for f, v, has in records])
        out[name] = (maps, dev, records, want)
    return out


def _train_table(dev, records, max_pixels):
    from derender3d import scene as sc
    from derender3d import train_items as ti
    from sdn_hip import ops
    tab = ti.id_item_table([(dev[f][0], dev[f][1] if has else None, v) for f, v, has in records])
    return ops.train_id_stats(sc.upload_int32([tab], DEV)[0], max_pixels).cpu().numpy()


@pytest.mark.parametrize('name', ['single', 'mixed'])
def test_train_id_stats_equals_the_sort_with_any_grid(items, name):
    """ops.train_id_stats documents max_pixels as the largest H W of the batch; the kernels' comment states more: a workgroup
    walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of its frame, so any max_pixels >= 1 gives the same table.  This
    test pins the kernels' statement: with the largest H W every workgroup has one chunk, with max_pixels = 1 the grid is one
    workgroup per item and the chunk loops of k_tid_pass_a and k_tid_pass_b run up to four times."""
    maps, dev, records, want = items[name]
    largest = max(s.size for s, _ in maps)
    got = _train_table(dev, records, largest)
    assert got.dtype == np.int32 and got.shape == (len(records), 8)
    assert np.array_equal(got, want), _rows(got, want)
    one = _train_table(dev, records, 1)
    assert np.array_equal(one, want), _rows(one, want)
    assert _train_table(dev, records, largest).tobytes() == got.tobytes()
    if name == 'mixed':
        assert largest > 3 * iu.ID_CHUNK and len(records) > 150
        # the rows of the category are the rows of the scene chain
        for f, v, has in records:
            if has and 26000 <= v < 27000 and (maps[f][0] == v).any():
                assert np.array_equal(want[records.index((f, v, has))], iu.plain_stats(*maps[f])[v - 26000])
                break


def test_cityscapes_gt_inputs_on_the_crowd(cases, plain):
    """16 of 40 objects are kept and many areas are tied: the selection, the thresholds and the planes"""
    from derender3d import scene as sc
    scene, disparity, _ = cases['crowd']
    masks, cover, rois, areas, ids, thr = sc.cityscapes_gt_inputs(_dev(scene), _dev(disparity))
    sels, ids_w, rois_w, areas_w, thr_w = cu.select_emulated(plain['crowd'])
    assert len(ids) == 16 and len(set(areas_w.tolist())) < 16
    assert np.array_equal(ids, ids_w) and np.array_equal(rois, rois_w) and np.array_equal(areas, areas_w)
    assert np.array_equal(thr, thr_w) and np.array_equal(thr, iu.plain_thresholds(scene, disparity)[ids - 26000])
    assert rois.dtype == areas.dtype == ids.dtype == thr.dtype == np.int32
    want_m, _, want_c = cu.planes_emulated(scene, disparity, ids_w.tolist(), thr_w.tolist())
    assert np.array_equal(masks.cpu().numpy(), want_m.astype(np.float32))
    assert np.array_equal(cover.cpu().numpy().view(np.uint32), want_c)
