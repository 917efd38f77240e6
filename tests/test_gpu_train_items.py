"""derender3d/train_items.py on the device against the fixture the reference's own VKitti class produced
(tests/golden/make_geo_train_golden.py): sdn_train_rois, sdn_train_crops, train_batch.  Run at the fixture's shapes only."""
import numpy as np
import pytest
import torch

import geo_train_util as u
import sdn_hip
from derender3d import scene as sc
from derender3d import train_items as ti
from sdn_hip import ops
from test_geo_train_items import check_targets

pytestmark = pytest.mark.gpu
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope='module')
def g():
    return u.golden()


@pytest.fixture(scope='module')
def batches(g):
    """both batches of the fixture on the device and train_batch's answer for them, computed once"""
    out = {}
    for tag, is_train in (('t', True), ('e', False)):
        frames, scenes, items, jitter, rois = u.batch_items(g, tag)
        fd, sd = torch.tensor(frames).cuda(), torch.tensor(np.ascontiguousarray(scenes)).cuda()
        if is_train:
            batch = ti.train_batch(fd, sd, items, True, jitter=jitter, rois=rois)
        else:
            batch = ti.train_batch(fd, sd, items, False)
        out[tag] = (fd, sd, items, jitter, rois, batch)
    return out


def first_records(items):
    return torch.tensor([[it.frame] + it.code.tolist() for it in items], dtype=torch.int32).cuda()


@pytest.mark.parametrize('tag', ['t', 'e'])
def test_train_rois_equal_the_fixture_and_scene_gt_masks(g, batches, tag):
    fd, sd, items, _, _, _ = batches[tag]
    table = ops.train_rois(sd, first_records(items)).cpu().numpy()
    scenes = g[tag + '_scenes']
    areas = [int(np.all(scenes[it.frame] == it.code, axis=2).sum()) for it in items]
    assert np.array_equal(table[:, :4], g[tag + '_mask_rois']) and table[:, 4].tolist() == areas
    for f in range(sd.shape[0]):
        mine = [b for b, it in enumerate(items) if it.frame == f]
        codes = torch.from_numpy(np.stack([items[b].code for b in mine])).cuda()
        _, rois, ar = ops.scene_gt_masks(sd[f], codes)
        assert np.array_equal(torch.cat([rois, ar[:, None]], dim=1).cpu().numpy(), table[mine])


def test_an_absent_code_gives_the_invalid_row_and_an_index_error(batches):
    fd, sd, items, _, _, _ = batches['e']
    rec = first_records(items[:2])
    rec[1, 1:] = torch.tensor([9, 8, 7], dtype=torch.int32)
    table = ops.train_rois(sd, rec).cpu().numpy()
    assert table[1].tolist() == [INT_MAX, INT_MAX, 0, 0, 0] and table[0, 4] > 0
    rec[0, 0] = 99            # a frame index outside Fr: the row stays empty, nothing is read
    assert ops.train_rois(sd, rec).cpu().numpy()[0].tolist() == [INT_MAX, INT_MAX, 0, 0, 0]
    codes = items[0].codes.copy()
    codes[items[0].index] = (9, 8, 7)
    ghost = ti.Item(items[0].frame, items[0].index, items[0].rows, codes)
    with pytest.raises(IndexError):
        ti.train_batch(fd, sd, [items[1], ghost], False)


@pytest.mark.parametrize('tag', ['t', 'e'])
def test_train_batch_is_bit_identical_to_the_reference(g, batches, tag):
    _, _, items, _, _, batch = batches[tag]
    for k in ('images', 'masks', 'ignores'):
        want = torch.from_numpy(g['%s_%s' % (tag, k)])
        have = batch[k].cpu()
        for b in range(len(items)):
            assert torch.equal(have[b], want[b]), '%s of item %d: %d values differ' % (k, b, int((have[b] != want[b]).sum()))
    assert batch['targets'].dtype == torch.int64 and batch['targets'].is_cuda
    host = {k: v.cpu().numpy() for k, v in batch.items() if k in u.TARGET_KEYS}
    for b in range(len(items)):
        check_targets({k: host[k][b] for k in u.TARGET_KEYS}, g, tag, b)
    assert set(batch) == set(u.TARGET_KEYS) | {'images', 'masks', 'ignores'} and all(v.is_cuda for v in batch.values())


def test_an_empty_order_equals_scene_crops(g, batches):
    """every object of one frame, is_train False: the image and mask crops of sdn_scene_crops on the same rois, and its ignore
    crops where the nearer codes are distinct (there a union is a count)"""
    fd, sd, items, _, _, _ = batches['e']
    rows, codes = items[0].rows, items[0].codes
    assert items[0].frame == 0 and len({tuple(c) for c in codes.tolist()}) == len(codes)
    every = [ti.Item(0, k, rows, codes) for k in range(len(codes))]
    batch = ti.train_batch(fd, sd, every, False)
    masks, rois, _ = sc.scene_gt_inputs(sd[0], codes)
    assert np.array_equal(batch['rois'].cpu().numpy(), rois.astype(np.float32))
    plan = sc.CropPlan(rois, int(sd.shape[1]), int(sd.shape[2]), 224, 256, fd.device)
    rgbs, crops, cover = sc.image_mask_crops(plan, fd[0], masks, ti.VKITTI_MEAN, ti.VKITTI_STD)
    nearer = torch.zeros(len(every), 1, dtype=torch.int64)
    for k, it in enumerate(every):
        for j in ti.vkitti_targets(it.row(), rows, rois[k])[1]:
            nearer[k, 0] |= 1 << int(j)
    assert nearer.count_nonzero() >= 3
    ignores = ops.scene_crops(ops.SCENE_IGNORE, plan.rois, plan.tables, plan.height, plan.width, 224, 256, ignore_cover=cover,
                              nearer=nearer.cuda())[2]
    assert torch.equal(batch['images'], rgbs) and torch.equal(batch['masks'], crops) and torch.equal(batch['ignores'], ignores)


def test_two_calls_give_identical_bytes(batches):
    fd, sd, items, jitter, rois, batch = batches['t']
    again = ti.train_batch(fd, sd, items, True, jitter=jitter, rois=rois)
    for k in batch:
        assert torch.equal(batch[k], again[k]), k


def raw_call(fd, sd, rois, items_tab, nearer=None, image_size=224, mask_size=256, cut_tables=False, objs_edit=None):
    """ops.train_crops on hand-made tables"""
    rois = np.asarray(rois, np.int32).reshape(-1, 4)
    objs, bounds, kk8 = sc.crop_tables(rois, int(sd.shape[1]), int(sd.shape[2]), image_size, mask_size)
    if objs_edit is not None:
        objs = objs_edit(objs.copy())
    if cut_tables:
        kk8 = kk8[:kk8.shape[0] // 2]
    tables = sc.upload_int32([objs, bounds, kk8, items_tab], fd.device)
    nearer = torch.zeros(0, 3, dtype=torch.uint8).cuda() if nearer is None else nearer
    return ops.train_crops(fd, sd, rois, objs, items_tab, tables[:3], tables[3], nearer, image_size, mask_size)


def test_invalid_arguments_are_refused_before_any_launch(batches):
    fd, sd, items, _, _, _ = batches['e']
    code = items[0].code
    good = ti.item_table([0], [code], [0], [0], [ti.NO_JITTER])
    roi = [[10, 20, 50, 61]]
    images, masks, ignores = raw_call(fd, sd, roi, good)                 # the valid call the cases below are edits of
    torch.cuda.synchronize()
    E = sdn_hip.SdnHipError
    # crop_tables refuses an empty roi itself: hand the entry point the tables of another roi
    objs, bounds, kk8 = sc.crop_tables(roi, int(sd.shape[1]), int(sd.shape[2]), 224, 256)
    tabs = sc.upload_int32([objs, bounds, kk8, good], fd.device)
    none = torch.zeros(0, 3, dtype=torch.uint8).cuda()
    with pytest.raises(E, match='is empty'):
        ops.train_crops(fd, sd, np.int32([[10, 20, 10, 61]]), objs, good, tabs[:3], tabs[3], none)
    with pytest.raises(E, match='not crop_square'):
        ops.train_crops(fd, sd, np.int32([[10, 20, 52, 61]]), objs, good, tabs[:3], tabs[3], none)
    with pytest.raises(E, match='staging tile'):
        raw_call(fd, sd, [[0, 0, 5000, 10]], good)
    with pytest.raises(E, match='source rows per output row'):
        raw_call(fd, sd, [[0, 0, 3500, 10]], good, image_size=3000)
    bad = good.copy()
    bad[0, 0] = int(sd.shape[0])
    with pytest.raises(E, match='frame'):
        raw_call(fd, sd, roi, bad)
    bad[0, 0] = -1
    with pytest.raises(E, match='frame'):
        raw_call(fd, sd, roi, bad)
    bad = good.copy()
    bad[0, 2:4] = (0, 1)
    with pytest.raises(E, match='nearer codes'):
        raw_call(fd, sd, roi, bad)
    with pytest.raises(E, match='does not fit'):
        raw_call(fd, sd, roi, good, cut_tables=True)

    def past_the_end(objs):
        objs[0, 5] = 10 ** 6
        return objs
    with pytest.raises(E, match='does not fit'):
        raw_call(fd, sd, roi, good, objs_edit=past_the_end)
    bad = good.copy()
    bad[0, 4:6] = (2, 1 | 1 << 4)
    with pytest.raises(E, match='permutation'):
        raw_call(fd, sd, roi, bad)
    bad = ti.item_table([0], [code], [0], [0], [([ti.CONTRAST], (1, 0.5, 1), 0)])
    with pytest.raises(E, match='contrast'):
        raw_call(fd, sd, [[0, 0, 1500, 10]], bad)
    torch.cuda.synchronize()                                             # nothing was launched that could fault
    again = raw_call(fd, sd, roi, good)
    assert all(torch.equal(a, b) for a, b in zip((images, masks, ignores), again))


def test_cpu_tensors_raise(batches):
    fd, sd, items, _, _, _ = batches['e']
    with pytest.raises(NotImplementedError):
        ti.train_batch(fd.cpu(), sd, items, False)
    with pytest.raises(NotImplementedError):
        ti.train_batch(fd, sd.cpu(), items, False)
    with pytest.raises(NotImplementedError):
        ops.train_rois(sd.cpu(), first_records(items))
