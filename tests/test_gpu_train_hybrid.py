"""derender3d/train_items.py's hybrid half on the device against the fixture the reference's own dataset classes and collate_fn
produced (tests/golden/make_geo_hybrid_golden.py): sdn_train_id_stats, sdn_train_crops_mixed, hybrid_batch.  Run at the
fixture's shapes only."""
import numpy as np
import pytest
import torch

import geo_hybrid_util as h
import geo_train_util as u
import sdn_hip
from derender3d import scene as sc
from derender3d import train_items as ti
from sdn_hip import ops
from test_geo_train_items import ulps

pytestmark = pytest.mark.gpu
INT_MAX = 2 ** 31 - 1
TAGS = ['vk', 'ko', 'ks', 'cs', 'ce', 'mr', 'mt', 'vc', 'kk']


@pytest.fixture(scope='module')
def g():
    return h.golden()


@pytest.fixture(scope='module')
def batches(g):
    """every batch of the fixture through hybrid_batch with the recorded rois and parameters, computed once"""
    assert h.batch_tags(g) == TAGS
    out = {}
    for tag in TAGS:
        keys, items, jitter, rois, is_train = h.host_items(g, tag)
        frames = h.device_frames(g, keys)
        batch = ti.hybrid_batch(frames, items, is_train, jitter=jitter, rois=rois) if is_train else ti.hybrid_batch(frames, items, False)
        out[tag] = (frames, items, jitter, rois, is_train, batch)
    return out


@pytest.mark.parametrize('tag', TAGS)
def test_hybrid_batch_is_bit_identical_to_the_collated_dict(g, batches, tag):
    batch = batches[tag][5]
    assert set(batch) == set(str(k) for k in g[tag + '_keys']) and all(v.is_cuda for v in batch.values())
    for k, v in batch.items():
        want = g['%s_%s' % (tag, k)]
        have = v.cpu().numpy()
        assert have.dtype == want.dtype and have.shape == want.shape, (k, have.dtype, have.shape)
        if k in u.LIBM_KEYS:      # through the host's log / cos / sin: one float32 step between machines, as test_geo_train_items
            assert ulps(have, want).max() <= 1, k
        else:
            assert np.array_equal(have, want), '%s: %d values differ' % (k, int((have != want).sum()))


def test_drawn_rois_and_jitters_follow_the_recorded_seeds(g, batches):
    """is_train with nothing prescribed: the module draws, item by item, what the reference drew under the same seed"""
    import random
    for tag in ('vc', 'cs'):
        frames, items, _, _, _, _ = batches[tag]
        drawn = np.flatnonzero(g[tag + '_drawn_roi'] & g[tag + '_drawn_jitter'])
        assert drawn.size
        for b in drawn:
            random.seed(int(g[tag + '_seeds'][b]))
            one = ti.hybrid_batch(frames, [items[b]], True)
            for k in ('images', 'masks', 'ignores'):
                assert np.array_equal(one[k].cpu().numpy()[0], g['%s_%s' % (tag, k)][b]), (tag, b, k)


def test_train_id_stats_equals_numpy_on_random_maps():
    rng = np.random.default_rng(5)
    shapes = [(37, 53), (64, 96), (50, 156)]          # 37 x 53 = 1961 is no multiple of 4
    maps = []
    for H, W in shapes:
        ids = rng.integers(0, 6, (H // 6 + 1, W // 7 + 1)).repeat(6, 0).repeat(7, 1)[:H, :W].astype(np.int32) + 26000
        disp = rng.integers(0, 65536, (H, W)).astype(np.int32)
        disp[rng.random((H, W)) < 0.3] = 0
        disp[ids == 26003] = rng.integers(0, 4, int((ids == 26003).sum())) * 500      # ties
        maps.append((ids, disp))
    dev = [(torch.tensor(i).cuda(), torch.tensor(d).cuda()) for i, d in maps]
    recs = [(0, 26001, True), (0, 26003, True), (1, 26002, True), (1, 26002, True), (2, 26005, True), (2, 99, True), (1, 26004, False),
            (0, 26000, True)]
    table = ops.train_id_stats(sc.upload_int32([ti.id_item_table([(dev[f][0], dev[f][1] if has else None, k) for f, k, has in recs])],
                                               dev[0][0].device)[0], max(H * W for H, W in shapes)).cpu().numpy()
    for row, (f, k, has) in zip(table, recs):
        ids, disp = maps[f]
        m = ids == k
        if not m.any():
            assert row.tolist() == [0, INT_MAX, INT_MAX, 0, 0, 0, 0, 0]
            continue
        ys, xs = np.nonzero(m)
        n, lo, hi = h.order_statistics(disp[m]) if has else (0, 0, 0)
        assert row.tolist() == [int(m.sum()), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, n, lo, hi], (f, k)
    assert (table[:, 5] > 1).sum() >= 4 and (table[:, 0] == 0).sum() == 1


def test_a_vkitti_batch_equals_train_crops(g):
    """the items of the VKITTI fixture through the mixed entry: train_batch's outputs, bit for bit"""
    tg = u.golden()
    frames, scenes, items, jitter, rois = u.batch_items(tg, 't')
    items, jitter, rois = items[:8], jitter[:8], rois[:8]
    fd, sd = torch.tensor(frames).cuda(), torch.tensor(np.ascontiguousarray(scenes)).cuda()
    want = ti.train_batch(fd, sd, items, True, jitter=jitter, rois=rois)
    have = ti.hybrid_batch([ti.SourceFrame(fd[f], sd[f]) for f in range(fd.shape[0])], items, True, jitter=jitter, rois=rois)
    assert set(have) == set(want)
    for k in want:
        assert torch.equal(have[k], want[k]), k


def raw_call(frame, roi, edit=None, maps=True, objs_edit=None, image_size=224, tables_edit=None):
    rec = {'frame': frame.rgb_u8, 'mask': (ti.MASK_ID, frame.ids, 26001), 'ignore': (ti.IGNORE_DISPARITY, frame.disparity, 100, 0, 0),
           'jitter': ti.NO_JITTER, 'mean': ti.IMAGENET_MEAN, 'std': ti.IMAGENET_STD}
    tab = ti.mixed_item_table([rec])
    if edit is not None:
        edit(tab)
    rois = np.int32([roi])
    objs, bounds, kk8 = sc.crop_tables([[10, 20, 50, 70]] if objs_edit == "other" else rois, frame.H, frame.W, max(image_size, 1), 256)
    if tables_edit is not None:
        objs, bounds, kk8 = tables_edit(objs.copy(), bounds, kk8)
    d = sc.upload_int32([tab, objs, bounds, kk8], frame.rgb_u8.device)
    none = torch.zeros(0, 3, dtype=torch.uint8).cuda()
    return ops.train_crops_mixed(rois, objs, tab, d[1:4], d[0], none, image_size, 256, maps=maps)


def test_invalid_tables_are_refused_before_any_launch(g):
    frame = h.device_frames(g, ['cs000019'])[0]
    roi = [10, 20, 50, 70]
    good = raw_call(frame, roi)
    torch.cuda.synchronize()
    E = sdn_hip.SdnHipError

    def put(col, value, wide=False):
        def edit(tab):
            (tab.view(np.uint64) if wide else tab)[0, col] = value
        return edit
    cases = [('null frame', put(0, 0, True)), ('null mask source', put(1, 0, True)), ('null ignore source', put(2, 0, True)),
             ('mask source kind', put(8, 3)), ('mask source kind', put(8, -1)), ('ignore source kind', put(10, 3)),
             ('ignore source kind', put(10, -1)), ('a frame of', put(6, 0)), ('a frame of', put(7, -5)),
             ('not aligned', put(1, frame.ids.data_ptr() + 2, True)), ('nearer codes', lambda t: t.__setitem__((0, slice(10, 14)), (1, 0, 0, 1))),
             ('ops, hue', put(19, 256)), ('permutation', lambda t: t.__setitem__((0, slice(14, 16)), (2, 1 | 1 << 4))),
             ('std is 0', put(24, 0))]
    for match, edit in cases:
        with pytest.raises(E, match=match):
            raw_call(frame, roi, edit)
    with pytest.raises(E, match='no masks / ignores output'):
        raw_call(frame, roi, maps=False)
    with pytest.raises(E, match='not crop_square'):
        raw_call(frame, [10, 20, 52, 70], objs_edit='other')
    with pytest.raises(E, match='staging tile'):
        raw_call(frame, [0, 0, 5000, 10])
    with pytest.raises(E, match='contrast'):
        raw_call(frame, [0, 0, 1500, 10], lambda t: t.__setitem__((0, slice(14, 16)), (1, ti.CONTRAST)))
    with pytest.raises(E, match='is empty'):
        raw_call(frame, [10, 20, 10, 70], objs_edit='other')
    with pytest.raises(E, match='bad crop sizes'):       # above the 12288 bytes of a row tile; nothing is written to the output
        raw_call(frame, roi, image_size=12289)
    with pytest.raises(E, match='source rows per output row'):
        raw_call(frame, [0, 0, 3500, 10], image_size=3000)

    def a_table_pillow_skips(objs, bounds, kk8):
        objs[0, 5:8] = (0, 0, 3)
        return objs, bounds, kk8
    with pytest.raises(E, match='Pillow skips'):
        raw_call(frame, [0, 0, 224, 100], tables_edit=a_table_pillow_skips)
    with pytest.raises(E, match='does not fit'):
        raw_call(frame, roi, tables_edit=lambda objs, bounds, kk8: (objs, bounds, kk8[:kk8.shape[0] // 2]))
    with pytest.raises(E, match='does not fit'):
        raw_call(frame, roi, tables_edit=lambda objs, bounds, kk8: (objs, bounds[:bounds.shape[0] // 2], kk8))

    def past_the_end(objs, bounds, kk8):
        objs[0, 5] = 10 ** 6
        return objs, bounds, kk8
    with pytest.raises(E, match='does not fit'):
        raw_call(frame, roi, tables_edit=past_the_end)
    with pytest.raises(E, match='bad sizes'):
        ops.train_id_stats(torch.zeros(1, 8, dtype=torch.int32).cuda(), 0)
    torch.cuda.synchronize()                                             # nothing was launched that could fault
    again = raw_call(frame, roi)
    assert all(torch.equal(a, b) for a, b in zip(good, again))


def test_an_absent_id_or_code_raises_index_error(g, batches):
    frames, items, _, _, _, _ = batches['vc']
    with pytest.raises(IndexError):
        ti.hybrid_batch(frames, [items[0], ti.CityscapesItem(items[1].frame, 26099)], False)
    codes = items[0].codes.copy()
    codes[items[0].index] = (9, 8, 7)
    with pytest.raises(IndexError):
        ti.hybrid_batch(frames, [ti.Item(items[0].frame, items[0].index, items[0].rows, codes), items[1]], False)


def test_two_runs_give_identical_outputs(batches):
    for tag in ('vc', 'cs'):
        frames, items, jitter, rois, is_train, batch = batches[tag]
        again = ti.hybrid_batch(frames, items, is_train, jitter=jitter, rois=rois)
        for k in batch:
            assert torch.equal(batch[k], again[k]), (tag, k)


def test_a_training_step_on_the_vkitti_cityscapes_batch(g, batches):
    """hybrid_batch (VKITTI + Cityscapes) -> Derenderer3d in .train() -> step_losses(mode=full) -> backward: finite losses, and
    geometry losses equal to those of the VKITTI items alone, made by train_batch and given the same predictions.  Both
    evaluations add the same fp64 terms in the same order (an item without the geometry bit adds exact zeros), so the fp32
    results may differ by the final rounding at most: one float32 step."""
    from derender3d import TargetType
    from derender3d import losses as L
    from test_gpu_dropin import _geometric_model
    frames, items, jitter, rois, is_train, batch = batches['vc']
    vk = [b for b, it in enumerate(items) if isinstance(it, ti.Item)]
    assert is_train and 0 < len(vk) < len(items) and any(isinstance(it, ti.CityscapesItem) for it in items)
    assert batch['targets'].tolist() == [int(TargetType.full) if b in vk else int(TargetType.finetune) for b in range(len(items))]
    torch.manual_seed(11)
    net, _ = _geometric_model(render_size=384)
    net = net.cuda().train()
    net.zero_grad()
    blob = net(batch['images'], batch['roi_norms'], batch['focals'])
    got = L.step_losses(blob, batch, TargetType.full)
    assert list(got) == list(L.step_loss_keys(TargetType.full))
    sum(got.values()).backward()
    for k, v in got.items():
        print('hybrid step %s: %.9g' % (k, float(v.detach())))
        assert np.isfinite(float(v.detach())), k
    assert torch.isfinite(net.derenderer.net.conv1.weight.grad).all() and float(net.derenderer._fc3.weight.grad.abs().max()) > 0
    # the VKITTI items alone through train_batch, with the predictions the hybrid batch got for them
    used = sorted({items[b].frame for b in vk})
    assert len({(frames[f].H, frames[f].W) for f in used}) == 1
    fd = torch.stack([frames[f].rgb_u8 for f in used])
    sd = torch.stack([frames[f].scene_u8 for f in used])
    alone_items = [ti.Item(used.index(items[b].frame), items[b].index, items[b].rows, items[b].codes) for b in vk]
    alone = ti.train_batch(fd, sd, alone_items, True, jitter=[jitter[b] for b in vk], rois=np.asarray(rois)[vk])
    index = torch.tensor(vk).cuda()
    for k in ('images', 'masks', 'ignores', 'thetas', 'translation2ds', 'log_scales', 'log_depths'):
        assert torch.equal(alone[k], batch[k][index]), k
    sub = {k: v.detach()[index].contiguous() for k, v in blob.items() if isinstance(v, torch.Tensor) and v.dim() and v.shape[0] == len(items)}
    ref = L.step_losses(sub, alone, TargetType.pretrain)
    assert list(ref) == list(L.GEOMETRY_LOSSES)
    for k in L.GEOMETRY_LOSSES:
        a, b = got[k].detach().cpu().numpy(), ref[k].detach().cpu().numpy()
        print('hybrid step %s: mixed %.9g, VKITTI items alone %.9g' % (k, float(a), float(b)))
        assert float(b) != 0 and ulps(a, b).max() <= 1, (k, a, b)
