"""maskrcnn.training_item (sdn_training_item, csrc/training_item.hip) against the reference's training item: the fixture
tests/golden/training_item_golden.npz holds what the reference's own load_image_gt, resize_image, resize_mask, extract_bboxes,
minimize_mask, compose_image_meta, mold_image and mold_inputs gave (tests/golden/make_training_item_golden.py);
tests/training_item_util.py restates them over the real Pillow and scipy for the jitter cases and the one case at the real size.

Every comparison is equality: every output is an integer or an exactly rounded value."""
import numpy as np
import pytest
import torch

import training_item_util as u
from maskrcnn import detection_targets as dt
from maskrcnn import rpn_targets as rt
from maskrcnn import training_item as ti   # the feature itself: without it this module does not import
from sdn_hip import pillow

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return u.golden()


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty that fills what it returns: NaN for floats, 99 for integers -- whatever a kernel leaves unwritten shows"""
    real_empty = torch.empty

    def poison(t):
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(99)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: poison(real_empty(*a, **k)))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def case_inputs(gold, name):
    p = name + '_'
    return up(gold[p + 'frame']), up(gold[p + 'inst_map']), up(gold[p + 'ids']), up(gold[p + 'class_ids'])


def numpy_item(item):
    d = {k: getattr(item, k).cpu().numpy() for k in ('image', 'gt_class_ids', 'gt_boxes', 'gt_boxes_int', 'gt_boxes_norm', 'gt_masks', 'areas', 'bad')}
    d['image_meta'], d['window'] = item.image_meta, item.window
    return d


def expected(gold, name, flip, use_mini):
    """what the fixture holds for the case, in the layout of the item"""
    cfg, p = u.case_config(gold, name), name + '_'
    G, M = len(gold[p + 'ids']), cfg.IMAGE_MAX_DIM
    image, full = gold[p + 'image_u8'], u.unpack(gold, p + 'full_bits', (M, M, G))
    if flip:
        image, full = np.fliplr(image), np.fliplr(full)
    masks = u.unpack(gold, p + 'mini_bits%d' % flip, cfg.MINI_MASK_SHAPE + (G,)) if use_mini else full
    boxes = gold[p + 'boxes%d' % flip]
    return {'image': u.mold(image, cfg), 'gt_boxes_int': boxes, 'gt_boxes': boxes.astype(np.float32),
            'gt_boxes_norm': (boxes.astype(np.float32) / np.float32(M))[None], 'gt_class_ids': gold[p + 'class_ids'],
            'gt_masks': np.ascontiguousarray(masks.transpose(2, 0, 1)).astype(np.float32), 'areas': gold[p + 'areas'], 'bad': gold[p + 'bad'],
            'image_meta': gold[p + 'meta'], 'window': tuple(gold[p + 'plan'][2:6].tolist())}


def same_bits(got, want, what):
    for k, w in want.items():
        g = got[k]
        if k == 'window':
            assert tuple(g) == tuple(w), (what, k)
            continue
        g, w = np.asarray(g), np.asarray(w)
        if k == 'image_meta':
            assert g.tolist() == w.tolist(), (what, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, int((g != w).sum()))


@pytest.mark.parametrize('name', u.CASES)
def test_the_item_equals_the_fixture(gold, name):
    cfg = u.case_config(gold, name)
    frame, inst_map, ids, class_ids = case_inputs(gold, name)
    assert inst_map.dtype == (torch.uint8 if name in ('down', 'exact') else torch.int32)   # both forms of the map
    for flip in (0, 1):
        for use_mini in (False, True):
            item = ti.training_item(frame, inst_map, ids, class_ids, cfg, flip=flip, use_mini_mask=use_mini)
            same_bits(numpy_item(item), expected(gold, name, flip, use_mini), (name, flip, use_mini))
    item = ti.training_item(frame, inst_map, ids, class_ids, cfg)           # use_mini_mask None reads the config
    assert tuple(item.gt_masks.shape) == (len(ids),) + cfg.MINI_MASK_SHAPE and tuple(item.gt_boxes_norm.shape) == (1, len(ids), 4)


def test_the_cases_quirks(gold):
    """asserted by the generator on the reference's output, here on the device's: the solid rectangle, the vanished instance, the line"""
    cfg = u.case_config(gold, 'down')
    item = ti.training_item(*case_inputs(gold, 'down'), cfg, use_mini_mask=True)
    boxes, masks, areas = item.gt_boxes_int.cpu().numpy(), item.gt_masks.cpu().numpy(), item.areas.cpu().numpy()
    hh, ww = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    assert areas[2] == hh[2] * ww[2] > 0 and masks[2].sum() == 0
    assert areas[3] == 0 and boxes[3].tolist() == [0, 0, 0, 0] and masks[3].sum() == 0 and item.bad.cpu().tolist() == [1]
    assert ww[4] == 1 and masks[4].sum() > 0
    assert ww[5] > 56 and ww[0] < 56 and ww[6] == 56 and boxes[1, 3] == 191


def test_load_image_gt_returns_the_references_five(gold):
    cfg = u.case_config(gold, 'up')
    image, meta, class_ids, bbox, mask = ti.load_image_gt(*case_inputs(gold, 'up'), cfg, image_id=0, flip=True, use_mini_mask=False)
    want = expected(gold, 'up', 1, False)
    assert image.cpu().numpy().tobytes() == want['image'].tobytes() and meta.tolist() == want['image_meta'].tolist()
    assert class_ids.cpu().numpy().tobytes() == want['gt_class_ids'].tobytes() and bbox.cpu().numpy().tobytes() == want['gt_boxes_int'].tobytes()
    assert tuple(mask.shape) == (192, 192, 3) and np.array_equal(mask.cpu().numpy(), want['gt_masks'].transpose(1, 2, 0))


@pytest.mark.parametrize('order', [[pillow.HUE, pillow.BRIGHTNESS, pillow.SATURATION], [pillow.SATURATION, pillow.CONTRAST, pillow.HUE, pillow.BRIGHTNESS],
                                   [pillow.CONTRAST], [pillow.BRIGHTNESS, pillow.CONTRAST]])
@pytest.mark.parametrize('name', ['down', 'same'])
def test_the_jitter_cases_equal_the_util(gold, name, order):
    """The last order puts an op that moves the mean of L in front of contrast: saturation, in the second, blends around L and keeps
    it, so a luma sum taken before the preceding ops gives the same grey there."""
    cfg, p = u.case_config(gold, name), name + '_'
    jitter = (order, (1.3, 0.7, 1.4), 37)
    item = ti.training_item(*case_inputs(gold, name), cfg, flip=1, jitter=jitter)
    want = u.training_item(gold[p + 'frame'], gold[p + 'inst_map'], gold[p + 'ids'], cfg, flip=True, jitter=jitter, use_mini_mask=True)
    plain = expected(gold, name, 1, True)
    assert want['image'].tobytes() != plain['image'].tobytes()                      # the jitter shows
    del want['image_u8']
    same_bits(numpy_item(item), want, (name, order))
    same_bits(numpy_item(item), {k: plain[k] for k in ('gt_boxes_int', 'gt_masks', 'areas')}, (name, order))   # and touches the image alone


def test_mold_inputs_equals_the_fixture(gold):
    cfg = u.Config(64, 128, 28)
    names = [str(n) for n in gold['mold_names']]
    assert len(set(names)) == 3 and len(names) == 4
    molded, metas, windows = ti.mold_inputs([up(gold[n + '_frame']) for n in names], cfg)
    assert molded.dtype == torch.float32 and tuple(molded.shape) == (4, 3, 128, 128)
    got = molded.cpu().numpy()
    for k, n in enumerate(names):
        assert got[k].tobytes() == u.mold(gold[n + '_image_u8'], cfg).tobytes(), n
    assert metas.tolist() == gold['mold_metas'].tolist() and windows.tolist() == gold['mold_windows'].tolist()
    one, _, _ = ti.mold_inputs([up(gold['many_frame'])], cfg)
    assert one.cpu().numpy()[0].tobytes() == u.mold(gold['many_image_u8'], cfg).tobytes()


def test_no_poison_and_two_runs_give_the_same_bits(gold, poisoned_empty):
    for name, use_mini in (('down', True), ('many', True), ('up', False)):
        cfg = u.case_config(gold, name)
        inputs = case_inputs(gold, name)
        a = numpy_item(ti.training_item(*inputs, cfg, flip=1, use_mini_mask=use_mini))
        b = numpy_item(ti.training_item(*inputs, cfg, flip=1, use_mini_mask=use_mini))
        same_bits(a, expected(gold, name, 1, use_mini), name)
        same_bits(b, {k: v for k, v in a.items()}, name)


class ChainConfig(u.Config):
    RPN_TRAIN_ANCHORS_PER_IMAGE = 64
    RPN_BBOX_STD_DEV = np.array([0.1, 0.1, 0.2, 0.2])
    TRAIN_ROIS_PER_IMAGE = 32
    ROI_POSITIVE_RATIO = 0.33
    BBOX_STD_DEV = np.array([0.1, 0.1, 0.2, 0.2])
    MASK_SHAPE = [28, 28]


def test_the_item_feeds_the_rpn_and_the_detection_targets(gold):
    name = 'down'
    base = u.case_config(gold, name)
    cfg = ChainConfig(base.IMAGE_MIN_DIM, base.IMAGE_MAX_DIM, base.MINI_MASK_SHAPE[0])
    M = cfg.IMAGE_MAX_DIM
    item = ti.training_item(*case_inputs(gold, name), cfg, flip=0, use_mini_mask=True)
    want = expected(gold, name, 0, True)
    anchors = up(rt.generate_pyramid_anchors((16, 32, 64), [0.5, 1, 2], [[M // s, M // s] for s in (4, 8, 16)], [4, 8, 16], 1))
    gen = torch.Generator().manual_seed(5)
    rpn_keys = torch.rand(2, anchors.shape[0], generator=gen).to(DEV)
    corners = torch.rand(200, 2, 2, generator=gen).sort(dim=1).values                # (y1, x1), (y2, x2) normalised
    proposals = corners.reshape(200, 4).contiguous().to(DEV)
    roi_keys = torch.rand(2, 200, generator=gen).to(DEV)
    mine = rt.rpn_targets_padded(anchors, item.gt_class_ids, item.gt_boxes, cfg, keys=rpn_keys) + \
        dt.detection_targets_padded(proposals, item.gt_class_ids, item.gt_boxes_norm, item.gt_masks, cfg, keys=roi_keys)
    host = rt.rpn_targets_padded(anchors, up(want['gt_class_ids']), up(want['gt_boxes']), cfg, keys=rpn_keys) + \
        dt.detection_targets_padded(proposals, up(want['gt_class_ids']), up(want['gt_boxes_norm']), up(want['gt_masks']), cfg, keys=roi_keys)
    assert len(mine) == len(host) == 10
    for k, (a, b) in enumerate(zip(mine, host)):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), k
    assert int(mine[3][0]) > 0 and int(mine[9][0]) > 0                               # there are positives on both sides


def test_the_real_size_with_a_box_taller_than_256_rows():
    """375 x 1242 -> 309 x 1024 in 1024 x 1024, the reference's sizes; the expectation is the util's, computed here"""
    rng = np.random.default_rng(11)
    H, W, cfg = 375, 1242, u.Config(800, 1024, 56)
    yy, xx = np.mgrid[0:H, 0:W]
    frame = np.clip((xx * 255 // (W - 1))[..., None] + rng.integers(-80, 81, (H, W, 3)), 0, 255).astype(np.uint8)
    codes = np.array([[200, 30, 100], [10, 27, 44], [0, 255, 7], [90, 90, 91]], np.uint8)
    scene = np.zeros((H, W, 3), np.uint8)
    scene[((yy - 187) / 180.0) ** 2 + ((xx - 300) / 90.0) ** 2 <= 1.0] = codes[0]      # 361 rows: 297 after the resize
    scene[((yy - 100) / 40.0) ** 2 + ((xx - 800) / 300.0) ** 2 <= 1.0] = codes[1]      # 601 columns wide
    scene[300:360, 1100:1242] = codes[2]
    scene[300:310, 1100:1110] = 0                                                      # touches the right edge, not solid
    scene[20:28, 600:640] = codes[3]
    scene[20:24, 600:620] = 0
    ids = ti.color_keys(codes)
    want = u.training_item(frame, scene, ids, cfg, flip=True, use_mini_mask=True)
    hh = want['gt_boxes_int'][:, 2] - want['gt_boxes_int'][:, 0]
    assert hh[0] > 256 and want['gt_boxes_int'][2, 1] == 0 and (want['gt_masks'].sum(axis=(1, 2)) > 0).all()
    item = ti.training_item(up(frame), up(scene), up(ids), up(np.array([1, 2, 1, 3], np.int32)), cfg, flip=1)
    del want['image_u8']
    same_bits(numpy_item(item), want, 'real size')
