"""GPU: the detector-output path -- sdn_unmold_masks / sdn_scene_gt_masks, maskrcnn.detections and
SceneSession.from_detections / from_scene_gt -- against tests/golden/detections_golden.npz (the reference's statements,
executed).  Every comparison is exact: the kernels restate integer and single IEEE fp32 operations.

  * planes and areas bit-equal for every detection of every case; the areas-only call equals the full call's areas;
  * unmold_detections returns the fixture's boxes, ids, scores and masks; the N = 0 shapes; an out-of-frame box raises;
  * from_detections selects the fixture's `sels`, its crops and interests equal those of a SceneSession built from the
    fixture's reference masks; from_detections(...).edit(...) -> EditSession.render_batch once;
  * scene_gt_masks masks, rois, areas bit-equal; the unmatched code raises; from_scene_gt."""
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

import detections_util as du  # noqa: E402
from maskrcnn import detections as det  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
R = 64


@pytest.fixture(scope='module')
def gold():
    return du.load()


@pytest.fixture(scope='module')
def geo():
    from derender3d import TargetType
    from derender3d.models import Derenderer3d, ShapenetObj
    from sdn_hip import synth
    objs = []
    for k in range(8):
        v, f = synth.car_like(600, seed=300 + k)
        objs.append(ShapenetObj(vertices=v[:, [2, 1, 0]] * np.asarray([-1, 1, 1], np.float32), faces=f))
    torch.manual_seed(21)
    return Derenderer3d(mode=TargetType.extend, image_size=64, render_size=R, objs=objs).to(DEV).eval()


def _plan(g, tag):
    H, W = (int(v) for v in g[tag + '_image_shape'][:2])
    boxes, ids, scores, keep = det.unmold_boxes(g[tag + '_detections'], (H, W), g[tag + '_window'])
    return det.UnmoldPlan(torch.from_numpy(g[tag + '_mrcnn_mask']).to(DEV), boxes, ids, keep, H, W)


def _same_planes(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert set(np.unique(got).tolist()) <= {0.0, 1.0}, what + ': values other than 0.0 and 1.0'
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i].astype(np.float32)), '%s: plane %d: %d pixels differ' % (
            what, i, int((got[i] != want[i]).sum()))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_unmold_masks_bit_equal_to_the_fixture(gold, tag):
    plan = _plan(gold, tag)
    masks, areas = plan.masks()
    _same_planes(masks, du.planes(gold, tag), 'case ' + tag)
    assert areas.dtype == torch.int32 and np.array_equal(areas.cpu().numpy(), gold[tag + '_areas'])
    only = plan.areas()
    assert torch.equal(only, areas)
    # a subset in another order
    if tag == 'a':
        sel = gold['a_sels']
        sub, sub_areas = plan.masks(sel)
        _same_planes(sub, du.planes(gold, tag)[sel], 'selected planes')
        assert np.array_equal(sub_areas.cpu().numpy(), gold['a_areas'][sel])


def test_planes_into_an_unaligned_dirty_buffer(gold):
    """the planes of a view that starts 4 bytes into an allocation and held 7.0: every element written, nothing beside"""
    from sdn_hip import check, lib, ptr, stream
    g = gold
    plan = _plan(g, 'b')
    H, W, n = plan.height, plan.width, plan.n
    buf = torch.full((n * H * W + 8,), 7.0, device=DEV)
    view = buf[1:1 + n * H * W]
    objs, bounds, kk8 = plan.tables
    check(lib().sdn_unmold_masks(ptr(plan.mrcnn_mask), *plan.mrcnn_mask.shape, plan.objs_host.ctypes.data, ptr(objs), n, ptr(bounds),
                                 bounds.shape[0], ptr(kk8), kk8.shape[0], H, W, view.data_ptr(), None, stream()))
    _same_planes(view.reshape(n, 1, H, W), du.planes(g, 'b'), 'unaligned')
    assert float(buf[0]) == 7.0 and bool((buf[1 + n * H * W:] == 7.0).all())


def test_unmold_detections_returns_the_reference_tuple(gold):
    g = gold
    for tag in 'ab':
        H, W = (int(v) for v in g[tag + '_image_shape'][:2])
        boxes, ids, scores, masks = det.unmold_detections(torch.from_numpy(g[tag + '_detections']).to(DEV),
                                                          torch.from_numpy(g[tag + '_mrcnn_mask']).to(DEV), (H, W, 3), g[tag + '_window'])
        for got, want in ((boxes, g[tag + '_boxes']), (ids, g[tag + '_class_ids']), (scores, g[tag + '_scores'])):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert masks.is_cuda
        _same_planes(masks, du.planes(g, tag), 'unmold_detections ' + tag)
    # no detection: the empty arrays of model.py:2140-2141, the masks in this module's layout
    boxes, ids, scores, masks = det.unmold_detections(torch.from_numpy(g['c_detections']).to(DEV),
                                                      torch.from_numpy(g['c_mrcnn_mask']).to(DEV), (60, 90, 3), g['c_window'])
    assert boxes.shape == (0, 4) and ids.shape == (0,) and scores.shape == (0,) and tuple(masks.shape) == (0, 1, 60, 90)
    # a box that leaves the frame
    d = g['a_detections'].copy()
    d[0, 3] += 900.0
    with pytest.raises(ValueError, match='leaves the 375 x 1242 frame'):
        det.unmold_detections(torch.from_numpy(d).to(DEV), torch.from_numpy(g['a_mrcnn_mask']).to(DEV), (375, 1242, 3), g['a_window'])


def test_the_launcher_refuses_what_would_leave_the_buffers(gold):
    from sdn_hip import SdnHipError, ops
    plan = _plan(gold, 'b')
    for col, value, match in ((5, plan.width + 1, 'leaves'), (0, 4, 'detection'), (1, 3, 'class'), (6, 100000, 'table')):
        bad = plan.objs_host.copy()
        bad[0, col] = value
        with pytest.raises(SdnHipError, match=match):
            ops.unmold_masks(plan.mrcnn_mask, bad, plan.tables, plan.height, plan.width)


def _frame(H, W, seed=5):
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 256, (3, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(cell.repeat(8, 1).repeat(8, 2)[:, :H, :W])).to(DEV)


CAMERA = du.Camera(725.0, 620.5, 187.0)


def test_from_detections_equals_a_session_of_the_reference_masks(gold, geo):
    from derender3d import scene
    g = gold
    image = _frame(375, 1242)
    sess = scene.SceneSession.from_detections(geo, CAMERA, image, torch.from_numpy(g['a_detections']).to(DEV),
                                              torch.from_numpy(g['a_mrcnn_mask']).to(DEV), g['a_window'], image_size=64, mask_size=48)
    sels = g['a_sels']
    assert np.array_equal(sess.detection_sels, sels) and np.array_equal(sess.rois, g['a_sel_rois'])
    assert sess.class_ids == g['a_sel_class_ids'].tolist() and np.array_equal(sess.mask_areas, g['a_areas'][sels])
    ref_masks = torch.from_numpy(du.planes(g, 'a')[sels].astype(np.float32)).to(DEV)
    assert torch.equal(sess.image_masks, ref_masks)
    ref = scene.SceneSession(geo, CAMERA, image, g['a_sel_class_ids'], ref_masks, g['a_sel_rois'], image_size=64, mask_size=48)
    assert torch.equal(sess.rgbs, ref.rgbs) and torch.equal(sess.masks, ref.masks)
    assert sess.interests == ref.interests and any(sess.interests)
    # fewer objects than detections, and none
    few = scene.SceneSession.from_detections(geo, CAMERA, image, torch.from_numpy(g['a_detections']).to(DEV),
                                             torch.from_numpy(g['a_mrcnn_mask']).to(DEV), g['a_window'], max_objects=3,
                                             image_size=64, mask_size=48)
    assert few.detection_sels.tolist() == sels[:3].tolist() and tuple(few.image_masks.shape) == (3, 1, 375, 1242)
    with pytest.raises(ValueError, match='no detections'):
        scene.SceneSession.from_detections(geo, du.Camera(90.0, 44.5, 29.5), _frame(60, 90), torch.from_numpy(g['c_detections']).to(DEV),
                                           torch.from_numpy(g['c_mrcnn_mask']).to(DEV), g['c_window'], image_size=64, mask_size=48)
    with pytest.raises(NotImplementedError):
        scene.SceneSession.from_detections(geo, CAMERA, image, g['a_detections'], torch.from_numpy(g['a_mrcnn_mask']), g['a_window'])


def test_from_detections_to_edit_session(gold, geo):
    import edit_util as eu
    from derender3d import scene
    from edit import EditSession
    from models.pix2pixHD_model import Pix2PixHDModel
    g = gold
    H, W = 94, 158
    image = _frame(H, W)
    # two detections of an image that was not molded (window = the image): the soft masks of case a, boxes + 0.25
    d = np.zeros((5, 6), np.float32)
    d[:2] = [[20.25, 10.25, 60.25, 70.25, 1, 0.9], [30.25, 60.25, 75.25, 120.25, 2, 0.8]]
    sess = scene.SceneSession.from_detections(geo, du.Camera(90.0, 79.0, 47.0), image, torch.from_numpy(d).to(DEV),
                                              torch.from_numpy(g['a_mrcnn_mask'][:5]).to(DEV), (0, 0, H, W), image_size=64, mask_size=48)
    assert sess.interests == [True, True] and sorted(sess.rois.tolist()) == [[20, 10, 60, 70], [30, 60, 75, 120]]
    opt = eu.options(24, fineHeight=96)
    torch.manual_seed(31)
    tex = Pix2PixHDModel()
    tex.initialize(opt)
    rng = np.random.default_rng(9)
    segm = torch.from_numpy(rng.integers(0, 13, (1, H, W), dtype=np.uint8)).to(DEV)
    source = sess.reconstruct()
    es = EditSession(tex, opt, eu.PARAMS, segm, image, source.inst_u8)
    frames = sess.edit([[{'type': 'modify', 'from': {'u': 40, 'v': 40}, 'to': {'u': 60, 'v': 45}, 'zoom': 1.2, 'ry': 0.5}], []])
    out = es.render_batch([(fr.inst_u8, fr.json, fr.normal_u8) for fr in frames], strict=False)
    assert tuple(out.shape) == (2, 3, 96, 160) and bool(torch.isfinite(out).all())


def test_scene_gt_masks_bit_equal_to_the_fixture(gold, geo):
    from derender3d import scene
    from sdn_hip import ops
    g = gold
    scene_d = torch.from_numpy(g['g_scene']).to(DEV)
    masks, rois, areas = ops.scene_gt_masks(scene_d, torch.from_numpy(g['g_codes']).to(DEV))
    _same_planes(masks, du.planes(g, 'g'), 'gt')
    assert np.array_equal(rois.cpu().numpy(), g['g_rois']) and np.array_equal(areas.cpu().numpy(), g['g_areas'])
    masks2, rois2, areas2 = scene.scene_gt_inputs(scene_d, g['g_codes'])
    assert torch.equal(masks2, masks) and np.array_equal(rois2, g['g_rois']) and np.array_equal(areas2, g['g_areas'])
    # a code that matches nothing: area 0 and an invalid roi from the kernel, the reference's IndexError from the host layer
    _, rois3, areas3 = ops.scene_gt_masks(scene_d, torch.from_numpy(g['h_codes']).to(DEV))
    assert areas3.cpu().tolist()[2] == 0 and rois3.cpu().tolist()[2] == [2 ** 31 - 1, 2 ** 31 - 1, 0, 0]
    assert np.array_equal(rois3.cpu().numpy()[:2], g['g_rois'][:2])
    assert str(g['h_error']) == 'IndexError'
    with pytest.raises(IndexError, match='matches no pixel'):
        scene.scene_gt_inputs(scene_d, g['h_codes'])
    # the session: the largest first (main.py:812), metas follow
    ids, metas = [1, 2, 1, 1, 2], [{'tid': k} for k in range(5)]
    image = _frame(70, 110)
    sess = scene.SceneSession.from_scene_gt(geo, du.Camera(90.0, 54.5, 34.5), image, scene_d, g['g_codes'], ids, metas=metas,
                                            image_size=64, mask_size=48)
    sels = g['g_sels']
    assert np.array_equal(sess.detection_sels, sels) and np.array_equal(sess.rois, g['g_rois'][sels])
    assert sess.class_ids == [ids[i] for i in sels] and sess.metas == [metas[i] for i in sels]
    want = torch.from_numpy(du.planes(g, 'g')[sels].astype(np.float32)).to(DEV)
    assert torch.equal(sess.image_masks, want)
    ref = scene.SceneSession(geo, du.Camera(90.0, 54.5, 34.5), image, sess.class_ids, want, g['g_rois'][sels], image_size=64,
                             mask_size=48)
    assert sess.interests == ref.interests and torch.equal(sess.masks, ref.masks)
    with pytest.raises(IndexError):
        scene.SceneSession.from_scene_gt(geo, du.Camera(90.0, 54.5, 34.5), image, scene_d, g['h_codes'], [1, 1, 1], image_size=64,
                                         mask_size=48)
