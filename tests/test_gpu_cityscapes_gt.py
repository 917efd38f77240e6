"""GPU: the Cityscapes ground-truth source -- sdn_scene_id_stats / sdn_scene_id_planes, derender3d.scene.cityscapes_gt_inputs and
SceneSession.from_cityscapes_gt / Scene2D.from_cityscapes_gt -- against tests/golden/cityscapes_gt_golden.npz (the reference's
statements, executed) and the numpy emulation of tests/cityscapes_util.py.  Every comparison is exact: the kernels are integer
arithmetic and the thresholds are the host's float64.

  * the table and the planes bit-equal to the fixture at K = 1, 3 and 33 cars (37 x 70: odd width, H W no multiple of 4; 64 x
    128: two workgroups; 33 objects: a second cover word);
  * planes, ignore planes and cover words into dirty buffers that start inside a 16-byte quad: everything written, nothing beside;
  * ignore_cover equals ops.scene_cover of the fp32 ignore planes;
  * one seeded 1024 x 2048 frame with 20 cars against the emulation;
  * from_cityscapes_gt equals a SceneSession built from the reference's masks, rois and image_ignores; optimize, edit and
    reconstruct run at this frame size; the 2D baseline's session;
  * the launcher's refusals and the SDN_DEBUG_CHECKS range check (nothing here provokes a device fault)."""
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

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
R = 64


@pytest.fixture(scope='module')
def gold():
    return cu.load()


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


def _maps(g, tag):
    return tuple(torch.from_numpy(a).to(DEV) for a in cu.maps(g, tag))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_planes(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert set(np.unique(got).tolist()) <= {0.0, 1.0}, what + ': values other than 0.0 and 1.0'
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i].astype(np.float32)), '%s: plane %d: %d pixels differ' % (
            what, i, int((got[i] != want[i]).sum()))


def _thresholds(g, tag):
    return np.floor(g[tag + '_percentiles']).astype(np.int32)


@pytest.mark.parametrize('tag', cu.CASES)
def test_table_and_planes_bit_equal_to_the_fixture(gold, tag):
    from derender3d import scene as sc
    from sdn_hip import ops
    g = gold
    scene, disparity = _maps(g, tag)
    table = ops.scene_id_stats(scene, disparity)
    assert table.dtype == torch.int32 and tuple(table.shape) == (1000, 8)
    got = table.cpu().numpy()
    want = cu.stats_emulated(*cu.maps(g, tag))
    j = g[tag + '_ids'] - 26000
    assert np.array_equal(got[j], g[tag + '_stats']), 'rows %s differ' % np.flatnonzero((got[j] != g[tag + '_stats']).any(axis=1))
    assert np.array_equal(got, want)                     # the absent ids too: area 0, the invalid roi
    assert np.array_equal(ops.scene_id_stats(scene, disparity).cpu().numpy(), got)      # the call clears its own workspace
    # all K objects (33: two cover words), thresholds from the table as the host layer computes them
    thr = sc.percentile95_threshold(got[j, 5], got[j, 6], got[j, 7])
    assert np.array_equal(thr, _thresholds(g, tag))
    masks, cover, ignores = ops.scene_id_planes(scene, disparity, _dev(g[tag + '_ids']), _dev(thr), ignore_planes=True)
    _same_planes(masks, cu.planes(g, tag, 'masks'), tag + ' masks')
    _same_planes(ignores, cu.planes(g, tag, 'ignores'), tag + ' ignores')
    assert cover.dtype == torch.int32 and tuple(cover.shape) == ((len(j) + 31) // 32,) + tuple(scene.shape)
    assert np.array_equal(cover.cpu().numpy().view(np.uint32), cu.planes_emulated(*cu.maps(g, tag), g[tag + '_ids'], thr)[2])
    assert torch.equal(cover, ops.scene_cover(ignores))
    # another category: the 24xxx id of the fixture, and one that is absent
    other = ops.scene_id_stats(scene, disparity, category=24).cpu().numpy()
    assert np.array_equal(other, cu.stats_emulated(*cu.maps(g, tag), category=24)) and other[1, 0] == 1
    assert not ops.scene_id_stats(scene, disparity, category=5).cpu().numpy()[:, 0].any()


def test_the_session_inputs_equal_the_reference_selection(gold):
    from derender3d import scene as sc
    g = gold
    for tag in cu.CASES:
        scene, disparity = _maps(g, tag)
        masks, cover, rois, areas, ids, thr = sc.cityscapes_gt_inputs(scene, disparity)
        sels = g[tag + '_sels']
        assert np.array_equal(ids, g[tag + '_ids'][sels]) and np.array_equal(rois, g[tag + '_rois'][sels])
        assert np.array_equal(areas, g[tag + '_areas'][sels]) and np.array_equal(thr, _thresholds(g, tag)[sels])
        assert rois.dtype == areas.dtype == ids.dtype == thr.dtype == np.int32
        _same_planes(masks, cu.planes(g, tag, 'masks')[sels], tag + ' selected masks')
        from sdn_hip import ops
        assert torch.equal(cover, ops.scene_cover(_dev(cu.planes(g, tag, 'ignores')[sels].astype(np.float32))))
    few = sc.cityscapes_gt_inputs(*_maps(g, 'c'), max_objects=3)
    assert np.array_equal(few[4], g['c_ids'][g['c_sels'][:3]]) and tuple(few[0].shape) == (3, 1, 64, 128)
    with pytest.raises(ValueError, match='no object of category 5'):
        sc.cityscapes_gt_inputs(*_maps(g, 'a'), category=5)


def test_planes_into_unaligned_dirty_buffers(gold):
    """every output a view that starts 4, 8 or 12 bytes into an allocation that held 7: every element written, nothing beside"""
    from sdn_hip import check, lib, ptr, stream
    g = gold
    scene, disparity = _maps(g, 'b')
    H, W = scene.shape
    n = 3
    ids, thr = _dev(g['b_ids']), _dev(_thresholds(g, 'b'))
    want_m, want_i, want_c = cu.planes_emulated(*cu.maps(g, 'b'), g['b_ids'], _thresholds(g, 'b'))
    assert (H * W) % 4 != 0
    bufs = [torch.full((n * H * W + 8,), 7.0, device=DEV), torch.full((n * H * W + 8,), 7.0, device=DEV),
            torch.full((H * W + 8,), 7, dtype=torch.int32, device=DEV)]
    views = [bufs[0][1:1 + n * H * W], bufs[1][2:2 + n * H * W], bufs[2][3:3 + H * W]]
    check(lib().sdn_scene_id_planes(ptr(scene), ptr(disparity), ptr(ids), ptr(thr), n, H, W, views[0].data_ptr(), views[2].data_ptr(),
                                    views[1].data_ptr(), stream()))
    _same_planes(views[0].reshape(n, 1, H, W), want_m, 'unaligned masks')
    _same_planes(views[1].reshape(n, 1, H, W), want_i, 'unaligned ignores')
    assert np.array_equal(views[2].cpu().numpy().view(np.uint32).reshape(1, H, W), want_c)
    for buf, off, size in ((bufs[0], 1, n * H * W), (bufs[1], 2, n * H * W), (bufs[2], 3, H * W)):
        assert bool((buf[:off] == 7).all()) and bool((buf[off + size:] == 7).all())
    # masks alone, and cover words alone
    only = torch.full((n * H * W + 8,), 7.0, device=DEV)
    check(lib().sdn_scene_id_planes(ptr(scene), ptr(disparity), ptr(ids), ptr(thr), n, H, W, only[3:].data_ptr(), None, None, stream()))
    _same_planes(only[3:3 + n * H * W].reshape(n, 1, H, W), want_m, 'masks alone')
    assert bool((only[:3] == 7).all()) and bool((only[3 + n * H * W:] == 7).all())
    words = torch.full((H * W + 8,), 7, dtype=torch.int32, device=DEV)
    check(lib().sdn_scene_id_planes(ptr(scene), ptr(disparity), ptr(ids), ptr(thr), n, H, W, None, words[1:].data_ptr(), None, stream()))
    assert np.array_equal(words[1:1 + H * W].cpu().numpy().view(np.uint32).reshape(1, H, W), want_c)
    assert int(words[0]) == 7 and bool((words[1 + H * W:] == 7).all())


@pytest.fixture(scope='module')
def big():
    scene, disparity = cu.big_frame()
    return scene, disparity, cu.stats_emulated(scene, disparity)


def test_a_full_size_frame_equals_the_emulation(big):
    """1024 x 2048, 20 cars, the largest 86 450 pixels: one launch chain"""
    from derender3d import scene as sc
    from sdn_hip import ops
    scene, disparity, want = big
    assert (want[:, 0] > 0).sum() == 20 and want[:, 0].max() > 80000 and want[999, 0] > 0
    scene_d, disparity_d = _dev(scene), _dev(disparity)
    got = ops.scene_id_stats(scene_d, disparity_d).cpu().numpy()
    assert np.array_equal(got, want), 'rows %s differ' % np.flatnonzero((got != want).any(axis=1))
    masks, cover, rois, areas, ids, thr = sc.cityscapes_gt_inputs(scene_d, disparity_d)
    sels, ids_w, rois_w, areas_w, thr_w = cu.select_emulated(want)
    assert len(ids) == 16 and np.array_equal(ids, ids_w) and np.array_equal(rois, rois_w) and np.array_equal(areas, areas_w)
    assert np.array_equal(thr, thr_w)
    # the thresholds are the percentiles of a sort
    for k in (0, 7, 15):
        d = disparity[scene == ids[k]]
        assert thr[k] == int(np.floor(np.percentile(d[d != 0], 95)))
    want_c = torch.zeros_like(cover[0])
    for k in range(16):
        assert torch.equal(masks[k, 0], (scene_d == int(ids[k])).float()), 'mask %d' % k
        want_c |= (disparity_d > int(thr[k])).int() << k
    assert torch.equal(cover[0], want_c)


def _frame(H, W, seed=5):
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 256, (3, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(cell.repeat(8, 1).repeat(8, 2)[:, :H, :W])).to(DEV)


CAMERA = cu.Camera(90.0, 63.5, 31.5)


def test_from_cityscapes_gt_equals_a_session_of_the_reference_arrays(gold, geo):
    from derender3d import scene as sc
    g = gold
    H, W = 64, 128
    image = _frame(H, W)
    scene, disparity = _maps(g, 'c')
    sess = sc.SceneSession.from_cityscapes_gt(geo, CAMERA, image, scene, disparity, image_size=64, mask_size=48)
    sels = g['c_sels']
    assert np.array_equal(sess.detection_sels, sels) and np.array_equal(sess.rois, g['c_rois'][sels])
    assert np.array_equal(sess.instance_ids, g['c_ids'][sels]) and np.array_equal(sess.mask_areas, g['c_areas'][sels])
    assert np.array_equal(sess.ignore_thresholds, _thresholds(g, 'c')[sels]) and sess.class_ids == [1] * 16
    ref_masks = _dev(cu.planes(g, 'c', 'masks')[sels].astype(np.float32))
    ref_ignores = _dev(cu.planes(g, 'c', 'ignores')[sels].astype(np.float32))
    ref = sc.SceneSession(geo, CAMERA, image, [1] * 16, ref_masks, g['c_rois'][sels], image_ignores=ref_ignores, image_size=64,
                          mask_size=48)
    assert torch.equal(sess.image_masks, ref_masks)
    assert torch.equal(sess.rgbs, ref.rgbs) and torch.equal(sess.masks, ref.masks) and torch.equal(sess.ignores, ref.ignores)
    assert sess.interests == ref.interests and any(sess.interests) and not all(sess.interests)
    assert 0.0 < float(sess.ignores.mean()) < 1.0
    # the keyword alone, on the constructor: cover words in the place of the planes
    from sdn_hip import ops
    kw = sc.SceneSession(geo, CAMERA, image, [1] * 16, ref_masks, g['c_rois'][sels], ignore_cover=ops.scene_cover(ref_ignores),
                         image_size=64, mask_size=48)
    assert torch.equal(kw.ignores, ref.ignores)
    with pytest.raises(ValueError, match='ignore_cover must be int32'):
        sc.SceneSession(geo, CAMERA, image, [1] * 16, ref_masks, g['c_rois'][sels], ignore_cover=ops.scene_cover(ref_ignores[:, :, :32]),
                        image_size=64, mask_size=48)


def test_optimize_edit_and_reconstruct_at_this_frame_size(gold, geo):
    from derender3d import scene as sc
    from derender3d import scene2d
    g = gold
    H, W = 64, 128
    scene, disparity = _maps(g, 'c')
    sess = sc.SceneSession.from_cityscapes_gt(geo, CAMERA, _frame(H, W), scene, disparity, image_size=64, mask_size=48)
    losses = sess.optimize(2)
    assert len(losses) == 2 and all(np.isfinite(losses))
    big = [k for k, keep in enumerate(sess.interests) if keep]
    y0, x0, y1, x1 = sess.rois[big[0]].tolist()
    u, v = (x0 + x1) / 2, (y0 + y1) / 2
    frames = sess.edit([[], [{'type': 'modify', 'from': {'u': u, 'v': v}, 'to': {'u': u + 10, 'v': v + 3}, 'zoom': 1.2, 'ry': 0.4}],
                        [{'type': 'delete', 'from': {'u': u, 'v': v}}]])
    assert len(frames) == 3
    for fr in frames:
        assert tuple(fr.inst_u8.shape) == (1, H, W) and tuple(fr.normal_u8.shape) == (3, H, W) and tuple(fr.depth_i32.shape) == (1, H, W)
    assert frames[0].interests == sess.interests and frames[2].interests[big[0]] is False
    assert set(frames[0].inst_u8.unique().cpu().tolist()) - {0} <= {k + 1 for k in big}
    assert (big[0] + 1) not in frames[2].inst_u8.unique().cpu().tolist()
    rec = sess.reconstruct()
    assert tuple(rec.inst_u8.shape) == (1, H, W) and len(rec.inst_u8.unique()) > len(big) + 1     # the small cars' masks are pasted
    # the 2D baseline of the same ground truth: masks and rois only
    s2 = scene2d.Scene2D.from_cityscapes_gt(None, scene, disparity)
    assert np.array_equal(s2.instance_ids, sess.instance_ids) and np.array_equal(s2.rois, sess.rois) and s2.class_ids == [1] * 16
    assert torch.equal(s2.cover, sess.cover) and torch.equal(s2.image_masks, sess.image_masks)
    painted = s2.reference_map()
    assert tuple(painted.shape) == (1, H, W) and torch.equal(painted[0] > 0, sess.image_masks.sum(dim=0)[0] > 0)
    (f2,) = s2.edit([[{'type': 'delete', 'from': {'u': u, 'v': v}}]])
    assert tuple(f2.inst_u8.shape) == (1, H, W) and f2.interests[big[0]] is False


def test_the_launcher_refuses_what_it_cannot_serve(gold, monkeypatch):
    from sdn_hip import SdnHipError, lib, ops, ptr, stream
    g = gold
    scene, disparity = _maps(g, 'b')
    ids, thr = _dev(g['b_ids']), _dev(_thresholds(g, 'b'))
    out = torch.empty(3, 1, 37, 70, device=DEV)
    L = lib()
    assert L.sdn_scene_id_planes(ptr(scene), ptr(disparity), ptr(ids), ptr(thr), 0, 37, 70, ptr(out), None, None, stream()) == -1
    assert b'bad sizes' in L.sdn_last_error()
    assert L.sdn_scene_id_planes(ptr(scene), ptr(disparity), ptr(ids), ptr(thr), 3, 37, 70, None, None, ptr(out), stream()) == -1
    assert b'neither' in L.sdn_last_error()
    assert L.sdn_scene_id_planes(None, ptr(disparity), ptr(ids), ptr(thr), 3, 37, 70, ptr(out), None, None, stream()) == -1
    assert b'null pointer' in L.sdn_last_error()
    with pytest.raises(ValueError, match='neither'):
        ops.scene_id_planes(scene, disparity, ids, thr, planes=False, cover=False)
    with pytest.raises(ValueError, match='disparity must be'):
        ops.scene_id_stats(scene, disparity[:, :8])
    with pytest.raises(TypeError):
        ops.scene_id_stats(scene.long(), disparity)
    with pytest.raises(ValueError, match='ids and thr'):
        ops.scene_id_planes(scene, disparity, ids, thr[:2])
    # the 16-bit precondition is verified only under SDN_DEBUG_CHECKS=1
    wide = disparity.clone()
    wide[0, 0] = 70000
    wide[1, 1] = -1
    assert tuple(ops.scene_id_stats(scene, wide).shape) == (1000, 8)
    monkeypatch.setenv('SDN_DEBUG_CHECKS', '1')
    assert np.array_equal(ops.scene_id_stats(scene, disparity).cpu().numpy(), cu.stats_emulated(*cu.maps(g, 'b')))
    with pytest.raises(SdnHipError, match='2 disparity values lie outside'):
        ops.scene_id_stats(scene, wide)
