"""GPU: the geometric edit path -- sdn_scene_cover / sdn_scene_crops / sdn_scene_edit and derender3d.scene.SceneSession.

  * the crops of every fixture case BIT-equal to tests/golden/scene_golden.npz (the reference's PIL statements, executed), both
    ignore pairings, caller-supplied ignore maps; N = 1 and N = 33 (second cover word) against the PIL restatement;
  * sdn_scene_edit bit-equal to the fixture at F = 1 and F = 4;
  * SceneSession at reduced size: F lists in one call = single calls, = oracle/composite_oracle on the same rendered maps,
    reconstruct pastes detector masks, optimize lowers the loss and restores the model's state;
  * SceneSession.edit -> EditSession.render_batch once;
  * no device-to-host copy inside the crop calls and the edit wrapper; error paths."""
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

import scene_util as su  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    return su.load()


def _device_inputs(g, s):
    image = torch.from_numpy(np.ascontiguousarray(g[s + '_image'].transpose(2, 0, 1))).to(DEV)
    masks = torch.from_numpy(g[s + '_image_masks'].astype(np.float32)).to(DEV)
    return image, masks


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got, want), '%s: %d of %d values differ, max |d| %g' % (
        what, int((got != want).sum()), want.size, float(np.abs(got - want).max()))


def test_crops_bit_equal_to_the_fixture_scene_a_both_pairings(gold):
    from derender3d import scene
    g = gold
    image, masks = _device_inputs(g, 'a')
    H, W = image.shape[1:]
    plan = scene.CropPlan(g['a_rois'], H, W, 224, 256, DEV)
    rgbs, crops, cover = scene.image_mask_crops(plan, image, masks, g['a_mean'].tolist(), g['a_std'].tolist())
    _same(rgbs, g['a_rgbs'], 'rgbs')
    _same(crops, g['a_masks'], 'masks')
    logd = torch.from_numpy(g['a_blob_log_depths']).to(DEV)
    droi = torch.from_numpy(g['a_blob_droi_norms']).to(DEV)
    _same(scene.ignore_crops(plan, cover, logd, droi, 'reference'), g['a_ignores'], 'ignores (reference pairing)')
    # the documented alternative: object n with the union of the objects nearer than n
    m = g['a_image_masks'].astype(np.float32)
    maps = su.ignore_maps(m, g['a_order'].tolist(), 'object')
    want = np.stack([su.transform_plane(maps[n, 0], g['a_rois'][n], 255).numpy() for n in range(len(m))])
    assert not np.array_equal(want, g['a_ignores'])
    _same(scene.ignore_crops(plan, cover, logd, droi, 'object'), want, 'ignores (object pairing)')
    # the same maps handed in by the caller (main.py:416)
    supplied = torch.from_numpy(g['a_image_ignores'].astype(np.float32)).to(DEV)
    _same(scene.ignore_crops(plan, cover, image_ignores=supplied), g['a_ignores'], 'ignores (supplied)')


def test_crops_bit_equal_to_the_fixture_scene_b_supplied_ignores(gold):
    from derender3d import scene
    g = gold
    image, masks = _device_inputs(g, 'b')
    plan = scene.CropPlan(g['b_rois'], image.shape[1], image.shape[2], 224, 256, DEV)
    rgbs, crops, cover = scene.image_mask_crops(plan, image, masks, g['b_mean'].tolist(), g['b_std'].tolist())
    _same(rgbs, g['b_rgbs'], 'rgbs')
    _same(crops, g['b_masks'], 'masks')
    supplied = torch.from_numpy(g['b_image_ignores'].astype(np.float32)).to(DEV)
    _same(scene.ignore_crops(plan, cover, image_ignores=supplied), g['b_ignores'], 'ignores')


@pytest.mark.parametrize('n', [1, 33])
def test_one_object_and_a_second_cover_word(n):
    from derender3d import scene
    rng = np.random.default_rng(50 + n)
    H, W, Si, Sm = 57, 83, 40, 48
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rois, masks = [], np.zeros((n, 1, H, W), np.float32)
    for k in range(n):
        y0, x0 = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 12))
        y1, x1 = y0 + int(rng.integers(4, 40)), x0 + int(rng.integers(4, 40))
        rois.append([y0, x0, min(y1, H), min(x1, W)])
        masks[k, 0, y0:y1, x0:x1] = rng.random((min(y1, H) - y0, min(x1, W) - x0)) < 0.7
    rois[0] = [10, 20, 50, 60]        # s = 40 = the image size
    logd = rng.permutation(n).astype(np.float32).reshape(n, 1)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    plan = scene.CropPlan(rois, H, W, Si, Sm, DEV)
    rgbs, crops, cover = scene.image_mask_crops(plan, torch.from_numpy(image.transpose(2, 0, 1).copy()).to(DEV),
                                                torch.from_numpy(masks).to(DEV), mean, std)
    assert tuple(cover.shape) == ((n + 31) // 32, H, W)
    _, mroi, droi = scene.roi_norms_host(rois, su.Camera(90.0, 41.0, 28.0))
    key = logd[:, 0] - np.log(droi.numpy()).sum(1)
    order = np.argsort(key, kind='stable').tolist()
    for pairing in ('reference', 'object'):
        got = scene.ignore_crops(plan, cover, torch.from_numpy(logd).to(DEV), droi.to(DEV), pairing)
        w_rgbs, w_masks, w_ign = su.pil_crops(image, masks, su.ignore_maps(masks, order, pairing), rois, mean, std, Si, Sm)
        _same(got, w_ign, 'ignores (%s), N = %d' % (pairing, n))
    _same(rgbs, w_rgbs, 'rgbs, N = %d' % n)
    _same(crops, w_masks, 'masks, N = %d' % n)


def _edit_case(g, s, lists_idx):
    from derender3d import scene
    cam = su.camera(g, s)
    lists = [su.operation_lists(g, s)[i] for i in lists_idx]
    _, mroi, droi = scene.roi_norms_host(g[s + '_rois'], cam)
    records, _ = scene.edit_records(lists, mroi, cam)
    # the host's float32 log / cos / sin may differ from the fixture host's in the last place: checked to 2 ulp and pinned
    # (scene_util.pin_transcendentals); the kernel's own arithmetic is then compared bit for bit
    return su.pin_transcendentals(records, g, s, lists_idx), mroi, droi


@pytest.mark.parametrize('s,lists_idx', [('a', [0]), ('a', [1]), ('a', [2]), ('a', [3]), ('a', [4]), ('a', [4, 2, 0, 1]), ('a', [1, 2, 3, 4]),
                                         ('b', [0]), ('b', [0, 1])])
def test_scene_edit_bit_equal_to_the_fixture(gold, s, lists_idx):
    from derender3d import scene
    from sdn_hip import ops
    g = gold
    records, mroi, droi = _edit_case(g, s, lists_idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    (rec_d,) = scene.upload_int32([records], DEV)
    th, tr, ld, it = ops.scene_edit(t(g[s + '_blob_theta_deltas']), t(g[s + '_blob_translation2ds']), t(g[s + '_blob_log_depths']),
                                    mroi.to(DEV), droi.to(DEV), t(g[s + '_interests']), rec_d)
    assert tuple(th.shape) == (len(lists_idx), len(mroi), 2) and tuple(ld.shape) == (len(lists_idx), len(mroi), 1)
    for f, i in enumerate(lists_idx):
        q = '%s_edit%d_' % (s, i)
        _same(th[f], g[q + 'theta_deltas'], 'list %d theta' % i)
        _same(tr[f], g[q + 'translation2ds'], 'list %d translation' % i)
        _same(ld[f], g[q + 'log_depths'], 'list %d depth' % i)
        _same(it[f], g[q + 'interests'], 'list %d interests' % i)


# ------------------------------------------------------------------------------------------------ the session, reduced size
H, W, R, FOCAL, U0, V0 = 94, 158, 64, 90.0, 79.0, 47.0
ROIS = [[20, 10, 60, 70], [30, 60, 75, 120], [10, 100, 40, 150], [50, 5, 80, 40]]
CLASS_IDS = [1, 2, 1, 3]          # the last one is not interesting (class)
LISTS = [
    [{'type': 'modify', 'from': {'u': 40, 'v': 40}, 'to': {'u': 60, 'v': 45}, 'zoom': 1.2, 'ry': 0.5}],
    [{'type': 'delete', 'from': {'u': 90, 'v': 52}}],
    [],
]


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


def _scene_inputs(seed=5):
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 256, (3, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    image = torch.from_numpy(np.ascontiguousarray(cell.repeat(8, 1).repeat(8, 2)[:, :H, :W])).to(DEV)
    masks = np.zeros((len(ROIS), 1, H, W), np.float32)
    for n, (y0, x0, y1, x1) in enumerate(ROIS):
        masks[n, 0, y0 + 2:y1 - 2, x0 + 3:x1 - 3] = 1.0
    return image, torch.from_numpy(masks).to(DEV)


def _session(geo, **kw):
    from derender3d import scene
    image, masks = _scene_inputs()
    return scene.SceneSession(geo, su.Camera(FOCAL, U0, V0), image, CLASS_IDS, masks, ROIS, image_size=64, mask_size=48, **kw)


def _frames_equal(a, b, what):
    assert torch.equal(a.inst_u8, b.inst_u8), what + ': instance map'
    assert torch.equal(a.normal_u8, b.normal_u8), what + ': normal map'
    assert torch.equal(a.depth_i32, b.depth_i32), what + ': depth map'
    assert a.json == b.json and a.interests == b.interests, what + ': json / interests'


def test_session_crops_and_interests(geo):
    sess = _session(geo)
    image, masks = _scene_inputs()
    m = masks.cpu().numpy()
    assert sess.interests == [True, True, True, False]
    assert tuple(sess.rgbs.shape) == (4, 3, 64, 64) and tuple(sess.masks.shape) == tuple(sess.ignores.shape) == (4, 1, 48, 48)
    key = (sess.blob['_log_depths'][:, 0] - torch.log(sess.blob['_droi_norms']).sum(1)).cpu().numpy()
    order = np.argsort(key, kind='stable').tolist()
    w_rgbs, w_masks, w_ign = su.pil_crops(image.permute(1, 2, 0).cpu().numpy(), m, su.ignore_maps(m, order), ROIS,
                                          (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), 64, 48)
    _same(sess.rgbs, w_rgbs, 'session rgbs')
    _same(sess.masks, w_masks, 'session masks')
    _same(sess.ignores, w_ign, 'session ignores')
    assert tuple(sess.blob['_roi_norms'].shape) == (4, 4) and '_ffd_coeffs' in sess.blob


def test_edit_of_three_lists_equals_three_calls_and_the_oracle(geo):
    from oracle import composite_oracle as co
    sess = _session(geo)
    frames = sess.edit(LISTS)
    blob = sess.last_blob
    assert len(frames) == 3
    assert frames[1].interests == [True, False, True, False] and 2 not in frames[1].json and 2 in frames[0].json
    assert sess.last_interests.cpu().tolist() == [fr.interests for fr in frames]
    n = len(ROIS)
    cpu = lambda x: x.detach().cpu()    # noqa: E731
    for f, fr in enumerate(frames):
        rows = slice(f * n, (f + 1) * n)
        ref = co.composite_frame(cpu(blob['_masks'][rows]), cpu(blob['_normals'][rows]), cpu(blob['_depth_maps'][rows]),
                                 cpu(blob['_depths'][rows]), cpu(blob['_zooms'][rows]), cpu(blob['_center2ds'][rows]),
                                 torch.tensor(fr.interests), FOCAL, U0, V0, H, W, R)
        for name, a, b in zip(('instance', 'normal', 'depth'), fr.maps, ref[:3]):
            assert torch.equal(a.cpu(), b), 'list %d: composited %s map differs from the oracle' % (f, name)
        assert 4 not in fr.inst_u8.unique().cpu().tolist()          # the non-interesting object is dropped in an edit
    assert len(frames[2].inst_u8.unique()) >= 3
    assert not torch.equal(frames[0].inst_u8, frames[2].inst_u8)    # the modify moved something
    for f, ops_ in enumerate(LISTS):
        (one,) = sess.edit([ops_])
        _frames_equal(one, frames[f], 'list %d alone' % f)


def test_reconstruct_pastes_the_detector_masks_of_other_objects(geo):
    sess = _session(geo)
    fr = sess.reconstruct()
    _, masks = _scene_inputs()
    inst = fr.inst_u8[0]
    assert bool((inst == 4).any())
    assert bool(((inst == 4) <= (masks[3, 0] > 0)).all())
    assert 4 not in fr.json and set(fr.json) == {1, 2, 3}
    (unedited,) = sess.edit([[]])
    keep = masks[3, 0] == 0
    assert torch.equal(unedited.inst_u8[0][keep], inst[keep])


def test_optimize_lowers_the_loss_and_restores_the_model(geo, monkeypatch):
    sess = _session(geo)
    assert not geo.training and geo._force_no_sample is False
    before = sess.blob['_theta_deltas'].clone()
    losses = sess.optimize(3)
    assert len(losses) == 3 and all(np.isfinite(losses))
    print('optimize(3) losses:', losses)
    assert losses[-1] < losses[0]
    assert not geo.training and geo._force_no_sample is False
    assert not torch.equal(before, sess.blob['_theta_deltas']) and not sess.blob['_theta_deltas'].requires_grad
    # an iteration that raises: the model's state is put back as it was found (here: train mode)
    def broken(blob):
        raise RuntimeError('render failed')
    geo.train()
    try:
        with monkeypatch.context() as mp:
            mp.setattr(geo, 'render', broken)
            with pytest.raises(RuntimeError, match='render failed'):
                sess.optimize(1)
        assert geo.training and geo._force_no_sample is False
    finally:
        geo.eval()
    assert sess.edit([[]])[0].inst_u8.shape == (1, H, W)


def test_scene_session_to_edit_session(geo):
    import edit_util as eu
    from edit import EditSession
    from models.pix2pixHD_model import Pix2PixHDModel
    opt = eu.options(24, fineHeight=96)
    torch.manual_seed(31)
    tex = Pix2PixHDModel()
    tex.initialize(opt)
    sess = _session(geo)
    image, _ = _scene_inputs()
    rng = np.random.default_rng(9)
    segm = torch.from_numpy(rng.integers(0, 13, (1, H, W), dtype=np.uint8)).to(DEV)
    source = sess.reconstruct()
    es = EditSession(tex, opt, eu.PARAMS, segm, image, source.inst_u8)
    frames = sess.edit(LISTS)
    out = es.render_batch([(fr.inst_u8, fr.json, fr.normal_u8) for fr in frames], strict=False)
    assert tuple(out.shape) == (3, 3, 96, 160) and bool(torch.isfinite(out).all())
    inst = es.last_inputs['inst']
    assert 2000 not in inst[1].unique().cpu().tolist()              # the deleted object is gone from the generator's input
    assert 2 not in frames[1].inst_u8.unique().cpu().tolist()


def test_no_device_to_host_copy_in_the_crop_calls_and_the_edit_wrapper(gold, monkeypatch):
    """torch.cuda.set_sync_debug_mode('error') raises on a synchronising call where the build supports it; whether or not this
    ROCm build does, .cpu() / .item() / .tolist() on a tensor are made to raise for the duration as well."""
    from derender3d import scene
    from sdn_hip import ops
    g = gold
    image, masks = _device_inputs(g, 'b')
    plan = scene.CropPlan(g['b_rois'], image.shape[1], image.shape[2], 224, 256, DEV)
    logd = torch.from_numpy(g['b_blob_log_depths']).to(DEV)
    droi = torch.from_numpy(g['b_blob_droi_norms']).to(DEV)
    records, mroi, _ = _edit_case(g, 'b', [0, 1])
    (rec_d,) = scene.upload_int32([records], DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    args = (t(g['b_blob_theta_deltas']), t(g['b_blob_translation2ds']), logd, mroi.to(DEV), droi, t(g['b_interests']), rec_d)
    supplied = t(g['b_image_ignores'].astype(np.float32))
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('device-to-host copy')
    was = torch.cuda.get_sync_debug_mode()
    with monkeypatch.context() as mp:
        for name in ('cpu', 'item', 'tolist', 'numpy'):
            mp.setattr(torch.Tensor, name, refuse)
        torch.cuda.set_sync_debug_mode('error')
        try:
            rgbs, crops, cover = scene.image_mask_crops(plan, image, masks)
            ign = scene.ignore_crops(plan, cover, logd, droi, 'reference')
            ign_o = scene.ignore_crops(plan, cover, logd, droi, 'object')
            ign_s = scene.ignore_crops(plan, cover, image_ignores=supplied)
            outs = ops.scene_edit(*args)
        finally:
            torch.cuda.set_sync_debug_mode(was)
    for x in (rgbs, crops, cover, ign, ign_o, ign_s) + tuple(outs):
        assert isinstance(x, torch.Tensor) and x.is_cuda
    _same(ign_s, g['b_ignores'], 'ignores')


def test_error_paths(gold, geo, monkeypatch):
    from derender3d import scene
    from sdn_hip import SdnHipError, ops
    image, masks = _device_inputs(gold, 'b')
    Hb, Wb = image.shape[1:]
    cam = su.Camera(90.0, 44.5, 29.5)
    with pytest.raises(NotImplementedError):
        scene.SceneSession(geo, cam, image.cpu(), [1, 1], masks, gold['b_rois'])
    with pytest.raises(NotImplementedError):
        scene.SceneSession(geo, cam, image, [1, 1], masks.cpu(), gold['b_rois'])
    with pytest.raises(ValueError, match='empty'):
        scene.SceneSession(geo, cam, image, [1, 1], masks, [[10, 5, 10, 45], [20, 40, 45, 85]])
    with pytest.raises(ValueError, match='2 class ids, 1 rois'):
        scene.SceneSession(geo, cam, image, [1, 1], masks, gold['b_rois'][:1])
    with pytest.raises(ValueError, match='masks'):
        scene.SceneSession(geo, cam, image, [1], masks, gold['b_rois'][:1])
    with pytest.raises(ValueError, match='ignore_pairing'):
        scene.SceneSession(geo, cam, image, [1, 1], masks, gold['b_rois'], ignore_pairing='nearest')
    # the C entry refuses an empty roi before anything is launched (the tables here are those of valid rois)
    plan = scene.CropPlan(gold['b_rois'], Hb, Wb, 224, 256, DEV)
    cover = ops.scene_cover(masks)
    bad = gold['b_rois'].copy()
    bad[1, 3] = bad[1, 1]
    with pytest.raises(SdnHipError, match='roi 1'):
        ops.scene_crops(ops.SCENE_MASK, bad, plan.tables, Hb, Wb, 224, 256, cover=cover)
    with pytest.raises(ValueError, match='nearer'):
        ops.scene_crops(ops.SCENE_IGNORE, gold['b_rois'], plan.tables, Hb, Wb, 224, 256, ignore_cover=cover)
    # binary masks are a precondition; SDN_DEBUG_CHECKS=1 verifies it (and makes the call synchronous)
    grey = masks.clone()
    grey[0, 0, 3, 4] = 0.5
    assert tuple(ops.scene_cover(grey).shape) == (1, Hb, Wb)
    monkeypatch.setenv('SDN_DEBUG_CHECKS', '1')
    assert tuple(ops.scene_cover(masks).shape) == (1, Hb, Wb)
    with pytest.raises(SdnHipError, match='neither 0 nor 1'):
        ops.scene_cover(grey)
