"""GPU: the 2D / 2D+ edit baselines -- sdn_scene_paint2d and derender3d.scene2d.Scene2D -- against Pillow itself, executed
here (tests/scene2d_util.py restates geometric/scripts/main.py:293-312 with PIL.Image and torch CPU tensors).  Every
comparison is bit equality.

  * F = 4 operation lists on a 40 x 96 frame with N = 3 overlapping objects (no-op; zoom 0.4 with 7 taps a pass; zoom 1.7
    clipped at the left / top and at the right / bottom border; a delete plus an object moved wholly outside), in one call
    and one by one; use_ry with ry = 1.0; N = 33 (second cover word, the highest index wins); N = 1; reference_map;
  * SceneSession.edit_2d = Scene2D.edit; Scene2D.from_scene_gt on the detections fixture;
  * Scene2D.edit -> EditSession.render_batch once, on a generator without pose and normal features;
  * no device-to-host copy inside edit / reference_map; error paths."""
import json
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

import scene2d_util as s2  # noqa: E402
from derender3d import scene2d  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

H, W = 40, 96
ROIS = [[4, 6, 30, 50], [10, 30, 38, 80], [2, 60, 25, 95]]
CLASS_IDS = [1, 2, 1]
LEFT_TOP = {'type': 'modify', 'from': {'u': 28, 'v': 17}, 'to': {'u': 5, 'v': 3}, 'zoom': 1.7, 'ry': 0.4}
RIGHT_BOTTOM = {'type': 'modify', 'from': {'u': 78, 'v': 13}, 'to': {'u': 92, 'v': 36}, 'zoom': 1.7, 'ry': 0.2}
SHRINK = {'type': 'modify', 'from': {'u': 55, 'v': 24}, 'to': {'u': 50.5, 'v': 20.25}, 'zoom': 0.4, 'ry': 1.0}
AWAY = {'type': 'modify', 'from': {'u': 78, 'v': 13}, 'to': {'u': 400, 'v': -200}, 'zoom': 1.3, 'ry': -0.7}
DELETE = {'type': 'delete', 'from': {'u': 54, 'v': 25}}
LISTS = [[], [SHRINK], [LEFT_TOP, RIGHT_BOTTOM], [DELETE, AWAY]]


def _masks(rois, h=H, w=W, seed=3, p=0.7):
    rng = np.random.default_rng(seed)
    m = np.zeros((len(rois), 1, h, w), np.float32)
    for n, (y0, x0, y1, x1) in enumerate(rois):
        m[n, 0, y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < p
    return m


@pytest.fixture(scope='module')
def three():
    masks = _masks(ROIS)
    masks[0, 0, 35, 90] = 1.0            # outside its roi: the reference map shows it, an edit never does
    want = {ry: [s2.baseline(CLASS_IDS, masks, ROIS, ops_, ry) for ops_ in LISTS] for ry in (False, True)}
    return masks, scene2d.Scene2D(CLASS_IDS, torch.from_numpy(masks).to(DEV), ROIS, H, W), want


def _check(fr, want, what):
    inst, js, keep = want
    got = fr.inst_u8.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == inst.shape, what
    assert np.array_equal(got, inst), '%s: %d of %d pixels differ' % (what, int((got != inst).sum()), inst.size)
    assert fr.json == js and fr.interests == keep, what


@pytest.mark.parametrize('use_ry', [False, True])
def test_four_lists_in_one_call_and_one_by_one(three, use_ry):
    masks, sc, want = three
    frames = sc.edit(LISTS, use_ry)
    assert len(frames) == 4 and all(fr.inst_u8.is_cuda and tuple(fr.inst_u8.shape) == (1, H, W) for fr in frames)
    for f, fr in enumerate(frames):
        _check(fr, want[use_ry][f], 'list %d of 4' % f)
    for f, ops_ in enumerate(LISTS):
        (one,) = sc.edit([ops_], use_ry)
        _check(one, want[use_ry][f], 'list %d alone' % f)
        assert torch.equal(one.inst_u8, frames[f].inst_u8)
    # the cases hold what they are for
    noop, shrunk, clipped, gone = (w[0] for w in want[use_ry])
    assert noop[0, 35, 90] == 0 and len(np.unique(noop)) == 4
    assert not np.array_equal(shrunk, noop) and (shrunk == 2).sum() < (noop == 2).sum() // 2
    assert (clipped[0, 0] == 1).any() and (clipped[0, :, 0] == 1).any()                  # clipped at the top and the left border
    assert (clipped[0, H - 1] == 3).any() and (clipped[0, :, W - 1] == 3).any()          # and at the bottom and the right
    assert 2 not in gone and 3 not in gone and 2 not in frames[3].json and 3 in frames[3].json
    assert frames[3].interests == [True, False, True]


def test_use_ry_scales_rows_and_columns_differently(three):
    masks, sc, _ = three
    ops_ = [{'type': 'modify', 'from': {'u': 28, 'v': 17}, 'to': {'u': 30, 'v': 18}, 'zoom': 1.3, 'ry': 1.0}]
    (plus,) = sc.edit([ops_], use_ry=True)
    (flat,) = sc.edit([ops_], use_ry=False)
    _check(plus, s2.baseline(CLASS_IDS, masks, ROIS, ops_, True), '2D+')
    _check(flat, s2.baseline(CLASS_IDS, masks, ROIS, ops_, False), '2D')
    bx = s2.boxes(*s2.geometry(ROIS, ops_, True)[:2])[0]
    assert bx[:2] == (33, 30)                                     # 26 x 44 by 1.3 and by 1.3 cos(1.0)
    assert not torch.equal(plus.inst_u8, flat.inst_u8)


def test_reference_map(three):
    masks, sc, _ = three
    got = sc.reference_map()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, H, W)
    want = s2.reference_map(masks)
    assert np.array_equal(got.cpu().numpy(), want) and want[0, 35, 90] == 1


def test_thirty_three_objects_the_highest_index_wins():
    rng = np.random.default_rng(33)
    rois = []
    for k in range(33):
        y0, x0 = int(rng.integers(0, H - 9)), int(rng.integers(0, W - 11))
        rois.append([y0, x0, y0 + int(rng.integers(2, 9)), x0 + int(rng.integers(2, 11))])
    rois[32] = list(rois[0])                                      # object 32 lies on object 0
    rois[31] = [rois[1][0], rois[1][1], rois[1][2], rois[1][3]]
    masks = _masks(rois, seed=34, p=0.8)
    masks[0, 0, rois[0][0]:rois[0][2], rois[0][1]:rois[0][3]] = 1.0
    masks[32] = masks[0]
    ids = [1 + k % 2 for k in range(33)]
    sc = scene2d.Scene2D(ids, torch.from_numpy(masks).to(DEV), rois)
    assert tuple(sc.cover.shape) == (2, H, W)
    cy, cx = (rois[31][0] + rois[31][2]) / 2.0, (rois[31][1] + rois[31][3]) / 2.0
    lists = [[], [{'type': 'modify', 'from': {'u': cx, 'v': cy}, 'to': {'u': cx + 3, 'v': cy - 2}, 'zoom': 2.0, 'ry': 0.3},
                  {'type': 'delete', 'from': {'u': (rois[0][1] + rois[0][3]) / 2.0, 'v': (rois[0][0] + rois[0][2]) / 2.0}}]]
    frames = sc.edit(lists)
    for f, fr in enumerate(frames):
        _check(fr, s2.baseline(ids, masks, rois, lists[f]), 'N = 33, list %d' % f)
    y, x = rois[0][0], rois[0][1]
    assert int(frames[0].inst_u8[0, y, x]) == 33                  # not 1: index-order painting leaves the highest on top
    # the delete is matched to object 0 (argmin takes the first of two equal centres): object 32 still covers it
    assert frames[1].interests[0] is False and int(frames[1].inst_u8[0, y, x]) == 33
    assert np.array_equal(sc.reference_map().cpu().numpy(), s2.reference_map(masks))


def test_one_object():
    rois = [[5, 7, 33, 61]]
    masks = _masks(rois, seed=8)
    sc = scene2d.Scene2D([2], torch.from_numpy(masks).to(DEV), rois)
    lists = [[], [{'type': 'modify', 'from': {'u': 0, 'v': 0}, 'to': {'u': -9, 'v': 4}, 'zoom': 0.55, 'ry': 0.0}],
             [{'type': 'delete', 'from': {'u': 3, 'v': 3}}, {'type': 'modify', 'from': {'u': 30, 'v': 30}, 'to': {}, 'zoom': 3.0, 'ry': 0.0}]]
    for f, fr in enumerate(sc.edit(lists)):
        _check(fr, s2.baseline([2], masks, rois, lists[f]), 'N = 1, list %d' % f)
    assert np.array_equal(sc.reference_map().cpu().numpy(), s2.reference_map(masks))


# ------------------------------------------------------------------------------------------------ with the 3D session
SH, SW, R = 94, 158, 64
SROIS = [[20, 10, 60, 70], [30, 60, 75, 120], [10, 100, 40, 150], [50, 5, 80, 40]]
SIDS = [1, 2, 1, 3]
SLISTS = [
    [{'type': 'modify', 'from': {'u': 40, 'v': 40}, 'to': {'u': 60, 'v': 45}, 'zoom': 1.2, 'ry': 0.5}],
    [{'type': 'delete', 'from': {'u': 90, 'v': 52}}],
    [],
]


def _scene_inputs(seed=5):
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 256, (3, (SH + 7) // 8, (SW + 7) // 8), dtype=np.uint8)
    image = torch.from_numpy(np.ascontiguousarray(cell.repeat(8, 1).repeat(8, 2)[:, :SH, :SW])).to(DEV)
    masks = np.zeros((len(SROIS), 1, SH, SW), np.float32)
    for n, (y0, x0, y1, x1) in enumerate(SROIS):
        masks[n, 0, y0 + 2:y1 - 2, x0 + 3:x1 - 3] = 1.0
    return image, masks


def test_scene_session_edit_2d_equals_scene2d():
    import scene_util as su
    from derender3d import TargetType, scene
    from derender3d.models import Derenderer3d, ShapenetObj
    from sdn_hip import synth
    objs = []
    for k in range(8):
        v, f = synth.car_like(600, seed=300 + k)
        objs.append(ShapenetObj(vertices=v[:, [2, 1, 0]] * np.asarray([-1, 1, 1], np.float32), faces=f))
    torch.manual_seed(21)
    geo = Derenderer3d(mode=TargetType.extend, image_size=64, render_size=R, objs=objs).to(DEV).eval()
    image, masks = _scene_inputs()
    masks_d = torch.from_numpy(masks).to(DEV)
    sess = scene.SceneSession(geo, su.Camera(90.0, 79.0, 47.0), image, SIDS, masks_d, SROIS, image_size=64, mask_size=48)
    sc = scene2d.Scene2D(SIDS, masks_d, SROIS)
    assert sess.interests == [True, True, True, False]
    for use_ry in (False, True):
        a, b = sess.edit_2d(SLISTS, use_ry), sc.edit(SLISTS, use_ry)
        for f, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x.inst_u8, y.inst_u8) and x.json == y.json and x.interests == y.interests
            _check(x, s2.baseline(SIDS, masks, SROIS, SLISTS[f], use_ry), 'session list %d' % f)
        assert 4 in a[2].json and bool((a[2].inst_u8 == 4).any())          # every object is interesting in the 2D baselines


def test_from_scene_gt_on_the_fixture():
    import detections_util as du
    g = du.load()
    scene_d = torch.from_numpy(g['g_scene']).to(DEV)
    ids, metas = [1, 2, 1, 1, 2], [{'tid': k} for k in range(5)]
    sc = scene2d.Scene2D.from_scene_gt(None, scene_d, g['g_codes'], ids, metas=metas)
    sels = g['g_sels']
    planes = du.planes(g, 'g')[sels].astype(np.float32)
    rois = g['g_rois'][sels]
    assert np.array_equal(sc.detection_sels, sels) and np.array_equal(sc.rois, rois)
    assert sc.class_ids == [ids[i] for i in sels] and sc.metas == [metas[i] for i in sels]
    assert torch.equal(sc.image_masks, torch.from_numpy(planes).to(DEV))
    assert np.array_equal(sc.reference_map().cpu().numpy(), s2.reference_map(planes))
    y0, x0, y1, x1 = [int(v) for v in rois[0]]
    u, v = (x0 + x1) / 2.0, (y0 + y1) / 2.0
    lists = [[], [{'type': 'modify', 'from': {'u': u, 'v': v}, 'to': {'u': u - 7, 'v': v + 4}, 'zoom': 0.8, 'ry': 0.6}]]
    for use_ry in (False, True):
        for f, fr in enumerate(sc.edit(lists, use_ry)):
            _check(fr, s2.baseline(sc.class_ids, planes, rois, lists[f], use_ry), 'gt list %d' % f)
    with pytest.raises(IndexError, match='matches no pixel'):
        scene2d.Scene2D.from_scene_gt(None, scene_d, g['h_codes'], [1, 1, 1])


def test_scene2d_to_edit_session(tmp_path):
    """The 2D baselines condition a generator built without pose and normal features: the JSON carries no alpha."""
    import edit_util as eu
    from edit import EditSession
    from models.pix2pixHD_model import Pix2PixHDModel
    opt = eu.options(0, feat_pose='', feat_normal='', fineHeight=96)
    torch.manual_seed(31)
    tex = Pix2PixHDModel()
    tex.initialize(opt)
    image, masks = _scene_inputs()
    ids = [1, 2, 1]
    sc = scene2d.Scene2D(ids, torch.from_numpy(masks[:3]).to(DEV), SROIS[:3])
    rng = np.random.default_rng(9)
    segm = torch.from_numpy(rng.integers(0, 13, (1, SH, SW), dtype=np.uint8)).to(DEV)
    es = EditSession(tex, opt, eu.PARAMS, segm, image, sc.reference_map())
    frames = sc.edit([SLISTS[0], []])
    assert all('alpha' not in rec for fr in frames for rec in fr.json.values())
    out = es.render_batch([(fr.inst_u8, fr.json, None) for fr in frames])
    assert tuple(out.shape) == (2, 3, 96, 160) and bool(torch.isfinite(out).all())
    assert es.last_missing == [0, 0]
    # the code follows the object: object 1 moved and grew; its new pixels carry its source row of the code table
    code_ids, means = es.codes
    row = means[code_ids.cpu().tolist().index(1000)]
    inst, feat = es.last_inputs['inst'], es.last_inputs['feat']
    moved, stayed = inst[0, 0] == 1000, inst[1, 0] == 1000
    assert int(moved.sum()) > 100 and not torch.equal(moved, stayed)
    assert torch.equal(stayed, es.base_item['inst'][0] == 1000)
    assert torch.equal(feat[0][:, moved], row[:, None].expand(-1, int(moved.sum())))
    # a model with pose bins still refuses a record without alpha
    from data import assemble as asm
    with pytest.raises(KeyError, match='alpha'):
        asm.edit_tables(eu.options(24), frames[0].json)
    # the wire format on disk
    frames[0].write(str(tmp_path), '00001')
    import PIL.Image
    assert np.array_equal(np.array(PIL.Image.open(os.path.join(str(tmp_path), '00001.png'))), frames[0].inst_u8[0].cpu().numpy())
    assert json.load(open(os.path.join(str(tmp_path), '00001.json'))) == {str(k): v for k, v in frames[0].json.items()}


def test_no_device_to_host_copy_in_edit_and_reference_map(three, monkeypatch):
    """torch.cuda.set_sync_debug_mode('error') raises on a synchronising call where the build supports it; whether or not this
    ROCm build does, .cpu() / .item() / .tolist() / .numpy() on a tensor are made to raise for the duration as well."""
    masks, sc, want = three
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('device-to-host copy')
    was = torch.cuda.get_sync_debug_mode()
    with monkeypatch.context() as mp:
        for name in ('cpu', 'item', 'tolist', 'numpy'):
            mp.setattr(torch.Tensor, name, refuse)
        torch.cuda.set_sync_debug_mode('error')
        try:
            frames = sc.edit(LISTS)
            plus = sc.edit(LISTS[1:3], use_ry=True)
            ref = sc.reference_map()
        finally:
            torch.cuda.set_sync_debug_mode(was)
    for f, fr in enumerate(frames):
        _check(fr, want[False][f], 'list %d' % f)
    for f, fr in enumerate(plus):
        _check(fr, want[True][1 + f], '2D+ list %d' % (1 + f))
    assert np.array_equal(ref.cpu().numpy(), s2.reference_map(masks))


def test_error_paths(three):
    from sdn_hip import SdnHipError, ops
    masks, sc, _ = three
    cpu = torch.from_numpy(masks)
    with pytest.raises(NotImplementedError):
        scene2d.Scene2D(CLASS_IDS, cpu, ROIS)
    with pytest.raises(NotImplementedError):
        scene2d.Scene2D.from_cover(CLASS_IDS, sc.cover.cpu(), ROIS)
    with pytest.raises(NotImplementedError):
        ops.scene_paint2d(sc.cover.cpu(), 3)
    with pytest.raises(NotImplementedError):
        scene2d.Scene2D.from_scene_gt(None, torch.zeros(8, 8, 3, dtype=torch.uint8), [[0, 0, 0]], [1])
    with pytest.raises(ValueError, match='is empty'):
        scene2d.Scene2D(CLASS_IDS, sc.image_masks, [ROIS[0], [10, 30, 10, 80], ROIS[2]])
    with pytest.raises(ValueError, match='3 class ids, 2 rois'):
        scene2d.Scene2D(CLASS_IDS, sc.image_masks, ROIS[:2])
    with pytest.raises(ValueError, match='height / width'):
        scene2d.Scene2D(CLASS_IDS, sc.image_masks, ROIS, H, W + 1)
    with pytest.raises(ValueError, match='no operation lists'):
        sc.edit([])
    flat = [{'type': 'modify', 'from': {'u': 28, 'v': 17}, 'to': {'u': 28, 'v': 17}, 'zoom': 0.03, 'ry': 0.0}]
    with pytest.raises(ValueError, match='frame 1 object 0'):
        sc.edit([[], flat])
    # the C entry validates the host copy of the records before anything is launched
    mrois, drois, keep, _ = scene2d.edit_geometry(ROIS, LISTS[1])
    rec, bounds, kk8 = scene2d.paint_tables(ROIS, [scene2d.paste_boxes(mrois, drois)], [keep], H, W)
    from derender3d import scene
    tables = scene.upload_int32([rec, bounds, kk8], DEV)
    assert tuple(ops.scene_paint2d(sc.cover, 3, rec, tables).shape) == (1, 1, H, W)
    bad = rec.copy()
    bad[0, 2, 4] = W                                              # a window that leaves the frame
    with pytest.raises(SdnHipError, match='frame 0 object 2'):
        ops.scene_paint2d(sc.cover, 3, bad, tables)
    bad = rec.copy()
    bad[0, 1, 9] = bounds.shape[0]                                # a table beyond the pool
    with pytest.raises(SdnHipError, match='does not fit'):
        ops.scene_paint2d(sc.cover, 3, bad, tables)
    bad = rec.copy()
    bad[0, 0, 5] = 0
    with pytest.raises(SdnHipError, match='output size'):
        ops.scene_paint2d(sc.cover, 3, bad, tables)
    with pytest.raises(ValueError, match='objects need'):
        ops.scene_paint2d(sc.cover, 33, rec, tables)
