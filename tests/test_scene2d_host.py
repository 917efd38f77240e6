"""CPU: the host half of the 2D / 2D+ baselines (derender3d/scene2d.py) against Pillow itself and the float32 restatement
of geometric/scripts/main.py:244-312 in tests/scene2d_util.py.  Every comparison is bit equality.

  * resample_u8_rect_numpy (the per-axis use of compositing.resample_tables / fixed_point) = PIL.Image.resize on seeded
    random 0 / 255 masks: shrink and enlarge on each axis independently, one axis unchanged, 1-pixel sides;
  * matching, delete, modify and use_ry geometry = the restatement: more operations than objects and fewer, negative paste
    corners, a centre pushed off the frame;
  * the host tables, evaluated with the kernel's arithmetic in numpy, paint what PIL paints;
  * a zero output size and an empty roi raise ValueError."""
import os
import sys

import numpy as np
import PIL.Image
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scene2d_util as s2  # noqa: E402
from derender3d import scene2d  # noqa: E402

H, W = 40, 96
ROIS = [[4, 6, 30, 50], [10, 30, 38, 80], [2, 60, 25, 95]]
CLASS_IDS = [1, 2, 1]


def _masks(rois=ROIS, seed=3, p=0.7):
    rng = np.random.default_rng(seed)
    m = np.zeros((len(rois), 1, H, W), np.float32)
    for n, (y0, x0, y1, x1) in enumerate(rois):
        m[n, 0, y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < p
    return m


# (h, w, out_h, out_w): both shrink (ksize > 3), both enlarge, mixed either way, one axis unchanged, 1-pixel sides
SIZES = [(26, 44, 10, 17), (13, 9, 30, 31), (26, 9, 7, 40), (7, 44, 39, 11), (20, 33, 20, 12), (20, 33, 45, 33), (20, 33, 20, 33),
         (1, 1, 5, 7), (1, 17, 1, 40), (23, 1, 9, 1), (19, 27, 1, 1), (1, 30, 12, 1), (39, 38, 69, 3), (5, 6, 4, 7)]


@pytest.mark.parametrize('h,w,oh,ow', SIZES)
def test_rect_resample_equals_pil(h, w, oh, ow):
    rng = np.random.default_rng(1000 * h + w)
    near = 0
    for _ in range(6):
        img = ((rng.random((h, w)) < 0.5) * 255).astype(np.uint8)
        want = np.array(PIL.Image.fromarray(img).resize((ow, oh), PIL.Image.BILINEAR))
        got = scene2d.resample_u8_rect_numpy(img, oh, ow)
        assert got.dtype == np.uint8 and got.shape == (oh, ow)
        assert np.array_equal(got, want), '%d x %d -> %d x %d: %d pixels differ' % (h, w, oh, ow, int((got != want).sum()))
        near += int(((want == 127) | (want == 128)).sum())
    print('%d x %d -> %d x %d: %d output pixels at 127 / 128' % (h, w, oh, ow, near))


def test_rect_resample_refuses_an_empty_output():
    with pytest.raises(ValueError, match='> 0'):
        scene2d.resample_u8_rect_numpy(np.zeros((4, 4), np.uint8), 0, 3)


MOVE = {'type': 'modify', 'from': {'u': 28, 'v': 17}, 'to': {'u': 5, 'v': 3}, 'zoom': 1.7, 'ry': 0.4}
SHRINK = {'type': 'modify', 'from': {'u': 55, 'v': 24}, 'to': {'u': 50.5, 'v': 20.25}, 'zoom': 0.4, 'ry': 1.0}
AWAY = {'type': 'modify', 'from': {'u': 78, 'v': 13}, 'to': {'u': 400, 'v': -200}, 'zoom': 1.3, 'ry': -0.7}
DELETE = {'type': 'delete', 'from': {'u': 54, 'v': 25}}
NO_TO = {'type': 'modify', 'from': {'u': 76, 'v': 12}, 'to': {}, 'zoom': 0.77, 'ry': 0.5}
OTHER = {'type': 'recolour', 'from': {'u': 28, 'v': 17}}
LISTS = [
    [],
    [MOVE],
    [SHRINK, AWAY],
    [DELETE, MOVE, NO_TO],
    [MOVE, SHRINK, AWAY, DELETE, NO_TO],          # more operations than objects: every object takes its nearest operation
    [MOVE, MOVE],                                 # two operations on one object: the second reads what the first left
    [OTHER, DELETE],
]


@pytest.mark.parametrize('use_ry', [False, True])
@pytest.mark.parametrize('k', range(len(LISTS)))
def test_geometry_equals_the_restatement(k, use_ry):
    ops_ = LISTS[k]
    mrois, drois, keep, pairs = scene2d.edit_geometry(ROIS, ops_, use_ry)
    centre, extent, want_keep = s2.geometry(ROIS, ops_, use_ry)
    assert mrois.dtype == torch.float32 and drois.dtype == torch.float32
    assert torch.equal(mrois, centre) and torch.equal(drois, extent) and keep == want_keep
    assert scene2d.paste_boxes(mrois, drois) == s2.boxes(centre, extent)
    if len(ops_) > len(ROIS):
        assert [p[0] for p in pairs] == list(range(len(ROIS)))
    else:
        assert [p[1] for p in pairs] == list(range(len(ops_)))


def test_the_cases_hold_what_they_are_for():
    b = s2.boxes(*s2.geometry(ROIS, [MOVE])[:2])
    assert b[0][2] < 0 and b[0][3] < 0                                   # negative paste corner
    c, e, _ = s2.geometry(ROIS, [SHRINK, AWAY])
    assert float(c[2, 0]) < 0 and float(c[2, 1]) > W                     # a centre pushed off the frame
    assert s2.boxes(c, e)[1][:2] == (11, 20)                             # 28 x 50 shrunk: 7 taps a pass
    _, e_ry, _ = s2.geometry(ROIS, [SHRINK], use_ry=True)
    assert int(e_ry[1, 1]) == 10 and int(e_ry[1, 0]) == 11               # cos(1.0) on the columns only
    assert s2.geometry(ROIS, [DELETE])[2] == [True, False, True]
    _, _, keep, pairs = scene2d.edit_geometry(ROIS, LISTS[4])
    assert pairs == [(0, 0), (1, 1), (2, 2)] and keep == [True, True, True]      # the delete is nobody's nearest operation


@pytest.mark.parametrize('use_ry', [False, True])
def test_host_tables_paint_what_pil_paints(use_ry):
    masks = _masks()
    masks[0, 0, 35, 90] = 1.0            # outside its roi: the reference map shows it, an edit never does
    boxes, keeps = [], []
    for ops_ in LISTS:
        mrois, drois, keep, _ = scene2d.edit_geometry(ROIS, ops_, use_ry)
        boxes.append(scene2d.paste_boxes(mrois, drois))
        keeps.append(keep)
    rec, bounds, kk8 = scene2d.paint_tables(ROIS, boxes, keeps, H, W)
    assert rec.shape == (len(LISTS), 3, scene2d.REC_INTS) and rec.dtype == np.int32 and bounds.dtype == np.int32 and kk8.dtype == np.int32
    assert rec[0, :, 11].tolist() == [0, 0, 0] and rec[0, :, 14].tolist() == [0, 0, 0]      # no-op: no pass at all
    assert rec[2, 2, 0] == 0 and keeps[2][2]                                               # wholly outside: paints nothing
    got = s2.emulate_paint(masks, rec, bounds, kk8)
    for f, ops_ in enumerate(LISTS):
        want, js, keep = s2.baseline(CLASS_IDS, masks, ROIS, ops_, use_ry)
        assert np.array_equal(got[f], want), 'list %d: %d pixels differ' % (f, int((got[f] != want).sum()))
        assert scene2d.frame_json(keeps[f], CLASS_IDS) == js and keeps[f] == keep
    assert got[0, 0, 35, 90] == 0 and s2.reference_map(masks)[0, 35, 90] == 1
    assert len(np.unique(got[1])) == 4 and not np.array_equal(got[0], got[1])


def test_a_zero_output_size_raises():
    flat = [{'type': 'modify', 'from': {'u': 28, 'v': 17}, 'to': {'u': 28, 'v': 17}, 'zoom': 0.03, 'ry': 0.0}]
    mrois, drois, keep, _ = scene2d.edit_geometry(ROIS, flat)
    bx = scene2d.paste_boxes(mrois, drois)
    assert bx[0][0] == 0
    with pytest.raises(ValueError, match='frame 1 object 0'):
        scene2d.paint_tables(ROIS, [s2.boxes(*s2.geometry(ROIS, [])[:2]), bx], [[True] * 3, keep], H, W)
    # 2D+: cos(ry) alone brings the column extent below one pixel
    thin = [{'type': 'modify', 'from': {'u': 28, 'v': 17}, 'to': {'u': 28, 'v': 17}, 'zoom': 1.0, 'ry': float(np.pi / 2)}]
    mrois, drois, keep, _ = scene2d.edit_geometry(ROIS, thin, use_ry=True)
    with pytest.raises(ValueError, match='frame 0 object 0.*> 0'):
        scene2d.paint_tables(ROIS, [scene2d.paste_boxes(mrois, drois)], [keep], H, W)
    # a deleted object is never resized
    gone = flat + [{'type': 'delete', 'from': {'u': 28, 'v': 17}}]
    mrois, drois, keep, _ = scene2d.edit_geometry(ROIS, gone)
    assert keep == [False, True, True] and scene2d.paste_boxes(mrois, drois)[0][0] == 0
    rec, _, _ = scene2d.paint_tables(ROIS, [scene2d.paste_boxes(mrois, drois)], [keep], H, W)
    assert rec[0, :, 0].tolist() == [0, 1, 1]


def test_an_empty_roi_raises():
    ok = s2.boxes(*s2.geometry(ROIS, [])[:2])
    with pytest.raises(ValueError, match='roi 1 .* is empty'):
        scene2d.paint_tables([ROIS[0], [10, 30, 10, 80], ROIS[2]], [ok], [[True] * 3], H, W)
    with pytest.raises(ValueError, match='roi 2 .* is empty'):
        scene2d.check_rois([ROIS[0], ROIS[1], [2, 60, 25, 60]], H, W)
    with pytest.raises(ValueError, match='leaves the 40 x 96 frame'):
        scene2d.check_rois([[2, 60, 41, 95]], H, W)


def test_the_c_entry_validates_the_records_without_a_gpu():
    """error paths return codes and set the message; no kernel is launched (fake non-null device pointers)"""
    import ctypes
    import sdn_hip
    L = sdn_hip.lib()
    fake = ctypes.c_void_p(4096)
    mrois, drois, keep, _ = scene2d.edit_geometry(ROIS, LISTS[2])
    rec, bounds, kk8 = scene2d.paint_tables(ROIS, [scene2d.paste_boxes(mrois, drois)], [keep], H, W)

    def call(r, n=3, h=H, w=W, host=True):
        r = np.ascontiguousarray(r, dtype=np.int32)
        return L.sdn_scene_paint2d(fake, r.ctypes.data if host else None, fake, 1, n, fake, bounds.shape[0], fake, kk8.shape[0], h, w,
                                   fake, None)
    assert call(rec, n=0) == -1 and b'bad sizes' in L.sdn_last_error()
    assert call(rec, n=256) == -1 and b'at most 255' in L.sdn_last_error()
    assert call(rec, host=False) == -1 and b'one side only' in L.sdn_last_error()
    bad = rec.copy()
    bad[0, 1, 1] = H - 1                                  # the window leaves the frame
    assert call(bad) == -1 and b'frame 0 object 1' in L.sdn_last_error()
    bad = rec.copy()
    bad[0, 0, 6] = 0
    assert call(bad) == -1 and b'output size' in L.sdn_last_error()
    bad = rec.copy()
    bad[0, 1, 13] = kk8.shape[0]                          # the column weights beyond the pool
    assert call(bad) == -1 and b'does not fit' in L.sdn_last_error()
    bad = rec.copy()
    bad[0, 1, 11] = 0                                     # ksize 0 although the size changes
    assert call(bad) == -1 and b'does not fit' in L.sdn_last_error()
