"""CPU: the host half of the detector-output path (geometric/maskrcnn/detections.py) and the numpy emulation of
sdn_unmold_masks / sdn_scene_gt_masks against tests/golden/detections_golden.npz (the reference's statements, executed:
tests/golden/make_detections_golden.py).  Exact comparisons throughout."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import detections_util as du  # noqa: E402
from maskrcnn import detections as det  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return du.load()


def test_fixture_is_small_and_holds_the_cases(gold):
    assert os.path.getsize(du.GOLDEN) < 1000000
    g = gold
    assert g['a_detections'].shape == (100, 6) and g['a_mrcnn_mask'].shape == (100, 3, 28, 28)
    assert len(g['a_areas']) == 25 and len(g['a_sels']) == 16 and len(set(g['a_areas'].tolist())) == 25
    assert int(g['a_bytes_f32_vs_f64']) > 0


def test_mold_window_equals_the_reference(gold):
    for tag in 'abc':
        window, scale = det.mold_window(tuple(gold[tag + '_image_shape']), *gold[tag + '_mold'].tolist())
        assert list(window) == gold[tag + '_window'].tolist(), tag
    window, scale = det.mold_window((375, 1242, 3), 300, 1024)
    assert window == (357, 0, 666, 1024) and scale == float(gold['a_scale'])
    assert det.mold_window((480, 640, 3), 800, 1024) == ((128, 0, 896, 1024), 1.6)     # scaled up, not beyond max_dim


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_unmold_boxes_equals_the_reference(gold, tag):
    g = gold
    boxes, ids, scores, keep = det.unmold_boxes(g[tag + '_detections'], tuple(g[tag + '_image_shape']), g[tag + '_window'])
    for got, want in ((boxes, g[tag + '_boxes']), (ids, g[tag + '_class_ids']), (scores, g[tag + '_scores'])):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), tag
    if tag == 'a':
        assert np.array_equal(keep, g['a_keep']) and 4 not in keep.tolist()           # the zero-area row
    if tag == 'c':   # model.py:2140-2141: no detection
        assert boxes.shape == (0, 4) and ids.shape == (0,) and scores.shape == (0,) and keep.shape == (0,)
        assert g['c_masks_shape'].tolist() == [0, 28, 28]


def test_unmold_boxes_without_a_zero_row_and_truncation_toward_zero():
    d = np.asarray([[10.9, 10.9, 20.9, 30.9, 1, 0.9], [-3.7, 4.2, 9.99, 8.0, 2, 0.8]], np.float32)
    boxes, ids, scores, keep = det.unmold_boxes(d, (64, 64, 3), (0, 0, 64, 64))
    assert boxes.tolist() == [[10, 10, 20, 30], [-3, 4, 9, 8]] and ids.tolist() == [1, 2] and keep.tolist() == [0, 1]


def test_select_largest_equals_the_reference(gold):
    assert np.array_equal(det.select_largest(gold['a_areas']), gold['a_sels'])
    assert np.array_equal(det.select_largest(gold['b_areas']), gold['b_sels'])
    assert np.array_equal(det.select_largest(gold['g_areas']), gold['g_sels'])
    assert det.select_largest(gold['a_areas'], 3).tolist() == gold['a_sels'][:3].tolist()
    ids, boxes = gold['a_class_ids'], gold['a_boxes']
    assert np.array_equal(ids[gold['a_sels']], gold['a_sel_class_ids']) and np.array_equal(boxes[gold['a_sels']], gold['a_sel_rois'])


def test_bytescale_follows_the_float32_rule(gold):
    g = gold
    keep, ids = g['a_keep'], g['a_class_ids']
    for i, (d, c) in enumerate(zip(keep, ids)):
        assert np.array_equal(du.bytescale_f32(g['a_mrcnn_mask'][d, c]), g['a_bytes'][i]), 'detection %d' % i
    # the float64 evaluation (what numpy 2 makes of the same expression) gives other bytes on this fixture
    plane = g['a_mrcnn_mask'][keep[24], ids[24]]
    f64 = ((plane - plane.min()).astype(np.float64) * (255.0 / float(plane.max() - plane.min()))).clip(0, 255) + 0.5
    assert not np.array_equal(f64.astype(np.uint8), g['a_bytes'][24])


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_emulation_equals_the_fixture_bit_for_bit(gold, tag):
    g = gold
    H, W = g[tag + '_image_shape'][:2]
    boxes, ids, scores, keep = det.unmold_boxes(g[tag + '_detections'], (H, W), g[tag + '_window'])
    objs, bounds, kk8 = det.unmold_tables(boxes, ids, keep, 28, 28)
    masks, areas = du.unmold_emulated(g[tag + '_mrcnn_mask'], objs, H, W)
    want = du.planes(g, tag)
    for i in range(len(boxes)):
        assert np.array_equal(masks[i], want[i]), 'detection %d: %d pixels differ' % (i, int((masks[i] != want[i]).sum()))
    assert np.array_equal(areas, g[tag + '_areas'])


def test_gt_emulation_equals_the_fixture(gold):
    g = gold
    masks, rois, areas = du.gt_emulated(g['g_scene'], g['g_codes'])
    assert np.array_equal(masks, du.planes(g, 'g')) and np.array_equal(rois, g['g_rois']) and np.array_equal(areas, g['g_areas'])
    assert areas[4] == 1 and str(g['h_error']) == 'IndexError'
    _, rois, areas = du.gt_emulated(g['g_scene'], g['h_codes'])
    assert areas[2] == 0 and rois[2, 0] > rois[2, 2]


def test_table_layout(gold):
    """the rows sdn_unmold_masks reads: (detection, class, box, tables of the rows, tables of the columns)"""
    g = gold
    boxes, ids, keep = g['a_boxes'], g['a_class_ids'], g['a_keep']
    objs, bounds, kk8 = det.unmold_tables(boxes, ids, keep, 28, 28)
    assert objs.dtype == bounds.dtype == kk8.dtype == np.int32 and objs.shape == (25, det.OBJ_INTS) and det.OBJ_INTS == 12
    assert np.array_equal(objs[:, 0], keep) and np.array_equal(objs[:, 1], ids) and np.array_equal(objs[:, 2:6], boxes)
    from derender3d import compositing as comp
    for i, (y1, x1, y2, x2) in enumerate(boxes.tolist()):
        for col, size in ((6, y2 - y1), (9, x2 - x1)):
            boff, koff, ksize = objs[i, col:col + 3].tolist()
            if size == 28:
                assert ksize == 0                                                    # Pillow skips the pass
                continue
            ks, b, kk = comp.resample_tables(28, size)
            assert ksize == ks and np.array_equal(bounds[boff:boff + size], b)
            assert np.array_equal(kk8[koff:koff + size * ks], comp.fixed_point(kk).reshape(-1))
    assert (objs[5, 6:9] == 0).all() and (objs[6, 9:12] == 0).all() and (objs[24, 6:12] == 0).all()
    # one table per distinct size pair
    sizes = set((y2 - y1) for y1, x1, y2, x2 in boxes.tolist()) | set((x2 - x1) for y1, x1, y2, x2 in boxes.tolist())
    assert bounds.shape[0] == sum(s for s in sizes if s != 28)


def test_out_of_frame_boxes_raise(gold):
    g = gold
    H, W = 375, 1242
    ids = g['a_class_ids']
    det.check_boxes(g['a_boxes'], ids, H, W, 3)
    for bad in ([10, 1200, 50, 1243], [-1, 5, 20, 30], [300, 5, 376, 30], [10, -2, 20, 30]):
        boxes = g['a_boxes'].copy()
        boxes[3] = bad
        with pytest.raises(ValueError, match='leaves the 375 x 1242 frame'):
            det.check_boxes(boxes, ids, H, W, 3)
    with pytest.raises(ValueError, match='class ids'):
        det.check_boxes(g['a_boxes'], np.full_like(ids, 3), H, W, 3)
    # unmold_detections raises the same ValueError for a detection whose box leaves the frame; that needs the device and is
    # covered in tests/test_gpu_detections.py.  Here: a CPU mrcnn_mask is refused.
    with pytest.raises(NotImplementedError):
        det.unmold_detections(g['a_detections'], torch.from_numpy(g['a_mrcnn_mask']), (H, W, 3), g['a_window'])
    with pytest.raises(ValueError, match='max_dim'):
        det.mold_window((375, 1242, 3), 300, None)


def test_cpu_tensors_are_refused(gold):
    from sdn_hip import ops
    g = gold
    with pytest.raises(NotImplementedError):
        ops.unmold_masks(torch.from_numpy(g['b_mrcnn_mask']), np.zeros((1, 12), np.int32), (None, None, None), 60, 90)
    with pytest.raises(NotImplementedError):
        ops.scene_gt_masks(torch.from_numpy(g['g_scene']), torch.from_numpy(g['g_codes']))
