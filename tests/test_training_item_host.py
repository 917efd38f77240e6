"""The host side of maskrcnn.training_item: the plan of resize_image, the restatement tests/training_item_util.py against the fixture
tests/golden/training_item_golden.npz (what the reference's own functions gave, tests/golden/make_training_item_golden.py), the gather
form of ndimage.zoom against scipy, the coefficient recipe the mini-mask kernel walks against Pillow's tables as sdn_hip/pillow.py
states them, the refusals, and tools/training_item_check.cpp under ASan and UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.ndimage
import torch

import training_item_util as u
from maskrcnn import training_item as ti   # the feature itself: without it this module does not import
from sdn_hip import pillow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return u.golden()


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    """tools/training_item_check.cpp built with ASan and UBSan and run once as a child process: (return code, output)"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src = os.path.join(ROOT, 'tools', 'training_item_check.cpp')
    exe = str(tmp_path_factory.mktemp('tri') / 'training_item_check')
    # the sanitizers' runtimes are linked into the program itself, so it runs the same whatever the environment preloads
    static = ['-static-libasan', '-static-libubsan'] if 'clang' not in os.path.basename(cxx) else ['-static-libsan']
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                          ['-I' + os.path.join(ROOT, '3d-sdn_amd', 'csrc'), src, '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return run.returncode, run.stdout.decode()


@pytest.mark.parametrize('name', u.CASES)
def test_resize_plan_is_resize_images(gold, name):
    cfg, plan = u.case_config(gold, name), gold[name + '_plan'].tolist()
    oh, ow, window, scale, padding = ti.resize_plan(gold[name + '_frame'].shape, cfg)
    assert [oh, ow] + list(window) + [padding[0][0], padding[0][1], padding[1][0], padding[1][1]] == plan and padding[2] == (0, 0)
    assert isinstance(oh, int) and isinstance(ow, int) and float(scale) == float(gold[name + '_scale'])
    block, window2 = ti.plan_block(gold[name + '_frame'].shape, cfg, flip=True)
    assert window2 == window and block.dtype == np.int32 and block[:8].tolist() == list(gold[name + '_frame'].shape[:2]) + [
        oh, ow, cfg.IMAGE_MAX_DIM, padding[0][0], padding[1][0], 1]


def test_resize_plan_at_the_reference_size():
    cfg = u.Config(800, 1024, 56)
    oh, ow, window, scale, padding = ti.resize_plan((375, 1242, 3), cfg)
    assert (oh, ow, window, scale) == (309, 1024, (357, 0, 666, 1024), 1024 / 1242) and padding == [(357, 358), (0, 0), (0, 0)]
    assert ti.zoom_table(1242, 1024)[-1] == 1241 and ti.zoom_table(375, 309)[-1] == 374 and ti.zoom_table(248, 192)[-1] == -1
    assert ti.zoom_table(5, 1).tolist() == [0]


@pytest.mark.parametrize('name', u.CASES)
@pytest.mark.parametrize('flip', [0, 1])
def test_the_restatement_gives_the_fixtures_bits(gold, name, flip):
    cfg, p = u.case_config(gold, name), name + '_'
    G, M = len(gold[p + 'ids']), cfg.IMAGE_MAX_DIM
    image = gold[p + 'image_u8']
    full = u.unpack(gold, p + 'full_bits', (M, M, G))
    if flip:
        image, full = np.fliplr(image), np.fliplr(full)
    for use_mini in (False, True):
        r = u.training_item(gold[p + 'frame'], gold[p + 'inst_map'], gold[p + 'ids'], cfg, flip=bool(flip), use_mini_mask=use_mini)
        masks = u.unpack(gold, p + 'mini_bits%d' % flip, cfg.MINI_MASK_SHAPE + (G,)) if use_mini else full
        assert np.array_equal(r['image_u8'], image) and r['image'].tobytes() == u.mold(image, cfg).tobytes()
        assert r['gt_boxes_int'].dtype == np.int32 and np.array_equal(r['gt_boxes_int'], gold[p + 'boxes%d' % flip])
        assert np.array_equal(r['gt_masks'], masks.transpose(2, 0, 1).astype(np.float32))
        assert np.array_equal(r['areas'], gold[p + 'areas']) and np.array_equal(r['bad'], gold[p + 'bad'])
        assert list(r['window']) == gold[p + 'plan'][2:6].tolist()


def test_the_mean_table_is_mold_image(gold):
    cfg = u.case_config(gold, 'down')
    table = ti.mean_table(cfg)
    image = gold['down_image_u8']
    looked_up = np.stack([table[c][image[..., c]] for c in range(3)])
    assert table.dtype == np.float32 and looked_up.tobytes() == u.mold(image, cfg).tobytes()
    assert table[:, 0].tolist() == [np.float32(-m) for m in cfg.MEAN_PIXEL]


def test_zoom_is_a_gather_also_beyond_the_edge():
    rng = np.random.default_rng(3)
    beyond = 0
    pairs = [(248, 192), (1242, 1024), (375, 309), (40, 96), (75, 58), (5, 1), (1, 3), (7, 7), (2, 5)] + [
        (int(a), int(b)) for a, b in rng.integers(2, 300, (150, 2))]
    for n_in, n_out in pairs:
        table = ti.zoom_table(n_in, n_out)
        beyond += int((table < 0).sum())
        line = rng.random((n_in, 1, 2)) < 0.5
        scale = n_out / n_in
        if int(round(n_in * scale)) != n_out:
            continue
        ref = scipy.ndimage.zoom(line, zoom=[scale, 1, 1], order=0)
        mine = line[np.maximum(table, 0)].copy()
        mine[table < 0] = False
        assert ref.shape == mine.shape and np.array_equal(ref, mine), (n_in, n_out)
    assert beyond > 0 and ti.zoom_table(248, 192)[-1] == -1
    # two axes at once, the util's form, at the scale the plan gives
    mask = rng.random((75, 248, 3)) < 0.5
    scale = 192 / 248
    assert np.array_equal(u.zoom_by_gather(mask, scale), scipy.ndimage.zoom(mask, zoom=[scale, scale, 1], order=0))


def _fnv(h, v):
    return ((h ^ (v & 0xffffffff)) * 1099511628211) & 0xffffffffffffffff


def _tables_hash(n_out, max_in):
    """the walk of the device's recipe equals Pillow's tables for every source size; returns the hash the check program prints"""
    h = 1469598103934665603
    for n_in in range(1, max_in + 1):
        ksize, bounds, coeffs = u.coefficient_walk(n_in, n_out)
        ref_ksize, ref_bounds, ref_kk = pillow.resample_tables(n_in, n_out)
        assert ksize == ref_ksize and bounds == ref_bounds.tolist() and coeffs == pillow.fixed_point(ref_kk).tolist(), (n_in, n_out)
        h = _fnv(h, ksize)
        for b, k in zip(bounds, coeffs):
            for v in k:
                h = _fnv(h, v)
            h = _fnv(_fnv(h, b[0]), b[1])
    return h


def test_the_devices_coefficient_recipe_is_pillows(check_program):
    rc, text = check_program
    assert rc == 0, text
    printed = dict(re.findall(r'tables (\d+) ([0-9a-f]{16})', text))
    assert printed['56'] == '%016x' % _tables_hash(56, 1024)
    assert printed['28'] == '%016x' % _tables_hash(28, 64)


def test_check_program_runs_clean_under_the_host_sanitizers(check_program):
    rc, text = check_program
    assert rc == 0 and 'training_item_check: 0 failures' in text and 'the validators: walked' in text, text
    assert 'ERROR' not in text and 'runtime error' not in text, text
    src = open(os.path.join(ROOT, 'tools', 'training_item_check.cpp')).read()
    assert re.findall(r'#include "([^"]+)"', src) == ['training_item_check.h'] and 'int main()' in src and 'hip_runtime' not in src


def _cpu_item(gold, name='same', G=None):
    p = name + '_'
    ids = gold[p + 'ids'] if G is None else np.arange(G, dtype=np.int32)
    return (torch.from_numpy(gold[p + 'frame'].copy()), torch.from_numpy(gold[p + 'inst_map'].copy()), torch.from_numpy(ids.copy()),
            torch.ones(len(ids), dtype=torch.int32))


def test_refusals(gold):
    cfg = u.case_config(gold, 'same')
    frame, inst_map, ids, class_ids = _cpu_item(gold)
    with pytest.raises(NotImplementedError, match='only runs on the GPU'):
        ti.training_item(frame, inst_map, ids, class_ids, cfg)
    with pytest.raises(NotImplementedError, match='only runs on the GPU'):
        ti.load_image_gt(frame, inst_map, ids, class_ids, cfg)
    with pytest.raises(NotImplementedError, match='only runs on the GPU'):
        ti.mold_inputs([frame], cfg)
    for G in (0, 129):
        f, m, i, c = _cpu_item(gold, G=G)
        with pytest.raises(ValueError, match='1 to 128 instances'):
            ti.training_item(f, m, i, c, cfg)
    few = u.case_config(gold, 'same')
    few.MAX_GT_INSTANCES = 2
    with pytest.raises(ValueError, match='MAX_GT_INSTANCES'):
        ti.training_item(frame, inst_map, ids, class_ids, few)
    loose = u.case_config(gold, 'same')
    loose.IMAGE_PADDING = False
    with pytest.raises(ValueError, match='not supported'):
        ti.resize_plan(frame.shape, loose)
    with pytest.raises(ValueError, match='not supported'):
        ti.training_item(frame, inst_map, ids, class_ids, loose)
    with pytest.raises(ValueError, match=r'class_ids must be \[G\]'):
        ti.training_item(frame, inst_map, ids, class_ids[:1], cfg)
    with pytest.raises(ValueError, match=r'uint8 \[H, W, 3\]'):
        ti.training_item(frame[..., 0], inst_map, ids, class_ids, cfg)
    with pytest.raises(ValueError, match='inst_map must be'):
        ti.training_item(frame, inst_map[:-1], ids, class_ids, cfg)
    with pytest.raises(TypeError, match='inst_map must be'):
        ti.training_item(frame, inst_map.to(torch.int64), ids, class_ids, cfg)
    with pytest.raises(TypeError, match='ids must be'):
        ti.training_item(frame, inst_map, ids.to(torch.int64), class_ids, cfg)
    with pytest.raises(ValueError, match='distinct ops'):
        ti.training_item(frame, inst_map, ids, class_ids, cfg, jitter=([1, 1], (1.0, 1.2, 1.0), 0))
    big = u.Config(64, 128, 57)
    with pytest.raises(ValueError, match='each side 1 to 56'):
        ti.training_item(frame, inst_map, ids, class_ids, big)


def test_color_keys():
    codes = np.array([[10, 27, 44], [255, 0, 1], [0, 0, 0]], np.uint8)
    want = [(10 << 16) | (27 << 8) | 44, (255 << 16) | 1, 0]
    assert ti.color_keys(codes).tolist() == want and ti.color_keys(codes).dtype == np.int32
    keys = ti.color_keys(torch.from_numpy(codes))
    assert keys.dtype == torch.int32 and keys.tolist() == want
    meta = ti.compose_image_meta(7, (375, 1242, 3), (357, 0, 666, 1024), np.ones(4, np.int32))
    assert meta.tolist() == [7, 375, 1242, 3, 357, 0, 666, 1024, 1, 1, 1, 1]
