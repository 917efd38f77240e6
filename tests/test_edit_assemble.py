"""The edit path without a GPU (textural/edit_vkitti.py:62-103, edit_benchmark.py:87-126 -> data.assemble.assemble_edit,
edit.EditSession, Pix2PixHDModel.encode_features): the entry point is declared and bound, the host-built object tables are
right, bad JSON keys are refused, and CPU tensors raise NotImplementedError as every other op of the project does.
The device side is tests/test_gpu_edit.py."""
import os
import re
from math import pi

import numpy as np
import pytest
import torch

import edit_util as eu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_bound():
    import sdn_hip
    src = open(os.path.join(ROOT, 'include', 'sdn_hip.h')).read()
    m = re.search(r'\bint\s+sdn_edit_assemble\s*\(([^;]*)\)\s*;', re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    assert m, 'include/sdn_hip.h does not declare sdn_edit_assemble'
    n_args = len(m.group(1).split(','))
    assert 'sdn_edit_assemble' in sdn_hip.exported_symbols()
    fn = sdn_hip.lib().sdn_edit_assemble
    assert len(fn.argtypes) == n_args == 18
    # argument checks come before any launch: no GPU needed
    assert fn(None, 0, None, None, None, None, None, 1, 1, 1, 16, 1, None, None, None, None, None, None) == -1
    assert b'null pointer' in sdn_hip.lib().sdn_last_error()
    import ctypes
    fake = ctypes.c_void_p(4096)
    args = lambda **kw: [fake, kw.get('stride', 16), fake, fake, fake, fake, fake, kw.get('K', 4), kw.get('C', 3), 1, 16,  # noqa: E731
                         kw.get('P', 1), fake, fake, fake, fake, fake, None]
    assert fn(*args(P=3)) == -1 and b'pose_channels' in sdn_hip.lib().sdn_last_error()
    assert fn(*args(stride=8)) == -1 and b'base_stride' in sdn_hip.lib().sdn_last_error()
    assert fn(*args(K=4096, C=5)) == -1 and b'LDS' in sdn_hip.lib().sdn_last_error()


def test_object_tables_follow_the_json():
    from data import assemble as asm
    seen_classes = set()
    for case in eu.cases():
        opt = eu.options(case.bins)
        bins = np.array(list(range(-180, 181, 360 // case.bins))) / 180 if case.bins else None
        for i in range(case.frames):
            _, js, _ = case.edit(i)
            label, pose = asm.edit_tables(opt, js)
            assert label.dtype == pose.dtype == np.int32 and label.shape == pose.shape == (256,)
            want_label, want_pose = np.zeros(256, np.int32), np.zeros(256, np.int32)
            for k, v in js.items():
                want_label[int(k)] = {1: 2, 2: 12}[v['class_id']]
                seen_classes.add(v['class_id'])
                if case.bins:
                    want_pose[int(k)] = int(np.digitize(v['alpha'] / pi, bins))
            assert np.array_equal(label, want_label) and np.array_equal(pose, want_pose)
            if not case.bins:
                assert not pose.any()
    assert seen_classes == {1, 2}
    assert any(not case.edit(i)[1] for case in eu.cases() for i in range(case.frames))   # a frame with no objects


@pytest.mark.parametrize('key', ['0', '256', '-3'])
def test_a_json_key_outside_the_uint8_ids_is_refused(key):
    from data import assemble as asm
    opt = eu.options(24)
    js = {'1': {'class_id': 1, 'alpha': 0.1}, key: {'class_id': 2, 'alpha': 0.2}}
    with pytest.raises(ValueError, match='outside 1..255'):
        asm.edit_tables(opt, js)
    inst = torch.zeros(1, 48, 160, dtype=torch.uint8)
    base = {'label': torch.ones(1, 48, 160), 'image': torch.zeros(3, 48, 160)}
    with pytest.raises(ValueError, match='outside 1..255'):
        asm.assemble_edit(opt, eu.PARAMS, base, inst, js, (torch.tensor([1]), torch.zeros(1, 3)))
    with pytest.raises(KeyError):   # an unknown class id: the reference's own dict look-up (edit_vkitti.py:79)
        asm.edit_tables(opt, {'1': {'class_id': 3, 'alpha': 0.0}})


def test_cpu_tensors_raise_not_implemented():
    from data import assemble as asm
    from edit import EditSession
    from models.pix2pixHD_model import Pix2PixHDModel
    from sdn_hip import ops
    case = eu.cases()[0]
    opt = eu.options(case.bins)
    segm, image, inst0, _, _ = case.source(0)
    ei, js, nrm = case.edit(0)
    base = asm.assemble_item(opt, eu.PARAMS, eu.chw(segm), eu.chw(image), inst=eu.chw(inst0))   # the loader's part runs anywhere
    codes = (torch.from_numpy(case.code_ids), torch.from_numpy(case.codes))
    with pytest.raises(NotImplementedError):
        asm.assemble_edit(opt, eu.PARAMS, base, eu.chw(ei), js, codes, eu.chw(nrm))
    with pytest.raises(NotImplementedError):
        asm.assemble_edit(opt, eu.PARAMS, [base] * 2, [eu.chw(ei)] * 2, [js] * 2, codes)
    with pytest.raises(NotImplementedError):
        ops.edit_assemble(base['label'][None], eu.chw(ei)[None], torch.zeros(1, 256, dtype=torch.int32),
                          torch.zeros(1, 256, dtype=torch.int32), codes[0].int(), codes[1].t().contiguous())
    with pytest.raises(NotImplementedError):
        EditSession(None, opt, eu.PARAMS, eu.chw(segm), eu.chw(image), eu.chw(inst0))
    model = object.__new__(Pix2PixHDModel)
    with pytest.raises(NotImplementedError):
        model.encode_features(torch.zeros(1, 3, 48, 160), torch.zeros(1, 1, 48, 160))


def test_fixture_has_the_cases_the_edit_path_needs():
    cs = {c.name: c for c in eu.cases()}
    assert {c.bins for c in cs.values()} == {24, 0}
    assert any(c.per_frame_source for c in cs.values()) and any(not c.per_frame_source for c in cs.values())
    b = cs['bench24']
    assert b.missing(0) > 0 and b.missing(1) == 0
    for c in cs.values():
        for i in range(c.frames):
            e = c.expected(i)
            assert e['pose'].shape[0] == (1 if c.bins else 2) and e['feat'].shape == (3, 48, 160)
            if not c.per_frame_source:   # edit_vkitti: every final instance id has a code (the reference raises otherwise)
                assert set(np.unique(e['inst']).astype(int).tolist()) <= set(c.code_ids.tolist())
    # an object moved onto former "misc" and former car pixels (source label 5 and 2 under its new footprint)
    v = cs['vkitti24']
    _, _, _, base_segm, _ = v.source(1)
    moved = v.expected(1)['inst'][0] == 2000
    assert {2.0, 5.0} <= set(np.unique(base_segm[0][moved]).tolist())
