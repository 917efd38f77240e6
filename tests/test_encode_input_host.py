"""Host side of the textural input encoding (textural/models/input_maps.py, sdn_hip.ops.encode_maps / inst_index,
csrc/encode_input.hip): the fixture tests/golden/encode_input_golden.npz against the restatement of tests/encode_input_util.py,
the emulated bitmap / prefix / rank scheme against numpy's unique, the header's arithmetic and validators walked by a stand-alone
program under ASan + UBSan, the exported names, and the refusals.  No GPU is needed: every refusal happens before the library is
touched, and the C entry points validate on the host."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import encode_input_util as u
import host_checks
import makefile_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'textural')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NAMES = ('sdn_encode_maps', 'sdn_inst_index_workspace_bytes', 'sdn_inst_index_build', 'sdn_inst_index_rank')


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_the_golden_file_reproduces_from_its_script():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    try:
        import make_encode_input_golden as mk
    finally:
        sys.path.pop(0)
    kept, made = np.load(u.GOLD), mk.arrays()
    assert sorted(kept.files) == sorted(made)
    for k, a in made.items():
        assert kept[k].dtype == a.dtype and kept[k].shape == a.shape and np.array_equal(kept[k], a, equal_nan=True), k
    assert os.path.getsize(u.GOLD) < 128 * 1024


def test_the_restatement_is_the_products_torch_expressions():
    """encode_reference on the cases without a bad index equals Pix2PixHDModel._one_hot / get_edges as the model states them"""
    from models.pix2pixHD_model import Pix2PixHDModel
    m = Pix2PixHDModel.__new__(Pix2PixHDModel)
    for name, c in u.encode_cases().items():
        if 'want_bad' in c:
            continue
        label, inst, pose = u.case_tensors(c)
        got, got_pose, bad = u.encode_reference(label, inst, pose, c['label_nc'], c['pose_ch'])
        want = m._one_hot(label, c['label_nc'])
        if inst is not None:
            want = torch.cat((want, m.get_edges(inst)), dim=1)
        assert bad == [0, 0] and torch.equal(got, want), name
        if pose is not None:
            assert torch.equal(got_pose, m._one_hot(pose, c['pose_ch'])), name
    c = u.encode_cases()['bad_indices']
    label, inst, pose = u.case_tensors(c)
    got, got_pose, bad = u.encode_reference(label, inst, pose, c['label_nc'], c['pose_ch'])
    assert bad == c['want_bad']
    assert got[0, :14, 0].sum(0).tolist() == [1, 1, 0, 0, 0, 1, 1, 0] and got[0, 0, 0].tolist() == [1, 1, 0, 0, 0, 0, 1, 0] and got[0, 13, 0, 5] == 1
    assert got_pose[0, :, 3].sum(0).tolist() == [1, 0, 0, 1, 0, 1, 1, 1] and got_pose[0, 24, 3, 0] == 1 and got_pose[0, 24, 3, 6] == 1
    e = u.get_edges_reference(u.case_tensors(u.encode_cases()['wide_floats'])[1])[0, 0]
    assert e[1, :2].tolist() == [1, 1] and e[0, 1:3].tolist() == [1, 1] and e[3, 6:].tolist() == [1, 0] and e[2, 6:].tolist() == [1, 1]


def test_the_disambiguation_of_the_restatement_is_the_encoders():
    from models import networks
    for name, (inst, _) in u.index_cases().items():
        assert torch.equal(u.disambiguate_reference(inst.clone()), networks.Encoder._disambiguate(inst.clone())), name
    # int16 wraps in torch as in the header: 20 000 * 4 + i mod 2^16
    d = u.index_reference(u.index_cases()['int16_wraparound'][0])[0]
    assert d.dtype == torch.int16 and d[:, 0, 0, 0].tolist() == [14464, 14465, 14466, 14467] and d[2, 0, 1, 3].tolist() == -2


@pytest.mark.parametrize('name', sorted(u.index_cases()))
def test_the_emulated_bitmap_and_rank_scheme_equals_numpys_unique(name):
    inst, path = u.index_cases()[name]
    d = u.disambiguate_reference(inst.clone())
    ids, seg, counts, overflow = u.emulate_index(d.numpy())
    keys = d.reshape(-1).long().numpy()
    inside = (keys >= u.KEY_MIN) & (keys <= u.KEY_LAST)
    want_ids, want_inv, want_counts = np.unique(keys[inside], return_inverse=True, return_counts=True)
    assert overflow == int((~inside).sum()) and (overflow == 0) == (path == 'device')
    assert np.array_equal(ids, want_ids) and np.array_equal(counts, want_counts)
    assert np.array_equal(seg.reshape(-1)[inside], want_inv.reshape(-1)) and (seg.reshape(-1)[~inside] == -1).all()
    if path == 'device':
        gold = np.load(u.GOLD)
        assert np.array_equal(ids, gold['index/%s/ids' % name]) and np.array_equal(seg, gold['index/%s/inverse' % name])
        assert np.array_equal(counts, gold['index/%s/counts' % name])


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_arithmetic_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/encode_input_check.cpp: a stand-alone program with its own main that includes only csrc/encode_input_check.h; host
    code on the CPU, never loaded into Python"""
    rc, out = host_checks.run_check_program('encode_input_check', ['encode_input_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out


# ---- names ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    assert all(name in history[history.index('#define SDN_ABI_VERSION') - 3000:history.index('#define SDN_ABI_VERSION')] for name in NAMES)
    assert 'pix2pixHD_model.py:124-166' in history and 'networks.py:310-325' in history
    host_checks.stale_library_is_refused(NAMES)
    import sdn_hip
    from sdn_hip import ops
    n = ctypes.c_size_t()
    assert sdn_hip.lib().sdn_inst_index_workspace_bytes(ctypes.byref(n)) == 0 and n.value == 2 * 65536 * 4 + 16
    assert ops.INST_HEAD_AT == 65536 * 4 and (ops.INST_KEY_MIN, ops.INST_KEY_BITS) == (u.KEY_MIN, u.KEY_BITS)
    assert (ops.MAP_U8, ops.MAP_I16, ops.MAP_I32, ops.MAP_F32) == tuple(int(re.search(r'#define SDN_MAP_%s (\d)' % k, history).group(1))
                                                                        for k in ('U8', 'I16', 'I32', 'F32'))


def test_the_kernels_are_built_without_fma_contraction():
    makefile_rules.assert_built_exactly('encode_input.hip')


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_c_entry_points_validate_on_the_host():
    import sdn_hip
    L = sdn_hip.lib()
    fake, odd, ws = ctypes.c_void_p(4096), ctypes.c_void_p(4098), 2 * 65536 * 4 + 16
    U8, I16, I32, F32 = 0, 1, 2, 3
    err = lambda: L.sdn_last_error()
    enc = lambda *a: L.sdn_encode_maps(*a, None)
    assert enc(None, U8, fake, I16, fake, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'sdn_encode_maps: label is NULL' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 14, 25, None, fake, fake) == -1 and b'input_label or bad is NULL' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 14, 25, fake, fake, None) == -1 and b'input_label or bad is NULL' in err()
    assert enc(fake, I16, fake, I16, fake, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'label dtype 1' in err()
    assert enc(fake, U8, fake, U8, fake, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'inst dtype 0' in err()
    assert enc(fake, U8, fake, I16, fake, U8, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'pose dtype 0' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 0, 25, fake, fake, fake) == -1 and b'label_nc is 0; 1 to 256' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 257, 25, fake, fake, fake) == -1 and b'label_nc is 257' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 14, 257, fake, fake, fake) == -1 and b'pose_ch is 257' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 14, -1, fake, fake, fake) == -1 and b'pose_ch is -1' in err()
    assert enc(fake, U8, fake, I16, None, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'pose or pose_onehot is NULL' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 14, 25, fake, None, fake) == -1 and b'pose or pose_onehot is NULL' in err()
    assert enc(odd, F32, fake, I16, fake, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'label is not aligned' in err()
    assert enc(fake, U8, ctypes.c_void_p(4097), I16, fake, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'inst is not aligned' in err()
    assert enc(fake, U8, fake, I16, odd, F32, 1, 2, 3, 14, 25, fake, fake, fake) == -1 and b'pose and pose_onehot must be aligned' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 1, 2, 3, 14, 25, odd, fake, fake) == -1 and b'input_label and bad must be aligned' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 0, 2, 3, 14, 25, fake, fake, fake) == -1 and b'bad sizes' in err()
    assert enc(fake, U8, fake, I16, fake, F32, 16, 4096, 4096, 14, 25, fake, fake, fake) == -1 and b'below 2^31' in err()

    build = lambda *a: L.sdn_inst_index_build(*a, None)
    assert build(None, F32, 1, 3, 5, fake, ws, fake, fake, 15) == -1 and b'sdn_inst_index_build: inst is NULL' in err()
    assert build(fake, U8, 1, 3, 5, fake, ws, fake, fake, 15) == -1 and b'inst dtype 0' in err()
    assert build(odd, F32, 1, 3, 5, fake, ws, fake, fake, 15) == -1 and b'inst is not aligned' in err()
    assert build(fake, F32, 1, 3, 5, None, ws, fake, fake, 15) == -1 and b'workspace is NULL' in err()
    assert build(fake, F32, 1, 3, 5, ctypes.c_void_p(4104), ws, fake, fake, 15) == -1 and b'workspace must be aligned to 16' in err()
    assert build(fake, F32, 1, 3, 5, fake, ws - 1, fake, fake, 15) == -1 and b'workspace holds 524303 bytes, 524304 are needed' in err()
    assert build(fake, F32, 1, 3, 5, fake, ws, None, fake, 15) == -1 and b'ids is NULL' in err()
    assert build(fake, F32, 1, 3, 5, fake, ws, ctypes.c_void_p(4100), fake, 15) == -1 and b'aligned to 8' in err()
    assert build(fake, F32, 1, 3, 5, fake, ws, fake, fake, 14) == -1 and b'ids holds 14 entries, 15 are needed' in err()
    assert build(fake, F32, 1, 0, 5, fake, ws, fake, fake, 15) == -1 and b'bad sizes' in err()
    assert build(fake, F32, 2, 32768, 32768, fake, ws, fake, fake, 1 << 21) == -1 and b'below 2^31' in err()
    rank = lambda *a: L.sdn_inst_index_rank(*a, None)
    assert rank(None, F32, 1, 3, 5, fake, ws, fake, fake) == -1 and b'sdn_inst_index_rank: inst is NULL' in err()
    assert rank(fake, F32, 1, 3, 5, fake, ws, None, fake) == -1 and b'seg is NULL' in err()
    assert rank(fake, F32, 1, 3, 5, fake, ws, odd, fake) == -1 and b'seg must be aligned' in err()
    assert rank(fake, F32, 1, 3, 5, fake, ws, fake, ctypes.c_void_p(4100)) == -1 and b'counts must be aligned' in err()
    assert rank(fake, F32, 1, 3, 5, fake, 16, fake, fake) == -1 and b'workspace holds 16' in err()
    assert L.sdn_inst_index_workspace_bytes(None) == -1 and b'bytes is NULL' in err()


def test_the_python_entries_refuse_before_the_library_is_touched(monkeypatch):
    from models import input_maps
    from sdn_hip import ops
    monkeypatch.setattr(ops, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was touched')))
    label, inst, pose = u.case_tensors(u.encode_cases()['real_channels'])
    for fn in (ops.encode_maps, input_maps.encode_maps):
        with pytest.raises(NotImplementedError):                       # CPU tensors, as every op of this library
            fn(label, inst, pose, 14, 25)
        with pytest.raises(NotImplementedError):
            fn(label.to(torch.uint8), None, None, 14, 0)
    for fn in (ops.inst_index, input_maps.instance_index):
        with pytest.raises(NotImplementedError):
            fn(inst.clone())
        with pytest.raises(NotImplementedError):
            fn(inst.to(torch.int16), with_counts=True)
    with pytest.raises(TypeError):
        ops.encode_maps(label.numpy(), inst, pose, 14, 25)
    with pytest.raises(TypeError):
        ops.encode_maps(label.double(), inst, pose, 14, 25)
    with pytest.raises(TypeError):
        ops.encode_maps(label.to(torch.int16), inst, pose, 14, 25)        # int16 labels are not taken
    with pytest.raises(TypeError):
        ops.encode_maps(label, inst.to(torch.uint8), pose, 14, 25)
    with pytest.raises(TypeError):
        ops.encode_maps(label, inst, pose.to(torch.uint8), 14, 25)
    with pytest.raises(ValueError):
        ops.encode_maps(label[:, 0], inst, pose, 14, 25)                   # three axes
    with pytest.raises(ValueError):
        ops.encode_maps(label, inst[:, :, :8], pose, 14, 25)               # another shape
    with pytest.raises(ValueError):
        ops.encode_maps(label[:, :, :0], None, None, 14, 0)                # an empty axis
    for nc, pc in ((0, 25), (257, 25), (14, 257), (14, -1)):
        with pytest.raises(ValueError):
            ops.encode_maps(label, inst, pose, nc, pc)
    with pytest.raises(ValueError, match='go together'):
        ops.encode_maps(label, inst, None, 14, 25)
    with pytest.raises(ValueError, match='go together'):
        ops.encode_maps(label, inst, pose, 14, 0)
    with pytest.raises(ValueError, match='2\\^31'):
        ops.encode_maps(torch.zeros(1, 1, 1, 1).expand(16, 1, 4096, 4096), None, None, 14, 0)
    with pytest.raises(TypeError):
        ops.inst_index(inst.double())
    with pytest.raises(TypeError):
        ops.inst_index(inst.to(torch.uint8))
    with pytest.raises(ValueError):
        ops.inst_index(inst[0])
    # the wiring's gate: CPU maps, unsupported dtypes and layouts take the torch expressions
    assert not input_maps.encode_maps_supported(label, inst, pose, 14, 25) and not input_maps.instance_index_supported(inst)


def test_cpu_maps_keep_the_torch_expressions_in_the_model_and_the_encoder(monkeypatch):
    """On CPU maps encode_input and Encoder._pooled run what they ran before; so they do with SDN_ENCODE_DEVICE=0"""
    from models import input_maps, networks
    from models.pix2pixHD_model import Pix2PixHDModel, default_options
    from sdn_hip import ops
    monkeypatch.setattr(ops, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was touched')))
    c = u.encode_cases()['real_channels']
    label, inst, pose = u.case_tensors(c)
    m = Pix2PixHDModel.__new__(Pix2PixHDModel)
    m.opt = default_options(feat_pose='1', feat_normal='1')
    m.use_features = True
    m._device = lambda: torch.device('cpu')
    got = m.encode_input(label, inst, pose_map=pose, normal_map=torch.zeros(2, 3, 16, 24))
    want, want_pose, _ = u.encode_reference(label, inst, pose, 14, 25)
    assert torch.equal(got[0], want) and torch.equal(got[4], want_pose) and torch.equal(got[1], inst) and m.last_encode_bad is None
    assert input_maps.device_path_enabled()
    monkeypatch.setenv('SDN_ENCODE_DEVICE', '0')
    assert not input_maps.device_path_enabled()
    assert hasattr(networks.Encoder, '_disambiguate') and hasattr(Pix2PixHDModel, '_one_hot') and hasattr(Pix2PixHDModel, 'get_edges')
