"""GPU: the textural input encoding -- sdn_encode_maps and sdn_inst_index_* (csrc/encode_input.hip) under
sdn_hip.ops.encode_maps / inst_index, textural/models/input_maps.py, Pix2PixHDModel.encode_input and Encoder._pooled.

The expected values are tests/golden/encode_input_golden.npz: the torch expressions the kernels replace, run on the CPU by
tests/encode_input_util.py (zeros + long + scatter_, get_edges' four ORs, cat; _disambiguate + torch.unique).  Every output is a
0, a 1, an integer or a copy of an input value, so every comparison is equality; there is no tolerance in this file."""
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

import edit_util as eu  # noqa: E402
import encode_input_util as u  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ENCODE = u.encode_cases()
INDEX = u.index_cases()


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


def _offset(t):
    """the same values in storage that begins one element past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _raw_encode(label, inst, pose, label_nc, pose_ch):
    """sdn_encode_maps on outputs pre-filled with NaN (and bad with a sentinel): what the kernel itself writes"""
    import sdn_hip
    from sdn_hip import ops
    N, _, H, W = label.shape
    input_label = torch.full((N, label_nc + (inst is not None), H, W), float('nan'), device=DEV)
    pose_onehot = torch.full((N, pose_ch, H, W), float('nan'), device=DEV) if pose_ch else None
    bad = torch.full((2,), -77, dtype=torch.int32, device=DEV)
    dt = lambda t: ops._MAP_DTYPES[t.dtype] if t is not None else 0
    sdn_hip.check(sdn_hip.lib().sdn_encode_maps(sdn_hip.ptr(label), dt(label), sdn_hip.ptr(inst), dt(inst), sdn_hip.ptr(pose), dt(pose), N, H, W,
                                                label_nc, pose_ch, sdn_hip.ptr(input_label), sdn_hip.ptr(pose_onehot), sdn_hip.ptr(bad),
                                                sdn_hip.stream()))
    return input_label, pose_onehot, bad


def _check_encode(gold, name, dt=None, offset=False):
    from models import input_maps
    c = ENCODE[name]
    maps = [None if t is None else (_offset(t.to(DEV)) if offset else t.to(DEV)) for t in u.case_tensors(c, dt)]
    before = [None if t is None else t.clone() for t in maps]
    want = torch.from_numpy(gold['encode/%s/input_label' % name])
    want_pose = torch.from_numpy(gold['encode/%s/pose_onehot' % name]) if c['pose_ch'] else None
    want_bad = gold['encode/%s/bad' % name].tolist()
    for form in (input_maps.encode_maps, _raw_encode):
        input_label, pose_onehot, bad = form(maps[0], maps[1], maps[2], c['label_nc'], c['pose_ch'])
        assert input_label.dtype == torch.float32 and tuple(input_label.shape) == tuple(want.shape)
        wrong = int((input_label.cpu() != want).sum())
        print('%s %s: %d of %d label / edge values differ, bad %s (expected %s)' % (name, form.__name__, wrong, want.numel(), bad.tolist(), want_bad))
        assert wrong == 0 and torch.equal(input_label.cpu(), want)                  # (NaN left in place differs from everything)
        if want_pose is None:
            assert pose_onehot is None
        else:
            assert pose_onehot.dtype == torch.float32 and torch.equal(pose_onehot.cpu(), want_pose)
        assert bad.dtype == torch.int32 and bad.tolist() == want_bad
    for t, b in zip(maps, before):                                                  # the inputs are only read
        assert t is None or torch.equal(t.view(torch.int32 if t.element_size() == 4 else t.dtype), b.view(torch.int32 if b.element_size() == 4 else b.dtype))


# ---- encode_maps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in ENCODE if n not in ('dtypes', 'offset_storage')])
def test_encode_maps_equals_the_torch_expressions(gold, name):
    _check_encode(gold, name)
    if 'want_bad' in ENCODE[name]:
        assert gold['encode/%s/bad' % name].tolist() == ENCODE[name]['want_bad']


def test_encode_maps_on_storage_that_breaks_the_16_byte_alignment(gold):
    """W % 4 == 0, but no base is 16-byte aligned: the scalar path, the same planes"""
    _check_encode(gold, 'offset_storage', offset=True)
    _check_encode(gold, 'offset_storage')
    _check_encode(gold, 'chunk_boundary', offset=True)


@pytest.mark.parametrize('dt', [(a, b, c) for a in u.LABEL_DTYPES for b in u.INST_DTYPES for c in u.POSE_DTYPES], ids='-'.join)
def test_encode_maps_in_every_dtype_combination(gold, dt):
    _check_encode(gold, 'dtypes', dt=dt)


def test_encode_maps_takes_a_strided_map_by_copying_it(gold):
    from models import input_maps
    c = ENCODE['real_channels']
    label, inst, pose = [t.to(DEV) for t in u.case_tensors(c)]
    wide = torch.zeros(2, 1, 16, 48, device=DEV)
    wide[..., ::2] = label
    got = input_maps.encode_maps(wide[..., ::2], inst, pose, 14, 25)
    assert torch.equal(got[0].cpu(), torch.from_numpy(gold['encode/real_channels/input_label']))
    assert not input_maps.encode_maps_supported(wide[..., ::2], inst, pose, 14, 25)   # the wiring leaves such a map to torch
    assert input_maps.encode_maps_supported(label, inst, pose, 14, 25)


# ---- inst_index ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_counts', [False, True], ids=['plain', 'counts'])
@pytest.mark.parametrize('name', sorted(INDEX))
def test_inst_index_equals_torchs_unique(gold, name, with_counts):
    from models import input_maps
    inst0, path = INDEX[name]
    inst = inst0.to(DEV)
    ids, seg, counts, info = input_maps.instance_index(inst, with_counts)
    print('%s: K %d, path %s, overflow %d' % (name, ids.numel(), info['path'], info['overflow']))
    assert info['path'] == path and info['overflow'] == (0 if path == 'device' else 1)
    assert ids.dtype == torch.int64 and seg.dtype == torch.int32 and tuple(seg.shape) == (inst0.shape[0],) + tuple(inst0.shape[2:])
    assert np.array_equal(ids.cpu().numpy(), gold['index/%s/ids' % name])
    assert np.array_equal(seg.cpu().numpy(), gold['index/%s/inverse' % name])
    if with_counts:
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), gold['index/%s/counts' % name])
        assert int(counts.sum()) == inst0.numel()
    else:
        assert counts is None
    # inst was disambiguated in place, as Encoder._disambiguate leaves it (int16: torch's own wraparound)
    assert inst.dtype == inst0.dtype and np.array_equal(inst.cpu().numpy(), gold['index/%s/inst' % name])
    assert torch.equal(ids[seg.long().reshape(-1)], inst.reshape(-1).long())


def test_inst_index_gives_the_same_bits_twice_and_on_offset_storage(gold):
    from models import input_maps
    for name in ('many_workgroups', 'many_workgroups_i16', 'every_pixel_its_own'):
        runs = [input_maps.instance_index(INDEX[name][0].to(DEV), True) for _ in range(2)]
        runs.append(input_maps.instance_index(_offset(INDEX[name][0].to(DEV)), True))        # the scalar kernels
        for ids, seg, counts, info in runs:
            assert info['path'] == 'device'
            assert torch.equal(ids, runs[0][0]) and torch.equal(seg, runs[0][1]) and torch.equal(counts, runs[0][2])
        assert np.array_equal(runs[2][2].cpu().numpy(), gold['index/%s/counts' % name])


def test_inst_index_refuses_a_strided_map():
    from models import input_maps
    wide = torch.zeros(1, 1, 4, 16, device=DEV)
    with pytest.raises(ValueError, match='contiguous'):
        input_maps.instance_index(wide[..., ::2])
    assert not input_maps.instance_index_supported(wide[..., ::2]) and input_maps.instance_index_supported(wide)


# ---- wiring --------------------------------------------------------------------------------------------------------------------------
def _model(opt, seed=31):
    from models.pix2pixHD_model import Pix2PixHDModel
    torch.manual_seed(seed)
    m = Pix2PixHDModel()
    m.initialize(opt)
    return m


def _frame(n=2, h=32, w=48, seed=5):
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    label = torch.from_numpy(rng.randint(0, 14, size=(n, 1, h, w))).float()
    pose = torch.from_numpy(rng.randint(0, 25, size=(n, 1, h, w))).float()
    inst = torch.from_numpy(u._blocky(rng, (n, 1, h, w), (0, 1000, 2000, 3000, 26, 7))).float()
    image, normal = torch.randn(n, 3, h, w, generator=g), torch.randn(n, 3, h, w, generator=g)
    return [t.to(DEV) for t in (label, inst, image, pose, normal)]


def _same(a, b, what):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (what, i))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    else:
        assert a == b, what


def test_the_model_gives_the_same_with_the_device_path_and_without(monkeypatch):
    """encode_input and fake_inference of a small Pix2PixHDModel (label_nc 14, 24 pose bins, normals, instance features) with
    SDN_ENCODE_DEVICE unset and then 0: equal bit for bit"""
    monkeypatch.setenv('SDN_DETERMINISTIC', '1')
    monkeypatch.delenv('SDN_ENCODE_DEVICE', raising=False)
    opt = eu.options(24)
    assert opt.label_nc == 14 and opt.feat_pose_num_bins == 24 and opt.feat_normal and opt.ngf == 8
    m = _model(opt)
    label, inst, image, pose, normal = _frame()
    m.last_encode_bad = None
    on = m.encode_input(label, inst.clone(), image, None, pose, normal)
    assert m.last_encode_bad is not None and m.last_encode_bad.tolist() == [0, 0] and m.last_encode_bad.device.type == 'cuda'
    assert tuple(on[0].shape) == (2, 15, 32, 48) and tuple(on[4].shape) == (2, 25, 32, 48)
    img_on = m.fake_inference(image, label, inst.clone(), pose=pose, normal=normal)
    assert m.netE.last_index_info['path'] == 'device'
    monkeypatch.setenv('SDN_ENCODE_DEVICE', '0')
    m.last_encode_bad = None
    m.netE.last_index_info = None
    off = m.encode_input(label, inst.clone(), image, None, pose, normal)
    img_off = m.fake_inference(image, label, inst.clone(), pose=pose, normal=normal)
    assert m.last_encode_bad is None and m.netE.last_index_info is None                 # the torch expressions ran
    _same(on, off, 'encode_input')
    _same(img_on, img_off, 'fake_inference')
    # the expressions themselves, on the CPU
    want, want_pose, _ = u.encode_reference(label.cpu(), inst.cpu(), pose.cpu(), 14, 25)
    assert torch.equal(on[0].cpu(), want) and torch.equal(on[4].cpu(), want_pose) and torch.equal(on[1], inst)


def test_the_encoder_gives_the_same_with_the_device_path_and_without(monkeypatch):
    monkeypatch.setenv('SDN_DETERMINISTIC', '1')
    monkeypatch.delenv('SDN_ENCODE_DEVICE', raising=False)
    E = _model(eu.options(24)).netE
    _, inst, image, _, _ = _frame()
    res = {}
    for mode in ('on', 'off'):
        if mode == 'off':
            monkeypatch.setenv('SDN_ENCODE_DEVICE', '0')
        E.last_index_info = None
        with torch.no_grad():
            a, b, c = inst.clone(), inst.clone(), inst.clone()
            res[mode] = (E.forward(image, a), E.feat_table(image, b), E.generate_feat_dict(image, c), a, b, c)
        assert (E.last_index_info is not None) == (mode == 'on')
        if mode == 'on':
            assert E.last_index_info['path'] == 'device'
    _same(res['on'], res['off'], 'Encoder')
    ids, means, counts = res['on'][1]
    assert ids.dtype == torch.int64 and counts.dtype == torch.int64 and int(counts.sum()) == inst.numel()
    assert torch.equal(res['on'][3], u.disambiguate_reference(inst.cpu().clone()).to(DEV))      # inst is left disambiguated


def test_an_edit_session_renders_the_same_with_the_device_path_and_without(monkeypatch):
    from edit import EditSession
    monkeypatch.setenv('SDN_DETERMINISTIC', '1')
    monkeypatch.delenv('SDN_ENCODE_DEVICE', raising=False)
    case = {c.name: c for c in eu.cases()}['vkitti24']
    opt = eu.options(case.bins)
    model = _model(opt)
    segm, image, inst0, _, _ = case.source(0)
    frames = []
    for i in range(case.frames):
        ei, js, nrm = case.edit(i)
        frames.append((eu.chw(ei, DEV), js, None if nrm is None else eu.chw(nrm, DEV)))
    out = {}
    for mode in ('on', 'off'):
        if mode == 'off':
            monkeypatch.setenv('SDN_ENCODE_DEVICE', '0')
        model.last_encode_bad = None
        sess = EditSession(model, opt, eu.PARAMS, eu.chw(segm, DEV), eu.chw(image, DEV), eu.chw(inst0, DEV))
        out[mode] = (sess.codes, sess.counts, sess.render_batch(frames))
        assert (model.last_encode_bad is not None) == (mode == 'on')
    _same(out['on'], out['off'], 'EditSession')
