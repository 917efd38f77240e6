"""assemble_batch (textural/data/assemble.py; csrc/assemble.hip: sdn_assemble_planes, sdn_assemble_maps) on the device,
bit for bit: the Cityscapes item against the reference loader's fixture (tests/golden/cityscapes_loader_golden.npz), the
VKITTI item against assemble_item on the same device tensors and against loader_golden.npz, a full-size Cityscapes frame
against Pillow executed here and the kernels' numpy emulation, the 255 / 256 pixel boundary, `missing`, and the refusals."""
import json
import os
import sys
from math import cos, sin

import numpy as np
import PIL.Image
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'textural'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cityscapes_loader_util as cu  # noqa: E402
from data import assemble as asm  # noqa: E402

pytestmark = pytest.mark.gpu
Z = cu.load_gold()
KEYS = ('label', 'inst', 'image', 'pose', 'normal')


def _dev(a):
    """a source map as the device tensor assemble_batch takes: uint8 [C, H, W]; the 16-bit ids as int32"""
    if a is None or isinstance(a, dict):
        return a
    if a.dtype == np.uint16:
        a = a.astype(np.int32)
    return torch.from_numpy(a if a.ndim == 3 else a[:, :, None]).permute(2, 0, 1).contiguous().cuda()


def _frame(src):
    return {k: _dev(v) for k, v in src.items()}


def _same(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.dtype, want.shape)
    assert np.array_equal(g, want), '%s differs in %d elements' % (what, int((g != want).sum()))


def _pinned_pose(opt, params, src, recorded):
    """the (cos, sin) planes with the values of THIS host's math.cos / math.sin (what assemble_batch calls), after checking
    that the fixture's recorded values lie within 2 ulp of them"""
    _, _, pose, _, _ = cu.emulate_maps(asm, opt, params, 'cityscapes', src['segm'], src['inst'], src['pose_inst'], src['pose_json'])
    values = {np.float32(f(rec['alpha'])) for rec in src['pose_json'].values() for f in (cos, sin)} | {np.float32(0)}
    assert set(np.unique(pose)) <= values
    assert (np.abs(pose.astype(np.float64) - recorded) <= 2 * np.spacing(np.abs(recorded).astype(np.float32))).all()
    assert ((pose != 0) == (recorded != 0)).all()
    return pose


def _check_case(ci, idx):
    opt, cfg = cu.case_opt(Z, ci)
    items = [cu.case_item(Z, ci, i) for i in idx]
    got = asm.assemble_batch(opt, [p for p, _ in items], [_frame(s) for _, s in items], dataset='cityscapes',
                             inst_wrap_int16=cu.wraps_int16(Z, ci))
    assert got['missing'].dtype == torch.int32 and got['missing'].cpu().tolist() == [0] * len(idx)
    for b, i in enumerate(idx):
        want = cu.case_expected(Z, ci, i)
        if cfg['feat_pose_num_bins'] == 0:
            want['pose'] = _pinned_pose(opt, items[b][0], items[b][1], want['pose'])
        for k in KEYS:
            assert got[k].is_cuda and got[k].shape[0] == len(idx)
            _same(got[k][b], want[k], 'case %d item %d %s' % (ci, i, k))


@pytest.mark.parametrize('ci', range(int(Z['ncases'])))
def test_cityscapes_item_equals_the_reference_loader(ci):
    _check_case(ci, [0])


@pytest.mark.parametrize('ci', [0, 1])
def test_three_cityscapes_items_with_their_own_crops_and_flips_in_one_call(ci):
    crops = {tuple(Z['c%d/i%d/crop_pos' % (ci, i)]) for i in range(3)}
    assert len(crops) == 3
    _check_case(ci, [0, 1, 2])


# ---------------------------------------------------------------------------------------------------------------------
def _vk_frame(seed, H, W):
    rng = np.random.default_rng(seed)
    segm = rng.integers(0, 14, (H, W), dtype=np.uint8)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    normal = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    inst = np.zeros((H, W), dtype=np.uint8)
    js = {}
    for k in range(1, 7):
        y0, x0 = int(rng.integers(0, H - H // 4)), int(rng.integers(0, W - W // 4))
        inst[y0:y0 + int(rng.integers(2, H // 4 + 1)), x0:x0 + int(rng.integers(2, W // 4 + 1))] = k
        if k != 5:   # one instance without a pose record
            js[str(k)] = {'class_id': 1, 'depth': 10.0, 'alpha': float(rng.uniform(-np.pi, np.pi))}
    js['77'] = {'class_id': 1, 'depth': 1.0, 'alpha': 0.3}
    return {'segm': segm, 'image': image, 'inst': inst, 'pose_inst': inst, 'pose_json': js, 'normal': normal}


_VK = {}


def _vk(size):
    """the device frames of one size and their B = 2 companions, made once"""
    if size not in _VK:
        H, W = size
        _VK[size] = [_frame(_vk_frame(H + s, H, W)) for s in range(2)]
    return _VK[size]


SIZES = {'small': ((37, 83), dict(loadSize=40, fineWidth=24, fineHeight=16)),
         'vkitti': ((375, 1242), dict(loadSize=624, fineWidth=624, fineHeight=192))}   # 188 -> 192, the reference's hack


# the precomputed branches do not depend on the geometry: one mode covers them
VK_CASES = [(size, roc, flip, pre) for size in ('small', 'vkitti') for roc in ('scale_width_and_crop', 'resize_and_crop', 'crop', 'none')
            for flip in (False, True) for pre in (False, True) if not pre or roc == 'scale_width_and_crop']


@pytest.mark.parametrize('size,roc,flip,pre', VK_CASES)
def test_vkitti_items_equal_assemble_item(size, roc, flip, pre):
    from test_assemble import _opt
    (H, W), geo = SIZES[size]
    opt = _opt(resize_or_crop=roc, segm_precomputed_path='p' if pre else '', inst_precomputed_path='q' if pre else '',
               feat_pose_num_bins=0 if pre and flip else 24, **geo)
    sh, sw, h, w, crops = asm.batch_geometry(opt, H, W)
    # the first item's box lies inside the scaled image, the second reaches past its right and lower edge
    params = [{'crop_pos': (max(0, sw - w) // 3, max(0, sh - h) // 2), 'flip': flip},
              {'crop_pos': (max(0, sw - w) + 5, max(0, sh - h) + 3), 'flip': not flip}]
    frames = _vk((H, W))
    frames = [frames[0], dict(frames[1], inst=None if pre else frames[1]['inst'], normal=None)]
    got = asm.assemble_batch(opt, params, frames, dataset='vkitti')
    assert tuple(got['image'].shape) == (2, 3, h, w)
    for b in range(2):
        f = frames[b]
        want = asm.assemble_item(opt, params[b], f['segm'], f['image'], f['inst'], f['pose_inst'], f['pose_json'], f['normal'])
        for k in KEYS:
            assert got[k][b].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
            assert torch.equal(got[k][b], want[k]), '%s of item %d differs in %d elements' % (k, b, int((got[k][b] != want[k]).sum()))


@pytest.mark.parametrize('ci', range(10))
def test_vkitti_items_equal_the_reference_loader_golden(ci):
    """every case of loader_golden.npz; of case 8 (--feat_depth) everything but `depth`, which stays with depth_feature"""
    from test_assemble import GOLD, _opt
    z = np.load(GOLD)
    assert int(z['ncases']) == 10
    p = 'c%d/' % ci
    cfg = json.loads(str(z[p + 'cfg']))
    opt = _opt(**{k: v for k, v in cfg.items() if k in cu.OPT_KEYS})
    opt.segm_precomputed_path = 'p' if cfg['segm_precomputed'] else ''
    opt.inst_precomputed_path = 'q' if cfg['inst_precomputed'] else ''
    opt.feat_pose = 'x' if cfg['pose'] else ''
    opt.feat_normal = 'x' if cfg['normal'] else ''
    params = {'crop_pos': (int(z[p + 'crop_pos'][0]), int(z[p + 'crop_pos'][1])), 'flip': bool(z[p + 'flip'])}
    frame = _frame({'segm': z[p + 'src_segm'], 'image': z[p + 'src_rgb'], 'inst': z[p + 'src_instmap'],
                    'pose_inst': z[p + 'src_instmap'] if cfg['pose'] else None, 'pose_json': json.loads(str(z[p + 'json'])),
                    'normal': z[p + 'src_normalmap'] if cfg['normal'] else None})
    got = asm.assemble_batch(opt, [params], [frame], dataset='vkitti')
    for k in KEYS:
        want = z[p + k]
        if want.shape == ():      # the loader's default: no instance map asked for, no pose / normal feature
            assert isinstance(got[k], int) and got[k] == int(want), k
        elif k == 'pose' and cfg['feat_pose_num_bins'] == 0:
            # (cos, sin) of the host's libm: within 2 ulp of the recorded values, and exactly assemble_item's on this host
            g = got[k][0].cpu().numpy()
            assert g.dtype == want.dtype and (np.abs(g.astype(np.float64) - want) <= 2 * np.spacing(np.abs(want))).all()
            item = asm.assemble_item(opt, params, frame['segm'], frame['image'], frame['inst'], frame['pose_inst'],
                                     frame['pose_json'], frame['normal'])
            assert torch.equal(got[k][0], item[k])
        else:
            _same(got[k][0], want, 'case %d %s' % (ci, k))


# ---------------------------------------------------------------------------------------------------------------------
def test_a_full_size_cityscapes_frame_equals_pillow_and_the_emulation():
    """1024 x 2048 scaled to width 1024, a 512 x 1024 crop: 9 taps per axis, 23 source rows of 1024 bytes per band of 8 output
    rows -- the Cityscapes size; a band still fits the 32 KiB tile (32 rows) here, the sub-bands have their own test below."""
    from test_assemble import _opt
    H, W = 1024, 2048
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H, 0:W]
    segm = ((y // 37 + x // 53) % 35).astype(np.uint8)
    segm[segm == 34] = 40
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    normal = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pose = np.zeros((H, W), dtype=np.uint8)
    js = {}
    for k in range(1, 12):
        y0, x0 = int(rng.integers(0, H - 200)), int(rng.integers(0, W - 400))
        pose[y0:y0 + int(rng.integers(10, 200)), x0:x0 + int(rng.integers(10, 400))] = k
        js[str(k)] = {'alpha': float(rng.uniform(-np.pi, np.pi))}
    inst = segm.astype(np.uint16)
    inst[pose > 0] = 26000 + pose[pose > 0].astype(np.uint16) * 700     # ids up to 33 700: above 32 767
    opt = _opt(loadSize=1024, fineWidth=1024, fineHeight=512, label_nc=20)
    params = {'crop_pos': (0, 0), 'flip': True}
    src = {'segm': segm, 'image': image, 'inst': inst, 'pose_inst': pose, 'pose_json': js, 'normal': normal}
    got = asm.assemble_batch(opt, [params], [_frame(src)], dataset='cityscapes', inst_wrap_int16=True)
    want = cu.cityscapes_item(opt, params, cu.pil(segm), cu.pil(image), cu.pil(inst), cu.pil(pose), js, cu.pil(normal),
                              label_table=asm.CITYSCAPES_LABEL_TABLE)
    assert want['inst'].dtype == torch.int16 and int(want['inst'].min()) < 0 and int(want['pose'].max()) > 0
    for k in KEYS:
        _same(got[k][0], want[k].numpy(), k)
    emu = cu.emulate_planes(asm, opt, params, np.ascontiguousarray(image.transpose(2, 0, 1)[:1]))
    _same(got['image'][0, :1], emu, 'image plane 0 (emulation)')
    assert got['missing'].cpu().tolist() == [0]


def test_a_window_too_wide_for_a_band_is_walked_in_sub_bands():
    """64 x 4000 scaled to width 2000 (32 rows), a 28 x 1990 window: 9 taps and two source rows per output row, so a band of 8
    rows needs 23 source rows and the 32 KiB tile holds 16 of 1990 bytes -- every band is walked in two sub-bands.  The second
    item's box starts at (15, 9): its columns from 1985 on lie past the image, its band of rows 16..23 ends at row 22 (a short
    last sub-band, then zero fill) and its band of rows 24..27 lies wholly past the image.  Against Pillow, executed here."""
    from oracle import loader_oracle as lo
    from test_assemble import _opt
    H, W = 64, 4000
    opt = _opt(loadSize=2000, fineWidth=1990, fineHeight=28, no_instance=True, feat_pose='', feat_normal='x')
    assert asm.batch_geometry(opt, H, W) == (32, 2000, 28, 1990, True) and asm._resample_table(H, 32, 'bicubic')[0].shape[1] == 9
    rng = np.random.default_rng(11)
    srcs = [{'segm': rng.integers(0, 14, (H, W), dtype=np.uint8), 'image': rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
             'normal': rng.integers(0, 256, (H, W, 3), dtype=np.uint8)} for _ in range(2)]
    params = [{'crop_pos': (3, 0), 'flip': False}, {'crop_pos': (15, 9), 'flip': True}]
    got = asm.assemble_batch(opt, params, [_frame(s) for s in srcs], dataset='vkitti')
    for b in range(2):
        t = lo.get_transform(opt, params[b])
        _same(got['image'][b], t(cu.pil(srcs[b]['image'])).numpy(), 'image of item %d' % b)
        _same(got['normal'][b], (t(cu.pil(srcs[b]['normal'])) + 1 / 255).numpy(), 'normal of item %d' % b)
        _same(got['label'][b], (lo.get_transform(opt, params[b], PIL.Image.NEAREST, False)(cu.pil(srcs[b]['segm'])) * 255.0).numpy(),
              'label of item %d' % b)
    assert (got['image'][1, :, 23:] == -1.0).all() and (got['image'][1, :, :23, :5] == -1.0).all()   # flipped: the fill is left


@pytest.mark.parametrize('shape', [(96, 128, 96, 80, 64), (64, 48, 48, 40, 36)])
def test_a_16_bit_instance_map_resized_on_one_axis_equals_pillow(shape):
    """`resize_and_crop` with loadSize equal to the height (the width alone shrinks, 128 -> 96) or to the width (the height
    alone, 64 -> 48): Pillow resizes the mode 'I;16' map by its generic transform all the same, and at these ratios its indices
    differ from ImagingScaleAffine's.  Against the restatement on real PIL images."""
    from test_assemble import _opt
    H, W, load, fw, fh = shape
    opt = _opt(resize_or_crop='resize_and_crop', loadSize=load, fineWidth=fw, fineHeight=fh, label_nc=20, feat_pose='')
    rng = np.random.default_rng(H)
    srcs = []
    for _ in range(2):
        segm = rng.integers(0, 34, (H, W), dtype=np.uint8)
        inst = rng.integers(0, 40000, (H, W)).astype(np.uint16)
        srcs.append({'segm': segm, 'image': rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 'inst': inst, 'pose_inst': None,
                     'pose_json': None, 'normal': rng.integers(0, 256, (H, W, 3), dtype=np.uint8)})
    params = [{'crop_pos': (2, 5), 'flip': True}, {'crop_pos': (load - fw + 3, load - fh), 'flip': False}]
    got = asm.assemble_batch(opt, params, [_frame(s) for s in srcs], dataset='cityscapes', inst_wrap_int16=True)
    for b in range(2):
        s = srcs[b]
        want = cu.cityscapes_item(opt, params[b], cu.pil(s['segm']), cu.pil(s['image']), cu.pil(s['inst']), None, None,
                                  cu.pil(s['normal']), label_table=asm.CITYSCAPES_LABEL_TABLE)
        assert want['inst'].dtype == torch.int16
        for k in ('label', 'inst', 'image', 'normal'):
            _same(got[k][b], want[k].numpy(), '%s of item %d' % (k, b))


def test_an_absent_integer_instance_map_is_zero_of_the_output_type():
    """sdn_assemble_maps with inst_mode 3 and an address of 0: the item's inst is 0 in the integer output (int16 with wrap16),
    never the fp32 label stored into the narrower buffer; the item after it is untouched by the one before.  assemble_batch
    itself refuses the mix (the loader would return tensors of two types)."""
    from sdn_hip import ops
    H, W = 20, 30
    rng = np.random.default_rng(3)
    segm = torch.from_numpy(rng.integers(1, 14, (3, H, W), dtype=np.uint8)).cuda()
    inst = torch.from_numpy(rng.integers(1, 40000, (H, W)).astype(np.int32)).cuda()
    items = np.zeros((3, 4), dtype=np.int32)
    tabs = torch.arange(256, dtype=torch.float32).repeat(4, 1).cuda()
    addr = lambda ts: torch.tensor([0 if t is None else t.data_ptr() for t in ts], dtype=torch.int64).cuda()
    for wrap in (True, False):
        label, out, _, _ = ops.assemble_maps(addr(list(segm)), addr([inst, None, inst]), None, items, torch.from_numpy(items).cuda(),
                                             None, None, tabs, ops.ASSEMBLE_INST_INT, H, W, H, W, H, W, wrap16=wrap)
        want = inst.to(torch.int16) if wrap else inst
        assert out.dtype == want.dtype and torch.equal(out[0, 0], want) and torch.equal(out[2, 0], want)
        assert int(out[1].abs().max()) == 0 and torch.equal(label[:, 0], segm.float())
    opt, params, src = _boundary_case()
    opt.inst_precomputed_path = ''
    a = _frame(dict(src, inst=Z['f0/inst16']))
    with pytest.raises(ValueError, match='separate calls'):
        asm.assemble_batch(opt, [params, params], [a, dict(a, inst=None)], dataset='cityscapes', inst_wrap_int16=True)


# ---------------------------------------------------------------------------------------------------------------------
def _boundary_case(drop=()):
    opt, _ = cu.case_opt(Z, 3)          # val, central crop: pose ids 1 and 2 cover exactly 256 and 255 transformed pixels
    opt.feat_pose_num_bins = 24
    params, src = cu.case_item(Z, 0, 0)
    params = {'crop_pos': (16, 8), 'flip': False}
    js = {k: v for k, v in src['pose_json'].items() if k not in drop}
    return opt, params, dict(src, pose_json=js)


@pytest.mark.parametrize('dataset,painted', [('cityscapes', (1,)), ('vkitti', (1, 2))])
def test_an_instance_of_255_pixels_gets_no_pose_one_of_256_does(dataset, painted):
    opt, params, src = _boundary_case()
    got = asm.assemble_batch(opt, [params], [_frame(src)], dataset=dataset)
    *_, counts = cu.emulate_maps(asm, opt, params, dataset, src['segm'], src['inst'], src['pose_inst'], src['pose_json'])
    assert counts[1] == 256 and counts[2] == 255
    from types import SimpleNamespace
    plain = SimpleNamespace(**dict(vars(opt), segm_precomputed_path='', inst_precomputed_path=''))
    ids = cu.emulate_maps(asm, plain, params, 'vkitti', src['pose_inst'])[0][0]     # the transformed id map, as floats
    pose = got['pose'][0, 0].cpu().numpy()
    bins = asm.pose_bins(24)
    for k in (1, 2):
        want = int(np.digitize(src['pose_json'][str(k)]['alpha'] / np.pi, bins)) if k in painted else 0
        assert (ids == k).sum() == (256 if k == 1 else 255)
        assert (pose[ids == k] == want).all(), (k, want)
    assert got['missing'].cpu().tolist() == [0]


def test_missing_counts_the_pixels_of_large_instances_without_a_record():
    opt, params, full = _boundary_case()
    _, _, no1 = _boundary_case(drop=('1',))      # 256 pixels: large enough, no record -> counted, painted 0
    _, _, no2 = _boundary_case(drop=('2',))      # 255 pixels: skipped before the look-up -> not counted
    got = asm.assemble_batch(opt, [params] * 3, [_frame(no1), _frame(full), _frame(no2)], dataset='cityscapes')
    assert got['missing'].cpu().tolist() == [256, 0, 0]
    assert torch.equal(got['pose'][1], got['pose'][2])
    differ = (got['pose'][0] != got['pose'][1]).sum().item()
    assert differ == 256 and int(got['pose'][0][got['pose'][0] != got['pose'][1]].abs().max()) == 0
    vk = asm.assemble_batch(opt, [params], [_frame(no2)], dataset='vkitti')      # min_area 1: id 2 has no record either
    assert vk['missing'].cpu().tolist() == [255]


# ---------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    opt, params, src = _boundary_case()
    frame = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in _frame(src).items()}
    with pytest.raises(NotImplementedError):
        asm.assemble_batch(opt, [params], [frame], dataset='cityscapes')


def test_frames_of_different_sizes_are_refused_before_any_launch():
    opt, params, src = _boundary_case()
    a = _frame(src)
    b = {k: (v[:, :60].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
    with pytest.raises(ValueError, match='source size'):
        asm.assemble_batch(opt, [params, params], [a, b], dataset='cityscapes')
    with pytest.raises(ValueError, match='dataset'):
        asm.assemble_batch(opt, [params], [a], dataset='kitti')


def test_a_window_whose_rows_do_not_fit_the_lds_tile_is_refused_with_a_message():
    """20 x 6010 scaled to width 6000 (19 rows): 7 source rows of 6000 bytes per output row, the 32 KiB tile holds 5"""
    import sdn_hip
    from test_assemble import _opt
    opt = _opt(resize_or_crop='scale_width', loadSize=6000, feat_pose='', feat_normal='', no_instance=True)
    frame = {'segm': torch.zeros(1, 20, 6010, dtype=torch.uint8, device='cuda'),
             'image': torch.zeros(3, 20, 6010, dtype=torch.uint8, device='cuda')}
    with pytest.raises(sdn_hip.SdnHipError, match='LDS tile'):
        asm.assemble_batch(opt, [{'crop_pos': (0, 0), 'flip': False}], [frame], dataset='vkitti')
