"""The semantic training batch on the device (csrc/segm_train.hip through semantic.train_items) against the reference's results
in tests/golden/segm_train_golden.npz (tests/golden/make_segm_train_golden.py: the installed Pillow and torch's CPU).  Every
comparison is an equality of bits; no tolerance is involved."""
import numpy as np
import pytest
import torch

import segm_train_util as u

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


@pytest.fixture(scope='module')
def small():
    frames, scenes, tables = u.small_inputs()
    return torch.from_numpy(frames).cuda(), torch.from_numpy(scenes).cuda(), tables


@pytest.fixture(scope='module')
def real():
    frames, scenes, tables = u.real_inputs()
    return torch.from_numpy(frames).cuda(), torch.from_numpy(scenes).cuda(), tables


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run_small(small, short, flip):
    from semantic import train_items as st
    flips, jitters = u.small_case(short, flip)
    c = u.SMALL
    return st.segm_train_batch(small[0], small[1], small[2], short, flips, jitters, c['img_max_size'], c['padding_constant'],
                               c['segm_downsampling_rate'], c['frame_size'])


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty that fills what it returns: NaN for floats, 99 for integers -- whatever the call leaves unwritten shows"""
    real_empty = torch.empty

    def empty(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(99)
    monkeypatch.setattr(torch, 'empty', empty)


@pytest.mark.parametrize('short', u.SMALL_SHORTS)
@pytest.mark.parametrize('flip', [False, True])
def test_small_cases_equal_the_fixture(gold, small, poisoned_empty, short, flip):
    out = run_small(small, short, flip)
    p = 'small/%s/' % u.case_name(short, flip)
    Hb, Wb = (int(v) for v in gold[p + 'HbWb'])
    img, lab, unknown = out['img_data'].cpu().numpy(), out['seg_label'].cpu().numpy(), out['unknown'].cpu().numpy()
    assert out['img_data'].dtype == torch.float32 and out['seg_label'].dtype == torch.int64 and out['unknown'].dtype == torch.int32
    assert img.shape == (3, 3, Hb, Wb) and lab.shape == (3, Hb // 8, Wb // 8)
    want = u.expected_img([gold[p + 'px%d' % i] for i in range(3)], gold['lut'], Hb, Wb)
    for i in range(3):
        assert same_bits(img[i], want[i]), 'item %d: %d elements differ' % (i, int((img[i].view(np.uint32) != want[i].view(np.uint32)).sum()))
    assert u.digest(img) == str(gold[p + 'img_sha256'])
    if p + 'img_data' in gold.files:
        assert same_bits(img, gold[p + 'img_data'])
    assert np.array_equal(lab, gold[p + 'seg_label'])
    assert np.array_equal(unknown, gold[p + 'unknown'])
    # the padding: exactly 0 / exactly -1, written by the kernels (the outputs were NaN and 99 before)
    h, w = (int(v) for v in gold[p + 'sizes'][0])
    assert (img[:, :, h:, :] == 0).all() and (img[:, :, :, w:] == 0).all() and not np.isnan(img).any()
    assert (lab[:, (h + 7) // 8:, :] == -1).all() and (lab[:, :, (w + 7) // 8:] == -1).all() and (lab != 99).all()


def test_real_size_case_equals_the_fixture(gold, real, poisoned_empty):
    from semantic import train_items as st
    for short in u.REAL_SHORTS:
        out = st.segm_train_batch(real[0], real[1], real[2], short, list(u.REAL_FLIPS), u.real_jitters(), frame_size=(375, 1242))
        p = 'real/%d/' % short
        Hb, Wb = (int(v) for v in gold[p + 'HbWb'])
        rows = gold[p + 'rows']
        img, lab = out['img_data'].cpu().numpy(), out['seg_label'].cpu().numpy()
        h, w = (int(v) for v in gold[p + 'sizes'][0])
        assert img.shape == (2, 3, Hb, Wb)
        for i in range(2):
            px = gold[p + 'px%d' % i]
            for c in range(3):
                assert same_bits(img[i, c][rows, :w], gold['lut'][c][px[:, :, 2 - c]]), (short, i, c)
        assert (img[:, :, h:, :] == 0).all() and (img[:, :, :, w:] == 0).all() and not np.isnan(img).any()
        assert u.digest(img) == str(gold[p + 'img_sha256'])   # the rows the fixture does not store, through torch's SHA-256
        assert np.array_equal(lab, gold[p + 'seg_label'])
        assert np.array_equal(out['unknown'].cpu().numpy(), gold[p + 'unknown'])


def test_identity_is_the_plain_bgr_normalisation(small):
    from semantic import train_items as st
    frames, scenes, tables = small
    out = st.segm_train_batch(frames, scenes, tables, 45, [False] * 3, None, 170, 8, 8, (45, 150))
    m = torch.tensor(u.MEAN, dtype=torch.float64).float().cuda().view(1, 3, 1, 1)
    s = torch.tensor(u.STD, dtype=torch.float64).float().cuda().view(1, 3, 1, 1)
    want = (frames.permute(0, 3, 1, 2).flip(1).float() - m) / s   # tensor operands: a true fp32 division on the device
    assert torch.equal(out['img_data'][:, :, :45, :150], want)
    assert bool((out['img_data'][:, :, 45:, :] == 0).all()) and bool((out['img_data'][:, :, :, 150:] == 0).all())


def test_two_calls_give_identical_bytes(real):
    from semantic import train_items as st
    a = st.segm_train_batch(real[0], real[1], real[2], 150, [True, False], u.real_jitters())
    b = st.segm_train_batch(real[0], real[1], real[2], 150, [True, False], u.real_jitters())
    for k in ('img_data', 'seg_label', 'unknown'):
        assert torch.equal(a[k].view(torch.uint8 if k == 'img_data' else a[k].dtype), b[k].view(torch.uint8 if k == 'img_data' else b[k].dtype)), k


def test_one_shared_table_serves_all_items(small):
    from semantic import train_items as st
    frames, scenes, tables = small
    table = st.color_table(*tables[2])
    a = st.segm_train_batch(frames, scenes[[2, 2, 2]], table, 33, [False, True, False], None, 170, 8, 8, (45, 150))
    b = st.segm_train_batch(frames, scenes[[2, 2, 2]], [tables[2]] * 3, 33, [False, True, False], None, 170, 8, 8, (45, 150))
    assert torch.equal(a['seg_label'], b['seg_label']) and torch.equal(a['seg_label'][0], a['seg_label'][2])


def test_invalid_arguments_are_refused_before_any_launch(small):
    from sdn_hip import SdnHipError
    from semantic import train_items as st
    frames, scenes, tables = small
    contrast = ([1], (1.0, 1.2, 1.0), 0)
    table = st.color_table(*tables[0])
    big = torch.zeros(1, 1024, 2049, 3, dtype=torch.uint8, device='cuda')
    with pytest.raises(SdnHipError, match='contrast on a frame'):
        st.segm_train_batch(big, big, table, 1024, [False], [contrast], img_max_size=4096)
    wide = torch.zeros(1, 100, 3000, 3, dtype=torch.uint8, device='cuda')   # halved: 5 taps over rows of 1500 bytes, 8 fit a plane
    with pytest.raises(SdnHipError, match='does not fit the LDS plan'):
        st.segm_train_batch(wide, wide, table, 50, [False], None, img_max_size=4000)
    with pytest.raises(ValueError, match='for 3 items'):
        st.segm_train_batch(frames, scenes, tables, 20, [False, False], None, 170, 8, 8, (45, 150))
    with pytest.raises(ValueError, match='for 3 items'):
        st.segm_train_batch(frames, scenes, tables[:2], 20, [False] * 3, None, 170, 8, 8, (45, 150))
    with pytest.raises(ValueError, match='scenes_u8 must be'):
        st.segm_train_batch(frames, scenes[:2], tables, 20, [False] * 3, None, 170, 8, 8, (45, 150))
    many = np.stack([np.arange(1025) % 256, np.arange(1025) // 256, np.zeros(1025, dtype=np.int64)], axis=1)
    with pytest.raises(ValueError, match='at most 1024'):
        st.segm_train_batch(frames, scenes, [(many, np.ones(1025, dtype=np.int64))] * 3, 20, [False] * 3, None, 170, 8, 8, (45, 150))
    packed = np.concatenate((np.arange(1025), np.ones(1025))).astype(np.int32)
    with pytest.raises(SdnHipError, match='1025 colour codes'):
        st.segm_train_batch(frames, scenes, packed, 20, [False] * 3, None, 170, 8, 8, (45, 150))
