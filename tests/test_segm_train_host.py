"""The semantic training batch without a GPU: the host arithmetic of semantic.train_items (batch_sizes, the composed label
gather, Pillow's tables as the kernel reads them) against tests/golden/segm_train_golden.npz, which the installed Pillow and
torch's CPU made (tests/golden/make_segm_train_golden.py), and the argument checks that run before any launch."""
import numpy as np
import pytest
import torch

import segm_train_util as u

from semantic import train_items as st  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return np.load(u.GOLD)


def jitters_of(gold, prefix):
    out = []
    for i in range(len(gold[prefix + 'present'])):
        if not gold[prefix + 'present'][i]:
            out.append(None)
            continue
        order = [int(o) for o in gold[prefix + 'order'][i] if o >= 0]
        out.append((order, tuple(float(f) for f in gold[prefix + 'factors'][i]), int(gold[prefix + 'shift'][i])))
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_the_seeded_inputs_and_parameters_are_the_fixtures(gold):
    frames, scenes, tables = u.small_inputs()
    assert np.array_equal(frames, gold['small/frames']) and np.array_equal(scenes, gold['small/scenes'])
    for i, (codes, labels) in enumerate(tables):
        assert np.array_equal(codes, gold['small/codes%d' % i]) and np.array_equal(labels, gold['small/labels%d' % i])
    assert jitters_of(gold, 'small/jitter_') == u.small_jitters()
    assert jitters_of(gold, 'real/jitter_') == u.real_jitters()
    orders = [tuple(j[0]) for j in u.small_jitters() if j is not None]
    assert len({o for o in orders if len(o) == 4}) == 24 and any(j is None for j in u.small_jitters())
    assert any(o[0] == 1 for o in orders)   # contrast first


@pytest.mark.parametrize('short', u.SMALL_SHORTS)
@pytest.mark.parametrize('flip', [False, True])
def test_numpy_restatement_equals_the_fixture_small(gold, short, flip):
    frames, scenes, tables = u.small_inputs()
    flips, jitters = u.small_case(short, flip)
    r = u.host_batch(frames, scenes, tables, short, flips, jitters, u.SMALL)
    p = 'small/%s/' % u.case_name(short, flip)
    assert np.array_equal(r['sizes'], gold[p + 'sizes']) and [r['Hb'], r['Wb']] == list(gold[p + 'HbWb'])
    for i in range(u.SMALL['B']):
        assert np.array_equal(r['px'][i], gold[p + 'px%d' % i]), 'item %d' % i
    assert u.digest(r['img_data']) == str(gold[p + 'img_sha256'])
    assert same_bits(r['img_data'], u.expected_img([gold[p + 'px%d' % i] for i in range(3)], gold['lut'], r['Hb'], r['Wb']))
    if p + 'img_data' in gold.files:
        assert same_bits(r['img_data'], gold[p + 'img_data'])
    # the composed label formula against the two Pillow calls on the padded array
    assert r['seg_label'].dtype == np.int64 and np.array_equal(r['seg_label'], gold[p + 'seg_label'])
    assert np.array_equal(r['unknown'], gold[p + 'unknown'])
    h = int(r['sizes'][0, 0])
    if h % 8:   # the last label row of an item whose height is no multiple of the rate samples the padding
        assert (r['seg_label'][:, (h + 7) // 8 - 1:] == -1).all() == (8 * (h // 8) + 4 >= h)


def test_two_small_cases_hold_the_whole_fp32_tensor(gold):
    assert sum(1 for k in gold.files if k.startswith('small/') and k.endswith('/img_data')) == 2


def test_numpy_restatement_equals_the_fixture_real_size(gold):
    frames, scenes, tables = u.real_inputs()
    assert u.digest(frames, scenes, *[a for t in tables for a in t]) == str(gold['real/inputs_sha256'])
    for short in u.REAL_SHORTS:
        r = u.host_batch(frames, scenes, tables, short, list(u.REAL_FLIPS), u.real_jitters(), u.REAL)
        p = 'real/%d/' % short
        rows = gold[p + 'rows']
        assert np.array_equal(r['sizes'], gold[p + 'sizes']) and [r['Hb'], r['Wb']] == list(gold[p + 'HbWb'])
        for i in range(2):
            assert np.array_equal(r['px'][i][rows], gold[p + 'px%d' % i]), (short, i)
        assert u.digest(r['img_data']) == str(gold[p + 'img_sha256'])
        assert np.array_equal(r['seg_label'], gold[p + 'seg_label']) and np.array_equal(r['unknown'], gold[p + 'unknown'])
    assert tuple(gold['real/300/rows']) == u.REAL_ROWS_300 and len(gold['real/100/rows']) == 100


def test_batch_sizes_equal_the_fixture(gold):
    for s in u.DEFAULT_SHORTS:
        sizes, Hb, Wb = st.batch_sizes(s, 2)
        assert sizes.dtype == np.int32 and np.array_equal(sizes, gold['default/%d/sizes' % s])
        assert [Hb, Wb] == list(gold['default/%d/HbWb' % s])
    assert st.batch_sizes(375, 1)[1:] == (376, 1248) and st.batch_sizes(300, 1)[0].tolist() == [[300, 993]]
    for short in u.SMALL_SHORTS:
        sizes, Hb, Wb = st.batch_sizes(short, 3, 170, 8, 8, (45, 150))
        p = 'small/%s/' % u.case_name(short, False)
        assert np.array_equal(sizes, gold[p + 'sizes']) and [Hb, Wb] == list(gold[p + 'HbWb'])
    with pytest.raises(ValueError, match='padding constant'):
        st.batch_sizes(300, 2, padding_constant=4, segm_downsampling_rate=8)
    with pytest.raises(ValueError):
        st.batch_sizes(300, 0)


def test_draw_item_draws_from_the_given_generators():
    import random
    short, flip, jit = st.draw_item([100, 150, 200], rng=random.Random(3), nprng=np.random.RandomState(3))
    assert short in (100, 150, 200) and isinstance(flip, bool)
    order, factors, shift = jit
    assert sorted(order) == [0, 1, 2, 3] and all(0.8 <= f <= 1.2 for f in factors) and 0 <= shift <= 255
    assert st.draw_item(300, random_flip=False, jitter=None)[:2] == (300, False)
    assert st.draw_item(300, jitter=None)[2] == st.NO_JITTER
    from derender3d import train_items as geo
    from sdn_hip import pillow
    assert st.jitter_params is geo.jitter_params is pillow.jitter_params   # one helper, not a copy
    import semantic
    for name in ('batch_sizes', 'draw_item', 'segm_train_batch'):
        assert getattr(semantic, name) is getattr(st, name)


def test_table_buffer_holds_every_table_once(gold):
    _, _, tables = u.small_inputs()
    tabs = st._as_tables(tables, 3)
    sizes = gold['small/s20n/sizes']
    flips, jitters = u.small_case(20, False)
    buf = st.table_buffer(sizes, tabs, flips, jitters, 45, 150)
    rows = buf[:3 * st.ITEM_INTS].reshape(3, st.ITEM_INTS)
    assert buf.dtype == np.int32 and (rows[:, 0] == 20).all() and (rows[:, 1] == 66).all()
    assert len(set(rows[:, 9])) == 1 and len(set(rows[:, 15])) == 1 and len(set(rows[:, 17])) == 3   # shared tables, own colours
    assert rows[0, 11] == 2 * 3 + 1 and rows[0, 14] == 2 * 3 + 1   # 150 / 66 and 45 / 20 round up to 3
    same = st.table_buffer(gold['small/s45n/sizes'], tabs, flips, jitters, 45, 150)[:60].reshape(3, 20)
    assert (same[:, 9:15] == 0).all()   # no resample: Pillow skips both passes
    one = st._as_tables(tabs[0], 3)
    assert all(t is one[0] for t in one)
    with pytest.raises(ValueError, match='permutation'):
        st.table_buffer(sizes, tabs, flips, [([1, 1], (1, 1, 1), 0)] * 3, 45, 150)
    with pytest.raises(ValueError, match='hue shift'):
        st.table_buffer(sizes, tabs, flips, [([3], (1, 1, 1), 256)] * 3, 45, 150)


def test_cpu_tensors_and_bad_arguments_raise():
    frames = torch.zeros(2, 45, 150, 3, dtype=torch.uint8)
    table = st.color_table(np.array([[0, 0, 0]]), np.array([1]))
    with pytest.raises(NotImplementedError):
        st.segm_train_batch(frames, frames, table, 20, [False, False], None)
    with pytest.raises(TypeError):
        st.segm_train_batch(frames.numpy(), frames, table, 20, [False, False], None)


# ---- the C entry point's checks: they run on the HOST copy of the tables, before any launch, so they need no GPU -----------------
def _call(buf, B, H, W, Hb, Wb, rate=8, workspace=1 << 20):
    import sdn_hip
    L = sdn_hip.lib()
    fake = 0x10000   # never dereferenced: every case below is refused first
    rc = L.sdn_segm_train_batch(fake, fake, B, H, W, buf.ctypes.data, fake, buf.size, Hb, Wb, rate, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, fake,
                                workspace, fake, fake, fake, None)
    return rc, L.sdn_last_error().decode()


def _buffer(H, W, h, w, jitter=None, K=2, B=1):
    table = np.concatenate((np.arange(K), np.ones(K))).astype(np.int32)
    return st.table_buffer(np.array([[h, w]] * B), [table] * B, [False] * B, [jitter] * B, H, W)


def test_the_entry_point_refuses_bad_tables_before_any_launch():
    contrast = ([1], (1.0, 1.2, 1.0), 0)
    rc, msg = _call(_buffer(1024, 2049, 1024, 2049, contrast), 1, 1024, 2049, 1024, 2056)
    assert rc != 0 and 'contrast on a frame of 2098176 pixels' in msg
    rc, msg = _call(_buffer(375, 1242, 375, 1242, contrast), 1, 375, 1242, 376, 1248, workspace=10)
    assert rc != 0 and 'workspace' in msg
    rc, msg = _call(_buffer(4000, 3000, 400, 3000), 1, 4000, 3000, 400, 3000)   # 21 taps over rows of 3000 bytes
    assert rc != 0 and 'does not fit the LDS plan' in msg
    rc, msg = _call(_buffer(100, 5000, 100, 5000), 1, 100, 5000, 104, 5000)
    assert rc != 0 and 'staging tile' in msg
    rc, msg = _call(_buffer(45, 150, 20, 66, K=1025), 1, 45, 150, 24, 72)
    assert rc != 0 and '1025 colour codes' in msg
    good = _buffer(45, 150, 20, 66, B=2)
    rc, msg = _call(good, 3, 45, 150, 24, 72)   # three rows would overlap the tables of a buffer made for two
    assert rc != 0 and 'outside the buffer' in msg
    for col, value, reason in ((0, 25, 'resized to'), (2, 2, 'flip'), (3, 5, 'ops'), (4, 0x11, 'permutation'), (8, 256, 'hue'),
                               (11, 5, 'taps'), (9, 7, 'outside the buffer'), (15, 10 ** 6, 'NEAREST'), (17, -4, 'colour table')):
        bad = good.copy()
        bad[20 + col] = value
        if col == 4:
            bad[20 + 3] = 2
        rc, msg = _call(bad, 2, 45, 150, 24, 72)
        assert rc != 0 and 'item 1' in msg and reason in msg, (col, msg)
    bad = good.copy()
    bad[bad[20 + 9] + 1] = 9   # a bound that reads beyond its taps
    rc, msg = _call(bad, 2, 45, 150, 24, 72)
    assert rc != 0 and 'bounds of output 0' in msg
    bad = good.copy()
    bad[bad[20 + 16] + 3] = 45   # a NEAREST row outside the frame
    rc, msg = _call(bad, 2, 45, 150, 24, 72)
    assert rc != 0 and 'reads row 45' in msg
    rc, msg = _call(good, 2, 45, 150, 16, 72)   # the batch is lower than the items
    assert rc != 0 and 'resized to' in msg


def test_the_label_map_must_hold_the_items_labels():
    # padding 12 and rate 8: an item 9 high rounds to 16 rows = 2 label rows, the batch of 12 rows holds 1; the reference fails too
    rc, msg = _call(_buffer(45, 150, 9, 30), 1, 45, 150, 12, 36)
    assert rc != 0 and 'do not fit' in msg
