"""Shared by tests/test_encode_input_host.py, tests/test_gpu_encode_input.py and tests/golden/make_encode_input_golden.py: the
cases of the textural input encoding (csrc/encode_input.hip), a torch-CPU restatement of what it replaces -- the expressions of
Pix2PixHDModel.encode_input / get_edges, and Encoder._disambiguate + torch.unique(sorted, return_inverse, return_counts) -- and a
numpy emulation of the bitmap / prefix / rank arithmetic of csrc/encode_input_check.h.  Everything here is exact: the tests
compare with equality."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encode_input_golden.npz')
KEY_MIN, KEY_BITS = -32768, 1 << 21                      # csrc/encode_input_check.h: IDX_KEY_MIN, IDX_BITS
KEY_LAST = KEY_MIN + KEY_BITS - 1
ENC_THREADS = 256                                        # csrc/encode_input_check.h: a workgroup's lanes, 4 pixels each (vector path)
TORCH = {'u8': torch.uint8, 'i16': torch.int16, 'i32': torch.int32, 'f32': torch.float32}
LABEL_DTYPES, INST_DTYPES, POSE_DTYPES = ('u8', 'i32', 'f32'), ('i16', 'i32', 'f32'), ('i32', 'f32')
NAN = float('nan')


# ---- the torch expressions ---------------------------------------------------------------------------------------------------------
def one_hot_reference(index_map, channels):
    """Pix2PixHDModel._one_hot (pix2pixHD_model.py:128-131: zeros, long, scatter_) on the CPU -> (planes fp32, bad).  Where the
    index lies outside [0, channels) or is NaN the reference has no answer (scatter_ raises on the CPU and asserts on the
    device); those pixels keep all planes 0 and are counted, and every other pixel goes through the reference's expression."""
    n, _, h, w = index_map.shape
    if index_map.is_floating_point():
        ok = (index_map > -1) & (index_map < channels)        # trunc(v) in [0, channels); NaN fails both
        index = torch.where(ok, index_map, torch.zeros_like(index_map)).long()
    else:
        index = index_map.long()
        ok = (index >= 0) & (index < channels)
        index = torch.where(ok, index, torch.zeros_like(index))
    out = torch.zeros(n, channels, h, w, dtype=torch.float32)
    if bool(ok.all()):
        return out.scatter_(1, index, 1.0), 0
    return out.scatter_(1, index, ok.float()), int((~ok).sum())


def get_edges_reference(t):
    """get_edges (pix2pixHD_model.py:343-349), the four in-place ORs, as the product's method states them"""
    edge = torch.zeros(t.shape, dtype=torch.bool)
    dx = t[:, :, :, 1:] != t[:, :, :, :-1]
    dy = t[:, :, 1:, :] != t[:, :, :-1, :]
    edge[:, :, :, 1:] |= dx
    edge[:, :, :, :-1] |= dx
    edge[:, :, 1:, :] |= dy
    edge[:, :, :-1, :] |= dy
    return edge.float()


def encode_reference(label, inst, pose, label_nc, pose_ch):
    """-> (input_label, pose_onehot or None, [bad_label, bad_pose]) of CPU maps, by the expressions of encode_input"""
    input_label, bad_label = one_hot_reference(label, label_nc)
    if inst is not None:
        input_label = torch.cat((input_label, get_edges_reference(inst)), dim=1)
    pose_onehot, bad_pose = (None, 0) if pose is None else one_hot_reference(pose, pose_ch)
    return input_label, pose_onehot, [bad_label, bad_pose]


def disambiguate_reference(inst):
    """Encoder._disambiguate (networks.py:313-316) in place on a CPU tensor, in its own dtype"""
    bs = inst.size(0)
    for i in range(bs):
        inst[i] = inst[i] * bs + i
    return inst


def index_reference(inst):
    """-> (the disambiguated map, ids int64, inverse int32 [N, H, W], counts int64) of a CPU map, by torch's own unique"""
    d = disambiguate_reference(inst.clone())
    ids, inverse, counts = torch.unique(d.reshape(-1).long(), sorted=True, return_inverse=True, return_counts=True)
    n, _, h, w = inst.shape
    return d, ids, inverse.to(torch.int32).reshape(n, h, w), counts


# ---- the bitmap / prefix / rank scheme, emulated -------------------------------------------------------------------------------------
def emulate_index(disambiguated):
    """The scheme of k_inst_mark / k_inst_scan / k_inst_rank on a numpy array of disambiguated values -> (ids int64, seg int32,
    counts int64, overflow): presence bits of key - KEY_MIN in 32-bit words, the words' exclusive popcount prefix, the rank of a
    key = prefix[word] + popcount(bits below).  Keys outside the window (NaN, Inf) get seg -1 and are counted in overflow."""
    v = np.asarray(disambiguated)
    flat = v.reshape(-1)
    if flat.dtype.kind == 'f':
        inside = (flat > np.float32(KEY_MIN - 1)) & (flat < np.float32(KEY_MIN + KEY_BITS))
        keys = np.where(inside, flat, 0).astype(np.int64)      # truncation toward zero
    else:
        keys = flat.astype(np.int64)
        inside = (keys >= KEY_MIN) & (keys <= KEY_LAST)
    bit = np.where(inside, keys - KEY_MIN, 0)
    words = np.zeros(KEY_BITS // 32, dtype=np.uint32)
    np.bitwise_or.at(words, bit[inside] >> 5, (np.uint32(1) << (bit[inside] & 31).astype(np.uint32)))
    pop = np.array([bin(int(x)).count('1') for x in words[words != 0]], dtype=np.int64)
    popc = np.zeros(words.size, dtype=np.int64)
    popc[words != 0] = pop
    prefix = np.cumsum(popc) - popc
    K = int(popc.sum())
    ids = np.array([w * 32 + b + KEY_MIN for w in np.nonzero(words)[0] for b in range(32) if (int(words[w]) >> b) & 1], dtype=np.int64)
    below = words[bit >> 5] & ((np.uint32(1) << (bit & 31).astype(np.uint32)) - np.uint32(1))
    rank = prefix[bit >> 5] + np.array([bin(int(x)).count('1') for x in below], dtype=np.int64)
    seg = np.where(inside, rank, -1).astype(np.int32)
    counts = np.zeros(K, dtype=np.int64)
    np.add.at(counts, seg[inside], 1)
    assert ids.size == K
    return ids, seg.reshape(v.shape[0], v.shape[2], v.shape[3]), counts, int((~inside).sum())


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))


def _blocky(rng, shape, values):
    """an instance-like map: rectangles of `values` over a background of values[0]"""
    n, _, h, w = shape
    a = np.full(shape, values[0], dtype=np.float64)
    for i in range(n):
        for v in values[1:]:
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            a[i, 0, y0:y0 + rng.randint(1, max(2, h // 2 + 1)), x0:x0 + rng.randint(1, max(2, w // 2 + 1))] = v
    return a


def _encode_case(name, shape, dt, label_nc, pose_ch, inst=True, inst_values=(0, 1000, 2000, 3000, 7, 26000)):
    """random labels in [0, label_nc), poses in [0, pose_ch), a blocky instance map; dt = (label, inst, pose) dtype names"""
    rng = _rng(name)
    label = rng.randint(0, label_nc, size=shape).astype(np.float64)
    pose = rng.randint(0, pose_ch, size=shape).astype(np.float64) if pose_ch else None
    im = _blocky(rng, shape, inst_values) if inst else None
    return {'name': name, 'label': label, 'inst': im, 'pose': pose, 'dt': dt, 'label_nc': label_nc, 'pose_ch': pose_ch}


def encode_cases():
    """name -> case.  The shapes are the smallest at which k_encode_maps can go wrong; the values are float64 arrays that every
    dtype of the case represents exactly (the special cases set their fp32 values themselves)."""
    f = ('f32', 'f32', 'f32')
    cs = [
        _encode_case('one_pixel', (1, 1, 1, 1), ('u8', 'i32', 'i32'), 14, 25),                 # borders only
        _encode_case('one_row', (1, 1, 1, 9), f, 14, 25),
        _encode_case('one_column', (1, 1, 9, 1), ('u8', 'i16', 'f32'), 14, 25),
        _encode_case('scalar_5x7', (2, 1, 5, 7), ('i32', 'i32', 'i32'), 14, 25),               # W % 4 != 0: the scalar path
        _encode_case('real_channels', (2, 1, 16, 24), f, 14, 25),                              # the real layout on the vector path
        # 34 groups of four pixels per row, 256 groups per workgroup: the workgroups' boundaries (groups 256, 512, ...) fall
        # inside rows 7, 15, 22 and 30, and the grid has five workgroups
        _encode_case('chunk_boundary', (1, 1, 33, 136), ('u8', 'i16', 'i32'), 3, 2),
        _encode_case('offset_storage', (1, 1, 6, 8), f, 14, 25),                               # the test breaks the 16-byte alignment
        _encode_case('label_nc_1', (1, 1, 4, 8), f, 1, 25),
        _encode_case('label_nc_256', (1, 1, 3, 8), ('u8', 'f32', 'f32'), 256, 25),
        _encode_case('no_pose', (1, 1, 6, 8), f, 14, 0),
        _encode_case('no_inst', (1, 1, 6, 8), f, 14, 25, inst=False),
        _encode_case('dtypes', (1, 1, 4, 12), f, 14, 25, inst_values=(0, 1000, 2000, 7, 26000)),   # run in all 18 dtype combinations
    ]
    assert (136 // 4) * 7 < ENC_THREADS < (136 // 4) * 8 and 33 * (136 // 4) > 4 * ENC_THREADS
    # indices the reference has no answer for, and the ones at the edge of having one: fractions truncate toward zero
    c = _encode_case('bad_indices', (1, 1, 4, 8), f, 14, 25)
    c['label'][0, 0, 0, :] = [0.5, -0.5, -1.0, 14.0, NAN, 13.999, -0.999, 1e30]      # 0, 0, bad, bad, bad, 13, 0, bad
    c['label'][0, 0, 1, :4] = [-1e30, 2.75, float('inf'), -float('inf')]               # bad, 2, bad, bad
    c['pose'][0, 0, 3, :] = [24.5, 25.0, NAN, -0.25, -3.0, 0.0, 24.999, 7.5]         # 24, bad, bad, 0, bad, 0, 24, 7
    c['want_bad'] = [7, 3]
    cs.append(c)
    # fp32 instance values above 2^24 (neighbours that differ by one ulp, and equal ones), NaN neighbours (NaN != NaN), -0 == 0
    c = _encode_case('wide_floats', (1, 1, 4, 8), f, 14, 25)
    c['inst'][0, 0] = [[16777216, 16777218, 16777218, 16777220, 16777220, 16777220, 33554432, 33554436],
                       [NAN, NAN, 5, 5, 5, 5, 33554432, 33554432],
                       [5, 5, 5, NAN, 5, 5, -0.0, 0.0],
                       [5, 5, 5, 5, 5, 5, 0.0, 0.0]]
    cs.append(c)
    return {c['name']: c for c in cs}


def case_tensors(case, dt=None):
    """(label, inst or None, pose or None) CPU tensors of a case in its dtypes (or the (label, inst, pose) names given)"""
    dl, di, dp = dt or case['dt']
    mk = lambda a, d: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(TORCH[d])
    return mk(case['label'], dl), mk(case['inst'], di), mk(case['pose'], dp)


def index_cases():
    """name -> (inst CPU tensor [N, 1, H, W], expected path).  The key of a pixel is inst[i] * bs + i in the map's dtype,
    truncated."""
    i32, f32, i16 = torch.int32, torch.float32, torch.int16
    t = lambda rows, dt, shape: torch.tensor(rows, dtype=dt).reshape(shape)
    rng = _rng('index')
    cs = {
        # KEY_MIN is a multiple of 32: keys 31 | 32, 33 .. 63 | 64 sit either side of the bitmap's word boundaries
        'word_boundaries': (t([31, 32, 33, 63, 64, 0, 64, 31], i32, (1, 1, 2, 4)), 'device'),
        'key_zero': (t([0] * 5 + [3, 0, 0], i32, (1, 1, 2, 4)), 'device'),
        'window_ends': (t([KEY_MIN, KEY_LAST, KEY_LAST, 5, KEY_MIN, 5, 0, -1], i32, (1, 1, 2, 4)), 'device'),
        'window_ends_f32': (t([KEY_MIN, KEY_LAST, KEY_MIN - 0.5, 5, KEY_LAST + 0.5, 5.5, -0.5, -1], f32, (1, 1, 2, 4)), 'device'),
        'below_window': (t([KEY_MIN - 1, KEY_MIN, 5, 5, 7, 7, 0, 9], i32, (1, 1, 2, 4)), 'torch'),
        'above_window': (t([KEY_LAST + 1, KEY_LAST, 5, 5, 7, 7, 0, 9], i32, (1, 1, 2, 4)), 'torch'),
        'same_id_bs2': (t([[7, 7, 0, 1000] * 3] * 2, f32, (2, 1, 3, 4)), 'device'),
        'same_id_bs3': (t([[7, 7, 0, 1000] * 3] * 3, i32, (3, 1, 3, 4)), 'device'),
        'vkitti_bs8': (t([[255000, 255000, 26, 0, 1000, 255000, 26, 26]] * 8, f32, (8, 1, 2, 4)), 'device'),     # 255 000 * 8 + 7
        'int16_wraparound': (t([[20000, 20000, 26, 0, 1000, -20000, 26, 32767]] * 4, i16, (4, 1, 2, 4)), 'device'),   # 20 000 * 4 wraps
        'one_id': (torch.full((1, 1, 8, 8), 1000, dtype=f32), 'device'),
        'every_pixel_its_own': (torch.from_numpy(rng.permutation(2000).astype(np.int32) * 3).reshape(1, 1, 40, 50), 'device'),
        'odd_total': (t([3, 3, 3, 9, 9, 0, 0, 0, 1000, 1000, 3, 3, 3, 3, 70000], i32, (1, 1, 3, 5)), 'device'),       # 15 pixels
        'odd_plane': (torch.from_numpy(_blocky(rng, (2, 1, 3, 6), (0, 4, 1000))).to(f32), 'device'),                  # H W = 18, N H W = 36
        # 4160 pixels: five workgroups of the vector kernels, 17 of the scalar ones
        'many_workgroups': (torch.from_numpy(_blocky(rng, (2, 1, 40, 52), (0, 1000, 2000, 3000, 26, 255000))).to(f32), 'device'),
        'many_workgroups_i16': (torch.from_numpy(_blocky(rng, (3, 1, 37, 41), (0, 1000, 2000, 3000, 26, 20000))).to(i16), 'device'),
    }
    return cs
