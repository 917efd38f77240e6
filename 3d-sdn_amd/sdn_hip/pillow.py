"""Pillow's (and torchvision 0.2.1's) host arithmetic that more than one branch shares: the coefficient tables of the bilinear
resampler, the index table of the NEAREST one and the draws of ColorJitter.  The geometric branch (derender3d.compositing,
derender3d.train_items), the textural loader (data.assemble) and the semantic loader (semantic.train_items) import them from
here; each is pinned against the installed Pillow by the tests of the module that first held it."""
import functools
import random

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3   # the op codes of a jitter order (csrc/train_items_common.h)

PRECISION_BITS = 32 - 8 - 2  # Pillow, Resample.c


@functools.lru_cache(maxsize=256)
def resample_tables(in_size, out_size):
    """Pillow's precompute_coeffs for the bilinear filter (support 1.0), box = the whole image.
    Returns (ksize, bounds int32 [out, 2] = (first source index, count), kk float64 [out, ksize]); cached per size pair
    (treat the arrays as read-only)."""
    scale = np.float64(np.float32(in_size) - np.float32(0.0)) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = (center - support + 0.5).astype(np.int64)   # C cast: truncation (the operands are > -1 here)
    xmin = np.maximum(xmin, 0)
    xmax = (center + support + 0.5).astype(np.int64)
    xmax = np.minimum(xmax, in_size)
    cnt = xmax - xmin
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        arg = (x + xmin - center + 0.5) * ss
        arg = np.where(arg < 0.0, -arg, arg)
        w = np.where(arg < 1.0, 1.0 - arg, 0.0)
        w = np.where(x < cnt, w, 0.0)
        kk[:, x] = w
        ww = ww + w          # same order as the C loop
    nz = ww != 0.0
    kk[nz] = kk[nz] / ww[nz, None]
    bounds = np.stack([xmin, cnt], axis=1).astype(np.int32)
    return ksize, bounds, kk


def fixed_point(kk):
    """normalize_coeffs_8bpc: (int)(+-0.5 + k * 2^22), C truncation."""
    v = kk * float(1 << PRECISION_BITS)
    return np.where(kk < 0, np.trunc(-0.5 + v), np.trunc(0.5 + v)).astype(np.int32)


@functools.lru_cache(maxsize=64)
def nearest_table(in_size, out_size):
    """Pillow ImagingScaleAffine: the source index of output x is (int) of xo, xo = a/2, a/2 + a, ... summed in double.
    Returns numpy int64 [out_size] (treat it as read-only)."""
    a = np.float64(in_size) / out_size
    xo = a * 0.5
    idx = np.zeros(out_size, dtype=np.int64)
    for x in range(out_size):
        idx[x] = int(xo)
        xo += a
    return np.minimum(idx, in_size - 1)


def jitter_params(brightness=.5, contrast=.5, saturation=.5, hue=.5, rng=random):
    """The draws of torchvision 0.2.1's ColorJitter.get_params -> (order, factors, hue_shift): `order` the ops present
    (BRIGHTNESS, CONTRAST, SATURATION, HUE) as shuffled, `factors` the brightness, contrast and saturation factors (1.0 for an
    absent op), `hue_shift` what adjust_hue adds to the H plane: int(hue_factor * 255) % 256, C's truncation toward zero and the
    wrap of np.uint8(...).  One uniform draw per present op in the order brightness, contrast, saturation, hue, then one shuffle
    of the list of ops.

    torchvision is not among this project's dependencies: the SAMPLING here is a restatement and is not pinned against it.
    Only the APPLICATION of given parameters (sdn_train_crops) is pinned, against Pillow."""
    order, factors, hue_shift = [], [1.0, 1.0, 1.0], 0
    if brightness > 0:
        factors[0] = rng.uniform(max(0, 1 - brightness), 1 + brightness)
        order.append(BRIGHTNESS)
    if contrast > 0:
        factors[1] = rng.uniform(max(0, 1 - contrast), 1 + contrast)
        order.append(CONTRAST)
    if saturation > 0:
        factors[2] = rng.uniform(max(0, 1 - saturation), 1 + saturation)
        order.append(SATURATION)
    if hue > 0:
        hue_shift = int(rng.uniform(-hue, hue) * 255) % 256
        order.append(HUE)
    rng.shuffle(order)
    return order, tuple(factors), hue_shift
