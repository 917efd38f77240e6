"""The two facts k_face_setup's handling of thin faces rests on, checked by brute force over every pixel (no GPU).

k_face_setup sends a face whose margin (face_margin_px) is not a small positive number down the band path of k_raster_tiles.
Two kinds of such faces need less than the whole band around the line through their longest edge:

 1. a face with a REPEATED VERTEX (two vertices with bit-identical NDC x and y) never records a pixel: face_inverse divides
    by den == 0 exactly, and wherever the edge tests pass the barycentric weights clamp to 0, their sum is 0 and the depth is
    NaN -- the face is dropped;
 2. a SLIVER WITH A FINITE MARGIN (THIN_MARGIN < m < S) passes the edge tests only inside its box dilated by m, like any
    ordinary face -- its thin record carries that box.

Below: float32 numpy restatements of inside_ndc, face_inverse, bary_weights and persp_depth (raster_math.h) and of
face_margin_px (raster_fwd.hip), operation by operation (numpy rounds every float32 operation once and fuses nothing), over
all S x S pixels at S = 96.
"""
import numpy as np
import torch

from oracle import nr_oracle as no

S = 96
F = np.float32
NEAR_LE, FAR = F(0.1), F(100.0)     # 0.1f > 0.1, so the largest float <= 0.1 is the one below it
if float(NEAR_LE) > 0.1:
    NEAR_LE = np.nextafter(NEAR_LE, F(-np.inf))
THIN_MARGIN = F(4.0)
U = F(9.5367432e-7)


def ndc_of_pixel(i):
    """pixel_to_ndc: (2 i + 1 - S) / S in double, rounded to float"""
    return ((2.0 * np.asarray(i, np.float64) + 1.0 - S) / S).astype(F)


def pixel_of_ndc(v):
    """ndc_to_pixel: 0.5 * ((v * S + S) - 1)"""
    return F(0.5) * ((v * F(S) + F(S)) - F(1))


def edge_tests(f):
    """inside_ndc for faces f [n, 3, 3] at every pixel -> bool [n, S, S] (row = y, column = x)"""
    xp = ndc_of_pixel(np.arange(S))[None, None, :]
    yp = ndc_of_pixel(np.arange(S))[None, :, None]
    ok = np.ones((len(f), S, S), bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        xa, ya = f[:, a, 0][:, None, None], f[:, a, 1][:, None, None]
        xb, yb = f[:, b, 0][:, None, None], f[:, b, 1][:, None, None]
        ok &= ~((yp - ya) * (xb - xa) < (xp - xa) * (yb - ya))
    return ok


def face_inverse(f):
    """-> (inv [n, 9], den [n]) from the pixel coordinates of the vertices"""
    px, py = pixel_of_ndc(f[:, :, 0]), pixel_of_ndc(f[:, :, 1])
    x0, x1, x2 = px.T
    y0, y1, y2 = py.T
    inv = np.stack([y1 - y2, x2 - x1, x1 * y2 - x2 * y1,
                    y2 - y0, x0 - x2, x2 * y0 - x0 * y2,
                    y0 - y1, x1 - x0, x0 * y1 - x1 * y0], 1)
    den = x2 * (y0 - y1) + x0 * (y1 - y2)
    den = den + x1 * (y2 - y0)
    with np.errstate(all='ignore'):
        inv = inv / den[:, None]
    return inv, den


def recorded(f, inv):
    """bary_weights + persp_depth + the depth window at every pixel -> bool [n, S, S]: the pixel would reach the z-buffer"""
    fx = np.arange(S, dtype=F)[None, None, :]
    fy = np.arange(S, dtype=F)[None, :, None]
    with np.errstate(all='ignore'):
        w = []
        total = np.zeros((len(f), S, S), F)
        for k in range(3):
            t = inv[:, 3 * k, None, None] * fx + inv[:, 3 * k + 1, None, None] * fy
            t = t + inv[:, 3 * k + 2, None, None]
            t = np.fmin(np.fmax(t, F(0)), F(1))     # fmaxf / fminf: a NaN operand loses
            w.append(t)
            total = total + t
        w = [t / total for t in w]
        z = [f[:, k, 2][:, None, None] for k in range(3)]
        s = w[0] / z[0] + w[1] / z[1]
        s = s + w[2] / z[2]
        zp = F(1) / s
        return (zp > NEAR_LE) & (zp < FAR)


def face_margin_px(f, S=S):
    """face_margin_px of raster_fwd.hip for faces [n, 3, 3] at internal size S -> m [n] (-1: no usable margin)"""
    with np.errstate(all='ignore'):
        e0, e1, e2 = f[:, 1, :2] - f[:, 0, :2], f[:, 2, :2] - f[:, 0, :2], f[:, 2, :2] - f[:, 1, :2]
        ln = [np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) for e in (e0, e1, e2)]
        lmax = np.maximum(ln[0], np.maximum(ln[1], ln[2]))
        perim = ln[0] + ln[1] + ln[2]
        cmax = np.abs(f[:, :, :2]).max((1, 2))
        area2 = np.abs(e0[:, 0] * e1[:, 1] - e1[:, 0] * e0[:, 1]) - U * lmax * lmax
        delta = U * (F(1) + cmax)
        base = F(0.004) * max(F(1), F(S) * F(1.0 / 1024.0)) + F(0.5) * F(S) * delta
        m = base + F(0.5) * F(S) * (delta * perim * lmax / area2)
        return np.where((area2 > 0) & (m < F(S)), m, F(-1)).astype(F)


def repeated_vertex_faces(rng, n_each):
    """[n, 3, 3] faces with two bit-identical vertices: three kinds of end points x the lone vertex in each position x both
    windings (the reversed vertex list moves the lone vertex and is listed as well)."""
    out = []
    for kind in range(3):
        for _ in range(n_each):
            if kind == 0:      # both end points on pixel centres (the line runs along a lattice direction)
                p = ndc_of_pixel(rng.integers(0, S, 2))
                q = ndc_of_pixel(rng.integers(0, S, 2))
            elif kind == 1:    # one on a pixel centre, one far outside the screen
                p = ndc_of_pixel(rng.integers(0, S, 2))
                q = (rng.uniform(2.0, 20.0, 2) * rng.choice([-1.0, 1.0], 2)).astype(F)
            else:
                p, q = rng.uniform(-1.5, 1.5, 2).astype(F), rng.uniform(-1.5, 1.5, 2).astype(F)
            if p[0] == q[0] and p[1] == q[1]:
                q = (q + F(0.25)).astype(F)
            zp, zq = rng.uniform(0.5, 5.0, 2).astype(F)
            zt = F(rng.uniform(0.5, 5.0))     # (the twin may differ in depth: only x and y are compared)
            P, T, Q = np.array([p[0], p[1], zp], F), np.array([p[0], p[1], zt], F), np.array([q[0], q[1], zq], F)
            for lone in range(3):
                v = [P, T]
                v.insert(lone, Q)
                out.append(np.stack(v))
                out.append(np.stack(v[::-1]))
    return np.stack(out)


def sliver_faces(rng, n_lattice, n_random):
    """Slivers: a long edge and an apex a tiny distance off it, both windings; the long edge through pixel centres (pixels
    sit ON the edge: the case in which rounding decides) or anywhere."""
    out = []
    for i in range(n_lattice + n_random):
        if i < n_lattice:
            a = rng.integers(0, S, 2).astype(np.float64)
            b = rng.integers(0, S, 2).astype(np.float64)
        else:
            a, b = rng.uniform(-10, S + 10, 2), rng.uniform(-10, S + 10, 2)
        d = b - a
        L = np.hypot(d[0], d[1])
        if L < 4.0:
            continue
        nrm = np.array([-d[1], d[0]]) / L
        c = a + rng.uniform(0.1, 0.9) * d + nrm * rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-4.2, -2.2)
        pix = np.stack([a, b, c])
        ndc = (2.0 * pix + 1.0 - S) / S
        v = np.concatenate([ndc, rng.uniform(0.5, 5.0, (3, 1))], 1).astype(F)
        out.append(v)
        out.append(v[::-1].copy())
    return np.stack(out)


def test_repeated_vertex_faces_record_no_pixel():
    rng = np.random.default_rng(11)
    f = repeated_vertex_faces(rng, 40)          # 3 kinds x 40 x 3 positions x 2 windings = 720 faces
    assert len(f) >= 300
    inv, den = face_inverse(f)
    assert (den == 0).all(), 'face_inverse must divide by exactly zero for a repeated vertex'
    passed = edge_tests(f)
    rec = passed & recorded(f, inv)
    print('repeated-vertex faces: %d, pixels passing the edge tests: %d, recorded: %d' % (len(f), passed.sum(), rec.sum()))
    assert passed.sum() >= 300, 'the check needs pixels that pass the edge tests'
    assert rec.sum() == 0
    alpha = no.rasterize_rgbad(torch.tensor(f[None]), None, S, False, 0.1, 100, 1e-3, None, False, True, False)['alpha']
    assert float(alpha.abs().max()) == 0.0, 'the oracle covers a pixel with repeated-vertex faces alone'


def test_bounded_slivers_stay_inside_their_dilated_box():
    rng = np.random.default_rng(12)
    f = sliver_faces(rng, 900, 900)
    m = face_margin_px(f)
    keep = (m > THIN_MARGIN) & (m < F(S))
    f, m = f[keep], m[keep]
    assert len(f) >= 500, 'only %d slivers with THIN_MARGIN < m < S' % len(f)
    px, py = pixel_of_ndc(f[:, :, 0]), pixel_of_ndc(f[:, :, 1])
    x0, x1 = np.ceil(px.min(1) - m), np.floor(px.max(1) + m)      # k_face_setup's dilated box, before clipping to the screen
    y0, y1 = np.ceil(py.min(1) - m), np.floor(py.max(1) + m)
    passed = edge_tests(f)
    xs = np.arange(S, dtype=F)[None, None, :]
    ys = np.arange(S, dtype=F)[None, :, None]
    inside = (xs >= x0[:, None, None]) & (xs <= x1[:, None, None]) & (ys >= y0[:, None, None]) & (ys <= y1[:, None, None])
    print('bounded slivers: %d (margins %.1f .. %.1f), pixels passing the edge tests: %d, outside the dilated box: %d'
          % (len(f), m.min(), m.max(), passed.sum(), (passed & ~inside).sum()))
    assert passed.sum() >= 500, 'the check needs pixels that pass the edge tests'
    assert (passed & ~inside).sum() == 0
