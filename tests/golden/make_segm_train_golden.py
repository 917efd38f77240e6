"""Writes tests/golden/segm_train_golden.npz: the training batch of the semantic branch as the reference makes it
(semantic/vkitti_dataset.py:83-159), performed with the installed Pillow and torch's CPU.

Written anew from the reference's statements, which it cites by line; none of its text is here.  What the reference calls
resolves to Pillow on every step:
  :124      torchvision 0.2.1's ColorJitter: functional.adjust_brightness / _contrast / _saturation are ImageEnhance.Brightness /
            Contrast / Color(img).enhance(factor); adjust_hue is convert('HSV'), a wrapping uint8 addition on H, convert back
  :135-136  cv2.flip(., 1): the columns mirrored (numpy here)
  :139-140  scipy.misc.imresize(arr, (h, w), interp) = toimage(arr).resize((w, h), resample); a uint8 array passes toimage
            unchanged (bytescale returns uint8 data as it is)
  :148-150  the same call on the array padded with zeros to multiples of the rate
  :152-154  astype(float32)[:, :, ::-1], transpose, Normalize: t.sub_(m).div_(s) per channel on torch's CPU
  :120      the dictionary look-up per pixel.  A colour outside the table raises KeyError there; the fixture gives it label 0
            (so -1 after :159) and counts the label positions it reaches by sending a 0 / 1 image through the same two resizes.

The small cases' inputs are stored; the real-size frames (5.6 MB) are drawn from the seed by tests/segm_train_util.py and the
fixture holds their SHA-256.  Expected images are stored as the uint8 pixels before :152; the fp32 batch tensor is stored for
two small cases and as a SHA-256 for every case, next to `lut` = the same torch statements applied to all 256 byte values --
this script asserts that the full torch result equals the gather of lut at the pixels, so the tests can rebuild it bit for bit.

    python tests/golden/make_segm_train_golden.py
"""
import os
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import segm_train_util as u  # noqa: E402

FULL_FP32 = ('s12n', 's33f')   # the small cases whose fp32 batch tensor is stored whole


def round_up(x, p):   # :17-18
    return ((x - 1) // p + 1) * p


def reference_sizes(short, cfg):
    """:91-106"""
    B, p, rate = cfg['B'], cfg['padding_constant'], cfg['segm_downsampling_rate']
    sizes = np.zeros((B, 2), np.int32)
    for i in range(B):
        fh, fw = cfg['frame_size']
        scale = min(short / min(fh, fw), cfg['img_max_size'] / max(fh, fw))
        sizes[i, :] = fh * scale, fw * scale
    assert p >= rate
    return sizes, int(round_up(np.max(sizes[:, 0]), p)), int(round_up(np.max(sizes[:, 1]), p))


def jitter_pil(img, jitter):
    """:124 with given parameters"""
    if jitter is None:
        return img
    order, factors, shift = jitter
    for op in order:
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(factors[0])
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(factors[1])
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(factors[2])
        else:
            h, s, v = img.convert('HSV').split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over='ignore'):
                np_h += np.uint8(shift)
            img = Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')
    return img


def imresize(arr, size, resample):
    return np.array(Image.fromarray(arr).resize((int(size[1]), int(size[0])), resample))


def reference_batch(frames, scenes, tables, short, flips, jitters, cfg):
    rate = cfg['segm_downsampling_rate']
    sizes, Hb, Wb = reference_sizes(short, cfg)
    B = cfg['B']
    batch_images = torch.zeros(B, 3, Hb, Wb)
    batch_segms = torch.zeros(B, Hb // rate, Wb // rate).long()
    unknown = np.zeros(B, dtype=np.int64)
    px = []
    for i in range(B):
        segm, unk = u.scene_labels(scenes[i], *tables[i])                               # :120
        maps = [segm.astype(np.uint8), unk.astype(np.uint8)]                             # :121
        img = np.array(jitter_pil(Image.fromarray(frames[i]), jitters[i]))               # :124-125
        if flips[i]:                                                                     # :135-136
            img = np.ascontiguousarray(img[:, ::-1])
            maps = [np.ascontiguousarray(m[:, ::-1]) for m in maps]
        img = imresize(img, sizes[i], Image.BILINEAR)                                    # :139
        small = []
        for m in maps:
            m = imresize(m, sizes[i], Image.NEAREST)                                     # :140
            rounded = np.zeros((round_up(m.shape[0], rate), round_up(m.shape[1], rate)), dtype='uint8')   # :143-146
            rounded[:m.shape[0], :m.shape[1]] = m
            small.append(imresize(rounded, (rounded.shape[0] // rate, rounded.shape[1] // rate), Image.NEAREST))   # :148-150
        px.append(img)
        t = torch.from_numpy(img.astype(np.float32)[:, :, ::-1].transpose((2, 0, 1)).copy())   # :152-153
        for c in range(3):                                                               # :154 (Normalize.__call__)
            t[c].sub_(u.MEAN[c]).div_(u.STD[c])
        batch_images[i][:, :t.shape[1], :t.shape[2]] = t                                 # :156
        batch_segms[i][:small[0].shape[0], :small[0].shape[1]] = torch.from_numpy(small[0].astype(np.int64))   # :157
        unknown[i] = int(small[1].sum())
    batch_segms = batch_segms - 1                                                        # :159
    return {'sizes': sizes, 'Hb': Hb, 'Wb': Wb, 'px': px, 'img_data': batch_images.numpy(), 'seg_label': batch_segms.numpy(),
            'unknown': unknown}


def put_jitters(out, prefix, jitters):
    order = np.full((len(jitters), 4), -1, dtype=np.int64)
    factors = np.ones((len(jitters), 3), dtype=np.float64)
    shift = np.zeros(len(jitters), dtype=np.int64)
    present = np.zeros(len(jitters), dtype=bool)
    for i, j in enumerate(jitters):
        if j is not None:
            present[i] = True
            order[i, :len(j[0])] = j[0]
            factors[i] = j[1]
            shift[i] = j[2]
    out[prefix + 'order'], out[prefix + 'factors'], out[prefix + 'shift'], out[prefix + 'present'] = order, factors, shift, present


def main():
    out = {}
    lut = torch.arange(256, dtype=torch.float32).repeat(3, 1)
    for c in range(3):
        lut[c].sub_(u.MEAN[c]).div_(u.STD[c])
    lut = lut.numpy()
    out['lut'] = lut

    def check_lut(r):
        assert np.array_equal(u.expected_img(r['px'], lut, r['Hb'], r['Wb']).view(np.uint32), r['img_data'].view(np.uint32))

    out['default/shorts'] = np.array(u.DEFAULT_SHORTS)
    for s in u.DEFAULT_SHORTS:
        sizes, Hb, Wb = reference_sizes(s, u.REAL)
        out['default/%d/sizes' % s], out['default/%d/HbWb' % s] = sizes, np.array([Hb, Wb])

    frames, scenes, tables = u.small_inputs()
    out['small/frames'], out['small/scenes'] = frames, scenes
    for i, (codes, labels) in enumerate(tables):
        out['small/codes%d' % i], out['small/labels%d' % i] = codes, labels
    put_jitters(out, 'small/jitter_', u.small_jitters())
    for short in u.SMALL_SHORTS:
        for flip in (False, True):
            name = u.case_name(short, flip)
            flips, jitters = u.small_case(short, flip)
            r = reference_batch(frames, scenes, tables, short, flips, jitters, u.SMALL)
            check_lut(r)
            assert r['unknown'][0] == 0 and r['unknown'][1] > 0 and r['unknown'][2] == 0, (name, r['unknown'])
            p = 'small/%s/' % name
            out[p + 'sizes'], out[p + 'HbWb'] = r['sizes'], np.array([r['Hb'], r['Wb']])
            for i, px in enumerate(r['px']):
                out[p + 'px%d' % i] = px
            out[p + 'seg_label'], out[p + 'unknown'] = r['seg_label'], r['unknown']
            out[p + 'img_sha256'] = np.array(u.digest(r['img_data']))
            if name in FULL_FP32:
                out[p + 'img_data'] = r['img_data']
            print(name, r['sizes'][0], r['Hb'], r['Wb'], 'unknown', r['unknown'])

    frames, scenes, tables = u.real_inputs()
    out['real/inputs_sha256'] = np.array(u.digest(frames, scenes, *[a for t in tables for a in t]))
    jitters = u.real_jitters()
    put_jitters(out, 'real/jitter_', jitters)
    for short in u.REAL_SHORTS:
        r = reference_batch(frames, scenes, tables, short, list(u.REAL_FLIPS), jitters, u.REAL)
        check_lut(r)
        p = 'real/%d/' % short
        out[p + 'sizes'], out[p + 'HbWb'] = r['sizes'], np.array([r['Hb'], r['Wb']])
        rows = np.array(u.REAL_ROWS_300) if short == 300 else np.arange(r['sizes'][0, 0])
        out[p + 'rows'] = rows
        for i, px in enumerate(r['px']):
            out[p + 'px%d' % i] = px[rows]
        out[p + 'seg_label'], out[p + 'unknown'] = r['seg_label'], r['unknown']
        out[p + 'img_sha256'] = np.array(u.digest(r['img_data']))
        print('real', short, r['sizes'][0], r['Hb'], r['Wb'], 'unknown', r['unknown'])

    np.savez_compressed(u.GOLD, **out)
    print('wrote %s: %d bytes' % (u.GOLD, os.path.getsize(u.GOLD)))


if __name__ == '__main__':
    main()
