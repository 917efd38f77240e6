#!/usr/bin/env python3
"""Writes tests/golden/encode_input_golden.npz: the expected results of the textural input encoding (csrc/encode_input.hip) for
the cases of tests/encode_input_util.py, computed on the CPU by that file's restatement of the torch expressions it replaces --
Pix2PixHDModel.encode_input / get_edges (zeros + long + scatter_, the four in-place ORs, cat) and Encoder._disambiguate +
torch.unique(sorted, return_inverse, return_counts).  Per encode case: input_label, pose_onehot (absent without pose), bad; per
index case: the disambiguated map, ids, inverse, counts.  No GPU and no library is needed:

    python tests/golden/make_encode_input_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import encode_input_util as u  # noqa: E402


def arrays():
    out = {}
    for name, c in u.encode_cases().items():
        label, inst, pose = u.case_tensors(c)
        input_label, pose_onehot, bad = u.encode_reference(label, inst, pose, c['label_nc'], c['pose_ch'])
        out['encode/%s/input_label' % name] = input_label.numpy()
        if pose_onehot is not None:
            out['encode/%s/pose_onehot' % name] = pose_onehot.numpy()
        out['encode/%s/bad' % name] = np.array(bad, dtype=np.int32)
    for name, (inst, _) in u.index_cases().items():
        d, ids, inverse, counts = u.index_reference(inst)
        out['index/%s/inst' % name] = d.numpy()
        out['index/%s/ids' % name] = ids.numpy()
        out['index/%s/inverse' % name] = inverse.numpy()
        out['index/%s/counts' % name] = counts.numpy()
    return out


if __name__ == '__main__':
    path = sys.argv[1] if len(sys.argv) > 1 else u.GOLD
    np.savez_compressed(path, **arrays())
    print('wrote %s: %d bytes' % (path, os.path.getsize(path)))
