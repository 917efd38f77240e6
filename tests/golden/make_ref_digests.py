#!/usr/bin/env python3
"""Writes tests/golden/ref_digests.json: dtype, shape and sha256 (tests/util.py digest) of every array the reference's own
code returns on the seeded inputs of tests/test_oracle_vs_ref.py (its rasterizer kernel strings, oracle/_ref/libnr_ref.so)
and tests/test_maskrcnn_oracle.py (its nms.c / crop_and_resize.c, oracle/_ref/libmaskrcnn_ref.so).  Where oracle/_ref
is absent those tests compare the oracle with these digests instead of the live reference.  Runs only where
oracle/build_ref.py could build oracle/_ref (the reference checkout is present)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import maskrcnn_np as mn  # noqa: E402
from oracle import raster_np as rn  # noqa: E402
import test_maskrcnn_oracle  # noqa: E402
import test_oracle_vs_ref  # noqa: E402
from util import REF_DIGESTS, digest  # noqa: E402


def main():
    assert rn.have_ref() and mn.have('ref'), 'oracle/_ref missing: run oracle/build_ref.py where the reference exists'
    out = {}
    for mod in (test_oracle_vs_ref, test_maskrcnn_oracle):
        for key, case, args in mod.cases():
            out[key] = {k: digest(v) for k, v in case(*args, impl='ref').items()}
    with open(REF_DIGESTS, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d cases' % (REF_DIGESTS, len(out)))


if __name__ == '__main__':
    main()
