#!/usr/bin/env python3
"""Measures how far the map gradients of pyramid_roi_align lie from the float64 gradients of the fixture
tests/golden/pyramid_roi_align_golden.npz over repeated backward runs: the order of the atomic adds differs from run to run, so one
run says little.  Per case of tests/pyramid_roi_align_util.py prints the worst distance per level as a share of the fixture's gate
and how many of --runs runs exceeded a gate.  Then the same for the ordered backward (SDN_DETERMINISTIC=1), together with its spread:
the number of runs whose bytes differ from the first run's, which must be zero.  On the GPU only."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=40)
    a = ap.parse_args()
    import pyramid_roi_align_util as u
    from maskrcnn import pyramid
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    gold = np.load(u.GOLD)
    assert 'SDN_DETERMINISTIC' not in os.environ, 'unset SDN_DETERMINISTIC: the tool runs both backward paths and sets it itself'
    for path in ('atomic', 'ordered'):
        if path == 'ordered':
            os.environ['SDN_DETERMINISTIC'] = '1'
        print('the %s backward' % path, flush=True)
        spread(a, u, pyramid, gold)


def spread(a, u, pyramid, gold):
    for name in u.CASES:
        c = u.draw_case(name)
        want = [gold[name + '/grad64_%d' % l] for l in range(u.LEVELS)]
        gate = gold[name + '/gate']
        worst, over, first, other_bytes = np.zeros(u.LEVELS), 0, None, 0
        for _ in range(a.runs):
            boxes = torch.from_numpy(c['boxes'].copy())[None].cuda()
            maps = [torch.from_numpy(m.copy())[None].cuda().requires_grad_(True) for m in c['maps']]
            pooled, _levels = pyramid.pyramid_levels([boxes] + maps, c['pool'], u.IMAGE_SHAPE)
            pooled.backward(torch.from_numpy(c['grads'].copy()).cuda())
            got = [m.grad[0].cpu().numpy() for m in maps]
            first = first or [g.tobytes() for g in got]
            other_bytes += int(first != [g.tobytes() for g in got])
            err = u.grad_error(got, want)
            worst = np.maximum(worst, err)
            over += int((err > gate).any())
        print('%-10s worst / gate %s   runs over a gate: %d of %d   runs with other bytes than the first: %d'
              % (name, ' '.join('%.3f' % v for v in worst / gate), over, a.runs, other_bytes), flush=True)
        assert os.environ.get('SDN_DETERMINISTIC') != '1' or other_bytes == 0, 'the ordered backward is not reproducible on %s' % name


if __name__ == '__main__':
    main()
