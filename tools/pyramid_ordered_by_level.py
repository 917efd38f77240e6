#!/usr/bin/env python3
"""Where the time of the pyramid RoIAlign's ordered backward goes: sdn_pyramid_roi_align_bwd_ordered and sdn_pyramid_roi_align_bwd
called directly at the reference's shapes (C = 256, maps of 256 .. 32 pixels square) with all R boxes drawn for ONE level at a time,
with log-uniform sides over all four, and with no box at all (the stores alone).  Per line the median of 7 regions of 20 calls.  On
the GPU only; the figures of one run are in profiles/pyramid_roi_align.md, "The ordered backward"."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd')):
    sys.path.insert(0, p)
import sdn_hip  # noqa: E402
from sdn_hip import ops  # noqa: E402

C, SIDES, AREA = 256, (256, 128, 64, 32), float(1024 * 1024)
# side lengths in pixels whose level value stays well inside one level: 4 + log2(side / 224)
RANGES = {'P2': (20, 70), 'P3': (90, 150), 'P4': (170, 300), 'P5': (340, 700), 'mixed': (16, 700)}


def boxes_of(rs, R, lo, hi):
    s = np.exp(rs.uniform(np.log(lo / 1024), np.log(hi / 1024), R))
    a = np.exp(rs.uniform(-0.15, 0.15, R))
    h, w = np.minimum(s * a, 0.99), np.minimum(s / a, 0.99)
    y1, x1 = rs.uniform(0, 1 - h), rs.uniform(0, 1 - w)
    return np.stack([y1, x1, y1 + h, x1 + w], 1).astype(np.float32)


def main():
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    L = sdn_hip.lib()
    ints = lambda v: (ctypes.c_int * 4)(*v)   # noqa: E731
    offsets, total = ops.pyramid_grad_floats(C, SIDES, SIDES)
    buf = torch.empty(total, device='cuda')
    rs = np.random.RandomState(5)
    for pool, R in ((7, 1000), (14, 200)):
        g = torch.randn(R, C, pool, pool, device='cuda')
        ws = torch.empty(ops.pyramid_ordered_workspace_bytes(R), dtype=torch.uint8, device='cuda')
        for name, (lo, hi) in RANGES.items():
            boxes = torch.from_numpy(boxes_of(rs, R, lo, hi)).cuda()

            def ordered():
                sdn_hip.check(L.sdn_pyramid_roi_align_bwd_ordered(g.data_ptr(), boxes.data_ptr(), R, ints(SIDES), ints(SIDES), C, pool, AREA,
                                                                  buf.data_ptr(), ws.data_ptr(), ws.numel(), sdn_hip.stream()))

            def atomic():
                sdn_hip.check(L.sdn_pyramid_roi_align_bwd(g.data_ptr(), boxes.data_ptr(), R, ints(SIDES), ints(SIDES), C, pool, AREA, buf.data_ptr(),
                                                          sdn_hip.stream()))
            out = {}
            for label, fn in (('ordered', ordered), ('atomic', atomic)):
                for _ in range(5):
                    fn()
                v = []
                for _ in range(7):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(20):
                        fn()
                    torch.cuda.synchronize()
                    v.append((time.perf_counter() - t0) * 1e3 / 20)
                out[label] = statistics.median(v)
            recs = ws.cpu().numpy().view(np.int32).reshape(R, 8)[:, 0]
            print('pool %2d R %4d boxes %-5s levels %s  ordered %.3f ms  atomic %.3f ms' % (pool, R, name, np.bincount(recs + 1, minlength=5)[1:].tolist(),
                                                                                            out['ordered'], out['atomic']), flush=True)
        # no boxes: the stores alone
        for _ in range(3):
            sdn_hip.check(L.sdn_pyramid_roi_align_bwd_ordered(None, None, 0, ints(SIDES), ints(SIDES), C, pool, AREA, buf.data_ptr(), None, 0, sdn_hip.stream()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            sdn_hip.check(L.sdn_pyramid_roi_align_bwd_ordered(None, None, 0, ints(SIDES), ints(SIDES), C, pool, AREA, buf.data_ptr(), None, 0, sdn_hip.stream()))
        torch.cuda.synchronize()
        print('pool %2d R 0: the stores alone %.3f ms' % (pool, (time.perf_counter() - t0) * 1e3 / 20), flush=True)


if __name__ == '__main__':
    main()
