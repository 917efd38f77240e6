#!/usr/bin/env python3
"""Times the semantic training batch at the reference's shape (two frames 375 x 1242, four jitter ops with contrast, one item
flipped; tests/segm_train_util.real_inputs) for every default short size.  Prints one JSON line with, per short size:
  device_ms   semantic.train_items.segm_train_batch: the host's table building, the one upload and at most three launches;
              inputs and outputs stay on the device
  kernels_us  the launches alone between two events on the stream (the table buffer built and validated again per call)
  host_ms     the loop of semantic/vkitti_dataset.py:111-157 restated with Pillow and torch's CPU on the same box
              (tests/golden/make_segm_train_golden.reference_batch), labels of the scene pixels looked up beforehand -- the
              reference's Python call per pixel (:120) is left out of the host's time, in its favour
host clock around a synchronised region, median of --reps after --warmup.  Checks that both forms give the same bits.  Needs
the repository's tests/ directory."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def events(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    a = ap.parse_args()
    import make_segm_train_golden as ref
    import segm_train_util as u
    from sdn_hip import ops
    from semantic import train_items as st
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU form of it'
    frames, scenes, tables = u.real_inputs()
    fd, sd = torch.from_numpy(frames).cuda(), torch.from_numpy(scenes).cuda()
    tabs = st._as_tables(tables, 2)
    flips, jitters = list(u.REAL_FLIPS), u.real_jitters()
    looked_up = [u.scene_labels(scenes[i], *tables[i]) for i in range(2)]
    real_lookup = u.scene_labels
    res = {'frames': [2, 375, 1242], 'reps': a.reps, 'sizes': {}}
    for short in u.DEFAULT_SHORTS:
        state = {}

        def device():
            state['out'] = st.segm_train_batch(fd, sd, tabs, short, flips, jitters)

        sizes, Hb, Wb = st.batch_sizes(short, 2)
        buf = st.table_buffer(sizes, tabs, flips, jitters, 375, 1242)

        def kernels():
            ops.segm_train_batch(fd, sd, buf, Hb, Wb, 8, st.MEAN, st.STD)

        it = iter(looked_up * (a.host_reps + 2))
        u.scene_labels = lambda *args: next(it)   # :120 done beforehand
        try:
            t0 = time.perf_counter()
            for _ in range(a.host_reps):
                host = ref.reference_batch(frames, scenes, tables, short, flips, jitters, u.REAL)
            host_ms = (time.perf_counter() - t0) * 1e3 / a.host_reps
        finally:
            u.scene_labels = real_lookup
        for _ in range(a.warmup):
            device()
        row = {'device_ms': wall(device, a.reps), 'kernels_us': events(kernels, a.reps), 'host_ms': host_ms,
               'batch': [Hb, Wb], 'table_ints': int(buf.size)}
        out = state['out']
        assert np.array_equal(out['img_data'].cpu().numpy().view(np.uint32), host['img_data'].view(np.uint32))
        assert np.array_equal(out['seg_label'].cpu().numpy(), host['seg_label'])
        res['sizes'][str(short)] = row
    print(json.dumps(res))


if __name__ == '__main__':
    main()
