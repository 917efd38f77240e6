#!/usr/bin/env python3
"""Times the detector-output stage on the 375 x 1242 case of tests/golden/detections_golden.npz (D = 100 rows, 25 detections,
16 selected).  Prints one JSON line:
  device   sdn_unmold_masks through the library's hipEvent timing (slot 6): the areas pass over all detections and the plane
           pass over the 16 selected, median of --reps warm launches each; bytes written and the rate of the plane pass; the
           wall time of SceneSession.from_detections up to the SceneSession call (host clock around a synchronised region)
  host     a restatement of the reference's flow (maskrcnn/model.py:1638-1653, 2084-2143, main.py:805-818): mrcnn_mask to the
           host, per detection bytescale + PIL resize + threshold + paste into uint8 planes, stack, sums over every plane,
           selection, float32 upload of the 16 survivors
           (its stages are reported one by one: copy down, resize + paste, stack, sums + selection, upload)
and checks the two give the same masks.  Needs the repository's tests/ directory (the fixture and tests/detections_util.py)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import PIL.Image
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import detections_util as du
    import sdn_hip
    from maskrcnn import detections as det
    g = du.load()
    dev = torch.device('cuda:0')
    H, W = 375, 1242
    detections = torch.from_numpy(g['a_detections']).to(dev)
    mrcnn_mask = torch.from_numpy(g['a_mrcnn_mask']).to(dev)
    window = g['a_window']
    state = {}

    def device_flow():     # from_detections up to the SceneSession call
        boxes, ids, scores, keep = det.unmold_boxes(detections.cpu().numpy(), (H, W), window)
        plan = det.UnmoldPlan(mrcnn_mask, boxes, ids, keep, H, W)
        areas = plan.areas().cpu().numpy()
        sels = det.select_largest(areas, 16)
        state['plan'], state['sels'] = plan, sels
        state['masks'] = plan.masks(sels)[0]

    stages = {}

    def host_flow():
        t = [time.perf_counter()]

        def lap(name):
            t.append(time.perf_counter())
            stages.setdefault(name, []).append((t[-1] - t[-2]) * 1e3)
        d = detections.cpu().numpy()
        soft = mrcnn_mask.permute(0, 2, 3, 1).cpu().numpy()
        lap('host_copy_down_ms')
        boxes, ids, scores, keep = det.unmold_boxes(d, (H, W), window)
        full = []
        for i, k in enumerate(keep):
            y1, x1, y2, x2 = boxes[i]
            b = du.bytescale_f32(soft[k, :, :, ids[i]])
            im = PIL.Image.frombytes('L', (28, 28), b.tobytes()).resize((x2 - x1, y2 - y1), PIL.Image.BILINEAR)
            m = np.where(np.array(im).astype(np.float32) / 255.0 >= 0.5, 1, 0).astype(np.uint8)
            plane = np.zeros((H, W), np.uint8)
            plane[y1:y2, x1:x2] = m
            full.append(plane)
        lap('host_resize_paste_ms')
        image_masks = np.expand_dims(np.transpose(np.stack(full, axis=-1), (2, 0, 1)), axis=1)
        lap('host_stack_ms')
        sels = np.flipud(np.argsort(np.sum(image_masks, axis=(1, 2, 3))))[:min(len(ids), 16)]
        lap('host_sums_select_ms')
        state['host_masks'] = torch.tensor(image_masks[sels].astype(np.float32)).cuda()
        torch.cuda.synchronize()
        lap('host_float32_upload_ms')

    for _ in range(a.warmup):
        device_flow(), host_flow()
    stages.clear()
    res = {'frame': [H, W], 'rows': int(detections.shape[0]), 'detections': int(state['plan'].n), 'selected': len(state['sels']),
           'reps': a.reps, 'device_flow_ms': wall(device_flow, a.reps), 'host_flow_ms': wall(host_flow, a.reps)}
    assert torch.equal(state['masks'], state['host_masks'])
    res.update({k: statistics.median(v) for k, v in stages.items()})     # the stages of the host flow, same runs
    plan, sels = state['plan'], state['sels']
    sdn_hip.timing_enable(True)
    sdn_hip.timing_read_slot(sdn_hip.SLOT_SCENE_MASKS)
    for name, fn in (('areas_pass_us', plan.areas), ('plane_pass_us', lambda: plan.masks(sels))):
        ts = []
        for _ in range(a.reps):
            fn()
            ms, n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_SCENE_MASKS)
            assert n == 1
            ts.append(ms * 1e3)
        res[name] = statistics.median(ts)
    sdn_hip.timing_enable(False)
    res['plane_bytes_written'] = len(sels) * H * W * 4
    res['plane_pass_TBps'] = res['plane_bytes_written'] / (res['plane_pass_us'] * 1e-6) / 1e12
    res['host_upload_bytes'] = len(sels) * H * W * 4
    res['host_download_bytes'] = int(mrcnn_mask.numel() * 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
