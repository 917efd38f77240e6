#!/usr/bin/env python3
"""Time the loss dict of a geometric training step on the GPU, forward + backward, at the training shape (B = 64 items, rendered
masks 384 x 384, target masks 256 x 256, _ffd_coeffs [64, 8, 21], mode extend): derender3d.losses.step_losses (sdn_train_losses_fwd /
_bwd: two launches forward, one backward) against the torch form a caller had to write before it -- the reference's
BaseNet.step_batch expressions in fp32 on the device, as tests/test_gpu_train_losses.py restates them (BaseNet.partial's
torch.nonzero + numel() branch and isnan().any() branch: two host waits per loss, six losses, twelve per step).

Same seeded inputs for both; the values are compared before any clock is read.  Device events around windows of back-to-back
steps after a warm-up, the two forms alternating, the median window reported.  Prints markdown.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

B, R, S = 64, 384, 256


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--mixed', action='store_true', help='half the items mask-only (targets 2), as a hybrid batch')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_train_losses needs a GPU: timings taken anywhere else say nothing')
    import test_gpu_train_losses as t
    from derender3d import TargetType
    from derender3d import losses as L
    targets = [3 if (i % 2 == 0 or not args.mixed) else 2 for i in range(B)]
    blob, batch = t.draw(B, R, S, targets, seed=7)
    bd = {k: v.cuda().requires_grad_() for k, v in blob.items()}
    td = {k: v.cuda() for k, v in batch.items()}
    mode = TargetType.extend

    def fused():
        for v in bd.values():
            v.grad = None
        d = L.step_losses(bd, td, mode)
        sum(d.values()).backward()
        return d

    def torch_form():
        for v in bd.values():
            v.grad = None
        d = t.reference_losses(bd, td, mode, 0.1, 1.0)
        sum(d.values()).backward()
        return d

    a = fused()
    ga = {k: v.grad.clone() for k, v in bd.items()}
    b = torch_form()
    for k in a:
        rel = abs(float(a[k]) - float(b[k])) / abs(float(b[k]))
        assert rel < 1e-5, (k, float(a[k]), float(b[k]))           # the torch form sums in fp32
    for k, v in bd.items():
        rel = float((v.grad - ga[k]).norm() / ga[k].norm())
        assert rel < 1e-5, (k, rel)
    for _ in range(3):
        window(fused, args.reps)
        window(torch_form, args.reps)
    tf, tt = [], []
    for _ in range(args.windows):
        tf.append(window(fused, args.reps))
        tt.append(window(torch_form, args.reps))
    nffd = blob['_ffd_coeffs'].numel()
    n_r = sum(1 for v in targets if v & 2)
    fwd_bytes = 4 * (n_r * (R * R + 2 * S * S) + nffd)
    bwd_bytes = 4 * (n_r * (R * R + 2 * S * S) + B * R * R + 2 * nffd)
    print('| forward + backward, B = %d, R = %d, S = %d, nffd = %d, %d of %d items reprojected, mode extend | ms per step (median of %d windows of %d) | min .. max |'
          % (B, R, S, nffd, n_r, B, args.windows, args.reps))
    print('|---|---|---|')
    print('| `step_losses` (2 launches forward, 1 backward, no host wait) | %.4f | %.4f .. %.4f |' % (statistics.median(tf), min(tf), max(tf)))
    print('| torch form (fp32 restatement of `BaseNet.step_batch`, 12 host waits) | %.4f | %.4f .. %.4f |' % (statistics.median(tt), min(tt), max(tt)))
    print()
    print('counted bytes of the fused form: %.1f MB forward, %.1f MB backward; over the median step that is %.0f GB/s '
          '(a lower bound on the kernels: the step includes autograd\'s host work and the launch gaps)'
          % (fwd_bytes / 1e6, bwd_bytes / 1e6, (fwd_bytes + bwd_bytes) / statistics.median(tf) / 1e6))


if __name__ == '__main__':
    main()
