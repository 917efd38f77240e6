#!/usr/bin/env python3
"""Generate tests/golden/segm_ppm_golden.npz: the pyramid pooling module of the reference's PPMBilinearDeepsup
(semantic/models.py:359-397), executed on the CPU in float64.

Imported from the reference as it lies: PPMBilinearDeepsup(num_class=5, fc_dim=16) -- its 512 branch channels are hard-coded --
with the drawn ppm.* state (tests/segm_ppm_util.draw_state), in eval() with randomised running statistics at [1, 16, 7, 13] and
in train() at [2, 16, 7, 13] (B = 1 makes BN raise on the 1 x 1 branch).  The input of decoder.conv_last is captured with a
forward pre-hook; the gradients of sum(go * that input) are taken in conv5 and the four 1 x 1 weights.  segm_ppm_util's stand-in
decoder, given the same state, must give the same: asserted here to 1e-13 before anything is stored.

Stored: the ppm.* state (the 1 x 1 weights as int8 sixty-fourths, the BN tensors as fp32: all exact) -- conv_last's own weight,
38 MB at these sizes, plays no part in what is compared and is not stored; per mode and quantity every n-th element of the float64
result plus its 2-norm (SAMPLE_STRIDE), as the loss fixture does; torch's own fp32 CPU error on each quantity (`err32/...`), the
yardstick of the training-mode gate; and torch's fp32 CPU errors on the operator-level cases of segm_ppm_util.CASES
(`op32/...`).  The inputs are redrawn by the tests from the same seeds.  Runs only where the reference exists.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
sys.path.insert(0, os.path.join(REF, 'semantic'))

import segm_ppm_util as u   # noqa: E402

warnings.filterwarnings('ignore')
import models as ref_models   # noqa: E402  the reference's semantic/models.py


def reference_module(mode, dtype):
    torch.manual_seed(u.MOD_SEED[mode])
    dec = ref_models.PPMBilinearDeepsup(num_class=u.MOD_CLASSES, fc_dim=u.MOD_FC).to(dtype)
    u.load_ppm_state(dec, u.draw_state())
    dec.train(mode == 'train')
    conv5, go = u.draw_module_case(mode)
    grabbed = []
    hook = dec.conv_last.register_forward_pre_hook(lambda mod, inp: grabbed.append(inp[0]))

    def concat(x):
        conv4 = torch.zeros(x.shape[0], u.MOD_FC // 2, 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
        dec([conv4, x])
        assert len(grabbed) == 1
        return grabbed[0]
    try:
        return u.module_results(dec, concat, conv5, go)
    finally:
        hook.remove()


def main():
    out = {}
    state = u.draw_state()
    for k in range(len(u.REF_SCALES)):
        q = np.round(state['ppm.%d.1.weight' % k] * 64.0)
        assert np.array_equal(q / 64.0, state['ppm.%d.1.weight' % k]) and np.abs(q).max() <= 127
        out['state/ppm.%d.1.weight_q64' % k] = q.astype(np.int8)
        for name in ('weight', 'bias', 'running_mean', 'running_var'):
            a = state['ppm.%d.2.%s' % (k, name)]
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
            out['state/ppm.%d.2.%s' % (k, name)] = a.astype(np.float32)
    for mode in ('eval', 'train'):
        theirs = reference_module(mode, torch.float64)
        ours = u.module_reference(mode)
        ours32 = u.module_reference(mode, dtype=torch.float32)
        for q in u.MOD_QUANTITIES:
            d = u.rel(ours[q], theirs[q])
            assert d <= 1e-13, 'case %s, %s: the restatement differs from the reference by %.3g' % (mode, q, d)
            a = theirs[q].reshape(-1)
            out['%s/%s_sample' % (mode, q)] = a[::u.SAMPLE_STRIDE[q]].copy()
            out['%s/%s_norm' % (mode, q)] = np.float64(np.linalg.norm(a))
            out['err32/%s/%s' % (mode, q)] = np.float64(u.rel(ours32[q], theirs[q]))
            print('%s %s: %d elements, norm %.6g, restatement rel %.1e, torch fp32 rel %.2e'
                  % (mode, q, a.size, np.linalg.norm(a), d, out['err32/%s/%s' % (mode, q)]))
        assert np.array_equal(theirs['cat'][:, :u.MOD_FC], u.draw_module_case(mode)[0].astype(np.float64))
    for name in u.CASES:
        case = u.draw_case(name)
        e = u.errors(u.reference(case, torch.float32), u.reference(case), case['C'])
        for q in u.QUANTITIES:
            out['op32/%s/%s' % (name, q)] = np.float64(e[q])
        print('case %s: torch fp32 against float64: %s' % (name, ', '.join('%s %.2e' % (q, e[q]) for q in u.QUANTITIES)))
    path = os.path.join(HERE, 'segm_ppm_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == '__main__':
    main()
