"""The host half (no GPU) of the Derenderer's device heads: the entry points in header, binding and library, how the kernel file is
built and what it may not contain, the mirrored constants, the C entry points' refusals (they run on the arguments alone, before any
launch), the wrapper's refusals, tools/derender_heads_check.cpp under ASan and UBSan, ResNet.pooled and the module switch, the
restatement's two non-linear gradients against autograd, and the conditions the fixtures of tests/derender_heads_util.py must meet."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import derender_heads_util as u
import host_checks
import makefile_rules
from derender3d.models import heads          # the feature itself: without it this module does not import
from sdn_hip import ops
from sdn_hip.ops import derender_heads       # noqa: F401  (likewise)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('sdn_derender_heads_workspace_bytes', 'sdn_derender_heads_fwd', 'sdn_derender_heads_bwd')
CSRC = os.path.join(ROOT, '3d-sdn_amd', 'csrc')


def test_header_binding_and_library_hold_the_entry_points():
    history = host_checks.entry_points(NAMES)
    at = history.index('#define SDN_ABI_VERSION')
    clause = 'still 20: sdn_derender_heads_workspace_bytes, sdn_derender_heads_fwd, sdn_derender_heads_bwd added'
    assert clause in history[at - 3000:at]
    assert history.index('sdn_pyramid_roi_align_bwd_ordered added') < history.index(clause) < at
    for line in ('derenderer.py:27-32', ':34-43', ':45-56', 'models/__init__.py:70-77'):      # the reference lines the entry points replace
        assert line in history, line
    host_checks.stale_library_is_refused(NAMES)        # added without a revision bump: a library built before them is stale


def test_the_kernel_file_is_built_exactly_and_keeps_the_contract():
    makefile_rules.assert_built_exactly('derender_heads.hip')
    text = open(os.path.join(CSRC, 'derender_heads.hip')).read()
    assert '#include "derender_heads_check.h"' in text
    code = text.split('namespace sdn {')[1]
    assert 'tomic' not in code and 'hipMemset' not in code and 'hipMemcpy' not in code and 'Synchronize' not in code
    assert len(re.findall(r'\bexpf\(', code)) == 1 and not re.search(r'__(expf|fdividef|frcp_r[a-z]|fdiv_r[a-z])\b', code)
    assert not re.search(r'\bf(min|max)f\(', code)                                 # they drop a NaN: the maximum is a comparison
    # no workgroup waits for another: no spin, no flag, no cooperative launch
    assert not re.search(r'\bwhile\s*\(|volatile|__threadfence|hipLaunchCooperativeKernel|s_sleep', code)
    # at most four launches each way: one launch statement per direction, reached through a helper that the entry point calls
    # at most four times, never in a loop
    assert len(re.findall(r'hipLaunchKernelGGL\(', text)) == 2
    fwd = text[text.index('SDN_API int sdn_derender_heads_fwd'):text.index('SDN_API int sdn_derender_heads_bwd')]
    bwd = text[text.index('SDN_API int sdn_derender_heads_bwd'):]
    assert len(re.findall(r'\bdh_launch_fwd\(', fwd)) == 4 and 'dh_launch_bwd(' not in fwd
    assert len(re.findall(r'\bdh_launch_bwd\(', bwd)) == 4 and 'dh_launch_fwd(' not in bwd
    assert not re.search(r'\b(for|while)\s*\(', fwd) and not re.search(r'\b(for|while)\s*\(', bwd)
    # every multiply-add is an explicit fmaf: no a * b + c left to a contraction the build forbids anyway
    assert len(re.findall(r'\bfmaf\(', code)) >= 20


def test_the_constants_are_mirrored():
    const = lambda name: host_checks.constexpr_int('derender_heads_check.h', name)   # noqa: E731
    assert ops.DERENDER_HEADS_MAX_CLASSES == const('DH_MAX_CLASSES') == 16 and ops.DERENDER_HEADS_MAX_N == const('DH_MAX_N') == 65535
    assert ops.DERENDER_HEADS_ROWS == const('DH_ROWS') == 16 and ops.DERENDER_HEADS_SLAB == const('DH_SLAB') == 128
    assert const('DH_FIXED') == 8 == sum(w for _k, w in __import__('derender3d.models.derenderer', fromlist=['x'])._FIXED_COLUMNS)
    # the workspace: the slabs of the three hidden gradients, rounded up to 256 bytes
    assert ops.derender_heads_workspace_bytes(16, 512, 256, 8, 192) == (13 + 2 + 2) * 16 * 256 * 4
    assert ops.derender_heads_workspace_bytes(1, 8, 4, 1, 3) == 256


# ---- the entry points' checks: they run on the arguments alone, before any launch, so they need no GPU ------------------------------
FAKE = 0x10000   # never dereferenced: every call below is refused first
W4 = (FAKE,) * 4


def _fwd(pooled=FAKE, roi=FAKE, centre=None, extent=None, w=W4, b=W4, n=16, F=512, Hd=256, classes=8, coeffs=192, out=FAKE,
         centre_out=FAKE, extent_out=FAKE, row=None, saved=FAKE):
    import sdn_hip
    lib = sdn_hip.lib()
    rc = lib.sdn_derender_heads_fwd(pooled, roi, centre, extent, w[0], b[0], w[1], b[1], w[2], b[2], w[3], b[3], n, F, Hd, classes, coeffs,
                                    out, centre_out, extent_out, row, saved, None)
    return rc, lib.sdn_last_error().decode()


def _bwd(g=(FAKE,) * 6, pooled=FAKE, centre=FAKE, extent=FAKE, w=W4, out=FAKE, saved=FAKE, n=16, F=512, Hd=256, classes=8, coeffs=192,
         wanted=(FAKE,) * 9, ws=FAKE, ws_bytes=1 << 30):
    import sdn_hip
    lib = sdn_hip.lib()
    rc = lib.sdn_derender_heads_bwd(*g, pooled, centre, extent, *w, out, saved, n, F, Hd, classes, coeffs, *wanted, ws, ws_bytes, None)
    return rc, lib.sdn_last_error().decode()


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    import sdn_hip
    lib = sdn_hip.lib()
    sizes = ((dict(n=0), 'n 0; 1 to 65535 objects'), (dict(n=65536), 'n 65536'), (dict(F=510), 'F 510; a positive multiple of 4'),
             (dict(F=0), 'F 0'), (dict(Hd=254), 'Hd 254; a positive multiple of 4'), (dict(Hd=-4), 'Hd -4'),
             (dict(classes=0), 'classes 0; 1 to 16'), (dict(classes=17), 'classes 17; 1 to 16'), (dict(coeffs=0), 'coeffs 0; at least 1'),
             (dict(n=65535, classes=16, coeffs=1 << 20), 'n * O ='), (dict(n=8, F=1 << 28, Hd=4, classes=1, coeffs=1), 'n * F = 2147483648'),
             (dict(n=1, F=4, Hd=1 << 16, classes=16, coeffs=3000), 'O * Hd ='),
             (dict(n=1, F=1 << 20, Hd=1 << 11, classes=1, coeffs=1), 'Hd * F = 2147483648'),
             (dict(n=1, F=4, Hd=1 << 16, classes=1, coeffs=1), 'Hd * (Hd + 4) ='),
             (dict(n=60000, F=4, Hd=4096, classes=16, coeffs=1), 'the workspace of'))
    hole, bent = (FAKE, FAKE, None, FAKE), (FAKE, FAKE + 4, FAKE, FAKE)
    for kw, reason in sizes + (
            (dict(pooled=None), 'pooled is NULL'), (dict(centre=FAKE, extent=FAKE), 'exactly one roi form'),
            (dict(roi=None, centre_out=None, extent_out=None), 'exactly one roi form'),
            (dict(roi=None, centre=FAKE, centre_out=None, extent_out=None), 'exactly one roi form'),
            (dict(centre_out=None), 'centre_out and extent_out go with roi_norms'),
            (dict(roi=None, centre=FAKE, extent=FAKE), 'centre_out and extent_out go with roi_norms'),
            (dict(w=hole), 'w2 is NULL'), (dict(b=hole), 'b2 is NULL'), (dict(w=bent), 'w1 must be aligned to 16 bytes'),
            (dict(b=(FAKE, FAKE, FAKE, FAKE + 2)), 'b3 must be aligned to 4 bytes'), (dict(out=None), 'out or saved is NULL'),
            (dict(saved=None), 'out or saved is NULL'), (dict(pooled=FAKE + 2), 'aligned to 4 bytes'), (dict(row=FAKE + 1), 'aligned to 4 bytes'),
            (dict(out=FAKE + 2), 'aligned to 4 bytes'), (dict(roi=FAKE + 2), 'aligned to 4 bytes')):
        rc, msg = _fwd(**kw)
        assert rc == -1 and msg.startswith('sdn_derender_heads_fwd: ') and reason in msg, (kw, msg)
    g_bent, want_bent = (FAKE, None, FAKE + 2, None, FAKE, FAKE), (FAKE,) * 4 + (FAKE + 2,) + (FAKE,) * 4
    for kw, reason in sizes[:9] + (
            (dict(pooled=None), 'pooled, centre or extent is NULL'), (dict(extent=None), 'pooled, centre or extent is NULL'),
            (dict(w=hole), 'w2 is NULL'), (dict(w=(FAKE, FAKE, FAKE, FAKE + 2)), 'w3 must be aligned to 4 bytes'),
            (dict(out=None), 'out or saved is NULL'), (dict(saved=None), 'out or saved is NULL'),
            (dict(g=g_bent), 'output gradient 2 must be aligned to 4 bytes'), (dict(wanted=want_bent), 'input gradient 4 must be aligned to 4 bytes'),
            (dict(centre=FAKE + 2), 'aligned to 4 bytes'), (dict(ws=None), 'workspace is NULL'),
            (dict(ws=FAKE + 4), 'workspace must be aligned to 16 bytes'), (dict(ws_bytes=278527), 'workspace of 278527 bytes; 278528 are needed')):
        rc, msg = _bwd(**kw)
        assert rc == -1 and msg.startswith('sdn_derender_heads_bwd: ') and reason in msg, (kw, msg)
    nbytes = ctypes.c_size_t(0)
    assert lib.sdn_derender_heads_workspace_bytes(16, 512, 256, 8, 192, None) == -1
    assert lib.sdn_last_error().decode() == 'sdn_derender_heads_workspace_bytes: bytes is NULL'
    assert lib.sdn_derender_heads_workspace_bytes(16, 512, 256, 17, 192, ctypes.byref(nbytes)) == -1
    assert lib.sdn_last_error().decode().startswith('sdn_derender_heads_workspace_bytes: classes 17')
    # nothing asked for: no launch, no error -- still before any use of the device
    assert _bwd(wanted=(None,) * 9) == (0, lib.sdn_last_error().decode())


def _layers(f=36, hd=20, classes=3, coeffs=24):
    O = 8 + classes + classes * coeffs
    return [(torch.zeros(hd, f), torch.zeros(hd)), (torch.zeros(hd, hd + 4), torch.zeros(hd)), (torch.zeros(hd, hd), torch.zeros(hd)),
            (torch.zeros(O, hd), torch.zeros(O))]


def test_the_wrapper_refuses_what_the_kernels_cannot_take():
    pooled, roi, L = torch.zeros(5, 36), torch.zeros(5, 4), _layers()
    pair = (torch.zeros(5, 2), torch.zeros(5, 2))
    # there is no torch form: CPU tensors are an error, in the op and in the module switch
    with pytest.raises(NotImplementedError, match='pooled is on cpu; the derenderer heads only run on the GPU'):
        ops.derender_heads(pooled, roi, *L, 3)
    with pytest.raises(NotImplementedError):
        ops.derender_heads(pooled, pair, *L, 3)
    with pytest.raises(NotImplementedError):
        ops.derender_heads(pooled[:0], roi[:0], *L, 3)
    # types
    with pytest.raises(TypeError, match='rois must be roi_norms'):
        ops.derender_heads(pooled, None, *L, 3)
    with pytest.raises(TypeError, match='rois must be roi_norms'):
        ops.derender_heads(pooled, (roi, roi, roi), *L, 3)
    with pytest.raises(TypeError, match='pooled must be a torch.Tensor'):
        ops.derender_heads(pooled.numpy(), roi, *L, 3)
    with pytest.raises(TypeError, match='pooled must be torch.float32'):
        ops.derender_heads(pooled.double(), roi, *L, 3)
    with pytest.raises(TypeError, match='extent must be torch.float32'):
        ops.derender_heads(pooled, (pair[0], pair[1].half()), *L, 3)
    with pytest.raises(TypeError, match=r'fc2.weight must be torch.float32'):
        ops.derender_heads(pooled, roi, L[0], L[1], (L[2][0].double(), L[2][1]), L[3], 3)
    with pytest.raises(TypeError, match='fc1 must be an nn.Linear with a bias or a'):
        ops.derender_heads(pooled, roi, L[0], torch.nn.Linear(24, 20, bias=False), L[2], L[3], 3)
    with pytest.raises(TypeError, match='fc3 must be an nn.Linear'):
        ops.derender_heads(pooled, roi, L[0], L[1], L[2], 7, 3)
    # shapes and sizes
    with pytest.raises(ValueError, match=r'pooled must be fp32 \[n, F\]'):
        ops.derender_heads(pooled[0], roi, *L, 3)
    with pytest.raises(ValueError, match='0 classes; 1 to 16'):
        ops.derender_heads(pooled, roi, *L, 0)
    with pytest.raises(ValueError, match='17 classes'):
        ops.derender_heads(pooled, roi, *L, 17)
    with pytest.raises(ValueError, match='F 34 and Hd 20'):
        ops.derender_heads(pooled[:, :34].contiguous(), roi, *L, 3)
    with pytest.raises(ValueError, match='F 36 and Hd 18'):
        ops.derender_heads(pooled, roi, (torch.zeros(18, 36), torch.zeros(18)), *L[1:], 3)
    with pytest.raises(ValueError, match='fc3 has 83 outputs; 8 . classes . classes . coeffs with 4 classes'):
        ops.derender_heads(pooled, roi, *L, 4)
    with pytest.raises(ValueError, match=r'fc1.weight must be \[20, 24\]'):
        ops.derender_heads(pooled, roi, L[0], (torch.zeros(20, 20), L[1][1]), L[2], L[3], 3)
    with pytest.raises(ValueError, match=r'fc3.bias must be \[83\]'):
        ops.derender_heads(pooled, roi, L[0], L[1], L[2], (L[3][0], torch.zeros(84)), 3)
    with pytest.raises(ValueError, match=r'roi_norms must be \[5, 4\]'):
        ops.derender_heads(pooled, roi[:4], *L, 3)
    with pytest.raises(ValueError, match=r'extent must be \[5, 2\]'):
        ops.derender_heads(pooled, (pair[0], roi), *L, 3)
    with pytest.raises(ValueError, match='n 65536; up to 65535'):
        ops.derender_heads(torch.zeros(1, 36).expand(65536, 36), roi, *L, 3)
    with pytest.raises(ValueError, match=r'must stay below 2\^31'):
        wide = 8 + 16 + 16 * (1 << 26)
        ops.derender_heads(torch.zeros(1, 4), torch.zeros(1, 4), (torch.zeros(4, 4), torch.zeros(4)), (torch.zeros(4, 8), torch.zeros(4)),
                           (torch.zeros(4, 4), torch.zeros(4)), (torch.zeros(1).expand(wide, 4), torch.zeros(1).expand(wide)), 16)
    with pytest.raises(ValueError, match='pooled must be contiguous'):
        ops.derender_heads(torch.zeros(36, 5).t(), roi, *L, 3)
    with pytest.raises(ValueError, match='fc.weight must be contiguous'):
        ops.derender_heads(pooled, roi, (torch.zeros(36, 20).t(), L[0][1]), *L[1:], 3)
    # the reference never asks for a gradient of the roi vectors
    with pytest.raises(ValueError, match='roi_norms requires a gradient'):
        ops.derender_heads(pooled, roi.clone().requires_grad_(True), *L, 3)
    with pytest.raises(ValueError, match='centre requires a gradient'):
        ops.derender_heads(pooled, (pair[0].clone().requires_grad_(True), pair[1]), *L, 3)
    # nn.Linear modules are taken as they are
    with pytest.raises(NotImplementedError):
        ops.derender_heads(pooled, roi, torch.nn.Linear(36, 20), torch.nn.Linear(24, 20), torch.nn.Linear(20, 20), torch.nn.Linear(20, 83), 3)


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------------
def test_the_headers_layouts_and_validators_walk_clean_under_asan_and_ubsan(tmp_path):
    """tools/derender_heads_check.cpp: a stand-alone program with its own main that includes only csrc/derender_heads_check.h; host code
    on the CPU, never loaded into Python"""
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, 'derender_heads_check.h')).read()) == ['check_common.h']
    rc, out = host_checks.run_check_program('derender_heads_check', ['derender_heads_check.h'], tmp_path)
    assert rc == 0 and b' 0 failures' in out and b'the validators' in out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def derenderer():
    from derender3d.models.derenderer import Derenderer
    torch.manual_seed(3)
    return Derenderer(num_classes=3, grid_size=2)


def test_resnet_has_pooled_and_forward_is_fc_of_it(derenderer):
    import inspect
    from derender3d.models.resnet import ResNet18
    assert list(inspect.signature(ResNet18.pooled).parameters) == ['self', 'x']
    body = inspect.getsource(ResNet18.forward)
    assert 'return self.fc(self.pooled(x))' in body
    with pytest.raises(NotImplementedError):           # as before: no torch form of the backbone
        derenderer.net.pooled(torch.zeros(1, 3, 64, 64))


def test_the_switch_is_a_flag_that_travels_with_dict_and_remove_clears_it(derenderer):
    from derender3d.models.derenderer import Derenderer
    names, keys = [n for n, _m in derenderer.named_modules()], list(derenderer.state_dict())
    assert derenderer._device_heads is False and '_device_heads' not in derenderer.__dict__
    handle = heads.use_device_heads(derenderer)
    assert derenderer.__dict__['_device_heads'] is True and 'forward' not in derenderer.__dict__     # a flag, not a bound method
    replica = Derenderer.__new__(Derenderer)                                                           # what DataParallel's replicate does
    replica.__dict__ = copy.copy(derenderer.__dict__)
    assert replica._device_heads is True
    assert [n for n, _m in derenderer.named_modules()] == names and list(derenderer.state_dict()) == keys
    with pytest.raises(NotImplementedError, match='the derenderer heads only run on the GPU|ResNet18|GPU'):   # the flag routes the forward
        derenderer(torch.zeros(2, 3, 64, 64), torch.zeros(2, 2), torch.zeros(2, 2))
    handle.remove()
    assert '_device_heads' not in derenderer.__dict__ and derenderer._device_heads is False
    handle.remove()                                                                                     # twice is harmless
    with heads.use_device_heads(derenderer) as h:
        assert derenderer._device_heads is True and isinstance(h, heads.DeviceHeadsHandle)
    assert derenderer._device_heads is False
    with pytest.raises(TypeError, match='must be a Derenderer3d or a Derenderer'):
        heads.use_device_heads(object())
    with pytest.raises(TypeError, match='must be a Derenderer3d or a Derenderer'):
        heads.use_device_heads(torch.nn.Linear(2, 2))


def test_the_switch_reaches_both_modules_of_a_derenderer3d():
    from derender3d import TargetType
    from derender3d.models import Derenderer3d
    model = Derenderer3d(TargetType.geometry, 256, 64)
    assert model._device_heads is False
    with heads.use_device_heads(model):
        assert model.__dict__['_device_heads'] is True and model.derenderer.__dict__['_device_heads'] is True
    assert '_device_heads' not in model.__dict__ and '_device_heads' not in model.derenderer.__dict__


# ---- the restatement and its fixtures -------------------------------------------------------------------------------------------------
def test_the_loop_gradients_are_autograds():
    g = torch.Generator().manual_seed(2)
    row2 = (torch.rand(7, 2, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    logits = (torch.rand(7, 5, generator=g, dtype=torch.float64) * 4 - 2).requires_grad_(True)
    g2, g5 = torch.rand(7, 2, generator=g, dtype=torch.float64) - 0.5, torch.rand(7, 5, generator=g, dtype=torch.float64) - 0.5
    d = row2 / torch.norm(row2, p=2, dim=1, keepdim=True)
    p = torch.softmax(logits, dim=1)
    torch.autograd.backward([d, p], [g2, g5])
    assert np.abs(u.norm_grad_loop(row2.detach().numpy(), g2.numpy()) - row2.grad.numpy()).max() < 1e-14
    assert np.abs(u.softmax_grad_loop(p.detach().numpy(), g5.numpy()) - logits.grad.numpy()).max() < 1e-15


@pytest.mark.parametrize('name', list(u.CASES))
def test_the_fixtures_meet_their_conditions(name):
    ratios, same, norms = u.fixture_figures(name)
    print('%s: smallest |pre-activation| / float32 distance per layer %s; pose norms %.3f .. %.3f' %
          (name, ['%.1f' % r for r in ratios], float(norms.min()), float(norms.max())))
    assert min(ratios) >= u.MARGIN and same
    if name == 'zero_row':
        assert float(norms[u.ZERO_ROW]) == 0.0
        norms = torch.cat((norms[:u.ZERO_ROW], norms[u.ZERO_ROW + 1:]))
    assert float(norms.min()) >= u.MIN_NORM
    f, hd, classes, coeffs, O, n = u.widths(name)
    ref = u.reference(name)
    assert ref['out64']['_ffd_coeffs'].shape == (n, classes, coeffs) and ref['grad64']['fc3.weight'].shape == (O, hd)
    assert ref['out64']['_class_probs'].dtype == torch.float64 and ref['out32']['_class_probs'].dtype == torch.float32
