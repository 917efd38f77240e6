#!/usr/bin/env python3
"""bench.py -- rendered-objects/sec of the geometric hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run measures the headline only: it builds the scene, runs W warm-up steps, times K steps and prints the JSON line
(`value`, `ms_per_step`, the kernel timings of the timed region and the rooflines derived from them).  Everything else below
-- the textural leg, the secondary meshes, K1, the real meshes, the host-issue time, the ALU roofline, the blocking exchange,
configs[2] / [4], compositing and the CPU baselines -- runs with --full.  --dump-outputs DIR writes what the last timed step
computed (the maps a caller receives -- gathered over the ranks when N > 1 -- and the gradients of the pose / FFD parameters)
as DIR/<name>.npy in float32; the inputs are seeded, so two builds can be compared output for output.

One STEP = one VKITTI frame's worth of objects (16, the cap of geometric/scripts/main.py:812) per GPU, each object
going through exactly what one iteration of the reference's test-time optimisation loop does
(geometric/scripts/main.py:439-456 over derender3d/models/__init__.py:161-224):
    FFD decode -> PerspectiveTransform (zoom-to-fit) -> silhouette + normal + depth at render_size 384
    (2x anti-aliasing: 768^2 internal), loss = MSE(mask, target) + 100 * mean(ffd^2), backward to the pose / FFD
    parameters.
Meshes: 8 procedural car-class templates of ~43k triangles (85.7k faces after fill_back) -- the ShapeNet files and
every dataset are absent on the benchmark box (sdn_hip/synth.py).  Inputs are resident in HBM before the timed
region; nothing leaves the device inside it.  With N > 1 the objects are sharded over the ranks (weak scaling: 16 per
GPU) and the rendered maps are exchanged with ONE RCCL all_gather per step, the only exchange this path has.

The second half of BASELINE.json's metric, "textural-GAN fwd+bwd ms at 375x1242", is measured with --full, right after, on
the same GPU(s): one Pix2PixHDModel.train_step (textural/train.py:69-95 -- G + E forward, three multiscale-D forwards, generator
and discriminator backward, two Adam updates) at batch 4, 384x1248 (375x1242 padded to a multiple of 16),
48-channel generator input, 3-scale discriminator, no VGG loss (its weights cannot be downloaded here).  Reported as
`textural_gan_fwd_bwd_ms` with its own roofline object.

Extra objects in the JSON line:
  roofline            dominant kernel group of the geometric step -- since r03 the silhouette edge gradient's k_edge_scan_sil
                      + k_edge_rows (or k_raster_tiles, whichever takes longer): algorithmic bytes per launch (SURVEY.md
                      8(d): 20 R^2 + 20 S^2 + 12 V per object backward) / mean launch time from hipEvents on the launch stream
                      inside the timed region, against 8 TB/s; `traffic` = counter bytes of the rocprofv3 PMC passes under
                      profiles/ (flagged `traffic_stale` when they were collected on another build of the library).
  roofline_raster_fwd / roofline_edge_bwd   the two candidates, same method;  roofline_alu: pixel tests of k_raster_tiles
                      counted by its counting build outside the timed region, against the fp32 vector peak.
  roofline_textural   the MFMA implicit-GEMM group (k_conv_gemm + k_conv_tile + k_conv_halo): algorithmic flops of the launches (r05: from
                      the layers' TRUE channel counts; the fp32 head kernels have their own slot, `narrow`) / their summed time,
                      against the 2.5 PFLOP/s dense bf16 MFMA peak; `issued_frac` counts the 3 MFMAs the bf16x3 split
                      issues per algorithmic product; `single_stream`: the same with every kernel alone on the chip.
  host_issue_ms_one_step   host time to issue ONE step into an empty queue (the host cost; `host_enqueue_ms_per_step` only
                      measures the depth of the HIP queue once the GPU is the bottleneck).
  headline_mesh       since r04 `value` runs on templates with the statistics of the reference's ShapeNet CAD files
                      (sdn_hip.synth.cad_like, profiles/cad_mesh_stats.json): long thin triangles, depth complexity ~8.
  car_like / value_car_like   the same frame step on the smooth car-sized templates that were the r01-r03 headline,
                      outside the headline's timed region.
  k1 / value_k1       (r05) the headline's frame step under neural_renderer.use_unsafe_rasterizer(True): the reference's DEFAULT
                      coverage rule K1 (scripts/env.sh:11), same mesh, outside the timed region.
  exchange            (r05, N > 1 only) algo (all_gather | p2p: SDN_EXCHANGE), payload (objects | frame: SDN_EXCHANGE_PAYLOAD),
                      bytes per rank and step, and the measured time of ONE exchange with nothing overlapping it.
  derender3d_loop (+ _car_like), edit_pipeline, compositing, textural_reference_default, textural_extras   configs[2]
                      (the reference's own optimisation loop on the product's Derenderer3d -- the DROP-IN route next to the fused
                      frame step of `value` -- on the headline's mesh family and on the r01-r03 one), configs[4] (r05: stage A with
                      4 frames' crops per encoder call and one host read per rank, stage B on 4 frames per fake_inference call)
                      and secondary numbers (single GPU only).
  cpu_baseline        the CPU oracle (port of the reference kernels, OpenMP over pixels) on whole objects of the same
                      workload -- one rgb+alpha+depth rasterisation + the silhouette backward each -- under a 25 s cap, with
                      thread count, affinity and per-phase seconds; cpu_baseline_textural: the G/D/E train step at bs 1,
                      192x624 through the pinned textural oracle (torch CPU fp32), median of 3.
"""
import argparse
import json
import os
import sys
import time

os.environ.pop('NEURAL_RENDERER_UNSAFE', None)   # the benchmark measures the default (safe-rule) rasterizer
ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, '3d-sdn_amd'), os.path.join(ROOT, '3d-sdn_amd', 'geometric'),
           os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault('SDN_ALLOW_RANDOM_INIT', '1')  # synthetic benchmark: random-init VGG-19 / ResNet-18, stated in `data`

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

OBJECTS_PER_FRAME = 16
RENDER_SIZE = 384
FOCAL = 725.0  # VKITTI camera (geometric/derender3d/datasets.py:207-213)
N_TRIS = 45000


HEADLINE_MESH, SECONDARY_MESH = 'cad_like', 'car_like'
REAL_TEMPLATES = os.path.join(ROOT, 'tests', 'golden', 'cad_templates.npz')
TEX_GEMM_GROUP = ['sdn::k_conv_gemm', 'sdn::k_conv_tile', 'sdn::k_conv_halo']
MESH_NOTES = {
    'cad_like': 'sdn_hip.synth.cad_like: triangle-area histogram, depth complexity (~8) and degenerate-face rate fitted to the six '
                'ShapeNet OBJs of the reference (profiles/cad_mesh_stats.json)',
    'car_like': 'sdn_hip.synth.car_like: a smooth closed car-sized surface with the CAD files\' triangle count (the r01-r03 headline)',
}


def build_scene(device, seed, mesh='car_like'):
    """8 templates + 16 object poses, everything resident on `device`.  mesh: 'car_like' (the headline's templates) or
    'cad_like' (templates with the statistics of the reference's ShapeNet CAD files, profiles/cad_mesh_stats.json)."""
    from derender3d.models.transforms import FFD, FFDBank, PerspectiveTransform
    from sdn_hip import synth
    rng = np.random.default_rng(seed)
    ffds, faces, sizes = [], [], []
    real = np.load(REAL_TEMPLATES) if mesh.startswith('real') else None
    for k in range(8):
        if real is not None:
            # the reference's own six ShapeNet templates (tests/golden/cad_templates.npz: ShapenetObj's vertices + faces, produced
            # from the OBJ files by tests/golden/make_cad_golden_hi.py --templates): 'real' = the six, two of them twice;
            # 'real:<j>' = eight copies of template j (the frame's 16 objects are then 16 poses of that one mesh)
            j = int(mesh.split(':')[1]) if ':' in mesh else k % 6
            v, f = real['t%d/verts' % j], real['t%d/faces' % j]
        else:
            v, f = (synth.cad_like(46000, seed=100 + k) if mesh == 'cad_like' else synth.car_like(N_TRIS, seed=100 + k))
            v = v[:, [2, 1, 0]] * np.asarray([-1, 1, 1], np.float32)  # ShapenetObj axis convention
        ffds.append(FFD(torch.tensor(v), constraints=[
            FFD.Constraint.symmetry(axis=FFD.Constraint.Axis.z),
            FFD.Constraint.homogeneity(axis=FFD.Constraint.Axis.y, index=[0, 1])]))
        faces.append(torch.tensor(f))
        sizes.append((v.shape[0], f.shape[0]))
    bank = FFDBank(ffds, faces).to(device)
    n = OBJECTS_PER_FRAME
    cls = rng.integers(0, 8, n)
    theta = rng.uniform(-np.pi, np.pi, n)
    params = {
        'ffd': torch.tensor(rng.normal(0, 0.02, (n, 192)).astype(np.float32), device=device, requires_grad=True),
        'log_scale': torch.tensor(np.log(np.array([3.9, 1.5, 1.6], np.float32))[None].repeat(n, 0) +
                                  rng.normal(0, 0.05, (n, 3)).astype(np.float32), device=device, requires_grad=True),
        'theta': torch.tensor(theta.astype(np.float32)[:, None], device=device, requires_grad=True),
        'translation': torch.tensor(np.stack([rng.uniform(-8, 8, n), rng.uniform(0.5, 2, n), -rng.uniform(8, 40, n)],
                                             1).astype(np.float32), device=device, requires_grad=True),
    }
    targets = torch.zeros(n, 1, RENDER_SIZE, RENDER_SIZE, device=device)
    targets[:, :, 120:270, 40:340] = 1
    return bank, sizes, cls, params, targets, PerspectiveTransform()


def make_step(device, bank, cls, params, targets, ptf, backward=True, pack=True):
    """The per-object work of derender3d/models/__init__.py:161-224 + the loss of scripts/main.py:445-453, for the 16
    objects of a frame in one batch of launches.  pack: return the three maps as ONE [n, 5, R, R] tensor (the payload of
    the multi-GPU all_gather; a single GPU has no use for that copy and gets the tuple)."""
    from derender3d.models.renderer import Renderer
    from derender3d.losses import silhouette_ffd_loss
    from sdn_hip import ops
    n = OBJECTS_PER_FRAME
    renderer = Renderer(image_size=RENDER_SIZE)
    renderer.viewing_angle = [np.arctan(RENDER_SIZE / (2.0 * FOCAL)) / np.pi * 180] * n
    zoom_to = torch.full((n, 1), RENDER_SIZE / (2.0 * FOCAL), device=device)
    cls_t = torch.tensor(cls, device=device, dtype=torch.int64)
    interests = torch.ones(n, dtype=torch.bool)

    def step():
        verts, faces = bank.decode(params['ffd'], cls_t)
        # derender3d/models/__init__.py:106-116 (quaternion of the yaw, exp of the log scales): one fused op, as Derenderer3d._pose
        rot, scales = ops.PoseParamsFn.apply(params['theta'], params['log_scale'])
        tr = params['translation']
        verts, zooms = ptf(verts, scales=scales, rotations=rot, translations=tr, perspective_translations=tr, zoom_tos=zoom_to)
        mask, normal, depth = renderer.render_maps(verts, faces)
        if backward:
            # scripts/main.py:445-451: mean(mse_loss(masks, target, reduce=False) + 100 * mean(ffd ** 2)), one fused op
            loss = silhouette_ffd_loss(mask, targets, params['ffd'])
            for p in params.values():
                p.grad = None
            loss.backward()
        if pack == 'frame':
            # SURVEY 8(e)'s preferred payload: the frame's objects composited on the device (sdn_composite_frame, the
            # reference's main.py:541-602) -> ONE [5, 375, 1242] map per frame = 9.3 MB instead of 16 x 2.95 MB
            from derender3d import compositing as comp
            with torch.no_grad():
                tz = tr[:, 2:3].abs()
                c2d = torch.stack([tr[:, 1] / tz[:, 0], tr[:, 0] / tz[:, 0]], 1)
                inst, nrm, dep, _ = comp.composite_frame(mask.detach(), normal.detach(), depth.detach(), tz, zooms.detach(),
                                                          c2d, interests, FOCAL, 620.5, 187.0, 375, 1242, RENDER_SIZE)
            return torch.cat([inst, nrm, dep], dim=0)[None]
        return torch.cat([mask, normal, depth], dim=1) if pack else (mask, normal, depth)

    return step


def cpu_baseline(time_cap_s=25.0, max_objects=20):
    """The CPU oracle (restatement of the reference's kernels, OpenMP over pixels) on the same workload: per object ONE
    rgb+alpha+depth rasterisation at 768^2 + the silhouette backward (the reference would rasterise three times).
    Protocol (BASELINE.md section 3 asks for 5 warm-up + 20 timed objects, median): an object costs ~10 s of host time here,
    so the 25-object protocol is replaced by an explicit TIME CAP -- one warm-up object, then timed objects (different
    templates) until `time_cap_s` is spent (at least 2, at most `max_objects`); the counts are reported.  Per-phase
    seconds: K2+K3 (safe forward rasterisation, rasterize.py:238-360 + K4 sampling), K5 (edge gradient, :523-745) and the
    torch glue around them (camera, gather, pooling, autograd)."""
    from oracle import nr_oracle as no
    from oracle import raster_np as rn
    from sdn_hip import synth
    from util import posed_mesh
    phase = {'raster_forward': 0.0, 'raster_backward': 0.0}
    real_fwd, real_bwd = rn.forward, rn.backward

    def timed_fwd(*a, **k):
        t = time.time()
        try:
            return real_fwd(*a, **k)
        finally:
            phase['raster_forward'] += time.time() - t

    def timed_bwd(*a, **k):
        t = time.time()
        try:
            return real_bwd(*a, **k)
        finally:
            phase['raster_backward'] += time.time() - t

    def one(seed):
        # the SAME template family as the headline's timed region
        v, f = synth.cad_like(46000, seed=seed) if HEADLINE_MESH == 'cad_like' else synth.car_like(N_TRIS, seed=seed)
        pv, ang = posed_mesh(v, f)
        r = no.NRRenderer()
        r.image_size = RENDER_SIZE
        r.viewing_angle = ang
        r.camera_mode = 'look'
        r.eye = torch.zeros(1, 3)
        r.camera_direction = torch.tensor([[0., 0., -1.]])
        r.up = torch.tensor([[0., 1., 0.]])
        vt = (torch.tensor(pv) * torch.tensor([-1., 1., 1.])).requires_grad_(True)
        fi = torch.tensor(f[None])
        t0 = time.time()
        filled = r._fill_back(fi)
        normals = r.face_normals(vt, filled)
        tex = normals[:, :, None, None, None, :].repeat(1, 1, 2, 2, 2, 1)
        faces9 = no.vertices_to_faces(r._camera(vt), filled)
        out = no.rasterize_rgbad(faces9, tex, RENDER_SIZE, True, 0.1, 100, 1e-3, (0, 0, 0), True, True, True)
        target = torch.zeros(1, RENDER_SIZE, RENDER_SIZE)
        target[:, 120:270, 40:340] = 1
        ((out['alpha'] - target) ** 2).mean().backward()
        return time.time() - t0, 2 * f.shape[0]
    rn.forward, rn.backward = timed_fwd, timed_bwd
    try:
        one(100)                                   # warm-up (page-in, OpenMP pool)
        for k in phase:
            phase[k] = 0.0
        times, faces = [], 0
        t_start = time.time()
        while len(times) < max_objects and (len(times) < 2 or time.time() - t_start < time_cap_s):
            dt, faces = one(101 + len(times))
            times.append(dt)
    finally:
        rn.forward, rn.backward = real_fwd, real_bwd
    med = float(np.median(times))
    total = float(np.sum(times))
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = None
    return {'value': 1.0 / med, 'unit': 'objects/s', 'cores': rn.num_threads(), 'kind': 'port',
            'affinity_cpus': affinity, 'omp_num_threads_env': os.environ.get('OMP_NUM_THREADS'), 'cpu_count': os.cpu_count(),
            'timed_objects': len(times), 'warmup_objects': 1, 'time_cap_s': time_cap_s,
            'phase_seconds_per_object': {'K2+K3+K4 forward rasterisation': phase['raster_forward'] / len(times),
                                         'K5 edge gradient (+K6/K7)': phase['raster_backward'] / len(times),
                                         'torch glue (camera, gather, pooling, autograd)':
                                             (total - phase['raster_forward'] - phase['raster_backward']) / len(times)},
            'mesh': HEADLINE_MESH,
            'sample': '%d objects after 1 warm-up under a %.0f s time cap (BASELINE.md asks for 5 + 20: ~10 s per object here); '
                      'each a %s template of %d faces (the headline\'s family), 768^2: ONE rgb+alpha+depth rasterisation + '
                      'silhouette backward (the reference would rasterise three times; no FFD / transform); seconds per '
                      'object %s, median %.1f'
                      % (len(times), time_cap_s, HEADLINE_MESH, faces, ['%.1f' % t for t in times], med)}


def derender3d_loop(device, n_opts=20, mesh=None):
    """configs[2]: one VKITTI frame's 16 objects through the derender3d branch as geometric/scripts/main.py:375-456 runs it.
      (a) inference: ResNet-18 encoder on 16 crops [16,3,224,224] + pose algebra + FFD decode + PerspectiveTransform +
          silhouette / normal / depth at render_size 384 (Derenderer3d.forward, eval mode);
      (b) the test-time optimisation loop (:404-456): model in train mode with _force_no_sample, Adam(lr 3e-2) over
          _theta_deltas / _translation2ds / _log_scales / _ffd_coeffs, per iteration render -> MSE(mask) + 100 mean(ffd^2)
          -> backward -> step; `n_opts` iterations (the reference's --num_opts; its default is 0, 20 is the benchmark
          setting of SURVEY.md 8d).  The reference prints loss.item() every iteration (a host sync); here the loop runs
          without host synchronisation.
    Random-init encoder (no ImageNet file here), synthetic crops and rois, 8 procedural templates of the `mesh` family
    (default: the headline's; this is the DROP-IN route -- the reference's unmodified loop on the product's Derenderer3d --
    next to the fused frame step the headline times)."""
    from derender3d import TargetType
    from derender3d.models import Derenderer3d, ShapenetObj
    from sdn_hip import synth
    mesh = mesh or HEADLINE_MESH
    objs = []
    for k in range(8):
        v, f = synth.cad_like(46000, seed=100 + k) if mesh == 'cad_like' else synth.car_like(N_TRIS, seed=100 + k)
        objs.append(ShapenetObj(vertices=v[:, [2, 1, 0]] * np.asarray([-1, 1, 1], np.float32), faces=f))
    torch.manual_seed(7)
    model = Derenderer3d(mode=TargetType.extend, image_size=256, render_size=RENDER_SIZE, objs=objs).to(device)
    n = OBJECTS_PER_FRAME
    rng = np.random.default_rng(1236)
    images = torch.tensor(rng.normal(size=(n, 3, 224, 224)).astype(np.float32), device=device)
    c = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.6, 0.6, n)], 1)
    h, w = rng.uniform(40, 150, n) / FOCAL, rng.uniform(60, 300, n) / FOCAL
    rois = torch.tensor(np.stack([c[:, 0] - h / 2, c[:, 1] - w / 2, c[:, 0] + h / 2, c[:, 1] + w / 2], 1).astype(np.float32),
                        device=device)
    focals = torch.full((n, 1), FOCAL, device=device)
    masks = torch.zeros(n, 1, RENDER_SIZE, RENDER_SIZE, device=device)
    masks[:, :, 120:270, 40:340] = 1

    def timed(fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    model.eval()

    def encoder_only():
        with torch.no_grad():
            return model.derenderer(images, (rois[:, 2:4] + rois[:, 0:2]) / 2, rois[:, 2:4] - rois[:, 0:2])

    def inference():
        with torch.no_grad():
            return model(images, rois, focals)
    out = {'objects': n, 'num_opts': n_opts, 'mesh': mesh}
    out['encoder_fwd_ms'] = timed(encoder_only, 2, 5)
    out['inference_ms'] = timed(inference, 2, 5)
    blob = inference()

    def optimise():
        model.train()
        model._force_no_sample = True
        b = {k: (v.clone().detach() if isinstance(v, torch.Tensor) else v) for k, v in blob.items()}
        params = {k: b[k].requires_grad_() for k in ('_theta_deltas', '_translation2ds', '_log_scales', '_ffd_coeffs')}
        opt = torch.optim.Adam(params.values(), lr=3e-2)
        for _ in range(n_opts):
            opt.zero_grad()
            b.update(model.render(b))
            loss = torch.nn.functional.mse_loss(b['_masks'], masks, reduction='none') + 100 * torch.mean(b['_ffd_coeffs'] ** 2)
            loss.mean().backward()
            opt.step()
        model.eval()
        model._force_no_sample = False
        return loss
    ms = timed(optimise, 1, 3)
    if os.environ.get('SDN_BENCH_HOST_PROFILE') == '1':   # development aid: where the loop's HOST time goes (stderr)
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            optimise()
            torch.cuda.synchronize()
        print(prof.key_averages().table(sort_by='self_cpu_time_total', row_limit=40, max_name_column_width=56), file=sys.stderr)
    out['optimisation_ms'] = ms
    out['optimisation_ms_per_iteration'] = ms / n_opts
    out['optimisation_objects_per_s'] = n * n_opts / (ms * 1e-3)
    # encoder training step (REINFORCE branch of main.py:114-154): forward + backward through encoder and renderer
    model.train()
    model._force_no_sample = False

    def train_step():
        for p in model.parameters():
            p.grad = None
        bl = model(images, rois, focals)
        mask_loss = ((bl['_masks'] - masks) ** 2).mean()
        reward = (bl['_class_log_probs'] * mask_loss.detach()).mean()
        (mask_loss + reward + 1e-2 * (bl['_ffd_coeffs'] ** 2).mean()).backward()
    out['train_step_ms'] = timed(train_step, 2, 3)
    model.eval()
    out['workload'] = ('configs[2]: 16 objects per frame, crops 224^2, ResNet-18 encoder + pose / FFD decode + three maps at '
                       '384 (768^2 internal), %d Adam iterations' % n_opts)
    return out


PIPE_FRAMES, PIPE_OBJECTS = 64, 10


PIPE_BATCH = 4   # frames per fake_inference call of stage B (frames are independent: textural/edit_vkitti.py:105)


def edit_pipeline(device, world, rank, n_frames=PIPE_FRAMES, n_obj=PIPE_OBJECTS, batch=PIPE_BATCH):
    """configs[4]: the full geometric + textural edit pipeline on synthetic VKITTI-shaped frames, FRAMES sharded by rank.
    Per frame (geometric/scripts/main.py:375-622, textural/data/vkitti_dataset.py:44-142, textural/edit_vkitti.py:105):
      A  derender3d inference for the frame's objects: ResNet-18 encoder on the crops, pose / FFD decode, silhouette +
         normal + depth at 384 (Derenderer3d.forward);  compositing of the objects into the 375 x 1242 frame
         (sdn_composite_frame, bit-identical to the PIL path) -> [5, 375, 1242] = instance, normal xyz, depth;
      -- ONE all_gather of the ranks' composited maps [f_r, 5, 375, 1242] (the path's only exchange) --
      B  wire-format quantisation, textural input assembly on the device (label / instance merge, pose bins, normal bias,
         make_power_2 -> 368 x 1248), Pix2PixHDModel.fake_inference (feature encoder + generator) on `batch` frames at a time
         (r05; the reference's loop feeds one frame per call -- at batch 1 the generator's grids cannot fill the chip).
    Frame f draws its inputs from seed 5000 + f whatever the rank, so the gathered maps -- and their checksum -- do not
    depend on the number of ranks beyond the run-to-run noise of the encoder's K-split float atomics (~3e-6 of the checksum:
    108618201.99 / 108618530.55 at N = 1 on two boxes, 108618538.26 from two ranks, profiles/r05x_share2_full.json).
    Random-init networks, procedural templates."""
    tex_dir = os.path.join(ROOT, '3d-sdn_amd', 'textural')
    if tex_dir not in sys.path:
        sys.path.insert(0, tex_dir)
    from data import assemble as asm
    from derender3d import TargetType
    from derender3d import compositing as comp
    from derender3d.models import Derenderer3d, ShapenetObj
    from models.pix2pixHD_model import Pix2PixHDModel, default_options
    from sdn_hip import dist as sdist
    from sdn_hip import synth
    H, W, R = 375, 1242, RENDER_SIZE
    objs = []
    for k in range(8):
        v, f = synth.car_like(N_TRIS, seed=100 + k)
        objs.append(ShapenetObj(vertices=v[:, [2, 1, 0]] * np.asarray([-1, 1, 1], np.float32), faces=f))
    torch.manual_seed(11)
    geo = Derenderer3d(mode=TargetType.extend, image_size=256, render_size=R, objs=objs).to(device).eval()
    opt = default_options(gpu_ids=[device.index], batchSize=1, num_D=3, feat_pose='1', feat_normal='1', no_vgg_loss=True,
                          isTrain=True, resize_or_crop='none', loadSize=1248, fineWidth=1248, fineHeight=368, no_flip=True,
                          segm_precomputed_path='geometric', inst_precomputed_path='geometric')
    torch.manual_seed(12)
    tex = Pix2PixHDModel()   # built as for training: inference mode would load a checkpoint (base_model.py), none exists here
    tex.initialize(opt)
    lo, hi = sdist.shard_range(n_frames, rank, world)

    def frame_inputs(f):
        rng = np.random.default_rng(5000 + f)
        images = torch.tensor(rng.normal(size=(n_obj, 3, 224, 224)).astype(np.float32), device=device)
        c = np.stack([rng.uniform(-0.12, 0.12, n_obj), rng.uniform(-0.7, 0.7, n_obj)], 1)
        h, w = rng.uniform(40, 150, n_obj) / FOCAL, rng.uniform(60, 300, n_obj) / FOCAL
        rois = torch.tensor(np.stack([c[:, 0] - h / 2, c[:, 1] - w / 2, c[:, 0] + h / 2, c[:, 1] + w / 2], 1)
                            .astype(np.float32), device=device)
        segm = torch.tensor(rng.integers(0, 13, (1, H, W), dtype=np.uint8), device=device)
        image = torch.tensor(rng.integers(0, 256, (3, H, W), dtype=np.uint8), device=device)
        return images, rois, segm, image
    inputs = [frame_inputs(f) for f in range(lo, hi)]   # resident in HBM before the timed region
    focals = torch.full((n_obj, 1), FOCAL, device=device)
    interests = torch.ones(n_obj, dtype=torch.bool)
    params = {'crop_pos': (0, 0), 'flip': False}

    def stage_a(images, rois):
        with torch.no_grad():
            blob = geo(images, rois, focals)
            inst, nrm, dep, order = comp.composite_frame(blob['_masks'], blob['_normals'], blob['_depth_maps'], blob['_depths'],
                                                         blob['_zooms'], blob['_center2ds'], interests, FOCAL, 620.5, 187.0,
                                                         H, W, R)
        classes = torch.argmax(blob['_class_probs'], dim=1)
        js = comp.frame_json(order, interests.tolist(), [1] * n_obj, blob['_depths'][:, 0].tolist(),
                             blob['_alphas'][:, 0].tolist())
        del classes
        return torch.cat([inst, nrm, dep], dim=0), js

    def stage_a_all(frames):
        # r05: the derender3d inference of ALL this rank's frames is issued first; the handful of per-object scalars the
        # compositing geometry and the JSON records need on the host come back in ONE copy (compositing.host_state), then
        # the compositing launches follow -- the per-frame form above reads five small tensors back per frame, each a device
        # synchronisation with an empty queue behind it
        blobs = []
        with torch.no_grad():
            # the encoder and the renderer see `batch` frames' objects at once (ResNet-18 on 10 crops is launch-bound: ~60
            # launches whatever the batch); per-object results do not depend on the batch (BatchNorm in eval mode)
            for g0 in range(0, len(frames), max(1, batch)):
                fs = frames[g0:g0 + max(1, batch)]
                big = geo(torch.cat([inputs[f - lo][0] for f in fs]), torch.cat([inputs[f - lo][1] for f in fs]),
                          focals.repeat(len(fs), 1))
                for k in range(len(fs)):
                    blobs.append({key: (v[k * n_obj:(k + 1) * n_obj] if isinstance(v, torch.Tensor) and v.dim() >= 1
                                        and v.shape[0] == len(fs) * n_obj else v) for key, v in big.items()})
            if not blobs:
                return []
            st = lambda key: torch.stack([b[key] for b in blobs])   # noqa: E731
            host = comp.host_state(st('_depths'), st('_zooms'), st('_center2ds'), st('_alphas'))
            out = []
            for k, blob in enumerate(blobs):
                inst, nrm, dep, order = comp.composite_frame(blob['_masks'], blob['_normals'], blob['_depth_maps'], blob['_depths'],
                                                             blob['_zooms'], blob['_center2ds'], [True] * n_obj, FOCAL, 620.5, 187.0,
                                                             H, W, R, host=host[k])
                js = comp.frame_json(order, [True] * n_obj, [1] * n_obj, host[k][:, 0].tolist(), host[k][:, 4].tolist())
                out.append((torch.cat([inst, nrm, dep], dim=0), js))
        return out

    def stage_b(maps, js, segm, image):
        inst_u8, nrm_u8, _ = comp.wire_tensors(maps[0:1], maps[1:4], maps[4:5])
        item = asm.assemble_item(opt, params, segm, image, inst=inst_u8, pose_inst=inst_u8,
                                 pose_json={str(k): v for k, v in js.items()}, normal=nrm_u8)
        return tex.fake_inference(item['image'][None], item['label'][None], item['inst'][None].clone(),
                                  pose=item['pose'][None].float(), normal=item['normal'][None])

    def stage_b_batch(fs, maps_list, js_list):
        items = []
        for f, maps, js in zip(fs, maps_list, js_list):
            inst_u8, nrm_u8, _ = comp.wire_tensors(maps[0:1], maps[1:4], maps[4:5])
            items.append(asm.assemble_item(opt, params, inputs[f - lo][2], inputs[f - lo][3], inst=inst_u8, pose_inst=inst_u8,
                                           pose_json={str(k): v for k, v in js.items()}, normal=nrm_u8))
        cat = lambda key: torch.stack([it[key] for it in items])
        out = tex.fake_inference(cat('image'), cat('label'), cat('inst').clone(), pose=cat('pose').float(), normal=cat('normal'))
        return [out[k:k + 1] for k in range(len(fs))]

    def run():
        if batch > 1:
            gathered, outs, _ = sdist.run_frames(
                n_frames, None, stage_b_batch, lambda: torch.zeros(0, 5, H, W, device=device), batch=batch,
                stage_a_all=stage_a_all)
            return gathered, outs
        gathered, outs, _ = sdist.run_frames(
            n_frames, lambda f: stage_a(inputs[f - lo][0], inputs[f - lo][1]),
            lambda f, maps, js: stage_b(maps, js, inputs[f - lo][2], inputs[f - lo][3]),
            lambda: torch.zeros(0, 5, H, W, device=device))
        return gathered, outs
    run()                                    # warm-up (chains compiled, tables cached)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    # three timed passes, the median reported: the stage is host-paced and a single 0.4 s pass moved between 6.0 and 8.9 ms per
    # frame from one run to the next on the same tree (profiles/r05n_pipe_lab.log)
    passes = []
    gathered = outs = None
    for _ in range(3):
        # the previous pass's results (1 GB: 64 frames of maps and generated images) are released first: with them alive the
        # caching allocator has to hipMalloc a second set, and that pass took 0.9-2.8 s instead of 0.4 (r05x / r05zb logs)
        gathered = outs = None
        t0 = time.perf_counter()
        gathered, outs = run()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        passes.append(elapsed)
    elapsed = sorted(passes)[1]
    if os.environ.get('SDN_BENCH_HOST_PROFILE') == '1':   # development aid: where the pipeline's HOST time goes (stderr)
        from torch.profiler import ProfilerActivity, profile
        try:   # without the verbose switch this torch build records empty Python stacks
            cfg = torch._C._profiler._ExperimentalConfig(verbose=True)
        except Exception:
            cfg = None
        with profile(activities=[ProfilerActivity.CPU], with_stack=True, experimental_config=cfg) as prof:
            run()
            torch.cuda.synchronize()
        print(prof.key_averages().table(sort_by='self_cpu_time_total', row_limit=25, max_name_column_width=56), file=sys.stderr)
        import collections
        agg = collections.defaultdict(lambda: [0, 0.0])   # the host-blocking ops by the repo lines that issue them
        for ev in prof.events():
            if ev.name not in ('aten::_local_scalar_dense', 'aten::_to_copy', 'aten::_unique2', 'aten::copy_', 'aten::nonzero'):
                continue
            frames = [fr.replace(ROOT + '/', '') for fr in (ev.stack or []) if '/torch/' not in fr and 'host_profile' not in fr][:3]
            agg[(ev.name, ' <- '.join(frames))][0] += 1
            agg[(ev.name, ' <- '.join(frames))][1] += ev.self_cpu_time_total
        for (name, where), (cnt, us) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:40]:
            print('%9.1f us %5d x  %-26s %s' % (us, cnt, name, where), file=sys.stderr)
    return {'workload': 'configs[4]: %d frames x %d objects (375x1242), frames sharded over %d rank(s): derender3d inference '
                        '+ compositing -> all_gather of [f_r,5,375,1242] maps -> input assembly + fake_inference at 368x1248, '
                        '%d frames per call' % (n_frames, n_obj, world, batch),
            'stage_b_batch': batch,
            'frames': n_frames, 'objects_per_frame': n_obj, 'seconds': elapsed, 'seconds_of_each_pass': passes, 'frames_per_s': n_frames / elapsed,
            'objects_per_s': n_frames * n_obj / elapsed, 'ms_per_frame_per_gpu': elapsed / max(1, hi - lo) * 1e3,
            'allgather_payload_bytes_per_rank': (hi - lo) * 5 * H * W * 4 if world > 1 else 0,
            'gathered_maps_checksum': float(gathered.double().sum().item()),
            'generated_checksum_rank0': float(sum(o.double().abs().sum().item() for o in outs)),
            'generated_shape': list(outs[0].shape) if outs else None}


def compositing_numbers(device, with_cpu):
    """the 16 objects of a 375 x 1242 frame composited on the device (one kernel, bit-identical to
    the reference's PIL path, geometric/scripts/main.py:541-602), next to that PIL path (oracle/composite_oracle.py)
    timed on the host -- the per-frame step that follows the renderer."""
    sys.path.insert(0, os.path.join(ROOT, '3d-sdn_amd', 'geometric'))
    from derender3d import compositing as comp
    n, R, H, W = OBJECTS_PER_FRAME, RENDER_SIZE, 375, 1242
    g = torch.Generator().manual_seed(55)
    base = torch.rand(n, 1, R // 8, R // 8, generator=g)
    masks = torch.nn.functional.interpolate((base > 0.45).float(), size=(R, R), mode='bilinear', align_corners=False)
    normals = torch.nn.functional.normalize(torch.randn(n, 3, R, R, generator=g), dim=1) * masks
    depth_maps = torch.rand(n, 1, R, R, generator=g) * 80 + 1
    depths = torch.rand(n, 1, generator=g) * 40 + 3
    zooms = torch.rand(n, generator=g) * 3 + 0.5
    c2d = torch.stack([(torch.rand(n, generator=g) - 0.5) * 0.5, (torch.rand(n, generator=g) - 0.5) * 1.9], 1)
    interests = torch.ones(n, dtype=torch.bool)
    dev = [t.to(device) for t in (masks, normals, depth_maps, depths, zooms, c2d, interests)]
    args = (725.0, 620.5, 187.0, H, W, R)
    comp.composite_frame(*dev, *args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        comp.composite_frame(*dev, *args)
    torch.cuda.synchronize()
    out = {'device_ms_per_frame': (time.perf_counter() - t0) / 5 * 1e3, 'objects': n,
           'note': 'includes the host-side Pillow coefficient tables; inputs resident on the GPU'}
    if with_cpu:
        from oracle import composite_oracle as co
        t0 = time.perf_counter()
        co.composite_frame(masks, normals, depth_maps, depths, zooms, c2d, interests, *args)
        out['cpu_pil_ms_per_frame'] = (time.perf_counter() - t0) * 1e3
    return out


TEX_BATCH, TEX_H, TEX_W = 4, 384, 1248
# conv flops (2 MAC) per image at 384x1248, counted from the reference modules (SURVEY.md Appendix C / BASELINE.md)
TEX_GFLOP_G, TEX_GFLOP_D3, TEX_GFLOP_E = 930.6, 71.5, 14.8


def textural_batch(model, device, seed, n=TEX_BATCH, h=TEX_H, w=TEX_W):
    """Synthetic VKITTI-shaped batch: label ids, instance ids (10 rectangles), image / normal in [-1, 1], pose bins."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    label = torch.randint(1, 14, (n, 1, h, w), generator=g).float()
    inst = torch.zeros(n, 1, h, w)
    pose = torch.zeros(n, 1, h, w)
    for b in range(n):
        for k in range(10):
            y0, x0 = int(torch.randint(0, h - 60, (1,), generator=g)), int(torch.randint(0, w - 200, (1,), generator=g))
            hh, ww = int(torch.randint(40, h // 2, (1,), generator=g)), int(torch.randint(60, w // 4, (1,), generator=g))
            inst[b, 0, y0:y0 + hh, x0:x0 + ww] = 1000 * (k + 1)
            pose[b, 0, y0:y0 + hh, x0:x0 + ww] = int(torch.randint(1, 25, (1,), generator=g))
    image = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    normal = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    return [t.to(device) for t in (label, inst, image, pose, normal)]


def textural_reference_default(device, steps=3):
    """The reference's OWN default training configuration (textural/options/base_options.py:36-39, train_options.py:28:
    batch 1, 192 x 624 crop, 2-scale discriminator), timed the same way -- SURVEY.md F6 asks for both."""
    sys.path.insert(0, os.path.join(ROOT, '3d-sdn_amd', 'textural'))
    from models.pix2pixHD_model import Pix2PixHDModel, default_options
    opt = default_options(gpu_ids=[device.index], batchSize=1, num_D=2, feat_pose='1', feat_normal='1',
                          no_vgg_loss=True, isTrain=True)
    torch.manual_seed(4322)
    model = Pix2PixHDModel()
    model.initialize(opt)
    label, inst, image, pose, normal = textural_batch(model, device, 78, 1, 192, 624)
    for _ in range(2):
        model.train_step(label, inst.clone(), image, None, pose, normal)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.train_step(label, inst.clone(), image, None, pose, normal)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    gflop = 3 * 232.7 + 3 * 3.7 + 8 * 17.7  # per image at 192 x 624, 2-scale D
    return {'ms_per_step': ms, 'steps': steps, 'tflops_algorithmic': gflop / ms,
            'config': 'reference default: bs 1, 192x624, num_D 2, no VGG loss'}


def textural_extras(device):
    """Two more numbers SURVEY.md 8(d) asks for, on the headline shapes: the GAN train step WITH the VGG19 perceptual
    loss (random-init VGG: the pretrained file cannot be downloaded) and configs[4]'s per-frame generator inference
    (Pix2PixHDModel.fake_inference, batch 1, encoder + generator forward)."""
    sys.path.insert(0, os.path.join(ROOT, '3d-sdn_amd', 'textural'))
    from models.pix2pixHD_model import Pix2PixHDModel, default_options
    opt = default_options(gpu_ids=[device.index], batchSize=TEX_BATCH, num_D=3, feat_pose='1', feat_normal='1',
                          no_vgg_loss=False, isTrain=True)
    torch.manual_seed(4323)
    model = Pix2PixHDModel()
    model.initialize(opt)
    label, inst, image, pose, normal = textural_batch(model, device, 79)

    def timed(fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    out = {}
    out['gan_step_with_vgg_ms'] = timed(lambda: model.train_step(label, inst.clone(), image, None, pose, normal), 1, 2)
    one = [t[:1].contiguous() for t in (image, label, inst, pose, normal)]
    out['fake_inference_bs1_ms'] = timed(
        lambda: model.fake_inference(one[0], one[1], one[2].clone(), pose=one[3], normal=one[4]), 2, 5)
    out['config'] = 'bs %d (train) / bs 1 (inference) at %dx%d, 3-scale D, random-init VGG19' % (TEX_BATCH, TEX_H, TEX_W)
    return out


def host_issue_ms(step, repeats=3):
    """Host time to ISSUE one step into an empty queue (min of `repeats`, each after a device synchronise): what the host
    costs per step when it is not waiting for the GPU.  `host_enqueue_ms_per_step` (the K timed steps issued back to back)
    cannot say that once the step is GPU-bound: the HIP queue is finite, so the host ends up waiting for the device."""
    best = float('inf')
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        step()
        best = min(best, time.perf_counter() - t)
    torch.cuda.synchronize()
    return best * 1e3


def textural_leg(device, steps, warmup, world):
    """K train steps of the textural GAN on this rank (replicas: the reference's only multi-GPU mode is DataParallel)."""
    sys.path.insert(0, os.path.join(ROOT, '3d-sdn_amd', 'textural'))
    from models.pix2pixHD_model import Pix2PixHDModel, default_options
    import sdn_hip
    opt = default_options(gpu_ids=[device.index], batchSize=TEX_BATCH, num_D=3, feat_pose='1', feat_normal='1',
                          no_vgg_loss=True, isTrain=True)
    torch.manual_seed(4321)
    model = Pix2PixHDModel()
    model.initialize(opt)
    label, inst, image, pose, normal = textural_batch(model, device, 77)

    def step():
        return model.train_step(label, inst.clone(), image, None, pose, normal)
    for _ in range(warmup):
        step()
    issue_ms = host_issue_ms(step)
    if world > 1:
        dist.barrier()
    sdn_hip.timing_enable(True)
    for slot in (sdn_hip.SLOT_CONV_GEMM, sdn_hip.SLOT_CONV_WGRAD, sdn_hip.SLOT_CONV_NARROW):
        sdn_hip.timing_read_slot(slot)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = step()
    enqueue = time.perf_counter() - t0   # host time to issue the steps' ~1800 launches each (the GPU runs behind it)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    gemm_ms, gemm_n, gemm_fl = sdn_hip.timing_read_slot(sdn_hip.SLOT_CONV_GEMM)
    wg_ms, wg_n, wg_fl = sdn_hip.timing_read_slot(sdn_hip.SLOT_CONV_WGRAD)
    nr_ms, nr_n, nr_fl = sdn_hip.timing_read_slot(sdn_hip.SLOT_CONV_NARROW)
    # The product runs the coarse discriminator columns and the weight gradients on side streams: kernels overlap, so
    # the per-launch durations above include the time a kernel shares the chip with others.  Two more steps with the
    # side streams off give the kernels' own durations (outside the timed region; reported next to the figures above).
    saved = {k: os.environ.get(k) for k in ('SDN_D_STREAMS', 'SDN_WGRAD_STREAM', 'SDN_UPDATE_STREAM')}
    os.environ['SDN_D_STREAMS'] = os.environ['SDN_WGRAD_STREAM'] = os.environ['SDN_UPDATE_STREAM'] = '0'
    step()
    torch.cuda.synchronize()
    for slot in (sdn_hip.SLOT_CONV_GEMM, sdn_hip.SLOT_CONV_WGRAD, sdn_hip.SLOT_CONV_NARROW):
        sdn_hip.timing_read_slot(slot)
    t1 = time.perf_counter()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    serial_ms = (time.perf_counter() - t1) / 2 * 1e3
    sg_ms, sg_n, sg_fl = sdn_hip.timing_read_slot(sdn_hip.SLOT_CONV_GEMM)
    sw_ms, sw_n, sw_fl = sdn_hip.timing_read_slot(sdn_hip.SLOT_CONV_WGRAD)
    sn_ms, sn_n, sn_fl = sdn_hip.timing_read_slot(sdn_hip.SLOT_CONV_NARROW)
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    sdn_hip.timing_enable(False)
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms = elapsed / steps * 1e3
    # algorithmic conv flops of one step as executed: G and E forward + data + weight gradients (3x), D: two forwards
    # (the fake image is scored once for both losses), two full backwards (loss_D) and one data-only backward (loss_G;
    # weights detached) -- see pix2pixHD_model.py's docstring; the reference executes 9 D units for the same updates
    step_gflop = TEX_BATCH * (3 * TEX_GFLOP_G + 3 * TEX_GFLOP_E + 7 * TEX_GFLOP_D3)
    from sdn_hip import conv as hc
    prec = hc.default_precision()
    ach = gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    return {
        'ms_per_step': ms, 'steps': steps, 'warmup': warmup, 'host_enqueue_ms_per_step': enqueue / steps * 1e3,
        'host_issue_ms_one_step': issue_ms,
        'config': {'workload': 'configs[3]: pix2pixHD GlobalGenerator(48->3, ngf 64, 4 down, 9 blocks) + 3-scale '
                               'discriminator + encoder train step, bs %d at %dx%d (375x1242 padded to /16), no VGG loss'
                               % (TEX_BATCH, TEX_H, TEX_W),
                   'precision': 'bf16x3 split MFMA, fp32 accumulate' if prec == 3 else 'bf16 MFMA, fp32 accumulate'},
        'step_tflop_algorithmic': step_gflop / 1e3,
        'tflops_algorithmic': step_gflop / ms,
        'images_per_s': world * TEX_BATCH / (ms * 1e-3),
        'losses': {k: (float(v.detach()) if isinstance(v, torch.Tensor) else float(v)) for k, v in losses.items()},
        'roofline': {'bound': 'mfma', 'kernel': 'every MFMA forward / data-gradient launch: ' + ' + '.join(k.split('::')[1] for k in TEX_GEMM_GROUP)
                               + ' (one timing slot; flops declared from the layers\' TRUE channel counts since r05; the '
                               'fp32 head kernels k_conv_narrow_fwd / k_wgrad_narrow are timed apart, see `narrow`)',
                     'achieved': ach, 'peak': 2500.0, 'unit': 'TFLOP/s',
                     'frac': ach / 2500.0, 'issued_frac': ach * (3 if prec == 3 else 1) / 2500.0,
                     # the bf16x3 scheme issues 3 MFMAs per algorithmic product: its ceiling is a third of the bf16 peak
                     'frac_of_split_ceiling': ach / (2500.0 / 3) if prec == 3 else ach / 2500.0,
                     'traffic_stale': bool((_pmc_traffic(TEX_GEMM_GROUP, 'pmc_tex_')[1] or '').count('STALE')),
                     'traffic': _pmc_traffic(TEX_GEMM_GROUP, 'pmc_tex_')[0],
                     'traffic_source': _pmc_traffic(TEX_GEMM_GROUP, 'pmc_tex_')[1],
                     'issued_frac_all_mfma_launches': ((gemm_fl + wg_fl) * (3 if prec == 3 else 1) / ((gemm_ms + wg_ms) * 1e-3)
                                                       / 1e12 / 2500.0) if gemm_ms + wg_ms > 0 else 0.0,
                     'launches': gemm_n, 'avg_launch_us': gemm_ms * 1e3 / max(gemm_n, 1),
                     'kernel_ms_per_step': gemm_ms / steps,
                     'wgrad': {'kernel': 'k_wgrad_tile + k_conv_wgrad', 'achieved': wg_fl / (wg_ms * 1e-3) / 1e12 if wg_ms > 0 else 0.0,
                               'launches': wg_n, 'kernel_ms_per_step': wg_ms / steps},
                     'narrow': {'kernel': 'the 3 / 5 / 1-channel head layers: k_conv_head_mfma (r05: 7x7 forward and the stem data gradient on '
                                          'v_mfma_f32_16x16x32_bf16, 16 rows issued for 3 / 5 real ones) + k_conv_narrow_fwd (4x4 discriminator '
                                          'heads) + k_wgrad_narrow (exact fp32 on the vector ALUs); flops = the REAL channels',
                                'achieved': nr_fl / (nr_ms * 1e-3) / 1e12 if nr_ms > 0 else 0.0, 'peak': 157.3,
                                'launches': nr_n, 'kernel_ms_per_step': nr_ms / steps,
                                'single_stream_kernel_ms_per_step': sn_ms / 2},
                     'declared_tflop_per_step': (gemm_fl + wg_fl + nr_fl) / steps / 1e12,
                     'note': 'launch durations of the timed region: kernels of concurrent streams overlap (discriminator '
                             'columns, weight gradients), so a duration includes time shared with other kernels',
                     'single_stream': {
                         'ms_per_step': serial_ms,
                         'achieved': sg_fl / (sg_ms * 1e-3) / 1e12 if sg_ms > 0 else 0.0,
                         'frac': sg_fl / (sg_ms * 1e-3) / 1e12 / 2500.0 if sg_ms > 0 else 0.0,
                         'issued_frac': sg_fl / (sg_ms * 1e-3) / 1e12 * (3 if prec == 3 else 1) / 2500.0 if sg_ms > 0 else 0.0,
                         'wgrad_achieved': sw_fl / (sw_ms * 1e-3) / 1e12 if sw_ms > 0 else 0.0,
                         'note': 'two extra steps with SDN_D_STREAMS=0 SDN_WGRAD_STREAM=0 (outside the timed region): '
                                 'every kernel alone on the chip'}},
    }


def cpu_baseline_textural(timed=3):
    """the G / D / E train step at batch 1, 192 x 624 (the reference's default crop, 2-scale D,
    48 input channels) in torch CPU fp32 with the reference's layer arithmetic -- oracle/textural_oracle.
    pix2pixhd_step_losses, which tests/test_trainstep_golden.py pins to the reference's own train loop -- forward, then
    loss_G.backward() and loss_D.backward() as textural/train.py:88-95 runs them (three discriminator forwards; the
    reference modules themselves cannot travel to the GPU box).  One warm-up + `timed` steps, median."""
    from oracle import textural_oracle as to
    sys.path.insert(0, os.path.join(ROOT, '3d-sdn_amd', 'textural'))
    from models import networks as N
    torch.manual_seed(1)
    G = N.define_G(48, 3, 64, 'global', 4, 9)
    D = N.define_D(18, 64, 3, 'instance', False, 2, True)
    E = N.define_G(3, 5, 16, 'encoder', 4)
    ps = []

    def leaves(net):
        sd = dict(net.state_dict())
        for k, v in list(sd.items()):
            if k.endswith('weight') or k.endswith('bias'):
                sd[k] = v.clone().requires_grad_(True)
                ps.append(sd[k])
        return sd
    sdG, sdD, sdE = leaves(G), leaves(D), leaves(E)
    h, w = 192, 624
    opt = {'label_nc': 14, 'feat_pose_num_bins': 24, 'n_downsample_global': 4, 'n_blocks_global': 9, 'n_downsample_E': 4,
           'num_D': 2, 'n_layers_D': 3, 'lambda_feat': 5.0, 'lambda_L1': 10.0}
    g = torch.Generator().manual_seed(2)
    inst = torch.zeros(1, 1, h, w)
    for k in range(10):
        y0, x0 = int(torch.randint(0, h - 40, (1,), generator=g)), int(torch.randint(0, w - 120, (1,), generator=g))
        inst[0, 0, y0:y0 + 40, x0:x0 + 120] = 1000 * (k + 1)
    batch = {'label': torch.randint(0, 14, (1, 1, h, w), generator=g).float(), 'inst': inst,
             'image': torch.rand(1, 3, h, w, generator=g) * 2 - 1, 'pose': torch.randint(0, 25, (1, 1, h, w), generator=g).float(),
             'normal': torch.rand(1, 3, h, w, generator=g) * 2 - 1}
    times = []
    for i in range(timed + 1):   # one warm-up, then the median
        for p in ps:
            p.grad = None
        t0 = time.time()
        L = to.pix2pixhd_step_losses(sdG, sdD, sdE, batch, opt)
        (L['G_GAN'] + L['G_GAN_Feat'] + L['G_L1']).backward(retain_graph=True)
        ((L['D_fake'] + L['D_real']) * 0.5).backward()
        if i:
            times.append(time.time() - t0)
    dt = float(np.median(times))
    # the reference's work per image at this size: 3 G + 9 D(2 scales) + 3 E (869 GFLOP)
    gflop = (3 * TEX_GFLOP_G + 3 * TEX_GFLOP_E) * (h * w) / (TEX_H * TEX_W) + 9 * 17.7
    return {'value': dt * 1e3, 'unit': 'ms per train step (bs 1, 192x624, 2-scale D)', 'tflops': gflop / dt / 1e3,
            'cores': torch.get_num_threads(), 'kind': 'port',
            'sample': 'G/D/E train step (forward, loss_G.backward, loss_D.backward) at 1 x 48 x %d x %d, torch CPU fp32: '
                      'median %.2f s of %d after a warm-up, seconds %s' % (h, w, dt, timed, ['%.2f' % t for t in times])}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: re-execute this file under torch.distributed.run with one rank per
    GPU (what the reference does with nn.DataParallel threads inside one process, geometric/scripts/main.py:182,631, is
    one PROCESS per GPU here).  Returns the launcher's exit code; rank 0 of the children prints the JSON line."""
    import subprocess
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC: RCCL needs it on this driver
    env.setdefault('OMP_NUM_THREADS', str(max(1, (os.cpu_count() or 8) // n)))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def stub_leg(args, device, world, rank):
    """Launcher / collective check without kernels (tests/test_bench_launcher.py, gloo on CPU): the same shard ->
    all_gather -> max-over-ranks timing skeleton as geometric_leg around a trivial per-object map."""
    from sdn_hip import dist as sdist
    n = world * OBJECTS_PER_FRAME
    lo, hi = sdist.shard_range(n, rank, world)

    def full_step():
        idx = torch.arange(lo, hi, dtype=torch.float32, device=device)
        maps = idx[:, None, None, None] + torch.zeros(hi - lo, 5, 8, 8, device=device)
        return sdist.gather_maps(maps, n) if world > 1 else maps
    for _ in range(args.warmup):
        full_step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = full_step()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ok = bool(torch.equal(out[:, 0, 0, 0].cpu(), torch.arange(n, dtype=torch.float32)))
    return {'metric': 'stub objects/s (launcher test, no kernels)', 'value': n * args.steps / elapsed, 'unit': 'objects/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': elapsed / args.steps * 1e3,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': 'stub'}, 'gathered_in_item_order': ok,
            'allgather_payload_bytes_per_rank': (hi - lo) * 5 * 8 * 8 * 4 if world > 1 else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--forward-only', action='store_true')
    ap.add_argument('--no-extras', action='store_true', help='skip the secondary textural numbers (profiling runs)')
    ap.add_argument('--skip-textural', action='store_true')
    ap.add_argument('--skip-geometric', action='store_true', help='development aid: only the textural leg')
    ap.add_argument('--textural-steps', type=int, default=0, help='default: min(steps, 5)')
    ap.add_argument('--stub', action='store_true', help='launcher / collective self-test without kernels (CPU, gloo)')
    ap.add_argument('--backend', default='nccl', help="torch.distributed backend: 'nccl' (= RCCL) | 'gloo' (--stub only)")
    ap.add_argument('--share-gpu', action='store_true',
                    help='development aid, never a measurement: all N ranks use cuda:0 and talk over gloo -- the sharded code '
                         'paths with the real kernels on a box with one GPU')
    ap.add_argument('--full', action='store_true',
                    help='everything besides the headline: the textural leg, secondary meshes, K1, real meshes, host-issue '
                         'time, the ALU roofline, the blocking exchange, configs[2] / [4], compositing, CPU baselines')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (maps, parameter gradients) as DIR/<name>.npy (float32)')
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit('bench.py: --steps must be at least 1')
    if args.skip_geometric and not args.full:
        raise SystemExit('bench.py: --skip-geometric leaves only the textural leg, which runs with --full')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher of N ranks
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit('bench.py: --gpus %d but the launcher started %d rank(s); refusing to report n_gpus for a world '
                         'that does not exist' % (args.gpus, world))
    if args.stub:
        device = torch.device('cpu')
    else:
        if not torch.cuda.is_available():
            raise SystemExit('bench.py needs an MI355X: the HIP path has no CPU fallback')
        if args.share_gpu:
            args.backend, local_rank = 'gloo', 0
        elif args.backend != 'nccl':
            raise SystemExit("bench.py: the measured path runs over RCCL (backend 'nccl'); 'gloo' is for --stub")
        if world > torch.cuda.device_count() and not args.share_gpu:
            raise SystemExit('bench.py: %d ranks but %d visible GPU(s)' % (world, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        device = torch.device('cuda', local_rank)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(args.backend, rank=rank, world_size=world)
        if dist.get_world_size() != args.gpus:
            raise SystemExit('bench.py: process group has %d ranks, --gpus %d' % (dist.get_world_size(), args.gpus))
    ranks_seen = dist.get_world_size() if world > 1 else 1
    if args.stub:
        line = stub_leg(args, device, world, rank)
        line['ranks_seen'] = ranks_seen
        if rank == 0:
            print(json.dumps(line))
        if world > 1:
            dist.destroy_process_group()
        return

    import sdn_hip
    sdn_hip.lib()
    line = {}
    if not args.skip_geometric:
        line.update(geometric_leg(args, device, world, rank))
    if args.full and not args.skip_textural:
        tsteps = args.textural_steps or max(1, min(args.steps, 5))
        tex = textural_leg(device, tsteps, 1, world)
        line['textural_gan_fwd_bwd_ms'] = tex['ms_per_step']
        line['textural'] = {k: v for k, v in tex.items() if k != 'roofline'}
        line['roofline_textural'] = tex['roofline']
        if world == 1 and not args.no_extras:
            try:
                line['textural_reference_default'] = textural_reference_default(device)
            except Exception as e:
                line['textural_reference_default'] = {'ms_per_step': None, 'error': repr(e)}
            try:
                line['textural_extras'] = textural_extras(device)
            except Exception as e:
                line['textural_extras'] = {'error': repr(e)}
    else:
        line['textural_gan_fwd_bwd_ms'] = None
    if world == 1 and args.full and not args.no_extras and not args.skip_geometric:
        try:
            line['compositing'] = compositing_numbers(device, not args.no_cpu_baseline)
        except Exception as e:
            line['compositing'] = {'error': repr(e)}
        for key, mesh in (('derender3d_loop', HEADLINE_MESH), ('derender3d_loop_' + SECONDARY_MESH, SECONDARY_MESH)):
            try:   # the drop-in route (the reference's own loop) on the headline's mesh family and on the r01-r03 one
                line[key] = derender3d_loop(device, mesh=mesh)
            except Exception as e:
                line[key] = {'error': repr(e)}
    if args.full and not args.no_extras and not args.skip_geometric and not args.skip_textural:
        try:   # configs[4] runs at every N (frames sharded by rank, one all_gather)
            line['edit_pipeline'] = edit_pipeline(device, world, rank)
        except Exception as e:
            import traceback
            line['edit_pipeline'] = {'error': repr(e), 'where': traceback.format_exc()[-400:]}
    line['ranks_seen'] = ranks_seen
    if args.share_gpu:
        line['share_gpu'] = 'development run: %d ranks on ONE GPU over gloo -- not a measurement' % world
    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:
            for key, fn in (('cpu_baseline', cpu_baseline), ('cpu_baseline_textural', cpu_baseline_textural)):
                if (key == 'cpu_baseline' and args.skip_geometric) or (key != 'cpu_baseline' and args.skip_textural):
                    continue
                try:
                    line[key] = fn()
                except Exception as e:  # a baseline must never take the GPU number down with it
                    line[key] = {'value': None, 'unit': '', 'cores': 0, 'kind': 'port', 'sample': 'failed: %r' % (e,)}
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


def _pmc_traffic(kernel, prefix='pmc_'):
    """HBM bytes per launch of `kernel` (exact name) from the rocprofv3 PMC passes committed under profiles/ (collected
    by tools/gpu_prof.sh with separate `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs of this same command): 2 x FETCH_SIZE +
    WRITE_SIZE KiB (the gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md, HBM section).  Returns (bytes, source) --
    (None, None) when the passes are absent.  Counters cannot be read from inside the benchmarked process, so the source
    (file + the tag of the run that produced it) is reported next to the number."""
    try:
        f = json.load(open(os.path.join(ROOT, 'profiles', prefix + 'FETCH_SIZE.json')))
        w = json.load(open(os.path.join(ROOT, 'profiles', prefix + 'WRITE_SIZE.json')))
        tag = f.get('_tag', 'untagged')
        src = 'profiles/%sFETCH_SIZE.json + %sWRITE_SIZE.json (run %s)' % (prefix, prefix, tag)
        state = _pmc_build_state(f)
        if state != 'current':
            src += '; STALE -- ' + state
        if isinstance(kernel, str):
            return (2 * f[kernel]['FETCH_SIZE']['mean'] + w[kernel]['WRITE_SIZE']['mean']) * 1024, src
        if kernel and kernel[0] == 'sum':     # kernels that run once each per unit (the edge pair): bytes summed
            return sum((2 * f[k]['FETCH_SIZE']['mean'] + w[k]['WRITE_SIZE']['mean']) * 1024 for k in kernel[1:]), src
        # a launch group timed as one slot (the implicit-GEMM kernels): dispatch-weighted mean per launch; kernels the
        # counted run did not launch are absent from the summaries
        tot = n = 0
        for k in kernel:
            if k in f and k in w:
                d = f[k]['FETCH_SIZE']['dispatches']
                tot += d * (2 * f[k]['FETCH_SIZE']['mean'] + w[k]['WRITE_SIZE']['mean']) * 1024
                n += d
        return (tot / n if n else None), src
    except Exception:
        return None, None


_LIB_HASH = []


def _pmc_build_state(summary):
    """'current' when the counter summary was collected on the libsdn_hip.so that is loaded now (sha256 recorded by
    tools/pmc_summary.py), else what is known: counter files go stale the moment a kernel changes."""
    import hashlib
    import sdn_hip
    if not _LIB_HASH:
        try:
            _LIB_HASH.append(hashlib.sha256(open(sdn_hip.LIB_PATH, 'rb').read()).hexdigest())
        except OSError:
            _LIB_HASH.append(None)
    rec = summary.get('_lib_sha256')
    if rec is None:
        return 'collected before builds were recorded (run %s): the kernels have changed since' % summary.get('_tag', '?')
    return 'current' if rec == _LIB_HASH[0] else 'collected on another build of libsdn_hip.so'


def real_meshes_leg(args, device, rank):
    """The headline's frame step (same poses, same loss, same 16 objects per frame) on the six ShapeNet CAD templates the
    reference ships (geometric/assets/*: 31.5-72.5 k triangles; tests/golden/cad_templates.npz).  `mixed`: a frame whose 16
    objects draw from all six (the analogue of `value`: objects_per_s is reported as `value_real_meshes`); `per_mesh`: 16
    poses of ONE template per frame -- the worst and the mean over the six say how far the synthetic family is from each."""
    import sdn_hip
    if not os.path.exists(REAL_TEMPLATES):
        return {'error': 'tests/golden/cad_templates.npz missing'}

    def run(mesh, steps):
        bank, sizes, cls, params, targets, ptf = build_scene(device, seed=1234 + rank, mesh=mesh)
        step = make_step(device, bank, cls, params, targets, ptf, backward=not args.forward_only, pack=False)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        for slot in (sdn_hip.SLOT_RASTER_TILES, sdn_hip.SLOT_EDGE_SCAN):
            sdn_hip.timing_read_slot(slot)
        best = float('inf')
        for _ in range(2):     # the faster of two passes (allocator first-touch stalls, see the car_like leg)
            t1 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t1) / steps * 1e3)
        f_ms, f_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_RASTER_TILES)
        b_ms, b_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_EDGE_SCAN)
        return {'objects_per_s': OBJECTS_PER_FRAME / (best * 1e-3), 'ms_per_step': best,
                'k_raster_tiles_us': f_ms / max(f_n, 1) * 1e3, 'edge_kernels_us': b_ms / max(b_n, 1) * 1e3,
                'triangles_mean': float(np.mean([sizes[c][1] for c in cls]))}
    steps = max(3, min(10, args.steps))
    out = run('real', steps)
    out['steps'] = steps
    names = [str(m) for m in np.load(REAL_TEMPLATES)['meshes']]
    per = {}
    for j, name in enumerate(names):
        per[name.split('/')[1][:8]] = run('real:%d' % j, steps)
    out['per_mesh'] = per
    rates = [v['objects_per_s'] for v in per.values()]
    out['per_mesh_worst_objects_per_s'] = min(rates)
    out['per_mesh_mean_objects_per_s'] = float(np.mean(rates))
    out['mesh'] = ('the six ShapeNet OBJs of /root/reference/geometric/assets as Derenderer3d holds them (fixture '
                   'tests/golden/cad_templates.npz); same poses / loss / frame size as `value`')
    return out


DUMP_BUDGET_BYTES = 60 * 10 ** 6


def dump_outputs(out_dir, arrays, seed=0):
    """--dump-outputs: every tensor of `arrays` as out_dir/<name>.npy in float32, so that two builds can be compared output
    for output.  When they hold more than DUMP_BUDGET_BYTES in all (the gathered maps of many ranks), each is replaced by a
    fixed, seeded sample of its flattened elements (sorted positions, the same for the same shape) of a proportional size."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.size for a in arrays.values()) * 4
    keep = min(1.0, DUMP_BUDGET_BYTES / max(total, 1))
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if keep < 1.0:
            idx = np.sort(np.random.default_rng(seed).integers(0, a.size, int(a.size * keep)))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + '.npy'), a)


def geometric_leg(args, device, world, rank):
    import sdn_hip
    bank, sizes, cls, params, targets, ptf = build_scene(device, seed=1234 + rank, mesh=HEADLINE_MESH)
    payload = os.environ.get('SDN_EXCHANGE_PAYLOAD', 'objects')   # 'objects': [16,5,384,384] per rank; 'frame': [1,5,375,1242]
    if payload not in ('objects', 'frame'):
        raise SystemExit('bench.py: SDN_EXCHANGE_PAYLOAD must be objects or frame')
    step = make_step(device, bank, cls, params, targets, ptf, backward=not args.forward_only,
                     pack=('frame' if payload == 'frame' else True) if world > 1 else False)
    from sdn_hip import dist as sdist
    # the path's only exchange: every rank ends up with all world * 16 objects' maps.  Overlapped (sdist.MapExchange): the
    # all_gather of step k runs on RCCL's stream while step k + 1 renders; a step waits for the PREVIOUS step's exchange, and
    # the last one is waited for inside the timed region -- K steps, K completed exchanges.
    if world == 1:
        ex = None
    elif payload == 'frame':
        ex = sdist.MapExchange(world, (5, 375, 1242), torch.float32, device)
    else:
        ex = sdist.MapExchange(world * OBJECTS_PER_FRAME, (5, RENDER_SIZE, RENDER_SIZE), torch.float32, device)
    pending = [None]

    def full_step():
        maps = step()
        if ex is None:
            return maps
        h = ex.post(maps.detach())
        out = ex.wait(pending[0]) if pending[0] is not None else None
        pending[0] = h
        return out

    def drain():
        if ex is not None and pending[0] is not None:
            out = ex.wait(pending[0])
            pending[0] = None
            return out

    extras = args.full and not args.no_extras and world == 1
    for _ in range(args.warmup):
        full_step()
    drain()
    issue_ms = None
    if args.full:
        issue_ms = host_issue_ms(full_step)
        drain()
    if world > 1:
        dist.barrier()
    sdn_hip.timing_enable(True)
    for slot in (sdn_hip.SLOT_RASTER_TILES, sdn_hip.SLOT_EDGE_SCAN):
        sdn_hip.timing_read_slot(slot)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps - 1):
        full_step()
    last = full_step()
    if ex is not None:
        last = drain()   # a step returns the PREVIOUS step's exchange: the last step's gathered maps
    enqueue = time.perf_counter() - t0   # host time to issue the steps (the GPU runs behind it)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    fwd_ms, fwd_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_RASTER_TILES)
    bwd_ms, bwd_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_EDGE_SCAN)
    if args.dump_outputs and rank == 0:
        # outside the timed region, before anything below runs the step again (the gradients are those of the last step)
        if ex is None:
            out = {'mask': last[0], 'normal': last[1], 'depth': last[2]}
        else:
            out = {'maps_' + payload: last}
        out.update(('grad_' + k, p.grad) for k, p in params.items() if p.grad is not None)
        dump_outputs(args.dump_outputs, out)
    del last
    # ---- N > 1: what ONE exchange costs when nothing overlaps it (outside the timed region): says whether the step or the
    # exchange bounds the headline, and whether RCCL ran the all_gather direct or through a ring (DESIGN section 4's budget)
    exchange = None
    if ex is not None and args.full:
        sdn_hip.timing_enable(False)
        maps = step().detach()
        torch.cuda.synchronize()
        dist.barrier()
        ex.wait(ex.post(maps))
        torch.cuda.synchronize()
        dist.barrier()
        t1 = time.perf_counter()
        for _ in range(10):
            ex.wait(ex.post(maps))
        torch.cuda.synchronize()
        dist.barrier()
        ems = (time.perf_counter() - t1) / 10 * 1e3
        recv_bytes = (world - 1) * maps.numel() * 4
        exchange = {'algo': ex.mode, 'payload': payload, 'payload_shape_per_rank': list(maps.shape),
                    'bytes_sent_per_rank_per_step': ex.bytes_sent_per_post, 'bytes_received_per_rank_per_step': recv_bytes,
                    'blocking_ms_per_exchange': ems, 'received_GBps_per_rank': recv_bytes / (ems * 1e-3) / 1e9,
                    'note': 'SDN_EXCHANGE=p2p selects W-1 direct isend/irecv pairs per rank instead of the collective, '
                            'SDN_EXCHANGE_PAYLOAD=frame the composited [1,5,375,1242] frame map; in the timed region the '
                            'exchange of step k overlaps the render of step k + 1 (MapExchange, double-buffered)'}
        sdn_hip.timing_enable(True)
    # ---- the same frame step on the OTHER template family (outside the headline's timed region): since r04 the headline runs on
    # the templates with the reference's CAD statistics, the smoother car_like family is the secondary number
    cad = None
    if extras:
        try:
            cbank, csizes, ccls, cparams, ctargets, cptf = build_scene(device, seed=4321 + rank, mesh=SECONDARY_MESH)
            cstep = make_step(device, cbank, ccls, cparams, ctargets, cptf, backward=not args.forward_only, pack=False)
            for _ in range(2):
                cstep()
            torch.cuda.synchronize()
            for slot in (sdn_hip.SLOT_RASTER_TILES, sdn_hip.SLOT_EDGE_SCAN):
                sdn_hip.timing_read_slot(slot)
            csteps = max(3, min(10, args.steps))
            cpass = []
            for _ in range(2):   # two passes, the faster one reported: one pass of r05u carried a 74 ms stall (a first-touch of
                t1 = time.perf_counter()   # fresh allocator blocks right after the scene was built), 8.3 instead of 0.83 ms per step
                for _ in range(csteps):
                    cstep()
                torch.cuda.synchronize()
                cpass.append((time.perf_counter() - t1) / csteps * 1e3)
            cms = min(cpass)
            cf_ms, cf_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_RASTER_TILES)
            cb_ms, cb_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_EDGE_SCAN)
            cad = {'objects_per_s': OBJECTS_PER_FRAME / (cms * 1e-3), 'ms_per_step': cms, 'steps': csteps, 'ms_per_step_of_each_pass': cpass,
                   'k_raster_tiles_us': cf_ms / max(cf_n, 1) * 1e3, 'edge_kernels_us': cb_ms / max(cb_n, 1) * 1e3,
                   'triangles_mean': float(np.mean([csizes[c][1] for c in ccls])),
                   'mesh': MESH_NOTES[SECONDARY_MESH]}
            del cbank, cparams, ctargets, cstep
        except Exception as e:   # the secondary number must not take the headline down
            cad = {'error': repr(e)}
    # ---- the SAME headline frame step under the reference's DEFAULT coverage rule K1 (scripts/env.sh:11 exports
    # NEURAL_RENDERER_UNSAFE=1 -> rasterize.py:102-236): what a reference user's environment selects
    k1 = None
    if extras:
        try:
            import neural_renderer as nr
            nr.use_unsafe_rasterizer(True)
            try:
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                sdn_hip.timing_read_slot(sdn_hip.SLOT_RASTER_TILES_K1)
                ksteps = max(3, min(20, args.steps))
                t1 = time.perf_counter()
                for _ in range(ksteps):
                    step()
                torch.cuda.synchronize()
                kms = (time.perf_counter() - t1) / ksteps * 1e3
                k_ms, k_n, _ = sdn_hip.timing_read_slot(sdn_hip.SLOT_RASTER_TILES_K1)
            finally:
                nr.use_unsafe_rasterizer(False)
            k1 = {'objects_per_s': OBJECTS_PER_FRAME / (kms * 1e-3), 'ms_per_step': kms, 'steps': ksteps,
                  'k_raster_tiles_k1_us': k_ms / max(k_n, 1) * 1e3,
                  'note': 'neural_renderer.use_unsafe_rasterizer(True): K1\'s scanline coverage rule and sorted-vertex '
                          'barycentrics, ties to the lowest face index; same mesh, same step, outside the timed region'}
        except Exception as e:
            k1 = {'error': repr(e)}
    # ---- the same frame step on the reference's OWN six ShapeNet templates: the synthetic family is fitted to
    # their statistics, these are the meshes themselves
    real = None
    if extras:
        try:
            real = real_meshes_leg(args, device, rank)
        except Exception as e:
            real = {'error': repr(e)}
    sdn_hip.timing_enable(False)
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    objects = world * OBJECTS_PER_FRAME * args.steps
    vmean = float(np.mean([sizes[c][0] for c in cls]))
    fmean = float(np.mean([sizes[c][1] for c in cls]))
    S, R = 2 * RENDER_SIZE, RENDER_SIZE
    per_launch = OBJECTS_PER_FRAME  # the whole frame is ONE launch of each kernel (bs = 16)
    fwd_bytes = per_launch * (12 * vmean + 12 * fmean + 20 * S * S + 20 * R * R)
    bwd_bytes_5ch = per_launch * (20 * R * R + 20 * S * S + 12 * vmean)   # all five channels differentiated
    # what the timed step differentiates is the SILHOUETTE only (scripts/main.py:445-451): g_alpha [R, R] read, the S x S
    # face-index map read, grad_faces [2F, 3, 3] written, grad_verts written
    bwd_bytes = per_launch * (4 * R * R + 4 * S * S + 36 * 2 * fmean + 12 * vmean)

    def roof(kernel, pmc_name, nbytes, ms, n, note):
        sec = ms / 1e3 / max(n, 1)
        ach = nbytes / sec / 1e9 if n else 0.0
        traffic, source = _pmc_traffic(pmc_name)
        r = {'bound': 'hbm', 'kernel': kernel, 'achieved': ach, 'peak': 8000.0, 'unit': 'GB/s', 'frac': ach / 8000.0,
             'traffic': traffic, 'traffic_source': source, 'algorithmic_bytes_per_launch': nbytes, 'launches': n,
             'avg_launch_us': sec * 1e6, 'objects_per_launch': per_launch, 'note': note}
        r['traffic_stale'] = bool(source and 'STALE' in source)
        if traffic and sec > 0:
            r['traffic_frac_of_peak'] = traffic / sec / 8e12
        return r
    line = {
        'metric': 'rendered-objects/sec (FFD decode + transform + silhouette/normal/depth @384, fwd+bwd)'
        if not args.forward_only else 'rendered-objects/sec (forward only)',
        'value': objects / elapsed,
        'unit': 'objects/s',
        'n_gpus': world,
        'steps': args.steps,
        'warmup': args.warmup,
        'ms_per_step': elapsed / args.steps * 1e3,
        'host_enqueue_ms_per_step': enqueue / args.steps * 1e3,
        'host_issue_ms_one_step': issue_ms,
        'value_' + SECONDARY_MESH: (cad or {}).get('objects_per_s'),
        SECONDARY_MESH: cad,
        'value_k1': (k1 or {}).get('objects_per_s'),
        'k1': k1,
        'value_real_meshes': (real or {}).get('objects_per_s'),
        'real_meshes': real,
        'headline_mesh': HEADLINE_MESH + ': ' + MESH_NOTES[HEADLINE_MESH],
        'higher_is_better': True,
        'scaling': 'weak',
        'vs_baseline': None,
        'dtype': 'f32',
        'data': 'synthetic',
        'allgather_payload_bytes_per_rank': ex.bytes_sent_per_post if world > 1 else 0,
        'exchange': exchange,
        'config': {'workload': 'configs[1]: car-class CAD-statistics mesh (%.0f tris, %.0f faces with fill_back) render fwd+bwd, '
                               '16 objects of a 375x1242 VKITTI frame per step per GPU, render_size 384 (768^2 '
                               'internal)' % (fmean, 2 * fmean),
                   'objects_per_step_per_gpu': OBJECTS_PER_FRAME, 'render_size': RENDER_SIZE,
                   'parallelism': 'objects sharded over %d rank(s)%s' % (
                       world, ', one RCCL exchange (%s) of %s maps per step, overlapped with the next step'
                       % (ex.mode, '[1,5,375,1242] composited frame' if payload == 'frame' else '[16,5,384,384] object')
                       if world > 1 else '')},
        'roofline_raster_fwd': roof('k_raster_tiles', 'sdn::k_raster_tiles', fwd_bytes, fwd_ms, fwd_n,
                                    'one launch = the 16 objects of a frame; vector-instruction-issue bound, see roofline_alu'),
    }
    # ALU view of the forward rasterizer: the counting build of the kernel tallies the pixel tests of one
    # more step, outside the timed region; flops per test are counted from csrc/raster_math.h (inside_ndc: 3 edges x
    # (4 sub + 2 mul + 1 compare) = 21; a covered pixel adds barycentric weights 23 + perspective depth 6 = 29)
    if args.full:
        try:
            from sdn_hip import ops
            fwd_step = make_step(device, bank, cls, params, targets, ptf, backward=False)
            with ops.verification(count_work=True):
                with torch.no_grad():
                    fwd_step()
            cand, passed, keys = ops.last_work()
            flops = 21.0 * cand + 29.0 * passed
            sec = fwd_ms / 1e3 / max(fwd_n, 1)
            line['roofline_alu'] = {'bound': 'valu fp32', 'kernel': 'k_raster_tiles', 'candidate_pixel_tests': cand,
                                    'tests_passed': passed, 'depth_keys': keys, 'flops_per_launch': flops,
                                    'achieved': flops / sec / 1e12 if fwd_n else 0.0, 'peak': 157.3, 'unit': 'TFLOP/s',
                                    'frac': flops / sec / 1e12 / 157.3 if fwd_n else 0.0,
                                    'pixel_tests_per_s': cand / sec if fwd_n else 0.0,
                                    'note': 'counted flops are a few per cent of the fp32 vector peak, yet the kernel ISSUES vector-ALU '
                                            'instructions ~84 %% of its cycles at 66 %% lane utilisation (SQ counters of the r05 tree, '
                                            'profiles/r05v_pmcgeo_sq1.json / _sq2.json: 148.0 M vector wave-instructions per launch = 119 per '
                                            '64-candidate pass all in; the wave-shared box loop itself is ~35 in the ISA: index arithmetic, table '
                                            'reads, three edge tests, depth cull, hit-queue bookkeeping) '
                                            'for 21 counted flops per test; ~%.0f candidate tests per covered pixel' % (
                                                cand / max(1.0, per_launch * 0.4 * S * S))}
        except Exception as e:
            line['roofline_alu'] = {'error': repr(e)}
    bwd = roof('k_edge_scan_sil + k_edge_rows + k_chunk_sum (one event pair)', ['sum', 'sdn::k_edge_scan_sil', 'sdn::k_edge_rows', 'sdn::k_chunk_sum'],
               bwd_bytes, bwd_ms, bwd_n,
               'silhouette edge gradient (K5): owners filed per row by the scan kernel, rows evaluated from LDS; algorithmic '
               'bytes are the SILHOUETTE-only backward (4 R^2 + 4 S^2 + 36 F + 12 V per object), not SURVEY 8(d)\'s '
               'five-channel figure, which this step does not differentiate')
    bwd['five_channel_bytes_per_launch'] = bwd_bytes_5ch
    line['roofline_edge_bwd'] = bwd
    line['roofline'] = bwd if (bwd_n and bwd_ms >= fwd_ms) else line['roofline_raster_fwd']
    return line


if __name__ == '__main__':
    main()
