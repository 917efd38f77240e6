"""Derenderer3d: encoder -> pose algebra -> per-object FFD decode, perspective transform and render.

Reference: /root/reference/geometric/derender3d/models/__init__.py:18-250 (same constructor, same `forward` /
`render` signatures, same blob keys).  What changes on MI355X:
  * all constants are created on the blob's device (the reference hard-codes `.cuda()`, :110-123,169);
  * each object is rasterized ONCE for silhouette + normal + depth (`Renderer.render_maps`) instead of three
    times (:203-224), with no host round trip (reference: derender3d/models/renderer.py:131-150);
  * mesh templates may be passed in (`objs=`) because two of the eight ShapeNet models the reference hard-codes
    are not shipped with it; the default still reads SHAPENET_ROOT_DIR like the reference.
"""
import weakref
import numpy as np
import os
import torch

from torch.distributions import Categorical
from torch.nn.modules import Module

import neural_renderer as nr

from derender3d import TargetType
from derender3d.models import heads
from derender3d.models.derenderer import Derenderer
from derender3d.models.renderer import RenderType, Renderer
from derender3d.models.transforms import FFD, FFDBank, PerspectiveTransform


class ShapenetObj(object):
    root_dir = os.getenv('SHAPENET_ROOT_DIR')

    def __init__(self,
                 class_id=None,
                 obj_id=None,
                 root_dir=None,
                 vertices=None,
                 faces=None):
        if vertices is None:
            root_dir = root_dir if root_dir is not None else ShapenetObj.root_dir
            path = os.path.join(root_dir, class_id, obj_id, 'models', 'model_normalized.obj')
            print('Reading {:s}'.format(path))
            (vertices, faces) = nr.load_obj(path)
            # unit extent per axis, then the (z, y, -x) axis convention of the reference (:29-31)
            vertices = vertices / np.ptp(vertices, axis=0)
            vertices = vertices[:, [2, 1, 0]] * np.asarray([-1, 1, 1], dtype=np.float32)
        self.vertices = torch.as_tensor(np.asarray(vertices), dtype=torch.float32)
        self.faces = torch.as_tensor(np.asarray(faces), dtype=torch.int32)


DEFAULT_OBJS = [
    ('02958343', '137f67657cdc9da5f985cd98f7d73e9a'),
    ('02958343', '5343e944a7753108aa69dfdc5532bb13'),
    ('02958343', '3776e4d1e2587fd3253c03b7df20edd5'),
    ('02958343', '3ba5bce1b29f0be725f689444c7effe2'),
    ('02958343', '53a031dd120e81dc3aa562f24645e326'),
    ('02924116', '7905d83af08a0ca6dafc1d33c05cbcf8'),
    ('02958343', 'a0fe4aac120d5f8a5145cad7315443b3'),
    ('02958343', 'cd7feedd6041209131ac5fb37e6c8324'),
]


def _unit_rows(m):
    return m / torch.norm(m, p=2, dim=1, keepdim=True)


def _camera_ray(centre2d):
    """Unit direction of the pixel at normalised image position (row, column) = centre2d [n, 2]: the camera looks down
    -z with +y up, so the ray is (column, -row, -1) normalised (reference: models/__init__.py:119-126, 139-146)."""
    minus_one = -torch.ones(centre2d.shape[0], device=centre2d.device)
    return _unit_rows(torch.stack((centre2d[:, 1], -centre2d[:, 0], minus_one), dim=1))


def _yaw_quaternion(theta):
    """Quaternion (cos t/2, 0, sin t/2, 0) of a rotation by theta [n, 1] about +y (:107-113)."""
    zero = torch.zeros_like(theta)
    return torch.cat((torch.cos(theta / 2), zero, torch.sin(theta / 2), zero), dim=1)


class Derenderer3d(Module):
    """Encoder + decoder of the geometric branch.  `forward(images, roi_norms, focals)` returns the blob of encoder
    outputs, pose quantities and (in reproject mode) the rendered silhouette / normal / depth maps; `render(blob)`
    re-renders from a (possibly edited or optimised) blob -- the call sites of geometric/scripts/main.py:443,516."""

    _device_heads = False   # heads.use_device_heads sets it on the instance

    def __init__(self, mode, image_size, render_size, objs=None):
        super(Derenderer3d, self).__init__()
        self.mode, self.image_size, self.render_size = mode, image_size, render_size
        self.derenderer = Derenderer()
        self._force_no_sample = False
        if not (mode & TargetType.reproject):
            return
        self.objs = objs if objs is not None else [ShapenetObj(class_id=c, obj_id=o) for (c, o) in DEFAULT_OBJS]
        lattice_constraints = (FFD.Constraint.symmetry(axis=FFD.Constraint.Axis.z),
                               FFD.Constraint.homogeneity(axis=FFD.Constraint.Axis.y, index=[0, 1]))
        self.ffds = torch.nn.ModuleList([FFD(obj.vertices, constraints=list(lattice_constraints)) for obj in self.objs])
        self.perspective_transform = PerspectiveTransform()
        self.renderer = Renderer(image_size=render_size)
        self._faces_on = {}
        self._banks = {}
        # True: decode + render all objects of a call in one batch of launches (same results as the per-object loop of
        # the reference, derender3d/models/__init__.py:161-224)
        self.batched = True

    # ------------------------------------------------------------------------------------------------ device state
    def bank(self, device=None):
        """The FFDBank resident on `device` (default: where the encoder lives).  One bank PER DEVICE, created once and
        never moved: nn.DataParallel replicas (scripts/main.py:182) share this dict and each finds its own device's copy,
        so no thread ever relocates buffers another thread's kernels are reading."""
        if device is None:
            device = next(self.derenderer.parameters()).device
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        hit = self._banks.get(device)
        if hit is None:
            hit = FFDBank(list(self.ffds), [obj.faces for obj in self.objs]).to(device)
            self._banks[device] = hit
        return hit

    def _faces(self, index, device):
        key = (index, device)
        if key not in self._faces_on:
            self._faces_on[key] = self.objs[index].faces.to(device).unsqueeze(dim=0).contiguous()
        return self._faces_on[key]

    # ------------------------------------------------------------------------------------------------ encoder
    def forward(self, images, roi_norms, focals):
        if self._device_heads:   # heads.use_device_heads: the roi arithmetic below and the derenderer's heads in the same launches
            got = heads.device_blob(self.derenderer, images, roi_norms)
            blob = {'_roi_norms': roi_norms, '_mroi_norms': got.pop('_mroi_norms'), '_droi_norms': got.pop('_droi_norms'),
                    '_focals': focals}
            blob.update(got)
            if self.mode & TargetType.reproject:
                blob.update(self.render(blob))
            return blob
        top_left, bottom_right = roi_norms[:, 0:2], roi_norms[:, 2:4]
        blob = {
            '_roi_norms': roi_norms,
            '_mroi_norms': (bottom_right + top_left) / 2.0,   # roi centre (row, column)
            '_droi_norms': bottom_right - top_left,           # roi extent
            '_focals': focals,
        }
        blob.update(self.derenderer(images, blob['_mroi_norms'], blob['_droi_norms']))
        if self.mode & TargetType.reproject:
            blob.update(self.render(blob))
        return blob

    # ------------------------------------------------------------------------------------------------ pose algebra
    def _pose(self, blob):
        """Everything render() derives from the encoder outputs before a mesh is touched (:95-158)."""
        centre, extent, focals = blob['_mroi_norms'], blob['_droi_norms'], blob['_focals']
        delta = blob['_theta_deltas']
        P = {}
        if delta.is_cuda and delta.dtype == torch.float32:
            # r04: the whole block below in one launch each way (sdn_pose_algebra, csrc/transform.hip; same formulas)
            from sdn_hip import ops
            (P['_thetas'], P['_alphas'], P['_rotations'], P['_scales'], P['_depths'], P['_center2ds'], P['_translations'],
             P['persp'], zoom) = ops.PoseAlgebraFn.apply(centre, extent, focals, delta, blob['_log_scales'], blob['_log_depths'],
                                                         blob['_translation2ds'], self.training, self.image_size,
                                                         self.render_size)
            P['_zooms' if self.training else 'zoom_tos'] = zoom
            self._classes(blob, P)
            return P
        P['_thetas'] = torch.atan2(delta[:, 1], delta[:, 0]).unsqueeze(dim=1)
        if P['_thetas'].is_cuda:
            # (cos t/2, 0, sin t/2, 0) and exp(log_scales) in one launch each way (sdn_pose_params, csrc/transform.hip)
            from sdn_hip import ops
            P['_rotations'], P['_scales'] = ops.PoseParamsFn.apply(P['_thetas'], blob['_log_scales'])
        else:   # host tensors: the reference's own element-wise arithmetic (tests of the pose algebra)
            P['_rotations'] = _yaw_quaternion(P['_thetas'])
            P['_scales'] = torch.exp(blob['_log_scales'])
        area = (extent[:, 0] * extent[:, 1]).unsqueeze(dim=1)
        P['_depths'] = torch.sqrt(torch.exp(blob['_log_depths']) / area)
        P['_center2ds'] = centre + blob['_translation2ds'] * extent
        P['_translations'] = P['_depths'] * _camera_ray(P['_center2ds'])
        t = P['_translations']
        # observation angle: yaw minus the bearing of the object centre, wrapped to [-pi, pi) (:128-129)
        alpha = -(P['_thetas'] - torch.atan(t[:, 0:1] / t[:, 2:3]))
        P['_alphas'] = torch.remainder(alpha + np.pi, 2 * np.pi) - np.pi
        self._classes(blob, P)
        if self.training:   # crop-centred camera with a fixed zoom (:139-150)
            P['persp'] = P['_depths'] * _camera_ray(centre)
            P['_zooms'] = (self.image_size / focals) / torch.max(extent, dim=1, keepdim=True)[0]
        else:               # object-centred camera, zoom-to-fit (:152-153)
            P['persp'] = P['_translations']
            P['zoom_tos'] = self.render_size / (2.0 * focals)
        return P

    def _classes(self, blob, P):
        probs = blob['_class_probs']
        if self.training and not self._force_no_sample:
            dist = Categorical(probs)                      # REINFORCE over the mesh class (:131-134)
            P['classes'] = dist.sample()
            P['_class_log_probs'] = dist.log_prob(P['classes'])
        else:
            # r05: the optimisation loop of scripts/main.py:433-456 hands in the SAME detached probabilities every iteration:
            # arg-max, log and the flat row index of the chosen class are kept for as long as the very same, unmodified
            # tensor arrives (identity + version counter + storage address + shape, like _viewing_angles; nothing is kept
            # when the probabilities carry a graph).  Four launches per iteration here, and -- because the bank's own cache
            # is keyed on the `classes` tensor -- the 8 MB face gather of FFDBank._class_rows with them.
            hit = self.__dict__.get('_argmax_hit')
            key = (probs._version, probs.data_ptr(), tuple(probs.shape))
            if hit is not None and hit[0]() is probs and hit[1] == key:
                P['classes'], P['_class_log_probs'], P['class_rows'] = hit[2]
                return
            best, P['classes'] = torch.max(probs, dim=1)
            P['_class_log_probs'] = torch.log(best)
            P['class_rows'] = torch.arange(probs.shape[0], device=probs.device) * probs.shape[1] + P['classes']
            if not probs.requires_grad:
                self.__dict__['_argmax_hit'] = (weakref.ref(probs), key, (P['classes'], P['_class_log_probs'], P['class_rows']))

    def _viewing_angles(self, focals):
        # np.arctan(render_size / (2 f)) / pi * 180 per object, in float64 like the reference (:202); one host read -- which
        # is a device synchronisation, so the answer is kept for as long as the SAME tensor object is handed in unmodified
        # (the optimisation loop of scripts/main.py:433-456 renders the same blob['_focals'] every iteration)
        # The key is (object, version counter, storage address, shape): in-place ops bump the version, `set_()` / a resized
        # storage change the address or the shape.  Writes THROUGH `focals.data` bump nothing (torch hides them from autograd
        # on purpose) -- a caller that edits focals that way must hand in a new tensor (or call invalidate_viewing_angles()).
        hit = self.__dict__.get('_angles_hit')
        key = (focals._version, focals.data_ptr(), tuple(focals.shape))
        if hit is not None and hit[0]() is focals and hit[1] == key:
            return hit[2]
        angles = [np.arctan(self.render_size / (2.0 * f)) / np.pi * 180 for f in focals.reshape(len(focals), -1)[:, 0].tolist()]
        self.__dict__['_angles_hit'] = (weakref.ref(focals), key, angles)
        return angles

    def invalidate_viewing_angles(self):
        """forget the cached per-object viewing angles (after writing through `blob['_focals'].data`)"""
        self.__dict__.pop('_angles_hit', None)

    def invalidate_class_cache(self):
        """forget the cached arg-max of `blob['_class_probs']` and the bank's class gather (after writing through `.data`)"""
        self.__dict__.pop('_argmax_hit', None)
        for bank in getattr(self, '_banks', {}).values():
            bank.invalidate_class_cache()

    # ------------------------------------------------------------------------------------------------ decoder
    def render(self, blob):
        P = self._pose(blob)
        want_normal = bool(self.mode & TargetType.normal)
        want_depth = bool(self.mode & TargetType.depth)
        angles = self._viewing_angles(blob['_focals'])
        coeffs = blob['_ffd_coeffs']
        n = coeffs.shape[0]
        if self.batched and type(self.renderer) is Renderer:
            # one FFD decode launch, one batched PerspectiveTransform, one rasterization launch set
            # coeffs[arange(n), classes] as ONE row gather on the flattened [n * classes] rows: advanced indexing costs an
            # arange + index forward and an eight-launch index_put backward (r05z_torch_ops_opt.txt); index_select's backward
            # is zeros + index_add_ (rows are unique: deterministic)
            rows = P.get('class_rows')
            if rows is None:
                rows = torch.arange(n, device=coeffs.device) * coeffs.shape[1] + P['classes']
            picked = coeffs.reshape(n * coeffs.shape[1], -1).index_select(0, rows)
            vertices, faces = self.bank(coeffs.device).decode(picked, P['classes'])
            vertices, zooms = self._place(vertices, P, slice(None))
            self.renderer.viewing_angle = angles
            masks, normals, depth_maps = self.renderer.render_maps(vertices, faces, normal=want_normal, depth=want_depth)
        else:
            # the reference's loop (:161-224): one object at a time through FFD.forward and the renderer
            rendered, zoom_rows = [], []
            for i, cls in enumerate(P['classes'].tolist()):
                vertices = self.ffds[cls](coeffs[i][cls]).unsqueeze(dim=0)
                vertices, z = self._place(vertices, P, slice(i, i + 1))
                zoom_rows.append(z)
                self.renderer.viewing_angle = angles[i]
                rendered.append(self.renderer.render_maps(vertices, self._faces(cls, coeffs.device), normal=want_normal,
                                                          depth=want_depth))
            zooms = torch.cat(zoom_rows, dim=0)
            masks = torch.cat([r[0] for r in rendered], dim=0)
            normals = torch.cat([r[1] for r in rendered], dim=0) if want_normal else []
            depth_maps = torch.cat([r[2] for r in rendered], dim=0) if want_depth else []
        out = {k: P[k] for k in ('_thetas', '_alphas', '_rotations', '_scales', '_depths', '_center2ds', '_translations',
                                 '_class_log_probs')}
        out['_zooms'] = zooms
        out['_masks'] = masks
        out['_normals'] = normals if want_normal else []
        out['_depth_maps'] = depth_maps if want_depth else []
        return out

    def _place(self, vertices, P, rows):
        """PerspectiveTransform of the objects `rows`; returns (vertices, zooms)."""
        take = (lambda t: t) if rows == slice(None) else (lambda t: t[rows])   # (the batched path passes every row)
        common = dict(scales=take(P['_scales']), rotations=take(P['_rotations']), translations=take(P['_translations']),
                      perspective_translations=take(P['persp']))
        if self.training:
            z = take(P['_zooms'])
            return self.perspective_transform(vertices, zooms=z, **common), z
        return self.perspective_transform(vertices, zoom_tos=take(P['zoom_tos']), **common)
