"""The Derenderer's heads on the device: opt-in switch and the call both forwards make when it is on.

`use_device_heads(model)` takes a `Derenderer3d` or a `Derenderer` and makes its forward run `net.fc`, the ReLUs, the cat with the
roi vectors, `fc1`, `fc2`, `_fc3`, the slices, the pose pair's normalisation and the class softmax -- and, for a `Derenderer3d`, the
roi centre / extent arithmetic in front of them -- as `sdn_hip.ops.derender_heads`: four launches each way in place of about twenty
forward and twice that backward (reference: geometric/derender3d/models/derenderer.py:34-56, models/__init__.py:70-77).  It returns a
handle: `handle.remove()` switches back, and the handle is a context manager.

The switch is a plain instance attribute, `_device_heads`, that `Derenderer.forward` and `Derenderer3d.forward` test; off (the class
default) both run exactly their own statements.  It is a flag and not an instance-level bound `forward` because `nn.DataParallel`
copies `__dict__` to its replicas: a flag travels and every replica reads its own parameters, a bound method would keep pointing at
the original's.  A switched `Derenderer3d.forward` calls `device_blob` itself, with `roi_norms`, instead of calling its
`derenderer` module: a forward hook registered on that submodule does not fire while the switch is on.  Parameters, module names, `state_dict` and blob keys are untouched; the layers are read in place, so an optimizer
step needs nothing refreshed.  fp32 tensors on the GPU only: `ops.derender_heads` raises for anything else."""
import torch.nn as nn

FLAG = '_device_heads'


def device_blob(derenderer, images, rois):
    """the blob of `Derenderer.forward`; rois: roi_norms [n, 4] (then `_mroi_norms` and `_droi_norms` come with it) or the pair
    (mroi_norms, droi_norms)"""
    from sdn_hip import ops
    net = derenderer.net
    rois = rois.contiguous() if not isinstance(rois, (tuple, list)) else tuple(r.contiguous() for r in rois)
    return ops.derender_heads(net.pooled(images), rois, net.fc, derenderer.fc1, derenderer.fc2, derenderer._fc3, derenderer.num_classes)


class DeviceHeadsHandle(object):
    def __init__(self, modules):
        self._modules = list(modules)

    def remove(self):
        for m in self._modules:
            m.__dict__.pop(FLAG, None)
        self._modules = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.remove()
        return False


def use_device_heads(model):
    from derender3d.models.derenderer import Derenderer
    if not isinstance(model, nn.Module):
        raise TypeError('model must be a Derenderer3d or a Derenderer, got %r' % type(model))
    modules = [model, model.derenderer] if isinstance(getattr(model, 'derenderer', None), Derenderer) else [model]
    derenderer = modules[-1]
    if not isinstance(derenderer, Derenderer):
        raise TypeError('model must be a Derenderer3d or a Derenderer, got %r' % type(model))
    if not callable(getattr(derenderer.net, 'pooled', None)):
        raise ValueError('derenderer.net has no pooled(): the device heads start from the pooled features (models/resnet.py)')
    for m in modules:
        setattr(m, FLAG, True)
    return DeviceHeadsHandle(modules)
