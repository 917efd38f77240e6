"""The input side of the textural networks on the device (reference: textural/models/pix2pixHD_model.py:124-166 with get_edges
:343-349, and the instance numbering of Encoder.forward, networks.py:310-325).

    input_label, pose_onehot, bad = encode_maps(label, inst, pose, opt.label_nc, opt.feat_pose_num_bins + 1)
    ids, seg, counts, info = instance_index(inst, with_counts=True)

The reference builds the label planes, the edge plane and the pose planes with zeros + long + scatter_ twice, about ten slice /
compare / or launches and a cat, and numbers the instances by sorting every pixel.  Here the planes are one launch that writes
every element once (csrc/encode_input.hip: k_encode_maps), and the numbering is a presence bitmap over a fixed key window, a
prefix count and a rank look-up: three launches and the one 8-byte copy to the host that sizes the result.  Pix2PixHDModel and
Encoder go through these for CUDA maps of a supported dtype; SDN_ENCODE_DEVICE=0 restores the torch expressions.

Two deviations, where the reference has no answer or a costly one: an index outside [0, channels) or a NaN sets no plane and is
counted in `bad` (the reference's scatter_ trips a device-side assert); a key outside [-32768, 2^21 - 32768) makes
instance_index fall back to torch.unique and say so in info['path'].
"""
import os

import torch

from sdn_hip import ops


def device_path_enabled():
    """False with SDN_ENCODE_DEVICE=0 in the environment: encode_input and the encoder's pooling run the torch expressions."""
    return os.environ.get('SDN_ENCODE_DEVICE', '1') != '0'


def _qualifies(t, dtypes):
    # (device.type, not is_cuda: tests/trace_stub.py answers True for is_cuda on CPU tensors)
    return (isinstance(t, torch.Tensor) and t.device.type == 'cuda' and t.dtype in dtypes and t.dim() == 4 and t.shape[1] == 1
            and t.numel() > 0 and t.is_contiguous())


def encode_maps_supported(label, inst, pose, label_nc, pose_ch):
    """Whether encode_maps takes these maps as they are: CUDA, contiguous [N, 1, H, W] of one shape, supported dtypes,
    1 <= label_nc <= 256, pose_ch <= 256 (inst and pose may be None)."""
    if not _qualifies(label, ops.ENCODE_LABEL_DTYPES) or not 1 <= int(label_nc) <= ops.ENCODE_MAX_CHANNELS:
        return False
    if inst is not None and not (_qualifies(inst, ops.ENCODE_INST_DTYPES) and inst.shape == label.shape and inst.device == label.device):
        return False
    if pose is not None and not (_qualifies(pose, ops.ENCODE_POSE_DTYPES) and pose.shape == label.shape and pose.device == label.device
                                 and 1 <= int(pose_ch) <= ops.ENCODE_MAX_CHANNELS):
        return False
    planes = max(int(label_nc) + (inst is not None), int(pose_ch) if pose is not None else 0)
    return label.numel() * planes < 2 ** 31


def instance_index_supported(inst):
    """Whether instance_index takes this map as it is: CUDA, contiguous [N, 1, H, W], int16 / int32 / float32."""
    return _qualifies(inst, ops.ENCODE_INST_DTYPES) and inst.numel() < 2 ** 31


def encode_maps(label, inst, pose, label_nc, pose_ch):
    """(input_label fp32 [N, label_nc (+ 1 with inst), H, W], pose_onehot fp32 [N, pose_ch, H, W] or None, bad int32 [2]): the
    one-hot planes of label and pose (the value truncated toward zero selects the plane) and the 4-neighbour edge plane of inst,
    every element written in one launch; bad counts the label / pose pixels whose index lies outside [0, channels) or is NaN,
    which set no plane.  See sdn_hip.ops.encode_maps."""
    return ops.encode_maps(label, inst, pose, label_nc, pose_ch)


def instance_index(inst, with_counts=False):
    """(ids int64 [K] ascending, seg int32 [N, H, W], counts int64 [K] or None, info) of inst [N, 1, H, W], which is
    disambiguated in place (inst[i] = inst[i] * bs + i): what torch.unique(inst.reshape(-1).long(), return_inverse=True,
    return_counts=with_counts) gives, without a sort.  info['path'] is 'device' or 'torch' (a key outside the window).  See
    sdn_hip.ops.inst_index."""
    return ops.inst_index(inst, with_counts)
