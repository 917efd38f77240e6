"""ctypes binding of libsdn_hip.so (include/sdn_hip.h) for torch tensors on an MI355X.

This is plumbing only: it checks dtype / device / contiguity, hands `tensor.data_ptr()` and the
current HIP stream to the C ABI and turns error codes into exceptions.  There is NO fallback: if
the shared library is missing or a tensor is not on the GPU the call raises (the reference's
CPU path raises NotImplementedError too, neural_renderer/rasterize.py:890-894).
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, '..', 'lib', 'libsdn_hip.so'))

# flags (include/sdn_hip.h)
RGB, ALPHA, DEPTH, AA, FACE_COLOR, SAVE_MAPS, ACCUMULATE, SERIAL_EDGES, STREAM_FACES, COUNT_WORK = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
K1_COVERAGE = 4096   # SDN_K1_COVERAGE: the reference's default ("unsafe") forward kernel's coverage rule, deterministic ties

ABI_VERSION = 20   # include/sdn_hip.h: SDN_ABI_VERSION this binding was written against (buffer sizes, argument lists)

_lib = None
_lock = threading.Lock()
_vp = ctypes.c_void_p
_ci = ctypes.c_int
_cl = ctypes.c_long
_cd = ctypes.c_double
_sz = ctypes.c_size_t


class SdnHipError(RuntimeError):
    pass


def _signatures():
    """THE list of entry points: name -> argtypes of every `int sdn_*(...)` of include/sdn_hip.h.  sdn_last_error and sdn_version,
    the two that do not return an error code, are declared by _declare itself."""
    sig = {
        'sdn_project_vertices': [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _vp],
        'sdn_project_vertices_bwd': [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp],
        'sdn_gather_faces': [_vp, _vp, _ci, _ci, _ci, _cl, _ci, _vp, _vp],
        'sdn_gather_faces_bwd': [_vp, _vp, _ci, _ci, _ci, _cl, _ci, _vp, _vp],
        'sdn_face_normals': [_vp, _cl, _vp, _vp],
        'sdn_face_normals_bwd': [_vp, _vp, _cl, _vp, _vp],
        'sdn_raster_workspace_bytes': [_ci, _ci, _ci, ctypes.POINTER(_sz)],
        'sdn_rasterize_fwd': [_vp, _vp, _ci, _ci, _ci, _ci, _cd, _cd, _cd, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp, _vp, _sz, _vp],
        'sdn_raster_bwd_workspace_bytes': [_ci, _ci, _ci, ctypes.POINTER(_sz)],
        'sdn_rasterize_bwd': [_vp, _vp, _ci, _ci, _ci, _ci, _cd, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp, _sz, _vp],
    }
    sig['sdn_raster_work_counters'] = [_vp, _ci, _ci, _ci, ctypes.POINTER(ctypes.c_ulonglong), _vp]
    sig['sdn_ffd_decode'] = [_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_ffd_decode_bwd'] = [_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp]
    _i8p = ctypes.POINTER(ctypes.c_int8)
    _cf = ctypes.c_float
    sig['sdn_conv_gemm_workspace_bytes'] = [_ci, _ci, _ci, _ci, ctypes.POINTER(_sz)]
    sig['sdn_conv_gemm'] = [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _i8p, _i8p,
                            _ci, _ci, _vp, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _vp, _sz, _vp]
    _i32p = ctypes.POINTER(ctypes.c_int32)
    sig['sdn_conv_gemm_phases'] = [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _i32p, _i32p, _i32p, _i32p, _i32p, _i8p,
                                   _ci, _ci, ctypes.POINTER(_vp), _i32p, _ci, _vp, _ci, _vp, _ci, _ci, _vp]
    sig['sdn_conv_wgrad'] = [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _i8p, _i8p, _ci, _ci, _ci, _ci,
                             _ci, _vp, _sz, _vp]
    sig['sdn_conv_wgrad_narrow'] = [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _i8p, _i8p, _ci, _ci, _ci,
                                    _vp]
    sig['sdn_conv_wgrad_head_mfma'] = [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _i8p, _i8p, _ci, _ci, _ci,
                                    _vp]
    sig['sdn_conv_narrow_fwd'] = [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci,
                                  _vp, _ci, _vp]
    sig['sdn_conv_head_steps'] = [_ci, _ci, _ci, ctypes.POINTER(_ci)]
    sig['sdn_conv_head_mfma'] = [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp]
    sig['sdn_in_apply'] = [_vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _cf, _ci, _ci, _cf, _vp, _vp, _vp, _cl, _ci, _vp]
    sig['sdn_in_bwd'] = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _cl, _vp]
    sig['sdn_act_bwd'] = [_vp, _vp, _vp, _cl, _ci, _ci, _vp, _cl, _vp]
    sig['sdn_reflect_fold'] = [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]
    sig['sdn_conv_pack_weights'] = [_vp, _ci, _ci, _cl, _cl, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_conv_unpack_grad'] = [_vp, _ci, _ci, _cl, _cl, _vp, _ci, _ci, _vp, _ci, _vp]
    sig['sdn_split_planes'] = [_vp, _cl, _ci, _vp, _cl, _vp]
    sig['sdn_assemble_nhwc'] = [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_conv_pack_weights_kmajor'] = [_vp, _ci, _ci, _cl, _cl, _vp, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_conv_tile'] = [_vp, _cl, _ci, _ci, _ci, _ci, _vp, _vp, _cl, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci,
                            _i8p, _i8p, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _vp]
    sig['sdn_conv_halo_blocks'] = [_ci, _ci, _ci, _ci, _ci, _ci, ctypes.POINTER(_ci), ctypes.POINTER(_ci), ctypes.POINTER(_cl)]
    sig['sdn_conv_halo'] = [_vp, _cl, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _i8p, _i8p, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp]
    sig['sdn_conv_wgrad_tile'] = [_vp, _cl, _vp, _cl, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _i8p, _i8p, _ci, _vp]
    sig['sdn_segment_mean'] = [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_l1_loss_fwd'] = [_vp, _vp, _cl, _vp, _vp, _vp]
    sig['sdn_l1_loss_bwd'] = [_vp, _vp, _cl, _vp, _vp, _vp, _vp]
    sig['sdn_silhouette_loss_fwd'] = [_vp, _vp, _vp, _cl, _vp, _cl, _vp, _vp, _vp]
    sig['sdn_silhouette_loss_bwd'] = [_vp, _vp, _vp, _cl, _vp, _cl, _vp, _vp, _vp, _vp, _vp]
    sig['sdn_pose_params'] = [_vp, _vp, _ci, _vp, _vp, _vp]
    sig['sdn_pose_params_bwd'] = [_vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp]
    sig['sdn_pose_algebra'] = [_vp] * 7 + [_ci, _ci, ctypes.c_float, ctypes.c_float] + [_vp] * 9 + [_vp]
    sig['sdn_pose_algebra_bwd'] = [_vp] * 8 + [_ci, _ci] + [_vp] * 8 + [_vp] * 4 + [_vp]
    sig['sdn_composite_frame'] = [_vp, _vp, _vp, _vp, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_edit_assemble'] = [_vp, _cl, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp]
    sig['sdn_scene_cover'] = [_vp, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_scene_crops'] = [_vp] * 8 + [_ci] * 6 + [_cf] * 6 + [_vp] * 4
    sig['sdn_scene_edit'] = [_vp] * 7 + [_ci, _ci, _ci] + [_vp] * 5
    sig['sdn_unmold_masks'] = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp]
    sig['sdn_scene_gt_masks'] = [_vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_scene_paint2d'] = [_vp, _vp, _vp, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_scene_id_workspace_bytes'] = [ctypes.POINTER(_sz)]
    sig['sdn_scene_id_stats'] = [_vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp]
    sig['sdn_scene_id_planes'] = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_assemble_planes'] = [_vp] * 5 + [_ci, _vp, _vp, _ci, _vp] + [_ci] * 9 + [_cf, _cf, _ci, _cf, _vp, _vp]
    sig['sdn_assemble_maps'] = [_vp] * 10 + [_ci] * 9 + [_vp] * 4 + [_ci, _ci] + [_vp] * 4
    sig['sdn_train_rois'] = [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_train_crops'] = [_vp, _vp, _ci, _ci, _ci] + [_vp] * 5 + [_ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci] + [_cf] * 6 + [_vp] * 5
    sig['sdn_train_id_stats_workspace_bytes'] = [_ci, ctypes.POINTER(_sz)]
    sig['sdn_train_id_stats'] = [_vp, _ci, _cl, _vp, _vp, _vp]
    sig['sdn_train_crops_mixed'] = [_vp] * 5 + [_ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci] + [_vp] * 5
    sig['sdn_segm_fuse'] = [_vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp]
    sig['sdn_segm_labels_from_colors'] = [_vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp, _vp]
    sig['sdn_segm_confusion'] = [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_segm_train_batch'] = [_vp, _vp, _ci, _ci, _ci, _vp, _vp, _cl, _ci, _ci, _ci] + [_cf] * 6 + [_vp, _cl, _vp, _vp, _vp, _vp]
    sig['sdn_segm_loss_fwd'] = [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _cf, _vp, _sz, _vp, _vp, _vp, _vp]
    sig['sdn_segm_loss_bwd'] = [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _cf, _vp, _vp, _vp, _vp, _vp, _vp]
    sig['sdn_segm_ppm_pool'] = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp, _vp]
    sig['sdn_segm_ppm_fill'] = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp]
    sig['sdn_segm_ppm_fill_bwd'] = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp]
    sig['sdn_segm_ppm_pool_bwd'] = [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp]
    sig['sdn_encode_maps'] = [_vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_inst_index_workspace_bytes'] = [ctypes.POINTER(_sz)]
    sig['sdn_inst_index_build'] = [_vp, _ci, _ci, _ci, _ci, _vp, _sz, _vp, _vp, _cl, _vp]
    sig['sdn_inst_index_rank'] = [_vp, _ci, _ci, _ci, _ci, _vp, _sz, _vp, _vp, _vp]
    sig['sdn_mrcnn_loss_workspace_bytes'] = [_ci, _ci, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    _mrl_inputs = [_vp, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci]
    sig['sdn_mrcnn_loss_fwd'] = _mrl_inputs + [_vp, _sz, _vp, _sz, _vp, _vp, _vp]
    sig['sdn_mrcnn_loss_bwd'] = _mrl_inputs + [_vp, _sz, _vp] + [_vp] * 5 + [_vp]
    _ip = ctypes.POINTER(_ci)
    sig['sdn_pyramid_roi_align_grad_floats'] = [_ci, _ip, _ip, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    sig['sdn_pyramid_roi_align_fwd'] = [_vp, _ci, ctypes.POINTER(_vp), _ip, _ip, _ci, _ci, _cf, _cf, _vp, _vp, _vp]
    sig['sdn_pyramid_roi_align_bwd'] = [_vp, _vp, _ci, _ip, _ip, _ci, _ci, _cf, _vp, _vp]
    sig['sdn_pyramid_roi_align_bwd_ordered_workspace_bytes'] = [_ci, ctypes.POINTER(_sz)]
    sig['sdn_pyramid_roi_align_bwd_ordered'] = [_vp, _vp, _ci, _ip, _ip, _ci, _ci, _cf, _vp, _vp, _sz, _vp]
    sig['sdn_proposal_layer_workspace_bytes'] = [_ci, _ci, _ci, ctypes.POINTER(_sz)]
    sig['sdn_proposal_layer'] = [_vp, _vp, _vp, _ci, ctypes.POINTER(_cf), _ci, _ci, _ci, _ci, _cf, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
    sig['sdn_detection_layer_workspace_bytes'] = [_ci, _ci, _ci, ctypes.POINTER(_sz)]
    sig['sdn_detection_layer'] = [_vp, _vp, _vp, _ci, _ci, ctypes.POINTER(_cf), ctypes.POINTER(_cf), _ci, _ci, _cf, _cf, _ci, _ci, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
    sig['sdn_detection_targets_workspace_bytes'] = [_ci] * 7 + [ctypes.POINTER(_sz)]
    sig['sdn_detection_targets'] = [_vp] * 5 + [_ci] * 5 + [_vp, _ci, _cd, ctypes.POINTER(_cf), _ci, _ci, _ci] + [_vp] * 9 + [_sz, _vp]
    sig['sdn_rpn_targets_workspace_bytes'] = [_ci] * 3 + [ctypes.POINTER(_sz)]
    sig['sdn_rpn_targets'] = [_vp] * 4 + [_ci] * 4 + [_vp, _ci, ctypes.POINTER(_cd)] + [_vp] * 5 + [_sz, _vp]
    sig['sdn_training_item_workspace_bytes'] = [_ci] * 4 + [ctypes.POINTER(_sz)]
    sig['sdn_training_item_image'] = [_vp, _ci, _ci, _ci, _vp, _vp, _cl, _vp, _sz, _vp, _vp]
    sig['sdn_training_item'] = [_vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _cl, _ci, _ci, _ci, _vp, _sz] + [_vp] * 7 + [_vp]
    _pp = ctypes.POINTER(_vp)
    sig['sdn_rpn_outputs_fwd'] = [_pp, _pp, _ip, _ip, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_rpn_outputs_bwd'] = [_vp, _vp, _vp, _vp, _ip, _ip, _ci, _ci, _ci, _pp, _pp, _vp]
    sig['sdn_derender_heads_workspace_bytes'] = [_ci] * 5 + [ctypes.POINTER(_sz)]
    sig['sdn_derender_heads_fwd'] = [_vp] * 12 + [_ci] * 5 + [_vp] * 5 + [_vp]
    sig['sdn_derender_heads_bwd'] = [_vp] * 15 + [_ci] * 5 + [_vp] * 9 + [_vp, _sz, _vp]
    sig['sdn_train_losses_scratch'] = [_ci, _ci, _cl, ctypes.POINTER(_sz)]
    sig['sdn_train_losses_fwd'] = [_vp] * 7 + [_cl] + [_vp] * 7 + [_ci, _ci, _ci, _ci, _cd, _cd, _vp, _vp, _vp]
    sig['sdn_train_losses_bwd'] = [_vp] * 6 + [_cl] + [_vp] * 7 + [_ci, _ci, _ci, _ci, _cd, _cd] + [_vp] * 9 + [_vp]
    sig['sdn_perspective_transform_scratch'] = [_ci, _ci, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    sig['sdn_perspective_transform'] = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_perspective_transform_bwd'] = [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp]
    sig['sdn_bn_forward'] = [_vp, _cl, _ci, _vp, _vp, _vp, _vp, _cf, _cf, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp]
    sig['sdn_bn_backward'] = [_vp, _vp, _vp, _vp, _vp, _cl, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
    sig['sdn_maxpool3x3s2_fwd'] = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp]
    sig['sdn_maxpool3x3s2_bwd'] = [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_avgpool_global'] = [_vp, _ci, _ci, _ci, _vp, _ci, _vp]
    sig['sdn_nms_workspace_bytes'] = [_ci, ctypes.POINTER(_sz)]
    sig['sdn_nms'] = [_vp, _vp, _ci, _cf, _ci, _vp, _vp, _vp, _sz, _vp]
    sig['sdn_crop_and_resize_fwd'] = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _cf, _vp, _vp]
    sig['sdn_crop_and_resize_bwd'] = [_vp, _vp, _vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _vp]
    sig['sdn_timing_enable'] = [_ci]
    sig['sdn_timing_declare_work'] = [_cd]
    sig['sdn_timing_read'] = [ctypes.POINTER(_cd), ctypes.POINTER(_cl)]
    sig['sdn_timing_read_slot'] = [_ci, ctypes.POINTER(_cd), ctypes.POINTER(_cl), ctypes.POINTER(_cd)]
    sig['sdn_ffd_coefficients'] = [_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp]
    sig['sdn_raster_phase_clocks'] = [_vp, _ci, _ci, _ci, ctypes.POINTER(ctypes.c_ulonglong), _vp]
    sig['sdn_render_maps_bytes'] = [_ci, _ci, _ci, _ci, _ci, _ci, ctypes.POINTER(_sz), ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    sig['sdn_render_maps_fwd'] = [_vp, _ci, _ci, _vp, _ci, _cl, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cd, _cd, _cd, _vp,
                                  _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]
    sig['sdn_render_maps_bwd'] = [_vp, _ci, _ci, _vp, _ci, _cl, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cd, _cd, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _sz, _vp, _sz, _vp]
    _lp = ctypes.POINTER(_cl)
    sig['sdn_avgpool3x3s2_fwd'] = [_vp, _ci, _ci, _ci, _ci, _lp, _vp, _lp, _ci, _vp]
    sig['sdn_avgpool3x3s2_bwd'] = [_vp, _ci, _ci, _ci, _ci, _lp, _vp, _lp, _ci, _vp]
    sig['sdn_program_create'] = [_vp, _ci, _vp, _sz, _ci, ctypes.POINTER(_vp)]
    sig['sdn_program_run'] = [_vp, ctypes.POINTER(_vp), _ci, _vp, _vp, ctypes.POINTER(_cf), ctypes.POINTER(_ci)]
    sig['sdn_program_destroy'] = [_vp]
    return sig


_SIG = _signatures()


def _declare(L):
    """Set argtypes and restype on the entry points of `L` (the library, or a stand-in of a test or tool); -> the table."""
    L.sdn_last_error.restype = ctypes.c_char_p
    L.sdn_version.restype = _ci
    for name, argtypes in _SIG.items():
        try:
            fn = getattr(L, name)
        except AttributeError:   # whatever the name: a library without it was built before it was added
            raise SdnHipError('%s does not export %s -- rebuild it (`python __graft_entry__.py build`)' % (LIB_PATH, name))
        fn.argtypes = argtypes
        fn.restype = _ci
    return _SIG


def lib():
    """Load the HIP library once; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise SdnHipError(
                        'libsdn_hip.so not found at %s -- run `python __graft_entry__.py build` (hipcc, gfx950); '
                        'there is no CPU or PyTorch fallback for this path' % LIB_PATH)
                L = ctypes.CDLL(LIB_PATH)
                L.sdn_version.restype = _ci
                have = L.sdn_version()
                if have != ABI_VERSION:
                    # signatures are plain C: a stale library would take buffers of the wrong size without a word
                    raise SdnHipError('%s reports ABI version %d, this binding needs %d -- rebuild it '
                                      '(`python __graft_entry__.py build`)' % (LIB_PATH, have, ABI_VERSION))
                _declare(L)
                _lib = L
    return _lib


def exported_symbols():
    """Names declared in include/sdn_hip.h that this binding expects."""
    return ['sdn_last_error', 'sdn_version'] + list(_SIG)


def deterministic():
    """The one rule for "deterministic": torch's own switch -- torch.use_deterministic_algorithms(True) -- or SDN_DETERMINISTIC=1.
    With it on, every path that would combine sums with float atomics takes its fixed-order form: the conv stack's split-K sums
    (sdn_hip.conv) and the pyramid RoIAlign's backward (sdn_hip.ops.pyramid_backward_path).  Read when a call runs, not at import."""
    return torch.are_deterministic_algorithms_enabled() or os.environ.get('SDN_DETERMINISTIC') == '1'


def check(rc):
    if rc != 0:
        raise SdnHipError('libsdn_hip error %d: %s' % (rc, lib().sdn_last_error().decode()))


def ptr(t):
    # (a plain int: ctypes converts it for the c_void_p parameters declared in _declare(); building a c_void_p object per
    # argument was a measurable share of the ~65 pointer arguments of a frame step)
    return None if t is None else t.data_ptr()


def stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def want(t, dtype, name):
    """Validate a tensor argument the way chainer's type_check did (rasterize.py:66-90), plus device."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(t)))
    if not t.is_cuda:
        # the reference: Rasterize.forward_cpu raises NotImplementedError (rasterize.py:890-891)
        raise NotImplementedError('%s is on %s; this renderer only runs on the GPU' % (name, t.device))
    if t.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    return t.contiguous()


_const_cache = {}


def const_f32(values, device):
    """Device copy of a small host constant (camera vectors, background colours, per-object tan(angle)), cached by value:
    the reference re-uploads these on every call (derender3d/models/renderer.py:243-248); a cached copy also keeps the
    render path free of host-to-device copies, which a HIP-graph capture of the step requires."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
    key = (a.tobytes(), a.shape, str(device))
    t = _const_cache.get(key)
    if t is None:
        if len(_const_cache) > 4096:
            _const_cache.clear()
        t = _const_cache[key] = torch.tensor(a, device=device)
    return t


def size_query(fn, ints=(), outputs=1):
    """What a size entry point of the library answers.  `fn` is the function object itself -- the caller writes
    `lib().sdn_..._bytes`, so that `lib` is looked up in the caller's module --, `ints` its int arguments, handed over as they
    are (a caller that takes sizes of any kind converts them), `outputs` the number of `size_t *` behind them.  -> an int, or a
    tuple of `outputs` ints."""
    out = [_sz(0) for _ in range(outputs)]
    check(fn(*ints, *[ctypes.byref(n) for n in out]))
    return out[0].value if outputs == 1 else tuple(n.value for n in out)


def c_ints(values):
    """an `int[len(values)]` of Python ints for a `const int *` parameter"""
    return (_ci * len(values))(*values)


def c_ptrs(tensors):
    """a `void *[len(tensors)]` of the tensors' addresses, NULL for None"""
    return (_vp * len(tensors))(*[ptr(t) for t in tensors])


def c_floats(values):
    """a `float[len(values)]` of host numbers"""
    return (ctypes.c_float * len(values))(*values)


def raster_workspace(bs, nf, S, device):
    return torch.empty(size_query(lib().sdn_raster_workspace_bytes, (bs, nf, S)), dtype=torch.uint8, device=device)


def perspective_transform_scratch(n, V):
    """(bytes of `key`, bytes of `acc`) of sdn_perspective_transform / _bwd, asked of the library."""
    return size_query(lib().sdn_perspective_transform_scratch, (n, V), 2)


def train_losses_scratch(B, R, nffd):
    """bytes of the `scratch` of sdn_train_losses_fwd / _bwd, asked of the library"""
    return size_query(lib().sdn_train_losses_scratch, (B, R, nffd))


def raster_bwd_workspace(bs, nf, S, device):
    return torch.empty(size_query(lib().sdn_raster_bwd_workspace_bytes, (bs, nf, S)), dtype=torch.uint8, device=device)


def scene_id_workspace(device):
    """the histograms of sdn_scene_id_stats, sized by the library; the call clears them itself"""
    return torch.empty(size_query(lib().sdn_scene_id_workspace_bytes), dtype=torch.uint8, device=device)


def train_id_workspace(B, device):
    """the histograms of sdn_train_id_stats for B items, sized by the library; the call clears them itself"""
    return torch.empty(size_query(lib().sdn_train_id_stats_workspace_bytes, (int(B),)), dtype=torch.uint8, device=device)


def timing_enable(on=True):
    check(lib().sdn_timing_enable(int(bool(on))))


def timing_read():
    """(total k_raster_tiles milliseconds, launches) since the previous read."""
    ms, n = _cd(0), _cl(0)
    check(lib().sdn_timing_read(ctypes.byref(ms), ctypes.byref(n)))
    return ms.value, n.value


SLOT_RASTER_TILES, SLOT_EDGE_SCAN, SLOT_CONV_GEMM, SLOT_CONV_WGRAD, SLOT_CONV_NARROW, SLOT_RASTER_TILES_K1 = 0, 1, 2, 3, 4, 5
SLOT_SCENE_MASKS = 6   # k_unmold_masks, k_scene_gt_masks (csrc/scene_masks.hip)


def timing_read_slot(slot):
    """(total milliseconds, launches, declared algorithmic work) of one timed kernel family since the previous read."""
    ms, n, w = _cd(0), _cl(0), _cd(0)
    check(lib().sdn_timing_read_slot(slot, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w)))
    return ms.value, n.value, w.value
