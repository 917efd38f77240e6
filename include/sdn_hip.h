/*
 * sdn_hip.h -- C ABI of libsdn_hip.so, the MI355X (gfx950) implementation of 3D-SDN's hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's allocator on the Python side),
 *     except `size_t* out`/`int* out` result slots and `const char*` returns, which are host memory;
 *   - every launcher takes a `sdnStream` (a hipStream_t passed as void*), enqueues asynchronously
 *     and returns 0 on success or a negative SDN_E* code; sdn_last_error() holds the text
 *     (thread-local);  there is no global mutable state, so the library is re-entrant across the
 *     one-Python-thread-per-GPU callers of nn.DataParallel
 *     (reference: geometric/scripts/main.py:182);
 *   - tensors are dense, row-major, float32 / int32, shapes as documented per argument.
 *
 * Each entry point cites the reference interface it replaces (paths under
 * /root/reference/geometric/ or /root/reference/textural/).  INTEGRATION.md shows the
 * reference-side binding (ctypes) a maintainer would add.
 */
#ifndef SDN_HIP_H
#define SDN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sdnStream;

#define SDN_OK 0
#define SDN_EINVAL (-1)   /* bad argument (shape, flag combination, null pointer) */
#define SDN_ELAUNCH (-2)  /* HIP launch / runtime error */
#define SDN_ENOMEM (-3)   /* workspace too small */

/* flags of sdn_rasterize_fwd / _bwd */
#define SDN_RGB 1          /* return_rgb   (rasterize.py:21) */
#define SDN_ALPHA 2        /* return_alpha */
#define SDN_DEPTH 4        /* return_depth */
#define SDN_AA 8           /* outputs are 2x2 average-pooled (rasterize.py:942-966) */
#define SDN_FACE_COLOR 16  /* `textures` is [bs,nf,3]: one colour per face, sampled through the same
                              trilinear arithmetic as a constant ts=2 texture (render_normal,
                              derender3d/models/renderer.py:78-79) */
#define SDN_SAVE_MAPS 32   /* keep the S x S maps needed by sdn_rasterize_bwd */
#define SDN_ACCUMULATE 64  /* sdn_rasterize_bwd: add into grad_faces / grad_textures instead of overwriting */
#define SDN_STREAM_FACES 256 /* sdn_rasterize_fwd: skip the per-tile face lists; every tile streams all faces (the path
                               taken automatically when the lists overflow their budget; for verification) */
#define SDN_COUNT_WORK 512 /* sdn_rasterize_fwd: also tally candidate pixel tests / tests passed / depth keys of k_raster_tiles
                             into the workspace (read with sdn_raster_work_counters; a measurement build of the kernel,
                             never timed) */
#define SDN_SPARSE_GRAD 1024 /* sdn_rasterize_bwd: grad_faces rows of faces that own no pixel of the face-index map (their
                                gradient is zero) are left UNWRITTEN; the caller must skip them -- their flags are
                                u32[bs * nf] at byte 256 of the workspace (used by sdn_render_maps_bwd: most faces of a mesh are
                                hidden, writing and re-reading 36 zero bytes for each was a tenth of the frame step) */
#define SDN_LAZY_MAPS 2048 /* sdn_rasterize_fwd with SDN_SAVE_MAPS: store only the face-index and depth maps (8 of the 32 bytes
                              per internal pixel); the barycentric-weight and colour maps are re-derived -- bit-identically, by
                              the forward's own shading routine -- when a backward pass needs them (depth / colour
                              gradients), never for the silhouette gradient.  Used by sdn_render_maps_fwd / _bwd. */
#define SDN_K1_COVERAGE 4096 /* sdn_rasterize_fwd / sdn_render_maps_fwd: the coverage rule and barycentric arithmetic of the
                              reference's DEFAULT forward kernel K1 (rasterize.py:102-236, selected by scripts/env.sh:11 through
                              NEURAL_RENDERER_UNSAFE=1): pixel-space scanlines over the x-sorted vertices instead of the safe
                              kernels' NDC edge tests.  Exact depth ties, which K1 leaves to thread scheduling, go to the lowest
                              face index.  A plain (untuned) tile kernel serves it; the backward entry points need no flag (they
                              read the maps and face_inv the forward call left, as the reference's do). */
#define SDN_SERIAL_EDGES 128 /* sdn_rasterize_bwd: walk every edge serially in the reference's summation order
                               (bit-comparable with rasterize.py:523-745; slow, for verification) */

const char* sdn_last_error(void);
/* The ABI revision this header describes.  It is raised whenever an entry point gains / loses an argument OR a caller-owned
 * buffer changes its required size behind an unchanged signature (r04: the `key` / `acc` scratch of
 * sdn_perspective_transform*, new arguments of sdn_in_apply / sdn_in_bwd / sdn_act_bwd / sdn_render_maps_*; r05: struct sdn_op
 * with 40 ints, sdn_render_maps_bwd takes bg; 9: sdn_edit_assemble added; 10: sdn_scene_cover, sdn_scene_crops,
 * sdn_scene_edit added; 11: sdn_unmold_masks, sdn_scene_gt_masks added, timing slot 6; 12: sdn_scene_paint2d added; 13:
 * sdn_scene_id_workspace_bytes, sdn_scene_id_stats, sdn_scene_id_planes added; 14: sdn_assemble_planes, sdn_assemble_maps
 * added; 15: sdn_train_rois, sdn_train_crops added; 16: sdn_train_losses_scratch, sdn_train_losses_fwd, sdn_train_losses_bwd
 * added; 17: sdn_train_id_stats_workspace_bytes, sdn_train_id_stats, sdn_train_crops_mixed added; 18: sdn_segm_fuse,
 * sdn_segm_labels_from_colors, sdn_segm_confusion added; 19: sdn_segm_train_batch added; 20: sdn_segm_loss_fwd,
 * sdn_segm_loss_bwd added; still 20: sdn_segm_ppm_pool, sdn_segm_ppm_fill, sdn_segm_ppm_fill_bwd, sdn_segm_ppm_pool_bwd added; still 20: sdn_encode_maps,
 * sdn_inst_index_workspace_bytes, sdn_inst_index_build, sdn_inst_index_rank added; still 20: sdn_mrcnn_loss_workspace_bytes,
 * sdn_mrcnn_loss_fwd, sdn_mrcnn_loss_bwd added; still 20: sdn_pyramid_roi_align_grad_floats, sdn_pyramid_roi_align_fwd,
 * sdn_pyramid_roi_align_bwd added; still 20: sdn_proposal_layer_workspace_bytes, sdn_proposal_layer added; still 20:
 * sdn_detection_layer_workspace_bytes, sdn_detection_layer added; still 20: sdn_detection_targets_workspace_bytes,
 * sdn_detection_targets added; still 20: sdn_rpn_targets_workspace_bytes, sdn_rpn_targets added; still 20: sdn_training_item_workspace_bytes,
 * sdn_training_item_image, sdn_training_item added; still 20: sdn_rpn_outputs_fwd, sdn_rpn_outputs_bwd added; still 20:
 * sdn_pyramid_roi_align_bwd_ordered_workspace_bytes, sdn_pyramid_roi_align_bwd_ordered added; still 20:
 * sdn_derender_heads_workspace_bytes, sdn_derender_heads_fwd, sdn_derender_heads_bwd added -- new entry
 * points only, no signature or buffer size of an existing one changed; a library without them fails to bind by name).  A binding must compare sdn_version() with the SDN_ABI_VERSION it was
 * written against and refuse a library that answers otherwise (sdn_hip/__init__.py: lib()): a stale lib/libsdn_hip.so would otherwise be handed buffers of the wrong
 * size. */
#define SDN_ABI_VERSION 20
int sdn_version(void);

/* ---- camera: neural_renderer/look.py:7-45, look_at.py:7-46, perspective.py:5-19 ------------------
 * out[b,v] = perspective(look*(verts[b,v] * (flip_x ? (-1,1,1) : 1))).
 * camera_mode: 0 none, 1 'look' (dir = viewing direction), 2 'look_at' (dir = `at` point).
 * eye/dir/up: [bs,3].  width: [bs] = tan(angle/180*3.1416) or NULL for no perspective division.
 * flip_x folds derender3d/models/renderer.py:243. */
int sdn_project_vertices(const float* verts, int bs, int nv, int camera_mode, const float* eye,
                         const float* dir, const float* up, const float* width, int flip_x,
                         float* out, sdnStream stream);
/* grad_verts[b,v] = d loss / d verts, given grad_out = d loss / d out.  (Chainer autograd of the ops
 * above; the reference only propagates to vertices, derender3d/models/renderer.py:205-213.) */
int sdn_project_vertices_bwd(const float* verts, int bs, int nv, int camera_mode, const float* eye,
                             const float* dir, const float* up, const float* width, int flip_x,
                             const float* grad_out, float* grad_verts, sdnStream stream);

/* ---- vertices_to_faces + fill_back: neural_renderer/vertices_to_faces.py:4-21, renderer.py:41 -----
 * faces_out[b, f]      = verts[b, faces[b,f,{0,1,2}]]            f <  nf0
 * faces_out[b, nf0+f]  = verts[b, faces[b,f,{2,1,0}]]            when fill_back
 * faces_idx may be shared by the whole batch (faces_batch_stride = 0) or per batch (= nf0*3). */
int sdn_gather_faces(const float* verts, const int32_t* faces_idx, int bs, int nv, int nf0,
                     long faces_batch_stride, int fill_back, float* faces_out, sdnStream stream);
/* scatter-add of grad_faces [bs,nf,3,3] into grad_verts [bs,nv,3] (zeroed by the callee). */
int sdn_gather_faces_bwd(const float* grad_faces, const int32_t* faces_idx, int bs, int nv, int nf0,
                         long faces_batch_stride, int fill_back, float* grad_verts, sdnStream stream);

/* ---- face normals: derender3d/models/renderer.py:66-76 (cross.py:25-38 + chainer normalize) -------
 * normals[b,f] = normalize(cross(v0 - v1, v2 - v1)), eps 1e-5 added to the norm. faces [bs,nf,3,3]. */
int sdn_face_normals(const float* faces, long n_faces_total, float* normals, sdnStream stream);
int sdn_face_normals_bwd(const float* faces, const float* grad_normals, long n_faces_total,
                         float* grad_faces, sdnStream stream);

/* ---- Rasterize: neural_renderer/rasterize.py:19-894 + rasterize_rgbad :897-974 --------------------
 * S = internal image size (2*image_size with SDN_AA).  Workspace: query first. */
int sdn_raster_workspace_bytes(int bs, int nf, int S, size_t* out);

/* Forward.  faces [bs,nf,3,3] post-projection (x,y NDC, z depth).
 * textures: NULL | [bs,nf,ts,ts,ts,3] | [bs,nf,3] with SDN_FACE_COLOR.   bg: [3] or [bs,3].
 * Saved state (required iff SDN_SAVE_MAPS; else may be NULL):
 *   face_index_map [bs,S,S] i32, weight_map [bs,S,S,3], depth_map [bs,S,S], rgb_map [bs,S,S,3]
 *   (only with SDN_RGB).   face_inv [bs,nf,3,3] is always written (workspace-like, caller-owned).
 * Outputs (R = S/2 with SDN_AA else S; vertically flipped like rasterize.py:953-957):
 *   rgb_out [bs,3,R,R], alpha_out [bs,R,R], depth_out [bs,R,R]; each may be NULL if its flag is off. */
int sdn_rasterize_fwd(const float* faces, const float* textures, int ts, int bs, int nf, int S,
                      double near, double far, double eps, const float* bg, int bg_per_batch, int flags,
                      float* face_inv, int32_t* face_index_map, float* weight_map, float* depth_map,
                      float* rgb_map, float* rgb_out, float* alpha_out, float* depth_out,
                      void* workspace, size_t workspace_bytes, sdnStream stream);

/* After a forward call with SDN_COUNT_WORK: out3 (HOST memory) = {candidate pixel tests, tests passed
 * (rasterize.py:311-313), depth keys submitted (:332)} of k_raster_tiles, summed over the launch.  Synchronises the stream.
 * Measurement aid for bench.py's ALU roofline; the counting build of the kernel is never the timed one. */
int sdn_raster_work_counters(const void* workspace, int bs, int nf, int S, unsigned long long* out3, sdnStream stream);

/* Same counting build: out8 (HOST memory) = shader-clock ticks summed over the launch's WAVES for {batch fetch + waiting
 * for the tile's other waves, the candidate stream (formerly: lane-private boxes), wave-shared row spans, thin faces, epilogue, whole kernel}, then the
 * longest wave's ticks and the number of waves (a 1/16 sample of the tiles; ticks of the 100 MHz constant clock).  Tells an unbalanced launch (max >> mean) from a uniformly slow one.
 * Measurement aid (tools/tile_stats.py); synchronises the stream. */
int sdn_raster_phase_clocks(const void* workspace, int bs, int nf, int S, unsigned long long* out8, sdnStream stream);

/* Backward (rasterize.py:846-886): K5 silhouette/colour edge gradient, K6 texture scatter, K7 depth.
 * g_* are gradients wrt the (pooled, flipped) outputs of the forward call, NULL = zero.
 * grad_faces [bs,nf,3,3] and grad_textures (same shape as textures) are fully written by the callee
 * (added to with SDN_ACCUMULATE).  Workspace: query sdn_raster_bwd_workspace_bytes first. */
int sdn_raster_bwd_workspace_bytes(int bs, int nf, int S, size_t* out);
int sdn_rasterize_bwd(const float* faces, const float* textures, int ts, int bs, int nf, int S,
                      double eps, int flags, const float* face_inv, const int32_t* face_index_map,
                      const float* weight_map, const float* depth_map, const float* rgb_map,
                      const float* g_rgb_out, const float* g_alpha_out, const float* g_depth_out,
                      float* grad_faces, float* grad_textures, void* workspace, size_t workspace_bytes,
                      sdnStream stream);

/* ---- the three maps of a frame's objects in one call each way ------------------------------------------------------------
 * Derenderer3d.render calls Renderer.forward three times per object (derender3d/models/__init__.py:203-224 ->
 * derender3d/models/renderer.py:216-272): x flip (:243), look + perspective, vertices_to_faces with fill_back, face normals
 * as a constant texture (:66-93), Rasterize, x sign of the normal map (:268-270); Chainer's autograd walks it back.
 * sdn_render_maps_fwd issues this library's launchers for all objects of a frame from C, in that order:
 *   [sdn_gather_faces(verts, x flipped) -> sdn_face_normals]  sdn_project_vertices -> sdn_gather_faces -> sdn_rasterize_fwd
 * and sdn_render_maps_bwd the matching sdn_rasterize_bwd (silhouette term with eps_alpha, colour + depth terms with eps:
 * what the reference's separate Rasterize calls use, renderer.py:37,57,90-92) -> sdn_gather_faces_bwd ->
 * sdn_project_vertices_bwd [-> sdn_face_normals_bwd -> sdn_gather_faces_bwd, added].
 * flags: SDN_RGB = the normal map is wanted, SDN_DEPTH, SDN_AA, SDN_SAVE_MAPS (required for _bwd), SDN_SERIAL_EDGES (_bwd).
 * verts [bs,nv,3] as handed to Renderer.forward (NOT flipped); faces_idx / camera arguments as sdn_gather_faces /
 * sdn_project_vertices; bg [3] device (normal map only).  Outputs alpha [bs,R,R], normal [bs,3,R,R], depth [bs,R,R]
 * (R = image_size; NULL when not requested).  state: caller-owned, sdn_render_maps_bytes; it carries the projected vertices,
 * both face arrays, the colours and the S x S maps to the backward call; scratch (fwd_scratch_bytes): the rasterizer's tile
 * lists, dead when the forward call returns to the stream (r04: no longer part of the state a live graph pins).
 * g_* NULL = no gradient for that map.  _bwd's bg (ABI 6): the forward call's background colour again (needed when g_normal or
 * g_depth is given with the normal map on: the lazily stored colour map is re-derived from it; the forward call no longer copies
 * it into the state). */
int sdn_render_maps_bytes(int bs, int nv, int nf0, int fill_back, int image_size, int flags, size_t* state_bytes,
                          size_t* bwd_workspace_bytes, size_t* fwd_scratch_bytes);
int sdn_render_maps_fwd(const float* verts, int bs, int nv, const int32_t* faces_idx, int nf0, long faces_batch_stride,
                        int fill_back, int camera_mode, const float* eye, const float* dir, const float* up,
                        const float* width, int flip_x, int image_size, int flags, double near, double far, double eps,
                        const float* bg, float* alpha_out, float* normal_out, float* depth_out, void* state,
                        size_t state_bytes, void* scratch, size_t scratch_bytes, sdnStream stream);
int sdn_render_maps_bwd(const float* verts, int bs, int nv, const int32_t* faces_idx, int nf0, long faces_batch_stride,
                        int fill_back, int camera_mode, const float* eye, const float* dir, const float* up,
                        const float* width, int flip_x, int image_size, int flags, double eps, double eps_alpha,
                        const float* bg, const float* g_alpha, const float* g_normal, const float* g_depth, float* grad_verts,
                        const void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, sdnStream stream);

/* ---- FFD decode: derender3d/models/transforms.py:68-99 (FFD.forward), batched over objects of different templates --
 * Bt  [n_classes, ncoef, vmax]  Bernstein basis of every template, coefficient-major (padded vertices repeat vertex 0)
 * P   [n, 3, ncoef]             control points P0 + dP of each object (constraints already applied)
 * cls [n] int32                 template of each object
 * out [n, vmax, 3]              deformed vertices.     grad_P [n, 3, ncoef] = d loss / d P given grad_out [n, vmax, 3]. */
int sdn_ffd_decode(const float* Bt, const float* P, const int32_t* cls, int n, int vmax, int ncoef,
                   float* out, sdnStream stream);
int sdn_ffd_decode_bwd(const float* Bt, const int32_t* cls, const float* grad_out, int n, int vmax,
                       int ncoef, float* grad_P, sdnStream stream);
/* The symmetry / homogeneity constraints of FFD.constrain (derender3d/models/transforms.py:69-95) are linear in the
 * coefficients: M [m, m] (row i = constrain(e_i), built once on the host side), m = 3 * grids^3.
 * out [n, m] = base [m] (optional) + x [n, m] . M   (transpose != 0: x . M^T, the gradient direction). */
int sdn_ffd_coefficients(const float* x, const float* M, const float* base, int n, int m, int transpose, float* out,
                         sdnStream stream);

/* ==== textural branch: pix2pixHD-style generator / discriminator / encoder conv stacks ==================================
 * Reference operator surface: textural/models/networks.py (GlobalGenerator :211-239, ResnetBlock :244-283,
 * Encoder :286-308, NLayerDiscriminator :412-461), i.e. nn.Conv2d / nn.ConvTranspose2d / nn.ReflectionPad2d /
 * nn.InstanceNorm2d(affine=False, track_running_stats=True) / ReLU / LeakyReLU(0.2) / Tanh, run by cuDNN there.
 * Activations are channels-last fp32 [N, H, W, Cp], Cp = channel count padded to a multiple of 16 (pad channels hold
 * zeros).  Weights are pre-packed by sdn_conv_pack_weights into one fragment-ordered bf16 (hi, lo) buffer.  `precision` is 3
 * (bf16x3 split products, fp32-class results; the default everywhere) or 1 (plain bf16).
 * dy / dx tap tables are HOST arrays (int8, at most 64 taps). */

/* out[n, qy*ostride+py, qx*ostride+px, co] (=|+=) act(bias[co] + sum_t sum_ci f(in[n, qy*istride+dy[t], qx*istride+dx[t], ci]) * W[co, t*Cip+ci])
 *   Conv2d forward (networks.py:218,224,261,291,297,420-437): ostride 1, istride = stride, dy = ky - pad;
 *   ConvTranspose2d forward (:233,303) and the data gradient of strided Conv2d: one call per output phase (py, px);
 *   pad_mode 0: outside = 0;  1: reflected (ReflectionPad2d folded in, :218,236,251,265).   in_relu: f = ReLU.
 *   act 0 none, 1 LeakyReLU(0.2), 2 tanh.   stats [N, SDN_STAT_SLOTS, Cop, 2] fp64 (zeroed by the caller): += sum, sum of
 *   squares of the pre-activation per (n, co), spread over SDN_STAT_SLOTS partial copies -- the InstanceNorm statistics.   w_packed: 2 * w_rows * Kp bf16 from sdn_conv_pack_weights. */
#define SDN_STAT_SLOTS 8
/*   Layers whose output grid cannot fill the chip are split over K.  workspace NULL: the K slices meet in `out` through float
 *   atomics (fastest; sums differ in the last bits run to run).  workspace (>= sdn_conv_gemm_workspace_bytes): every slice
 *   stores its partial tile and one pass adds them in slice order -- bit-reproducible results (torch's deterministic mode). */
int sdn_conv_gemm_workspace_bytes(int N, int OH, int OW, int Cop, size_t* out);
int sdn_conv_gemm(const float* in, int N, int IH, int IW, int Cip, float* out, int OH, int OW, int Cop, int QH, int QW,
                  int istride, int ostride, int py, int px, int ntaps, const int8_t* dy, const int8_t* dx, int pad_mode,
                  int in_relu, const void* w_packed, int Kp, int w_rows, const float* bias, int act,
                  double* stats, int accumulate, int precision, void* workspace, size_t workspace_bytes,
                  sdnStream stream);

/* The s*s PHASE launches of a ConvTranspose2d forward (networks.py:233,303) or of a strided Conv2d's data gradient -- one
 * sdn_conv_gemm call per output phase (py, px) so far -- as ONE launch (r05).  Common arguments as sdn_conv_gemm; per phase k <
 * nphase (<= 4): its output sub-grid QH[k] x QW[k] at (py[k], px[k]), ntaps[k] (<= 16) taps, its packed weights w_packed[k]
 * (sdn_conv_pack_weights of that phase's tap list, Kp[k] columns).  `taps`: HOST int8, per phase dy[ntaps[k]] then
 * dx[ntaps[k]], phases concatenated; QH .. ntaps, Kp, w_packed are HOST arrays.  No split K (a phase never owns the whole
 * output tensor); bias / act / stats / accumulate apply to every phase's outputs as in the single-phase call. */
int sdn_conv_gemm_phases(const float* in, int N, int IH, int IW, int Cip, float* out, int OH, int OW, int Cop, int istride,
                         int ostride, int nphase, const int32_t* QH, const int32_t* QW, const int32_t* py, const int32_t* px,
                         const int32_t* ntaps, const int8_t* taps, int pad_mode, int in_relu, const void* const* w_packed,
                         const int32_t* Kp, int w_rows, const float* bias, int act, double* stats, int accumulate,
                         int precision, sdnStream stream);

/* dw[r, t*Cc + c] += sum_{n,q} a(rows[n, q, r]) * b(gath[n, q*istride + d_t, c])   (autograd of the layers above wrt their
 * weights).  rows [N, QH, QW, Cr], gath [N, GH, GW, Cc], dw [Cr, ntaps*Cc] fp32, ADDED TO in both modes (the caller zeroes it for a
 * plain gradient; rows and channels of the padding receive sums of zeros and keep their values).  splits: K slices over the
 * positions (at most one per 32-position step); workspace NULL: combined with float atomics; workspace of splits * Cr * ntaps*Cc
 * floats: combined in slice order (bit-reproducible); one too small for the slices actually used is SDN_ENOMEM. */
int sdn_conv_wgrad(const float* rows, const float* gath, float* dw, int N, int QH, int QW, int Cr, int GH, int GW, int Cc,
                   int istride, int ntaps, const int8_t* dy, const int8_t* dx, int pad_mode, int relu_rows,
                   int relu_gath, int splits, int precision, void* workspace, size_t workspace_bytes, sdnStream stream);
/* The same sum for stride-1 layers whose `rows` operand has only rows_used <= 8 meaningful channels (the heads:
 * networks.py:236 c7s1-3, :306 c7s1-5, :437 the discriminators' last 4x4 conv): exact fp32 on the vector ALUs with
 * the gathered operand's tile + halo resident in LDS, instead of a 32-row MFMA tile that re-gathers the input per tap. */
int sdn_conv_wgrad_narrow(const float* rows, const float* gath, float* dw, int N, int QH, int QW, int Cr, int rows_used,
                          int GH, int GW, int Cc, int ntaps, const int8_t* dy, const int8_t* dx, int pad_mode,
                          int relu_rows, int relu_gath, sdnStream stream);

/* The same weight gradient for the 7 x 7 layers with Cr == 16 (rows_used <= 16) on the matrix cores (conv_whead.hip, r06):
 * the generator head 64 -> 3, the encoder head 16 -> 5 and the encoder stem 3 -> 16 (networks.py:236, 306, 291).  bf16 x 3
 * split products with fp32 accumulation, the precision class of sdn_conv_wgrad.  The taps must be a dense 7 x 7 window (any
 * order), Cc 16 or 64; arguments, dw layout and the caller's zero fill as sdn_conv_wgrad_narrow.  Its workgroups meet in dw
 * through float atomics: not for the deterministic mode. */
int sdn_conv_wgrad_head_mfma(const float* rows, const float* gath, float* dw, int N, int QH, int QW, int Cr, int rows_used,
                             int GH, int GW, int Cc, int ntaps, const int8_t* dy, const int8_t* dx, int pad_mode,
                             int relu_rows, int relu_gath, sdnStream stream);

/* Stride-1 convolutions with rows_used <= 8 output channels (the heads above, forward; and a data gradient restricted to
 * a few input channels): exact fp32 on the vector ALUs, the input tile + halo kept in LDS as channel planes.
 *   out[n, q, r] = act(bias[r] + sum_{dy,dx,c} f(in[n, q + (dy_min + dy, dx_min + dx), c]) * w_dense[dy, dx, c, r])
 * w_dense [KH, KW, Cip, RP] fp32 with RP = 1 / 4 / 8 for rows_used 1 / 2-4 / 5-8 (absent taps, channels, rows = 0);
 * KH == KW in {3, 4, 7}.  out [N, QH, QW, Cop]: channels >= rows_used are written as zeros.  pad_mode / in_relu / act as
 * sdn_conv_gemm. */
int sdn_conv_narrow_fwd(const float* in, int N, int IH, int IW, int Cip, float* out, int QH, int QW, int Cop,
                        int rows_used, const float* w_dense, int KH, int KW, int dy_min, int dx_min, int pad_mode,
                        int in_relu, const float* bias, int act, sdnStream stream);

/* The same head layers on the matrix cores (r05, csrc/conv_head.hip): 7 x 7 windows over Cip = 16 or 64 input channels,
 * rows_used <= 16 output channels in a 16-channel (padded) output tensor -- networks.py:236 (64 -> 3), :306 (16 -> 5) and the
 * stem's data gradient towards the encoder features.  v_mfma_f32_16x16x32_bf16, bf16 x 3 split products (fp32-class, not
 * bit-exact fp32 like sdn_conv_narrow_fwd), the input patch of an 8 x 32 output block staged once in LDS.
 * w_frag: [steps][2 (hi, lo)][64][8] bf16, steps = sdn_conv_head_steps: element (s, part, lane, j) = weight of output channel
 * lane % 16 at 8-channel slot u = 4 s + lane / 16 (tap = u / (Cip / 8) in window order ky * KW + kx, channels 8 (u % (Cip / 8)) + j),
 * zero for channels >= rows_used and slots behind the last tap.  Other arguments as sdn_conv_narrow_fwd.
 * r06 (ABI 7): `stats` (optional, [N, SDN_STAT_SLOTS, Cop, 2] fp64, zeroed by the caller) receives the InstanceNorm statistics of
 * bias + sum, as sdn_conv_gemm's epilogue files them -- the encoder's stem (networks.py:291-293: 3 -> 16 channels under
 * InstanceNorm) runs here; and Cop may be 64 over a 16-channel input (rows_used <= 64: the data gradient of the generator head
 * towards its 64 input channels, networks.py:236 backwards), w_frag then holds four row groups [4][steps][2][64][8]. */
int sdn_conv_head_steps(int Cip, int KH, int KW, int* steps);
int sdn_conv_head_mfma(const float* in, int N, int IH, int IW, int Cip, float* out, int QH, int QW, int Cop, int rows_used,
                       const void* w_frag, int KH, int KW, int dy_min, int dx_min, int pad_mode, int in_relu,
                       const float* bias, int act, double* stats, sdnStream stream);

/* InstanceNorm2d forward from the statistics the conv epilogue gathered (networks.py:27): first mr[n, c] = (mean, rstd)
 * ([N, Cp, 2] fp32, written here and kept for the backward pass) and the running_mean / running_var update torch does
 * in training mode (pointers may be NULL), then z <- (z - mean) * rstd in place (act 1: LeakyReLU(0.2) materialised);
 * out2 (optional) = z + f(res) (ResnetBlock, :281-283; f = ReLU when res_relu).  planes (optional, r04): bf16 (hi, lo)
 * operand planes (see sdn_split_planes) of what the tensor's consumers multiply -- out2 when there is one, else z --
 * through ReLU when planes_relu. */
int sdn_in_apply(float* z, const double* stats, float* mr, const float* res, float* out2, int N, int HW, int C, int Cp,
                 float eps, int act, int res_relu, float momentum, float* running_mean, float* running_var, void* planes,
                 long plane_stride, int planes_relu, sdnStream stream);
/* InstanceNorm2d (+ deferred ReLU / materialised LeakyReLU) backward, in place on g.  mode 0: stored = xhat; 1: stored =
 * xhat and consumers applied ReLU; 2: stored = LeakyReLU(xhat); | SDN_IN_BWD_SUMS_ZEROED (8): `sums` arrives zeroed (else the call
 * clears it with one fill launch).  mr from sdn_in_apply; sums: [N, Cp, 2] fp64 scratch.
 * planes (optional): the result also as bf16 operand planes (for sdn_conv_tile / sdn_conv_wgrad_tile). */
#define SDN_IN_BWD_SUMS_ZEROED 8
int sdn_in_bwd(float* g, const float* stored, const float* mr, double* sums, int N, int HW, int Cp, int mode, void* planes,
               long plane_stride, sdnStream stream);
/* layers without a norm: g <- g * act'(y) in place (act 0 none, 1 LeakyReLU, 2 tanh, 3 deferred ReLU) and
 * bias_grad[c] += sum g (optional, [Cp]).  planes (optional): the result also as bf16 operand planes. */
int sdn_act_bwd(float* g, const float* y, float* bias_grad, long npos, int Cp, int act, void* planes, long plane_stride,
                sdnStream stream);
/* adjoint of nn.ReflectionPad2d(pad): gp [N, H+2pad, W+2pad, Cp] -> out [N, H, W, Cp] (+= with accumulate). */
int sdn_reflect_fold(const float* gp, float* out, int N, int H, int W, int Cp, int pad, int accumulate, sdnStream stream);
/* Logical matrix Wm[r, k] = w[r*sr + c*sc + tapidx[t]] with k = t*Ccp + c -- or, when Ccp % 32 == 0 and Kp == ntaps*Ccp,
 * k = ((c/32)*ntaps + t)*32 + c%32 (channel-block-major: the taps of a 32-channel block are adjacent K steps of
 * sdn_conv_gemm, which applies the same rule to its gather) --, zero padded to [rows, Kp] (rows % 32 == 0, Kp % 32 == 0),
 * split into bf16 hi / lo and stored in MFMA fragment order: 2 * rows * Kp bf16 at
 *   packed[(((r/32) * (Kp/16) + k/16) * 2 + part) * 512 + (r%32 + 32*((k%16)/8)) * 8 + k%8],  part 0 = hi, 1 = lo.
 * tapidx is a DEVICE int32 array.  (sr, sc) select Conv2d [O,I,kh,kw] / ConvTranspose2d [I,O,kh,kw], forward /
 * data-gradient orientation.  Ccp % 8 == 0 (a thread packs eight columns of one row / tap; SDN_EINVAL otherwise). */
int sdn_conv_pack_weights(const float* w, int R, int C, long sr, long sc, const int32_t* tapidx, int ntaps, int Ccp,
                          int Kp, int rows, void* packed, sdnStream stream);
/* ---- r04: tiled MFMA kernels on bf16 operand PLANES (csrc/conv_tile.hip, conv_wtile.hip, conv_planes.hip).  Same layers,
 * same arithmetic (three bf16 products of split operands, fp32 accumulation) as sdn_conv_gemm / sdn_conv_wgrad, i.e. the
 * Conv2d / ConvTranspose2d forward, data gradient and weight gradient that /root/reference/textural/models/networks.py:211-283,
 * 412-461 leaves to cuDNN; the operands arrive pre-split and are copied to LDS by LDS-DMA.
 * A plane pair is [2][n] bf16: plane 0 = hi = bf16(x), plane 1 = lo = bf16(x - hi), `plane_stride` elements apart
 * (>= n, a multiple of 8).  relu != 0 splits max(x, 0) -- the deferred ReLU of the conv chains. */
int sdn_split_planes(const float* x, long n, int relu, void* planes, long plane_stride, sdnStream stream);
/* A chain's input: the NCHW fp32 tensors the caller would torch.cat along the channels (pix2pixHD_model.py:155-166, 199-210;
 * networks.py:238-239 then runs the first Conv2d on it) written side by side into ONE channels-last buffer out [N, H, W, Cp],
 * Cp >= sum(channels), pad channels zero.  parts / channels: HOST arrays of nparts (<= 8) device pointers / channel counts;
 * every part dense [N, channels[k], H, W].  Cp <= 128. */
int sdn_assemble_nhwc(const float* const* parts, const int32_t* channels, int nparts, int N, int H, int W, int Cp, float* out,
                      sdnStream stream);
/* K-major weights for sdn_conv_tile: packed[r][step][part][32] bf16 (part 0 = hi, 1 = lo), step = cb * ntaps + t over
 * 32-channel blocks cb and taps t, element = W[r, cb*32 + k%32, tap t]; rows >= R a multiple of 64, Ccp % 32 == 0;
 * 2 * rows * ntaps * Ccp bf16.  (sr, sc, tapidx) as sdn_conv_pack_weights. */
int sdn_conv_pack_weights_kmajor(const float* w, int R, int C, long sr, long sc, const int32_t* tapidx, int ntaps, int Ccp,
                                 int rows, void* packed, sdnStream stream);
/* sdn_conv_gemm's contract on planes: in_planes [2][N,IH,IW,Cip] (Cip % 32 == 0), out fp32 [N,OH,OW,Cop]; geometry, taps,
 * pad_mode, bias, act, stats, accumulate as sdn_conv_gemm.  out_planes (optional): the stored value, (ReLU'd when
 * planes_relu,) split, for the next layer.  w_rows >= Cop rounded up to the N tile (128 for Cop > 64, else 64).
 * ksplit > 1 (dense launches only: ostride 1, QH x QW = OH x OW, no act / stats / planes / accumulate): the LAST 256-position
 * tile of every image is computed as ksplit K slices by ksplit workgroups and summed with float atomics (summation order
 * not fixed) into rows the launcher zeroes -- for grids like the 26 x 80 data gradient of the residual layers, whose 32
 * leftover rows per image would otherwise cost a second round of the 256 CUs. */
int sdn_conv_tile(const void* in_planes, long plane_stride, int N, int IH, int IW, int Cip, float* out, void* out_planes,
                  long out_plane_stride, int planes_relu, int OH, int OW, int Cop, int QH, int QW, int istride, int ostride,
                  int py, int px, int ntaps, const int8_t* dy, const int8_t* dx, int pad_mode, const void* w_kmajor,
                  int w_rows, const float* bias, int act, double* stats, int accumulate, int ksplit, sdnStream stream);
/* Stride-1 convolutions with the input patch staged in LDS (csrc/conv_halo.hip): sdn_conv_tile's contract for launches with
 * istride = ostride = 1, py = px = 0, QH x QW = OH x OW whose taps fill a kh x kw window (kh * kw = ntaps >= 9) -- the 3x3
 * residual-block layers and the 4x4 stride-1 discriminator layers of textural/models/networks.py:244-283, 431-442, forward and
 * data gradient.  A workgroup owns a TH x TW block of output positions and copies the block's (TH + kh - 1) x (TW + kw - 1)
 * input patch once per 32-channel block instead of one activation tile per tap.  Needs Cop > 64 (128-channel N tiles).
 * sdn_conv_halo_blocks: the block shape the launcher picks and the grid size (blocks = 0: no block fits the window). */
int sdn_conv_halo_blocks(int N, int OH, int OW, int Cop, int kh, int kw, int* TH, int* TW, long* blocks);
int sdn_conv_halo(const void* in_planes, long plane_stride, int N, int IH, int IW, int Cip, float* out, int OH, int OW, int Cop,
                  int ntaps, const int8_t* dy, const int8_t* dx, int pad_mode, const void* w_kmajor, int w_rows,
                  const float* bias, int act, double* stats, int accumulate, sdnStream stream);
/* sdn_conv_wgrad's contract on planes: rows_planes [2][N*QH*QW, Cr], gath_planes [2][N,GH,GW,Cc] (ReLU already applied
 * where the fp32 entry point took relu_* flags); dw [Cr, ntaps*Cc] fp32 is ADDED to (zeroed by the caller): the work is
 * split stream-K style over one workgroup per CU and the parts of a tile meet in float atomics. */
int sdn_conv_wgrad_tile(const void* rows_planes, long rows_stride, const void* gath_planes, long gath_stride, float* dw,
                        int N, int QH, int QW, int Cr, int GH, int GW, int Cc, int istride, int ntaps, const int8_t* dy,
                        const int8_t* dx, int pad_mode, sdnStream stream);
/* grad_w[r*sr + c*sc + tapidx[t]] (+)= dw[r, t*Ccp + c]  (inverse of the packing map, for sdn_conv_wgrad's output).
 * accumulate 0: plain stores (a tap list covering the whole window defines every element: grad_w needs no zero fill).
 * Ccp % 4 == 0 and dw 16-byte aligned (16-byte loads of four columns of one row / tap; SDN_EINVAL otherwise). */
int sdn_conv_unpack_grad(const float* dw, int R, int C, long sr, long sc, const int32_t* tapidx, int ntaps, int Ccp,
                         float* grad_w, int accumulate, sdnStream stream);

/* ---- derender3d encoder: torchvision ResNet-18 behind geometric/derender3d/models/derenderer.py:25-27,48 ----------------------
 * Its convolutions are sdn_conv_gemm / sdn_conv_wgrad launches (bias-free 7x7 s2, 3x3 s1/s2, 1x1 s2); the entries below are
 * the rest of the network on channels-last fp32 tensors [rows = N*H*W, C] (C % 4 == 0; C <= 64 a power of two, else C % 64 == 0).
 *
 * nn.BatchNorm2d (+ the BasicBlock tail `relu(bn(x) + identity)`):  out = f((x - mean) * scale + beta + res), f = ReLU when
 * relu, scale = gamma * rstd (evaluated centred, as torch does; shift = beta - mean * scale is only reported in ss).
 * training: batch mean / biased variance over the rows (sums: [C,2] fp64
 * scratch), running_mean / running_var (may be NULL) updated with momentum and the unbiased variance; eval: the running
 * statistics.  mr [C,2] = (mean, rstd) and ss [C,2] = (scale, shift) are written for the backward pass.  res may be NULL. */
int sdn_bn_forward(const float* x, long rows, int C, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps, int training, const float* res, int relu, float* out,
                   float* mr, float* ss, double* sums, sdnStream stream);
/* Backward of the above.  gm [rows,C] <- g masked by the ReLU (out > 0): also the gradient of `res`.  dx <- gradient wrt x.
 * sums [C,2] fp64 <- (sum gm, sum gm * xhat) = (d beta, d gamma). */
int sdn_bn_backward(const float* g, const float* out, const float* x, const float* mr, const float* gamma, long rows, int C,
                    int training, int relu, float* gm, float* dx, double* sums, sdnStream stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of torchvision's ResNet stem on [N,H,W,C]; idx [N,OH,OW,C] int8 = window
 * tap of the first maximum, OH = (H - 1) / 2 + 1.  The backward pass gathers (deterministic, no atomics). */
int sdn_maxpool3x3s2_fwd(const float* x, int N, int H, int W, int C, float* out, int8_t* idx, sdnStream stream);
int sdn_maxpool3x3s2_bwd(const float* g, const int8_t* idx, int N, int H, int W, int C, float* gin, sdnStream stream);
/* nn.AdaptiveAvgPool2d(1) (derenderer.py:26): forward x [N,HW,C] -> out [N,C]; backward (flag) x = g [N,C] -> out [N,HW,C]. */
int sdn_avgpool_global(const float* x, int N, int HW, int C, float* out, int backward, sdnStream stream);

/* Instance-wise average pooling of the Encoder (networks.py:310-325): x [N, C, HW] fp32 (NCHW), seg [N, HW] int32 dense
 * segment ids in [0, K) (ids are unique across the batch, as after networks.py:313-316).  sums [C, K] and counts [K] are
 * caller-owned scratch that is also the result table (sums[c, k] / counts[k] = mean feature of segment k, what
 * generate_feat_dict reports, :327-346); out [N, C, HW] = the mean of each pixel's segment.  The backward pass is the
 * same call on the incoming gradient.  With K <= 4096 and K <= HW the sums are added in a fixed order (the same input
 * gives the same bits on every call); `out` then serves as scratch for the partial sums before it is written and must not
 * alias x.  Larger tables are summed with float atomics, in arrival order. */
int sdn_segment_mean(const float* x, const int32_t* seg, int N, int C, int HW, int K, float* sums, float* counts,
                     float* out, sdnStream stream);

/* nn.AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False): the input pyramid of MultiscaleDiscriminator
 * (networks.py:392, 406) and LocalEnhancer (:190).  in [N,C,H,W] / out [N,C,OH,OW] (OH = (H-1)/2+1) addressed through HOST
 * arrays of 4 element strides (n, c, h, w), so NCHW tensors and channels-last views need no copy; inner_c: threads run channel
 * fastest (channels-last storage).  _bwd: g [N,C,OH,OW] -> gin [N,C,H,W] (H, W = the INPUT size), gather form, no atomics. */
int sdn_avgpool3x3s2_fwd(const float* in, int N, int C, int H, int W, const long* in_strides, float* out,
                         const long* out_strides, int inner_c, sdnStream stream);
int sdn_avgpool3x3s2_bwd(const float* g, int N, int C, int H, int W, const long* g_strides, float* gin,
                         const long* gin_strides, int inner_c, sdnStream stream);

/* torch.nn.L1Loss() between two fp32 tensors of the same dense memory layout, flattened to n elements: `criterionFeat`
 * of the textural model (textural/models/pix2pixHD_model.py:86; discriminator feature matching :213-221, image
 * reconstruction).  fwd: out[0] = mean |a - b| (sum: one fp64 of device scratch).  bwd: grad_a = sgn(a - b) *
 * grad_out[0] / n, grad_b = -grad_a; either may be null.  All pointers are device pointers, 16-byte aligned. */
int sdn_l1_loss_fwd(const float* a, const float* b, long n, double* sum, float* out, sdnStream stream);
int sdn_l1_loss_bwd(const float* a, const float* b, long n, const float* grad_out, float* grad_a, float* grad_b,
                    sdnStream stream);
/* The loss of the test-time optimisation loop, geometric/scripts/main.py:445-451:
 *     loss = mean( mse_loss(masks, target, reduce=False) [* (1 - ignore)] + 100 * mean(ffd ** 2) )
 * fused: forward = one partial sum per block + one finishing wave that adds them in block order and writes out[0] (no
 * atomics: the same bits every run); backward = d loss / d masks and d loss / d ffd (either may be NULL) in one launch,
 * scaled by grad_out[0].  sums: SDN_SIL_LOSS_SUMS doubles of device scratch, no initialisation needed, kept for the
 * backward call (which reads the first three).  n = elements of masks / target / ignore (ignore may be NULL), nffd =
 * elements of ffd. */
#define SDN_SIL_LOSS_BLOCKS 512
#define SDN_SIL_LOSS_SUMS (3 + 3 * SDN_SIL_LOSS_BLOCKS)
int sdn_silhouette_loss_fwd(const float* masks, const float* target, const float* ignore, long n, const float* ffd, long nffd,
                            double* sums, float* out, sdnStream stream);
int sdn_silhouette_loss_bwd(const float* masks, const float* target, const float* ignore, long n, const float* ffd, long nffd,
                            const double* sums, const float* grad_out, float* grad_masks, float* grad_ffd, sdnStream stream);
/* The loss dict of a training step of the geometric branch, geometric/scripts/main.py:114-154 (BaseNet.step_batch with
 * BaseNet.partial, :97-112, and Transforms.pad_like, derender3d/datasets.py:29-33), which the reference writes as torch
 * expressions: per loss a torch.nonzero + numel() branch and an isnan().any() branch (two host waits each, six losses), two
 * padded copies of the batch's masks / ignore maps at the render size and about a dozen element-wise launches each way.
 * Here `targets` is data: B items, rendered masks R x R, target masks / ignore maps S x S, p = (R - S) / 2 (R - S even and
 * >= 0, else SDN_EINVAL: pad_like pads (R - S) // 2 on both sides and an odd difference does not line up).
 *   sel_g = targets & 1 (TargetType.geometry), n_g items;  sel_r = targets & 2 (TargetType.reproject), n_r items
 *   mode & 1:  out[0] theta_delta_loss   = mean over sel_g x 2 of (_theta_deltas - (cos thetas, sin thetas))^2  (cos / sin in
 *                                          double, rounded once to fp32)
 *              out[1] translation2d_loss, out[2] scale_loss, out[3] depth_loss: mean over sel_g x (2, 3, 1) of (pred - batch)^2
 *              n_g = 0: exactly 0, no gradient (the torch.tensor(0.0) branch of `partial`)
 *   mode & 2:  m_i = mask_weight / R^2 * sum_{y,x} (1 - ignores_i[clamp(y - p), clamp(x - p)]) (_masks_i[y, x] - masks_i[y - p, x - p])^2
 *              with masks = 0 outside [0, S)^2 (pad_like 'constant') and the ignore index clamped to [0, S - 1] ('replicate');
 *              the padding is index arithmetic, no copy is made
 *              out[4] class_reward = mean over sel_r of _class_log_probs_i * m_i   (m_i detached: gradient to the log-probs only)
 *              out[5] mask_loss    = mean over sel_r of m_i;   n_r = 0: both exactly 0, no gradient
 *              out[6] ffd_coeff_reg = ffd_coeff_reg * mean(_ffd_coeffs^2) over ALL items (the reference does not mask it)
 *   the slots of a group `mode` does not ask for are 0 and its pointers may be NULL.  Items outside sel_r are not read.
 * fwd: one launch of per-block fp64 partial sums (grid: item x chunk of rows; 16-byte loads of _masks when R % 4 == 0, of masks /
 * ignores when S % 4 == 0 and p % 4 == 0 too, and the pointers allow; scalar loads otherwise) -- skipped when mode lacks
 * reproject -- and one finishing wave that adds them in block order: no atomics, no memset, the same bits every run.
 * bwd: ONE launch from grad_out[7] (DEVICE):
 *   grad_masks[i,y,x] = grad_out[5] [i in sel_r] mask_weight 2 (1 - ign) (_masks - masks) / (n_r R^2), zeros elsewhere
 *   grad_class_log_probs[i] = grad_out[4] [i in sel_r] m_i / n_r;   grad_ffd = grad_out[6] 2 ffd_coeff_reg ffd / nffd
 *   the four head gradients grad_out[k] 2 (pred - target) / (cols n_g) on the rows of sel_g, zeros elsewhere
 * any grad_* may be NULL (not wanted); every element of a non-NULL one is written.
 * scratch: DEVICE, sdn_train_losses_scratch(B, R, nffd) bytes aligned to 8, no initialisation needed, kept between the fwd
 * call and its bwd call (n_g, n_r, m_i live there).  All tensors fp32 DEVICE arrays, dense; targets int64 [B].
 * _theta_deltas / _translation2ds / translation2ds [B,2], _log_scales / log_scales [B,3], _log_depths / log_depths / thetas
 * [B,1], _class_log_probs [B], _masks [B,1,R,R], masks / ignores [B,1,S,S], _ffd_coeffs nffd elements. */
int sdn_train_losses_scratch(int B, int R, long nffd, size_t* bytes);
int sdn_train_losses_fwd(const float* p_theta_deltas, const float* p_translation2ds, const float* p_log_scales,
                         const float* p_log_depths, const float* p_class_log_probs, const float* p_masks, const float* p_ffd,
                         long nffd, const float* thetas, const float* translation2ds, const float* log_scales,
                         const float* log_depths, const float* masks, const float* ignores, const int64_t* targets, int B, int R,
                         int S, int mode, double mask_weight, double ffd_coeff_reg, void* scratch, float* out, sdnStream stream);
int sdn_train_losses_bwd(const float* p_theta_deltas, const float* p_translation2ds, const float* p_log_scales,
                         const float* p_log_depths, const float* p_masks, const float* p_ffd, long nffd, const float* thetas,
                         const float* translation2ds, const float* log_scales, const float* log_depths, const float* masks,
                         const float* ignores, const int64_t* targets, int B, int R, int S, int mode, double mask_weight,
                         double ffd_coeff_reg, const void* scratch, const float* grad_out, float* grad_theta_deltas,
                         float* grad_translation2ds, float* grad_log_scales, float* grad_log_depths, float* grad_class_log_probs,
                         float* grad_masks, float* grad_ffd, sdnStream stream);
/* Pose parameters of a frame's objects, derender3d/models/__init__.py:106-116: quat[n,4] = (cos(theta/2), 0, sin(theta/2), 0),
 * scales[n,3] = exp(log_scales); and the adjoint (g_quat / g_scales may be NULL = no gradient arrived). */
int sdn_pose_params(const float* theta, const float* log_scales, int n, float* quat, float* scales, sdnStream stream);
/* The whole pose algebra of Derenderer3d.render, derender3d/models/__init__.py:95-158, for a frame's n objects in one launch
 * each way (the reference: ~45 element-wise torch ops forward, as many autograd nodes backward):
 *   thetas = atan2(delta_1, delta_0);  rotations = (cos t/2, 0, sin t/2, 0);  scales = exp(log_scales);
 *   depths = sqrt(exp(log_depths) / (extent_0 extent_1));  center2ds = centre + translation2ds * extent;
 *   translations = depths * ray(center2ds), ray(row, col) = (col, -row, -1) / |.|;
 *   alphas = remainder(-(thetas - atan(t_x / t_z)) + pi, 2 pi) - pi;
 *   training != 0 (crop-centred camera, :139-150): persp = depths * ray(centre), zooms = (image_size / focals) / max(extent);
 *   else (object-centred, :152-153): persp = translations, zooms = render_size / (2 focals)  (the `zoom_tos`).
 * centre / extent / theta_deltas / translation2ds / center2ds [n,2], focals / log_depths / thetas / alphas / depths / zooms [n],
 * log_scales / scales / translations / persp [n,3], rotations [n,4]; all fp32 device arrays.  _bwd: any g_* input may be NULL
 * (no gradient arrived), any g_* output may be NULL (not wanted); zooms depend on no differentiable input. */
int sdn_pose_algebra(const float* centre, const float* extent, const float* focals, const float* theta_deltas,
                     const float* log_scales, const float* log_depths, const float* translation2ds, int n, int training,
                     float image_size, float render_size, float* thetas, float* alphas, float* rotations, float* scales,
                     float* depths, float* center2ds, float* translations, float* persp, float* zooms, sdnStream stream);
int sdn_pose_algebra_bwd(const float* centre, const float* extent, const float* theta_deltas, const float* thetas,
                         const float* scales, const float* depths, const float* center2ds, const float* translations, int n,
                         int training, const float* g_thetas, const float* g_alphas, const float* g_rotations,
                         const float* g_scales, const float* g_depths, const float* g_center2ds, const float* g_translations,
                         const float* g_persp, float* g_theta_deltas, float* g_log_scales, float* g_log_depths,
                         float* g_translation2ds, sdnStream stream);
int sdn_pose_params_bwd(const float* theta, const float* scales, const float* g_quat, const float* g_scales, int n,
                        float* g_theta, float* g_log_scales, sdnStream stream);

/* ---- per-frame compositing of the rendered objects: geometric/scripts/main.py:541-602 ---------------------------------------
 * masks [n,R,R], normals [n,3,R,R], depth_maps [n,R,R], zooms [n] (device).  objs: DEVICE int32 [m,7] rows
 * (object index, paste size, left, top, first row of its `bounds` table, first element of its coefficient tables, ksize)
 * in painter's order (far first); bounds [.,2] = (first source index, count) per output index, kk8 = Pillow's 22-bit
 * fixed-point bilinear weights, kkf = the same weights as doubles (Resample.c precompute_coeffs / normalize_coeffs_8bpc,
 * prepared by derender3d/compositing.py).  inst [H,W], nrm [3,H,W], dep [H,W] are updated where an object covers the
 * pixel (the caller initialises them to 0 / 0.5 / 1 as main.py:545-547 does).  Bit-identical to the PIL path. */
int sdn_composite_frame(const float* masks, const float* normals, const float* depth_maps, const float* zooms, int n,
                        int R, const int32_t* objs, int m, const int32_t* bounds, const int32_t* kk8, const double* kkf,
                        int H, int W, float* inst, float* nrm, float* dep, sdnStream stream);

/* ---- textural inputs of F edited frames in one launch: textural/edit_vkitti.py:62-103, edit_benchmark.py:87-126 ------------
 * base_segm [1 | F, HW] fp32: the SOURCE frame's label map as the loader leaves it with both *_precomputed_path options
 * (+1 applied, car pixels without an instance already "misc": edit_vkitti.py:50-53); base_stride 0 shares one source among
 * the F frames (edit_vkitti), HW gives each frame its own (edit_benchmark).  edit_inst [F, HW] uint8: the raw object ids of
 * NNNNN.png.  obj_label / obj_pose [F, 256] int32: per-frame tables indexed by raw object id, built by the caller from
 * NNNNN.json -- label {1: 2, 2: 12}[class_id] (0 = id not in the JSON), pose np.digitize(alpha / pi, bins).
 * Per pixel, with s = base label (2 / 12 -> 5) and k = raw id:  k in the JSON: segm = obj_label[k], inst = 1000 k,
 * pose = obj_pose[k];  otherwise segm = s, inst = (k == 0 ? s : k), pose = 0.  (Raw ids are <= 255 < 1000, so the
 * reference's sequential in-place rewrites never alias and this table form is exact.)
 * feat[f, c, p] = codes[c, row], row = position of the pixel's final instance id in code_ids (int32 [K], ascending -- the
 * unique ids of the source's instance map) and codes [C, K] the source's mean feature per id (sdn_segment_mean's table).
 * An id without a code paints 0 in all C channels and counts the pixel in missing[f] (int32 [F], cleared by the call).
 * pose_channels: 1 (binned pose) or 2 (feat_pose_num_bins == 0: the reference allocates two channels and writes neither,
 * so both are zero).  Outputs are dense fp32: segm_out, inst_out [F, 1, HW], pose_out [F, pose_channels, HW],
 * feat_out [F, C, HW].  Kpad + C K <= 12288 (Kpad = K rounded up to a power of two): the tables live in LDS. */
int sdn_edit_assemble(const float* base_segm, long base_stride, const uint8_t* edit_inst, const int32_t* obj_label,
                      const int32_t* obj_pose, const int32_t* code_ids, const float* codes, int K, int C, int F, int HW,
                      int pose_channels, float* segm_out, float* inst_out, float* pose_out, float* feat_out,
                      int32_t* missing, sdnStream stream);

/* ---- the geometric branch's inputs from a frame and the detector's output: geometric/scripts/main.py:365-373, 405-421 with
 * derender3d/datasets.py:49-71 (Transforms.crop_square) and :141-172 (BaseDataset.transform_rgb / _mask / _ignore) ----------
 * The reference crops, resizes (PIL bilinear) and converts on the host, three PIL round trips per object.  Three entries:
 *
 * sdn_scene_cover: masks [N, H W] fp32, BINARY (exactly 0 or 1: what Mask R-CNN delivers; checked only when the environment
 * holds SDN_DEBUG_CHECKS=1, which makes the call synchronous) -> cover uint32 [ceil(N / 32), H W]: bit (n & 31) of word
 * n / 32 is set where object n's mask is.  Also used for caller-supplied ignore maps (main.py:416). */
int sdn_scene_cover(const float* masks, int N, int H, int W, uint32_t* cover, sdnStream stream);
/* sdn_scene_crops: one launch for all N objects.  kinds: 1 image crops, 2 mask crops, 4 ignore crops (any sum).
 *   rgbs    [N, 3, image_size, image_size]  from frame uint8 [3, H, W], outside the frame 127,
 *           value ((u8 / 255) - mean[c]) / std[c] in three fp32 operations (to_tensor, Normalize)
 *   masks   [N, 1, mask_size, mask_size]    from bit n of `cover`, outside 0, value u8 / 255
 *   ignores [N, 1, mask_size, mask_size]    slot n = ((ignore_cover & nearer[n]) != 0) * 255, outside 255, value u8 / 255;
 *           nearer int64 [N, ceil(N / 32)] (low 32 bits used): the objects whose union is slot n's map (main.py:407-414:
 *           those sorted before position n), or bit n alone when ignore_cover holds caller-supplied maps
 * Per object exactly crop_square -> PIL resize -> to_tensor: the window of side s = max(h, w) at
 * (roi[0] - (s - h) / 2, roi[1] - (s - w) / 2); crop_square pads right / bottom by max(0, roi end + d - size) only, so when
 * s - w (s - h) is odd the window's last column (row) lies beyond the padded image and PIL's crop makes it 0 -- reproduced.
 * rois_host: HOST int32 [N, 4] = (y0, x0, y1, x1), read before the launch for validation (an empty roi, or a window whose
 * filter does not fit the 32 KiB row tile, is SDN_EINVAL).  objs: DEVICE int32 [N, 12] rows (window y, x, s, x limit, y limit
 * of the padded image, then for image_size and for mask_size: first row of `bounds`, first element of `kk8`, ksize -- 0 when
 * s equals the output size and Pillow skips the resampling -- and one unused int); bounds / kk8 as for sdn_composite_frame. */
int sdn_scene_crops(const uint8_t* frame, const uint32_t* cover, const uint32_t* ignore_cover, const int64_t* nearer,
                    const int32_t* rois_host, const int32_t* objs, const int32_t* bounds, const int32_t* kk8, int N, int H, int W,
                    int image_size, int mask_size, int kinds, float mean0, float mean1, float mean2, float std0, float std1,
                    float std2, float* rgbs, float* masks, float* ignores, sdnStream stream);
/* ---- F edit lists applied to one de-rendered scene: geometric/scripts/main.py:481-514 ------------------------------------------
 * theta_deltas, translation2ds, mroi_norms, droi_norms [N, 2], log_depths [N, 1], interests uint8 [N].  records: DEVICE int32
 * [F, P, 8] rows (object index or -1 for an unused slot, type 0 delete / 1 modify, then as float bits: new centre row, column,
 * 2 log(zoom), cos(-ry), sin(-ry); one unused int), in the reference's iteration order.  Outputs [F, N, ...]: copies, and per
 * record  translation2d = (centre - mroi) / droi,  log_depth -= 2 log zoom,  theta_delta = (c cos - s sin, s cos + c sin);
 * delete clears interests_out[f, n].  A later record of the same object reads what the earlier one left. */
int sdn_scene_edit(const float* theta_deltas, const float* translation2ds, const float* log_depths, const float* mroi_norms,
                   const float* droi_norms, const uint8_t* interests, const int32_t* records, int F, int N, int P,
                   float* theta_out, float* translation_out, float* log_depth_out, uint8_t* interests_out, sdnStream stream);

/* ---- the detector's output as binary full-frame masks: geometric/maskrcnn/model.py:1638-1653 (detect's tail), :2084-2143
 * (MaskRCNN.unmold_detections), maskrcnn/utils.py:378-395 (unmold_mask) and geometric/scripts/main.py:797-818 -------------------
 * The reference copies mrcnn_mask to the host, runs scipy.misc.imresize(.., 'bilinear') per detection, thresholds, pastes into
 * uint8 planes, sums each plane to pick the 16 largest and uploads the survivors as float32.  sdn_unmold_masks does, for n
 * objects in one launch and bit for bit, per object:
 *   1. bytescale of plane (det, cls) of mrcnn_mask [D, C, Mh, Mw] (scipy 1.0.1 misc/pilutil.py under numpy 1.14: fp32 array
 *      arithmetic): cmin / cmax over the plane, cscale = cmax - cmin (0 -> 1), scale = (float)(255.0 / (double)cscale),
 *      byte = (uint8)(clip((x - cmin) * scale + 0, 0, 255) + 0.5) -- so the threshold below is relative to the plane's range;
 *   2. Pillow's BILINEAR resize of the bytes to (y2 - y1, x2 - x1): horizontal pass rounded to uint8, then the vertical pass;
 *   3. (float)v / 255 >= 0.5, i.e. v >= 128;
 *   4. paste at [y1:y2, x1:x2].
 * masks [n, 1, H, W] fp32 (may be NULL) receives exactly 0.0 / 1.0, every element written (no memset needed); areas [n] int32
 * (may be NULL, not both) the number of ones (cleared by the call).  With masks NULL only the areas are made.
 * objs: DEVICE int32 [n, 12] rows (detection index, class id, y1, x1, y2, x2, then for the rows Mh -> y2 - y1 and for the
 * columns Mw -> x2 - x1: first row of `bounds`, first element of `kk8`, ksize -- 0 when the sizes are equal and Pillow skips
 * the pass); objs_host: the same table on the HOST, validated before the launch (a box that is empty or leaves the frame, an
 * index outside mrcnn_mask, a table outside the n_bounds rows of `bounds` / n_kk8 elements of `kk8` is SDN_EINVAL).  bounds /
 * kk8 as for sdn_composite_frame.  Mh, Mw <= 64. */
int sdn_unmold_masks(const float* mrcnn_mask, int D, int C, int Mh, int Mw, const int32_t* objs_host, const int32_t* objs, int n,
                     const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8, int H, int W, float* masks,
                     int32_t* areas, sdnStream stream);
/* ---- the same inputs from ground truth (--source gt): geometric/scripts/main.py:724-795 with derender3d/datasets.py:75-76
 * (Transforms.scene_to_mask) and :95-103 (mask_to_roi), which run per object on the host -----------------------------------------
 * scene uint8 [H, W, 3], codes uint8 [K, 3] (both DEVICE) -> masks [K, 1, H, W] fp32 = all(scene == code, axis 2),
 * rois int32 [K, 4] = (first row, first column, last row + 1, last column + 1) of each mask, areas int32 [K].  A code that
 * matches no pixel leaves area 0 and the roi (INT_MAX, INT_MAX, 0, 0): mask_to_roi raises there, and so must the caller. */
int sdn_scene_gt_masks(const uint8_t* scene, const uint8_t* codes, int K, int H, int W, float* masks, int32_t* rois,
                       int32_t* areas, sdnStream stream);

/* ---- the same inputs from Cityscapes ground truth (--dataset cityscapes --source gt): geometric/scripts/main.py:763-795, 812-818
 * and the same statements in derender3d/datasets.py:930-971, with Transforms.mask_to_roi (datasets.py:95-103) ------------------
 * The reference runs np.unique over the instance-id map (id = category * 1000 + k), keeps the ids with id // 1000 == 26 and, per
 * object on the host, gathers the disparities under the mask, drops the zeros, takes np.percentile(., 95) of the rest (0 if
 * nothing is left) and compares the whole disparity frame with it: the object's ignore map.
 *
 * sdn_scene_id_stats: scene, disparity DEVICE int32 [H, W]; the disparities lie in 0 .. 65535 (16-bit PNGs; checked only when
 * the environment holds SDN_DEBUG_CHECKS=1, which makes the call synchronous; SDN_EINVAL otherwise).  table: DEVICE int32
 * [1000, 8], row j = id - 1000 category: (area, y0, x0, y1, x1, n, lo, hi) -- the pixel count and the roi of mask_to_roi (first
 * row, first column, last row + 1, last column + 1); n = the pixels under the mask whose disparity is not 0; lo, hi = those n
 * values' order statistics of rank i = (19 (n - 1)) / 20 (= floor((n - 1) 0.95)) and min(i + 1, n - 1), zero-based, ascending,
 * both 0 when n == 0: the two values np.percentile's `linear` method interpolates between.  The row of an absent id holds
 * area 0 and the invalid roi (INT_MAX, INT_MAX, 0, 0) of sdn_scene_gt_masks.  An id equal to the bare category is not
 * category * 1000 + k and is ignored (26 // 1000 == 0 in the reference).  An exact two-level radix select, five launches on
 * `stream`, integer atomics only (the result does not depend on scheduling), nothing copied to the host.  workspace: DEVICE,
 * sdn_scene_id_workspace_bytes (3 088 000: histograms of the high byte [1000, 256], select records [1000, 4], histograms of
 * the low byte [1000, 2, 256], int32), aligned to 16 bytes; the call clears it and the table.
 *
 * sdn_scene_id_planes: the outputs of n selected objects in one launch.  ids, thr: DEVICE int32 [n], the full instance ids and
 * the thresholds floor(np.percentile(.., 95)) (the disparities are integers: d > t is d > floor(t)), computed on the HOST from
 * (n, lo, hi) in float64 as numpy does (derender3d.scene.percentile95_threshold).  masks [n, 1, H, W] fp32 (may be NULL): 1.0
 * where scene == ids[k], else 0.0.  ignore_cover uint32 [ceil(n / 32), H W] (may be NULL, not both): bit (k & 31) of word
 * k / 32 is set where disparity > thr[k] -- the layout of sdn_scene_cover.  ignores [n, 1, H, W] fp32 (may be NULL): the same
 * predicate as planes (the reference's image_ignores).  Every element is written (no memset needed), one writer per word. */
int sdn_scene_id_workspace_bytes(size_t* out);
int sdn_scene_id_stats(const int32_t* scene, const int32_t* disparity, int category, int H, int W, int32_t* table,
                       void* workspace, sdnStream stream);
int sdn_scene_id_planes(const int32_t* scene, const int32_t* disparity, const int32_t* ids, const int32_t* thr, int n, int H, int W,
                        float* masks, uint32_t* ignore_cover, float* ignores, sdnStream stream);

/* ---- the textural loader's item on the device, batched: textural/data/base_dataset.py:41-104 (get_transform, __scale_width,
 * __crop, __make_power_2, __flip) with vkitti_dataset.py:44-129 and cityscapes_dataset.py:32-111, which run per item with PIL
 * and numpy on the host ----------------------------------------------------------------------------------------------------
 * All B items of a call share the source size [H, W], the options and so the scaled size [sh, sw] (the one resize of the mode:
 * Scale, __scale_width or __make_power_2) and the output size [h, w]; items_host / items: the same int32 [B, 4] rows (crop x1,
 * y1, flip 0 / 1, unused) on the HOST (validated: x1, y1 >= 0) and on the DEVICE.  An output pixel (y, x) is the scaled image's
 * pixel (y1 + y, x1 + (flip ? w - 1 - x : x)), 0 where that lies beyond [sh, sw] (PIL's crop).  Only the window is computed.
 * The per-item map addresses are DEVICE int64 [B] tables, so that one host-to-device copy carries every table of a call.
 *
 * sdn_assemble_planes (base_dataset.py:41-66 for the image and the normal map; vkitti_dataset.py:63-66, 121-127,
 * cityscapes_dataset.py:48-52, 95-100): src[b] = address of a DEVICE uint8 [C, H, W] map, 0 = the map is absent and the item's
 * planes are 0.0.  Pillow's ImagingResample, bit for bit: xmin [sw] / xk [sw, xks] and ymin [sh] / yk [sh, yks] are
 * precompute_coeffs' first source index and normalize_coeffs_8bpc's 22-bit weights (0 beyond a window) per scaled column / row;
 * xks == 0 exactly when sw == W (no horizontal pass), yks == 0 exactly when sh == H.  Then lut [256] (ToTensor: float32(k) / 255
 * computed on the host), (v - mean) / std when normalize, + add when bias (the normal branch's 1 / 255).  out fp32
 * [B, C, h, w].  SDN_EINVAL when yks source rows of w bytes do not fit the 32 KiB LDS tile.  One launch.
 *
 * sdn_assemble_maps (NEAREST: vkitti_dataset.py:52-57, 68-118, cityscapes_dataset.py:41-42, 55-93, 102-105): segm[b], inst[b],
 * pose[b] = addresses of DEVICE uint8 [H, W] maps (inst[b] int32 [H, W] when inst_mode is 3); inst[b] == 0: the loader's
 * FileNotFoundError branch, inst = label (inst_mode 3, whose output is an integer tensor: the item's inst is 0; mix nothing
 * there); pose[b] == 0: "no cars", the pose plane is 0.  nx [sw] / ny [sh]: ImagingScaleAffine's source index per scaled
 * column / row, NULL exactly when the size does not change.  inst_nx [sw] / inst_ny [sh] (each may be NULL: nx / ny; non-NULL
 * only where that size changes, inst_mode 3 only): the same for an instance map whose image mode Pillow resizes by its generic
 * transform (mode 'I;16': int(a (x + 0.5)) on every axis that changes, instead of the running sum).  tabs fp32 [4, 256] by raw
 * value: the label of a segm value, the label where the instance value is 0 (inst_mode 2; vkitti_dataset.py:75-78), the value that fills such an
 * instance, the instance value of an inst byte.  inst_mode: 0 no instance output (inst, inst_out may be NULL), 1 inst =
 * tabs[3][i], 2 the same with zeros filled, 3 the int32 map handed through; inst_out [B, 1, h, w] fp32, for mode 3 int32, or
 * int16 when wrap16 (torchvision's ToTensor reads a mode 'I;16' image through np.int16).  label fp32 [B, 1, h, w].
 * The pose plane (pose_out non-NULL; else pose, pose_has, pose_val, counts may be NULL): counts DEVICE int32 [B, 256] receives
 * the number of transformed pixels per raw pose id (integer atomics, aggregated per workgroup in LDS); a second launch paints
 * pose_out [B, pose_channels, h, w] 32-bit words = pose_val [B, 256, pose_channels] (int32 bins, or the bits of fp32 cos, sin) of
 * every id != 0 whose count is >= min_area (cityscapes_dataset.py:82: 256; vkitti: 1) and pose_has [B, 256] is set; the pixels
 * of such an id without a record are painted 0 and counted in missing int32 [B] (the reference raises KeyError there).
 * The call clears counts and missing itself; nothing is copied to the host. */
int sdn_assemble_planes(const int64_t* src, const int32_t* items_host, const int32_t* items, const int32_t* xmin,
                        const int32_t* xk, int xks, const int32_t* ymin, const int32_t* yk, int yks, const float* lut, int B, int C,
                        int H, int W, int sh, int sw, int h, int w, int normalize, float mean, float std, int bias, float add,
                        float* out, sdnStream stream);
int sdn_assemble_maps(const int64_t* segm, const int64_t* inst, const int64_t* pose, const int32_t* items_host,
                      const int32_t* items, const int32_t* nx, const int32_t* ny, const int32_t* inst_nx, const int32_t* inst_ny,
                      const float* tabs, int inst_mode, int wrap16, int B, int H, int W, int sh, int sw, int h, int w, float* label, void* inst_out, const int32_t* pose_has,
                      const void* pose_val, int pose_channels, int min_area, void* pose_out, int32_t* counts, int32_t* missing,
                      sdnStream stream);

/* ---- the training items of the geometric branch, batched over several frames: geometric/derender3d/datasets.py:332-420
 * (VKitti.__getitem__), :37-46 (roi_jitter), :141-172 (transform_rgb / _mask / _ignore with Transforms.color_jitter) and
 * data_loader.py:17-37 (collate_fn), which run per object with numpy and PIL on the host ----------------------------------------
 * sdn_train_rois (datasets.py:345-347): scenes DEVICE uint8 [Fr, H, W, 3], items DEVICE int32 [B, 4] rows (frame index, r, g, b)
 * -> table DEVICE int32 [B, 5] rows (y0, x0, y1, x1, area) of all(scenes[frame] == code, axis 2): mask_to_roi's box (last index
 * + 1) and the pixel count.  A code that matches no pixel, or a frame index outside [0, Fr), leaves the empty row of
 * sdn_scene_gt_masks, (INT_MAX, INT_MAX, 0, 0) with area 0.  Several items may name one frame.  The call clears the table;
 * integer atomics only (the result does not depend on scheduling); nothing is copied to the host.
 *
 * sdn_train_crops (datasets.py:141-172, 390-391, 415-417): for B items in one launch, after a statistics launch when an item's
 * jitter holds contrast,
 *   images  [B, 3, image_size, image_size]  from frames uint8 [Fr, 3, H, W], outside the frame 127; the item's colour jitter on
 *           every pixel of the s x s window (fill and quirk pixels included, as PIL sees them) BEFORE the resize; then
 *           ((u8 / 255) - mean[c]) / std[c] in three fp32 operations
 *   masks   [B, 1, mask_size, mask_size]    scenes[frame] == the item's code, outside 0, value u8 / 255
 *   ignores [B, 1, mask_size, mask_size]    count = the number of the item's nearer codes equal to the scene pixel (a code listed
 *           twice counts twice), byte (255 count) & 255 as np.uint8(255 * count) wraps, outside 255, value u8 / 255
 * with the window, the padding quirk and Pillow's resize of sdn_scene_crops, bit for bit; objs / objs_host: its object table
 * [B, 12] on the DEVICE and on the HOST, rois_host HOST int32 [B, 4].  items / items_host: DEVICE and HOST int32 [B, 12] rows
 * (frame index; code r | g << 8 | b << 16; first row and number of rows of the item's codes in `nearer`; number of ops 0 .. 4;
 * the ops in order, 4 bits each from bit 0: 0 brightness, 1 contrast, 2 saturation, 3 hue, each at most once; the brightness,
 * contrast and saturation factors as fp32 bits; the hue shift 0 .. 255; two unused ints).  nearer: DEVICE uint8 [n_nearer, 3].
 * The ops are Pillow's as torchvision 0.2.1 applies drawn parameters: ImageEnhance.Brightness (Image.blend with black),
 * .Contrast (blend with the solid grey int(mean(L) + 0.5) of the window as it is at that point of the order; the sum of L by
 * 64-bit integer atomics in the statistics launch, the mean as (2 sum + n) / (2 n) in integers), .Color (blend with
 * convert('L')), and convert('HSV'), H + shift modulo 256, convert('RGB').  No ops: exactly sdn_scene_crops' outputs.
 * workspace: DEVICE, 8 B bytes aligned to 8 (the sums; when an item holds contrast the call clears it with one
 * hipMemsetAsync on `stream` in front of the statistics launch).  The kernels clamp what they read out of `bounds` (first
 * indices, tap counts, row runs); the rows of objs / items themselves are trusted as in sdn_scene_crops: only their HOST
 * copies are validated, and a DEVICE table that differs from them reads out of bounds.  Validated on the host before any launch,
 * SDN_EINVAL: an empty roi; a window table that is not crop_square's of the roi; a window wider than 4096 pixels (one source row
 * must fit the staging tile), wider than 1448 with contrast (s^2 <= 2^21, where the integer mean is exact), or whose filter does
 * not fit the 12 KiB row tile of a channel; a frame index outside [0, Fr); nearer rows outside [0, n_nearer]; an op listed
 * twice or unknown; a resampling table outside the n_bounds rows of `bounds` / n_kk8 elements of `kk8`. */
int sdn_train_rois(const uint8_t* scenes, const int32_t* items, int Fr, int B, int H, int W, int32_t* table, sdnStream stream);
int sdn_train_crops(const uint8_t* frames, const uint8_t* scenes, int Fr, int H, int W, const int32_t* rois_host,
                    const int32_t* objs_host, const int32_t* objs, const int32_t* items_host, const int32_t* items, int B,
                    const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8, const uint8_t* nearer, int n_nearer,
                    int image_size, int mask_size, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                    void* workspace, float* images, float* masks, float* ignores, sdnStream stream);

/* ---- the training items of the real-image sets and of the hybrid batches: geometric/derender3d/datasets.py:549-606
 * (KittiObject.__getitem__), :737-769 (KittiSemantics), :930-971 (CityscapesSemantics), :1077-1112 (CityscapesMaskRCNN), mixed
 * with :332-420 (VKitti) by HybridDataset (:175-190) and data_loader.py:17-37 (collate_fn) ------------------------------------
 * sdn_train_id_stats (datasets.py:938-955 with :95-103 mask_to_roi, per object on the host: a full-frame comparison, a gather, a
 * sort inside np.percentile): for B items over several frames in one call.  items: DEVICE int32 [B, 8] rows, aligned to 8 bytes
 * (address of the item's int32 [H, W] id map as two ints, low word first; address of its int32 [H, W] disparity map, or 0; H; W;
 * the id; one unused int).  Frames may differ in size, several items may name one frame.  max_pixels: the largest H W among the
 * items (it sizes the launch; a larger frame is still walked completely).  table: DEVICE int32 [B, 8] rows (area, y0, x0, y1,
 * x1, n, lo, hi) with the meaning of sdn_scene_id_stats' rows: the pixel count of ids == id, mask_to_roi's box, the number n of
 * non-zero disparities under the mask, and their order statistics of zero-based rank floor(0.95 (n - 1)) and min(that + 1,
 * n - 1) -- what np.percentile(., 95) interpolates between (derender3d.scene.percentile95_threshold); both 0 when n == 0 or
 * when there is no disparity map.  An id that matches no pixel leaves area 0 and the roi (INT_MAX, INT_MAX, 0, 0).  An exact
 * two-level radix select on the 16-bit values, per item: LDS histograms per workgroup, integer atomics only (the result does
 * not depend on scheduling); the call clears table and workspace itself; nothing is copied to the host.  Disparities lie in
 * 0 .. 65535; verified only with SDN_DEBUG_CHECKS=1 in the environment, which makes the call synchronous.  workspace: DEVICE,
 * sdn_train_id_stats_workspace_bytes(B) bytes aligned to 16.  The rows of `items` are trusted: an address or a size that does
 * not describe a live map reads out of bounds.
 *
 * sdn_train_crops_mixed (datasets.py:141-172 as called from :572-577, :764-767, :960-962, :1103-1110 and :415-417): the images
 * [B, 3, image_size, image_size], masks and ignores [B, 1, mask_size, mask_size] of B items in one launch, after a statistics
 * launch when an item's jitter holds contrast.  Window, padding quirk, fill values (127 / 0 / 255), Pillow's bilinear resize,
 * to_tensor and the three fp32 operations of Normalize are those of sdn_train_crops, bit for bit.  rois_host, objs_host / objs,
 * bounds, kk8, nearer and workspace as there, the object table made with each item's OWN frame size.  items / items_host: DEVICE
 * (aligned to 8 bytes) and HOST int32 [B, 32] rows:
 *   0-1    address of the item's uint8 [3, H, W] frame (two ints, low word first)
 *   2-3    address of the mask source      4-5  address of the ignore source
 *   6, 7   H, W of the item's frame
 *   8      mask source: 0 none (the plane is 0.0), 1 colour code on a uint8 [H, W, 3] image, 2 id == on an int32 [H, W] map
 *   9      the code r | g << 8 | b << 16, or the id
 *   10     ignore source: 0 the plane is 0.0 everywhere, with no fill value (torch.zeros(1, 256, 256) of :767 and :1110, and
 *          collate's zero fill); 1 the count of the item's nearer codes on a uint8 [H, W, 3] image, exactly as sdn_train_crops;
 *          2 disparity > thr on an int32 [H, W] map, bytes 0 / 255, outside the frame 255
 *   11     thr        12, 13  first row and number of rows of the item's codes in `nearer`
 *   14-19  the colour jitter: number of ops, the ops in order, the three factors as fp32 bits, the hue shift (sdn_train_crops)
 *   20-22  mean as fp32 bits    23-25  std as fp32 bits    26-31 unused
 * masks and ignores may both be null (a batch without either; every item's sources must then be 0).  The validation of
 * sdn_train_crops applies per item, on the HOST tables before any launch; in addition SDN_EINVAL for a null address that the
 * item's sources need, a source kind outside the lists above, an int32 map that is not aligned to 4 bytes, a frame size below
 * 1 or above INT_MAX / 4 pixels, a std of 0.  The validator is csrc/train_hybrid_check.h (tools/train_hybrid_check.cpp walks
 * it on the CPU).  No float atomics, no host round trip: the outputs are identical from run to run. */
int sdn_train_id_stats_workspace_bytes(int B, size_t* bytes);
int sdn_train_id_stats(const int32_t* items, int B, long max_pixels, int32_t* table, void* workspace, sdnStream stream);
int sdn_train_crops_mixed(const int32_t* rois_host, const int32_t* objs_host, const int32_t* objs, const int32_t* items_host,
                          const int32_t* items, int B, const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8,
                          const uint8_t* nearer, int n_nearer, int image_size, int mask_size, void* workspace, float* images,
                          float* masks, float* ignores, sdnStream stream);

/* ---- the semantic tail: semantic/vkitti_test.py:56-73, vkitti_eval.py:64-107, models.py:401-402, utils.py:101-129,
 * vkitti_dataset.py:206-209, 238 ---------------------------------------------------------------------------------------------
 * The reference upsamples the decoder's scores of every test scale to the frame (nn.functional.upsample, bilinear,
 * align_corners=False), takes the softmax there, averages the S full-resolution tensors, copies the sum to the host and takes
 * torch.max on the CPU; its evaluation runs accuracy() and intersectionAndUnion() in numpy per frame on a ground-truth map
 * built by a Python call per pixel.
 *
 * sdn_segm_fuse (vkitti_test.py:58-72, models.py:401-402): labels uint8 [B, 1, H, W] = arg-max over the classes of
 * sum_s softmax_c(upsample(scores_s))[c] / S, in one launch, no full-resolution intermediate.  table_host: HOST int32 [S, 4]
 * rows (address of the fp32 [B, C, h_s, w_s] DEVICE map as two ints, low word first; h_s; w_s); it travels as the kernel's
 * argument, no copy of its own.  Per output pixel and scale: src = max(0, (dst + 0.5) * (h_s / H) - 0.5) with a float quotient,
 * taps int(src) and the next row clamped to h_s - 1, columns alike; the four taps interpolated in fp32 for all C classes
 * (l0y * (l0x a + l1x b) + l1y * (l0x c + l1x d), no FMA); softmax with the maximum subtracted and expf; p / S added in scale
 * order.  The lowest class wins an exact tie, as torch.max on the CPU; a NaN among a pixel's inputs makes all its sums NaN and
 * its label 0.  pred: fp32 [B, C, H, W], the sums, or NULL (the hot path).  1 <= S <= 8, 1 <= C <= 32, 1 <= B <= 65535,
 * H, W, h_s, w_s <= 16384, h_s <= 2 H and w_s <= 2 W (a map may be larger than the output, up to twice); SDN_EINVAL otherwise
 * and for a null or misaligned address.  No atomics: identical from run to run.  The tile, its LDS arithmetic and the validator
 * are csrc/segm_tail_check.h (tools/segm_tail_check.cpp walks them on the CPU).
 *
 * sdn_segm_labels_from_colors (vkitti_dataset.py:206-209, 238): labels_gt int16 [B, H, W] = table label of the pixel's colour
 * - 1 (unlabelled is -1) for scene uint8 [B, H, W, 3], the layout of sdn_scene_gt_masks.  table / table_host: DEVICE and HOST
 * int32 [2 K]: the K codes r | g << 8 | b << 16 in strictly ascending order, then their K labels (0 .. 255, the reference's
 * astype(np.uint8)); 1 <= K <= 1024; validated on the HOST copy.  A colour that is not in the table (the reference raises
 * KeyError) gets -32768 and is counted: unknown int32 [B], cleared by the call.  scene, table and unknown aligned to 4 bytes,
 * labels_gt to 8.
 *
 * sdn_segm_confusion (utils.py:101-129): counts int64 [B, 3 C + 3] per frame: area_intersection[C], area_pred[C], area_lab[C],
 * acc_sum, valid_sum, the number of pixels with labels_gt == -32768; for labels uint8 [B, 1, H, W] and labels_gt int16
 * [B, H, W].  The reference's masking: valid = labels_gt >= 0; the prediction counts only where valid; a label >= C falls out of
 * the histograms (np.histogram(., bins=C, range=(1, C)) of label + 1) and still counts as valid -- and as wrong unless the
 * prediction equals it -- in accuracy().  1 <= C <= 256.  Integer atomics only: exact, whatever the order.  The call clears
 * counts and writes nothing outside it. */
int sdn_segm_fuse(const int32_t* table_host, int S, int B, int C, int H, int W, uint8_t* labels, float* pred, sdnStream stream);
int sdn_segm_labels_from_colors(const uint8_t* scene, int B, int H, int W, const int32_t* table_host, const int32_t* table, int K,
                                int16_t* labels_gt, int32_t* unknown, sdnStream stream);
int sdn_segm_confusion(const uint8_t* labels, const int16_t* labels_gt, int B, int H, int W, int C, int64_t* counts,
                       sdnStream stream);

/* ---- the semantic training batch: semantic/vkitti_dataset.py:74-163 (TrainDataset.__getitem__) ------------------------------------
 * The reference builds every item on the host: the label of every scene pixel by a Python call (:120), torchvision's ColorJitter
 * through Pillow (:124), cv2.flip (:132-136), scipy.misc.imresize three times (:139-150), RGB to BGR and Normalize (:152-154),
 * and the copy into the zero batch tensors (:107-109, :156-159).  sdn_segm_train_batch does :120-159 for B items in at most
 * three launches (the luma sums of the contrast op, only when an item has one; the images; the labels), bit for bit with Pillow:
 *   img_data fp32 [B, 3, Hb, Wb]: per item the frame after the jitter ops in the item's order (Pillow's arithmetic as
 *     sdn_train_crops applies it; the contrast grey is int(mean(L) + 0.5) over the WHOLE frame), mirrored when flip is set,
 *     resized to (h, w) by Pillow's BILINEAR resize (horizontal pass into bytes, then vertical, 22-bit coefficients; a pass whose
 *     size does not change is skipped), then out[c, y, x] = ((float)px[y, x, 2 - c] - mean_c) / std_c in fp32 with a true
 *     division: mean and std are indexed by the OUTPUT channel, so the reference's RGB constants meet the BGR planes (:152-154).
 *     0 where y >= h or x >= w.  Every element is written.
 *   seg_label int64 [B, Hb / rate, Wb / rate]: the NEAREST resize to (h, w), the zero padding to multiples of rate and the
 *     NEAREST resize by exactly rate (:140-150) composed: table label of scene[yn[rate y + rate / 2], flip(xn[rate x + rate / 2])]
 *     - 1 where rate y + rate / 2 < h and rate x + rate / 2 < w, -1 elsewhere (:159).  A colour that is not in the item's table
 *     (the reference raises KeyError at :120) gives -1 and is counted in unknown int32 [B]; only SAMPLED pixels are looked up.
 * frames, scenes: uint8 [B, H, W, 3] DEVICE.  tables / tables_host: DEVICE and HOST copies of ONE int32 buffer of n_tables ints, so
 * that everything goes up in one copy: B item rows of 20 ints first (csrc/segm_train_check.h: h, w, flip, nops, order, the three
 * factors as floats, hue shift, then offsets into the same buffer: horizontal bounds [w][2] and coefficients [w][ksize] with
 * their ksize (0 for a skipped pass), the vertical ones, the NEAREST column and row tables, the colour table (K codes ascending,
 * K labels) and K, one pad), then the tables the rows name.  Every entry is validated on the HOST copy before any launch:
 * SDN_EINVAL for a bad row, a table outside the buffer, a bound outside the frame, contrast on a frame of more than 2^21 pixels,
 * W > 4096, or an item whose band of 4 output rows needs more resampled source rows than the 12 KiB LDS plane holds (refused,
 * never truncated).  workspace: int32 [n_workspace], at least B * ceil(H W / 2048) ints when an item has contrast.  No float
 * atomics; the one integer atomic is the unknown count: identical from run to run. */
int sdn_segm_train_batch(const uint8_t* frames, const uint8_t* scenes, int B, int H, int W, const int32_t* tables_host,
                         const int32_t* tables, long n_tables, int Hb, int Wb, int rate, float mean0, float mean1, float mean2,
                         float std0, float std1, float std2, int32_t* workspace, long n_workspace, float* img_data,
                         int64_t* seg_label, int32_t* unknown, sdnStream stream);

/* ---- the semantic training loss: semantic/models.py:15-21, 39-45 (pixel_acc and the training branch of
 * SegmentationModule.forward), the decoders' log_softmax (models.py:279-280, 412-413), nn.NLLLoss(ignore_index=-1)
 * (vkitti_train.py:133) ------------------------------------------------------------------------------------------------------------
 * The reference takes log_softmax of both decoder heads, applies NLLLoss to each, adds loss + loss_deepsup * deep_sup_scale and
 * runs pixel_acc (torch.max, two .long() masks, two sums, a float division): about twenty small launches each way.
 *
 * sdn_segm_loss_fwd (models.py:39-45 with :15-21, :279-280, :412-413), two launches:
 *   scores, scores_deepsup: fp32 [B, C, h, w] DEVICE, the outputs of decoder.conv_last / conv_last_deepsup BEFORE log_softmax;
 *     scores_deepsup may be NULL (no deep supervision: loss = loss_main, loss_deepsup = 0).  seg_label: int64 [B, h, w], what
 *     sdn_segm_train_batch writes.  A pixel is valid iff 0 <= label < C; -1 is the ignore label; any other label is ignored in the
 *     loss and in the accuracy and counted in `bad` (the reference raises there).
 *   out fp32 [4]: loss = loss_main + loss_deepsup * deep_sup_scale (fp32, :42), acc = float(acc_sum) / (float(pixel_sum) + 1e-10f)
 *     in fp32 (:20; 0 without a valid pixel), loss_main and loss_deepsup = the sum over the valid pixels of -(x[label] - lse) /
 *     pixel_sum, lse = max + log(sum exp(x - max)) per pixel in fp32, the sum in fp64 (0 / 0 = NaN without a valid pixel, as
 *     NLLLoss gives).  counts int64 [3]: acc_sum, pixel_sum, bad.  The prediction of pixel_acc is the arg-max of the main head's
 *     SCORES with a strict >: the lowest class wins an exact tie (torch.max on the CPU) and a NaN never wins (torch.max would
 *     return the NaN's class); a NaN score makes lse and, on a valid pixel, the loss NaN.
 *   lse fp32 [2, B, h, w]: both heads' lse for the backward call (zeros for an absent head).  scratch: scratch_bytes >= 32 *
 *     B * ceil(h w / 256) bytes, aligned to 8 (csrc/segm_loss_check.h: SGL_PIXELS, SGL_PART_BYTES); nothing needs zeroing.
 * sdn_segm_loss_bwd (the autograd of the above), one launch: grad_scores / grad_scores_deepsup fp32 [B, C, h, w], either may be
 *   NULL; every element of a given one is written: (exp(x[c] - lse) - [c == label]) * g / pixel_sum on a valid pixel, 0 on an
 *   ignored one, with g = grad_out[0] + grad_out[2] for the main head and grad_out[0] * deep_sup_scale + grad_out[3] for the
 *   deepsup head (grad_out fp32 [4] DEVICE, the gradient of `out`; acc carries none); pixel_sum is read from counts on the device.
 * 1 <= C <= 32, B, h, w >= 1, B * C * h * w < 2^31; SDN_EINVAL with a message otherwise and for a NULL pointer, before any launch.
 * 16-byte loads across four adjacent pixels when h * w % 4 == 0 and every base is 16-byte aligned, scalar loads otherwise.  No
 * atomics; identical from run to run; nothing crosses to the host. */
int sdn_segm_loss_fwd(const float* scores, const float* scores_deepsup, const int64_t* seg_label, int B, int C, int h, int w,
                      float deep_sup_scale, void* scratch, size_t scratch_bytes, float* lse, float* out, int64_t* counts,
                      sdnStream stream);
int sdn_segm_loss_bwd(const float* scores, const float* scores_deepsup, const int64_t* seg_label, int B, int C, int h, int w,
                      float deep_sup_scale, const float* lse, const int64_t* counts, const float* grad_out, float* grad_scores,
                      float* grad_scores_deepsup, sdnStream stream);

/* ---- the pyramid pooling module of the semantic decoders: semantic/models.py:336-346, 387-397 (csrc/segm_ppm.hip) -----------------
 * PPMBilinear / PPMBilinearDeepsup.forward: for every pool scale AdaptiveAvgPool2d(s) of conv5, the branch's 1 x 1 conv / BN / ReLU,
 * a bilinear upsample back to conv5's size, then torch.cat([conv5, branch outputs], 1): nine full-tensor launches forward, about
 * twice that backward.  The four calls below go around the caller's branch modules, two launches forward and two backward.
 * Everything is fp32, contiguous NCHW, DEVICE; scales, branch_channels, y, grad_y, grad_p are HOST arrays of S entries
 * (1 <= S <= 4, 1 <= scales[k] <= 8, branch_channels[k] = K_k >= 1; Ctot = C + sum K_k; B * Ctot * h * w < 2^31).
 *
 * sdn_segm_ppm_pool, one launch: conv5 [B, C, h, w] is read once; cat [B, Ctot, h, w] gets conv5 in its first C channels, bit for
 *   bit, its other channels are left alone; pooled holds p_0 .. p_{S-1}, p_k [B, C, s_k, s_k] contiguous, one after the other
 *   (p_k begins at float B * C * sum_{k' < k} s_k'^2).  Bins are torch's: rows floor(i h / s) up to ceil((i + 1) h / s), columns
 *   likewise, value = sum / area; the sum is taken in fp64, columns then rows in ascending order, and rounded once.
 * sdn_segm_ppm_fill, one launch for all branches: y[k] [B, K_k, s_k, s_k], the branch outputs; channel C + sum_{k' < k} K_k' + j
 *   of cat becomes the bilinear upsampling of y[k][:, j] to h x w, align_corners=False, torch's fp32 rule: scale = (float)s / n,
 *   src = max(scale * (o + 0.5f) - 0.5f, 0), i0 = (int)src, i1 = min(i0 + 1, s - 1), lambda = src - i0.  Every element of those
 *   channels is written, nothing else.
 * sdn_segm_ppm_fill_bwd, one launch: grad_cat [B, Ctot, h, w]; grad_y[k] [B, K_k, s_k, s_k] = the transposed interpolation of
 *   the planes grad_cat[:, C + ...], summed in fp64 in a fixed order.  A NULL grad_y[k] is skipped and its planes are not read
 *   (not all may be NULL); the first C channels are not read.
 * sdn_segm_ppm_pool_bwd, one launch: grad_conv5 [B, C, h, w] = grad_cat[:, :C] + for every scale the sum of grad_p[k][bin] /
 *   area(bin) over the bins that cover the pixel (one or two per axis when h >= s, more when h < s).  grad_cat may be NULL,
 *   grad_p may be NULL and so may any grad_p[k], but not all of them.  branch_channels is needed for grad_cat's stride.
 * SDN_EINVAL with a message before any launch for a NULL or misaligned pointer and for sizes outside the above.  16-byte loads and
 * stores when w % 4 == 0 and the bases are 16-byte aligned, scalar ones otherwise.  No atomics, nothing to zero; identical from
 * run to run; nothing crosses to the host. */
int sdn_segm_ppm_pool(const float* conv5, int B, int C, int h, int w, const int* scales, const int* branch_channels, int S, float* cat,
                      float* pooled, sdnStream stream);
int sdn_segm_ppm_fill(const float* const* y, int B, int C, int h, int w, const int* scales, const int* branch_channels, int S, float* cat,
                      sdnStream stream);
int sdn_segm_ppm_fill_bwd(const float* grad_cat, int B, int C, int h, int w, const int* scales, const int* branch_channels, int S,
                          float* const* grad_y, sdnStream stream);
int sdn_segm_ppm_pool_bwd(const float* grad_cat, const float* const* grad_p, int B, int C, int h, int w, const int* scales,
                          const int* branch_channels, int S, float* grad_conv5, sdnStream stream);

/* ---- the input side of the textural networks (csrc/encode_input.hip) ------------------------------------------------------------------
 * Element types of the index and instance maps below: */
#define SDN_MAP_U8 0
#define SDN_MAP_I16 1
#define SDN_MAP_I32 2
#define SDN_MAP_F32 3
/* sdn_encode_maps, one kernel launch: the label planes, the edge plane and the pose planes of Pix2PixHDModel.encode_input
 * (textural/models/pix2pixHD_model.py:124-166 with get_edges :343-349: zeros + long + scatter_ twice, about ten slice / compare / or
 * launches and a cat).  All maps are contiguous [N, 1, H, W], DEVICE: label uint8 / int32 / float32; inst int16 / int32 / float32 or
 * NULL (no edge plane); pose int32 / float32, read when pose_ch > 0.  1 <= label_nc <= 256, 0 <= pose_ch <= 256
 * (feat_pose_num_bins + 1, or 0 for none).
 *   input_label fp32 [N, label_nc (+ 1 with inst), H, W]: plane trunc(label) holds 1.0f (the value truncated toward zero, as
 *     .long() does: -0.5 selects plane 0), every other label plane 0.0f; the last plane is 1.0f where the instance value differs
 *     (!= in the map's own dtype: NaN differs from NaN) from its left, right, upper or lower neighbour inside the map.
 *   pose_onehot fp32 [N, pose_ch, H, W] likewise from pose; not touched (may be NULL) when pose_ch == 0.
 *   bad int32 [2]: where the reference's scatter_ trips a device-side assert -- an index outside [0, channels) or a NaN -- no plane
 *     is set and the pixel is counted, bad[0] for label, bad[1] for pose (the convention of sdn_segm_loss_fwd's counts[2]).
 * Every element of both outputs is written; the caller zeroes nothing (the entry point clears the 8 bytes of bad on the stream).
 * 16-byte plane stores when W % 4 == 0 and all bases are 16-byte aligned, scalar ones otherwise.  Nothing crosses to the host.
 *
 * sdn_inst_index_*: the instance numbering of Encoder.forward (textural/models/networks.py:310-325: inst[i] = inst[i] * bs + i,
 * then np.unique over every pixel) without a sort.  The key of a pixel is the disambiguated value truncated toward zero; the
 * product and sum are taken in the map's own dtype (fp32: two roundings; int32, int16: wraparound).  Keys live in the window
 * [-32768, 2^21 - 32768); workspace: sdn_inst_index_workspace_bytes (a presence bitmap, the words' prefix counts, K, overflow),
 * aligned to 16 bytes, caller-owned, cleared by sdn_inst_index_build itself.
 * sdn_inst_index_build, two launches: writes the disambiguated values back into inst [N, 1, H, W] in place (as the reference does)
 *   and sets every key's bit; then one workgroup forms the prefix counts, K and ids int64 [id_capacity >= min(N H W, 2^21)], the
 *   first K entries ascending, and clears counts int64 [id_capacity] (may be NULL) in its first K entries.  int32 [2] at byte
 *   65536 * 4 of the workspace: K and overflow, the number of pixels whose key lies outside the window or is NaN / Inf -- the
 *   one 8-byte copy a caller needs before it can size its results.  With overflow != 0 the numbering is incomplete.
 * sdn_inst_index_rank, one launch, after build on the same stream, inst as build left it: seg int32 [N, H, W] = the position of
 *   the pixel's key in ids (-1 outside the window); counts [k] += the pixels of id k when not NULL (integer atomics, summed per
 *   lane and per workgroup first).  Identical from run to run.
 * SDN_EINVAL with a message before any launch for a NULL or misaligned pointer, an unsupported dtype, sizes of 2^31 or more, channel
 * counts outside the above, or a workspace / ids buffer that is too small. */
int sdn_encode_maps(const void* label, int label_dtype, const void* inst, int inst_dtype, const void* pose, int pose_dtype, int N, int H,
                    int W, int label_nc, int pose_ch, float* input_label, float* pose_onehot, int32_t* bad, sdnStream stream);
int sdn_inst_index_workspace_bytes(size_t* bytes);
int sdn_inst_index_build(void* inst, int inst_dtype, int N, int H, int W, void* workspace, size_t workspace_bytes, int64_t* ids,
                         int64_t* counts, long id_capacity, sdnStream stream);
int sdn_inst_index_rank(const void* inst, int inst_dtype, int N, int H, int W, const void* workspace, size_t workspace_bytes,
                        int32_t* seg, int64_t* counts, sdnStream stream);

/* ---- the training losses of Mask R-CNN: geometric/maskrcnn/model.py:1004-1147 (compute_losses and the five functions it calls)
 * and the sum of :1955 (csrc/mrcnn_loss.hip) --------------------------------------------------------------------------------------------
 * The reference selects the contributing anchors and RoIs with four torch.nonzero calls (:1020, 1047, 1091, 1121; each one waits
 * for the device), gathers through index tensors, runs cross_entropy twice, smooth_l1_loss twice and binary_cross_entropy once, and
 * backward turns every gather into a zero fill and an index_put.  Everything below is DEVICE memory, contiguous.
 *   rpn_match [1, A, 1] int32 (match_i64 = 0) or int64 (1): 1 positive, -1 negative, 0 neutral; rpn_bbox fp32 [1, T, 4] (targets);
 *   rpn_class_logits fp32 [1, A, 2]; rpn_pred_bbox fp32 [1, A, 4]; `batch` is their first dimension and must be 1 (:1053).
 *   target_class_ids [R] int32 (ids_i64 = 0) or int64 (1); mrcnn_class_logits fp32 [R, C]; target_deltas fp32 [R, 4]; mrcnn_bbox
 *   fp32 [R, C, 4]; target_mask fp32 [R, h, w]; mrcnn_mask fp32 [R, C, h, w], probabilities.  With R = 0 the head tensors are not
 *   read (they may be NULL) and the three head losses are 0 (:1070, 1088, 1118).
 * 1 <= A <= 2^24, 1 <= T, 0 <= R, 2 <= C <= 128, R * C * h * w < 2^31.
 *
 * sdn_mrcnn_loss_workspace_bytes: the sizes of `workspace` (forward only; nothing needs zeroing) and `saved` (written by forward,
 *   read by backward: the four selection counts, the RoIs' log-sum-exps, the positive anchors before every chunk of 1024 anchors).
 * sdn_mrcnn_loss_fwd, three launches (replaces :1004-1147 and :1955):
 *   out fp32 [6]: rpn_class_loss (:1004-1029: mean over the anchors with match != 0 of the 2-class cross entropy against
 *     [match == 1]), rpn_bbox_loss (:1032-1058: the k-th positive anchor in anchor order against target row k, smooth L1 with beta
 *     1, mean over 4 n_rpn_pos), mrcnn_class_loss (:1061-1077: mean cross entropy over the RoIs), mrcnn_bbox_loss (:1080-1106:
 *     smooth L1 over the RoIs with id > 0, the deltas of the RoI's class, mean over 4 n_roi_pos), mrcnn_mask_loss (:1109-1136:
 *     torch's binary_cross_entropy, each log clamped at -100, of the positive RoIs' class plane, mean over n_roi_pos h w), and
 *     their sum (:1955).  Each element is evaluated in fp64, each loss summed in fp64 in a fixed order and rounded to fp32 once;
 *     the sum is the fp64 sum of the five, rounded once.  A mean over an empty selection is NaN, as torch's.
 *   counts int64 [4]: n_rpn_valid (match 1 or -1), n_rpn_pos (the positives in the box loss), n_roi_pos, bad.  `bad` counts what
 *     the reference has no defined answer for, each left out of its loss: an rpn_match value outside {-1, 0, 1}; a positive anchor
 *     with T or more positives before it (it stays in the class loss); a target_class_ids value outside [0, C) (the RoI is left
 *     out of all three head losses and of their divisors).  A mask probability outside [0, 1] makes that loss NaN.
 * sdn_mrcnn_loss_bwd, one launch (the autograd of the above): grad_out fp32 [6], the gradient of `out`; each of the five gradients
 *   has the shape of its input and may be NULL (skipped; not all).  Every element of a given one is written exactly once, +0.0
 *   outside the selections; the binary cross entropy's is torch's (p - y) / max((1 - p) p, 1e-12).  The targets get none.
 * SDN_EINVAL with a message before any launch for a NULL or misaligned pointer, a batch other than 1 and sizes outside the above.
 * A lane takes four adjacent anchors: 16-byte loads and stores of rpn_match, the logits and the [A, 4] rows when all RPN bases are
 * 16-byte aligned, and of the mask planes when h * w % 4 == 0 and their bases are; scalar ones otherwise.  No atomics, no
 * workgroup waits for another; identical from run to run; nothing crosses to the host. */
int sdn_mrcnn_loss_workspace_bytes(int A, int R, size_t* workspace_bytes, size_t* saved_bytes);
int sdn_mrcnn_loss_fwd(const void* rpn_match, int match_i64, const float* rpn_bbox, const float* rpn_class_logits,
                       const float* rpn_pred_bbox, int batch, int A, int T, const void* target_class_ids, int ids_i64,
                       const float* mrcnn_class_logits, const float* target_deltas, const float* mrcnn_bbox, const float* target_mask,
                       const float* mrcnn_mask, int R, int C, int h, int w, void* workspace, size_t workspace_bytes, void* saved,
                       size_t saved_bytes, float* out, int64_t* counts, sdnStream stream);
int sdn_mrcnn_loss_bwd(const void* rpn_match, int match_i64, const float* rpn_bbox, const float* rpn_class_logits,
                       const float* rpn_pred_bbox, int batch, int A, int T, const void* target_class_ids, int ids_i64,
                       const float* mrcnn_class_logits, const float* target_deltas, const float* mrcnn_bbox, const float* target_mask,
                       const float* mrcnn_mask, int R, int C, int h, int w, const void* saved, size_t saved_bytes, const float* grad_out,
                       float* grad_rpn_class_logits, float* grad_rpn_pred_bbox, float* grad_mrcnn_class_logits, float* grad_mrcnn_bbox,
                       float* grad_mrcnn_mask, sdnStream stream);

/* ---- the 2D and 2D+ edit baselines: geometric/scripts/main.py:215-322 (_test_2d, _test_2d_plus), the loop at :293-312 ----------
 * The reference, per object and frame: slices the detector mask at its roi, fetches it to the host, PIL-resizes it (bilinear)
 * to (int(d0), int(d1)), pastes it into a new frame-sized 'L' image at (int(m1 - d1 / 2), int(m0 - d0 / 2)), uploads it,
 * torch.round()s it and blends (1 - m) * map + m * (1 + index), objects in index order.  sdn_scene_paint2d paints F frames in
 * one launch, bit for bit:
 *   out uint8 [F, 1, H, W]: per pixel the HIGHEST active object index n whose pasted, resized mask covers it, + 1; 0 for none.
 *   "Covers": the pixel lies inside the paste box (PIL's paste clips at the frame; a box wholly outside paints nothing) and
 *   Pillow's resize of the 0 / 255 window evaluated there -- horizontal pass rounded and clipped to 8 bits, then the vertical
 *   pass, 22-bit fixed point, a pass skipped when its size does not change -- is v with round(v / 255) == 1, i.e. v >= 128.
 * cover: the words of sdn_scene_cover for the N masks [ceil(N / 32), H W].  recs: DEVICE int32 [F, N, 16] rows (active flag,
 * window first row, first column, rows, columns, output rows, columns, paste top, left, then for the rows and for the columns:
 * first row of `bounds`, first element of `kk8`, ksize -- 0 when the sizes are equal --, one unused int); recs_host: the same
 * table on the HOST, validated before the launch (an active row whose window is empty or leaves the frame, whose output size
 * is below 1, or whose tables lie outside the n_bounds rows of `bounds` / n_kk8 elements of `kk8` is SDN_EINVAL).  bounds / kk8
 * as for sdn_composite_frame.  With recs and recs_host NULL ("identity"; bounds / kk8 unused) every frame is the unedited masks
 * painted in index order, the highest set cover bit + 1: the NAME-ref.png map of main.py:236-238.  N <= 255 (uint8 ids). */
int sdn_scene_paint2d(const uint32_t* cover, const int32_t* recs_host, const int32_t* recs, int F, int N, const int32_t* bounds,
                      int n_bounds, const int32_t* kk8, int n_kk8, int H, int W, uint8_t* out, sdnStream stream);

/* ---- PerspectiveTransform: derender3d/models/transforms.py:102-158, all objects of a frame at once -----------------------
 * out[b,v] = zoom( shear( R(quat[b]) (verts[b,v] * scales[b]) + trans[b] ) ),  shear: x -= x0/z0 * z, y -= y0/z0 * z with
 * (x0,y0,z0) = persp[b].  Test-time form (zoom_fixed NULL, :147-158): zooms[b] = min_v |z| / max(|x|,|y|) * zoom_to[b];
 * training form (zoom_fixed [n], :139-150, also what the optimisation loop of scripts/main.py:433-456 runs because it puts
 * the model in train mode): zooms[b] = zoom_fixed[b], zoom_to unused (may be NULL).  z /= zooms[b] either way.
 * key: n * (1 + ceil(V / 256)) uint64 (caller-owned, no initialisation needed, kept for the backward pass): key[b] = bits
 * of zooms[b] / zoom_to[b] << 32 | the argmin vertex (0xffffffff in the training form); the rest is scratch (one minimum
 * per block of 256 vertices). */
/* bytes of the two caller-owned scratch buffers above / below for n objects of V vertices (so that a binding never restates
 * the formulas; the reference's PerspectiveTransform, derender3d/models/transforms.py:102-158, has no scratch -- its minimum and
 * its sums are torch reductions): *key_bytes for sdn_perspective_transform's `key`, *acc_bytes for sdn_perspective_transform_bwd's `acc`. */
int sdn_perspective_transform_scratch(int n, int V, size_t* key_bytes, size_t* acc_bytes);
int sdn_perspective_transform(const float* verts, const float* scales, const float* quat, const float* trans,
                              const float* persp, const float* zoom_to, const float* zoom_fixed, int n, int V, float* out,
                              float* zooms, void* key, sdnStream stream);
/* gradients of the above given g_out [n,V,3] and (optional) g_zooms [n]; acc: 36 n floats of scratch (no initialisation
 * needed).  After the training
 * form pass zoom_to = ones [n]: g_zoom_to[b] * zoom_to / zoom_fixed[b] ... i.e. g_zoom_to[b] / zoom_fixed[b] is then
 * d loss / d zoom_fixed[b].   g_persp may equal g_trans (one tensor passed as both
 * translations): the two gradients are then added into it (r06). */
int sdn_perspective_transform_bwd(const float* verts, const float* scales, const float* quat, const float* trans,
                                  const float* persp, const float* zoom_to, int n, int V, const float* out,
                                  const void* key, const float* g_out, const float* g_zooms, float* g_verts,
                                  float* g_scales, float* g_quat, float* g_trans, float* g_persp, float* g_zoom_to,
                                  float* acc, sdnStream stream);

/* ---- Mask R-CNN custom ops (only `--source maskrcnn` of geometric/scripts/main.py:642-661 needs them) -------
 * Greedy NMS: geometric/maskrcnn/nms/src/nms.c:4-69 (cpu_nms) / nms_cuda.c:17-67 + cuda/nms_kernel.cu:26-82.
 * boxes_sorted [n,4] and areas_sorted [n] (= (x2-x1+1)*(y2-y1+1), as pth_nms.py computes them) are already in descending
 * score order.  keep [n] int64 receives the kept positions (indices into the sorted arrays, ascending), *count their
 * number -- both DEVICE memory: the greedy pass runs on the device too (the reference copies the mask to the host).
 * strict 0: suppress when IoU >= thresh (cpu_nms, nms.c:59); 1: IoU > thresh (nms_kernel.cu:66).  Workspace: query first. */
int sdn_nms_workspace_bytes(int n, size_t* out);
int sdn_nms(const float* boxes_sorted, const float* areas_sorted, int n, float thresh, int strict, long long* keep,
            long long* count, void* workspace, size_t workspace_bytes, sdnStream stream);
/* crop_and_resize: geometric/maskrcnn/roialign/roi_align/src/crop_and_resize.c:7-158 (forward), :160-251 (backward);
 * CUDA twins cuda/crop_and_resize_kernel.cu:10-185.  image [B,C,H,W]; boxes [n,4] = (y1,x1,y2,x2) normalised to [0,1];
 * box_index [n] int32 in [0,B); crops [n,C,crop_h,crop_w]: bilinear samples, `extrapolation` outside the image.  The
 * backward pass zeroes grads_image [B,C,H,W] and scatter-adds (float atomics, as the reference's CUDA path). */
int sdn_crop_and_resize_fwd(const float* image, int B, int C, int H, int W, const float* boxes, const int32_t* box_index,
                            int n, int crop_h, int crop_w, float extrapolation, float* crops, sdnStream stream);
int sdn_crop_and_resize_bwd(const float* grads, const float* boxes, const int32_t* box_index, int n, int crop_h, int crop_w,
                            float* grads_image, int B, int C, int H, int W, sdnStream stream);
/* Pyramid RoIAlign: pyramid_roi_align of geometric/maskrcnn/model.py:414-502 with log2 of :95-100 (csrc/pyramid_roi_align.hip).
 * boxes fp32 [R, 4] = (y1, x1, y2, x2) normalised; maps[4]: P2 .. P5, each fp32 [C, H[l], W[l]] contiguous; image_area =
 * float(image_shape[0] * image_shape[1]).  Box r is sampled from level clamp(rint(4 + log(sqrt(h * w) / (224 / sqrt(image_area))) /
 * log(2)), 2, 5), computed in fp32 operation for operation as :445-457; a non-finite value (area <= 0, NaN) gives level 2, which is
 * what the reference's CPU run yields through the x86 float-to-int conversion and the clamp.  The samples are those of
 * sdn_crop_and_resize_fwd with crop_h = crop_w = pool (1 <= pool <= 32), bit for bit.
 * _fwd, ONE launch: pooled fp32 [R, C, pool, pool] in BOX order (row r is box r: no sort, no gather) and levels int32 [R] (2 .. 5).
 * _bwd, a zero fill and ONE scatter launch: grads fp32 [R, C, pool, pool]; grad_maps is one caller-owned allocation, 16-byte aligned,
 * of `total` floats that holds the four maps' gradients, level l as [C, H[l], W[l]] at float offsets[l] (every offset a multiple of
 * four) -- ask sdn_pyramid_roi_align_grad_floats.  The whole allocation is zeroed first, so levels without a box are all zero.  The
 * scatter uses fp32 atomic adds (as sdn_crop_and_resize_bwd and the reference's CUDA kernel): the gradients are NOT bit-reproducible
 * from run to run.  The boxes get no gradient (the reference detaches them, :473).  R = 0: _fwd launches nothing, _bwd still zeroes.
 * SDN_EINVAL with a message for: NULL pointers with R > 0, C <= 0, a level with H or W <= 0, pool outside [1, 32], image_area not
 * finite or <= 0, C * H * W of a level or C * pool * pool not below 2^31.  Nothing is copied to the host. */
int sdn_pyramid_roi_align_grad_floats(int C, const int* H, const int* W, size_t* offsets, size_t* total);
int sdn_pyramid_roi_align_fwd(const float* boxes, int R, const float* const* maps, const int* H, const int* W, int C, int pool,
                              float image_area, float extrapolation, float* pooled, int32_t* levels, sdnStream stream);
int sdn_pyramid_roi_align_bwd(const float* grads, const float* boxes, int R, const int* H, const int* W, int C, int pool,
                              float image_area, float* grad_maps, sdnStream stream);
/* The ORDERED backward of the pyramid RoIAlign: the same arguments, the same grad_maps layout, level rule and sample arithmetic as
 * sdn_pyramid_roi_align_bwd, but bit-reproducible: no float atomics and no zero fill.  Every element of grad_maps -- the padding
 * between the levels and whole levels without a box included -- is stored exactly once by a plain store.  Its value: the four fp32
 * terms of every inside sample that lands on it, formed operation for operation as crop_and_resize.c:241-247 (a sample on a pixel
 * row or column sends two terms to one pixel, both are added, so 0 * inf gives NaN as there), widened to fp64, added to +0.0 in an
 * order that depends on the arguments' values only (ascending box, then sample row, sample column, tap), rounded to fp32 once.
 * TWO launches: a record per box (level, touched window) into `workspace`, then one workgroup per (level, tile of 8 x 8 pixels, chunk
 * of 64 channels) that gathers from the boxes whose window meets its tile.  workspace: caller-owned, 16-byte aligned, at least
 * sdn_pyramid_roi_align_bwd_ordered_workspace_bytes(R) bytes (32 per box; R = 0 needs none and may pass NULL; the whole buffer is
 * then +0.0).  Nothing crosses to the host; the call can be captured in a graph.  SDN_EINVAL as _bwd, and for: workspace NULL,
 * misaligned or too small with R > 0; the query refuses R < 0 and a NULL `bytes`. */
int sdn_pyramid_roi_align_bwd_ordered_workspace_bytes(int R, size_t* bytes);
int sdn_pyramid_roi_align_bwd_ordered(const float* grads, const float* boxes, int R, const int* H, const int* W, int C, int pool,
                                      float image_area, float* grad_maps, void* workspace, size_t workspace_bytes, sdnStream stream);
/* Proposal layer: proposal_layer of geometric/maskrcnn/model.py:344-407 with apply_box_deltas (:307-328) and clip_boxes (:331-341)
 * (csrc/proposal_layer.hip).  rpn_probs fp32 [A, 2] = (bg, fg); rpn_bbox fp32 [A, 4]; anchors fp32 [A, 4] = (y1, x1, y2, x2) in pixels;
 * std_dev: four floats in HOST memory, read during the call; 1 <= K <= min(A, 8192) anchors enter the NMS (the caller passes
 * K = min(pre_nms_limit, A)), 1 <= P <= 8192 proposals leave it; 1 <= A < 2^24.
 *  1. The K anchors with the largest rpn_probs[:, 1], best first, equal scores lower index first: torch.sort(descending=True,
 *     stable=True), NaN above +inf.  An exact radix select finds the K-th score; the column is read in place, nothing sorts all A.
 *  2. Decode and clip of those K rows in fp32, operation by operation as :370, :313-326, :336-340 (no FMA contraction; expf is the only
 *     operation that can differ from the reference's CPU run); a NaN coordinate stays NaN, as torch.clamp leaves it.
 *  3. Greedy NMS in score order with sdn_nms's own pair test (+1 pixel convention; strict 1: IoU > nms_threshold, 0: >=), stopped once P
 *     boxes are kept: keep equals the first P entries sdn_nms keeps on the same boxes.
 *  4. rois[r] = boxes_px[keep[r]] / (height, width, height, width), one IEEE division per coordinate (:402).
 * Results, all DEVICE memory: order int32 [K] (anchor indices), boxes_px fp32 [K, 4], keep int32 [P] (positions in `order`; -1 behind
 * *count), count int32 [1], rois fp32 [P, 4] (+0.0 behind *count).  Every element is written: nothing needs clearing.  Nothing is
 * differentiable (the reference detaches the boxes where it differentiates past them, :473).  Workspace: query first; 16-byte aligned,
 * as boxes_px and rois.  Two calls on the same inputs give the same bits.  Nothing is copied to the host, every launch goes to
 * `stream`.  SDN_EINVAL with a message, before any launch, for sizes outside the ranges above, height or width < 1, NULL or misaligned
 * pointers and a workspace that is too small. */
int sdn_proposal_layer_workspace_bytes(int A, int K, int P, size_t* out);
int sdn_proposal_layer(const float* rpn_probs, const float* rpn_bbox, const float* anchors, int A, const float* std_dev, int height,
                       int width, int K, int P, float nms_threshold, int strict, int32_t* order, float* boxes_px, int32_t* keep,
                       int32_t* count, float* rois, void* workspace, size_t workspace_bytes, sdnStream stream);

/* Detection layer: refine_detections of geometric/maskrcnn/model.py:744-837 with apply_box_deltas (:307-328) and clip_to_window
 * (:731-741) (csrc/detection_layer.hip).  rois fp32 [N, 4] = (y1, x1, y2, x2) normalised; probs fp32 [N, C]; deltas fp32 [N, C, 4];
 * window (y1, x1, y2, x2 in pixels) and std_dev: four floats each in HOST memory, read during the call; 1 <= N <= 8192, 1 <= C,
 * 1 <= D <= 8192 (max_instances); roi_count: int32 [1] in DEVICE memory or NULL (= N): rows at or behind it are never detections.
 *  1. Per row: class_id = the first index of the row's maximum (a NaN is the maximum, the first NaN wins: torch.max on the CPU),
 *     score = that element; the class's deltas times std_dev, apply_box_deltas in normalised coordinates, times (height, width,
 *     height, width), clamp to the window as torch.clamp (a NaN stays), round half to even -- fp32, operation by operation, no FMA
 *     contraction; expf is the only operation that can differ from the reference's CPU run.
 *  2. A row is valid if it lies below *roi_count, class_id > 0 and, unless min_confidence == 0 (:796), score >= min_confidence.
 *  3. Per-class greedy NMS on the rounded boxes with sdn_nms's pair test (+1 pixel convention; strict 1: IoU > nms_threshold, 0: >=),
 *     rows in descending score order, equal scores lower row first; of the rows kept, the best D by score, best first.  Computed as
 *     one scan in that order over a pair mask that also requires equal class ids, stopped at D.
 * Results, all DEVICE memory: class_ids int32 [N], scores fp32 [N], boxes_px fp32 [N, 4] (every row); keep int32 [D] (rows; -1 behind
 * *count), count int32 [1], detections fp32 [D, 6] = (y1, x1, y2, x2, class_id, score) and boxes_norm fp32 [D, 4] = detections[:, :4]
 * / (height, width, height, width), one IEEE division per coordinate (:1769); both +0.0 behind *count.  Where no row is valid *count
 * is 0 (the reference raises).  Every element is written: nothing needs clearing.  Nothing is differentiable.  Workspace: query first;
 * 16-byte aligned, as boxes_px and boxes_norm.  Two calls on the same inputs give the same bits.  Nothing is copied to the host, every
 * launch goes to `stream`.  SDN_EINVAL with a message, before any launch, for sizes outside the ranges above, height or width < 1,
 * NULL or misaligned pointers and a workspace that is too small. */
int sdn_detection_layer_workspace_bytes(int N, int C, int D, size_t* out);
int sdn_detection_layer(const float* rois, const float* probs, const float* deltas, int N, int C, const float* window,
                        const float* std_dev, int height, int width, float min_confidence, float nms_threshold, int D, int strict,
                        const int32_t* roi_count, int32_t* class_ids, float* scores, float* boxes_px, int32_t* keep, int32_t* count,
                        float* detections, float* boxes_norm, void* workspace, size_t workspace_bytes, sdnStream stream);

/* Detection targets: detection_target_layer of geometric/maskrcnn/model.py:545-724 with bbox_overlaps (:508-542) and
 * utils.box_refinement (utils.py:92-113) for one image (csrc/detection_targets.hip).  All pointers but std_dev are DEVICE memory.
 * proposals fp32 [N, 4] = (y1, x1, y2, x2) normalised, 1 <= N <= 8192; gt_class_ids int32 [G] (ids_int64 0) or int64 [G] (1); gt_boxes
 * fp32 [G, 4] normalised; gt_masks fp32 [G, mask_h, mask_w]; 1 <= G <= 128; keys fp32 [2, N]: the randomness, as data; roi_count int32
 * [1] or NULL (= N): rows at or behind it are never sampled; R = TRAIN_ROIS_PER_IMAGE, 1 <= R <= 8192; positive_ratio in (0, 1];
 * std_dev four positive floats in HOST memory, read during the call; (H, W) = MASK_SHAPE, each side 1 to 64.
 *  1. IoU of every proposal with every box as bbox_overlaps computes it in fp32: compare-based max and min that hand a NaN on, a
 *     clamp at 0 likewise, one IEEE division, no contraction.  If any id is negative, boxes with id < 0 are crowd boxes and only
 *     boxes with id > 0 stay ground truth (:579-591); otherwise all G boxes stay, those with id 0 included.
 *  2. A row's maximum over the ground truth and its FIRST index, a NaN being the maximum (torch.max).  Positive: maximum >= 0.5.
 *     Negative: maximum < 0.5 and, with a crowd, the maximum over the crowd < 0.001.  A NaN maximum is neither.
 *  3. The positives taken are the positive rows with the cap = int(R * positive_ratio) smallest keys[0], in key order; key order is the
 *     usual monotone image of the float's bits, then lower row first.  With P of them taken, the negatives are the negative rows with
 *     the min(int((1.0 / positive_ratio) * P - P), R - P) smallest keys[1], likewise; the count is Python's fp64 expression (:669-670).
 *     Without a positive there is no negative either (:667); where the crowd filter leaves no box (the reference raises) *count is 0.
 * Results, positives first, then negatives: rois fp32 [R, 4] (+0.0 behind *count); target_class_ids int32 [R] (the matched box's id,
 * 0 for negatives, -1 behind *count: what sdn_mrcnn_loss_fwd leaves out); target_deltas fp32 [R, 4] = box_refinement / std_dev in fp32
 * operation by operation, logf being the only operation whose last bit may differ from a CPU run (+0.0 for negatives and behind
 * *count); target_mask fp32 [R, H, W]: crop_and_resize of the matched mask, rounded half to even -- with use_mini_mask the roi
 * re-expressed in the matched box's frame (:642-650), otherwise the roi itself on a full-size mask (+0.0 for negatives and behind
 * *count); rows int32 [R]: the proposal of every output row, -1 behind *count; assign int32 [R]: the matched box's index among the G,
 * -1 for all but positives; count, n_pos int32 [1].  Every element is written: nothing needs clearing.  Nothing is differentiable.
 * Two dependent launches on `stream`, no atomics: two calls on the same inputs give the same bits.  Nothing is copied to the host.
 * Workspace: query first; 16-byte aligned, as rois and target_deltas.  SDN_EINVAL with a message, before any launch, for sizes outside
 * the ranges above, NULL or misaligned pointers and a workspace that is too small. */
int sdn_detection_targets_workspace_bytes(int N, int G, int mask_h, int mask_w, int R, int H, int W, size_t* out);
int sdn_detection_targets(const float* proposals, const void* gt_class_ids, const float* gt_boxes, const float* gt_masks,
                          const float* keys, int N, int G, int mask_h, int mask_w, int ids_int64, const int32_t* roi_count, int R,
                          double positive_ratio, const float* std_dev, int H, int W, int use_mini_mask, float* rois,
                          int32_t* target_class_ids, float* target_deltas, float* target_mask, int32_t* rows, int32_t* assign,
                          int32_t* count, int32_t* n_pos, void* workspace, size_t workspace_bytes, sdnStream stream);

/* RPN targets: build_rpn_targets of geometric/maskrcnn/model.py:1214-1322 with compute_overlaps / compute_iou (utils.py:52-89) for one
 * image (csrc/rpn_targets.hip).  All pointers but std_dev are DEVICE memory.  anchors fp64 [A, 4] = (y1, x1, y2, x2) in pixels,
 * 1 <= A < 2^24; gt_class_ids int32 [G] (ids_int64 0) or int64 [G] (1); gt_boxes fp32 [G, 4] (boxes_int32 0) or int32 [G, 4] (1) in
 * pixels, widened exactly to fp64; 1 <= G <= 128; keys fp32 [2, A]: the randomness, as data; gt_count int32 [1] or NULL (= G): rows of
 * gt_class_ids and gt_boxes at or behind it are not read; T = RPN_TRAIN_ANCHORS_PER_IMAGE, 2 <= T <= 8192; std_dev =
 * RPN_BBOX_STD_DEV, four positive doubles in HOST memory, read during the call.  All arithmetic is fp64, operation for operation
 * numpy's (no contraction, IEEE division), 0.3, 0.7 and 0.001 are compared in fp64; only rpn_bbox is rounded to fp32 at the end.
 *  1. If any id is negative, boxes with id < 0 are crowd boxes and only boxes with id > 0 stay (:1235-1241); otherwise all boxes stay,
 *     those with id 0 included.  IoU as compute_iou: maxima and minima that hand a NaN on, a clamp at 0 likewise.
 *  2. An anchor's maximum over the boxes and its FIRST index (np.argmax: the first NaN is a maximum); its maximum over the crowd
 *     (np.amax).  -1 where the maximum < 0.3 and, with a crowd, the crowd's maximum < 0.001 (:1265); then every box's best anchor --
 *     the first anchor of its largest IoU, anchor 0 for a box that overlaps nothing -- becomes 1 (:1269); then 1 where the maximum
 *     >= 0.7 (:1271).  Where no box stays (the reference raises) every maximum counts as 0 and there is no positive.
 *  3. Of more than T / 2 positives the T / 2 with the smallest keys[0] stay and the others become 0; then of more than T - n_pos
 *     negatives the T - n_pos with the smallest keys[1] stay (:1275-1288).  Key order is the usual monotone image of the float's bits;
 *     equal keys keep the lower anchor.
 * Results: rpn_match int32 [A]; rpn_bbox fp32 [T, 4]: row k holds the deltas of the k-th positive anchor in anchor order against the
 * box of its arg-max (:1295-1320: a zero-height box gives -inf), divided by std_dev, +0.0 behind n_pos; rows int32 [T]: the anchor of
 * every row, -1 behind n_pos; counts int32 [2] = (n_pos, n_neg) after sampling.  Every element is written: nothing needs clearing.
 * Nothing is differentiable.  Eight dependent launches on `stream`, no [A, G] matrix, integer atomics only: two calls on the same
 * inputs give the same bits; log is the only operation whose last bit may differ from a CPU run.  Nothing is copied to the host.
 * Workspace: query first; 16-byte aligned, as anchors and rpn_bbox.  SDN_EINVAL with a message, before any launch, for sizes outside
 * the ranges above, NULL or misaligned pointers and a workspace that is too small. */
int sdn_rpn_targets_workspace_bytes(int A, int G, int T, size_t* out);
int sdn_rpn_targets(const double* anchors, const void* gt_class_ids, const void* gt_boxes, const float* keys, int A, int G,
                    int ids_int64, int boxes_int32, const int32_t* gt_count, int T, const double* std_dev, int32_t* rpn_match,
                    float* rpn_bbox, int32_t* rows, int32_t* counts, void* workspace, size_t workspace_bytes, sdnStream stream);

/* The training item of Mask R-CNN for one image (csrc/training_item.hip): what Dataset.__getitem__ (geometric/maskrcnn/model.py:1371-1409)
 * makes on the host through load_image_gt (:1154-1211) -- utils.resize_image (utils.py:272-320: scipy.misc.imresize of a uint8 RGB
 * frame = Pillow's BILINEAR resize), resize_mask (:323-335: ndimage.zoom(order=0) and np.pad), np.fliplr (model.py:1189-1190),
 * extract_bboxes (utils.py:26-49), minimize_mask (:338-353) and mold_image (model.py:2196-2201) -- and the division of the boxes by the
 * image shape (:1790-1794).  sdn_training_item_image is its image half alone, for B frames of one size: mold_inputs (:2046-2082).
 * All pointers but plan_host are DEVICE memory.  frames uint8 [B, H, W, 3]; plan_host / plan: the parameter block (csrc/
 * training_item_check.h: TriPlan, 24 ints, then the tables it names by offset: Pillow's bounds and fixed-point coefficients W -> ow and
 * H -> oh, absent for a pass Pillow skips; the source row of every resized row and the source column of every resized column of
 * ndimage.zoom, -1 where it yields the constant 0; fp32(fp64(byte) - MEAN_PIXEL[c]) as a [3][256] table) in HOST memory, read and
 * checked during the call, and its copy on the device, n_plan ints each.  inst_map int32 [H, W] (map_rgb 0) or uint8 [H, W, 3]
 * (map_rgb 1: the id of a pixel is r << 16 | g << 8 | b); ids int32 [G], 1 <= G <= 128: instance g is inst_map == ids[g].
 * The colour jitter of the plan is applied to the frame's pixels before the resize; the horizontal pass is rounded to bytes, then the
 * vertical pass; the zero padding comes first and the padded image and masks are mirrored then (flip).  Results: image fp32
 * [B, 3, M, M]; gt_boxes_int int32 [G, 4] = (y1, x1, y2, x2), first and last + 1 row and column of the instance in the padded,
 * mirrored frame, zeros for an instance without a pixel; gt_boxes the same as fp32; gt_boxes_norm = gt_boxes / M in fp32; areas int32
 * [G]: the instance's pixels; bad int32 [1]: the instances without a pixel (minimize_mask raises there); gt_masks fp32 0 / 1:
 * [G, mini_h, mini_w] with use_mini_mask -- bytescale of the crop (0 / 255; all 0 for a crop whose every pixel is set, where
 * cmax == cmin), Pillow's BILINEAR resize of the crop with the coefficients computed on the device in fp64 (precompute_coeffs,
 * normalize_coeffs_8bpc) and >= 128; all zero for an instance without a pixel -- or [G, M, M] without: the mask itself.
 * M <= 1024, W <= 4096, mini_h and mini_w <= 56, H W <= 2^21 with a contrast op.  Every element is written: nothing needs clearing.
 * Launches on `stream`: one more with a contrast op (the frame's luma mean), the image, then for the item the boxes and the masks.
 * Integer atomics only: two calls on the same inputs give the same bits.  Nothing is copied to the host.  Workspace: query first
 * (G = 0 for the image alone); 16-byte aligned.  SDN_EINVAL with a message, before any launch, for sizes outside these ranges, a
 * plan that does not fit them or the frame, NULL or misaligned pointers and a workspace that is too small. */
int sdn_training_item_workspace_bytes(int B, int H, int W, int G, size_t* out);
int sdn_training_item_image(const uint8_t* frames, int B, int H, int W, const int32_t* plan_host, const int32_t* plan, long n_plan,
                            void* workspace, size_t workspace_bytes, float* image, sdnStream stream);
int sdn_training_item(const uint8_t* frame, const void* inst_map, int map_rgb, const int32_t* ids, int H, int W, int G,
                      const int32_t* plan_host, const int32_t* plan, long n_plan, int use_mini_mask, int mini_h, int mini_w,
                      void* workspace, size_t workspace_bytes, float* image, int32_t* gt_boxes_int, float* gt_boxes,
                      float* gt_boxes_norm, float* gt_masks, int32_t* areas, int32_t* bad, sdnStream stream);

/* The RPN's outputs over all pyramid levels (csrc/rpn_outputs.hip): what RPN.forward does after its convs on every level,
 * geometric/maskrcnn/model.py:896-911 -- permute(0, 2, 3, 1).contiguous().view of the class map (:897-899) and of the box map
 * (:909-911), the softmax over (bg, fg) (:902) -- and the three torch.cat(dim=1) over the levels in MaskRCNN.predict (:1729-1740).
 * class_maps / bbox_maps: L pointers in host memory (1 <= L <= 8), level l fp32 [B, 2k, H[l], W[l]] / [B, 4k, H[l], W[l]] contiguous
 * NCHW on the device, as conv_class / conv_bbox emit them; k anchors per location (1 <= k <= 16), B images (1 <= B <= 65535).  With
 * A = k * sum_l H[l] W[l]: rpn_class_logits fp32 [B, A, 2], rpn_probs fp32 [B, A, 2], rpn_bbox fp32 [B, A, 4].  Level l starts at
 * anchor k * sum_{m<l} H[m] W[m]; in a level, anchor (y * W + x) * k + a, component j, is channel a * 2 + j (boxes: a * 4 + j) at pixel
 * (y, x).  Logits and boxes are copies, bit for bit; rpn_probs is exp(x_j - max(x_0, x_1)) / (e_0 + e_1) in fp32, a non-finite logit
 * following the formula ((+inf, x), (-inf, -inf) and a NaN give NaN twice, as torch's softmax).
 * _fwd, ONE launch: every output element is written once; no memset, no atomics, no workspace.  The maps need 4-byte alignment only
 * (views into a larger buffer are fine), the three outputs 16 bytes.
 * _bwd, ONE launch: grad_logits, grad_probs, grad_bbox (shapes of the outputs; each may be NULL and then counts as zero without being
 * read) and the saved rpn_probs (read only beside grad_probs) -> grad_class_maps / grad_bbox_maps, L pointers each, every element of
 * the 2L gradients written once: the boxes' is the transposed copy, the classes' g_logit_j + p_j * (g_p_j - (g_p_0 p_0 + g_p_1 p_1)),
 * which without grad_probs is the transposed copy of grad_logits.  The same bits every run.
 * SDN_EINVAL with a message, before any launch, for L, k or B outside these ranges, a level with H or W < 1, B * A * 4 not below 2^31,
 * NULL pointers (but the three gradients) and misaligned ones.  Nothing is copied to the host. */
int sdn_rpn_outputs_fwd(const float* const* class_maps, const float* const* bbox_maps, const int* H, const int* W, int L, int k, int B,
                        float* rpn_class_logits, float* rpn_probs, float* rpn_bbox, sdnStream stream);
int sdn_rpn_outputs_bwd(const float* grad_logits, const float* grad_probs, const float* grad_bbox, const float* rpn_probs, const int* H,
                        const int* W, int L, int k, int B, float* const* grad_class_maps, float* const* grad_bbox_maps, sdnStream stream);

/* The Derenderer's heads (csrc/derender_heads.hip): net.fc, ReLU, the cat with the two roi vectors, fc1, ReLU, fc2, ReLU, _fc3, the
 * six slices, the pose pair's normalisation and the class softmax -- geometric/derender3d/models/derenderer.py:27-32 (the layers),
 * :34-43 (the MLP), :45-56 (split, norm :54, softmax :55, view :56) -- and the roi centre / extent arithmetic in front of it,
 * geometric/derender3d/models/__init__.py:70-77.  fp32 throughout; no atomics, no memset, no host copy, no workgroup waits for
 * another; every sum's order follows from the widths alone (a weight gradient's walk over the objects: from the object's index), so
 * the bits are the same every run and object r of a batch gets what it gets alone.
 * Widths: F (pooled features) and Hd (hidden) positive multiples of 4, classes 1 to 16, coeffs >= 1 per class,
 * O = 8 + classes + classes * coeffs, n = 1 to 65535 objects; every element count below 2^31.  w0 [Hd, F], w1 [Hd, Hd + 4],
 * w2 [Hd, Hd], w3 [O, Hd] and their biases: nn.Linear's own tensors, read in place.
 * _fwd, FOUR launches (one per layer).  pooled fp32 [n, F]; the roi vectors as roi_norms [n, 4] -- then centre = (br + tl) / 2 and
 * extent = br - tl, bit-equal to torch, are written to centre_out / extent_out [n, 2] -- or as centre and extent [n, 2] (then
 * centre_out / extent_out are NULL).  out [n * O]: _theta_deltas [n, 2] = row[:, 0:2] / sqrt(r0^2 + r1^2) (a zero pair gives NaN, as
 * the formula does), _translation2ds [n, 2], _log_scales [n, 3], _log_depths [n, 1], _class_probs [n, classes] = expf(x - max) / sum
 * (one expf per element; a non-finite logit follows the formula), _ffd_coeffs [n, classes, coeffs], one after the other, each
 * contiguous.  row (may be NULL): _fc3's own output [n, O].  saved [n * (3 Hd + 1)]: the three post-ReLU activations [n, Hd] and the
 * pose pair's norm [n], for _bwd.  The weights need 16-byte alignment, everything else 4.
 * _bwd, at most FOUR launches.  The six output gradients in out's order, any of which may be NULL (not read, no zeros made); pooled,
 * centre, extent (the forward's centre_out / extent_out in the roi_norms form), the four weights, the forward's out and saved.  It
 * undoes the normalisation, (g - d (d.g)) / norm, and the softmax, p (g - sum p g), and writes g_pooled [n, F], the four weight and
 * the four bias gradients, each only if its pointer is given and every element once; what nobody asks for is not computed.
 * workspace: sdn_derender_heads_workspace_bytes(n, F, Hd, classes, coeffs), 16-byte aligned, not cleared by the caller.
 * SDN_EINVAL with a message, before any launch, for widths outside these ranges, both roi forms or neither, NULL or misaligned
 * pointers and a workspace that is too small. */
int sdn_derender_heads_workspace_bytes(int n, int F, int Hd, int classes, int coeffs, size_t* bytes);
int sdn_derender_heads_fwd(const float* pooled, const float* roi_norms, const float* centre, const float* extent, const float* w0,
                           const float* b0, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                           const float* b3, int n, int F, int Hd, int classes, int coeffs, float* out, float* centre_out,
                           float* extent_out, float* row, float* saved, sdnStream stream);
int sdn_derender_heads_bwd(const float* g_theta, const float* g_trans, const float* g_scales, const float* g_depths, const float* g_probs,
                           const float* g_ffd, const float* pooled, const float* centre, const float* extent, const float* w0,
                           const float* w1, const float* w2, const float* w3, const float* out, const float* saved, int n, int F, int Hd,
                           int classes, int coeffs, float* g_pooled, float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2,
                           float* g_b2, float* g_w3, float* g_b3, void* workspace, size_t workspace_bytes, sdnStream stream);

/* ==== launch lists: one host call per conv-chain pass ===========================================================================
 * In the reference one pass over a network is `self.model(input)` (textural/models/networks.py:238-239, 306-308, 395-407)
 * and `loss.backward()` (textural/train.py:88-95): PyTorch walks the module list / the autograd graph and launches
 * kernel after kernel.  Here a pass of a conv chain is 50-400 launches of the entry points above whose scalar arguments
 * depend only on the chain and the input shape.  The host plans them ONCE into an array of sdn_op records and replays the
 * array with one call per pass: sdn_program_run resolves every record's pointer arguments from a caller-built table of
 * DEVICE pointers (`slots`), and calls the launcher the record names -- the very entry points of this header, in array
 * order, each on the main or the side stream.  Nothing is fused or re-ordered: a program is the launch sequence, stored.
 *
 * Record layout: code = SDN_OP_*; stream 0 = main, 1 = side; buf[k] = slot index of the k-th pointer argument of that
 * entry point (in declaration order, -1 = NULL); i[] / f[] / l[] = its int / float / long-or-size_t arguments in declaration
 * order; taps = byte offset of the op's `int8 dy[ntaps], dx[ntaps]` pair in the program's tap blob (or -1).  Conv records
 * may carry their algorithmic GFLOP (true channel counts) in f[3] for the timing slots (sdn_timing_declare_work). */
typedef struct sdn_op {
    int32_t code, stream;
    int32_t buf[8];
    int32_t i[40];
    float f[4];
    int64_t l[2];
    int32_t taps, reserved;
} sdn_op;

enum {
    SDN_OP_CONV_GEMM = 1,     /* sdn_conv_gemm: buf in,out,w_packed,bias,stats,workspace; i N,IH,IW,Cip,OH,OW,Cop,QH,QW,istride,
                                 ostride,py,px,ntaps,pad_mode,in_relu,Kp,w_rows,act,accumulate,precision; l workspace_bytes */
    SDN_OP_CONV_NARROW_FWD,   /* sdn_conv_narrow_fwd: buf in,out,w_dense,bias; i N,IH,IW,Cip,QH,QW,Cop,rows_used,KH,KW,dy_min,
                                 dx_min,pad_mode,in_relu,act */
    SDN_OP_IN_APPLY,          /* sdn_in_apply: buf z,stats,mr,res,out2,running_mean,running_var,planes; i N,HW,C,Cp,act,res_relu,
                                 planes_relu; f eps,momentum; l plane_stride */
    SDN_OP_IN_BWD,            /* sdn_in_bwd: buf g,stored,mr,sums,planes; i N,HW,Cp,mode; l plane_stride */
    SDN_OP_ACT_BWD,           /* sdn_act_bwd: buf g,y,bias_grad,planes; l npos,plane_stride; i Cp,act */
    SDN_OP_REFLECT_FOLD,      /* sdn_reflect_fold: buf gp,out; i N,H,W,Cp,pad,accumulate */
    SDN_OP_CONV_WGRAD,        /* sdn_conv_wgrad: buf rows,gath,dw,workspace; i N,QH,QW,Cr,GH,GW,Cc,istride,ntaps,pad_mode,
                                 relu_rows,relu_gath,splits,precision; l workspace_bytes */
    SDN_OP_CONV_WGRAD_NARROW, /* sdn_conv_wgrad_narrow: buf rows,gath,dw; i N,QH,QW,Cr,rows_used,GH,GW,Cc,ntaps,pad_mode,
                                 relu_rows,relu_gath */
    SDN_OP_PACK_WEIGHTS,      /* sdn_conv_pack_weights: buf w,tapidx,packed; i R,C,ntaps,Ccp,Kp,rows; l sr,sc */
    SDN_OP_UNPACK_GRAD,       /* sdn_conv_unpack_grad: buf dw,tapidx,grad_w; i R,C,ntaps,Ccp,accumulate; l sr,sc */
    SDN_OP_MEMSET,            /* hipMemsetAsync(buf[0], 0, l[0] bytes) */
    SDN_OP_COPY,              /* hipMemcpyAsync(buf[0] <- buf[1], l[0] bytes, device to device) */
    SDN_OP_ADD,               /* buf[0][k] = buf[1][k] + buf[2][k], k < l[0] floats (l[0] % 4 == 0; gradient of a tensor read twice) */
    SDN_OP_COLSUM,            /* buf[1][c] = sum over l[0] rows of buf[0][row, c], c < i[1], row pitch i[0] floats, in a fixed
                                 order (bias gradients in deterministic mode) */
    SDN_OP_FORK,              /* the side stream waits for everything enqueued on the main stream so far */
    SDN_OP_JOIN,              /* the main stream waits for everything enqueued on the side stream so far */
    SDN_OP_SPLIT_PLANES,      /* sdn_split_planes: buf x,planes; l n,plane_stride; i relu */
    SDN_OP_PACK_WEIGHTS_KMAJOR, /* sdn_conv_pack_weights_kmajor: buf w,tapidx,packed; i R,C,ntaps,Ccp,rows; l sr,sc */
    SDN_OP_CONV_TILE,         /* sdn_conv_tile: buf in_planes,out,out_planes,w_kmajor,bias,stats; l plane_stride,out_plane_stride;
                                 i N,IH,IW,Cip,planes_relu,OH,OW,Cop,QH,QW,istride,ostride,py,px,ntaps,pad_mode,w_rows,act,accumulate,ksplit */
    SDN_OP_CONV_HALO,         /* sdn_conv_halo: buf in_planes,out,w_kmajor,bias,stats; l plane_stride;
                                 i N,IH,IW,Cip,OH,OW,Cop,ntaps,pad_mode,w_rows,act,accumulate */
    SDN_OP_CONV_WGRAD_TILE,   /* sdn_conv_wgrad_tile: buf rows_planes,gath_planes,dw; l rows_stride,gath_stride;
                                 i N,QH,QW,Cr,GH,GW,Cc,istride,ntaps,pad_mode */
    SDN_OP_CONV_GEMM_PHASES,  /* sdn_conv_gemm_phases: buf in,out,w_packed[0..3],bias,stats; i N,IH,IW,Cip,OH,OW,Cop,istride,ostride,
                                 nphase,pad_mode,in_relu,w_rows,act,accumulate,precision, then per phase k: i[16+6k ..] = QH,QW,py,px,
                                 ntaps,Kp; taps = offset of the phases' concatenated (dy, dx) lists */
    SDN_OP_CONV_HEAD_MFMA,    /* sdn_conv_head_mfma: buf in,out,w_frag,bias,stats; i N,IH,IW,Cip,QH,QW,Cop,rows_used,KH,KW,dy_min,dx_min,
                                 pad_mode,in_relu,act */
    SDN_OP_CONV_WGRAD_HEAD,   /* sdn_conv_wgrad_head_mfma: the record of SDN_OP_CONV_WGRAD_NARROW */
    SDN_OP_CODES
};

typedef struct sdn_program sdn_program;
/* Copies the records and the tap blob (HOST memory) and validates codes, slot indices and tap offsets. */
int sdn_program_create(const sdn_op* ops, int n_ops, const int8_t* taps, size_t tap_bytes, int n_slots, sdn_program** out);
/* Replays the program.  slots: HOST array of n_slots DEVICE pointers.  side may equal main (one stream; FORK / JOIN are then
 * no-ops).  op_ms: NULL, or a HOST array of n_ops floats: every record is then bracketed by events on its stream, the call
 * synchronises both streams and reports each record's duration in milliseconds (a measurement mode, never the timed path).
 * On failure *failed_op (may be NULL) is the index of the record whose launcher returned the error. */
int sdn_program_run(const sdn_program* prog, void* const* slots, int n_slots, sdnStream main, sdnStream side, float* op_ms,
                    int* failed_op);
int sdn_program_destroy(sdn_program* prog);

/* ---- measurement aid (bench.py): when enabled, every sdn_rasterize_fwd brackets its k_raster_tiles launch with a
 * hipEvent pair on the launch stream; sdn_timing_read synchronises them, returns the summed kernel time and the
 * number of launches since the last read, and clears the list.  Off by default; process-wide. */
int sdn_timing_enable(int enable);
int sdn_timing_read(double* ms_total, long* launches);
/* the same for any timed kernel family: slot 0 k_raster_tiles, 1 the silhouette edge-gradient kernels, 2 the MFMA forward /
 * data-gradient kernels (k_conv_gemm, k_conv_tile, k_conv_halo, k_conv_s2), 3 the MFMA weight-gradient kernels (k_conv_wgrad,
 * k_wgrad_tile), 4 the exact-fp32 head kernels (k_conv_narrow_fwd, k_wgrad_narrow), 5 k_raster_tiles_k1, 6 k_unmold_masks and
 * k_scene_gt_masks; *work (may be NULL) receives the summed algorithmic work of the launches (flops for the conv slots, 0 for
 * the raster slots, bytes of the planes for slot 6). */
int sdn_timing_read_slot(int slot, double* ms_total, long* launches, double* work);
/* The conv launchers compute their work from the PADDED channel counts they are handed.  A caller that knows the layer's
 * true channel counts declares the work (flops) of the next timed launch this thread issues; sdn_program_run does so for
 * every record whose f[3] is non-zero (f[3] = the record's algorithmic GFLOP). */
int sdn_timing_declare_work(double work);

#ifdef __cplusplus
}
#endif
#endif /* SDN_HIP_H */
