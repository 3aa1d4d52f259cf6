/*
 * nr_hip.h -- C ABI of libnr_hip.so: the MI355X (gfx950) rasterizer hot path of neural_renderer.
 *
 * Drop-in boundary.  The reference launches its stages through
 *     chainer.cuda.elementwise(in_params, out_params, body, name)(loop, *arrays)
 * i.e. CuPy's ElementwiseKernel FFI: raw device arrays + constants pasted into the source, launched
 * asynchronously on the current stream.  Each entry point below replaces one such launch site and is
 * named after the reference method that owns it (reference = /root/reference/neural_renderer/rasterize.py):
 *
 *   nr_forward_face_index_map    <- Rasterize.forward_face_index_map_gpu   rasterize.py:94-359  (K1+K2)
 *   nr_forward_texture_sampling  <- Rasterize.forward_texture_sampling      rasterize.py:361-438 (K4)
 *                                   + forward_background_gpu / forward_alpha_map_gpu  :440-465   (K5)
 *   nr_backward_pixel_map        <- Rasterize.backward_pixel_map_gpu        rasterize.py:517-748 (K6)
 *   nr_backward_textures         <- Rasterize.backward_textures_gpu         rasterize.py:750-792 (K7)
 *   nr_backward_depth_map        <- Rasterize.backward_depth_map_gpu        rasterize.py:794-847 (K8)
 *   nr_forward_rasterize         <- Rasterize.forward_gpu  (K1+K2 -> K4+K5 fused) rasterize.py:467-513
 *   nr_backward_rasterize        <- Rasterize.backward_gpu (K6 -> K7 -> K8 fused)  rasterize.py:849-889
 *   nr_vertices_to_faces[_backward] <- vertices_to_faces + its get_item backward    vertices_to_faces.py:4-21
 *   nr_image_epilogue[_backward]  <- transpose + flip + average_pooling_2d of rasterize_rgbad   rasterize.py:953-969
 *   nr_adam_update                <- AdamRule.update_core_gpu                                  optimizers.py:17-34
 *   nr_load_textures              <- load_textures kernel of load_obj(load_texture=True)      load_obj.py:87-144
 *   nr_create_texture_image       <- create_texture_image kernels of save_obj(textures=...)   save_obj.py:32-146
 *   nr_bake_uv_textures[_backward], nr_uv_texture_map: the bake of nr_load_textures as a differentiable step on learnable
 *                                   images (UVTextures); not in the reference
 *   nr_forward_rasterize_uv / nr_backward_uv_images: the same images sampled at every covered pixel instead of baked into
 *                                   cubes (UVImages); not in the reference
 *   nr_forward_rasterize_uv_smooth / nr_backward_uv_images_smooth: the same with a light colour per CORNER of every face,
 *                                   interpolated at the pixel (smooth light on UV images); not in the reference
 *   nr_forward_rasterize_corner / nr_backward_corner_colors: three colours per face, one per corner, interpolated at every
 *                                   covered pixel; nr_vertex_shade_forward/_backward: those colours from per-vertex colours
 *                                   and flat or smooth (vertex-normal) light (VertexColors); not in the reference
 *   nr_frontend_forward/_backward <- fill_back + lighting + look_at/look + perspective + vertices_to_faces
 *                                    of Renderer.render*                                  renderer.py:35-107
 *   nr_frontend_forward_projection / _backward_projection: the same front-end with a calibrated camera (K, R, t,
 *                                    lens distortion) in place of look_at / look + perspective; not in the reference
 *   nr_forward_rasterize_lit / nr_backward_rasterize_lit / nr_frontend_forward_light / _backward_light: the fused
 *                                   rasterizer and front-end with per-face light colours instead of lit, duplicated
 *                                   textures (renderer.py:77-103 with lighting.py:50-51 moved into K4 / K7)
 *
 * Conventions
 *   - plain device pointers (hipMalloc / torch caching allocator memory), C-contiguous, float32 / int32, every buffer
 *     16-byte aligned (hipMalloc gives 256, torch 512: the kernels move maps, textures and workspaces as 16-byte words).
 *     The library does not check this for every entry; the Python package enforces it by copying: every tensor of a
 *     caller and every upstream gradient goes through _lib.dense, which hands a view that is strided or off the grid
 *     over as a contiguous, aligned copy ("Tensor boundary").  Other callers must align themselves;
 *     sizes are int32; near / far / eps are doubles because the reference pastes their Python repr into
 *     the kernel source as double literals (rasterize.py:226-234, 428-433, 737-743).
 *   - the library owns no memory and keeps no state between calls (it reads no environment variable; the one thing it
 *     remembers is which dynamic-LDS limit the driver already granted to a kernel): outputs, residuals and scratch
 *     ("workspace", size from nr_*_workspace_bytes) all belong to the caller.
 *   - every launch goes to `stream` (a hipStream_t passed as void*; NULL = the null stream), is
 *     asynchronous, and never synchronises the device.  Functions are re-entrant and thread-safe.
 *   - return value: 0 on success; < 0 argument error (NR_E_*); > 0 a hipError_t from the launch.
 *     nr_error_string() renders either.
 *   - layouts (B batch, F faces, S raster size, ts texture size):
 *       faces [B,F,3,3] xyz per vertex: x,y in NDC (y up), z = positive camera depth
 *       textures / grad_textures [B,F,ts,ts,ts,3]
 *       face_index_map [B,S,S] int32 (-1 = no face), weight_map [B,S,S,3], depth_map [B,S,S],
 *       face_inv_map [B,S,S,3,3], rgb_map / grad_rgb_map [B,S,S,3], alpha_map / grad_alpha_map [B,S,S],
 *       sampling_index_map [B,S,S,8] int32, sampling_weight_map [B,S,S,8]; row 0 is the BOTTOM row
 *       (the public Python API flips afterwards, rasterize.py:956-960).
 */
#ifndef NR_HIP_H
#define NR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NR_VERSION 600 /* 0.6.0 (additions without a version step: NR_CAMERA_PROJECTION, nr_projection and
                          *        nr_frontend_{forward,backward}_projection, nr_frontend_projection_workspace_bytes;
                          *        nr_bake_uv_textures[_backward], nr_uv_texture_map[_workspace_bytes]; nr_uv_images,
                          *        nr_forward_rasterize_uv, nr_backward_uv_images[_workspace_bytes];
                          *        nr_corner_light, nr_forward_rasterize_uv_smooth, nr_backward_uv_images_smooth[_workspace_bytes];
                          *        nr_forward_rasterize_corner, nr_backward_corner_colors[_workspace_bytes],
                          *        nr_vertex_shade_forward, nr_vertex_shade_backward, nr_vertex_shade_workspace_bytes;
                          *        NR_FLAG_SHARED_TEXTURES, nr_backward_textures_shared[_workspace_bytes];
                          *        nr_laplacian_forward, nr_laplacian_backward, nr_flatness_forward, nr_flatness_backward,
                          *        nr_mesh_loss_workspace_bytes;
                          *        nr_edge_length_forward, nr_edge_length_backward, nr_cot_weights, nr_cot_apply;
                          *        nr_lights, nr_lights_grad, nr_light_colors_forward, nr_light_colors_backward,
                          *        nr_light_colors_workspace_bytes;
                          *        nr_iou_loss_forward, nr_iou_loss_backward, nr_squared_error_forward, nr_squared_error_backward,
                          *        nr_image_loss_workspace_bytes;
                          *        nr_ssim_loss_forward, nr_ssim_loss_backward, nr_ssim_workspace_bytes;
                          *        nr_stencil_apply;
                          *        nr_vertex_normals_forward, nr_vertex_normals_backward, nr_face_normals_forward,
                          *        nr_face_normals_backward, nr_corner_normals_forward, nr_corner_normals_backward,
                          *        nr_normals_workspace_bytes;
                          *        nr_soft_silhouette_forward, nr_soft_silhouette_backward, nr_soft_silhouette_workspace_bytes;
                          *        nr_soft_render_forward, nr_soft_render_backward, nr_soft_render_workspace_bytes;
                          *        nr_soft_corners_forward, nr_soft_corners_backward, nr_soft_corners_workspace_bytes;
                          *        nr_soft_uv_forward, nr_soft_uv_backward, nr_soft_uv_workspace_bytes;
                          *        nr_soft_cubes_forward, nr_soft_cubes_backward, nr_soft_cubes_workspace_bytes;
                          *        nr_point_mesh_points_to_faces, nr_point_mesh_faces_to_points, nr_point_mesh_loss,
                          *        nr_point_mesh_backward_points, nr_point_mesh_backward_vertices, nr_point_mesh_workspace_bytes;
                          *        nr_winding_forward, nr_winding_backward_points, nr_winding_backward_vertices,
                          *        nr_winding_workspace_bytes;
                          *        nr_ray_mesh_first_hit, nr_ray_mesh_any_hit, nr_ray_mesh_workspace_bytes;
                          *        nr_isosurface_count, nr_isosurface_emit, nr_isosurface_workspace_bytes);
                          *        K6's two arithmetic modes on ONE band kernel for every call size (k_bpm_row: a line record per 16 lanes,
                          *        the sums of a record on the matrix pipe in double); NR_FLAG_K6_PX is ignored;
                          * 0.5.0: K6's default mode on the lane-parallel band kernel (k_bpm_px; NR_FLAG_K6_LEGACY keeps k_bpm_fast); the
                          *        measurement hook nr_profile_band_kernel left the product ABI (include/nr_hip_profile.h, libnr_hip_prof.so);
                          * 0.4.1: NR_FLAG_SERIAL_BACKWARD (the fused backward's gather shares a launch with K6's line setup);
                          * 0.4.0: NR_FLAG_EXACT_GRADIENT and NR_FLAG_K6_SCAN combine (one band kernel, two arithmetic modes);
                          *        NR_FLAG_SPARSE_WEIGHT_MAP;
                          * 0.3.0: any `near` (NR_E_NEAR removed); 0.2.0: faces_z_ref, visible_faces, flags on the K6 entry points */

/* argument errors */
#define NR_E_NULL (-1)      /* a required pointer is NULL */
#define NR_E_SIZE (-2)      /* a size is out of range (B,F,S < 1, B > 65535, S > 16384, ts < 2, index overflow) */
#define NR_E_WORKSPACE (-3) /* workspace missing or too small */
#define NR_E_MODE (-4)      /* nothing to do / inconsistent optional arguments */
/* (-5 was NR_E_NEAR up to 0.2.0: `near` may be any number now, as in the reference, rasterize.py:331) */
#define NR_E_INDEX (-6)     /* a vertex index outside [0, num_vertices) */

/* flags */
#define NR_FLAG_FIX_TEXTURE_BATCH_Z 1 /* texture sampling (K4 / K7): read the face's z from the pixel's own batch element
                                         instead of batch 0 (the reference reads batch 0: rasterize.py:389) */
#define NR_FLAG_EXACT_GRADIENT 2      /* K6: every per-pixel term with the reference's arithmetic (its operations one by one, IEEE
                                         division, the double `dist +- eps`), all sums in double: bit-identical terms, bound 2e-6
                                         against the exactly summed reference terms.  Default (flag clear): float terms through
                                         fused multiply-adds and v_rcp_f32, ~1 ulp per term: within the north star's 1e-4 of the
                                         exactly summed reference terms (measured <= 5e-5 on the BASELINE configurations) -- plus,
                                         on entries that cancel down to 1e-3 of the largest gradient, where one ulp of a large
                                         term counts as 1.2e-4, twice the reference's own float-summation noise (worst scene of a
                                         soak built to cancel: 1.8e-4 where the reference's own sums are 7e-4 off).  Same sweep
                                         structure either way; what the modes cost and measure:
                                         profiles/<round>_parity_summary.md, DESIGN.md 3.
                                         REPRODUCIBILITY (since 0.6.0): both modes return the same grad_faces bits from call to
                                         call, for a batch and its shards, and for fused and staged calls wherever k_bpm_row runs
                                         (raster <= 1024): a record's sums have a fixed order and everything above is added in
                                         double.  NR_FLAG_K6_LEGACY / the scan path in the default mode (k_bpm_fast: float run sums
                                         grouped by arrival) agree to ~1.2e-5 of the largest gradient between two calls. */
#define NR_FLAG_K6_GLOBAL 4           /* K6: force the global-memory kernel that otherwise only serves rasters whose band
                                         does not fit in LDS (a testing aid) */
#define NR_FLAG_K6_SCAN 8             /* K6: let every band workgroup derive its lines from the image's visible-face list
                                         itself, the path that otherwise only serves images whose line records exceed the
                                         workspace's record buffer (a testing aid) */

#define NR_FLAG_ZBUF_EPOCH 16          /* nr_forward_rasterize: the forward workspace is KEPT by the caller between calls (same
                                         sizes, same stream order) and this call's epoch number is in bits 8..15 of `flags`
                                         (0..254): the z-buffer is neither filled before nor cleaned after the call -- a word
                                         written under a larger epoch number loses every atomic minimum against this call's
                                         and reads as empty.  Contract: fill the workspace with 0xff bytes once, then call with
                                         epochs 254, 253, ..., 0; fill again before starting over (or call without the flag,
                                         which fills).  Needs num_faces < 2^24 (ignored otherwise).  Saves the 8 B / pixel fill
                                         of every forward (7 us and 33.5 MB at the headline size). */
#define NR_ZBUF_EPOCH_FLAGS(e) (NR_FLAG_ZBUF_EPOCH | (((e) & 0xff) << 8))
#define NR_FLAG_SPARSE_WEIGHT_MAP 32   /* nr_forward_rasterize: weight_map is written for the pixels a face covers only; the
                                         elements of uncovered pixels (zeros in the reference, rasterize.py:479) are left as
                                         they are.  For callers that keep weight_map as a residual of the backward -- which
                                         reads it at covered pixels only -- and do not hand it out: 7 of 8 pixels of a teapot
                                         view are uncovered (44 of the map's 50 MB at the headline size). */
#define NR_FLAG_SERIAL_BACKWARD 64     /* nr_backward_rasterize[_lit]: K6's line setup, its band kernel and the K7 / K8 gather as
                                         launches of their own, one after the other -- the order every call of more than 96 k
                                         faces (batch x faces) takes anyway.  Smaller calls with texture_size <= 13 put the
                                         gather and the zeros of grad_textures into ONE launch with the line setup, in front of
                                         the band kernel (both only need the visible-face lists), and add K6's sums onto
                                         grad_faces last.  Same values: one float addition per element of grad_faces either
                                         way; a testing / measuring aid. */

#define NR_FLAG_K6_LEGACY 128          /* K6, either arithmetic mode: the piece-per-lane band kernel of rounds 3-4 (k_bpm_fast) instead of
                                         k_bpm_row.  A testing / measuring aid: same sweeps, terms rounded (default mode) and summed
                                         another way (both within the mode's bound of the oracle). */
#define NR_FLAG_K6_PX 65536              /* accepted and ignored since 0.6.0 (it forced round 5's lane-parallel kernel, whose place
                                         k_bpm_row has taken for every call: both arithmetic modes have one band kernel -- 16 lanes
                                         per line record, four records per wave instruction -- wherever its band fits the LDS
                                         (raster <= 1024; the default mode: eps > 0); the scan path, larger rasters and the default
                                         mode with eps = 0 run on k_bpm_fast).  Which kernel a call takes does not depend on its
                                         batch size. */
#define NR_FLAG_SHARED_TEXTURES 131072   /* nr_forward_rasterize[_lit]: `textures` is ONE set of cubes, [Nf, ts,ts,ts, 3], for all B images
                                         (texture batch stride 0; Nf as the call says: F, or lit->texture_faces).  Same arithmetic
                                         as on B copies of it: bit-identical maps.  Its texture gradient, summed over the images,
                                         is nr_backward_textures_shared's; nr_backward_rasterize[_lit] gives grad_faces for such a
                                         call with grad_textures == NULL.  Every entry point that strides cubes by the batch and is
                                         handed the flag -- nr_forward_texture_sampling, nr_backward_textures, nr_backward_rasterize[_lit]
                                         with grad_textures -- returns NR_E_MODE. */

/*
 * faces_z_ref (nr_forward_texture_sampling, nr_forward_rasterize, nr_backward_textures, nr_backward_rasterize):
 * the reference samples textures with the vertex depths of BATCH ELEMENT 0 (`&faces[face_index * 9]`, rasterize.py:389,
 * SURVEY Q1).  NULL = batch element 0 of `faces`, i.e. the reference's behaviour for a call that holds the whole
 * batch.  A caller that holds only a SHARD of the batch (views [start, stop) on one GPU) passes the [F,3,3] faces of
 * the GLOBAL batch element 0 here (device memory; neural_renderer_amd.distributed.broadcast_reference_faces), so that
 * sharded and unsharded runs give identical bits.  Ignored when NR_FLAG_FIX_TEXTURE_BATCH_Z is set.
 *
 * visible_faces (uint8 [B,F], optional everywhere): 1 for every face that owns at least one pixel of its image.  The
 * forward writes every element when the pointer is given; the K6 pipeline starts from it (it otherwise rebuilds the flags
 * with one more pass over face_index_map).  It is a residual like face_index_map: pass back what the forward produced.
 */

int nr_version(void);
const char *nr_error_string(int code);

/* Scratch needed by the forward: the packed 64-bit z-buffer (depth bits << 32 | face index, one word per pixel) and the
 * queue of faces with large screen boxes.  The reference's `faces_inv` scratch (rasterize.py:240) is not materialised. */
size_t nr_forward_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t image_size);

/* Scratch needed by nr_backward_pixel_map / nr_backward_rasterize: per image the sorted list of visible faces, their edge
 * line ranges, face -> list position, six double sums per listed face and the band line records (+ the flags when
 * visible_faces is not passed).  With return_rgb == return_alpha == 0 (a depth-only nr_backward_rasterize: no K6) only the
 * lists are needed and the size is B * F * 4 bytes + a header. */
size_t nr_backward_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t image_size,
                                   int32_t return_rgb, int32_t return_alpha);

/*
 * Visibility (K1+K2, rasterize.py:240-359; tie rule "min depth, then lowest face index").
 * Writes EVERY element of face_index_map (-1 where empty), weight_map (0), depth_map (far) and, when
 * non-NULL, face_inv_map (0) -- the caller need not pre-fill them (the reference does, :478-496).
 * weight_map, depth_map, face_inv_map and visible_faces may each be NULL when the caller does not need them.
 * near / far may be any numbers (rasterize.py:331 pastes them as literals): depths enter the packed z-buffer through an
 * order-preserving integer key, so near <= 0 (faces behind the camera, negative depths) behaves as in the reference.
 */
int nr_forward_face_index_map(const float *faces, int32_t *face_index_map, float *weight_map, float *depth_map,
                              float *face_inv_map, uint8_t *visible_faces, int32_t batch_size, int32_t num_faces,
                              int32_t image_size, double near, double far, void *workspace, size_t workspace_bytes,
                              void *stream);

/*
 * Shading (K4 + K5, rasterize.py:361-465): trilinear sampling of the winning face's texture cube,
 * background blending and alpha.  rgb_map (needs faces, textures, weight_map, depth_map, background)
 * and alpha_map are each optional (NULL = not requested) but at least one must be given.
 * background: 3 floats, or batch_size*3 floats when bg_per_batch != 0 (device memory).
 * sampling_index_map / sampling_weight_map: optional residuals of the reference (:394-395); zero where empty.
 */
int nr_forward_texture_sampling(const float *faces, const float *faces_z_ref, const float *textures,
                                const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                float *rgb_map, int32_t *sampling_index_map, float *sampling_weight_map,
                                const float *background, int32_t bg_per_batch, float *alpha_map, int32_t batch_size,
                                int32_t num_faces, int32_t image_size, int32_t texture_size, double eps, int32_t flags,
                                void *stream);

/*
 * Approximate gradient of rgb / alpha w.r.t. vertex x, y (K6, rasterize.py:517-748).
 * STORES every element of grad_faces [B,F,3,3] (z components and back faces = 0), like the reference
 * (:736 after the zero fill of :851).  rgb_map must be the post-background map.
 * return_rgb / return_alpha select the terms; the matching map and gradient pointers must be non-NULL.
 * flags: NR_FLAG_EXACT_GRADIENT, NR_FLAG_K6_GLOBAL; visible_faces: the forward's flags or NULL.
 */
int nr_backward_pixel_map(const float *faces, const int32_t *face_index_map, const float *rgb_map,
                          const float *alpha_map, const float *grad_rgb_map, const float *grad_alpha_map,
                          float *grad_faces, int32_t batch_size, int32_t num_faces, int32_t image_size, double eps,
                          int32_t return_rgb, int32_t return_alpha, int32_t flags, const uint8_t *visible_faces,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Texture gradient (K7, rasterize.py:750-792): the sum of w * grad_rgb over the 8 taps of every pixel a
 * face owns.  STORES every element of grad_textures [B,F,ts,ts,ts,3] (zeros for faces that own no pixel):
 * the caller's zero fill (:853) is not needed.  faces is always required (screen boxes).  If both sampling
 * maps are given they are used as in the reference; if both are NULL the indices/weights are recomputed
 * from faces, weight_map, depth_map, eps and flags with the forward's arithmetic (saves 64 B/pixel of
 * residuals).
 */
int nr_backward_textures(const int32_t *face_index_map, const float *sampling_weight_map,
                         const int32_t *sampling_index_map, const float *faces, const float *faces_z_ref,
                         const float *weight_map, const float *depth_map, const float *grad_rgb_map, float *grad_textures,
                         int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t texture_size, double eps,
                         int32_t flags, void *stream);

/*
 * Depth gradient (K8, rasterize.py:794-847): ACCUMULATES into grad_faces (run after nr_backward_pixel_map,
 * :881-883).  face_inv_map may be NULL: the per-face inverse is then recomputed from faces with the
 * forward's arithmetic (saves 36 B/pixel of residuals).
 */
int nr_backward_depth_map(const float *faces, const float *depth_map, const int32_t *face_index_map,
                          const float *face_inv_map, const float *weight_map, const float *grad_depth_map,
                          float *grad_faces, int32_t batch_size, int32_t num_faces, int32_t image_size, void *stream);

/*
 * Fused forward = Rasterize.forward_gpu (rasterize.py:467-513): nr_forward_face_index_map followed by
 * nr_forward_texture_sampling, identical results, one resolve pass (the winner is shaded while still in
 * registers).  rgb_map / alpha_map / weight_map / depth_map are each optional (NULL = not requested).
 */
int nr_forward_rasterize(const float *faces, const float *faces_z_ref, const float *textures, int32_t *face_index_map,
                         float *weight_map, float *depth_map, float *rgb_map, float *alpha_map, uint8_t *visible_faces,
                         const float *background, int32_t bg_per_batch, int32_t batch_size, int32_t num_faces,
                         int32_t image_size, int32_t texture_size, double near, double far, double eps, int32_t flags,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused backward = Rasterize.backward_gpu (rasterize.py:849-889): K6, then K7, then K8, identical results to the
 * three stage calls above, sharing the per-image lists of visible faces that K6 builds (the gathers then
 * visit only the faces that own a pixel).  A NULL gradient pointer means "that output has no gradient"
 * (the reference substitutes zeros, :858-878): the corresponding terms are skipped.  STORES every element of
 * grad_faces and, when grad_rgb_map and grad_textures are given, of grad_textures.  Needs weight_map / depth_map
 * when grad_rgb_map or grad_depth_map is given, rgb_map / alpha_map for their gradients; workspace as for
 * nr_backward_pixel_map.  visible_faces (optional): the forward's per-face flags; K6 builds its lists from them, and with
 * only grad_depth_map given (no K6, no lists) the depth gather skips the faces they mark as owning no pixel.
 */
int nr_backward_rasterize(const float *faces, const float *faces_z_ref, const int32_t *face_index_map,
                          const float *weight_map, const float *depth_map, const float *rgb_map, const float *alpha_map,
                          const float *grad_rgb_map, const float *grad_alpha_map, const float *grad_depth_map,
                          float *grad_faces, float *grad_textures, int32_t batch_size, int32_t num_faces,
                          int32_t image_size, int32_t texture_size, double eps, int32_t flags,
                          const uint8_t *visible_faces, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Per-face light colours instead of lit, duplicated textures.  Renderer.render (reference renderer.py:77-103)
 * hands the rasterizer textures that fill_back duplicated (:79, the copy with its first and third cube axis exchanged) and
 * lighting multiplied by one colour per face (lighting.py:50-51): 2 x B x Nf x ts^3 x 3 floats that are written, read back
 * by the few faces that own a pixel, and whose equally large gradient travels the other way.  The _lit entry points take
 * the ORIGINAL cubes plus the per-face colours and do both inside the shading:
 *     rgb(pixel of face f) = light[b, f, :] * sum_taps w * cube(f)[tap]          cube(f) = textures[b, f] for f < Nf,
 *                                                                               textures[b, f - Nf] transposed for f >= Nf
 * which is the reference's value up to the rounding order of the light product (the reference rounds light * texel per
 * texel and sums, this rounds the sum and multiplies: 1 ulp class, <= 2e-7 relative; tests/test_face_light_gpu.py).
 * Every other output is bit-identical (the geometry does not depend on textures).
 *   light [B, F, 3]; texture_faces = Nf with F == Nf or F == 2 * Nf; textures / grad_textures [B, Nf, ts,ts,ts, 3].
 *   backward: grad_textures is the gradient w.r.t. the ORIGINAL cubes (light factor included); grad_light [B, F, 3]
 *   (optional) the gradient of the colours, for nr_frontend_backward_light.  lit == NULL: exactly nr_forward_rasterize /
 *   nr_backward_rasterize.
 */
typedef struct nr_face_light {
    const float *light;     /* DEVICE [B, F, 3] */
    int32_t texture_faces;  /* Nf */
    const float *textures;  /* backward: the cubes again (DEVICE), needed when grad_light is given */
    float *grad_light;      /* backward: DEVICE [B, F, 3] or NULL; every element stored */
} nr_face_light;

int nr_forward_rasterize_lit(const nr_face_light *lit, const float *faces, const float *faces_z_ref, const float *textures,
                             int32_t *face_index_map, float *weight_map, float *depth_map, float *rgb_map, float *alpha_map,
                             uint8_t *visible_faces, const float *background, int32_t bg_per_batch, int32_t batch_size,
                             int32_t num_faces, int32_t image_size, int32_t texture_size, double near, double far,
                             double eps, int32_t flags, void *workspace, size_t workspace_bytes, void *stream);
int nr_backward_rasterize_lit(const nr_face_light *lit, const float *faces, const float *faces_z_ref,
                              const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                              const float *rgb_map, const float *alpha_map, const float *grad_rgb_map,
                              const float *grad_alpha_map, const float *grad_depth_map, float *grad_faces,
                              float *grad_textures, int32_t batch_size, int32_t num_faces, int32_t image_size,
                              int32_t texture_size, double eps, int32_t flags, const uint8_t *visible_faces,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Texture cubes shared by the batch (not in the reference; DESIGN K7 "Shared cubes"): the texture gradient of a forward that ran
 * with NR_FLAG_SHARED_TEXTURES.  grad_textures [Nf, ts,ts,ts, 3] = the sum over the B images of what nr_backward_rasterize[_lit]
 * stores per image -- the reference's per-pixel terms (rasterize.py:780), with lit times light[b, f, :], the reversed copies
 * Nf + f folded into cube f -- and every element is stored (zeros for cubes that own no pixel in any image).  lit == NULL:
 * F cubes, sampled as they are; with lit, lit->texture_faces cubes, and lit->grad_light [B, F, 3] (optional, needs
 * lit->textures = the ONE set of cubes) receives each image's own colour gradient, every element stored.
 * A group of lanes owns one (image, face) pair whose visible_faces flag is set (NULL: every pair), sums the pair's pixels
 * privately (float registers at texture_size 2 with static taps, doubles in LDS otherwise) and adds each texel's sum ONCE, in
 * double, onto the workspace's [Nf, ts^3 * 3] doubles; a second launch rounds them to float.  Nothing grows with B * Nf * ts^3.
 * The double additions of the images arrive in no fixed order, so the last bit of a sum may differ between calls.
 * texture_size in [2, 13] (NR_E_SIZE above: no shared counterpart of the per-pixel scatter); weight_map and depth_map are the
 * forward's; flags: NR_FLAG_FIX_TEXTURE_BATCH_Z as the forward had it.  The size query runs on the host alone and does not
 * depend on batch_size (0 for sizes out of range).  No host synchronisation; capturable.
 */
size_t nr_backward_textures_shared_workspace_bytes(int32_t batch_size, int32_t texture_faces, int32_t texture_size);
int nr_backward_textures_shared(const nr_face_light *lit, const float *faces, const float *faces_z_ref,
                                const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                const float *grad_rgb_map, const uint8_t *visible_faces, float *grad_textures,
                                int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t texture_size, double eps,
                                int32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/*
 * vertices_to_faces (reference neural_renderer/vertices_to_faces.py:4-21): faces_out[b,f,k,:] = vertices[b, faces_idx[.,f,k], :]
 * and its backward (Chainer's get_item backward = scatter-add): grad_vertices[b, faces_idx[.,f,k], :] += grad_faces[b,f,k,:]
 * with hardware float atomics; grad_vertices [B,Nv,3] is zero-filled by the call.  faces_idx is [B,Nf,3] int32 when
 * idx_per_batch != 0, else one [Nf,3] topology shared by the batch.  Indices must lie in [0, Nv): the Python binding checks
 * that (IndexError, like the reference's get_item); the kernels clamp, so a bad index never leaves the buffers.
 */
int nr_vertices_to_faces(const float *vertices, const int32_t *faces_idx, float *faces_out, int32_t batch_size,
                         int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch, void *stream);
int nr_vertices_to_faces_backward(const float *grad_faces, const int32_t *faces_idx, float *grad_vertices,
                                  int32_t batch_size, int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch,
                                  void *stream);

/*
 * Image epilogue of rasterize_rgbad (reference rasterize.py:953-969), one bandwidth-bound kernel per direction:
 * rgb [B,S,S,3] -> [B,3,is,is] (NHWC -> NCHW), alpha / depth [B,S,S] -> [B,is,is], every output flipped vertically
 * (row 0 of the maps is the bottom row, row 0 of the images the top row) and, when anti_aliasing != 0, averaged over
 * 2x2 blocks (is = S/2, S even; else is = S).  Each map / image pair is optional (both NULL = not requested).
 * The backward writes every element of the requested map gradients.
 */
int nr_image_epilogue(const float *rgb_map, const float *alpha_map, const float *depth_map, float *rgb_out,
                      float *alpha_out, float *depth_out, int32_t batch_size, int32_t image_size, int32_t anti_aliasing,
                      void *stream);
int nr_image_epilogue_backward(const float *grad_rgb_out, const float *grad_alpha_out, const float *grad_depth_out,
                               float *grad_rgb_map, float *grad_alpha_map, float *grad_depth_map, int32_t batch_size,
                               int32_t image_size, int32_t anti_aliasing, void *stream);

/*
 * Fused geometry + lighting front-end of Renderer.render / render_silhouettes / render_depth
 * (reference renderer.py:35-107): fill_back (:37-38, :77-79), lighting (lighting.py:8-51), look_at (look_at.py:7-46) or
 * look (look.py:7-45), perspective (perspective.py:5-19) and vertices_to_faces (vertices_to_faces.py:4-21) in one kernel,
 * and their whole backward (including the light -> normal -> vertex path, the face -> vertex scatter and the gradient of
 * the camera position) in one kernel plus a per-image camera kernel.
 *
 *   vertices [B,Nv,3] world space; faces_idx int32 [B,Nf,3] (idx_per_batch != 0) or [Nf,3]; textures [B,Nf,ts,ts,ts,3] or
 *   NULL (silhouette / depth rendering: no lighting); eye: DEVICE pointer, [B,3] (eye_per_batch != 0) or [3];
 *   faces_out [B,F,3,3] with F = Nf * (fill_back ? 2 : 1): face f and, at Nf + f, its copy with reversed vertex order;
 *   textures_out [B,F,ts,ts,ts,3]: textures * light and, at Nf + f, the (i,j,k) -> (k,j,i) transposed textures * the
 *   light of the reversed face.  nr_camera / nr_light live in HOST memory and are read during the call.
 */
#define NR_CAMERA_LOOK_AT 1 /* rotation from eye -> target, target = `at` (look_at.py) */
#define NR_CAMERA_LOOK 2    /* rotation from a fixed viewing direction, target = `direction` (look.py) */

typedef struct nr_camera {
    int32_t mode;        /* NR_CAMERA_LOOK_AT or NR_CAMERA_LOOK */
    int32_t perspective; /* != 0: x/z/width, y/z/width (perspective.py:15-17) */
    float target[3];     /* `at` or `direction` */
    float up[3];
    float width;         /* tan(viewing_angle / 180 * 3.1416), computed by the host in float32 (perspective.py:10-13) */
} nr_camera;

typedef struct nr_light { /* lighting.py:9-13 */
    float intensity_ambient, intensity_directional;
    float color_ambient[3], color_directional[3], direction[3];
} nr_light;

/* Scratch for nr_frontend_backward when grad_eye is requested (per-image camera sums). */
size_t nr_frontend_workspace_bytes(int32_t batch_size);

int nr_frontend_forward(const float *vertices, const int32_t *faces_idx, const float *textures, const float *eye,
                        float *faces_out, float *textures_out, int32_t batch_size, int32_t num_vertices,
                        int32_t num_faces, int32_t texture_size, int32_t idx_per_batch, int32_t eye_per_batch,
                        int32_t fill_back, const nr_camera *camera, const nr_light *light, void *stream);

/*
 * grad_faces [B,F,3,3] and grad_textures_out [B,F,ts,ts,ts,3] (NULL = the lit textures received no gradient) are the
 * gradients of the two outputs.  Each result is optional (NULL = not needed): grad_vertices [B,Nv,3] (zero-filled by the
 * call, accumulated with hardware float atomics), grad_textures [B,Nf,ts,ts,ts,3] (every element stored; needs
 * grad_textures_out), grad_eye [B,3] or [3] (needs grad_vertices and the workspace).  `at`, `up`, `direction`, the
 * viewing angle and the light parameters are constants of the call (no gradients), as in Renderer.
 */
int nr_frontend_backward(const float *vertices, const int32_t *faces_idx, const float *textures, const float *eye,
                         const float *grad_faces, const float *grad_textures_out, float *grad_vertices,
                         float *grad_textures, float *grad_eye, int32_t batch_size, int32_t num_vertices,
                         int32_t num_faces, int32_t texture_size, int32_t idx_per_batch, int32_t eye_per_batch,
                         int32_t fill_back, const nr_camera *camera, const nr_light *light, void *workspace,
                         size_t workspace_bytes, void *stream);

/*
 * The same front-end for the _lit rasterizer entry points: no textures in or out.  light_out [B,F,3] receives the colour of
 * every face (lighting.py:28-47) and of its reversed copy; nr_frontend_backward_light takes the gradient of those colours
 * (grad_light [B,F,3], e.g. from nr_backward_rasterize_lit; NULL = none) in place of grad_textures_out.  The gradient of the
 * textures does not pass through here (nr_backward_rasterize_lit stores it).
 */
int nr_frontend_forward_light(const float *vertices, const int32_t *faces_idx, const float *eye, float *faces_out,
                              float *light_out, int32_t batch_size, int32_t num_vertices, int32_t num_faces,
                              int32_t idx_per_batch, int32_t eye_per_batch, int32_t fill_back, const nr_camera *camera,
                              const nr_light *light, void *stream);
int nr_frontend_backward_light(const float *vertices, const int32_t *faces_idx, const float *eye, const float *grad_faces,
                               const float *grad_light, float *grad_vertices, float *grad_eye, int32_t batch_size,
                               int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch, int32_t eye_per_batch,
                               int32_t fill_back, const nr_camera *camera, const nr_light *light, void *workspace,
                               size_t workspace_bytes, void *stream);

/*
 * Projection camera (Renderer.camera_mode = 'projection', neural_renderer_amd/projection.py; not in the reference): the same
 * front-end -- fill_back, lighting in world space, vertices_to_faces -- with a calibrated camera in place of look_at / look
 * and perspective.  For world-space vertex w of image b, in float32 and in this order:
 *
 *   c   = R[b] w + t[b]                        camera space, OpenCV axes: x right, y down, z forward
 *   x'  = c.x / c.z,  y' = c.y / c.z
 *   r2  = x'^2 + y'^2
 *   rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3        dist_coeffs = (k1, k2, p1, p2, k3), OpenCV order
 *   x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2)
 *   y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y'
 *   u   = K[0,0] x'' + K[0,1] y'' + K[0,2]     row 2 of K is ignored
 *   v   = K[1,0] x'' + K[1,1] y'' + K[1,2]
 *   out = ((2u - orig_size) / orig_size, (orig_size - 2v) / orig_size, c.z)    the rasterizer's NDC (y up) + depth
 *
 * u, v are continuous pixel coordinates of an orig_size^2 image, pixel i spanning [i, i+1): with orig_size == image_size a
 * point at (u, v) = (i + 0.5, j + 0.5) lands on the centre of column i and row j counted from the TOP of the returned image
 * (the photo's row).  OpenCV intrinsics put pixel centres at integers: add 0.5 to cx and cy.  dist_coeffs == NULL: no
 * distortion (those terms are skipped).  Nothing is clamped: c.z <= near is culled by the rasterizer.
 *
 * K, R, t and dist_coeffs are DEVICE arrays, [B,3,3] / [B,3,3] / [B,3] / [B,5] when their *_per_batch != 0, else one
 * [3,3] / [3,3] / [3] / [5] for the whole batch.  The library never reads them on the host, so the calls stay asynchronous
 * and can be captured into a graph.  The nr_projection struct itself lives in HOST memory and is read during the call.
 */
#define NR_CAMERA_PROJECTION 3

typedef struct nr_projection {
    const float *K, *R, *t, *dist_coeffs; /* device pointers; dist_coeffs may be NULL */
    int32_t K_per_batch, R_per_batch, t_per_batch, dist_per_batch;
    float orig_size; /* > 0 */
} nr_projection;

/* Scratch for nr_frontend_backward_projection when grad_K, grad_R or grad_t is requested (per-image sums in double). */
size_t nr_frontend_projection_workspace_bytes(int32_t batch_size);

/*
 * textures / textures_out as in nr_frontend_forward, or light_out [B,F,3] as in nr_frontend_forward_light; the two outputs
 * are mutually exclusive, both NULL = silhouette / depth rendering.  `light` is needed with either.
 */
int nr_frontend_forward_projection(const float *vertices, const int32_t *faces_idx, const float *textures, float *faces_out,
                                   float *textures_out, float *light_out, int32_t batch_size, int32_t num_vertices,
                                   int32_t num_faces, int32_t texture_size, int32_t idx_per_batch, int32_t fill_back,
                                   const nr_projection *projection, const nr_light *light, void *stream);

/*
 * Gradients as in nr_frontend_backward (grad_textures_out + grad_textures) or nr_frontend_backward_light (grad_light; then
 * textures == NULL).  grad_K [B,3,3] or [3,3] (row 2 is 0), grad_R [B,3,3] or [3,3], grad_t [B,3] or [3], shaped like the
 * parameter, are optional and need grad_vertices and the workspace; shared ones are zero-filled and accumulated with float
 * atomics.  dist_coeffs receives no gradient.
 */
int nr_frontend_backward_projection(const float *vertices, const int32_t *faces_idx, const float *textures,
                                    const float *grad_faces, const float *grad_textures_out, const float *grad_light,
                                    float *grad_vertices, float *grad_textures, float *grad_K, float *grad_R, float *grad_t,
                                    int32_t batch_size, int32_t num_vertices, int32_t num_faces, int32_t texture_size,
                                    int32_t idx_per_batch, int32_t fill_back, const nr_projection *projection,
                                    const nr_light *light, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Texture baking of load_obj(load_texture=True) (K10, reference load_obj.py:87-144): for every texel (i0,i1,i2) of every
 * face with is_update[f] != 0, textures[f,i0,i1,i2,:] = bilinear lookup of `image` at the barycentric point
 * (i0,i1,i2)/(i0+i1+i2) of the face's uv triangle.  image [H,W,3] float32 in [0,1], ALREADY flipped vertically (:85);
 * faces_uv [Nf,3,2]; textures [Nf,ts,ts,ts,3] in/out (other faces untouched).  Texel (0,0,0) of an updated face is NaN, as
 * in the reference (0/0); reads outside the image are clamped to the nearest pixel (zero weight when the reference is defined).
 */
int nr_load_textures(const float *image, const float *faces_uv, const int32_t *is_update, float *textures,
                     int32_t num_faces, int32_t texture_size, int32_t image_height, int32_t image_width, void *stream);

/*
 * Learnable UV texture images (not in the reference; DESIGN K10, neural_renderer_amd/uv_textures.py): the bake of
 * nr_load_textures as a differentiable step, for every image of a mesh at once.
 *
 * A UV layout of a mesh with F faces: faces_uv [F,3,2] (wrapped as load_obj does), face_image [F] (which of the M images a
 * face samples; any value outside [0, M) = none), base [F,ts,ts,ts,3] (the texels of faces without an image) and the M image
 * sizes.  The images are packed one after another, each [H_m,W_m,3] float32 with its TOP row first (file orientation; the
 * kernels mirror the row index instead of flipping the image): images [Bi,P,3] with P = sum H_m*W_m, and image_table
 * [M,3] int32 = (first pixel of image m in the packing, H_m, W_m) on the device.  The caller keeps the table consistent
 * with P; the library reads it on the device only.
 *
 * nr_bake_uv_textures: textures [Bi,F,ts,ts,ts,3].  A face with image m takes, at every texel other than (0,0,0), the
 * value nr_load_textures computes from image m flipped vertically, bit for bit (its clamped reads, yi1 = (int)(pos_y + 1)
 * and double literals included).  DEPARTURE from nr_load_textures: texel (0,0,0), NaN there (0/0), is the same bilinear
 * lookup at the uv centroid, with barycentric weights 1/3 in float.  Faces without an image copy `base`.  One launch;
 * no host synchronisation; capturable in a graph.
 */
int nr_bake_uv_textures(const float *images, const int32_t *image_table, const float *faces_uv, const int32_t *face_image,
                        const float *base, float *textures, int32_t batch_size, int32_t num_faces, int32_t texture_size,
                        int32_t num_images, int32_t num_pixels, void *stream);

/*
 * The inverse of the bake, built once per layout: every bilinear read of every texel of a face with an image, grouped by
 * the packed pixel it reads (CSR).  row_ptr [P+1]: the entries of pixel p are [row_ptr[p], row_ptr[p+1]), ordered by
 * (face, texel, corner); entry_texel / entry_weight [4*F*ts^3]: the texel f*ts^3 + t and the weight of that read (the
 * weights nr_bake_uv_textures uses).  Entries from row_ptr[P] on are unused.  Needs 4*F*ts^3 <= 2^31-1, P < 2^31-1 and
 * the workspace of nr_uv_texture_map_workspace_bytes (a stable device radix sort; the query needs a visible device and
 * returns 0 without one or for sizes out of range).  Not on the per-step path: it allocates nothing, but it is not
 * meant for graph capture.
 */
size_t nr_uv_texture_map_workspace_bytes(int32_t num_faces, int32_t texture_size, int32_t num_images, int32_t num_pixels);
int nr_uv_texture_map(const int32_t *image_table, const float *faces_uv, const int32_t *face_image, int32_t *row_ptr,
                      int32_t *entry_texel, float *entry_weight, int32_t num_faces, int32_t texture_size, int32_t num_images,
                      int32_t num_pixels, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Adjoint of nr_bake_uv_textures with respect to the images: grad_images [Bi,P,3] (every pixel written, 0 where no texel
 * reads it) from grad_textures [Bi,F,ts,ts,ts,3] and the map of nr_uv_texture_map.  One thread per (b, pixel) walks the
 * pixel's entries in map order and sums grad * weight in double, rounded once: no atomics, the same bits on every call, and
 * a batch equals its elements one at a time.  No gradient to faces_uv or base.  No host synchronisation; capturable.
 */
int nr_bake_uv_textures_backward(const float *grad_textures, const int32_t *row_ptr, const int32_t *entry_texel,
                                 const float *entry_weight, float *grad_images, int32_t batch_size, int32_t num_faces,
                                 int32_t texture_size, int32_t num_pixels, void *stream);

/*
 * Per-pixel UV texture images (not in the reference; DESIGN K10 "Per-pixel UV images"): the rasterizer samples the images of
 * a UV layout at every covered pixel instead of at the ts^3 texels of a baked cube.  The layout and the images are those of
 * nr_bake_uv_textures (Nf = lit->texture_faces faces; images [image_batch, P, 3], top row first; image_batch = the batch B,
 * or 1 for images shared by the batch: image batch stride 0, no expanded copy).  Per-face light colours are required
 * (lit->light [B, F, 3], F == Nf or F == 2 * Nf as for nr_forward_rasterize_lit); baked lighting has no place in images that
 * many faces share.
 *
 * Forward, at a pixel of batch element b covered by face f with weights w and depth zp (all float32, in this order):
 *   f' = f for f < Nf; for a reversed copy f' = f - Nf, and the weights are taken in reversed corner order (w2, w1, w0);
 *   z   = the three vertex depths of face f in batch element b ITSELF (NR_FLAG_FIX_TEXTURE_BATCH_Z is implied; faces_z_ref
 *         does not apply);
 *   d_k = fminf(fmaxf(w_k * (zp / z_k), 0), 1)            (the cube path's product without the ts - 1 factor);
 *   face f' with image m: the four bilinear reads (q_r, omega_r) of image m at the barycentric point d of faces_uv[f'] that
 *         nr_bake_uv_textures takes at a texel (rows mirrored, reads clamped into the image), c = ((0 + img[q_0] omega_0) +
 *         img[q_1] omega_1) + ... in read order;  face f' without an image: c = the cube path's trilinear sample of base[f']
 *         (with eps, and the transposed cube for a reversed copy);
 *   rgb = (c * light[b, f]) * 1 + 0 * background.
 * Uncovered pixels, alpha, depth, face_index_map, weight_map and visible_faces are exactly nr_forward_rasterize_lit's.
 *
 * Backward (nr_backward_uv_images), for the upstream g = grad_rgb_map, over the covered pixels:
 *   grad_images[b or 0, q_r, :] += g * light[b, f] * omega_r     (faces with an image; shared images sum over the batch)
 *   grad_light[b, f, :]         += g * c                          (every covered pixel; c as in the forward)
 * Every element of grad_images [image_batch, P, 3] and grad_light [B, F, 3] is stored (0 where nothing reads).  No gradient
 * to faces_uv or base.  grad_faces comes from nr_backward_rasterize_lit(NULL, ..., grad_textures = NULL, ...) on the rgb_map
 * of this forward (K6 and K8 read only the maps and the geometry).  Both sums are accumulated in double and rounded once to
 * float: within 1e-6 of the sum of |terms| of the exact adjoint, also where thousands of pixels read one image pixel.  The
 * double additions arrive in no fixed order, so the last bits of a double sum may differ between calls; rounded to float
 * they gave the same bits in every run measured (tests/test_uv_pixel_gpu.py).  rgb_map repeats bit for bit.
 *
 * Neither call synchronises the host or reads device values on the host: both can be captured into a graph.
 */
typedef struct nr_uv_images {
    const float *images;         /* DEVICE [image_batch, num_pixels, 3] */
    const int32_t *image_table;  /* DEVICE [num_images, 3]: first pixel, H, W (as nr_bake_uv_textures) */
    const float *faces_uv;       /* DEVICE [Nf, 3, 2] */
    const int32_t *face_image;   /* DEVICE [Nf]: the image of a face, any value outside [0, num_images) = none */
    const float *base;           /* DEVICE [Nf, ts, ts, ts, 3]: the texels of faces without an image */
    int32_t texture_size, num_images, num_pixels, image_batch;  /* ts in [2, 1024]; image_batch 1 or B */
} nr_uv_images;

/* rgb_map and background are required; lit->light is required; the other arguments as in nr_forward_rasterize_lit. */
int nr_forward_rasterize_uv(const nr_face_light *lit, const nr_uv_images *uv, const float *faces, int32_t *face_index_map,
                            float *weight_map, float *depth_map, float *rgb_map, float *alpha_map, uint8_t *visible_faces,
                            const float *background, int32_t bg_per_batch, int32_t batch_size, int32_t num_faces,
                            int32_t image_size, double near, double far, double eps, int32_t flags, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Scratch of nr_backward_uv_images: the double sums of the images and of the light colours (0 for sizes out of range). */
size_t nr_backward_uv_images_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t num_pixels, int32_t image_batch);

/*
 * grad_images [image_batch, P, 3] and lit->grad_light [B, F, 3] (either may be NULL, not both); face_index_map, weight_map and
 * depth_map are the forward's (weight_map is read at covered pixels only); eps the forward's.  lit->light is required,
 * lit->textures is not read.
 */
int nr_backward_uv_images(const nr_face_light *lit, const nr_uv_images *uv, const float *faces,
                          const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                          const float *grad_rgb_map, float *grad_images, int32_t batch_size, int32_t num_faces,
                          int32_t image_size, double eps, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Smooth light on per-pixel UV images (not in the reference; DESIGN K10 "Smooth light on UV images"): the calls above with
 * one light colour per CORNER of every face, lit->light [B, F, 3(corner), 3(rgb)], interpolated perspective-correctly at the
 * pixel -- the light nr_vertex_shade_forward(smooth = 1) gives a white mesh.  nr_uv_images, F == Nf or 2 Nf, the workspace
 * of the forward and every other argument are nr_forward_rasterize_uv's / nr_backward_uv_images'.
 *
 * Forward, at a pixel of batch element b covered by face f with weights w and depth zp (all float32, in this order, no
 * multiply-add contraction), z_k = faces[b, f, k, 2]:
 *   c     = exactly nr_forward_rasterize_uv's sample (for a reversed copy: f' = f - Nf, the weights reversed for the lookup,
 *           the transposed base cube);
 *   e_k   = fminf(fmaxf(w_k * (zp / z_k), 0), 1)    in the face's OWN corner order, also for a reversed copy (its light
 *           corners arrive flipped, as nr_vertex_shade_forward flips the corner colours of a reversed copy);
 *   L_c   = (light[b,f,0,c] * e_0 + light[b,f,1,c] * e_1) + light[b,f,2,c] * e_2
 *   rgb_c = (c_c * L_c) * 1 + 0 * background_c.
 * Uncovered pixels, alpha, depth, face_index_map, weight_map and visible_faces are bit for bit nr_forward_rasterize_uv's.
 *
 * Backward (nr_backward_uv_images_smooth), for the upstream g = grad_rgb_map, over the covered pixels:
 *   grad_images[b or 0, q_r, c] += g_c * L_c * omega_r    (faces with an image; L_c the forward's float32 value)
 *   grad_light[b, f, k, c]      += g_c * c_c * e_k         (every covered pixel)
 * Every element of grad_images [image_batch, P, 3] and lit->grad_light [B, F, 3, 3] is stored (0 where nothing reads; either
 * may be NULL, not both).  One pass over the pixels produces both.  The terms are formed and summed in double -- the nine
 * light sums of a face first over the runs of consecutive pixels of a wave that share the face, then with double atomics --
 * and rounded once to float: within 1e-6 of the sum of |terms| of the exact adjoint, also where thousands of pixels feed one
 * image pixel or one face.  The double additions arrive in no fixed order (see nr_backward_uv_images); rgb_map repeats bit
 * for bit.  No gradient to faces_uv or base.  grad_faces comes from nr_backward_rasterize_lit(NULL, ..., grad_textures =
 * NULL, ...) on the rgb_map of this forward.
 *
 * Argument errors (a NULL pointer, F not in {Nf, 2 Nf}, image_batch not in {1, B}, a workspace that is too small) return
 * NR_E_* before any launch.  Neither call synchronises the host or reads device values on the host: both can be captured
 * into a graph.
 */
typedef struct nr_corner_light {
    const float *light;     /* DEVICE [B, F, 3(corner), 3(rgb)] */
    int32_t texture_faces;  /* Nf; F == Nf or 2 Nf */
    float *grad_light;      /* backward: DEVICE [B, F, 3, 3] or NULL; every element stored */
} nr_corner_light;

int nr_forward_rasterize_uv_smooth(const nr_corner_light *lit, const nr_uv_images *uv, const float *faces,
                                   int32_t *face_index_map, float *weight_map, float *depth_map, float *rgb_map,
                                   float *alpha_map, uint8_t *visible_faces, const float *background, int32_t bg_per_batch,
                                   int32_t batch_size, int32_t num_faces, int32_t image_size, double near, double far,
                                   double eps, int32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* Scratch of nr_backward_uv_images_smooth: the double sums of the images and nine per face (0 for sizes out of range). */
size_t nr_backward_uv_images_smooth_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t num_pixels,
                                                    int32_t image_batch);

int nr_backward_uv_images_smooth(const nr_corner_light *lit, const nr_uv_images *uv, const float *faces,
                                 const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                 const float *grad_rgb_map, float *grad_images, int32_t batch_size, int32_t num_faces,
                                 int32_t image_size, double eps, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Corner colours (not in the reference; DESIGN K10 "Vertex colours"): corner_colors [B, F, 3, 3] float32, indexed (batch, face,
 * corner k, rgb), already lit.  F is the rasterizer's face count: with fill_back a reversed copy carries its own nine numbers in
 * its own corner order.  Forward, at a pixel of batch element b covered by face f with weights w and depth zp (float32, in
 * this order, no multiply-add contraction), z_k = faces[b, f, k, 2] (always the face's own batch element):
 *   d_k   = fminf(fmaxf(w_k * (zp / z_k), 0), 1)
 *   rgb_c = (C[b,f,0,c] * d_0 + C[b,f,1,c] * d_1) + C[b,f,2,c] * d_2
 *   rgb_c = rgb_c * 1 + 0 * background_c
 * Uncovered pixels, alpha, depth, face_index_map, weight_map and visible_faces are exactly nr_forward_rasterize's; the
 * workspace is nr_forward_workspace_bytes'.  rgb_map, background and corner_colors are required.
 *
 * Backward (nr_backward_corner_colors): grad_corner[b,f,k,c] = sum over the pixels owned by (b, f) of grad_rgb_map[pixel, c] *
 * d_k, every element stored (exact zeros for faces that own no pixel).  A face of up to 1024 candidate pixels (its box, as
 * the forward scans it) gathers its own pixels: double sums in a fixed order, no atomics, the same bits in every run.  A
 * larger face -- one may own the whole raster -- is summed per pixel: the lanes of a wave that share the face (runs of
 * consecutive pixels) add up first, in float in a tree of depth 6, the runs' sums are accumulated with double atomics and
 * rounded once to float: 8 float roundings at most, in no fixed order (see nr_backward_uv_images).  Either way the result is
 * within 1e-6 of the sum of |terms|.  visible_faces: the forward's flags [B, F] (faces without a pixel skip their scan), or
 * NULL.  grad_faces comes from
 * nr_backward_rasterize(textures = NULL, grad_textures = NULL) on the rgb_map of this forward.
 * Neither call synchronises the host: both can be captured into a graph.
 */
int nr_forward_rasterize_corner(const float *corner_colors, const float *faces, int32_t *face_index_map, float *weight_map,
                                float *depth_map, float *rgb_map, float *alpha_map, uint8_t *visible_faces,
                                const float *background, int32_t bg_per_batch, int32_t batch_size, int32_t num_faces,
                                int32_t image_size, double near, double far, int32_t flags, void *workspace,
                                size_t workspace_bytes, void *stream);

/* Scratch of nr_backward_corner_colors: nine double sums and a flag per face (0 for sizes out of range). */
size_t nr_backward_corner_colors_workspace_bytes(int32_t batch_size, int32_t num_faces);

int nr_backward_corner_colors(const float *faces, const int32_t *face_index_map, const float *weight_map,
                              const float *depth_map, const float *grad_rgb_map, const uint8_t *visible_faces,
                              float *grad_corner, int32_t batch_size, int32_t num_faces, int32_t image_size, void *workspace,
                              size_t workspace_bytes, void *stream);

/*
 * Vertex shading (not in the reference): corner_colors [B, F, 3, 3] (F = Nf * (fill_back ? 2 : 1)) from world-space vertices
 * [B, Nv, 3], faces_idx [Nf, 3] (or [B, Nf, 3] with idx_per_batch), per-vertex colors [color_batch, Nv, 3] (color_batch 1 or B)
 * and the light.  N_f = cross(v0 - v1, v2 - v1) is the unnormalised normal of face f (lighting.py:36-39).
 *   smooth = 0: light[b, f] and light[b, Nf + f] are exactly nr_frontend_forward_light's colours of the face and of its
 *     reversed copy; corner[b, f, k] = colors[v_k] * light[b, f], corner[b, Nf + f, k] = colors[v_(2-k)] * light[b, Nf + f].
 *   smooth = 1: m_v = the sum of N_f over the (face, corner) pairs of vertex v in ascending (f, k) order in float32
 *     (area-weighted), n_v = m_v / (|m_v| + 1e-5), light_front[v] = Ia Ca + Id (Cd max(n_v . dir, 0)), light_back[v] the same
 *     with max(-n_v . dir, 0); the corners of f take colors * light_front, those of Nf + f colors * light_back in reversed
 *     corner order.  A vertex without a face, or with a zero normal sum, gets the ambient light only.
 * adj_offsets [T, Nv + 1] and adj_entries [T, 3 Nf] (T = B with idx_per_batch, else 1) are the vertex -> (face, corner) table
 * of faces_idx: the entries adj_entries[adj_offsets[v] .. adj_offsets[v + 1]) of vertex v are its pairs 3 f + k in ascending
 * order.  The forward needs them with smooth = 1, the backward always; every sum around a vertex is a gather through them,
 * so there are no atomics and the results repeat bit for bit.  The workspace (nr_vertex_shade_workspace_bytes) is needed with
 * smooth = 1, by the forward and by a backward with grad_vertices.
 *
 * Backward, from grad_corner [B, F, 3, 3]: grad_colors [color_batch, Nv, 3] (shared colours: the sum over the batch, in double
 * in one fixed order) and grad_vertices [B, Nv, 3] through light -> normal -> normalize -> cross product (to be ADDED to the
 * geometry front-end's).  Either may be NULL, not both; every element is stored.  The light is a constant of the call.
 * nr_light lives in HOST memory; no call synchronises the host.
 */
size_t nr_vertex_shade_workspace_bytes(int32_t batch_size, int32_t num_vertices);

int nr_vertex_shade_forward(const float *vertices, const int32_t *faces_idx, const float *colors, const int32_t *adj_offsets,
                            const int32_t *adj_entries, float *corner_colors, int32_t batch_size, int32_t num_vertices,
                            int32_t num_faces, int32_t color_batch, int32_t idx_per_batch, int32_t fill_back, int32_t smooth,
                            const nr_light *light, void *workspace, size_t workspace_bytes, void *stream);

int nr_vertex_shade_backward(const float *vertices, const int32_t *faces_idx, const float *colors, const int32_t *adj_offsets,
                             const int32_t *adj_entries, const float *grad_corner, float *grad_colors, float *grad_vertices,
                             int32_t batch_size, int32_t num_vertices, int32_t num_faces, int32_t color_batch,
                             int32_t idx_per_batch, int32_t fill_back, int32_t smooth, const nr_light *light, void *workspace,
                             size_t workspace_bytes, void *stream);

/*
 * Normals (not in the reference): the normals that vertex shading forms and folds into a light colour, as outputs of their
 * own, from world-space vertices [B, Nv, 3] and faces_idx [Nf, 3] (or [B, Nf, 3] with idx_per_batch).  All float32, in the
 * operation order of nr_vertex_shade_forward, so that the two agree bit for bit:
 *   N_f = cross(v0 - v1, v2 - v1) (lighting.py:36-39), n_f = N_f / (|N_f| + 1e-5): face normals [B, Nf, 3];
 *   m_v = the sum of N_f over the (face, corner) pairs of vertex v in ascending (f, k) order (area-weighted),
 *     n_v = m_v / (|m_v| + 1e-5): vertex normals [B, Nv, 3].
 *   A vertex without a face, a zero normal sum and a zero-area face give exactly 0.
 * Corner normals [B, F, 3, 3] (F = Nf * (fill_back ? 2 : 1)), the rasterizer's corner colours (nr_forward_rasterize_corner):
 *   smooth = 0: corner[b, f, k] = n_f; smooth = 1: corner[b, f, k] = n_(v_k); the reversed copy of a face carries the negated
 *   normal in its own flipped corner order, corner[b, Nf + f, k] = -corner[b, f, 2 - k] (nr_vertex_shade_forward's layout).
 * adj_offsets / adj_entries: the vertex -> (face, corner) table of nr_vertex_shade_forward.  The vertex normals and the
 * smooth corner normals need it forward, every backward needs it; nr_face_normals_forward does not.
 *
 * Backward: grad_vertices [B, Nv, 3], the exact adjoint, through normalize's backward g / (r + eps) - v (g . v) / ((r + eps)^2 r)
 * (the second term 0 where r = 0) and the cross product.  Two launches: the first brings the upstream gradient (for corner
 * normals: front minus flipped back, summed over the corners of a face or around a vertex in table order) to a gradient of
 * N_f or m_v in the workspace, the second gathers it to the vertices; a smooth face takes (g_m(v0) + g_m(v1)) + g_m(v2).
 * Every sum is a gather through the table in ascending entry order: no atomics, every output element is stored, the same
 * bits in every run and for an image alone or inside a batch.  The workspace (nr_normals_workspace_bytes; 0 for sizes out of
 * range) is needed by every backward and by nr_corner_normals_forward with smooth = 1.  No call synchronises the host;
 * NR_E_* before any launch.
 */
size_t nr_normals_workspace_bytes(int32_t batch_size, int32_t num_vertices, int32_t num_faces);

int nr_vertex_normals_forward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                              const int32_t *adj_entries, float *normals, int32_t batch_size, int32_t num_vertices,
                              int32_t num_faces, int32_t idx_per_batch, void *stream);

int nr_vertex_normals_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                               const int32_t *adj_entries, const float *grad_normals, float *grad_vertices,
                               int32_t batch_size, int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch,
                               void *workspace, size_t workspace_bytes, void *stream);

int nr_face_normals_forward(const float *vertices, const int32_t *faces_idx, float *normals, int32_t batch_size,
                            int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch, void *stream);

int nr_face_normals_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                             const int32_t *adj_entries, const float *grad_normals, float *grad_vertices, int32_t batch_size,
                             int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch, void *workspace,
                             size_t workspace_bytes, void *stream);

int nr_corner_normals_forward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                              const int32_t *adj_entries, float *corner, int32_t batch_size, int32_t num_vertices,
                              int32_t num_faces, int32_t idx_per_batch, int32_t fill_back, int32_t smooth, void *workspace,
                              size_t workspace_bytes, void *stream);

int nr_corner_normals_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                               const int32_t *adj_entries, const float *grad_corner, float *grad_vertices, int32_t batch_size,
                               int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch, int32_t fill_back,
                               int32_t smooth, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Soft silhouettes (not in the reference): a probabilistic silhouette of the Soft Rasterizer family, with the exact
 * gradient of its definition.  faces [B, F, 3, 3] as for the rasterizer (x, y in NDC with y up, z the positive camera depth),
 * WITHOUT fill_back copies (a duplicated face would count twice); alpha, transmittance, grad_alpha [B, S, S] with row 0 the
 * BOTTOM row, pixel centres (2 i + 1 - S) / S; no anti-aliasing.  All float32.
 *   A face contributes iff its nine coordinates are finite and near <= z_k <= far at its three vertices; any other face is
 *   absent from every product and has a zero gradient.  Orientation plays no role.
 *   Per contributing face f and pixel p, with the segments 0, 1, 2 = v0v1, v1v2, v2v0: c_k the nearest point of segment k to
 *   p (parameter clamped to [0, 1]; a zero-length segment gives its endpoint), d2 = min_k |p - c_k|^2 (the lowest k on a tie);
 *   s = +1 if the three edge functions of p are all > 0 or all < 0, else -1 (a zero-area face has no inside);
 *   x = s d2 / sigma, D = 1 / (1 + e^-x).
 *   Q_p = the product over f, ascending, of 1 - D_pf evaluated as 1 / (1 + e^x); alpha_p = 1 - Q_p; transmittance = Q.
 *   Backward, with G_p = grad_alpha_p Q_p: dL/dx_pf = G_p D_pf (no division by 1 - D).  For the chosen segment a -> b with
 *   nearest point c = a + t (b - a) and r = p - c: d d2 / da = -2 (1 - t) r, d d2 / db = -2 t r (a clamped t hands the whole
 *   of -2 r to that endpoint), times s / sigma, summed over the pixels.  The third vertex and every z receive 0.
 *   A (pixel, face) pair is taken iff the pixel lies in the face's box: the pixel range of the triangle's bounding box grown
 *   by sqrt(17 sigma).  A pair outside it is outside the triangle with d2 > 17 sigma, D < 2^-24, and is left out of the
 *   product and of the gradient.
 * Coordinates: results are finite for |x|, |y| up to about 1e18; beyond that the squares of the edge lengths overflow in
 * float32 and alpha, transmittance and grad_faces of the pixels and faces concerned may be NaN (no index depends on them:
 * the boxes are clamped before the conversion to int).
 * sigma: 1e-30 <= sigma <= 1e30 (NR_E_MODE otherwise, as for a NaN near or far), no gradient.  Sizes: 1 <= batch_size <= 65535,
 * 1 <= image_size <= 16384, 1 <= num_faces <= 2^24 and batch_size * num_faces * 9 < 2^31 (NR_E_SIZE otherwise).
 * The forward stores alpha and transmittance; the backward takes the forward's transmittance (not 1 - alpha) and stores
 * every entry of grad_faces [B, F, 3, 3].  Both need a workspace of nr_soft_silhouette_workspace_bytes (0 for sizes out of
 * range), in which each writes a record per face first; nothing is kept in it between calls.  No atomics: the same bits in
 * every run and for an image alone or inside a batch.  No call synchronises the host; NR_E_* before any launch.
 */
size_t nr_soft_silhouette_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t image_size);

int nr_soft_silhouette_forward(const float *faces, float *alpha, float *transmittance, int32_t batch_size, int32_t num_faces,
                               int32_t image_size, double sigma, double near, double far, void *workspace,
                               size_t workspace_bytes, void *stream);

int nr_soft_silhouette_backward(const float *faces, const float *transmittance, const float *grad_alpha, float *grad_faces,
                                int32_t batch_size, int32_t num_faces, int32_t image_size, double sigma, double near, double far,
                                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Soft colour rendering (not in the reference): the soft silhouette's coverage aggregated over the faces by Soft Rasterizer's
 * depth-weighted softmax, with the exact gradient of its definition to x, y, z and the face colours.  faces [B, F, 3, 3] as
 * for nr_soft_silhouette_forward; colors [B, F, 3] (colors_per_batch = 1) or [F, 3] shared by the batch and read in place
 * (colors_per_batch = 0), one RGB colour per face; rgba, grad_rgba [B, 4, S, S], transmittance [B, S, S] and normaliser
 * [B, 2, S, S] (m, then Z) with row 0 the BOTTOM row, pixel centres (2 i + 1 - S) / S; no anti-aliasing.  All float32.
 *   A face contributes iff its nine coordinates are finite, near <= z_k <= far at its three vertices and its doubled area
 *   (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0), evaluated in double, is not 0 (a zero-area face has no plane to take a depth from).
 *   Per contributing face f and pixel p: d2, the chosen segment k (the lowest on a tie), its clamped t, r = p - c, the side s,
 *   x = s d2 / sigma and D = 1 / (1 + e^-x), 1 - D = 1 / (1 + e^x) as for the soft silhouette; c_0, c_1, c_2 the edge
 *   functions of the segments v0v1, v1v2, v2v0 at p.  The pair is TAKEN iff s = +1 or d2 <= 17 sigma: part of the definition.
 *   Inverse depth: inside, A = c_0 + c_1 + c_2, lambda_0 = c_1 / A, lambda_1 = c_2 / A, lambda_2 = c_0 / A; outside, at the
 *   nearest point of the chosen segment a -> b, lambda_a = 1 - t, lambda_b = t, the third 0;
 *   iz = lambda_0 / z0 + lambda_1 / z1 + lambda_2 / z2 (continuous across every edge), zp = 1 / iz,
 *   zn = (far - zp) / (far - near).
 *   Over the taken pairs of p in ascending f, with m = max(eps, max_f zn_f): w_f = D_f exp((zn_f - m) / gamma),
 *   w_b = exp((eps - m) / gamma), Z = w_b + sum w_f, rgb = (w_b background + sum w_f C_f) / Z, Q = prod 1 / (1 + e^x_f),
 *   alpha = 1 - Q; transmittance = Q, normaliser = (m, Z).
 *   Backward, per taken pair, from the stored rgb, Q, m and Z: W = D exp((zn - m) / gamma) / Z, h = g_rgb . (C_f - rgb);
 *   dL/dC_f += W g_rgb; dL/dx = h W (1 - D) + g_alpha Q D; dL/dzn = h W / gamma.  dx goes to the two ends of the chosen
 *   segment as in nr_soft_silhouette_backward; dzn/dzp = -1 / (far - near), dzp/diz = -zp^2, diz/dz_k = -lambda_k / z_k^2;
 *   diz reaches x and y through lambda (inside) or through t where 0 < t < 1 (outside; a clamped t has derivative 0).
 * colors shared by the batch get their gradient [F, 3] as the sum over the images in ascending b, in double, rounded once.
 * sigma and gamma in [1e-30, 1e30], far > near, near, far, eps and the background finite, colors_per_batch 0 or 1 (NR_E_MODE
 * otherwise); no gradients for them.  Sizes as for nr_soft_silhouette_forward (NR_E_SIZE).  The forward stores every element of
 * rgba, transmittance and normaliser; the backward takes them back and stores every entry of grad_faces [B, F, 3, 3] and of
 * grad_colors ([B, F, 3] or [F, 3]).  Both need a workspace of nr_soft_render_workspace_bytes (0 for sizes out of range), in
 * which each writes a record per face first; nothing is kept in it between calls.  No atomics: the same bits in every run
 * and for an image alone or inside a batch.  No call synchronises the host; NR_E_* before any launch.
 */
size_t nr_soft_render_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t image_size);

int nr_soft_render_forward(const float *faces, const float *colors, float *rgba, float *transmittance, float *normaliser,
                           int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t colors_per_batch, double sigma,
                           double gamma, double near, double far, double eps, double background_r, double background_g,
                           double background_b, void *workspace, size_t workspace_bytes, void *stream);

int nr_soft_render_backward(const float *faces, const float *colors, const float *rgba, const float *transmittance,
                            const float *normaliser, const float *grad_rgba, float *grad_faces, float *grad_colors,
                            int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t colors_per_batch, double sigma,
                            double gamma, double near, double far, double eps, double background_r, double background_g,
                            double background_b, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Soft colour rendering with corner colours: nr_soft_render_* with three colours per face, interpolated at the pixel.
 * colors [B, F, 3, 3] (colors_per_batch = 1) or [F, 3, 3] shared by the batch and read in place (colors_per_batch = 0),
 * indexed (face, corner, rgb); grad_colors has the shape of colors.  Everything else -- the contribution rule, the taken
 * rule, lambda_k, iz, zp, zn, m, w_f, w_b, Z, Q, alpha, the layouts, the ranges, the NR_E_* codes before any launch and the
 * workspace rule (nr_soft_corners_workspace_bytes) -- is nr_soft_render_*'s, except the colour of a taken pair:
 *   u_k = lambda_k / z_k,  mu_k = u_k zp  (the perspective-correct weights; they add up to 1 in exact arithmetic),
 *   C_f(p) = (mu_0 C_f0 + mu_1 C_f1) + mu_2 C_f2 per channel,  rgb = (w_b background + sum w_f C_f(p)) / Z.
 *   Inside lambda is the rasterizer's barycentric form; outside lambda = (1 - t, t, 0) on the chosen segment: the colour at
 *   the nearest boundary point, continuous across every edge and single-valued (the nearest point of a triangle is unique).
 *   Backward, per taken pair: h = g_rgb . (C_f(p) - rgb); dL/dC_fk += W mu_k g_rgb; with E_k = W zp (g_rgb . (C_fk - C_f(p)))
 *   and d_k = diz + E_k (diz: nr_soft_render_backward's dL/diz): dL/dlambda_k = d_k / z_k, dL/dz_k = -d_k lambda_k / z_k^2;
 *   inside dL/dc_i = (dL/dlambda_v(i) - diz iz) / A with v(0) = 2, v(1) = 0, v(2) = 1 (sum_k lambda_k dL/dlambda_k = diz iz
 *   in exact arithmetic); outside with a free t on a -> b: dL/dt = d_b / z_b - d_a / z_a; a clamped t has derivative 0;
 *   dL/dx is nr_soft_render_backward's.  Three equal corner colours: every E_k = 0 and the gradient is the flat one.
 */
size_t nr_soft_corners_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t image_size);

int nr_soft_corners_forward(const float *faces, const float *colors, float *rgba, float *transmittance, float *normaliser,
                            int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t colors_per_batch, double sigma,
                            double gamma, double near, double far, double eps, double background_r, double background_g,
                            double background_b, void *workspace, size_t workspace_bytes, void *stream);

int nr_soft_corners_backward(const float *faces, const float *colors, const float *rgba, const float *transmittance,
                             const float *normaliser, const float *grad_rgba, float *grad_faces, float *grad_colors,
                             int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t colors_per_batch, double sigma,
                             double gamma, double near, double far, double eps, double background_r, double background_g,
                             double background_b, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Soft colour rendering with UV texture images: nr_soft_render_* with the images of a UV layout (nr_uv_images above) sampled
 * at every taken pair.  light [B, F, 3] (light_per_batch = 1) or [F, 3] shared by the batch and read in place
 * (light_per_batch = 0): one light colour per face; grad_light has its shape.  F is the layout's face count -- uv->faces_uv
 * [F, 3, 2], uv->face_image [F], uv->base [F, ts, ts, ts, 3]; the struct carries no count, and the soft path has no fill_back
 * copies -- and uv->image_batch is 1 (images shared by the batch, image batch stride 0) or B.  Everything else -- the
 * contribution rule, the taken rule, lambda_k, iz, zp, zn, m, w_f, w_b, Z, Q, alpha, the layouts, the ranges -- is
 * nr_soft_render_*'s, and u_k = lambda_k / z_k, mu_k = u_k zp are nr_soft_corners_*'s, except the colour of a taken pair:
 *   C_f(p)_c = L_fc T_f(p)_c,  rgb = (w_b background + sum w_f C_f(p)) / Z.
 *   Face f with an image m = face_image[f] in [0, num_images) whose table row lies inside the num_pixels packed pixels:
 *     d_k = fminf(fmaxf(mu_k, 0), 1) (the clamp removes rounding excess only; its derivative is taken as 1), and T_f(p) is
 *     the bilinear lookup nr_bake_uv_textures takes at a texel, at the barycentric point d of faces_uv[f] in image m [H, W]:
 *     pos_x = (sum_k uvx_fk d_k) (W - 1), pos_y = (sum_k uvy_fk d_k) (H - 1); xi = (int)pos_x, yi = (int)pos_y,
 *     yi1 = (int)(pos_y + 1); wx1 = pos_x - xi, wx0 = 1 - wx1, wy1 = pos_y - yi, wy0 = 1 - wy1; the four reads (yi, xi),
 *     (yi1, xi), (yi, xi + 1), (yi1, xi + 1) with the weights wx0 wy0, wx0 wy1, wx1 wy0, wx1 wy1, rows counted from the
 *     bottom of an image stored top row first, each flat index row * W + col clamped to [0, H W - 1] -- NO READ LEAVES THE
 *     IMAGE, whatever uv holds (outside [0, 1], infinite, NaN) --, T = ((0 + I[q_0] w_0) + I[q_1] w_1) + ... in read order.
 *   Any other face: T_f = the mean of its base cube (summed in double, rounded once), a constant without a gradient.
 *   Inside a face this is the texture nr_forward_rasterize_uv shows, outside the texture at the nearest boundary point:
 *   continuous across every edge, as the corner colours are.
 * Backward, per taken pair, with W = w_f / Z and h = g_rgb . (C_f(p) - rgb) as in nr_soft_render_backward.  The read indices
 * carry no gradient; wx1 and wy1 move with pos_x and pos_y:
 *   Tx_c = sum_r (dw_r / dwx1) I[q_r]_c = wy0 (I[q_2] - I[q_0])_c + wy1 (I[q_3] - I[q_1])_c,
 *   Ty_c = sum_r (dw_r / dwy1) I[q_r]_c = wx0 (I[q_1] - I[q_0])_c + wx1 (I[q_3] - I[q_2])_c,
 *   G_k  = sum_c g_c L_fc (Tx_c uvx_fk (W - 1) + Ty_c uvy_fk (H - 1))     (0 for a face without an image)
 *   grad_images[b or 0, q_r, c] += W g_c L_fc w_r     (faces with an image; shared images: one sum over the batch)
 *   grad_light[b or 0, f, c]    += W g_c T_f(p)_c
 *   E_k = W zp (G_k - sum_j mu_j G_j)
 * and everything after E_k is nr_soft_corners_backward's: d_k = diz + E_k, the z terms, the free-t term and the inside terms.
 * faces_uv, face_image and base receive no gradient.
 * grad_faces and grad_light: fixed order, no atomics, the same bits in every run and for an image alone or inside a batch;
 * shared light is added over the batch in ascending b in double and rounded once.  grad_images [image_batch, num_pixels, 3]
 * (every element stored; NULL: not computed): each entry is ROUNDED ONCE FROM A DOUBLE SUM WHOSE ADDITIONS ARRIVE IN NO FIXED
 * ORDER (double atomics into a zero-filled scratch in the workspace; terms that are 0 are skipped): its bits are not
 * promised.
 * NR_E_* before any launch, nr_soft_render_*'s codes in their order with nr_forward_rasterize_uv's checks of *uv added: a
 * NULL pointer (uv and its five tables included) NR_E_NULL; sizes out of range, texture_size outside [2, 1024], num_images
 * or num_pixels < 1, image_batch not in {1, B} NR_E_SIZE; the numbers and light_per_batch NR_E_MODE; a NULL or short
 * workspace NR_E_WORKSPACE.  nr_soft_uv_workspace_bytes reads uv->num_pixels and uv->image_batch only (0 for NULL or sizes out
 * of range).  No host synchronisation; capturable.
 */
size_t nr_soft_uv_workspace_bytes(const nr_uv_images *uv, int32_t batch_size, int32_t num_faces, int32_t image_size);

int nr_soft_uv_forward(const nr_uv_images *uv, const float *faces, const float *light, float *rgba, float *transmittance,
                       float *normaliser, int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t light_per_batch,
                       double sigma, double gamma, double near, double far, double eps, double background_r,
                       double background_g, double background_b, void *workspace, size_t workspace_bytes, void *stream);

int nr_soft_uv_backward(const nr_uv_images *uv, const float *faces, const float *light, const float *rgba,
                        const float *transmittance, const float *normaliser, const float *grad_rgba, float *grad_faces,
                        float *grad_light, float *grad_images, int32_t batch_size, int32_t num_faces, int32_t image_size,
                        int32_t light_per_batch, double sigma, double gamma, double near, double far, double eps,
                        double background_r, double background_g, double background_b, void *workspace, size_t workspace_bytes,
                        void *stream);

/*
 * Soft colour rendering with texture cubes sampled at the pixel (not in the reference): textures [B, F, ts, ts, ts, 3]
 * (textures_per_batch = 1) or [1, F, ts, ts, ts, 3] shared by the batch (textures_per_batch = 0, read in place), the
 * rasterizer's cubes WITHOUT fill_back copies, 2 <= ts <= 8; light [B, F, 3] (light_per_batch = 1) or [1, F, 3]
 * (light_per_batch = 0): one light colour per face; grad_textures and grad_light have their shapes.  Everything else -- the
 * contribution rule, the taken rule, lambda_k, iz, zp, zn, m, w_f, w_b, Z, Q, alpha, the layouts, the ranges -- is
 * nr_soft_render_*'s, and u_k = lambda_k / z_k, mu_k = u_k zp are nr_soft_corners_*'s, except the colour of a taken pair:
 *   C_f(p)_c = L_fc T_f(p)_c,  rgb = (w_b background + sum w_f C_f(p)) / Z.
 *   v_k = mu_k (ts - 1); v_k = fmaxf(v_k, 0) (a NaN becomes 0); v_k = (float)fmin((double)v_k, (double)(ts - 1) - texture_eps):
 *   the rasterizer's sequence with mu_k where it has w_k (zp / z_k).  i_k = (int)v_k, fr_k = v_k - i_k; eight taps pn = 0..7,
 *   bit k of pn picks (i_k + 1, fr_k), else (i_k, 1 - fr_k); the weight w_pn = ((1 . f_0) f_1) f_2, the flat index (i_0 ts +
 *   i_1) ts + i_2 of the picked indices.  A tap whose flat index is >= ts^3 is skipped, never read (its weight is an exact 0):
 *   NO READ LEAVES THE FACE'S CUBE, whatever mu holds.  T = ((0 + w_0 tex_0) + w_1 tex_1) + ... in tap order.
 *   Inside a face this is the texture nr_forward_rasterize shows, outside the texture at the nearest boundary point:
 *   continuous across every edge.  texture_eps, 0 <= texture_eps < 1, is the rasterizer's eps; it is not `eps`, which places
 *   the background in the depth order.
 * Backward, per taken pair, with W = w_f / Z and h = g_rgb . (C_f(p) - rgb) as in nr_soft_render_backward.  The tap indices
 * carry no gradient and both clamps are taken with derivative 1 (the lower one removes rounding excess only; the upper one
 * acts on a sliver of relative width texture_eps / (ts - 1) at a vertex, where the gradient is the unclamped derivative):
 *   D_kc = sum_pn (dw_pn / dfr_k) tex[tap_pn]_c   (four differences of the taps with and without bit k, each times the other
 *          two dimensions' factors; a skipped tap counts as 0)
 *   G_k  = (ts - 1) sum_c g_c L_fc D_kc
 *   grad_textures[b or 0, f, tap_pn, c] += W g_c L_fc w_pn   (shared cubes: one sum over the batch)
 *   grad_light[b or 0, f, c]            += W g_c T_f(p)_c
 *   E_k = W zp (G_k - sum_j mu_j G_j)
 * and everything after E_k is nr_soft_corners_backward's.  Every output: fixed order, no atomics, every element stored, the
 * same bits in every run and for an image alone or inside a batch.  grad_textures (NULL: not computed): the wave that owns
 * (image, face) adds the terms of its taken pairs in double in the order of its walk and rounds each entry once; the entries
 * of a dropped face or an untouched texel are exact zeros; no zero fill is expected from the caller.  Shared cubes and shared
 * light: the per-image results are added over the batch in ascending b in double and rounded once.
 * NR_E_* before any launch, nr_soft_render_*'s codes in their order: a NULL pointer NR_E_NULL; sizes out of range, ts
 * outside [2, 8] or F ts^3 3 above 2^31 - 257 NR_E_SIZE; the numbers, texture_eps outside [0, 1), textures_per_batch or
 * light_per_batch NR_E_MODE; a NULL or short workspace NR_E_WORKSPACE.  nr_soft_cubes_workspace_bytes: 0 for sizes out of
 * range.  No host synchronisation; capturable.
 */
size_t nr_soft_cubes_workspace_bytes(int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t texture_size,
                                     int32_t textures_per_batch);

int nr_soft_cubes_forward(const float *faces, const float *textures, const float *light, float *rgba, float *transmittance,
                          float *normaliser, int32_t batch_size, int32_t num_faces, int32_t image_size, int32_t texture_size,
                          int32_t textures_per_batch, int32_t light_per_batch, double sigma, double gamma, double near,
                          double far, double eps, double background_r, double background_g, double background_b,
                          double texture_eps, void *workspace, size_t workspace_bytes, void *stream);

int nr_soft_cubes_backward(const float *faces, const float *textures, const float *light, const float *rgba,
                           const float *transmittance, const float *normaliser, const float *grad_rgba, float *grad_faces,
                           float *grad_light, float *grad_textures, int32_t batch_size, int32_t num_faces, int32_t image_size,
                           int32_t texture_size, int32_t textures_per_batch, int32_t light_per_batch, double sigma,
                           double gamma, double near, double far, double eps, double background_r, double background_g,
                           double background_b, double texture_eps, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Mesh losses (not in the reference's library; the two shape priors of its paper, section 5): on world-space vertices
 * [B, Nv, 3] with ONE topology for the call, described by host-built int32 tables (neural_renderer_amd/mesh_losses.py).
 *   N(v): the distinct u != v that share a face with v; nbr_offsets [Nv + 1], nbr [num_nbr]: N(v) = nbr[nbr_offsets[v] ..
 *     nbr_offsets[v + 1]) ascending, deg v its length.
 *   quads [E2, 4]: (v0 < v1, v2, v3) for every edge {v0, v1} that lies in exactly two faces (faces with a repeated index
 *     not counted), v2 / v3 the opposite vertices, v2 from the lower-numbered face; ordered by (v0, v1).
 *   inc_offsets [Nv + 1], inc [4 E2]: the (quad, slot) pairs 4 q + slot in which vertex v occurs, ascending.
 * Laplacian: delta_v = x_v - (sum of x_u over N(v), table order) / deg v (0 with deg v = 0), loss[b] = sum_v |delta_v|^2;
 *   delta [B, Nv, 3] is stored for the backward (NULL: not stored).  Backward from grad_loss [B]:
 *   grad_vertices[b, v] = 2 g_b (delta_v - sum over N(v) of delta_u / deg u), a gather, N being symmetric.
 * Flatness, per quad: a = x1 - x0, b_i = x_(i+1) - x0, c_i = b_i - ((a . b_i) / (a . a + eps)) a, l_i = sqrt(c_i . c_i + eps),
 *   cos = (c1 . c2) / (l1 l2 + eps), loss[b] = sum over the quads of (cos + 1)^2: 0 (up to eps) on a flat mesh, finite for
 *   every finite input with eps > 0.  eps is rounded to float.  E2 = 0: loss = 0 and zero gradients (quads, inc_offsets,
 *   inc may be NULL).  Backward: every vertex adds, for each of its (quad, slot) pairs in table order, that slot's
 *   derivative recomputed from the quad's four vertices.
 * The float operation order of every formula: the header comment of csrc/nr_mesh_losses.hip.  The losses: per block of
 * 256 vertices / quads a double sum in a fixed order into the workspace (nr_mesh_loss_workspace_bytes(B, Nv) resp. (B, E2)),
 * the blocks added in block order in double by a second kernel, rounded once.  No atomics in any kernel: the same bits in
 * every run.  Every output element is stored; no call synchronises the host; NR_E_* before any launch.
 */
size_t nr_mesh_loss_workspace_bytes(int32_t batch_size, int32_t num_items);

int nr_laplacian_forward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr, float *delta, float *loss,
                         int32_t batch_size, int32_t num_vertices, int32_t num_nbr, void *workspace, size_t workspace_bytes,
                         void *stream);

int nr_laplacian_backward(const float *delta, const int32_t *nbr_offsets, const int32_t *nbr, const float *grad_loss,
                          float *grad_vertices, int32_t batch_size, int32_t num_vertices, int32_t num_nbr, void *stream);

int nr_flatness_forward(const float *vertices, const int32_t *quads, float *loss, int32_t batch_size, int32_t num_vertices,
                        int32_t num_quads, double eps, void *workspace, size_t workspace_bytes, void *stream);

int nr_flatness_backward(const float *vertices, const int32_t *quads, const int32_t *inc_offsets, const int32_t *inc,
                         const float *grad_loss, float *grad_vertices, int32_t batch_size, int32_t num_vertices,
                         int32_t num_quads, double eps, void *stream);

/*
 * Edge-length and cotangent Laplacian losses (DESIGN "Mesh losses: edge length and cotangent Laplacian"), on the same vertices,
 * tables, block sums and workspace query as the two above.
 *   edges [E, 2]: the distinct undirected pairs (v0 < v1) that share a face -- the pairs of nbr --, ordered by (v0, v1);
 *   nbr_edge [num_nbr]: the edge number of every entry of nbr.
 * Edge length: l_e = |x_v1 - x_v0|, loss[b] = sum_e (l_e - t_e)^2.  The target t: `target` [E] (target_per_batch = 0) or [B, E]
 *   (1), read in place; or, with target NULL, the number target_value >= 0 for every edge, and then target_value = 0 skips the
 *   square root: loss[b] = sum_e |e|^2.  Workspace: nr_mesh_loss_workspace_bytes(B, E).  E = 0: loss = 0 (edges may be NULL).
 *   Backward: grad_vertices[b, v] = 2 g_b sum over u in N(v), table order, of ((l - t) / l) (x_v - x_u), every edge recomputed
 *   from its two vertices and its target read through nbr_edge (which may be NULL with target NULL); a term with l = 0 is
 *   exactly 0.
 * Cotangent Laplacian: nr_cot_weights writes cot [B, F, 3] for faces [F, 3]: cot_c = (a . b) / sqrt(|a x b|^2 + eps) with
 *   a = x_(c+1) - x_c, b = x_(c+2) - x_c (corners mod 3; eps rounded to float); a face with a repeated index stores three zeros.
 *   nr_cot_apply applies L to field [B, Nv, 3] through the vertex -> (face, corner) table adj_offsets [Nv + 1], adj_entries
 *   [3 F] (ascending 3 f + c within a vertex; ONE topology):
 *     L(phi)_v = 1/2 sum over the entries (f, c) of v of cot[f, c+2] (phi_(c+1) - phi_v) + cot[f, c+1] (phi_(c+2) - phi_v),
 *   out[b, v] = L(field)_v, times 2 scale[b] with scale [B] not NULL; with loss not NULL loss[b] = sum_v |out[b, v]|^2
 *   (workspace nr_mesh_loss_workspace_bytes(B, Nv); otherwise the workspace is not read) and out may be NULL.
 *   The loss's forward is L applied to the vertices; its backward, the weights being constants of the step and L symmetric,
 *   is L applied to the stored H with scale = grad_loss.
 * No atomics, every output element stored, no host synchronisation, NR_E_* before any launch, as above.
 */
int nr_edge_length_forward(const float *vertices, const int32_t *edges, const float *target, float *loss, int32_t batch_size,
                           int32_t num_vertices, int32_t num_edges, int32_t target_per_batch, double target_value,
                           void *workspace, size_t workspace_bytes, void *stream);

int nr_edge_length_backward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr, const int32_t *nbr_edge,
                            const float *target, const float *grad_loss, float *grad_vertices, int32_t batch_size,
                            int32_t num_vertices, int32_t num_nbr, int32_t num_edges, int32_t target_per_batch,
                            double target_value, void *stream);

int nr_cot_weights(const float *vertices, const int32_t *faces, float *cot, int32_t batch_size, int32_t num_vertices,
                   int32_t num_faces, double eps, void *stream);

int nr_cot_apply(const float *field, const float *cot, const int32_t *faces, const int32_t *adj_offsets,
                 const int32_t *adj_entries, const float *scale, float *out, float *loss, int32_t batch_size,
                 int32_t num_vertices, int32_t num_faces, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Point-to-mesh distance (not in the reference's library; DESIGN "Point-to-mesh distance"): points [B, N, 3] -- or ONE cloud
 * [N, 3] for the batch with points_per_batch = 0 --, world-space vertices [B, Nv, 3] and ONE topology faces [F, 3] int32.
 *   nr_point_mesh_points_to_faces: per point the nearest face by a brute-force sweep: dist2 [B, N], face_ids [B, N] int32 (the
 *     lowest face number among the minimal computed distances), barycentric [B, N, 3] (w0, w1, w2 of the closest point).
 *   nr_point_mesh_faces_to_points: per face the nearest point: dist2 [B, F], point_ids [B, F] int32 (the lowest point number
 *     on a tie), barycentric [B, F, 3] of the point of the face nearest to that cloud point.
 *   The closest point of a triangle: csrc/nr_point_triangle.h, one definition for both (the same bits for the same pair),
 *   exact on faces without area.  A NaN distance never wins; ids are always in range; a row of NaN pairs reports id 0 and a
 *   non-finite dist2.  split: 0 lets the call decide whether to cut the streamed side (faces resp. points) over several
 *   workgroups, n >= 1 asks for n parts (1: none); the result does not depend on it.  The workspace holds the parts' minima:
 *   nr_point_mesh_workspace_bytes(B, N, F, faces_to_points, split), 0 when the call is not split (workspace may then be NULL).
 *   nr_point_mesh_loss: loss[b] = weight_points * sum_i dist2_points[b, i] + weight_faces * sum_f dist2_faces[b, f], either
 *     array may be NULL (its term is left out; both: NR_E_MODE); the sums in double in a fixed order, rounded once.
 *   Backward, from per-pair upstream gradients grad_dist2_points [B, N] and grad_dist2_faces [B, F]; the pairs of one
 *   direction are left out by passing its ids as NULL (both: NR_E_MODE).  r = ((p - v0) - w1 (v1 - v0)) - w2 (v2 - v0).
 *   nr_point_mesh_backward_points (points [B, N, 3]): grad_points[b, i] = 2 g r of its own pair, then 2 g r of the faces that
 *     chose point i, in the order of order_faces [B, F] (face numbers sorted by point id, stable) between
 *     offsets_points[b, i] and offsets_points[b, i + 1] ([B, N + 1]).
 *   nr_point_mesh_backward_vertices: grad_vertices[b, v] = 0, then for each entry (f, k) of v in the vertex -> (face, corner)
 *     table (adj_offsets [Nv + 1], adj_entries [3 F]: 3 f + k ascending) minus (2 g w_k) r of face f's own pair, then of the
 *     points that chose f, in the order of order_points [B, N] (point numbers sorted by face id, stable) between
 *     offsets_faces[b, f] and offsets_faces[b, f + 1] ([B, F + 1]).
 * Sizes: 1 <= B <= 65535, B N <= (2^31 - 1) / 3, B F <= (2^31 - 1) / 18, B Nv <= (2^31 - 1) / 6 (NR_E_SIZE; also a forced
 * split that asks for more than 2^31 - 1 workgroups; nr_point_mesh_workspace_bytes returns 0 for either).  No atomics: the
 * same bits in every run and for an image alone or inside a batch.  Every output element is stored exactly once; no call
 * synchronises the host; NR_E_* before any launch (NULL before sizes).
 */
size_t nr_point_mesh_workspace_bytes(int32_t batch_size, int32_t num_points, int32_t num_faces, int32_t faces_to_points,
                                     int32_t split);

int nr_point_mesh_points_to_faces(const float *points, const float *vertices, const int32_t *faces, float *dist2,
                                  int32_t *face_ids, float *barycentric, int32_t batch_size, int32_t num_points,
                                  int32_t num_vertices, int32_t num_faces, int32_t points_per_batch, int32_t split,
                                  void *workspace, size_t workspace_bytes, void *stream);

int nr_point_mesh_faces_to_points(const float *points, const float *vertices, const int32_t *faces, float *dist2,
                                  int32_t *point_ids, float *barycentric, int32_t batch_size, int32_t num_points,
                                  int32_t num_vertices, int32_t num_faces, int32_t points_per_batch, int32_t split,
                                  void *workspace, size_t workspace_bytes, void *stream);

int nr_point_mesh_loss(const float *dist2_points, const float *dist2_faces, float *loss, int32_t batch_size, int32_t num_points,
                       int32_t num_faces, double weight_points, double weight_faces, void *stream);

int nr_point_mesh_backward_points(const float *points, const float *vertices, const int32_t *faces, const int32_t *face_ids,
                                  const float *barycentric_points, const float *grad_dist2_points, const int32_t *point_ids,
                                  const float *barycentric_faces, const float *grad_dist2_faces, const int32_t *order_faces,
                                  const int32_t *offsets_points, float *grad_points, int32_t batch_size, int32_t num_points,
                                  int32_t num_vertices, int32_t num_faces, void *stream);

int nr_point_mesh_backward_vertices(const float *points, const float *vertices, const int32_t *faces, const int32_t *adj_offsets,
                                    const int32_t *adj_entries, const int32_t *face_ids, const float *barycentric_points,
                                    const float *grad_dist2_points, const int32_t *order_points, const int32_t *offsets_faces,
                                    const int32_t *point_ids, const float *barycentric_faces, const float *grad_dist2_faces,
                                    float *grad_vertices, int32_t batch_size, int32_t num_points, int32_t num_vertices,
                                    int32_t num_faces, int32_t points_per_batch, void *stream);

/*
 * Winding numbers (not in the reference's library; DESIGN "Winding numbers"): points [B, N, 3] -- or ONE cloud [N, 3] for the
 * batch with points_per_batch = 0 (any value but 0 and 1: NR_E_MODE) --, world-space vertices [B, Nv, 3] and ONE topology
 * faces [F, 3] int32.  w[b, i] = (1 / 4 pi) sum_f Omega_f(p_bi), Omega = 2 atan2(num, den) the signed solid angle of face f seen
 * from the point (csrc/nr_solid_angle.h: one definition for the three calls, the same bits for the same pair).  A face with
 * two corners equal as positions contributes exactly 0 to every output; num = den = 0 gives Omega = 0 and a zero gradient; a
 * non-finite coordinate gives NaN.  The sums are a two-level definition: the streamed side (faces; for the gradient to the
 * vertices, points) in fixed tiles of 256; a tile's terms added in double, ascending, from 0; the tile sums added in double,
 * ascending; the total scaled in double and rounded once.
 *   nr_winding_forward: winding [B, N].
 *   nr_winding_backward_points (points [B, N, 3]): grad_points[b, i] = (g_bi / 4 pi) sum_f dOmega_f/dp, g = grad_winding [B, N].
 *   nr_winding_backward_vertices: per face corner (1 / 4 pi) sum_i g_bi dOmega_f(p_bi)/dv_k into the workspace, then
 *     grad_vertices[b, v] = the sum of the corners (f, k) of v in the vertex -> (face, corner) table (adj_offsets [Nv + 1],
 *     adj_entries [3 F]: 3 f + k ascending), in table order, in float32.
 *   split: 0 lets the call decide whether to cut the streamed side at tile boundaries over several workgroups, n >= 1 asks for
 *   n parts (1: none); a split call stores its tile sums in the workspace and merges them in the same ascending order, so the
 *   result does not depend on it, to the bit (tile sums above 256 MiB: the call is not split).
 *   nr_winding_workspace_bytes(B, N, F, which, split), which = 0 forward, 1 backward_points, 2 backward_vertices (else 0): the
 *   tile sums of a split call, plus for 2 the corner gradients; 0: workspace may be NULL.
 * Sizes: 1 <= B <= 65535, B N <= (2^31 - 1) / 3, B F <= (2^31 - 1) / 18, B Nv <= (2^31 - 1) / 6 (NR_E_SIZE; also a forced
 * split that asks for more than 2^31 - 1 workgroups, for which nr_winding_workspace_bytes returns 0).  No atomics: the
 * same bits in every run, for an image alone or inside a batch, split or not.  Every output element is stored exactly once; no
 * call synchronises the host; NR_E_* before any launch (NULL before sizes).
 */
size_t nr_winding_workspace_bytes(int32_t batch_size, int32_t num_points, int32_t num_faces, int32_t which, int32_t split);

int nr_winding_forward(const float *points, const float *vertices, const int32_t *faces, float *winding, int32_t batch_size,
                       int32_t num_points, int32_t num_vertices, int32_t num_faces, int32_t points_per_batch, int32_t split,
                       void *workspace, size_t workspace_bytes, void *stream);

int nr_winding_backward_points(const float *points, const float *vertices, const int32_t *faces, const float *grad_winding,
                               float *grad_points, int32_t batch_size, int32_t num_points, int32_t num_vertices,
                               int32_t num_faces, int32_t split, void *workspace, size_t workspace_bytes, void *stream);

int nr_winding_backward_vertices(const float *points, const float *vertices, const int32_t *faces, const int32_t *adj_offsets,
                                 const int32_t *adj_entries, const float *grad_winding, float *grad_vertices, int32_t batch_size,
                                 int32_t num_points, int32_t num_vertices, int32_t num_faces, int32_t points_per_batch,
                                 int32_t split, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Ray casting (not in the reference's library; DESIGN "Ray casting"): rays o + t d with origins and directions [B, R, 3] -- or ONE
 * bundle [R, 3] each for the batch with rays_per_batch = 0 (any value but 0 and 1: NR_E_MODE) --, d not normalised, world-space
 * vertices [B, Nv, 3] and ONE topology faces [F, 3] int32.  Whether a ray hits a face is csrc/nr_ray_triangle.h, one definition
 * (the same bits for the same pair): with e1 = v1 - v0, e2 = v2 - v0, pvec = d x e2, det = e1 . pvec, tvec = o - v0, qvec =
 * tvec x e1, s = sign(det), D = |det|, U = s (tvec . pvec), V = s (d . qvec), T = s (e2 . qvec) a hit iff D > 0, U >= 0, V >= 0,
 * U + V <= D, with cull = 1 det > 0 (cull neither 0 nor 1: NR_E_MODE), and near <= t < far for t = T / D (a NaN near or far:
 * NR_E_MODE; far may be +inf).  A NaN fails every test; a face with a non-finite corner and a face with D = 0 are never hit.
 *   nr_ray_mesh_first_hit: per ray the smallest t by a brute-force sweep, a strict < over ascending face numbers (the lowest
 *     face wins a tie): t [B, R], face_ids [B, R] int32, barycentric [B, R, 3] = (max((1 - w1) - w2, 0), w1 = U / D, w2 = V / D).
 *     A miss reports t = +inf, face_id = -1 and weights 0.
 *   nr_ray_mesh_any_hit: occluded [B, R] bytes, 1 when any face is hit, else 0.
 *   split: 0 lets the call decide whether to cut the faces over several workgroups, n >= 1 asks for n parts (1: none); the
 *   parts are merged in ascending order with the same strict < (with OR), so the result does not depend on it.  The workspace
 *   holds the parts: nr_ray_mesh_workspace_bytes(B, R, F, any_hit, split), 0 when the call is not split (workspace may then be
 *   NULL).
 * Sizes: 1 <= B <= 65535, B R <= (2^31 - 1) / 3, B F <= (2^31 - 1) / 18, B Nv <= (2^31 - 1) / 6 (NR_E_SIZE; also a forced
 * split that asks for more than 2^31 - 1 workgroups, for which nr_ray_mesh_workspace_bytes returns 0).  No atomics: the
 * same bits in every run, for an image alone or inside a batch, split or not.  Every output element is stored exactly once; no
 * call synchronises the host; NR_E_* before any launch (NULL before sizes, sizes before modes).
 */
size_t nr_ray_mesh_workspace_bytes(int32_t batch_size, int32_t num_rays, int32_t num_faces, int32_t any_hit, int32_t split);

int nr_ray_mesh_first_hit(const float *origins, const float *directions, const float *vertices, const int32_t *faces, float *t,
                          int32_t *face_ids, float *barycentric, int32_t batch_size, int32_t num_rays, int32_t num_vertices,
                          int32_t num_faces, int32_t rays_per_batch, double near, double far, int32_t cull, int32_t split,
                          void *workspace, size_t workspace_bytes, void *stream);

int nr_ray_mesh_any_hit(const float *origins, const float *directions, const float *vertices, const int32_t *faces,
                        unsigned char *occluded, int32_t batch_size, int32_t num_rays, int32_t num_vertices, int32_t num_faces,
                        int32_t rays_per_batch, double near, double far, int32_t cull, int32_t split, void *workspace,
                        size_t workspace_bytes, void *stream);

/*
 * Isosurface extraction (not in the reference's library; DESIGN "Isosurface extraction"): marching tetrahedra on values
 * [B, D, H, W] at the level iso (rounded to float32), inside = value < iso (above = 0) or value > iso (above = 1; neither: NR_E_MODE,
 * as a non-finite iso); a node at iso is outside.  The cut of a cell, the triangles of every case, their orientation and the
 * order of vertices and faces are csrc/nr_marching_tets.h, one definition.  Two calls around ONE readback by the caller:
 *   nr_isosurface_count: fills the workspace and totals [B, 3] int32 = per image the number of vertices, the number of
 *     triangles (read it as unsigned) and 1 where the image holds a non-finite value (its counts then mean nothing).
 *   nr_isosurface_emit: with the SAME workspace, untouched in between, and the same B, D, H, W, run: edge_nodes [num_vertices, 2]
 *     int32 -- the nodes a < b (linear indices within the image) of each vertex's edge -- and faces [num_faces, 3] int32 -- vertex
 *     numbers within the image --, the images one behind the other in the order of the batch; num_vertices and num_faces are
 *     the sums of the totals (the rows the caller allocated: no store goes beyond them; both 0: nothing is launched and the
 *     pointers may be NULL).  It reads the workspace only, not the values.
 *   run: the nodes a workgroup walks, 0 = the library's choice, at most 4096 (else NR_E_SIZE); the result does not depend on it.
 *   nr_isosurface_workspace_bytes(B, D, H, W, run): 6 bytes per node and 20 per workgroup; 0 for sizes out of range.
 * Sizes: 1 <= B <= 65535, D, H, W >= 2, 7 D H W < 2^31 (NR_E_SIZE).  No atomics and no workgroup that waits for another: the same
 * bits in every run, for an image alone or inside a batch.  No call synchronises the host; NR_E_* before any launch.
 */
size_t nr_isosurface_workspace_bytes(int32_t batch_size, int32_t depth, int32_t height, int32_t width, int32_t run);

int nr_isosurface_count(const float *values, int32_t *totals, int32_t batch_size, int32_t depth, int32_t height, int32_t width,
                        double iso, int32_t above, int32_t run, void *workspace, size_t workspace_bytes, void *stream);

int nr_isosurface_emit(int32_t *edge_nodes, int32_t *faces, size_t num_vertices, size_t num_faces, int32_t batch_size,
                       int32_t depth, int32_t height, int32_t width, int32_t run, void *workspace, size_t workspace_bytes,
                       void *stream);

/*
 * Image losses (not in the reference; DESIGN "Image losses"): the objective of a fit on images, one loss per image, on an
 * image pyramid of `levels` in 1 .. 5 levels.  P_0(z) = z; P_l(z) is the 2 x 2 mean of P_(l-1)(z),
 * (((p00 + p01) + p10) + p11) * 0.25f with the upper row first, in float32.  H and W must be multiples of 2^(levels - 1)
 * (NR_E_SIZE).  level_weights is a HOST array of `levels` doubles, read during the call and handed to the kernels by value.
 *   IoU, alpha [B, H, W], target [B, H, W] (target_per_image = 1) or [H, W] (0: one target for the batch, read in place):
 *     a_l = P_l(alpha), t_l = P_l(target), I_l = sum a_l t_l, U_l = sum (a_l + t_l - a_l t_l),
 *     loss[b] = sum_l w_l (1 - I_l / (U_l + eps)).  Two empty silhouettes give exactly sum w_l.  sums [B, 2 levels] doubles
 *     (or NULL) receives I_0, U_0, I_1, U_1, ... for the backward, which reads the target and these sums, not alpha:
 *     grad_alpha[b, p] = -g_b sum_l w_l 4^-l (t_l(P) (U_l + eps) - I_l (1 - t_l(P))) / (U_l + eps)^2, P the level-l block of p.
 *   Squared error, images [B, C, H, W], target [B, C, H, W] or [C, H, W], mask [B, H, W] or [H, W] or NULL (= 1), the mask
 *     applied to every channel: d = mask (images - target), d_l = P_l(d), loss[b] = sum_l w_l sum_(c, P) d_l^2;
 *     grad_images[b, c, p] = sum_l 2 g_b w_l 4^-l mask(p) d_l(c, P), the differences recomputed.
 * No gradient to target or mask.  The sums of an image: per tile of 64 x 16 pixels a double sum per level in a fixed order
 * into the workspace (nr_image_loss_workspace_bytes; 0 for sizes out of range), the tiles added in tile order in double by a
 * second kernel, the loss evaluated in double and rounded once.  Each backward is one launch.  No atomics in any kernel: the
 * same bits in every run, and an image alone gives the bits it has in a batch.  16-byte loads when W is a multiple of 4
 * and the pointers are 16-byte aligned.  The float operation order: the header comment of csrc/nr_image_losses.hip.  Every
 * output element is stored; no call synchronises the host or reads device memory on the host; NR_E_* before any launch.
 */
size_t nr_image_loss_workspace_bytes(int32_t batch_size, int32_t height, int32_t width, int32_t levels);

int nr_iou_loss_forward(const float *alpha, const float *target, int32_t target_per_image, const double *level_weights,
                        float *loss, double *sums, int32_t batch_size, int32_t height, int32_t width, int32_t levels,
                        double eps, void *workspace, size_t workspace_bytes, void *stream);

int nr_iou_loss_backward(const float *target, int32_t target_per_image, const double *sums, const double *level_weights,
                         const float *grad_loss, float *grad_alpha, int32_t batch_size, int32_t height, int32_t width,
                         int32_t levels, double eps, void *stream);

int nr_squared_error_forward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                             int32_t mask_per_image, const double *level_weights, float *loss, int32_t batch_size,
                             int32_t channels, int32_t height, int32_t width, int32_t levels, void *workspace,
                             size_t workspace_bytes, void *stream);

int nr_squared_error_backward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                              int32_t mask_per_image, const double *level_weights, const float *grad_loss,
                              float *grad_images, int32_t batch_size, int32_t channels, int32_t height, int32_t width,
                              int32_t levels, void *stream);

/*
 * SSIM loss (not in the reference; DESIGN "Image losses: SSIM"): the structural similarity of images [B, C, H, W] and a target
 * [B, C, H, W] (target_per_image = 1) or [C, H, W] (0: one target for the batch, read in place) under a mask [B, H, W] or
 * [H, W] or NULL (= 1) that applies to every channel.  window: a HOST array of window_size = 2R + 1 floats w, window_size odd
 * in 3 .. 11 (NR_E_SIZE otherwise), read during the call and handed to the kernels by value; the 2-D window is w (x) w and G*z
 * the windowed sum of z.  valid = 0 ('same'): z reads as 0 outside the image and every pixel is a window centre, Hq x Wq =
 * H x W; valid = 1: only the windows inside the image, Hq x Wq = (H - 2R) x (W - 2R) (NR_E_SIZE when that is empty).  Per
 * channel and window centre q, in float32:
 *     mu_x = G*x, mu_y = G*y, sxx = G*(x x) - mu_x^2, syy = G*(y y) - mu_y^2, sxy = G*(x y) - mu_x mu_y,
 *     a1 = 2 mu_x mu_y + c1, a2 = 2 sxy + c2, b1 = mu_x^2 + mu_y^2 + c1, b2 = sxx + syy + c2, S = (a1 a2) / (b1 b2)
 *   (c1, c2 rounded to float32), and
 *     loss[b] = k sum_(c, q) m_b(q) (1 - S_c(q)),
 *   m the mask at the window's centre pixel, k = 1 (mean = 0) or 1 / (C sum_q m_b(q)) (mean = 1; 0 when that sum is 0).
 *   Bit-equal images and target give S = 1 at every window and a loss of exactly 0.
 * The forward stores S into ssim_map [B, C, Hq, Wq] when that is given, and, when grad_maps [3, B, C, Hq, Wq] and scales [B]
 * doubles are given (both or neither: NR_E_NULL), what the backward reads: the maps
 *     M3 = dS/dsxy = 2 a1 / (b1 b2),  M2 = dS/dsxx = -S / b2,
 *     M1 = 2 mu_y a2 / (b1 b2) - 2 mu_x S / b1 - 2 mu_x M2 - mu_y M3,
 *   which depend on neither g, k nor the mask, and k per image.  The backward is a gather over the windows that contain a pixel:
 *     grad_images[b, c, p] = -g_b k_b sum_q m_b(q) w(q - p) (M1(q) + 2 x(p) M2(q) + y(p) M3(q)).
 * No gradient to target or mask.  The sums of an image: per tile of 64 x 16 window centres a double sum of m (1 - S) and of m
 * in a fixed order into the workspace (nr_ssim_workspace_bytes; 0 for sizes out of range), the tiles added in tile order in
 * double by a second kernel, the loss evaluated in double and rounded once.  The backward is one launch.  No atomics in any
 * kernel: the same bits in every run, and an image alone gives the bits it has in a batch.  16-byte loads and stores where
 * a plane's width is a multiple of 4 and its pointer is 16-byte aligned.  The float operation order: the header comment of
 * csrc/nr_ssim.hip.  Every output element is stored; no call synchronises the host or reads device memory on the host;
 * NR_E_* before any launch.
 */
size_t nr_ssim_workspace_bytes(int32_t batch_size, int32_t height, int32_t width, int32_t window_size, int32_t valid);

int nr_ssim_loss_forward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                         int32_t mask_per_image, const float *window, float *loss, float *ssim_map, float *grad_maps,
                         double *scales, int32_t batch_size, int32_t channels, int32_t height, int32_t width,
                         int32_t window_size, int32_t valid, int32_t mean, double c1, double c2, void *workspace,
                         size_t workspace_bytes, void *stream);

int nr_ssim_loss_backward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                          int32_t mask_per_image, const float *window, const float *grad_maps, const double *scales,
                          const float *grad_loss, float *grad_images, int32_t batch_size, int32_t channels, int32_t height,
                          int32_t width, int32_t window_size, int32_t valid, void *stream);

/*
 * Mesh subdivision (not in the reference; DESIGN "Mesh subdivision"): one level of Loop or midpoint refinement is a sparse
 * linear operator on per-vertex data, given as a host-built CSR table (neural_renderer_amd/subdivision.py) with a row per
 * output vertex; the backward of a level is the transposed table, a row per input vertex, applied by the same call.
 *   One level on faces [F, 3] over Nv vertices.  Edges: every unordered pair {p < q} that is a side of a face, E of them,
 *   ordered by (p, q); edge e owns new vertex Nv + e and old vertices keep their indices, Nv' = Nv + E.  m(e): the (face,
 *   side) occurrences of e, duplicate faces counted; e is sharp when m(e) != 2.  Face f = (a, b, c) becomes faces
 *   4 f .. 4 f + 3 = (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca).
 *     midpoint: old vertex {v: 1}; edge vertex {p: 1/2, q: 1/2}.
 *     loop, N(v) the distinct vertices joined to v by an edge, n = |N(v)|, s(v) the sharp edges at v:
 *       old vertex: n = 0: {v: 1};  s = 0: beta = 3/16 if n = 3 else 3 / (8 n), {v: 1 - n beta, u: beta for u in N(v)};
 *                   s = 2: {v: 3/4, the two sharp neighbours: 1/8 each};  any other s: {v: 1};
 *       edge vertex: sharp: {p: 1/2, q: 1/2};  m = 2: {p: 3/8, q: 3/8, o1: 1/8, o2: 1/8}, o1 / o2 the opposite vertices.
 *   Weights in float64, entries of a row with one column added in float64, rounded to float32 once; rows sum to 1.
 * nr_stencil_apply: x [B, num_in, C] -> y [B, num_out, C], C = channels in 1 .. 16 (NR_E_SIZE otherwise, as batch_size >
 * 65535), with row_offsets [num_out + 1], cols and weights [num_entries], the entries of a row in ascending column:
 *   acc = w_0 * x_0 (one rounding), then acc = fmaf(w_k, x_k, acc) in table order; a row without entries gives 0.
 * A row {v: 1} copies its input bit for bit.  No atomics; every output element is stored; the same bits in every run, and
 * an image alone gives the bits it has inside a batch.  One launch; the call does not synchronise the host or read device
 * memory on the host; NR_E_* before any launch.
 */
int nr_stencil_apply(const float *x, const int32_t *row_offsets, const int32_t *cols, const float *weights, float *y,
                     int32_t batch_size, int32_t num_in, int32_t num_out, int32_t channels, int32_t num_entries,
                     void *stream);

/*
 * Learnable lights (not in the reference; DESIGN "Learnable lights"): the light colour of every face (flat) or of every face
 * corner (smooth) from world-space vertices and light parameters that live in DEVICE memory -- shared by the batch or one per
 * image, possibly learnable -- with gradients to the vertices and to every parameter.  The result is what the rasterizer
 * takes as its face light (nr_face_light.light [B, F, 3], nr_corner_light.light [B, F, 3, 3]).
 *
 * With n = N / (|N| + 1e-5) = (x, y, z), all float32 in this order, no multiply-add contraction:
 *   L_c(n) = Ia Ca_c + Id (Cd_c max(n . d, 0)) + sum over k = 0 .. 8, ascending, of sh[k, c] Y_k(n)
 *   Y0 = c0, Y1 = c1 y, Y2 = c1 z, Y3 = c1 x, Y4 = (c2 x) y, Y5 = (c2 y) z, Y6 = c3 ((3 z) z - 1), Y7 = (c2 x) z,
 *   Y8 = c4 (x x - y y);  c0 = 0.282095f, c1 = 0.488603f, c2 = 1.092548f, c3 = 0.315392f, c4 = 0.546274f
 * i.e. amb = Ia Ca_c, then amb + Id (Cd_c cos) exactly as nr_frontend_forward_light / nr_vertex_shade_forward, then the SH
 * terms added one by one.  n . d = (x d0 + y d1) + z d2; d is not normalised and L is not clamped: the nine sh rows are
 * IRRADIANCE coefficients (the cosine lobe already folded in).  Both lamp terms are always evaluated (an intensity of 0 is
 * a device value); the SH term is absent exactly when lights->sh is NULL.
 *   smooth = 0: N = cross(v0 - v1, v2 - v1) of the face; light_out [B, F, 3], F = Nf * (fill_back ? 2 : 1); the reversed copy
 *     Nf + f sees -n: max(-(n . d), 0), and Y1 .. Y3 with the opposite sign.
 *   smooth = 1: N = m_v, the float32 sum of the face normals over the (face, corner) pairs of vertex v in ascending order
 *     (adj_offsets / adj_entries: the table of nr_vertex_shade_forward); light_out [B, F, 3(corner), 3]: corner k of face f
 *     takes the front light of its vertex, corner 2 - k of the reversed copy Nf + f the back light, as nr_vertex_shade_forward
 *     lays out a white mesh.  The workspace holds the two colours of every vertex.
 * N = 0 (a degenerate face, a vertex without a face) gives n = 0: L = Ia Ca + c0 sh[0] - c3 sh[6], and no gradient to the
 * vertices.  The derivative of max(., 0) is taken for n . d > 0 strictly.
 *
 * Backward from grad_light (the layout of light_out).  grad_vertices [B, Nv, 3] (or NULL): light -> n -> normalisation ->
 * cross product, every sum around a vertex a gather through the table in ascending order; the directional part has the
 * operation order of nr_vertex_shade_backward.  The parameter gradients (nr_lights_grad, each with its parameter's layout,
 * NULL = not needed) are linear in 36 sums per image over the faces (flat) or the vertices (smooth, the corner gradients
 * around a vertex gathered first), the front and the reversed copy entering with n and -n, G their gradient:
 *   S[phi, c] = sum phi G_c for phi in {1, cos, Y0 .. Y8};   T = sum [+-n . d > 0] (+-n) (G . Cd)
 *   g_Ia = sum_c S[1, c] Ca_c,  g_Ca = Ia S[1, .],  g_Id = sum_c S[cos, c] Cd_c,  g_Cd = Id S[cos, .],  g_dir = Id T,
 *   g_sh[k, .] = S[Y_k, .]
 * accumulated in double: every block of 256 items writes its sums into the workspace in a fixed order, a second kernel adds
 * the blocks in block order -- for a shared parameter the images' contributions in image order -- and rounds once.  Sums
 * whose gradients are all NULL are not formed; without grad_vertices the vertex kernels are not launched.  No atomics: every
 * output repeats bit for bit, and an image alone gives the bits it has inside a batch.
 *
 * Every output element is stored.  nr_lights and nr_lights_grad are HOST structs read during the call; all their pointers
 * are device memory.  The workspace (nr_light_colors_workspace_bytes; 0 for sizes out of range) serves both directions: the
 * forward needs it with smooth = 1, the backward for parameter gradients and, with smooth = 1, for grad_vertices.  The
 * adjacency table is needed by the forward with smooth = 1 and by every backward.  NR_E_* before any launch (NR_E_MODE: a
 * backward with nothing to compute, smooth not 0 / 1, per_image bits beyond the six); no call synchronises the host.
 */
typedef struct nr_lights {
    const float *intensity_ambient;     /* [1] | [B] */
    const float *intensity_directional; /* [1] | [B] */
    const float *color_ambient;         /* [3] | [B, 3] */
    const float *color_directional;     /* [3] | [B, 3] */
    const float *direction;             /* [3] | [B, 3] */
    const float *sh;                    /* [9, 3] | [B, 9, 3]; NULL: no SH term */
    int32_t per_image;                  /* bit j: parameter j (in the order above) is one per image */
} nr_lights;

typedef struct nr_lights_grad {
    float *intensity_ambient, *intensity_directional, *color_ambient, *color_directional, *direction, *sh;
} nr_lights_grad;

size_t nr_light_colors_workspace_bytes(int32_t batch_size, int32_t num_vertices, int32_t num_faces, int32_t smooth);

int nr_light_colors_forward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                            const int32_t *adj_entries, const nr_lights *lights, float *light_out, int32_t batch_size,
                            int32_t num_vertices, int32_t num_faces, int32_t idx_per_batch, int32_t fill_back, int32_t smooth,
                            void *workspace, size_t workspace_bytes, void *stream);

int nr_light_colors_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                             const int32_t *adj_entries, const nr_lights *lights, const float *grad_light,
                             float *grad_vertices, const nr_lights_grad *grads, int32_t batch_size, int32_t num_vertices,
                             int32_t num_faces, int32_t idx_per_batch, int32_t fill_back, int32_t smooth, void *workspace,
                             size_t workspace_bytes, void *stream);

/*
 * Texture atlas of save_obj(..., textures) (K11, reference save_obj.py:10-146): image [tile_height*tso, tile_width*tso, 3]
 * (NOT yet flipped) from textures [Nf,tsi,tsi,tsi,3] and the per-face tile triangles tile_vertices [Nf,3,2] in atlas pixel
 * coordinates (save_obj.py:17-25); tiles beyond the last face are written as 0.  Includes the seam pass (:115-146).
 */
int nr_create_texture_image(const float *textures, const float *tile_vertices, float *image, int32_t num_faces,
                            int32_t texture_size_in, int32_t texture_size_out, int32_t tile_width, int32_t tile_height,
                            void *stream);

/*
 * Masked Adam update (reference optimizers.py:17-34): for every element with grad != 0
 *   m += one_minus_beta1 * (grad - m);  v += one_minus_beta2 * (grad * grad - v);  v = max(v, 0);
 *   param -= lr * m / (sqrt(v) + eps);
 * elements with a zero gradient keep parameter and moments.  float32, in place; `lr` = alpha_t * the parameter's multiplier.
 */
int nr_adam_update(float *param, const float *grad, float *m, float *v, size_t count, float lr, float one_minus_beta1,
                   float one_minus_beta2, float eps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NR_HIP_H */
