/*
 * nr_hip_profile.h -- the measurement hook of the MEASUREMENT build of the library (libnr_hip_prof.so: the same sources as
 * libnr_hip.so compiled with -DNR_PROFILE_HOOK, neural_renderer_amd._build.build_profile()).  The product library
 * (include/nr_hip.h) neither exports these functions nor keeps their state: up to 0.4.1 they were part of the product ABI, which
 * put a process-wide event pair into a library whose header promises "keeps no state between calls".
 * Used by bench.py (`roofline.avg_launch_us`: the dominant kernel's own duration, measured live with HIP events on the launch
 * stream) and tests/test_hip_parity.py::test_band_kernel_timing_hook.
 */
#ifndef NR_HIP_PROFILE_H
#define NR_HIP_PROFILE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* With enable != 0 every K6 band-kernel launch of nr_backward_pixel_map /
 * nr_backward_rasterize[_lit] is bracketed by a pair of HIP events recorded on the call's stream (events of the library's own,
 * created on the first enable); nr_profile_band_kernel_ms() waits for the last pair and returns the time between them in
 * milliseconds (< 0: no launch was bracketed, or an event call failed).  That is the duration of the path's dominant kernel
 * alone, without the helper launches of its stage call, as `rocprofv3 --kernel-trace --stats` reports it.  (A fused backward
 * whose plan puts the K7 / K8 gather's workgroups behind the band kernel's in one grid -- k_band_gather, calls of more than
 * 96 k faces with texture_size 2 -- has that MERGED launch bracketed: band kernel and gather together.  bench.py's
 * `in_fused_backward_us` is then the merged launch's time; `avg_launch_us`, from nr_backward_pixel_map, stays k_bpm_row's.)
 * Process-wide, not
 * thread-safe, and the two event packets cost the stream a few microseconds per call: off outside measurements. */
int nr_profile_band_kernel(int32_t enable);
float nr_profile_band_kernel_ms(void);
/* which band kernel the last bracketed launch was: 0 k_bpm_fast, 1 k_bpm_row (-1: none) */
int nr_profile_band_kernel_which(void);
/* which band kernel a call takes, as a function of the call (host logic only, callable without a device): 1 k_bpm_row, 0
 * k_bpm_fast (NR_FLAG_K6_SCAN / _LEGACY, rasters beyond 1024, the default mode with eps = 0) or the global-memory kernel
 * (NR_FLAG_K6_GLOBAL, rasters whose band does not fit in LDS).  The batch size does not enter. */
int nr_profile_k6_choice(int32_t B, int32_t F, int32_t S, int32_t return_rgb, int32_t return_alpha, double eps, int32_t flags);

/* The launch plan of a fused backward (nr_backward_rasterize[_lit]) as a function of the call: host logic only, no launch, no
 * device.  The call is described instead of given: its sizes; which of the three upstream gradients are passed (grad_rgb /
 * grad_alpha / grad_depth != 0); eps and flags as the entry point takes them; light_texture_faces, the
 * nr_face_light::texture_faces of a call with per-face light colours (0: none; its textures are given, its grad_light iff
 * grad_light != 0); the low four bits of grad_textures' address (< 0: grad_textures is not passed); whether visible_faces is
 * passed; and workspace_bytes (0: what nr_backward_workspace_bytes says for the call).  The function builds the description the
 * entry point builds and hands it to the planning function the launch path runs; it returns that function's code (0 or an NR_E_*), and
 * on 0 writes NR_PLAN_FIELDS values to out (on an error: all -1), in this order.  The first 25 are the plan's discrete fields:
 *    0 k6               K6 runs
 *    1 kernel           K6's kernel: 0 k_bpm_fast, 1 k_bpm_row, 2 k_bpm_global (-1 without K6)
 *    2 use_records      line records from k_line_setup
 *    3 overflow_pass    k_bpm_fast's overflow pass follows k_bpm_row
 *    4 row_chunked      k_bpm_row cuts its lines into chunks
 *    5 threads          threads of k_bpm_fast's band workgroup, 256 | 512 (0 without K6)
 *    6 bands            K6 runs through the band pipeline (not k_bpm_global)
 *    7 face_zeros       the compaction's zeros of grad_faces: 0 none, 1 the unlisted faces, 2 every face
 *    8 gather_first     the gather goes out in front of the band kernel
 *    9 gather_in_tail   the gather's workgroups behind the band kernel's in one grid
 *   10 setup_alone      k_line_setup as a launch of its own
 *   11 setup_in_gather  k_line_setup inside the gather's launch
 *   12 tex_zeros        who zeroes grad_textures: 0 nobody, 1 the band kernel, 2 k_setup_gather, 3 a fill launch, 4 the band
 *                       kernel, the unlisted faces' cubes only
 *   13 light_fill       grad_light zero-filled in front of the gather
 *   14 gather           K7's gather: 0 none, 1 per face, 2 per-pixel atomics
 *   15 listed           the face gather and k_backward_big walk K6's lists
 *   16 static_taps      texture_size 2 on static taps
 *   17 lanes            lanes per face in the face gather (16 | 64 | 256; 0 without K7)
 *   18 depth_in_gather  K8 rides in the K7 gather
 *   19 big              k_backward_big follows the face gather
 *   20 big_overflow     ... with K6's overflow pass in its launch
 *   21 finish           who rounds K6's sums into grad_faces: 0 nobody, 1 k_bpm_finalize, 2 the gather, 3 k_backward_big,
 *                       4 k_bpm_finalize adding onto K8's sums
 *   22 depth            K8 as launches of its own
 *   23 fill_faces       grad_faces zero-filled (a call without K6)
 *   24 depth_lists      ... and K8's lists built from the forward's flags
 * and the sizes that the thresholds compare:
 *   25 tex_bytes        grad_textures' bytes
 *   26 gather_lds       the face gather's dynamic LDS bytes
 *   27 fast_lds, 28 row_lds   the band kernels' LDS bytes
 *   29 fill_max         the largest zero fill that the band kernel takes along
 *   30 W_fast, 31 W_row, 32 W, 33 n_bands   band widths (lines) of the two band kernels and of the band tables, bands per image
 *   34 setup_lds        k_line_setup's dynamic LDS bytes (0 without line records)
 */
#define NR_PLAN_FIELDS 35
int nr_profile_backward_plan(int32_t B, int32_t F, int32_t S, int32_t ts, int32_t grad_rgb, int32_t grad_alpha, int32_t grad_depth,
                             double eps, int32_t flags, int32_t light_texture_faces, int32_t grad_light,
                             int32_t grad_textures_low_bits, int32_t visible_faces, size_t workspace_bytes, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* NR_HIP_PROFILE_H */
