// nr_backward.hip -- the backward's C-ABI entry points (K6 nr_backward_pixel_map, K7 nr_backward_textures, K8
// nr_backward_depth_map, and all three fused: nr_backward_rasterize[_lit], rasterize.py:849-889), the plan that decides a
// call's launches and the executor that launches them.  The kernels and their host-side steps live in
// nr_backward_pixel_map.hip (K6) and nr_backward_gather.hip (K7 / K8).
#include "nr_device.h"
#include "nr_band_lines.h"
#include "nr_k6_tune.h"

using namespace nr;

// Every argument check of the call, then every launch decision.  The fused backward reuses the visible-face lists built for K6
// in the K7 / K8 gathers, which then visit ~1/5 of the faces; its results are those of the three stages in the reference's order.
int nr::plan_backward(const BackwardCall &c, BackwardPlan &p)
{
    p = {};
    const bool fused = c.stages == STAGE_ALL;
    const bool k6 = (c.stages & STAGE_K6) && (c.rgb || c.alpha);
    const bool k7 = (c.stages & STAGE_K7) && (!fused || (c.grad_rgb_map && c.grad_textures));
    const bool k8 = (c.stages & STAGE_K8) && (!fused || c.grad_depth_map);
    const bool sampled = c.sampling_weight_map != nullptr;
    if (!c.faces || !c.face_index_map) return NR_E_NULL;
    if ((c.stages & (STAGE_K6 | STAGE_K8)) && !c.grad_faces) return NR_E_NULL;
    if (c.stages == STAGE_K6 && !k6) return NR_E_MODE;  // rasterize.py:523-524 returns early; callers skip the call
    if (k6 && c.rgb && (!c.rgb_map || !c.grad_rgb_map)) return NR_E_NULL;
    if (k6 && c.alpha && (!c.alpha_map || !c.grad_alpha_map)) return NR_E_NULL;
    if (k7) {
        if (!c.grad_rgb_map || !c.grad_textures) return NR_E_NULL;
        if ((c.sampling_index_map != nullptr) != sampled) return NR_E_MODE;
        if (!sampled && (!c.weight_map || !c.depth_map)) return NR_E_NULL;
    }
    if (k8 && (!c.depth_map || !c.weight_map || !c.grad_depth_map)) return NR_E_NULL;
    if (int e = check_sizes(c.B, c.F, c.S)) return e;
    if (k6 && (size_t)c.B * c.S * c.S > 0x7fffffffull / 3) return NR_E_SIZE;  // int32 pixel indexing inside the kernels
    if (k7 && (c.ts < 2 || c.ts > 1024)) return NR_E_SIZE;
    if (k7 && c.lit.light && sampled) return NR_E_MODE;  // (the taps are recomputed in the original cube's layout)
    if (k7 && (c.flags & NR_FLAG_SHARED_TEXTURES)) return NR_E_MODE;  // (K7 strides the cubes by the batch: nr_backward_textures_shared)

    const int B = c.B, F = c.F, ts = c.ts;
    p.k6 = k6;
    if (k6) {
        p.k6p = plan_k6(B, F, c.S, c.rgb, c.eps, c.flags);
        p.bands = p.k6p.kernel != K6_KERNEL_GLOBAL;
        if (p.bands && (!c.workspace || c.workspace_bytes < nr_backward_workspace_bytes(B, F, c.S, 1, 0))) return NR_E_WORKSPACE;
    }
    // K6's last step (rounding the double sums into grad_faces, zeros for the unlisted faces) rides in the K7 / K8 gather's
    // launch when there is one that walks faces (texture_size <= 13)
    const bool fold = p.bands && k7 && ts <= 13;
    // Small launches (up to 96 k faces in the call: 16 views of the 4928-face teapot) take the order
    //   compaction | line setup + gather + zeros of grad_textures in ONE grid | band kernel | K6's overflow pass + the faces
    //   the gather left out + K6's sums onto grad_faces (one launch: big_overflow below)
    // where the line setup and the gather -- two chains of dependent round trips that need nothing of each other -- run side
    // by side (8 views: backward 82 -> 72 us, 16: 111 -> 104; 32: 156 -> 152, not taken).  Larger ones keep
    //   compaction | line setup | band kernel with the fill on the side | gather with K6's finish:
    // there both launches are bound by how many workgroups the chip holds, a shared grid takes the sum of their times (64
    // views: 254.7 us either way), and the fill inside the band kernel and the finish inside the gather are worth more
    // (config 4: 0.80 vs 0.87 ms, 1024 views of 32 x 32: 0.72 vs 0.85, config 5 with its 4 GB of zeros: 1.57 vs 1.97).
    p.gather_first = fold && (size_t)B * F <= k6::SHARED_LAUNCH_MAX_FACES && !(c.flags & NR_FLAG_SERIAL_BACKWARD);
    // Above that, up to TAIL_GATHER_MAX_FACES, where the gather is the static-tap face gather (texture_size 2, the Renderer's
    // default) and K6 takes k_bpm_row in the default arithmetic on whole lines:
    //   compaction | line setup | band kernel + gather in ONE grid, the gather's workgroups behind the band's | K6's overflow
    //   pass + the faces the gather left out + K6's sums onto grad_faces (one launch: big_overflow below)
    // The gather starts in the slots that the band kernel's last round frees instead of behind a launch boundary on an empty
    // chip (k_band_gather, nr_k6_row.h; measured: nr_k6_tune.h).  The band workgroups zero the unlisted faces'
    // cubes of grad_textures only: the gather of the same launch stores the listed ones.
    // static taps (TS2 path): valid when the clamp of rasterize.py:402 keeps every index float below 1, i.e. when
    // (ts - 1) - eps still rounds below ts - 1 in float32 (eps > 2^-25); otherwise a coordinate can be exactly 1.0
    const bool ts2_static = ts == 2 && (float)(1.0 - c.eps) < 1.0f;
    p.gather_in_tail = k6::TAIL_GATHER_MAX_FACES > 0 && fold && !p.gather_first && !(c.flags & NR_FLAG_SERIAL_BACKWARD) &&
                       ts2_static && !sampled && !c.lit.light && p.k6p.kernel == K6_KERNEL_ROW && !(c.flags & NR_FLAG_EXACT_GRADIENT) &&
                       !p.k6p.row_chunked && c.S <= 512 && (size_t)B * F <= k6::TAIL_GATHER_MAX_FACES;
    // the compaction stores the zeros of grad_faces that no later launch stores: of the unlisted faces when the gather's
    // epilogue stores the listed ones, of every face when the gather runs first and adds K8's sums before K6's arrive
    const bool gather_early = p.gather_first || p.gather_in_tail;  // the gather does not wait for K6's sums
    p.face_zeros = gather_early ? FACE_ZEROS_ALL : (fold ? FACE_ZEROS_UNLISTED : FACE_ZEROS_NONE);
    p.finish = !p.bands ? FINISH_NONE : gather_early ? (ts <= 8 ? FINISH_BIG : FINISH_ADD) : (fold ? FINISH_GATHER : FINISH_KERNEL);

    if (k7) {
        const size_t n_tex = (size_t)ts * ts * ts * 3;
        p.static_taps = ts2_static && !sampled;
        p.gather = ts <= 13 ? GATHER_FACE : GATHER_ATOMIC;  // (above: the per-pixel scatter)
        p.listed = p.bands && ts <= 13;                      // (the atomic fallback walks pixels, not faces)
        p.lanes = p.static_taps ? 16 : (ts <= 5 ? 16 : (ts <= 8 ? 64 : 256));
        p.gather_lds = p.static_taps ? 0 : (size_t)(256 / p.lanes) * n_tex * sizeof(double);
        p.big = ts <= 8;
        // K8 is fused only into the one-wave-per-group gathers, on recomputed taps
        p.depth_in_gather = k8 && ts <= 8 && !sampled && !(ts == 2 && !ts2_static);
        p.tex_bytes = (size_t)B * (c.lit.light ? c.lit.tex_faces : F) * n_tex * sizeof(float);
        if (p.gather_first) {
            // The line setup rides in the gather's launch (k_setup_gather) when the two fit one launch's dynamic LDS, and the
            // zeros of grad_textures ride along too (plain path), else they are filled in front.  (The shared launch's dynamic
            // LDS is the larger of the two bodies' and its static arrays -- both bodies', ~6 KB -- come on top; without a
            // hipFuncSetAttribute call a launch may use 64 KB in all, so the dynamic part is kept to 40 KB: texture_size 12
            // (41.5 KB of gather accumulators) and rasters whose line setup needs more than 32 KB take the two launches.)
            p.setup_in_gather = p.k6p.use_records && k6_line_setup_args(c, p.k6p).lds_bytes <= 32768 && p.gather_lds <= 40960;
            if (p.setup_in_gather && !c.lit.light && ((size_t)c.grad_textures & 15) == 0) p.tex_zeros = TEX_ZEROS_SETUP;
        } else if (fold && p.tex_bytes % 16 == 0 && ((size_t)c.grad_textures & 15) == 0 && p.tex_bytes <= p.k6p.fill_max) {
            // the band kernel's slices (with per-face light colours: the original cubes); beside the gather: the unlisted faces'
            p.tex_zeros = p.gather_in_tail ? TEX_ZEROS_BAND_UNLISTED : TEX_ZEROS_BAND;
        }
        // Only visible faces are visited, and the per-pixel scatter adds: everything else is zero.  With per-face light
        // colours a face and its reversed copy share one cube, and only the one that owns a pixel stores.  (Round 4 tried to
        // spare the listed faces' cubes, which the gathers store completely -- config 5: a 4 GB fill, 565 us at 7.1 TB/s --
        // with a fill predicated on K6's face -> position table: 622-787 us in four forms, the division / table load /
        // predicate cost more than the ~10 % of the bytes they save; as a launch of its own the plain fill stays.)
        if (p.tex_zeros == TEX_ZEROS_NONE && (c.lit.light || p.listed || ts > 13)) p.tex_zeros = TEX_ZEROS_FILL;
        p.light_fill = c.lit.light && c.lit.grad_light;
    }
    // The overflow pass behind k_bpm_row -- normally an empty launch -- rides in k_backward_big's when that launch finishes K6 (the
    // gather-first and the tail order), in the instantiations these two orders reach: 256-thread band workgroups, static taps, no
    // per-face light colours.  NR_FLAG_SERIAL_BACKWARD never gets here (neither order is taken).
    p.big_overflow = k6::MERGE_OVERFLOW && p.finish == FINISH_BIG && p.big && p.k6p.overflow_pass && p.k6p.shape.threads == 256 &&
                     p.static_taps && p.listed && !c.lit.light;
    p.setup_alone = p.bands && p.k6p.use_records && !p.setup_in_gather;
    p.depth = k8 && !p.depth_in_gather;
    // depth only: no K6 and therefore no lists -- built from the forward's flags when there are any (one launch), so that the
    // K8 gather visits the ~1/6 of the faces that own a pixel
    p.fill_faces = fused && !k6;  // :851
    p.depth_lists = p.fill_faces && k8 && c.visible_faces && c.workspace && k6_lists_fit(B, F, c.workspace_bytes);
    return 0;
}

// grad_textures' zeros in front of the gather, and grad_light's
static int fill_texture_zeros(const BackwardCall &c, const BackwardPlan &p)
{
    int e = p.tex_zeros == TEX_ZEROS_FILL ? fill_bytes(c.grad_textures, 0, p.tex_bytes, c.st) : 0;
    if (e == 0 && p.light_fill) e = fill_bytes(c.lit.grad_light, 0, (size_t)c.B * c.F * 3 * sizeof(float), c.st);
    return e;
}

int nr::run_backward(const BackwardCall &c)
{
    BackwardPlan p;
    if (int e = plan_backward(c, p)) return e;
    K6Lists l = {};
    if (p.fill_faces)
        if (int e = fill_bytes(c.grad_faces, 0, (size_t)c.B * c.F * 9 * sizeof(float), c.st)) return e;
    if (p.depth_lists) l = k6_list_visible(c);
    LineSetupArgs ls = {};
    if (p.k6) {
        if (p.bands) {
            if (int rc = k6_compact(c, p.k6p, p.face_zeros, l)) return rc;
            ls = k6_line_setup_args(c, p.k6p);
        }
        if (p.gather_first) {
            if (int rc = fill_texture_zeros(c, p)) return rc;
            if (int rc = gather_faces(c, p, l, p.setup_in_gather ? &ls : nullptr)) return rc;
        }
        if (p.setup_alone)
            if (int rc = run_line_setup(ls, c.st)) return rc;
        if (p.gather_in_tail)  // (a fill too large for the band workgroups goes out in front of the launch whose gather stores)
            if (int rc = fill_texture_zeros(c, p)) return rc;
        const bool band_fill = p.tex_zeros == TEX_ZEROS_BAND || p.tex_zeros == TEX_ZEROS_BAND_UNLISTED;
        if (int rc = k6_band(c, p.k6p, l, ls, band_fill ? c.grad_textures : nullptr, band_fill ? p.tex_bytes : 0,
                             p.gather_in_tail ? &p : nullptr, p.big_overflow))
            return rc;
        if (p.finish == FINISH_KERNEL) k6_finalize(c, l, false);
    }
    if (p.gather != GATHER_NONE && !p.gather_first && !p.gather_in_tail) {
        if (int rc = fill_texture_zeros(c, p)) return rc;
        if (p.gather == GATHER_FACE)
            if (int rc = gather_faces(c, p, l, nullptr)) return rc;
    }
    if (p.big_overflow) {
        if (int rc = k6_big_overflow(c, p, l, ls)) return rc;
    } else if (p.big) {
        gather_big(c, p, l);
    }
    if (p.gather == GATHER_ATOMIC) gather_atomic(c);
    if (p.depth) gather_depth(c, l);
    if (p.finish == FINISH_ADD) k6_finalize(c, l, true);
    return launch_status();
}

NR_API int nr_backward_pixel_map(const float *faces, const int32_t *face_index_map, const float *rgb_map,
                                 const float *alpha_map, const float *grad_rgb_map, const float *grad_alpha_map,
                                 float *grad_faces, int32_t B, int32_t F, int32_t S, double eps, int32_t return_rgb,
                                 int32_t return_alpha, int32_t flags, const uint8_t *visible_faces, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    BackwardCall c = {};
    c.stages = STAGE_K6, c.rgb = return_rgb != 0, c.alpha = return_alpha != 0;
    c.faces = faces, c.face_index_map = face_index_map, c.rgb_map = rgb_map, c.alpha_map = alpha_map;
    c.grad_rgb_map = grad_rgb_map, c.grad_alpha_map = grad_alpha_map, c.grad_faces = grad_faces;
    c.B = B, c.F = F, c.S = S, c.eps = eps, c.flags = flags, c.visible_faces = visible_faces;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.st = (hipStream_t)stream;
    return run_backward(c);
}

NR_API int nr_backward_textures(const int32_t *face_index_map, const float *sampling_weight_map,
                                const int32_t *sampling_index_map, const float *faces, const float *faces_z_ref,
                                const float *weight_map, const float *depth_map, const float *grad_rgb_map,
                                float *grad_textures, int32_t B, int32_t F, int32_t S, int32_t ts, double eps, int32_t flags,
                                void *stream)
{
    BackwardCall c = {};
    c.stages = STAGE_K7;
    c.faces = faces, c.faces_z_ref = faces_z_ref, c.face_index_map = face_index_map;
    c.sampling_weight_map = sampling_weight_map, c.sampling_index_map = sampling_index_map;
    c.weight_map = weight_map, c.depth_map = depth_map, c.grad_rgb_map = grad_rgb_map, c.grad_textures = grad_textures;
    c.B = B, c.F = F, c.S = S, c.ts = ts, c.eps = eps, c.flags = flags, c.st = (hipStream_t)stream;
    return run_backward(c);
}

NR_API int nr_backward_depth_map(const float *faces, const float *depth_map, const int32_t *face_index_map,
                                 const float *face_inv_map, const float *weight_map, const float *grad_depth_map,
                                 float *grad_faces, int32_t B, int32_t F, int32_t S, void *stream)
{
    BackwardCall c = {};
    c.stages = STAGE_K8;
    c.faces = faces, c.face_index_map = face_index_map, c.face_inv_map = face_inv_map, c.weight_map = weight_map;
    c.depth_map = depth_map, c.grad_depth_map = grad_depth_map, c.grad_faces = grad_faces;
    c.B = B, c.F = F, c.S = S, c.st = (hipStream_t)stream;
    return run_backward(c);
}

NR_API int nr_backward_rasterize(const float *faces, const float *faces_z_ref, const int32_t *face_index_map,
                                 const float *weight_map, const float *depth_map, const float *rgb_map,
                                 const float *alpha_map, const float *grad_rgb_map, const float *grad_alpha_map,
                                 const float *grad_depth_map, float *grad_faces, float *grad_textures, int32_t B,
                                 int32_t F, int32_t S, int32_t ts, double eps, int32_t flags,
                                 const uint8_t *visible_faces, void *workspace, size_t workspace_bytes, void *stream)
{
    return nr_backward_rasterize_lit(nullptr, faces, faces_z_ref, face_index_map, weight_map, depth_map, rgb_map, alpha_map,
                                     grad_rgb_map, grad_alpha_map, grad_depth_map, grad_faces, grad_textures, B, F, S, ts,
                                     eps, flags, visible_faces, workspace, workspace_bytes, stream);
}

// The fused call as plan_backward and run_backward see it: what the entry point below hands on (and what the measurement build's
// nr_profile_backward_plan plans without launching)
static int fused_call(const nr_face_light *lit, const float *faces, const float *faces_z_ref, const int32_t *face_index_map,
                      const float *weight_map, const float *depth_map, const float *rgb_map, const float *alpha_map,
                      const float *grad_rgb_map, const float *grad_alpha_map, const float *grad_depth_map, float *grad_faces,
                      float *grad_textures, int32_t B, int32_t F, int32_t S, int32_t ts, double eps, int32_t flags,
                      const uint8_t *visible_faces, void *workspace, size_t workspace_bytes, void *stream, BackwardCall &c)
{
    c = {};
    // per-face light colours: only the texture gather sees them (the geometry gradients do not)
    if (int e = face_light_args(grad_rgb_map && grad_textures ? lit : nullptr, F, true, c.lit)) return e;
    c.stages = STAGE_ALL, c.rgb = grad_rgb_map != nullptr, c.alpha = grad_alpha_map != nullptr;
    c.faces = faces, c.faces_z_ref = faces_z_ref, c.face_index_map = face_index_map, c.weight_map = weight_map;
    c.depth_map = depth_map, c.rgb_map = c.rgb ? rgb_map : nullptr, c.alpha_map = c.alpha ? alpha_map : nullptr;
    c.grad_rgb_map = grad_rgb_map, c.grad_alpha_map = grad_alpha_map, c.grad_depth_map = grad_depth_map;
    c.grad_faces = grad_faces, c.grad_textures = grad_textures;
    c.B = B, c.F = F, c.S = S, c.ts = ts, c.eps = eps, c.flags = flags, c.visible_faces = visible_faces;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.st = (hipStream_t)stream;
    return 0;
}

NR_API int nr_backward_rasterize_lit(const nr_face_light *lit, const float *faces, const float *faces_z_ref,
                                     const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                     const float *rgb_map, const float *alpha_map, const float *grad_rgb_map,
                                     const float *grad_alpha_map, const float *grad_depth_map, float *grad_faces,
                                     float *grad_textures, int32_t B, int32_t F, int32_t S, int32_t ts, double eps,
                                     int32_t flags, const uint8_t *visible_faces, void *workspace, size_t workspace_bytes,
                                     void *stream)
{
    BackwardCall c;
    if (int e = fused_call(lit, faces, faces_z_ref, face_index_map, weight_map, depth_map, rgb_map, alpha_map, grad_rgb_map,
                           grad_alpha_map, grad_depth_map, grad_faces, grad_textures, B, F, S, ts, eps, flags, visible_faces,
                           workspace, workspace_bytes, stream, c))
        return e;
    return run_backward(c);
}

// Measurement build only (include/nr_hip_profile.h): the plan of a fused call, read without a launch and without a device.  The
// pointers are stand-ins that nothing dereferences: plan_backward looks at which are given and at grad_textures' low bits.
#ifdef NR_PROFILE_HOOK
#include "../../include/nr_hip_profile.h"
NR_API int nr_profile_backward_plan(int32_t B, int32_t F, int32_t S, int32_t ts, int32_t grad_rgb, int32_t grad_alpha,
                                    int32_t grad_depth, double eps, int32_t flags, int32_t light_texture_faces, int32_t grad_light,
                                    int32_t grad_textures_low_bits, int32_t visible_faces, size_t workspace_bytes, int64_t *out)
{
    if (!out) return NR_E_NULL;
    for (int i = 0; i < NR_PLAN_FIELDS; ++i) out[i] = -1;
    float *const given = reinterpret_cast<float *>((uintptr_t)1 << 20);  // a 16-byte aligned stand-in address
    float *const gt = grad_textures_low_bits < 0 ? nullptr  // (a call whose colours come from another shading source: no K7)
                                                 : reinterpret_cast<float *>(((uintptr_t)1 << 21) + (uintptr_t)(grad_textures_low_bits & 15));
    nr_face_light lit = {};
    lit.light = given, lit.texture_faces = light_texture_faces, lit.textures = given, lit.grad_light = grad_light ? given : nullptr;
    if (workspace_bytes == 0) workspace_bytes = nr_backward_workspace_bytes(B, F, S, grad_rgb != 0, grad_alpha != 0);
    BackwardCall c;
    if (int e = fused_call(light_texture_faces ? &lit : nullptr, given, nullptr, (const int32_t *)given, given, given, given, given,
                           grad_rgb ? given : nullptr, grad_alpha ? given : nullptr, grad_depth ? given : nullptr, given,
                           gt, B, F, S, ts, eps, flags, visible_faces ? (const uint8_t *)given : nullptr,
                           given, workspace_bytes, nullptr, c))
        return e;
    BackwardPlan p;
    if (int e = plan_backward(c, p)) return e;
    const K6Plan &k = p.k6p;
    const int64_t v[NR_PLAN_FIELDS] = {
        p.k6, p.k6 ? k.kernel : -1, k.use_records, k.overflow_pass, k.row_chunked, p.k6 ? k.shape.threads : 0,
        p.bands, p.face_zeros, p.gather_first, p.gather_in_tail, p.setup_alone, p.setup_in_gather, p.tex_zeros, p.light_fill,
        p.gather, p.listed, p.static_taps, p.lanes, p.depth_in_gather, p.big, p.big_overflow, p.finish, p.depth, p.fill_faces,
        p.depth_lists,
        (int64_t)p.tex_bytes, (int64_t)p.gather_lds, (int64_t)k.fast_lds, (int64_t)k.row_lds, (int64_t)k.fill_max, k.W_fast, k.W_row,
        k.W, k.n_bands,
        p.bands && k.use_records ? (int64_t)k6_line_setup_args(c, k).lds_bytes : 0};
    for (int i = 0; i < NR_PLAN_FIELDS; ++i) out[i] = v[i];
    return 0;
}
#endif
