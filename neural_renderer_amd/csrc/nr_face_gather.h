// nr_face_gather.h -- the K7 / K8 face gather's kernel body (one face per group of lanes, walking the pixels the face owns) and
// what it needs.
//
// Shared by nr_backward_gather.hip (k_backward_textures_face, k_setup_gather) and nr_backward_pixel_map.hip (nr_k6_row.h), whose merged
// launch k_band_gather runs the gather's workgroups behind the band kernel's in ONE grid: both are bound by the workgroups the
// chip holds, and the gather's fill the slots that the band kernel's last round frees.
#pragma once
#include "nr_device.h"

namespace nr {
namespace {

constexpr int BIG_PX = 2048;  // candidate sets above this size are walked by k_backward_big (A/B on config 4: 256 cost 0.25 ms)

__device__ __forceinline__ float group_sum(float v, int width)
{
    for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// Sum over a 16-lane group (= one DPP row), delivered in the group's LAST lane (sub == 15): four v_add_f32 with a row_shr
// DPP operand (lanes shifted in from outside the row read 0) instead of four LDS-crossbar swizzles + adds per value.  The 33
// sums of a face (24 texel + 9 vertex accumulators) make this the longest instruction run of the gather kernels.
__device__ __forceinline__ float row16_sum_last(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));  // row_shr:1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));  // row_shr:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true));  // row_shr:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true));  // row_shr:8
    return v;
}

// K8's per-face constants (rasterize.py:830-833) when the inverse matrix is recomputed from the vertices: tmp_l = sum_m
// -face_inv[m][l] / z_m, evaluated ONCE per face with the reference's own operations (the three terms cancel: reciprocal
// shortcuts here showed up as 5e-4 in grad_faces), instead of once per pixel.  zz[k] = z_k * z_k (:826).
struct DepthConst {
    float tmp[3], zz[3];
};
__device__ __forceinline__ DepthConst depth_constants(const float f[9], int S)
{
    const float fs = (float)S;
    const float px[3] = {to_pixel(f[0], fs), to_pixel(f[3], fs), to_pixel(f[6], fs)};
    const float py[3] = {to_pixel(f[1], fs), to_pixel(f[4], fs), to_pixel(f[7], fs)};
    float inv[9];
    compute_face_inv(px, py, inv);
    DepthConst d;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d.tmp[k] = 0.0f;
#pragma unroll
        for (int l = 0; l < 3; l++) d.tmp[k] += -inv[3 * l + k] / f[3 * l + 2];
        d.zz[k] = f[3 * k + 2] * f[3 * k + 2];
    }
    return d;
}

// Walk of a face's candidate pixels by its group of L lanes, the lanes of a wave in step, in two passes.  Ownership pass: one
// lane per candidate, only face_index_map is read; the owned pixels (a quarter of a typical box) are ballot-compacted into
// the group's LDS queue.  Evaluation pass: whenever a group has QL pixels waiting -- and once at the end, for all groups of the
// wave together -- each lane takes one owned pixel and calls eval(pixel offset in the image).  (With the ownership test in
// front of the evaluation in one loop, the evaluation ran in every candidate step in which *any* lane of the wave owned its
// pixel: three to four times per wave instead of once or twice.)  The order in which a lane meets its pixels, and therefore
// the rounding of its float sums, is fixed by the candidate order: results are reproducible and identical between the
// kernels that use this walk.
//   n_mine: candidates of this lane's face (0: none, the lane only keeps step); queue: 2 * QL words of LDS per queue group
//   (QL = min(L, 64) lanes: the face's group, or one wave of it when L == 256).
template <int STEPS, class Eval>
__device__ __forceinline__ void walk_owned_pixels(const Cand &cd, int n_mine, int fn, const int32_t *__restrict__ fi_img,
                                                  int S, int sub, int L, int *__restrict__ queue_base, Eval eval)
{
    const int tid = threadIdx.x;
    const int QL = L < 64 ? L : 64;
    int *queue = queue_base + (tid / QL) * (2 * QL);
    const int qsub = tid & (QL - 1);
    const int qshift = (tid & 63) & ~(QL - 1);
    const unsigned long long qmask = QL == 64 ? ~0ull : ((1ull << QL) - 1ull);
    int waiting = 0;
    // STEPS candidate steps per round (1 or 2): with 2, both ownership words are requested before either is used -- a face's
    // walk is a chain of dependent round trips (list, vertices, ownership, pixel data) and a workgroup's time is that chain's,
    // not its instructions' (K8's gather 62 -> 58 us) -- where the second pair of registers does not cost a wave of occupancy
    // (K7 + K8 with static taps: 95 -> 102 VGPRs, four waves per SIMD instead of five, 252 -> 261 us for the fused backward).
    // The steps themselves run one after the other, so the order in which a lane meets its pixels is the candidate order.
    for (int i = sub;; i += STEPS * L) {
        bool more2[STEPS], owned2[STEPS];
        int off2[STEPS];
#pragma unroll
        for (int h = 0; h < STEPS; ++h) {
            const int ii = i + h * L;
            more2[h] = ii < n_mine;
            int x = 0, y = 0, f = 0;
            off2[h] = 0;
            bool in = false;
            if (more2[h] && cand_pixel(cd, ii, S, x, y)) {
                off2[h] = y * S + x;
                f = fi_img[off2[h]];
                in = true;
            }
            owned2[h] = in && f == fn;
        }
        bool done = false;
#pragma unroll
        for (int h = 0; h < STEPS; ++h) {
            if (done) break;
            const bool more = more2[h], owned = owned2[h];
            const int off = off2[h];
            const bool any_more = __ballot(more) != 0ull;
            const unsigned long long m = (__ballot(owned) >> qshift) & qmask;
            if (owned) queue[waiting + __popcll(m & ((1ull << qsub) - 1ull))] = off;
            waiting += __popcll(m);
            const bool ready = waiting >= QL || (!any_more && waiting > 0);
            if (__ballot(ready) != 0ull) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int take = ready ? (waiting < QL ? waiting : QL) : 0;
                const int e = qsub < take ? queue[qsub] : 0;
                const int rest = (ready && qsub + QL < waiting) ? queue[qsub + QL] : 0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                waiting -= take;
                if (ready && qsub < waiting) queue[qsub] = rest;
                if (qsub < take) eval(e);
            }
            if (!any_more) done = true;  // (the evaluation above took everything that was waiting)
        }
        if (done) break;
    }
}

// --------------------------------------------------------------------------------------------------
// B2: one face per group of L lanes (L = 16 | 64 | 256, a power of two; 256 / L faces per workgroup).
// TS2 = true: texture_size == 2 and eps > 0, so every tap index is static: corner pn -> texel
// (pn & 1) * 4 + ((pn >> 1) & 1) * 2 + ((pn >> 2) & 1)   (floor(tif) == 0 because tif <= 1 - eps, :402).
// DEPTH = true additionally evaluates K8 (backward_depth_map) for the same owned pixels and adds the face's 9
// sums onto grad_faces, so that one walk of the screen box serves both gradients (fused backward only).
// LIT = true: per-face light colours (FaceLight in nr_device.h) -- a template parameter, so that the kernels of the plain
// path are exactly what they were without it (as a run-time branch it cost them registers: K7 alone 72 -> 76 VGPRs, one
// wave of occupancy, 62 -> 71 us).
struct FaceGatherArgs {
    const int32_t *face_index_map;
    const float *sampling_weight_map;
    const int32_t *sampling_index_map;
    const float *faces, *zbase, *weight_map, *depth_map, *g_rgb;
    float *grad_textures;
    int n_faces_total, F, S, ts;
    double eps;
    int fix_batch_z, L;
    const int *vis_list, *vis_count;
    const float *g_depth;
    float *grad_faces;
    const double *k6_scratch;
    const int *slot_of;
    FaceLight lit;
};

// the gather's arguments for a call and its plan (K8 riding along and K6's finish in the epilogue as the plan says)
inline FaceGatherArgs face_gather_args(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l)
{
    const bool fold = p.finish == FINISH_GATHER;
    return {c.face_index_map, c.sampling_weight_map, c.sampling_index_map, c.faces,
            c.faces_z_ref ? c.faces_z_ref : c.faces,  // :389 reads batch 0 of the GLOBAL batch (see nr_hip.h)
            c.weight_map, c.depth_map, c.grad_rgb_map, c.grad_textures, c.B * c.F, c.F, c.S, c.ts, c.eps,
            (c.flags & NR_FLAG_FIX_TEXTURE_BATCH_Z) ? 1 : 0, p.lanes, p.listed ? l.vis_list : nullptr, l.vis_count,
            p.depth_in_gather ? c.grad_depth_map : nullptr,
            (p.depth_in_gather || fold) ? c.grad_faces : nullptr, fold ? l.scratch : nullptr,
            fold ? l.slot_of : nullptr, c.lit};
}

// bx, by: the workgroup's place in the gather's grid (blockIdx of k_backward_textures_face; k_band_gather hands the same
// pairs out in working-first order: image_fastest, nr_device.h)
template <bool TS2, bool DEPTH, bool LIT>
__device__ __forceinline__ void face_gather_body(const FaceGatherArgs &a, const int bx, const int by)
{
    const int32_t *__restrict__ face_index_map = a.face_index_map;
    const float *__restrict__ sampling_weight_map = a.sampling_weight_map;
    const int32_t *__restrict__ sampling_index_map = a.sampling_index_map;
    const float *__restrict__ faces = a.faces, *__restrict__ zbase = a.zbase, *__restrict__ weight_map = a.weight_map,
                *__restrict__ depth_map = a.depth_map, *__restrict__ g_rgb = a.g_rgb;
    float *__restrict__ grad_textures = a.grad_textures;
    const int n_faces_total = a.n_faces_total, F = a.F, S = a.S, ts = a.ts;
    const double eps = a.eps;
    const int fix_batch_z = a.fix_batch_z, L = a.L;
    const int *__restrict__ vis_list = a.vis_list, *__restrict__ vis_count = a.vis_count;
    const float *__restrict__ g_depth = a.g_depth;
    float *__restrict__ grad_faces = a.grad_faces;
    const double *__restrict__ k6_scratch = a.k6_scratch;
    const FaceLight &lit = a.lit;
    extern __shared__ __attribute__((aligned(16))) double s_acc[];  // [256 / L][ts^3 * 3] (general path)
    __shared__ int s_queue[512];  // owned pixels waiting for their evaluation (walk_owned_pixels)
    __shared__ int s_own;         // lit, L == 256: does the workgroup's face own a pixel?
    __shared__ float s_gl[3];     // lit, L == 256: the face's light-colour gradient

    const int tid = threadIdx.x;
    const int grp = tid / L, sub = tid - grp * L;
    const int n_tex = ts * ts * ts * 3;
    int gi = bx * (256 / L) + grp;  // global face index b * F + fn
    bool face_ok = gi < n_faces_total;
    int slot = 0;
    if (vis_list) {  // by = image, slot -> face through the image's visible list
        // The grid covers F list slots per image, the list holds the ~1/6 of them that own a pixel: the other workgroups
        // leave here (they used to run the 24-sum reduction below on zeros -- 40 % of the kernel's instructions at the
        // headline size).
        // (Fused backward with K6's scratch handed over: the epilogue also finishes K6 for the listed faces.  The unlisted
        // faces' zeros come from K6's compaction kernel (grad_faces) and from the fill in front of this launch (grad_textures):
        // storing them from here -- every workgroup the faces with its numbers -- was measured: neutral at the headline size,
        // +19 us on config 4 and 2.5x this kernel's time on 1024 views of 32 x 32, where 5 M faces mean 300 k workgroups that
        // each wait for a slot_of load before they can leave.)
        slot = gi;
        const int n_vis = vis_count[by];
        if (bx * (256 / L) >= n_vis) return;
        face_ok = slot < n_vis;
        // (requesting the list entry beside the list's length instead of behind it -- one round trip less in front of the walk
        // -- was measured: 48.7 vs 46.6 us at 64 views, 20.4 vs 20.0 at 8; five of six workgroups only want the length)
        gi = face_ok ? by * F + vis_list[(size_t)by * F + slot] : 0;
    }
    double *acc_l = s_acc + (size_t)grp * n_tex;

    float acc[24];
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] = 0.0f;
    float dacc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) dacc[k] = 0.0f;
    bool any_box = false;
    bool own = false;  // this lane evaluated a pixel of the face (lit: only such faces store, see FaceLight)
    if (!TS2) {
        for (int k = sub; k < n_tex; k += L) acc_l[k] = 0.0;
        if (LIT) {
            if (tid < 3) s_gl[tid] = 0.0f;
            if (tid == 0) s_own = 0;
        }
        __syncthreads();
    }

    Cand cd;
    cd.n = 0;
    int fn = 0;
    size_t img = 0;
    DepthConst dc;
#pragma unroll
    for (int k = 0; k < 3; k++) dc.tmp[k] = dc.zz[k] = 0.0f;
    float face_z[3] = {1.0f, 1.0f, 1.0f};
    // lit: the face's original cube.  Its reversed copy shares it and samples it with axes 0 and 2 exchanged: the walk below
    // flattens that copy's taps in the ORIGINAL layout (compute_taps' flip), so the sums need no transposition afterwards.
    bool flip = false;
    size_t cube = 0;  // b * Nf + original face
    if (LIT) {
        const int b = vis_list ? by : gi / F, f = gi - b * F;
        flip = f >= lit.tex_faces;
        cube = (size_t)b * lit.tex_faces + (flip ? f - lit.tex_faces : f);
    }
    if (face_ok) {
        const int b = gi / F;
        fn = gi - b * F;
        const float *f = faces + (size_t)gi * 9;
        cd = face_candidates(f[0], f[1], f[3], f[4], f[6], f[7], S);
        if (cd.n > 0 && (L == 256 || (cd.n <= BIG_PX))) {  // the rest is k_backward_big's
            any_box = true;
            if (DEPTH) {
                float fv[9];
#pragma unroll
                for (int k = 0; k < 9; k++) fv[k] = f[k];
                dc = depth_constants(fv, S);
            }
            // z of the three vertices as the forward sampled them: batch 0's geometry (zbase) unless fixed (:389, Q1)
            const float *fz = (fix_batch_z ? faces + (size_t)b * F * 9 : zbase) + (size_t)fn * 9;
            face_z[0] = fz[2]; face_z[1] = fz[5]; face_z[2] = fz[8];
            img = (size_t)b * S * S;
        }
    }
    walk_owned_pixels<(TS2 && DEPTH) ? 1 : 2>(cd, any_box ? cd.n : 0, fn, face_index_map + img, S, sub, L, s_queue, [&](int off) {
        const size_t p = img + (size_t)off;
        float wk[3] = {0.0f, 0.0f, 0.0f}, depth = 0.0f, gd = 0.0f;
        if (weight_map) { wk[0] = weight_map[3 * p]; wk[1] = weight_map[3 * p + 1]; wk[2] = weight_map[3 * p + 2]; }
        if (depth_map) depth = depth_map[p];
        if (DEPTH) gd = g_depth[p];
        const float g[3] = {g_rgb[3 * p], g_rgb[3 * p + 1], g_rgb[3 * p + 2]};
        if (LIT) own = true;
        Taps t;
        if (sampling_weight_map) {
#pragma unroll
            for (int pn = 0; pn < 8; pn++) {
                t.w[pn] = sampling_weight_map[8 * p + pn];
                t.isc[pn] = sampling_index_map[8 * p + pn];
            }
        } else {
            compute_taps(face_z, wk, depth, ts, eps, t, LIT && flip);
        }
        if (DEPTH) {  // [k8-terms] K8 terms of this pixel (rasterize.py:824-837), as in k_backward_depth_face
            const float depth2 = depth * depth;
#pragma unroll
            for (int k = 0; k < 3; k++) dacc[3 * k + 2] += gd * wk[k] * depth2 / dc.zz[k];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int l = 0; l < 2; l++) dacc[3 * k + l] += -gd * dc.tmp[l] * wk[k] * depth2 * (float)S / 2.0f;
        }
#pragma unroll
        for (int pn = 0; pn < 8; pn++) {
            if (TS2) {
                acc[3 * pn + 0] += t.w[pn] * g[0];  // :780
                acc[3 * pn + 1] += t.w[pn] * g[1];
                acc[3 * pn + 2] += t.w[pn] * g[2];
            } else {
                if (t.isc[pn] * 3 >= n_tex) continue;  // outside the cube: weight 0 (compute_taps)
                double *q = acc_l + t.isc[pn] * 3;
                atomicAdd(q + 0, (double)(t.w[pn] * g[0]));
                atomicAdd(q + 1, (double)(t.w[pn] * g[1]));
                atomicAdd(q + 2, (double)(t.w[pn] * g[2]));
            }
        }
    });

    // lit: does the face own a pixel at all?  (only then it stores: FaceLight)
    bool owned = false;
    if (LIT) {
        if (L <= 64) {
            const unsigned long long bm = __ballot(own);
            owned = L == 64 ? bm != 0ull : ((bm >> (tid & 48)) & 0xffffull) != 0ull;
        } else {
            if (own) s_own = 1;
            __syncthreads();
            owned = s_own != 0;
        }
    }
    if (TS2) {
        // L == 16 here: reduce inside the 16-lane row, its last lane stores the face's 24 floats (96 B)
#pragma unroll
        for (int k = 0; k < 24; k++) acc[k] = row16_sum_last(acc[k]);
        if (LIT) {
            if (face_ok && sub == 15 && owned) {
                // corner pn holds texel bitrev3(pn) of the sampled cube (the static taps above); the reversed copy samples the
                // transposed cube, whose texel bitrev3(pn) is texel pn of the original one
                const float *lc = lit.light + (size_t)gi * 3;
                const float l3[3] = {lc[0], lc[1], lc[2]};
                float tx[24];
                if (lit.textures) {  // 96 B per cube, 16 B aligned (nr_hip.h)
                    const float4 *src = reinterpret_cast<const float4 *>(lit.textures + cube * 24);
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        const float4 v = src[k];
                        tx[4 * k] = v.x; tx[4 * k + 1] = v.y; tx[4 * k + 2] = v.z; tx[4 * k + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 24; k++) tx[k] = 0.0f;
                }
                float o[24], gl[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int r = (u & 1) * 4 + (u & 2) + (u >> 2);
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const float a = flip ? acc[3 * u + c] : acc[3 * r + c];
                        o[3 * u + c] = a * l3[c];
                        gl[c] += a * tx[3 * u + c];
                    }
                }
                float4 *dst = reinterpret_cast<float4 *>(grad_textures + cube * 24);
#pragma unroll
                for (int k = 0; k < 6; k++) dst[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
                if (lit.grad_light) {
                    float *gd = lit.grad_light + (size_t)gi * 3;
                    gd[0] = gl[0]; gd[1] = gl[1]; gd[2] = gl[2];
                }
            }
        } else if (face_ok && sub == 15) {
            float o[24];
#pragma unroll
            for (int pn = 0; pn < 8; pn++) {
                const int isc = (pn & 1) * 4 + ((pn >> 1) & 1) * 2 + ((pn >> 2) & 1);
                o[3 * isc + 0] = acc[3 * pn + 0];
                o[3 * isc + 1] = acc[3 * pn + 1];
                o[3 * isc + 2] = acc[3 * pn + 2];
            }
            float4 *dst = reinterpret_cast<float4 *>(grad_textures + (size_t)gi * 24);
#pragma unroll
            for (int k = 0; k < 6; k++) dst[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
    } else if (LIT) {
        __syncthreads();
        float gl0 = 0.0f, gl1 = 0.0f, gl2 = 0.0f;
        if (face_ok && owned) {
            const float *lc = lit.light + (size_t)gi * 3;
            const float l3[3] = {lc[0], lc[1], lc[2]};
            const float *tex = lit.textures ? lit.textures + cube * n_tex : nullptr;
            float *dst = grad_textures + cube * n_tex;
            // (the loads of the cube in a loop of their own: interleaved with the stores, which the compiler must assume to
            // alias them, every one of them would be a separate round trip)
            if (tex) {
                for (int k = sub; k < n_tex; k += L) {
                    const int c = k % 3;
                    const float v = (float)acc_l[k] * tex[k];
                    gl0 += c == 0 ? v : 0.0f;
                    gl1 += c == 1 ? v : 0.0f;
                    gl2 += c == 2 ? v : 0.0f;
                }
            }
            for (int k = sub; k < n_tex; k += L) {
                const int c = k % 3;
                dst[k] = (float)acc_l[k] * (c == 0 ? l3[0] : (c == 1 ? l3[1] : l3[2]));
            }
        }
        if (lit.grad_light) {
            if (L <= 64) {
                gl0 = group_sum(gl0, L); gl1 = group_sum(gl1, L); gl2 = group_sum(gl2, L);
            } else {
                if (gl0 != 0.0f) atomicAdd(&s_gl[0], gl0);
                if (gl1 != 0.0f) atomicAdd(&s_gl[1], gl1);
                if (gl2 != 0.0f) atomicAdd(&s_gl[2], gl2);
                __syncthreads();
                gl0 = s_gl[0]; gl1 = s_gl[1]; gl2 = s_gl[2];
            }
            if (face_ok && owned && sub == 0) {
                float *gd = lit.grad_light + (size_t)gi * 3;
                gd[0] = gl0; gd[1] = gl1; gd[2] = gl2;
            }
        }
    } else {
        __syncthreads();
        if (face_ok) {
            float *dst = grad_textures + (size_t)gi * n_tex;
            for (int k = sub; k < n_tex; k += L) dst[k] = (float)acc_l[k];
        }
    }
    if (DEPTH || k6_scratch) {  // L <= 64 when DEPTH (the host only fuses K8 when a face group fits in one wave)
        if (DEPTH && __ballot(any_box) != 0ull) {
#pragma unroll
            for (int k = 0; k < 9; k++) dacc[k] = (L == 16) ? row16_sum_last(dacc[k]) : group_sum(dacc[k], L);
        }
        if (face_ok && sub == ((L == 16) ? 15 : 0)) {
            float *gf = grad_faces + (size_t)gi * 9;
            if (k6_scratch) {
                // K6's result for this face (rasterize.py:736 stores, K8 then accumulates, :881-883): the double sums of
                // its list position rounded to float, z = 0; the K8 sums (zero without a box of this kernel's) on top
                const double *sc = k6_scratch + ((size_t)by * F + slot) * 6;
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    gf[3 * v + 0] = (float)sc[2 * v + 0] + dacc[3 * v + 0];
                    gf[3 * v + 1] = (float)sc[2 * v + 1] + dacc[3 * v + 1];
                    gf[3 * v + 2] = 0.0f + dacc[3 * v + 2];
                }
            } else if (any_box) {
#pragma unroll
                for (int k = 0; k < 9; k++) gf[k] += dacc[k];
            }
        }
    }
}

// Zeros of grad_textures beside a gather that stores the listed faces' cubes completely: every unlisted face's cube (slot_of < 0),
// 2048 elements of 16 or 4 bytes per workgroup, so that no fill has to finish before the gather may store.
struct ZeroArgs {
    float *grad_textures;
    const int *slot_of;
    int F;
    int epf;        // elements per face cube: ts^3 * 3 floats, or a quarter of that in 16-byte elements
    int vec;        // 16-byte elements (the cube is a multiple of four floats and the array 16-byte aligned)
    unsigned wgs;   // zero workgroups per image
};

__device__ __forceinline__ void zero_unlisted_body(const ZeroArgs &z, const int bx, const int by)
{
    const size_t per_image = (size_t)z.F * z.epf;
    const size_t e0 = (size_t)bx * 2048, e1 = e0 + 2048 < per_image ? e0 + 2048 : per_image;
    const int *__restrict__ slot = z.slot_of + (size_t)by * z.F;
    for (size_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const int face = (int)(e / (unsigned)z.epf);
        if (slot[face] >= 0) continue;
        const size_t at = (size_t)by * per_image + e;
        if (z.vec) reinterpret_cast<float4 *>(z.grad_textures)[at] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else z.grad_textures[at] = 0.0f;
    }
}


// --------------------------------------------------------------------------------------------------
// Faces with many candidate pixels (a ground plane, a backdrop, the strip of a needle) would keep one 16-lane group of
// the kernels above busy for thousands of iterations while the rest of the chip idles.  Those kernels therefore leave
// every face whose candidate set exceeds BIG_PX pixels untouched (zeros stored / nothing added), and this
// kernel, launched right after them, gives each such face a whole workgroup: one thread per face finds the big ones of a
// 256-face range, then all 256 lanes walk each of them in turn (coalesced rows), texel sums in LDS doubles, depth sums
// through a wave + LDS reduction.  With no big face in the range the workgroup exits after ~150 instructions.
// TEX: 0 no textures, 1 grad_textures through per-face LDS double accumulators (any texture_size <= 8), 2 texture_size 2 with
// static taps (24 register sums per lane, as in the TS2 gather); DEPTH: the K8 terms.
struct BigArgs {
    const int32_t *face_index_map;
    const float *sampling_weight_map;
    const int32_t *sampling_index_map;
    const float *face_inv_map, *faces, *zbase, *weight_map, *depth_map, *g_rgb;
    float *grad_textures;
    int n_faces_total, F, S, ts;
    double eps;
    int fix_batch_z;
    const int *vis_list, *vis_count;
    const float *g_depth;
    float *grad_faces;
    const unsigned char *visible;
    FaceLight lit;
    const double *k6_scratch;
    const int *lines_ok;  // K6's finish spares the listed faces of the images marked 0 here (NULL: none; k_big_overflow)
};

// bid = (range of 256 faces or list slots, image, share), nz shares per range: blockIdx and gridDim.z of k_backward_big
template <int TEX, bool DEPTH, bool LIT>
__device__ __forceinline__ void backward_big_body(const BigArgs &a, const uint3 bid, const unsigned nz)
{
    const int32_t *__restrict__ face_index_map = a.face_index_map;
    const float *__restrict__ sampling_weight_map = a.sampling_weight_map;
    const int32_t *__restrict__ sampling_index_map = a.sampling_index_map;
    const float *__restrict__ face_inv_map = a.face_inv_map, *__restrict__ faces = a.faces, *__restrict__ zbase = a.zbase,
                *__restrict__ weight_map = a.weight_map, *__restrict__ depth_map = a.depth_map, *__restrict__ g_rgb = a.g_rgb;
    float *__restrict__ grad_textures = a.grad_textures;
    const int n_faces_total = a.n_faces_total, F = a.F, S = a.S, ts = a.ts;
    const double eps = a.eps;
    const int fix_batch_z = a.fix_batch_z;
    const int *__restrict__ vis_list = a.vis_list, *__restrict__ vis_count = a.vis_count;
    const float *__restrict__ g_depth = a.g_depth;
    float *__restrict__ grad_faces = a.grad_faces;
    const unsigned char *__restrict__ visible = a.visible;
    const FaceLight &lit = a.lit;
    const double *__restrict__ k6_scratch = a.k6_scratch;
    extern __shared__ __attribute__((aligned(16))) double s_tex[];  // [ts^3 * 3] texel sums of the face being walked
    __shared__ int s_list[256];
    __shared__ int s_wave_n[4];
    // 9 depth sums + 24 texel sums (TEX == 2) per WAVE, added up in wave order by whoever reads them (red() below: float atomics
    // of the four waves onto one word arrived in any order, and the bits of a big face's gradients changed from run to run) +
    // 3 light-colour sums (lit; row 0)
    __shared__ float s_red[4][36];
    __shared__ int s_own;        // lit: the face being walked owns a pixel
    const int tid = threadIdx.x;
    if (vis_list && (int)bid.x * 256 >= vis_count[bid.y]) return;  // slots behind the image's list
    int n_big;
    {   // one face per thread: is its candidate set this kernel's business?  The list is built in thread order, so that the
        // (int)nz workgroups that scan the same range agree on it and can share it out (entry q -> workgroup q % (int)nz:
        // with one workgroup per range a 2048 x 2048 view, whose faces are all "big", kept 20 workgroups busy for 5 ms).
        int gi = bid.x * 256 + tid;
        bool ok = gi < n_faces_total;
        if (vis_list) {
            ok = gi < vis_count[bid.y];
            gi = ok ? (int)bid.y * F + vis_list[(size_t)bid.y * F + gi] : 0;
        }
        // K6's last step for the listed faces rides in this launch (the fused backward whose gather did not wait for the band
        // kernel: grad_faces holds the gather's K8 sums, or zeros): K6's double sums of the face's list position, rounded, go
        // on top, requested here beside the face's vertices.  A face of this kernel's own also receives its K8 sums from one
        // of the launch's workgroups (below): float atomics for it, the two additions onto the gather's zero commute.  Every
        // other face's entries are this thread's alone: a plain read-modify-write (58 k listed faces at the headline size:
        // 350 k float atomics took this launch from 4.6 to 16 us).
        // (an image whose records overflowed the line buffer receives its K6 sums in this very launch -- k_big_overflow -- and is
        // finished by the overflow pass's last workgroup)
        const bool finish = k6_scratch && ok && bid.z == 0 && !(a.lines_ok && a.lines_ok[bid.y] == 0);
        float k6v[6], had[6];
        float *gf = grad_faces + (size_t)gi * 9;
        if (finish) {
            const double *sc = k6_scratch + ((size_t)bid.y * F + bid.x * 256 + tid) * 6;
#pragma unroll
            for (int v = 0; v < 3; v++) {
                k6v[2 * v + 0] = (float)sc[2 * v + 0]; k6v[2 * v + 1] = (float)sc[2 * v + 1];
                had[2 * v + 0] = gf[3 * v + 0]; had[2 * v + 1] = gf[3 * v + 1];
            }
        }
        bool big = false;
        if (ok && !vis_list && visible && !visible[gi]) ok = false;
        if (ok) {
            const float *f = faces + (size_t)gi * 9;
            const Cand cd = face_candidates(f[0], f[1], f[3], f[4], f[6], f[7], S);
            big = cd.n > BIG_PX;
        }
        if (finish) {
#pragma unroll
            for (int v = 0; v < 3; v++) {
                if (big) {  // [k8-atomics] K6's rounded total joins K8's float sums, in any order
                    atomicAdd(gf + 3 * v + 0, k6v[2 * v + 0]);
                    atomicAdd(gf + 3 * v + 1, k6v[2 * v + 1]);
                } else {
                    gf[3 * v + 0] = k6v[2 * v + 0] + had[2 * v + 0];
                    gf[3 * v + 1] = k6v[2 * v + 1] + had[2 * v + 1];
                }
            }
        }
        const unsigned long long m = __ballot(big);
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) s_wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; w++) before += s_wave_n[w];
        if (big) s_list[before + __popcll(m & ((1ull << lane) - 1ull))] = gi;
        n_big = s_wave_n[0] + s_wave_n[1] + s_wave_n[2] + s_wave_n[3];
        __syncthreads();
    }
    const int n_tex = TEX ? ts * ts * ts * 3 : 0;
    const int n_lds = TEX == 1 ? n_tex : 0;
    for (int q = bid.z; q < n_big; q += (int)nz) {
        const int gi = s_list[q];
        const int b = gi / F, fn = gi - b * F;
        const float *fp = faces + (size_t)gi * 9;
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; k++) f[k] = fp[k];
        const Cand cd = face_candidates(f[0], f[1], f[3], f[4], f[6], f[7], S);
        DepthConst dc;
        if (DEPTH) dc = depth_constants(f, S);
        const float *fz = (fix_batch_z ? faces + (size_t)b * F * 9 : zbase) + (size_t)fn * 9;  // :389, Q1
        const float face_z[3] = {fz[2], fz[5], fz[8]};
        const bool flip = TEX && LIT && fn >= lit.tex_faces;  // the reversed copy: taps in the original cube's layout
        for (int k = tid; k < n_lds; k += 256) s_tex[k] = 0.0;
        if (tid < 4 * 36) (&s_red[0][0])[tid] = 0.0f;
        if (LIT && tid == 0) s_own = 0;
        __syncthreads();
        bool own = false;
        float dacc[9], tacc[24];
#pragma unroll
        for (int k = 0; k < 9; k++) dacc[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < 24; k++) tacc[k] = 0.0f;
        const size_t img = (size_t)b * S * S;
        for (int i = tid; i < cd.n; i += 256) {
            int x, y;
            if (!cand_pixel(cd, i, S, x, y)) continue;
            const size_t p = img + (size_t)y * S + x;
            if (face_index_map[p] != fn) continue;
            if (LIT) own = true;
            float wk[3] = {0.0f, 0.0f, 0.0f}, depth = 0.0f;
            if (weight_map) { wk[0] = weight_map[3 * p]; wk[1] = weight_map[3 * p + 1]; wk[2] = weight_map[3 * p + 2]; }
            if (depth_map) depth = depth_map[p];
            if (TEX) {
                Taps t;
                if (sampling_weight_map) {
#pragma unroll
                    for (int pn = 0; pn < 8; pn++) {
                        t.w[pn] = sampling_weight_map[8 * p + pn];
                        t.isc[pn] = sampling_index_map[8 * p + pn];
                    }
                } else {
                    compute_taps(face_z, wk, depth, ts, eps, t, flip);
                }
                const float g[3] = {g_rgb[3 * p], g_rgb[3 * p + 1], g_rgb[3 * p + 2]};
#pragma unroll
                for (int pn = 0; pn < 8; pn++) {
                    if (TEX == 2) {
                        tacc[3 * pn + 0] += t.w[pn] * g[0];  // :780
                        tacc[3 * pn + 1] += t.w[pn] * g[1];
                        tacc[3 * pn + 2] += t.w[pn] * g[2];
                    } else {
                        if (t.isc[pn] * 3 >= n_tex) continue;  // outside the cube: weight 0 (compute_taps)
                        double *a = s_tex + t.isc[pn] * 3;
                        atomicAdd(a + 0, (double)(t.w[pn] * g[0]));
                        atomicAdd(a + 1, (double)(t.w[pn] * g[1]));
                        atomicAdd(a + 2, (double)(t.w[pn] * g[2]));
                    }
                }
            }
            if (DEPTH) {  // rasterize.py:824-837, as in k_backward_depth_face
                const float gd = g_depth[p];
                const float depth2 = depth * depth;
                float tmp[3] = {dc.tmp[0], dc.tmp[1], dc.tmp[2]};
                if (face_inv_map) {  // the reference's per-pixel residual: its values, its divisions
                    tmp[0] = tmp[1] = tmp[2] = 0.0f;
#pragma unroll
                    for (int k = 0; k < 3; k++)
#pragma unroll
                        for (int l = 0; l < 3; l++) tmp[k] += -face_inv_map[9 * p + 3 * l + k] / f[3 * l + 2];
                }
#pragma unroll
                for (int k = 0; k < 3; k++) dacc[3 * k + 2] += gd * wk[k] * depth2 / dc.zz[k];
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int l = 0; l < 2; l++) dacc[3 * k + l] += -gd * tmp[l] * wk[k] * depth2 * (float)S / 2.0f;
            }
        }
        if (DEPTH) {
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const float v = group_sum(dacc[k], 64);
                if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
            }
        }
        if (TEX == 2) {
#pragma unroll
            for (int k = 0; k < 24; k++) {
                const float v = group_sum(tacc[k], 64);
                if ((tid & 63) == 0) s_red[tid >> 6][9 + k] = v;
            }
        }
        if (TEX && LIT && own) s_own = 1;
        __syncthreads();
        auto red = [&](int k) { return ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k]; };
        if (TEX && LIT) {  // the original cube, times the face's light colour; only a face that owns a pixel stores
            if (s_own) {
                const size_t cube = (size_t)b * lit.tex_faces + (flip ? fn - lit.tex_faces : fn);
                const float *lc = lit.light + (size_t)gi * 3;
                const float *tex = lit.textures ? lit.textures + cube * n_tex : nullptr;
                float *dst = grad_textures + cube * n_tex;
                for (int k = tid; k < n_tex; k += 256) {
                    const int q = k / 3, c = k - 3 * q;
                    int u = k;
                    float a;
                    if (TEX == 2) {  // k = 3 * corner + c, the corner's texel as in the TS2 gather
                        u = 3 * (flip ? q : (q & 1) * 4 + (q & 2) + (q >> 2)) + c;
                        a = red(9 + k);
                    } else {
                        a = (float)s_tex[k];
                    }
                    dst[u] = a * lc[c];
                    if (tex && a != 0.0f) atomicAdd(&s_red[0][33 + c], a * tex[u]);
                }
                if (lit.grad_light) {
                    __syncthreads();
                    if (tid < 3) lit.grad_light[(size_t)gi * 3 + tid] = s_red[0][33 + tid];
                }
            }
        } else {
        if (TEX == 1) {
            float *dst = grad_textures + (size_t)gi * n_tex;
            for (int k = tid; k < n_tex; k += 256) dst[k] = (float)s_tex[k];
        }
        if (TEX == 2 && tid < 24) {  // corner pn = tid / 3 -> texel (pn & 1) * 4 + ((pn >> 1) & 1) * 2 + ((pn >> 2) & 1)
            const int pn = tid / 3, c = tid - 3 * pn;
            const int isc = (pn & 1) * 4 + ((pn >> 1) & 1) * 2 + ((pn >> 2) & 1);
            grad_textures[(size_t)gi * 24 + 3 * isc + c] = red(9 + tid);
        }
        }
        if (DEPTH && tid < 9) {
            if (k6_scratch) atomicAdd(grad_faces + (size_t)gi * 9 + tid, red(tid));  // (see the top of the kernel)
            else grad_faces[(size_t)gi * 9 + tid] += red(tid);
        }
        __syncthreads();
    }
}


// k_backward_big's arguments for a call and its plan (K8 riding along and K6's finish as the plan says)
inline BigArgs big_args(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l)
{
    const double *finish_k6 = p.finish == FINISH_BIG ? l.scratch : nullptr;
    BigArgs a = {};
    a.face_index_map = c.face_index_map, a.sampling_weight_map = c.sampling_weight_map, a.sampling_index_map = c.sampling_index_map;
    a.faces = c.faces, a.zbase = c.faces_z_ref ? c.faces_z_ref : c.faces, a.weight_map = c.weight_map, a.depth_map = c.depth_map;
    a.g_rgb = c.grad_rgb_map, a.grad_textures = c.grad_textures;
    a.n_faces_total = c.B * c.F, a.F = c.F, a.S = c.S, a.ts = c.ts, a.eps = c.eps;
    a.fix_batch_z = (c.flags & NR_FLAG_FIX_TEXTURE_BATCH_Z) ? 1 : 0;
    a.vis_list = p.listed ? l.vis_list : nullptr, a.vis_count = l.vis_count;
    a.g_depth = p.depth_in_gather ? c.grad_depth_map : nullptr;
    a.grad_faces = (p.depth_in_gather || finish_k6) ? c.grad_faces : nullptr;
    a.lit = c.lit, a.k6_scratch = finish_k6;
    return a;
}

// k_backward_big's grid: one workgroup per range of 256 faces (or list slots), times as many workgroups per range (z) as it
// takes to put ~4096 workgroups on the chip -- they share out the range's big faces.  (Small launches: a workgroup per 64
// faces of the call, at least 1024 -- with nothing to do, as on a fine mesh, the kernel costs what dispatching it costs.)
inline dim3 big_grid(bool listed, int B, int F)
{
    const size_t n = (size_t)B * F;
    const dim3 g = listed ? dim3((unsigned)((F + 255) / 256), (unsigned)B) : dim3((unsigned)((n + 255) / 256));
    const size_t ranges = (size_t)g.x * g.y;
    const size_t target = n / 64 < 1024 ? 1024 : (n / 64 > 4096 ? 4096 : n / 64);
    const size_t z = target / ranges;
    return dim3(g.x, g.y, (unsigned)(z < 1 ? 1 : (z > 64 ? 64 : z)));
}

}  // namespace
}  // namespace nr
