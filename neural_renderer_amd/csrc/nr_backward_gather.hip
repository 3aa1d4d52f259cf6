// nr_backward_gather.hip -- K7 backward_textures (rasterize.py:750-792) and K8 backward_depth_map
// (rasterize.py:794-847) + their C-ABI entry points.
//
// The reference scatters from pixels: 24 (K7) / 9 (K8) float atomicAdds per covered pixel, all pixels of a
// face hitting the same few addresses.  On MI355X that formulation is bound by same-address atomic
// serialisation in L2 (measured: 0.9 ms / 0.33 ms at the headline size, profiles/r01a).  Both gradients are
// sums over "the pixels a face owns", so here they are GATHERED per face instead:
//   * a group of lanes (16, 64 or 256 depending on the texture size) owns one face, walks the pixels of the
//     face's screen box (the same box the forward used), keeps the pixels whose face_index equals the face,
//     evaluates the reference's per-pixel terms and accumulates them privately;
//   * K7: texture_size 2 (the Renderer default) has a static tap pattern -> 24 register accumulators per
//     lane, group reduction, one 96-byte store per face; larger cubes accumulate in LDS (double);
//     every element of grad_textures is STORED (zeros for faces that own nothing): no zero fill, no atomics;
//   * K8: 9 register accumulators, group reduction, one read-modify-write of the face's 9 floats by a single
//     lane (K6 stored them before, rasterize.py:881-883): no atomics.
// Per-pixel terms use the reference's arithmetic; the order of the additions differs (as it does between
// any two runs of the reference, whose atomics are unordered).
// Fused backward (nr_backward_rasterize): one gather serves K7 and K8, visits only the faces of K6's visible lists and either
// finishes K6 in its epilogue (large calls) or shares ONE launch with K6's line setup and the zeros of grad_textures, in front of
// K6's band kernel (calls of up to 96 k faces: k_setup_gather below).
#include "nr_device.h"
#include "nr_band_lines.h"
#include "nr_face_gather.h"
#include "nr_k6_tune.h"
#include <type_traits>

using namespace nr;

namespace {

// the face gather (face_gather_body and its walk: nr_face_gather.h) as a launch of its own
template <bool TS2, bool DEPTH, bool LIT>
__global__ __launch_bounds__(256) void k_backward_textures_face(FaceGatherArgs a)
{
    face_gather_body<TS2, DEPTH, LIT>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// --------------------------------------------------------------------------------------------------
// The fused backward's launch between K6's compaction and its band kernel: the line setup (nr_band_lines.h), the K7 / K8
// gather and the zeros of grad_textures in ONE grid.  All three need the visible-face lists and nothing else of each other;
// the first two are latency-bound launches that each leave most of the chip idle (at the headline size 25.8 us on ~1000
// working workgroups and 44.6 us on ~1900), the third is what would otherwise be a fill in front of the gather.  Side by
// side they take what the longest takes.  (On two streams with event fork / join the same overlap cost 8 + 6 us of barrier
// packets on the critical stream and a finishing launch: 3 us gained of 250; LAB-NOTEBOOK, round 4.)
//   grid.x = [line setup | gather | zeros], grid.y = image.  The line-setup workgroups come first: the band kernel behind
//   this launch waits for their records, the chip's dispatcher hands out workgroups in grid order.
//   Zeros: every unlisted face's cube (slot_of < 0: the gather stores the listed ones completely), 2048 elements of 16 or 4
//   bytes per workgroup, so that no fill has to finish before the gather may store (zero_unlisted_body, nr_face_gather.h).
//   The launch is 1-D with the image fastest (image_fastest, nr_device.h): the working workgroups of all images' line setups,
//   then those of their gathers, in front of the ones that read a list's length and leave (NR_FLAG_SERIAL_BACKWARD never takes
//   this launch).
template <bool TS2, bool DEPTH, bool LIT>
__global__ __launch_bounds__(256) void k_setup_gather(LineSetupArgs ls, FaceGatherArgs g, ZeroArgs z, unsigned gather_x)
{
#if NR_SETUP_GATHER_IMAGE_FASTEST
    const SlotImage w = image_fastest(blockIdx.x, ls.grid_y);
    const unsigned bx = (unsigned)w.bx;
    const int by = w.by;
#else
    const unsigned bx = blockIdx.x;
    const int by = (int)blockIdx.y;
#endif
    if (bx < ls.grid_x) line_setup_body(ls, (int)bx, by);
    else if (bx < ls.grid_x + gather_x) face_gather_body<TS2, DEPTH, LIT>(g, (int)(bx - ls.grid_x), by);
    else zero_unlisted_body(z, (int)(bx - ls.grid_x - gather_x), by);
}

// the faces the face gather leaves out (more than BIG_PX candidates), a workgroup each: backward_big_body, nr_face_gather.h
template <int TEX, bool DEPTH, bool LIT>
__global__ __launch_bounds__(256) void k_backward_big(BigArgs a)
{
    backward_big_body<TEX, DEPTH, LIT>(a, make_uint3(blockIdx.x, blockIdx.y, blockIdx.z), gridDim.z);
}

// --------------------------------------------------------------------------------------------------
// B2 (fallback, texture_size > 13): per-pixel scatter with hardware f32 atomics (-munsafe-fp-atomics =>
// global_atomic_add_f32), the reference's own formulation (rasterize.py:750-792).  The caller's
// zero fill is replaced by a hipMemsetAsync in the entry point.
__global__ __launch_bounds__(256) void k_backward_textures_atomic(
    const int32_t *__restrict__ face_index_map, const float *__restrict__ sampling_weight_map,
    const int32_t *__restrict__ sampling_index_map, const float *__restrict__ faces,
    const float *__restrict__ zbase, const float *__restrict__ weight_map, const float *__restrict__ depth_map,
    const float *__restrict__ g_rgb, float *__restrict__ grad_textures, int F, int S, int ts, double eps,
    int fix_batch_z, size_t n_pixels)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const int fi = face_index_map[i];
    if (fi < 0) return;
    const int b = (int)(i / ((size_t)S * S));
    Taps t;
    if (sampling_weight_map) {
#pragma unroll
        for (int pn = 0; pn < 8; pn++) {
            t.w[pn] = sampling_weight_map[8 * i + pn];
            t.isc[pn] = sampling_index_map[8 * i + pn];
        }
    } else {
        const float *face = (fix_batch_z ? faces + (size_t)b * F * 9 : zbase) + (size_t)fi * 9;
        const float w[3] = {weight_map[3 * i], weight_map[3 * i + 1], weight_map[3 * i + 2]};
        const float fz[3] = {face[2], face[5], face[8]};
        compute_taps(fz, w, depth_map[i], ts, eps, t);
    }
    const float g[3] = {g_rgb[3 * i], g_rgb[3 * i + 1], g_rgb[3 * i + 2]};
    float *gt = grad_textures + ((size_t)b * F + fi) * ts * ts * ts * 3;
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        if (t.isc[pn] >= ts * ts * ts) continue;  // outside the cube: weight 0 (compute_taps)
        float *p = gt + t.isc[pn] * 3;
        atomicAdd(p + 0, t.w[pn] * g[0]);  // :780
        atomicAdd(p + 1, t.w[pn] * g[1]);
        atomicAdd(p + 2, t.w[pn] * g[2]);
    }
}


// the same with per-face light colours (FaceLight): the taps are flattened in the original cube's layout, the contribution
// carries the face's colour, and the colour's own gradient -- g_c times the pixel's unlit sample -- goes to grad_light
__global__ __launch_bounds__(256) void k_backward_textures_atomic_lit(
    const int32_t *__restrict__ face_index_map, const float *__restrict__ faces, const float *__restrict__ zbase,
    const float *__restrict__ weight_map, const float *__restrict__ depth_map, const float *__restrict__ g_rgb,
    float *__restrict__ grad_textures, int F, int S, int ts, double eps, int fix_batch_z, size_t n_pixels, FaceLight lit)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const int fi = face_index_map[i];
    if (fi < 0) return;
    const int b = (int)(i / ((size_t)S * S));
    const bool flip = fi >= lit.tex_faces;
    const size_t cube = ((size_t)b * lit.tex_faces + (flip ? fi - lit.tex_faces : fi)) * ts * ts * ts * 3;
    Taps t;
    const float *face = (fix_batch_z ? faces + (size_t)b * F * 9 : zbase) + (size_t)fi * 9;
    const float w[3] = {weight_map[3 * i], weight_map[3 * i + 1], weight_map[3 * i + 2]};
    const float fz[3] = {face[2], face[5], face[8]};
    compute_taps(fz, w, depth_map[i], ts, eps, t, flip);
    const float g[3] = {g_rgb[3 * i], g_rgb[3 * i + 1], g_rgb[3 * i + 2]};
    const float *lc = lit.light + ((size_t)b * F + fi) * 3;
    const float l3[3] = {lc[0], lc[1], lc[2]};
    float *gt = grad_textures + cube;
    const float *tex = lit.textures ? lit.textures + cube : nullptr;
    float sample[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        if (t.isc[pn] >= ts * ts * ts) continue;  // outside the cube: weight 0 (compute_taps)
        float *p = gt + t.isc[pn] * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            atomicAdd(p + c, (t.w[pn] * g[c]) * l3[c]);
            if (tex) sample[c] += t.w[pn] * tex[t.isc[pn] * 3 + c];
        }
    }
    if (lit.grad_light) {
        float *gl = lit.grad_light + ((size_t)b * F + fi) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) atomicAdd(gl + c, g[c] * sample[c]);
    }
}

// --------------------------------------------------------------------------------------------------
// B3: one face per group of 16 lanes; 9 register accumulators; a single lane adds the totals onto what K6
// stored.  The per-face inverse matrix is recomputed from the vertices with the forward's arithmetic
// (compute_face_inv) unless the caller supplies the reference's per-pixel face_inv_map residual.
__global__ __launch_bounds__(256) void k_backward_depth_face(
    const float *__restrict__ faces, const float *__restrict__ depth_map, const int32_t *__restrict__ face_index_map,
    const float *__restrict__ face_inv_map, const float *__restrict__ weight_map, const float *__restrict__ g_depth,
    float *__restrict__ grad_faces, int n_faces_total, int F, int S, const int *__restrict__ vis_list,
    const int *__restrict__ vis_count, const unsigned char *__restrict__ visible)
{
    constexpr int L = 16;
    const int tid = threadIdx.x;
    const int grp = tid / L, sub = tid - grp * L;
    if (vis_list && (int)blockIdx.x * (256 / L) >= vis_count[blockIdx.y]) return;  // slots behind the image's list
    int gi = blockIdx.x * (256 / L) + grp;
    bool face_ok = gi < n_faces_total;
    if (vis_list) {
        const int slot = gi;
        face_ok = slot < vis_count[blockIdx.y];
        gi = face_ok ? (int)blockIdx.y * F + vis_list[(size_t)blockIdx.y * F + slot] : 0;
    } else if (visible && face_ok && !visible[gi]) {
        face_ok = false;  // the forward's flags (depth-only rendering has no K6 lists): 5/6 of a mesh's faces own no pixel
    }
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = 0.0f;
    bool any_box = false;
    __shared__ int s_queue[512];
    Cand cd;
    cd.n = 0;
    int fn = 0;
    size_t img = 0;
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = 1.0f;
    DepthConst dc;
#pragma unroll
    for (int k = 0; k < 3; k++) dc.tmp[k] = dc.zz[k] = 0.0f;
    if (face_ok) {
        const int b = gi / F;
        fn = gi - b * F;
        const float *fp = faces + (size_t)gi * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) f[k] = fp[k];
        cd = face_candidates(f[0], f[1], f[3], f[4], f[6], f[7], S);
        if (cd.n > 0 && cd.n <= BIG_PX) {  // the rest is k_backward_big's
            any_box = true;
            dc = depth_constants(f, S);
            img = (size_t)b * S * S;
        }
    }
    walk_owned_pixels<2>(cd, any_box ? cd.n : 0, fn, face_index_map + img, S, sub, L, s_queue, [&](int off) {
        const size_t p = img + (size_t)off;
        const float depth = depth_map[p];
        const float w[3] = {weight_map[3 * p], weight_map[3 * p + 1], weight_map[3 * p + 2]};
        const float gd = g_depth[p];
        const float depth2 = depth * depth;
        // [k8-terms] :824-827
#pragma unroll
        for (int k = 0; k < 3; k++) acc[3 * k + 2] += gd * w[k] * depth2 / dc.zz[k];
        // :830-837
        float tmp[3] = {dc.tmp[0], dc.tmp[1], dc.tmp[2]};
        if (face_inv_map) {  // the reference's per-pixel residual: its values, its divisions
            tmp[0] = tmp[1] = tmp[2] = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int l = 0; l < 3; l++) tmp[k] += -face_inv_map[9 * p + 3 * l + k] / f[3 * l + 2];
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int l = 0; l < 2; l++) acc[3 * k + l] += -gd * tmp[l] * w[k] * depth2 * (float)S / 2.0f;
    });
    if (__ballot(any_box) == 0ull) return;  // whole wave has nothing to add
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = row16_sum_last(acc[k]);
    if (face_ok && any_box && sub == 15) {
        float *gf = grad_faces + (size_t)gi * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) gf[k] += acc[k];
    }
}

// --------------------------------------------------------------------------------------------------
// Shared cubes (nr_backward_textures_shared, DESIGN K7 "Shared cubes"): ONE set of cubes [Nf, ts^3, 3] sampled by all B images,
// its gradient the sum over the images.  The batched gathers above store a cube per (image, face); here the pairs of all
// images meet in one cube, so a pair's group sums its pixels privately as before -- the same walk, the same taps, float
// registers with static taps, LDS doubles otherwise -- and then adds every texel's sum ONCE, in double, onto sums [Nf][ts^3 * 3]
// (zero-filled in front; k_round_sums stores the floats, all of them).  Atomics per (pair, texel that received something),
// never per pixel; nothing of size B * Nf * ts^3 exists.
//   grid = (ranges of 256 faces, image).  A workgroup reads the forward's `visible` flags of its range, one face per thread,
//   and compacts the pairs that own a pixel into two LDS lists: `small` (candidate sets up to BIG_PX; a group of L = 16 | 64
//   lanes each, 256 / L at a time, until the list is done) and `wide` (above BIG_PX -- a ground plane --, and every pair at
//   texture_size 9 .. 13, where one cube of doubles is all the LDS holds: the whole workgroup walks each in turn, as
//   k_backward_big does).  So the ~5/6 of a mesh's pairs that own nothing cost one byte load, and a workgroup's groups stay
//   busy while its list lasts.  LIT: the contribution carries light[b, f], a reversed copy Nf + f lands in cube f (its taps
//   are flattened in the original layout: compute_taps' flip), and grad_light[b, f] -- the pair's own -- is stored by whoever
//   handles the pair, zeros by the scan for pairs that own nothing.
struct SharedGatherArgs {
    const int32_t *face_index_map;
    const float *faces, *zbase, *weight_map, *depth_map, *g_rgb;
    const unsigned char *visible;  // [B, F] or NULL (every pair is scanned)
    double *sums;                  // [Nf][ts^3 * 3]
    int F, S, ts;
    double eps;
    int fix_batch_z, L, wide_all, n_lds;  // n_lds: doubles of dynamic LDS
    FaceLight lit;
};

template <bool TS2, bool LIT>
__global__ __launch_bounds__(256) void k_shared_gather(SharedGatherArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_acc[];  // [256 / L][ts^3 * 3]; a wide pair: the first cube
    __shared__ int s_queue[512];                                    // walk_owned_pixels
    __shared__ int s_small[256], s_wide[256];
    __shared__ int s_wave_n[4][2];
    __shared__ int s_own;
    __shared__ float s_gl[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, F = a.F, S = a.S, ts = a.ts, L = a.L;
    const int n_tex = ts * ts * ts * 3;
    const FaceLight &lit = a.lit;
    const int Nf = LIT ? lit.tex_faces : F;
    const size_t img = (size_t)b * S * S;
    const float *__restrict__ faces_b = a.faces + (size_t)b * F * 9;
    const float *__restrict__ zfaces = a.fix_batch_z ? faces_b : a.zbase;  // :389, Q1
    float *__restrict__ grad_light = LIT ? lit.grad_light : nullptr;

    int n_small, n_wide;
    {   // the range's pairs, one per thread; both lists in thread order
        const int f = (int)blockIdx.x * 256 + tid;
        const bool vis = f < F && (!a.visible || a.visible[(size_t)b * F + f] != 0);
        bool small = false, wide = false;
        if (vis) {
            const float *fp = faces_b + (size_t)f * 9;
            const Cand cd = face_candidates(fp[0], fp[1], fp[3], fp[4], fp[6], fp[7], S);
            wide = cd.n > BIG_PX || (a.wide_all && cd.n > 0);
            small = cd.n > 0 && !wide;
        }
        if (grad_light && f < F && !small && !wide) {
            float *gl = grad_light + ((size_t)b * F + f) * 3;
            gl[0] = 0.0f; gl[1] = 0.0f; gl[2] = 0.0f;
        }
        const unsigned long long ms = __ballot(small), mw = __ballot(wide);
        if (lane == 0) { s_wave_n[wave][0] = __popcll(ms); s_wave_n[wave][1] = __popcll(mw); }
        for (int k = tid; k < a.n_lds; k += 256) s_acc[k] = 0.0;
        __syncthreads();
        int bs = 0, bw = 0;
        for (int w = 0; w < wave; w++) { bs += s_wave_n[w][0]; bw += s_wave_n[w][1]; }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (small) s_small[bs + __popcll(ms & below)] = f;
        if (wide) s_wide[bw + __popcll(mw & below)] = f;
        n_small = s_wave_n[0][0] + s_wave_n[1][0] + s_wave_n[2][0] + s_wave_n[3][0];
        n_wide = s_wave_n[0][1] + s_wave_n[1][1] + s_wave_n[2][1] + s_wave_n[3][1];
        __syncthreads();
    }

    // the small pairs: 256 / L at a time, a group of L lanes each (every lane of the workgroup takes every round: the walk
    // keeps the lanes of a wave in step, the barriers below the workgroup)
    const int per = 256 / L, grp = tid / L, sub = tid - grp * L;
    double *acc_l = s_acc + (TS2 ? 0 : (size_t)grp * n_tex);
    for (int q0 = 0; q0 < n_small; q0 += per) {
        const bool face_ok = q0 + grp < n_small;
        const int fn = face_ok ? s_small[q0 + grp] : 0;
        Cand cd;
        cd.n = 0;
        float face_z[3] = {1.0f, 1.0f, 1.0f};
        const bool flip = LIT && fn >= Nf;
        const int cube = flip ? fn - Nf : fn;
        if (face_ok) {
            const float *fp = faces_b + (size_t)fn * 9;
            cd = face_candidates(fp[0], fp[1], fp[3], fp[4], fp[6], fp[7], S);
            const float *fz = zfaces + (size_t)fn * 9;
            face_z[0] = fz[2]; face_z[1] = fz[5]; face_z[2] = fz[8];
        }
        float acc[24];
#pragma unroll
        for (int k = 0; k < 24; k++) acc[k] = 0.0f;
        bool own = false;
        walk_owned_pixels<2>(cd, face_ok ? cd.n : 0, fn, a.face_index_map + img, S, sub, L, s_queue, [&](int off) {
            const size_t p = img + (size_t)off;
            const float wk[3] = {a.weight_map[3 * p], a.weight_map[3 * p + 1], a.weight_map[3 * p + 2]};
            const float depth = a.depth_map[p];
            const float g[3] = {a.g_rgb[3 * p], a.g_rgb[3 * p + 1], a.g_rgb[3 * p + 2]};
            own = true;
            Taps t;
            compute_taps(face_z, wk, depth, ts, a.eps, t, flip);
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
        const unsigned long long bm = __ballot(own);
        const bool owned = L == 64 ? bm != 0ull : ((bm >> (tid & 48)) & 0xffffull) != 0ull;
        float l3[3] = {1.0f, 1.0f, 1.0f};
        if (LIT && face_ok) {
            const float *lc = lit.light + ((size_t)b * F + fn) * 3;
            l3[0] = lc[0]; l3[1] = lc[1]; l3[2] = lc[2];
        }
        if (TS2) {  // L == 16: the row's last lane holds the pair's 24 sums (corner pn = texel bitrev3(pn) of the sampled cube)
#pragma unroll
            for (int k = 0; k < 24; k++) acc[k] = row16_sum_last(acc[k]);
            if (face_ok && sub == 15) {
                float gl[3] = {0.0f, 0.0f, 0.0f};
                if (owned) {
                    float tx[24];
#pragma unroll
                    for (int k = 0; k < 24; k++) tx[k] = 0.0f;
                    if (LIT && lit.textures) {  // 96 B per cube, 16 B aligned (nr_hip.h)
                        const float4 *src = reinterpret_cast<const float4 *>(lit.textures + (size_t)cube * 24);
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            const float4 v = src[k];
                            tx[4 * k] = v.x; tx[4 * k + 1] = v.y; tx[4 * k + 2] = v.z; tx[4 * k + 3] = v.w;
                        }
                    }
                    double *dst = a.sums + (size_t)cube * 24;
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int r = (u & 1) * 4 + (u & 2) + (u >> 2);
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const float av = flip ? acc[3 * u + c] : acc[3 * r + c];
                            const float o = LIT ? av * l3[c] : av;
                            if (LIT) gl[c] += av * tx[3 * u + c];
                            if (o != 0.0f) atomicAdd(dst + 3 * u + c, (double)o);
                        }
                    }
                }
                if (grad_light) {
                    float *gd = grad_light + ((size_t)b * F + fn) * 3;
                    gd[0] = gl[0]; gd[1] = gl[1]; gd[2] = gl[2];
                }
            }
        } else {
            __syncthreads();
            float gl0 = 0.0f, gl1 = 0.0f, gl2 = 0.0f;
            if (face_ok && owned) {
                const float *tex = (LIT && lit.textures) ? lit.textures + (size_t)cube * n_tex : nullptr;
                double *dst = a.sums + (size_t)cube * n_tex;
                for (int k = sub; k < n_tex; k += L) {
                    const float av = (float)acc_l[k];
                    acc_l[k] = 0.0;  // (the next round's zeros)
                    if (av == 0.0f) continue;
                    const int c = k % 3;
                    if (tex) {
                        const float v = av * tex[k];
                        gl0 += c == 0 ? v : 0.0f;
                        gl1 += c == 1 ? v : 0.0f;
                        gl2 += c == 2 ? v : 0.0f;
                    }
                    atomicAdd(dst + k, (double)(LIT ? av * (c == 0 ? l3[0] : (c == 1 ? l3[1] : l3[2])) : av));
                }
            }
            if (grad_light) {
                gl0 = group_sum(gl0, L); gl1 = group_sum(gl1, L); gl2 = group_sum(gl2, L);
                if (face_ok && sub == 0) {
                    float *gd = grad_light + ((size_t)b * F + fn) * 3;
                    gd[0] = gl0; gd[1] = gl1; gd[2] = gl2;
                }
            }
            __syncthreads();
        }
    }

    // the wide pairs: the whole workgroup walks each in turn (coalesced rows), texel sums in the first cube of LDS doubles
    for (int q = 0; q < n_wide; q++) {
        const int fn = s_wide[q];
        const float *fp = faces_b + (size_t)fn * 9;
        const Cand cd = face_candidates(fp[0], fp[1], fp[3], fp[4], fp[6], fp[7], S);
        const float *fz = zfaces + (size_t)fn * 9;
        const float face_z[3] = {fz[2], fz[5], fz[8]};
        const bool flip = LIT && fn >= Nf;
        const int cube = flip ? fn - Nf : fn;
        if (tid < 3) s_gl[tid] = 0.0f;
        if (tid == 0) s_own = 0;
        __syncthreads();
        bool own = false;
        for (int i = tid; i < cd.n; i += 256) {
            int x, y;
            if (!cand_pixel(cd, i, S, x, y)) continue;
            const size_t p = img + (size_t)y * S + x;
            if (a.face_index_map[p] != fn) continue;
            own = true;
            const float wk[3] = {a.weight_map[3 * p], a.weight_map[3 * p + 1], a.weight_map[3 * p + 2]};
            const float g[3] = {a.g_rgb[3 * p], a.g_rgb[3 * p + 1], a.g_rgb[3 * p + 2]};
            Taps t;
            compute_taps(face_z, wk, a.depth_map[p], ts, a.eps, t, flip);
#pragma unroll
            for (int pn = 0; pn < 8; pn++) {
                if (t.isc[pn] * 3 >= n_tex) continue;  // outside the cube: weight 0 (compute_taps)
                double *d = s_acc + t.isc[pn] * 3;
                atomicAdd(d + 0, (double)(t.w[pn] * g[0]));
                atomicAdd(d + 1, (double)(t.w[pn] * g[1]));
                atomicAdd(d + 2, (double)(t.w[pn] * g[2]));
            }
        }
        if (own) s_own = 1;
        __syncthreads();
        if (s_own) {
            const float *lc = LIT ? lit.light + ((size_t)b * F + fn) * 3 : nullptr;
            const float *tex = (LIT && lit.textures) ? lit.textures + (size_t)cube * n_tex : nullptr;
            double *dst = a.sums + (size_t)cube * n_tex;
            for (int k = tid; k < n_tex; k += 256) {
                const float av = (float)s_acc[k];
                s_acc[k] = 0.0;  // (the next pair's zeros)
                if (av == 0.0f) continue;
                const int c = k % 3;
                if (tex) atomicAdd(&s_gl[c], av * tex[k]);
                atomicAdd(dst + k, (double)(LIT ? av * lc[c] : av));
            }
        }
        __syncthreads();
        if (grad_light && tid < 3) grad_light[((size_t)b * F + fn) * 3 + tid] = s_gl[tid];
        __syncthreads();
    }
}

// the shared gather's double sums, rounded once: every element of grad_textures
__global__ __launch_bounds__(256) void k_round_sums(const double *__restrict__ sums, float *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)sums[i];
}

}  // namespace

// ====================================================================================================
// The gathers' steps: run_backward (nr_backward.hip) launches them in the order its plan says

// K7's face gather (K8 riding along when the plan says so, K6's finish in its epilogue when the plan says so) -- or, with ls,
// the line setup, that gather and the zeros of the unlisted faces' cubes in one launch (k_setup_gather)
int nr::gather_faces(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l, const LineSetupArgs *ls)
{
    const int B = c.B, F = c.F, n = B * F, ts = c.ts;
    const size_t n_tex = (size_t)ts * ts * ts * 3;
    const int per = 256 / p.lanes;
    const int *vis_list = p.listed ? l.vis_list : nullptr;
    const dim3 grid = vis_list ? dim3((unsigned)((F + per - 1) / per), (unsigned)B) : dim3((unsigned)((n + per - 1) / per));
    const FaceGatherArgs ga = face_gather_args(c, p, l);
    // (the kernels take the per-face light mode as a template parameter: see k_backward_textures_face)
    auto go = [&](auto ts2, auto dep, auto lit) {
        constexpr bool T = decltype(ts2)::value, D = decltype(dep)::value, LIT = decltype(lit)::value;
        if (ls) {
            ZeroArgs z = {c.grad_textures, l.slot_of, F, (int)n_tex, 0, 0u};
            if (p.tex_zeros == TEX_ZEROS_SETUP) {
                z.vec = n_tex % 4 == 0;
                z.epf = z.vec ? (int)(n_tex / 4) : (int)n_tex;
                z.wgs = (unsigned)(((size_t)F * z.epf + 2047) / 2048);
            }
            const size_t both = p.gather_lds > ls->lds_bytes ? p.gather_lds : ls->lds_bytes;
            const unsigned per_image = ls->grid_x + grid.x + z.wgs;
            hipLaunchKernelGGL((k_setup_gather<T, D, LIT>), NR_SETUP_GATHER_IMAGE_FASTEST ? dim3(per_image * (unsigned)B) : dim3(per_image, (unsigned)B),
                               dim3(256), both, c.st, *ls, ga, z, grid.x);
        } else {
            hipLaunchKernelGGL((k_backward_textures_face<T, D, LIT>), grid, dim3(256), p.gather_lds, c.st, ga);
        }
    };
    auto with_lit = [&](auto ts2, auto dep) {
        if (c.lit.light) go(ts2, dep, std::true_type()); else go(ts2, dep, std::false_type());
    };
    using T = std::true_type;
    using N = std::false_type;
    if (p.static_taps) { if (p.depth_in_gather) with_lit(T(), T()); else with_lit(T(), N()); }
    else { if (p.depth_in_gather) with_lit(N(), T()); else with_lit(N(), N()); }
    return launch_status();
}

// the faces the face gather left out (more than BIG_PX candidates): a workgroup each.  FINISH_BIG: K6's sums of the listed
// faces go on top of what the gather left in grad_faces, in this launch
void nr::gather_big(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l)
{
    const BigArgs a = big_args(c, p, l);
    const dim3 grid = big_grid(a.vis_list != nullptr, c.B, c.F);
    const size_t lds = p.static_taps ? 0 : (size_t)c.ts * c.ts * c.ts * 3 * sizeof(double);
    auto go = [&](auto lit) {
        constexpr bool LIT = decltype(lit)::value;
#define NR_BIG(T, D) hipLaunchKernelGGL((k_backward_big<T, D, LIT>), grid, dim3(256), lds, c.st, a)
        if (p.static_taps) { if (a.g_depth) NR_BIG(2, true); else NR_BIG(2, false); }
        else { if (a.g_depth) NR_BIG(1, true); else NR_BIG(1, false); }
#undef NR_BIG
    };
    if (c.lit.light) go(std::true_type()); else go(std::false_type());
}

// texture_size > 13: the reference's per-pixel scatter with hardware atomics, onto the zeros filled in front
void nr::gather_atomic(const BackwardCall &c)
{
    const size_t np = (size_t)c.B * c.S * c.S;
    const float *zbase = c.faces_z_ref ? c.faces_z_ref : c.faces;
    const int fix = (c.flags & NR_FLAG_FIX_TEXTURE_BATCH_Z) ? 1 : 0;
    if (c.lit.light)
        hipLaunchKernelGGL(k_backward_textures_atomic_lit, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c.st,
                           c.face_index_map, c.faces, zbase, c.weight_map, c.depth_map, c.grad_rgb_map, c.grad_textures, c.F,
                           c.S, c.ts, c.eps, fix, np, c.lit);
    else
        hipLaunchKernelGGL(k_backward_textures_atomic, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c.st, c.face_index_map,
                           c.sampling_weight_map, c.sampling_index_map, c.faces, zbase, c.weight_map, c.depth_map,
                           c.grad_rgb_map, c.grad_textures, c.F, c.S, c.ts, c.eps, fix, np);
}

// K8 on its own: added onto grad_faces; the faces of K6's lists (or of the depth-only call's), else those the forward's
// flags mark (the staged entry point has neither)
void nr::gather_depth(const BackwardCall &c, const K6Lists &l)
{
    const int B = c.B, F = c.F, n = B * F;
    const dim3 grid = l.vis_list ? dim3((unsigned)((F + 15) / 16), (unsigned)B) : dim3((unsigned)((n + 15) / 16));
    hipLaunchKernelGGL(k_backward_depth_face, grid, dim3(256), 0, c.st, c.faces, c.depth_map, c.face_index_map, c.face_inv_map,
                       c.weight_map, c.grad_depth_map, c.grad_faces, n, F, c.S, l.vis_list, l.vis_count, c.visible_faces);
    const dim3 grid_big = big_grid(l.vis_list != nullptr, B, F);
    BigArgs a = {};
    a.face_index_map = c.face_index_map, a.face_inv_map = c.face_inv_map, a.faces = c.faces, a.zbase = c.faces;
    a.weight_map = c.weight_map, a.depth_map = c.depth_map, a.n_faces_total = n, a.F = F, a.S = c.S, a.ts = 2;
    a.vis_list = l.vis_list, a.vis_count = l.vis_count, a.g_depth = c.grad_depth_map, a.grad_faces = c.grad_faces;
    a.visible = c.visible_faces;
    hipLaunchKernelGGL((k_backward_big<0, true, false>), grid_big, dim3(256), 0, c.st, a);
}

// ====================================================================================================
// Texture cubes shared by the batch (include/nr_hip.h): zeros of the double sums, the gather over (image, face) pairs, the rounding

NR_API size_t nr_backward_textures_shared_workspace_bytes(int32_t B, int32_t Nf, int32_t ts)
{
    if (B < 1 || B > 65535 || Nf < 1 || ts < 2 || ts > 13) return 0;
    return align_up((size_t)Nf * ts * ts * ts * 3 * sizeof(double), 256);  // (the batch does not enter)
}

NR_API int nr_backward_textures_shared(const nr_face_light *lit, const float *faces, const float *faces_z_ref,
                                       const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                       const float *grad_rgb_map, const uint8_t *visible_faces, float *grad_textures, int32_t B,
                                       int32_t F, int32_t S, int32_t ts, double eps, int32_t flags, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (!faces || !face_index_map || !weight_map || !depth_map || !grad_rgb_map || !grad_textures) return NR_E_NULL;
    if (int e = check_sizes(B, F, S)) return e;
    if (ts < 2 || ts > 13) return NR_E_SIZE;
    SharedGatherArgs a = {};
    if (int e = face_light_args(lit, F, true, a.lit)) return e;
    const int Nf = lit ? a.lit.tex_faces : F;
    const size_t n_tex = (size_t)ts * ts * ts * 3, n = (size_t)Nf * n_tex;
    if (!workspace || workspace_bytes < nr_backward_textures_shared_workspace_bytes(B, Nf, ts)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    a.face_index_map = face_index_map, a.faces = faces, a.zbase = faces_z_ref ? faces_z_ref : faces;
    a.weight_map = weight_map, a.depth_map = depth_map, a.g_rgb = grad_rgb_map, a.visible = visible_faces;
    a.sums = (double *)workspace;
    a.F = F, a.S = S, a.ts = ts, a.eps = eps, a.fix_batch_z = (flags & NR_FLAG_FIX_TEXTURE_BATCH_Z) ? 1 : 0;
    // the batched gather's shapes (plan_backward): static taps at texture_size 2, 16 lanes per pair up to 5, a wave up to 8;
    // above, a cube of doubles per workgroup
    const bool ts2 = ts == 2 && (float)(1.0 - eps) < 1.0f;
    a.L = (ts2 || ts <= 5) ? 16 : 64;
    a.wide_all = ts > 8 ? 1 : 0;
    a.n_lds = (int)((ts2 || a.wide_all) ? n_tex : (size_t)(256 / a.L) * n_tex);
    if (int e = fill_bytes(a.sums, 0, n * sizeof(double), st)) return e;
    const dim3 grid((unsigned)((F + 255) / 256), (unsigned)B);
    const size_t lds = (size_t)a.n_lds * sizeof(double);
    if (ts2) {
        if (lit) hipLaunchKernelGGL((k_shared_gather<true, true>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_shared_gather<true, false>), grid, dim3(256), lds, st, a);
    } else {
        if (lit) hipLaunchKernelGGL((k_shared_gather<false, true>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_shared_gather<false, false>), grid, dim3(256), lds, st, a);
    }
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(k_round_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.sums, grad_textures, n);
    return launch_status();
}
