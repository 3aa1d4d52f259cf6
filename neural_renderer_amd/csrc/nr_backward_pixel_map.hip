// nr_backward_pixel_map.hip -- K6, the approximate gradient of rgb / alpha w.r.t. vertex x, y
// (reference Rasterize.backward_pixel_map_gpu, rasterize.py:517-748): its kernels and their host-side steps (the entry point and
// the plan that orders the steps: nr_backward.hip).
//
// One translation unit; the kernel families live in headers that only this file includes, inside its anonymous namespace:
// nr_k6_global.h, nr_k6_lists.h, nr_k6_fast.h, nr_k6_row.h (the lists below say what is where).  This file keeps k_bpm_finalize,
// k_big_overflow, the workspace layouts, the host plan (plan_k6), the launchers, K6's steps as run_backward calls them, the profiling hook.
//
// Which band kernel serves a call (k6_row_band / plan_k6 below; decided on the host from the call's shape alone):
//   k_bpm_row     the default: every call whose raster fits its band (<= 1024), both arithmetic modes;
//   k_bpm_fast    what k_bpm_row does not do: the in-kernel face scan (NR_FLAG_K6_SCAN), the images of a k_bpm_row call whose
//                 records exceed the line buffer (an overflow-only launch behind k_bpm_row, or inside k_big_overflow), rasters
//                 above 1024, the default mode with eps = 0, B > 65535, and NR_FLAG_K6_LEGACY (tests, measurements);
//   k_bpm_global  rasters that fit no LDS band, and NR_FLAG_K6_GLOBAL.
// Measurements on the headline scene (profiles/r01b) showed the global-memory kernel to be bound by memory latency and, for the
// vertical sweeps (axis 0, stride S), by 3x cache-line amplification; the band kernels make every sweep an LDS access.
//
// The band pipeline, in launch order (each step is described where its kernel is):
//   [k_mark_visible]  k_compact_par | k_count_visible + k_compact_visible [+ k_band_scan | k_band_total]   nr_k6_lists.h
//   k_line_setup (or inside the gather's launch: nr_backward_gather.hip, k_setup_gather)                  nr_k6_lists.h
//   k_bpm_row | k_band_gather | k_bpm_fast: line sums into a double scratch array (global_atomic_add_f64) nr_k6_row.h, nr_k6_fast.h
//   [k_bpm_fast, overflow only | k_big_overflow]   behind k_bpm_row: the images over the line buffer      nr_k6_fast.h, below
//   k_bpm_finalize   rounds the scratch sums to float and STORES grad_faces (z = 0; zeros for unlisted faces) -- unless the
//          fused backward's gather or k_backward_big finishes K6 (BackwardPlan::finish)                   below
//
// Two arithmetic modes for the per-pixel terms in either band kernel (DESIGN.md "K6 numerics"; which pixels are visited, by which
// thread, is the same in both; the operations: fast_sweeps in nr_k6_fast.h, the head of nr_k6_row.h): K6_FAST, the north star's
// tolerance (1e-4) spent where it buys time, and K6_EXACT / K6_EXACT_POW2 (NR_FLAG_EXACT_GRADIENT), the reference's arithmetic term
// by term and all sums in double: <= 2e-6 against the exactly summed oracle (_POW2: S is a power of two, x * 2. / S one exact multiply).
#include "nr_device.h"
#include "nr_band_lines.h"
#include "nr_face_gather.h"
#include "nr_k6_tune.h"

#include <atomic>
#include <mutex>
#include <type_traits>

using namespace nr;

namespace {

enum { K6_FAST = 0, K6_EXACT_POW2 = 1, K6_EXACT = 2 };  // the arithmetic modes (above): MODE of both band kernels, K6Plan::mode
#include "nr_k6_global.h"
#include "nr_k6_lists.h"
#include "nr_k6_fast.h"
#include "nr_k6_row.h"

// add: grad_faces holds what K8 left for the face (zeros from the compaction, then the gather's sums: the fused backward whose
// gather runs beside the line setup) and K6's rounded sums go on top -- the one float addition per element that the in-gather
// finish makes, operands exchanged
__global__ __launch_bounds__(256) void k_bpm_finalize(const double *__restrict__ scratch, const int *__restrict__ slot_of,
                                                      float *__restrict__ grad_faces, int F, int n_faces_total, int add)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_faces_total) return;
    const int pos = slot_of[i];
    float *o = grad_faces + (size_t)i * 9;
    if (add) {
        if (pos < 0) return;
        const double *src = scratch + ((size_t)(i / F) * F + pos) * 6;
#pragma unroll
        for (int v = 0; v < 3; v++) {
            o[3 * v + 0] = (float)src[2 * v + 0] + o[3 * v + 0];
            o[3 * v + 1] = (float)src[2 * v + 1] + o[3 * v + 1];
        }
        return;
    }
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (pos >= 0) {
        const double *src = scratch + ((size_t)(i / F) * F + pos) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) a[k] = src[k];
    }
#pragma unroll
    for (int v = 0; v < 3; v++) {
        o[3 * v + 0] = (float)a[2 * v + 0];
        o[3 * v + 1] = (float)a[2 * v + 1];
        o[3 * v + 2] = 0.0f;  // K6 never touches z
    }
}

// --------------------------------------------------------------------------------------------------
// The overflow pass behind k_bpm_row and k_backward_big with K6's finish (FINISH_BIG) in ONE launch: as a launch of its own the
// overflow pass -- which normally finds no image over the line buffer and leaves -- cost 4.6 us of every step.
//   grid = [n_ovf overflow workgroups | k_backward_big's (ranges, images, shares), x fastest]
// This launch is nearly empty -- a few hundred workgroups that leave, and the big faces' -- so the larger of the two bodies'
// registers and LDS costs nothing here (in the band launch k_bpm_fast's 40 KB would cost k_bpm_row a workgroup per CU).
// Nothing waits: with no image over the buffer the overflow workgroups leave after their one look at the verdicts, and
// k_backward_big's threads finish every listed face as before.  Otherwise those threads spare the listed faces of the overflowed
// images, whose sums are still arriving, and the overflow workgroups take a ticket each when their bands are done (the sums
// released at device scope in front of it); whoever draws the last one has thereby acquired all of them and finishes those faces:
// K6's sums, read at device scope, onto grad_faces with the operands and the rule of backward_big_body -- float atomics for a face
// above BIG_PX candidates, whose K8 sums arrive in this launch too (the two additions onto the gather's zero commute), a plain
// read-modify-write for every other, which no one else touches.
struct FastOverflowArgs {
    const float *faces;
    const int32_t *fi_map;
    const float *rgb_map, *alpha_map, *g_rgb, *g_alpha;
    const int *vis_list, *vis_count;
    const unsigned *rng;
    double *scratch;
    const int *band_lines, *band_start, *lines_ok;
    const BandLine *line_buf;
    size_t cap;
    int F, S, W, SP;
    double eps;
    float k2s;
    int B, win_lines, qcap;
    int *ticket;     // zeroed by the compaction
    unsigned n_ovf;  // overflow workgroups in front of k_backward_big's
    unsigned big_x, big_y, big_z;
};

template <bool RGB, bool ALPHA, int MODE, bool DEPTH>
__global__ __launch_bounds__(256, 4) void k_big_overflow(FastOverflowArgs f, BigArgs g)
{
    if (blockIdx.x >= f.n_ovf) {
        const unsigned id = blockIdx.x - f.n_ovf, row = id / f.big_x;
        backward_big_body<2, DEPTH, false>(g, make_uint3(id - row * f.big_x, row % f.big_y, row / f.big_y), f.big_z);
        return;
    }
    if (!bpm_fast_body<RGB, ALPHA, MODE, 256, true>(f.faces, f.fi_map, f.rgb_map, f.alpha_map, f.g_rgb, f.g_alpha, f.vis_list,
                                                     f.vis_count, f.rng, f.scratch, f.band_lines, f.band_start, f.lines_ok, f.line_buf,
                                                     f.cap, f.F, f.S, f.W, f.SP, f.eps, f.k2s, f.B, f.win_lines, f.qcap, nullptr, 0,
                                                     blockIdx.x, f.n_ovf))
        return;
    __shared__ int s_last;
    const int tid = threadIdx.x;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this thread's additions to the sums, in front of the barrier and the ticket
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(f.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)f.n_ovf - 1;
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int F = f.F;
    for (int b = 0; b < f.B; ++b) {
        if (f.lines_ok[b] != 0) continue;
        const int n_vis = f.vis_count[b];
        for (int slot = tid; slot < n_vis; slot += 256) {
            const size_t gi = (size_t)b * F + f.vis_list[(size_t)b * F + slot];
            const double *sc = f.scratch + ((size_t)b * F + slot) * 6;
            const float *fv = f.faces + gi * 9;
            const bool big = face_candidates(fv[0], fv[1], fv[3], fv[4], fv[6], fv[7], f.S).n > BIG_PX;
            float *gf = g.grad_faces + gi * 9;
#pragma unroll
            for (int v = 0; v < 3; v++) {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const float k6v = (float)__hip_atomic_load(sc + 2 * v + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (big) atomicAdd(gf + 3 * v + k, k6v);
                    else gf[3 * v + k] = k6v + gf[3 * v + k];
                }
            }
        }
    }
}

// ====================================================================================================

struct BpmLayout {
    size_t flags_off, scratch_off, count_off, chunk_off, cband_off, list_off, rng_off, slot_off, band_off, start_off, cursor_off, ok_off,
        ticket_off, lines_off, total, cap;
    int n_chunks;
};

// capacity (line records per image) of the band line buffer: a mesh has a few lines per face (teapot 3.8, dense meshes ~2);
// scenes of few large faces are covered by the S term.  Images beyond it take the scan path of k_bpm_fast.
size_t line_capacity(int F, int S)
{
    // + S sqrt(F): a mesh whose V visible faces tile a fixed share of the image has ~ sqrt(V) S records (teapot views: ~100 k at
    // 1024^2, over 8 F + 32 S from raster ~600 on: the scan path cost k_bpm_fast 30 % there and the lane-parallel kernel -- whose
    // overflow launch strides over one-line bands -- a factor).  1.2 S sqrt(F): a mesh that FILLS the image has ~2.1 sqrt(F) S
    // records, which this holds for every raster up to 1264 -- so up to k_bpm_row's largest raster nothing about a mesh's
    // coverage has to be guessed when the band kernel is chosen
    const size_t want = (size_t)8 * F + (size_t)32 * S + (size_t)(1.2 * (double)S * sqrt((double)F));
    // (the images' buffers follow one another: a stride near a multiple of 2 MiB -- 65 579 records x 32 B at the headline shape --
    // puts the same band of every image on the same memory channels and cost k_line_setup 3 us of 25; the stride is kept at
    // 34 KiB past a multiple of 64 KiB)
    return (want + 2047 - 1088) / 2048 * 2048 + 1088;
}

BpmLayout bpm_layout(int B, int F, int S)
{
    BpmLayout L;
    const size_t n = (size_t)B * F;
    L.flags_off = 0;                                  // n bytes (only used when the caller has no visible_faces)
    L.scratch_off = align_up(n, 256);                 // n * 6 doubles, indexed by list position
    L.count_off = align_up(L.scratch_off + n * 6 * sizeof(double), 256);
    L.n_chunks = (F + VIS_CHUNK - 1) / VIS_CHUNK;
    L.chunk_off = L.count_off + align_up((size_t)B * sizeof(int), 256);
    // rows of k_compact_par: [B][n_chunks][2 * n_bands], n_bands <= S
    L.cband_off = L.chunk_off + align_up((size_t)B * L.n_chunks * sizeof(int), 256);
    L.list_off = L.cband_off + (L.n_chunks <= SMALL_CHUNKS ? align_up((size_t)B * L.n_chunks * 2 * S * sizeof(int), 256) : 0);
    L.rng_off = L.list_off + align_up(n * sizeof(int), 256);
    L.slot_off = L.rng_off + align_up(n * 6 * sizeof(unsigned), 256);  // rng: [B][axis][position][edge]
    const size_t per_band = align_up((size_t)B * 2 * S * sizeof(int), 256);  // per (image, axis, band): at most S bands (W = 1)
    L.band_off = L.slot_off + align_up(n * sizeof(int), 256);
    L.start_off = L.band_off + per_band;
    L.cursor_off = L.start_off + per_band;
    L.ok_off = L.cursor_off + per_band;
    L.ticket_off = L.ok_off + align_up((size_t)B * sizeof(int), 256);  // one int: the overflow pass's ticket counter (k_big_overflow)
    L.lines_off = L.ticket_off + 256;
    L.cap = line_capacity(F, S);
    L.total = L.lines_off + (size_t)B * L.cap * sizeof(BandLine);
    return L;
}

// the depth-only backward keeps just the visible-face lists (k_list_visible): [B] counts, then [B][F] list entries
struct ListsLayout {
    size_t count_off, list_off, total;
};
ListsLayout lists_layout(int B, int F)
{
    ListsLayout L;
    L.count_off = 0;
    L.list_off = align_up((size_t)B * sizeof(int), 256);
    L.total = L.list_off + (size_t)B * F * sizeof(int);
    return L;
}

// Shape of a band workgroup, chosen per launch by the raster size (round 4, scripts/k6_variants.py -> profiles/r04_k6_shapes.jsonl;
// K6 stage in us, variants timed in one process behind a throw-away pass: 512 threads / 4-line bands / 53 KB  ->  256
// threads / 2-line bands / 40 KB):
//   teapot 64 x 256^2  209 -> 204    16 x 256^2  99 -> 87    8 x 256^2  69 -> 65    64 x 384^2  499 -> 400   256 x 128^2  330 -> 273
//   config 4 (64 spiky meshes x 10 240 faces, 256^2)  433 -> 367
//   teapot 64 x 448^2  524 -> 579    64 x 512^2  682 -> 701    4 x 1024^2  338 -> 349
// i.e. while a two-line band leaves room for a window of >= 128 lines (raster <= 400 with colours) it wins, walked by four
// waves: the same ~110 lines and ~1 200 pieces per window as four lines give eight waves, in workgroups half the size --
// four per CU, a finer grain for the tail and for the mix of busy and empty bands.  Beyond that the wide shape stays.
BandShape band_shape(int S)
{
    if (S <= k6::SMALL_RASTER_MAX) return {256, 2, (size_t)40 * 1024};  // four workgroups per 160 KB CU
    // rasters of ~600 ... 830: a two-line band no longer fits 53 KB beside a useful line window, and a one-line band stages single
    // columns (64 teapot views, K6 stage: 576^2 857 us -> 608^2 1242, 640^2 1461); with 80 KB -- two workgroups per CU, still four
    // waves per SIMD -- the band stays two lines wide: 640^2 1061, 768^2 1574 -> 1400 (at 512^2 / 576^2 / 1024^2 the same budget
    // costs 5 ... 15 %: there the band width does not change)
    if (S > k6::WIDE_BUDGET_FROM && S <= k6::WIDE_BUDGET_TO) return {512, k6::WMAX, (size_t)80 * 1024};
    return {512, k6::WMAX, k6::LDS_BUDGET};
}

// LDS of k_bpm_fast: pixel arrays [W][SP] (face index 4 B, gradients and colours 16 B each -- 4 B each for alpha alone),
// coverage bits, and what is left is split between the line window (32 B record + two double sums per line; at most one line
// per thread) and the piece queue (2 or 4 B per descriptor).  Returns W (0: the raster does not fit, global fallback).
int fast_band_config(int S, bool rgb, const BandShape &shape, int w_max, size_t *lds_bytes, int *win, int *qcap)
{
    const size_t per_px = rgb ? 36 : 12, SP = (size_t)S + 4, dsz = S > 63 * FSEG ? 4 : 2;
    // pieces per line the split is made for: measured, stage times in us, raster 256: S/22 (192 lines, 3072 descriptors)
    // 240, S/32 (224, 2560) 230, S/48 (256, 2048: two rounds per window) 267; raster 512: S/22 (160, 4096) 906, S/32 (192,
    // 3584) 891, S/48 (224, 2560) 766 -- a band of a 512 x 512 teapot view has ~185 lines: one window instead of two
    const size_t segs_per_line = (size_t)S / (S <= 320 ? 32 : 48) + 3;
    const size_t NT = (size_t)shape.threads, LDS_BUDGET = shape.budget;
    const int win_max = BAND_WIN < shape.threads ? BAND_WIN : shape.threads;
    auto lines_bytes = [&](int ww) { return (sizeof(BandLine) + 16) * (size_t)ww; };
    for (int W = w_max; W >= 1; W >>= 1) {
        const size_t px = (size_t)W * SP * per_px + (size_t)W * (((SP + 31) / 32 + 3) / 4 * 4) * 4 + 16 /* bg */ + 32 /* spans */ + 64 /* scan */ +
                          8 * 16 /* alignment slack */;
        // the budget of the shape; a one-line band may take the whole LDS
        const size_t lim = (W == 1 && px + lines_bytes(32) + NT * dsz > LDS_BUDGET) ? 160 * 1024 : LDS_BUDGET;
        if (px + lines_bytes(32) + NT * dsz > lim) continue;
        const size_t rest = lim - px;
        int w = (int)(rest / (48 + segs_per_line * dsz));
        w = max(32, min(win_max, w / 32 * 32));
        while (w > 32 && lines_bytes(w) + NT * dsz > rest) w -= 32;
        if (W > 1 && w < 96) continue;  // a band this wide leaves no room for a useful line window: narrower bands
        size_t q = (rest - lines_bytes(w)) / dsz / NT * NT;
        q = q > 16384 ? 16384 : q;
        *win = w;
        *qcap = (int)q;
        *lds_bytes = px + lines_bytes(w) + q * dsz;
        return W;
    }
    return 0;
}

// A kernel that asks for more than 48 KB of dynamic LDS has to be told so (hipFuncSetAttribute).  The attribute is sticky,
// so the largest size granted so far is remembered per kernel instantiation and device and the launch path only makes the
// runtime call when a launch needs more than that -- in a steady loop, never.  (A cache of an idempotent driver setting,
// not library state: losing it would only repeat the call.)
struct LdsLimit {
    std::atomic<size_t> granted[32];
    std::mutex mtx;
    LdsLimit() { for (auto &g : granted) g.store(48 * 1024); }
    int ensure(const void *kern, size_t lds)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = 31;
        if (lds <= granted[dev].load(std::memory_order_acquire) && dev != 31) return 0;
        // hipFuncSetAttribute SETS the limit: concurrent callers must never lower it, so the call and the record are one
        // critical section and the value passed is the maximum of what was granted and what is asked for
        std::lock_guard<std::mutex> lock(mtx);
        const size_t have = granted[dev].load(std::memory_order_relaxed);
        if (lds <= have && dev != 31) return 0;
        const size_t want = lds > have ? lds : have;
        const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
        if (e != 0) return e;
        granted[dev].store(want, std::memory_order_release);
        return 0;
    }
};

// The launch of a kernel with dynamic LDS: the limit, then the launch.  The kernel is a template ARGUMENT, so that every kernel
// instantiation has a remembered limit of its own (instantiations of one template share their pointer's TYPE).
template <auto Kern, class... Args> int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args)
{
    static LdsLimit limit;
    if (int rc = limit.ensure((const void *)Kern, lds)) return rc;
    hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
    return 0;
}

// The call's (rgb, alpha) as template arguments of f(r, a): the three map combinations of the ABI (rgb and alpha, rgb, alpha) ...
template <class Fn> int with_k6_maps(bool rgb, bool alpha, const Fn &f)
{
    using T = std::true_type;
    using N = std::false_type;
    return (rgb && alpha) ? f(T(), T()) : (rgb ? f(T(), N()) : f(N(), T()));
}
// ... and (rgb, alpha, mode) of f(r, a, m): times the three arithmetic modes.  Both band kernels are launched through it.
template <class Fn> int with_k6_types(bool rgb, bool alpha, int mode, const Fn &f)
{
    return with_k6_maps(rgb, alpha, [&](auto r, auto a) {
        if (mode == K6_FAST) return f(r, a, std::integral_constant<int, K6_FAST>());
        if (mode == K6_EXACT_POW2) return f(r, a, std::integral_constant<int, K6_EXACT_POW2>());
        return f(r, a, std::integral_constant<int, K6_EXACT>());
    });
}

template <bool RGB, bool ALPHA, int MODE, bool OVF>
int launch_fast(const K6Plan &p, const BackwardCall &c, const K6Lists &l, const LineSetupArgs &ls, void *zero_ptr, size_t zero_bytes)
{
    const int B = c.B, S = c.S;
    const unsigned total_wg = (unsigned)((S + p.W_fast - 1) / p.W_fast) * 2u * (unsigned)B;
    // 1-D grid: the kernel maps ids to (image, axis, band) per XCD
    // (overflow-only launch behind k_bpm_row -- where the plan does not put the pass into k_backward_big's launch, k_big_overflow:
    // a resident grid that strides over the bands, k6::OVF_GRID workgroups.  With nothing to do it costs 4.6 us in a traced step
    // whatever the grid -- a launch (1.3 us for up to 256 workgroups that leave at once,
    // scripts/dev/empty_launch_probe.hip) and one dependent load of the images' verdicts from memory the line setup wrote with
    // atomics; with every image over the line buffer -- 32 teapot views at 1024^2 -- 1024 workgroups took 5.0 ms against 7.3 at 256)
    const unsigned grid = OVF ? (total_wg < k6::OVF_GRID ? total_wg : k6::OVF_GRID) : xcd_grid(total_wg);
    auto go = [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        return launch_lds<k_bpm_fast<RGB, ALPHA, MODE, NT, OVF>>(
            dim3(grid), dim3(NT), p.fast_lds, c.st, c.faces, c.face_index_map, c.rgb_map, c.alpha_map, c.grad_rgb_map, c.grad_alpha_map,
            l.vis_list, l.vis_count, ls.rng, l.scratch, ls.band_lines, ls.band_start, ls.lines_ok, ls.line_buf, ls.cap, c.F, S, p.W_fast,
            S + 4, c.eps, ls.k2s, B, p.win_lines, p.qcap, (uint4 *)zero_ptr, zero_bytes / 16);
    };
    return p.shape.threads == 256 ? go(std::integral_constant<int, 256>()) : go(std::integral_constant<int, 512>());
}

// k_bpm_row's chunks: a line is cut into ceil(S / 512) pieces of equal length (a multiple of 32 pixels, the last one shorter):
// the whole line up to raster 512, 2 x 320 at 640, 2 x 512 at 1024 (see the kernel) -- on meshes of fewer than 2^15 faces.  A
// record is set up once per chunk, and on a dense mesh (hundreds of records per line) that costs more than the column bands'
// staging gains: config 5 (655 360 faces at 1024^2) 1.34 ms per step with whole lines, 1.38 with half lines.
constexpr int ROW_CHUNK_PX = 512;  // the longest chunk
int row_chunk(int S, int F)
{
    if (F >= (1 << 15)) return (S + 31) & ~31;
    const int n_ch = (S + ROW_CHUNK_PX - 1) / ROW_CHUNK_PX, len = (S + n_ch - 1) / n_ch;
    return (len + 31) & ~31;
}

// k_bpm_row's band: the widest power of two of lines (<= one per wave) whose chunks fit its LDS regions (rowk::MAX_PX); 0: the
// raster is too large for it (k_bpm_fast takes the launch)
int row_band_config(int S, int F, bool rgb, bool exact, int B, size_t *lds_bytes)
{
    if ((((size_t)S + 31) & ~(size_t)31) / rowk::SEG > (size_t)rowk::MAX_SEGS) return 0;
    const size_t SP = (size_t)row_chunk(S, F), n_ch = ((size_t)S + SP - 1) / SP;
    for (int W = rowk::NW; W >= 1; W >>= 1) {
        // (small launches: narrower bands while there are few band workgroups -- the waves of a workgroup then share the windows of
        // a line.  One-line bands stage single columns and most lines have one window, i.e. one busy wave: only below
        // ROW_MIN_WGS_1 workgroups.  K6 stage, us, four- / two- / one-line bands: 4 views 46.3 (1) -> 45.4 (2); 8 views 62.8 (4),
        // 59.3 (2), 61.8 (1); 16 views 79.9 (4), 75.6 (2), 86.0 (1); 8 views at 512^2 115.6 (2), 122.5 (1))
        const size_t wgs = (size_t)B * 2 * ((S + W - 1) / W) * n_ch;
        if ((W > 2 && wgs < k6::ROW_MIN_WGS) || (W == 2 && wgs < k6::ROW_MIN_WGS_1)) continue;
        if ((size_t)W * SP > (size_t)rowk::MAX_PX) continue;
        const size_t npx = (size_t)W * SP;
        *lds_bytes = rgb ? (exact ? rowk::lds_bytes<true, true>(npx) : rowk::lds_bytes<true, false>(npx))
                         : (exact ? rowk::lds_bytes<false, true>(npx) : rowk::lds_bytes<false, false>(npx));
        return W;
    }
    return 0;
}

template <bool RGB, bool ALPHA, int MODE>
int launch_row(const K6Plan &p, const BackwardCall &c, const K6Lists &l, const LineSetupArgs &ls, void *zero_ptr, size_t zero_bytes)
{
    const int B = c.B, F = c.F, S = c.S;
    const int CH = row_chunk(S, F), W = p.W_row;
    const unsigned n_ch = (unsigned)((S + CH - 1) / CH), total_wg = (unsigned)((S + W - 1) / W) * 2u * (unsigned)B * n_ch;
    auto go = [&](auto chunked) {  // (40 KB of LDS at most with the product's constants: the limit is never raised)
        return launch_lds<k_bpm_row<RGB, ALPHA, MODE, decltype(chunked)::value>>(
            dim3(xcd_grid(total_wg)), dim3(rowk::NT), p.row_lds, c.st, c.face_index_map, c.rgb_map, c.alpha_map, c.grad_rgb_map,
            c.grad_alpha_map, l.scratch, ls.band_lines, ls.band_start, ls.lines_ok, ls.line_buf, ls.cap, F, S, W, CH, (float)c.eps, c.eps, B,
            (uint4 *)zero_ptr, zero_bytes / 16);
    };
    return n_ch > 1 ? go(std::true_type()) : go(std::false_type());
}

// The merged launch: k_bpm_row's grid with the K7 / K8 face gather's workgroups behind it (k_band_gather).  fill: grad_textures
// when the band workgroups zero the unlisted faces' cubes (texture_size 2: six 16-byte words per cube), else NULL.
template <bool RGB, bool ALPHA>
int launch_band_gather(const K6Plan &p, const BackwardCall &c, const BackwardPlan &bp, const K6Lists &l, const LineSetupArgs &ls,
                       void *fill, size_t fill_bytes)
{
    const int B = c.B, F = c.F, S = c.S, W = p.W_row;
    const unsigned total_wg = (unsigned)((S + W - 1) / W) * 2u * (unsigned)B, band_grid = xcd_grid(total_wg);
    const unsigned gather_x = ((unsigned)((F + 15) / 16) + k6::SLOT_STRIDE - 1) / k6::SLOT_STRIDE;  // (k_band_gather loops)
    BandRowArgs ra = {};
    ra.fi_map = c.face_index_map;   ra.rgb_map = c.rgb_map;         ra.alpha_map = c.alpha_map;
    ra.g_rgb = c.grad_rgb_map;      ra.g_alpha = c.grad_alpha_map;  ra.scratch = l.scratch;
    ra.band_lines = ls.band_lines;  ra.band_start = ls.band_start;  ra.lines_ok = ls.lines_ok;
    ra.line_buf = ls.line_buf;      ra.cap = ls.cap;                ra.B = B;
    ra.F = F;                       ra.S = S;                       ra.W = W;
    ra.CH = S;  // (whole lines)
    ra.eps_f = (float)c.eps;        ra.eps_d = c.eps;
    ra.zero16 = (uint4 *)fill;      ra.n_zero16 = fill_bytes / 16;  ra.zero_slot = l.slot_of;       ra.zero_epf = 6u;
    const FaceGatherArgs ga = face_gather_args(c, bp, l);
    auto go = [&](auto depth) {
        return launch_lds<k_band_gather<RGB, ALPHA, decltype(depth)::value>>(dim3(band_grid + gather_x * (unsigned)B), dim3(rowk::NT),
                                                                             p.row_lds, c.st, ra, ga, band_grid, gather_x);
    };
    return bp.depth_in_gather ? go(std::true_type()) : go(std::false_type());
}

// Whether k_bpm_row takes a call whose raster has a k_bpm_fast band: its band width (lines per workgroup) and LDS bytes, or 0.
// Both arithmetic modes have ONE band kernel since round 6, k_bpm_row: it is ahead of k_bpm_fast on every shape measured
// (profiles/r06_k6_kernels.md: 8 ... 128 teapot views at 256^2, 64 views at rasters 320 ... 768, 32 and 4 views at 1024^2, 256
// views at 128^2, 1024 at 32^2, configs 4 and 5; the exact mode: 64 views at 256^2 and 512^2), so nothing about the call's size
// enters the choice -- a batch and its shards take the same kernel.  k_bpm_fast keeps what k_bpm_row does not do: the in-kernel
// face scan (NR_FLAG_K6_SCAN, and the images of a call whose records exceed the line buffer: an overflow-only launch behind
// k_bpm_row), rasters beyond k_bpm_row's LDS band (> 1024), the default mode with eps = 0 (a lane outside a sweep multiplies 0
// by 1 / (|c t| + eps), and t = 0 -- the crossing point on a pixel centre -- would make that 0 * Inf; the exact mode selects in
// front of its division and takes any eps), and NR_FLAG_K6_LEGACY (tests, measurements).
// With k_bpm_row the band tables and the line records are binned per LINE (band width 1).
int k6_row_band(int B, int F, int S, bool rgb, double eps, int flags, size_t *row_lds)
{
    const bool exact = (flags & NR_FLAG_EXACT_GRADIENT) != 0;
    const bool possible = !(flags & (NR_FLAG_K6_SCAN | NR_FLAG_K6_LEGACY)) && B <= 65535 && (exact || (float)eps >= 1e-30f);
    return possible ? row_band_config(S, F, rgb, exact, B, row_lds) : 0;
}

}  // namespace

// Which band kernel a call takes, and how it is shaped: decided once per call, on the host, from the call's shape alone (no
// device).  plan_backward (nr_backward.hip) takes it into the call's plan; nr_profile_k6_choice reports its kernel.
K6Plan nr::plan_k6(int B, int F, int S, bool rgb, double eps, int flags)
{
    K6Plan p = {};
    const bool exact = (flags & NR_FLAG_EXACT_GRADIENT) != 0;
    p.mode = !exact ? K6_FAST : ((S & (S - 1)) == 0 ? K6_EXACT_POW2 : K6_EXACT);
    // Narrower bands when the launch would have few band workgroups (small batches): the chip holds 768 of them at a time and
    // half of a teapot view's bands are empty; 16 views: stage 113 -> 104 us with W = 2, 4 views 70 -> 50, 1 view 66 -> 40 (W = 1).
    p.shape = band_shape(S);
    int w_max = p.shape.w_max, win = BAND_WIN;
    while (w_max > 1 && (size_t)B * 2 * ((S + w_max - 1) / w_max) < 3072) w_max >>= 1;
    p.W_fast = fast_band_config(S, rgb, p.shape, w_max, &p.fast_lds, &win, &p.qcap);
    if (p.W_fast == 0 || (flags & NR_FLAG_K6_GLOBAL)) {  // raster too large for an LDS band (or the fallback asked for: tests)
        p.kernel = K6_KERNEL_GLOBAL;
        return p;
    }
    // lines per window: the packed piece scan keeps each class count in 16 bits (<= win * 2 * S / FSEG pieces)
    p.win_lines = min(win, max(4, min(BAND_WIN, (int)(65535ll * FSEG / (2ll * S))) & ~3));
    p.W_row = k6_row_band(B, F, S, rgb, eps, flags, &p.row_lds);
    const bool row = p.W_row > 0;
    p.kernel = row ? K6_KERNEL_ROW : K6_KERNEL_FAST;
    p.overflow_pass = row;
    p.row_chunked = row && row_chunk(S, F) < S;
    p.W = row ? 1 : p.W_fast;
    p.n_bands = (S + p.W - 1) / p.W;
    // line records from k_line_setup, unless NR_FLAG_K6_SCAN asks for the in-kernel face scan (tests) or the launch is
    // outside k_line_setup's shape (grid.y, 72 KB of LDS)
    p.use_records = !(flags & NR_FLAG_K6_SCAN) && B <= 65535 && p.n_bands <= 3072;
    // (a fill that rides in the band kernel: 16-byte words, and a slice per workgroup that is small next to the
    // workgroup's own work -- k6::FOLD_KB per band workgroup: 4 KB at the headline size, 61 KB on config 4; config 5's
    // 4 GB would be 2 MB for each of 2048 workgroups and go at 7 TB/s through a fill launch instead.  A 256-thread workgroup
    // takes half of what a 512-thread one does.)
    const int W_band = row ? p.W_row : p.W_fast;
    const size_t band_wgs = (size_t)((S + W_band - 1) / W_band) * 2 * (size_t)B;
    p.fill_max = band_wgs * ((size_t)k6::FOLD_KB << 10) * (size_t)(row ? rowk::NT : p.shape.threads) / 512;
    return p;
}

NR_API size_t nr_backward_workspace_bytes(int32_t B, int32_t F, int32_t S, int32_t return_rgb, int32_t return_alpha)
{
    if (check_sizes(B, F, S)) return 0;
    // depth only (no K6): nothing but the per-image lists of the faces that own a pixel, for the K8 gather
    if (!return_rgb && !return_alpha) return lists_layout(B, F).total;
    return bpm_layout(B, F, S).total;
}

// Measurement hook (include/nr_hip_profile.h, nr_profile_band_kernel): a pair of events around the band kernel's launch.  Only in the
// measurement build of the library (libnr_hip_prof.so, -DNR_PROFILE_HOOK: neural_renderer_amd._build.build_profile); the product
// library keeps no such state and does not export the two functions.
#ifdef NR_PROFILE_HOOK
#include "../../include/nr_hip_profile.h"
namespace {
struct BandKernelTimer {
    bool on = false, recorded = false;
    int which = -1;  // the bracketed launch: 0 k_bpm_fast, 1 k_bpm_row
    hipEvent_t start = nullptr, stop = nullptr;
} g_band_timer;
}  // namespace

NR_API int nr_profile_band_kernel(int32_t enable)
{
    BandKernelTimer &t = g_band_timer;
    if (enable && !t.start) {
        if (hipEventCreate(&t.start) != hipSuccess || hipEventCreate(&t.stop) != hipSuccess) {
            t.start = t.stop = nullptr;
            return launch_status();
        }
    }
    t.on = enable != 0 && t.start != nullptr;
    t.recorded = false;
    return 0;
}

NR_API float nr_profile_band_kernel_ms(void)
{
    BandKernelTimer &t = g_band_timer;
    float ms = -1.0f;
    if (!t.recorded || hipEventSynchronize(t.stop) != hipSuccess || hipEventElapsedTime(&ms, t.start, t.stop) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0f;
    }
    return ms;
}
NR_API int nr_profile_band_kernel_which(void) { return g_band_timer.recorded ? g_band_timer.which : -1; }
// (pure host logic, no device needed: the per-launch rule as a function of the call's shape, for tests/test_abi.py)
NR_API int nr_profile_k6_choice(int32_t B, int32_t F, int32_t S, int32_t return_rgb, int32_t return_alpha, double eps, int32_t flags)
{
    (void)return_alpha;
    return plan_k6(B, F, S, return_rgb != 0, eps, flags).kernel == K6_KERNEL_ROW ? 1 : 0;
}
#define NR_BAND_TIMER_START(st, kernel) if (g_band_timer.on) { g_band_timer.which = (kernel); g_band_timer.recorded = hipEventRecord(g_band_timer.start, st) == hipSuccess; }
#define NR_BAND_TIMER_STOP(st) if (g_band_timer.on && g_band_timer.recorded) g_band_timer.recorded = hipEventRecord(g_band_timer.stop, st) == hipSuccess
#else
#define NR_BAND_TIMER_START(st, kernel) ((void)0)
#define NR_BAND_TIMER_STOP(st) ((void)0)
#endif

// --------------------------------------------------------------------------------------------------
// K6's steps: run_backward (nr_backward.hip) launches them in the order its plan says

// the compaction writes the chunk rows of k_compact_par (n_sum > 0: the consumer adds them up) while the two fit its LDS
static bool compact_in_one_launch(const BpmLayout &L, int n_bands) { return L.n_chunks <= SMALL_CHUNKS && n_bands <= 4096; }

int nr::k6_compact(const BackwardCall &c, const K6Plan &plan, int face_zeros, K6Lists &out)
{
    const int B = c.B, F = c.F, S = c.S, n = B * F;
    const BpmLayout L = bpm_layout(B, F, S);
    const hipStream_t st = c.st;
    unsigned char *ws = (unsigned char *)c.workspace;
    int *band_lines = (int *)(ws + L.band_off);
    const int W = plan.W, n_bands = plan.n_bands;
    double *scratch = (double *)(ws + L.scratch_off);
    int *vis_count = (int *)(ws + L.count_off);
    int *vis_list = (int *)(ws + L.list_off);
    int *slot_of = (int *)(ws + L.slot_off);
    unsigned *rng = (unsigned *)(ws + L.rng_off);
    int *ticket = (int *)(ws + L.ticket_off);
    out = {vis_list, vis_count, slot_of, scratch, ticket};
    const unsigned char *vflags = c.visible_faces;
    if (!vflags) {  // the forward's flags were not kept: one pass over face_index_map rebuilds them
        unsigned char *f = ws + L.flags_off;
        const int he = fill_bytes(f, 0, (size_t)n, st);
        if (he != 0) return he;
        const size_t P = (size_t)B * S * S;
        hipLaunchKernelGGL(k_mark_visible, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, c.face_index_map, f, F,
                           S * S, P);
        vflags = f;
    }
    int *band_start = (int *)(ws + L.start_off), *band_cursor = (int *)(ws + L.cursor_off), *lines_ok = (int *)(ws + L.ok_off);
    float *zero_faces = face_zeros != FACE_ZEROS_NONE ? c.grad_faces : nullptr;
    const int zero_listed = face_zeros == FACE_ZEROS_ALL ? 1 : 0;
    if (compact_in_one_launch(L, n_bands)) {
        int *chunk_band = (int *)(ws + L.cband_off);
        // (line-difference counting while the two line arrays fit beside the band counters: raster sides up to 3583)
        const int use_diff = (size_t)(2 * n_bands + 2 * (S + 1)) * sizeof(int) <= 40960 ? 1 : 0;
        hipLaunchKernelGGL(k_compact_par, dim3((unsigned)L.n_chunks, (unsigned)B), dim3(VIS_CHUNK),
                           (size_t)(2 * n_bands + (use_diff ? 2 * (S + 1) : 0)) * sizeof(int), st, vflags, vis_list, vis_count,
                           slot_of, F, L.n_chunks, c.faces, rng, scratch, S, chunk_band, n_bands, W, band_cursor, zero_faces,
                           zero_listed, use_diff, ticket);
        if (!plan.use_records)
            hipLaunchKernelGGL(k_band_total, dim3((unsigned)B), dim3(256), 0, st, chunk_band, L.n_chunks, band_lines, band_start,
                               lines_ok, n_bands);
    } else {
        int *chunk_count = (int *)(ws + L.chunk_off);
        hipLaunchKernelGGL(k_count_visible, dim3((unsigned)L.n_chunks, (unsigned)B), dim3(VIS_CHUNK), 0, st, vflags,
                           chunk_count, F, L.n_chunks, band_lines, n_bands);
        const int lds_counters = n_bands <= 4096;  // 32 KB of LDS at most
        hipLaunchKernelGGL(k_compact_visible, dim3((unsigned)L.n_chunks, (unsigned)B), dim3(VIS_CHUNK),
                           lds_counters ? (size_t)2 * n_bands * sizeof(int) : 0, st, vflags, chunk_count, vis_list, vis_count,
                           slot_of, F, L.n_chunks, c.faces, rng, scratch, S, band_lines, n_bands, W, lds_counters, zero_faces,
                           zero_listed);
        // (capacity 0: every image is told to take the scan path)
        hipLaunchKernelGGL(k_band_scan, dim3((unsigned)B), dim3(256), 0, st, band_lines, band_start, band_cursor, lines_ok,
                           n_bands, plan.use_records ? L.cap : 0, 0, ticket);
    }
    return launch_status();
}

LineSetupArgs nr::k6_line_setup_args(const BackwardCall &c, const K6Plan &plan)
{
    const BpmLayout L = bpm_layout(c.B, c.F, c.S);
    unsigned char *ws = (unsigned char *)c.workspace;
    const int n_bands = plan.n_bands;
    // the distance coefficients of a record: x 2 / S up front in the tolerance mode, as the reference has them in the exact one
    const float k2s = (c.flags & NR_FLAG_EXACT_GRADIENT) ? 1.0f : 2.0f / (float)c.S;
    // workgroups per image: a slot of LS_FACES list positions each, or every k6::SLOT_STRIDE-th slot and a loop (line_setup_body)
    const unsigned slots = (unsigned)((c.F + LS_FACES - 1) / LS_FACES);
    const unsigned stride = (c.flags & NR_FLAG_SERIAL_BACKWARD) ? 1u : k6::SLOT_STRIDE;
    return {c.faces, c.face_index_map, (const int *)(ws + L.list_off), (const int *)(ws + L.count_off),
            (const unsigned *)(ws + L.rng_off), (const int *)(ws + L.cband_off), compact_in_one_launch(L, n_bands) ? L.n_chunks : 0,
            (int *)(ws + L.band_off), (int *)(ws + L.start_off), (int *)(ws + L.cursor_off), (int *)(ws + L.ok_off),
            (BandLine *)(ws + L.lines_off), L.cap, c.F, c.S, plan.W, n_bands, k2s, (slots + stride - 1) / stride,
            (unsigned)c.B, (size_t)6 * n_bands * sizeof(int)};
}

int nr::run_line_setup(const LineSetupArgs &a, hipStream_t st)
{
    const int rc = launch_lds<k_line_setup>(dim3(a.grid_x * a.grid_y), dim3(256), a.lds_bytes, st, a);
    return rc ? rc : launch_status();
}

// The global-memory kernel, or the band kernel (k_bpm_row or k_bpm_fast, with the zero fill `fill` when the plan gave it one)
// and then the overflow-only k_bpm_fast launch behind k_bpm_row: the images whose records exceed the line buffer, by the face
// scan, no fill.  (l, ls: the compaction's lists and the band tables and line records of k6_line_setup_args.)
// tail: the plan of a fused backward whose K7 / K8 gather shares k_bpm_row's launch (gather_in_tail; the fill then spares the
// listed faces' cubes), else NULL.  overflow_later: the overflow pass rides in k_backward_big's launch (k6_big_overflow).
int nr::k6_band(const BackwardCall &c, const K6Plan &plan, const K6Lists &l, const LineSetupArgs &ls, void *fill, size_t fill_bytes,
                const BackwardPlan *tail, bool overflow_later)
{
    if (plan.kernel == K6_KERNEL_GLOBAL)
        return with_k6_maps(c.rgb, c.alpha, [&](auto r, auto a) {
            hipLaunchKernelGGL((k_bpm_global<decltype(r)::value, decltype(a)::value>), dim3((unsigned)(c.B * c.F)), dim3(WAVE), 0,
                               c.st, c.faces, c.face_index_map, c.rgb_map, c.alpha_map, c.grad_rgb_map, c.grad_alpha_map,
                               c.grad_faces, c.F, c.S, c.eps);
            return launch_status();
        });
    auto band_fast = [&](auto overflow_only, void *zp, size_t zb) {
        return with_k6_types(c.rgb, c.alpha, plan.mode, [&](auto r, auto a, auto m) {
            return launch_fast<decltype(r)::value, decltype(a)::value, decltype(m)::value, decltype(overflow_only)::value>(
                plan, c, l, ls, zp, zb);
        });
    };
    auto band_row = [&]() {
        return with_k6_types(c.rgb, c.alpha, plan.mode, [&](auto r, auto a, auto m) {
            return launch_row<decltype(r)::value, decltype(a)::value, decltype(m)::value>(plan, c, l, ls, fill, fill_bytes);
        });
    };
    auto band_gather = [&]() {
        return with_k6_maps(c.rgb, c.alpha, [&](auto r, auto a) {
            return launch_band_gather<decltype(r)::value, decltype(a)::value>(plan, c, *tail, l, ls, fill, fill_bytes);
        });
    };
    NR_BAND_TIMER_START(c.st, plan.kernel);
    int rc = tail ? band_gather() : (plan.kernel == K6_KERNEL_ROW ? band_row() : band_fast(std::false_type(), fill, fill_bytes));
    NR_BAND_TIMER_STOP(c.st);
    if (rc == 0 && plan.overflow_pass && !overflow_later) rc = band_fast(std::true_type(), nullptr, 0);
    return rc ? rc : launch_status();
}

// k_bpm_fast's overflow pass and k_backward_big with K6's finish in one launch (k_big_overflow; BackwardPlan::big_overflow)
int nr::k6_big_overflow(const BackwardCall &c, const BackwardPlan &bp, const K6Lists &l, const LineSetupArgs &ls)
{
    const K6Plan &p = bp.k6p;
    const int B = c.B, S = c.S;
    const unsigned total_wg = (unsigned)((S + p.W_fast - 1) / p.W_fast) * 2u * (unsigned)B;
    const unsigned n_ovf = total_wg < k6::OVF_GRID ? total_wg : k6::OVF_GRID;
    BigArgs ga = big_args(c, bp, l);
    ga.lines_ok = ls.lines_ok;
    const dim3 big = big_grid(ga.vis_list != nullptr, B, c.F);
    const FastOverflowArgs fa = {c.faces, c.face_index_map, c.rgb_map, c.alpha_map, c.grad_rgb_map, c.grad_alpha_map, l.vis_list,
                                 l.vis_count, ls.rng, l.scratch, ls.band_lines, ls.band_start, ls.lines_ok, ls.line_buf, ls.cap, c.F, S,
                                 p.W_fast, S + 4, c.eps, ls.k2s, B, p.win_lines, p.qcap, l.ticket, n_ovf, big.x, big.y, big.z};
    const size_t n_wg = (size_t)n_ovf + (size_t)big.x * big.y * big.z;
    if (n_wg > 0x7fffffffull) return NR_E_SIZE;
    const int rc = with_k6_types(c.rgb, c.alpha, p.mode, [&](auto r, auto a, auto m) {
        auto go = [&](auto depth) {
            return launch_lds<k_big_overflow<decltype(r)::value, decltype(a)::value, decltype(m)::value, decltype(depth)::value>>(
                dim3((unsigned)n_wg), dim3(256), p.fast_lds, c.st, fa, ga);
        };
        return ga.g_depth ? go(std::true_type()) : go(std::false_type());
    });
    return rc ? rc : launch_status();
}

// add: on top of what grad_faces holds, listed faces only (see the kernel)
void nr::k6_finalize(const BackwardCall &c, const K6Lists &l, bool add)
{
    const int n = c.B * c.F;
    hipLaunchKernelGGL(k_bpm_finalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, l.scratch, l.slot_of, c.grad_faces,
                       c.F, n, add ? 1 : 0);
}

bool nr::k6_lists_fit(int B, int F, size_t workspace_bytes)
{
    return workspace_bytes >= lists_layout(B, F).total && (F + VIS_CHUNK - 1) / VIS_CHUNK <= SMALL_CHUNKS;
}

// the lists alone, from the forward's flags (a depth-only fused backward: no K6)
K6Lists nr::k6_list_visible(const BackwardCall &c)
{
    const ListsLayout L = lists_layout(c.B, c.F);
    const int n_chunks = (c.F + VIS_CHUNK - 1) / VIS_CHUNK;
    unsigned char *ws = (unsigned char *)c.workspace;
    int *list = (int *)(ws + L.list_off), *count = (int *)(ws + L.count_off);
    hipLaunchKernelGGL(k_list_visible, dim3((unsigned)n_chunks, (unsigned)c.B), dim3(VIS_CHUNK), 0, c.st, c.visible_faces, list,
                       count, c.F, n_chunks);
    return {list, count, nullptr, nullptr};
}
