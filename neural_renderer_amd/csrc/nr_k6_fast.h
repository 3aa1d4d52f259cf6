// nr_k6_fast.h -- k_bpm_fast, the band kernel that gives a lane a PIECE of a sweep.  Part of the translation unit
// nr_backward_pixel_map.hip (included there and nowhere else, behind nr_k6_lists.h); what it still serves: that file's overview.
//   k_bpm_fast<RGB, ALPHA, MODE>   one workgroup per (image, axis, band of W consecutive lines d0); workgroup ids are
//          mapped so that all bands of an image run on one XCD (xcd_block).  It
//          1. stages the band's W x S pixels in LDS, laid out [line][d1] so that a sweep is a contiguous LDS run
//             whatever the axis;
//          2. takes its line records a window at a time: the band's slice of k_line_setup's buffer -- or, for an image whose
//             records exceed the buffer (and with NR_FLAG_K6_SCAN), a scan of the image's visible faces (one per thread, 12
//             coalesced bytes each: the precomputed d0 ranges clipped to the band) that sets the window's lines up in place;
//          3. sweeps (fast_sweeps): the in / out sweeps of all lines are cut into pieces of <= FSEG = 15 pixels, sorted into
//             coverage classes, numbered through by one packed scan and handed to the threads through a descriptor queue;
//             the two partial sums of a piece are added to per-line LDS accumulators (ds_add_f64);
//          4. adds the line sums to a double scratch array [B][list position][3 vertices][x|y] (global_atomic_add_f64).
constexpr int BAND_WIN = 256;    // line records per window, at most
constexpr int FSEG = 15;         // pixels per piece (odd: consecutive pieces of a sweep start on different LDS banks;
                                 // re-swept in round 3: 9 / 12 / 15 / 18 pixels -> stage 242 / 237 / 230 / 233 us)

struct FastPx {  // LDS pixel data of a band, [line][d1]
    int *fi;     // face index
    float *g;    // gradients (g_alpha, g_r, g_g, g_b) -- or g_alpha alone
    float *c;    // colours   (alpha, r, g, b)         -- or alpha alone
    float *bg;   // colour of the band's uncovered pixels
    unsigned *cov;  // coverage bits [line][CW words]: bit d1 & 31 of word d1 >> 5 set <=> a face owns pixel (line, d1)
    int CW;         // words per line
    int *span;      // [line][2]: first and last covered pixel of the line (first > last: none)
};

// Four adjacent pixels of a map row with one 16-byte load per field (both band kernels' staging)
struct PxQuad {
    int fi[4];
    float al[4], ga[4], rr[12], qq[12];
};
template <bool RGB, bool ALPHA>
__device__ __forceinline__ PxQuad load_px_quad(const int32_t *fi_map, const float *rgb_map, const float *alpha_map, const float *g_rgb,
                                               const float *g_alpha, size_t g)
{
    PxQuad q;
    const int4 vf = *reinterpret_cast<const int4 *>(fi_map + g);
    float4 va = make_float4(0, 0, 0, 0), vg = va;
    if (ALPHA) {
        va = *reinterpret_cast<const float4 *>(alpha_map + g);
        vg = *reinterpret_cast<const float4 *>(g_alpha + g);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) q.rr[k] = q.qq[k] = 0.0f;
    if (RGB) {
        const float4 *pr = reinterpret_cast<const float4 *>(rgb_map + 3 * g);
        const float4 *pg = reinterpret_cast<const float4 *>(g_rgb + 3 * g);
        const float4 r0 = pr[0], r1 = pr[1], r2 = pr[2], q0 = pg[0], q1 = pg[1], q2 = pg[2];
        q.rr[0] = r0.x; q.rr[1] = r0.y; q.rr[2] = r0.z; q.rr[3] = r0.w; q.rr[4] = r1.x; q.rr[5] = r1.y; q.rr[6] = r1.z; q.rr[7] = r1.w;
        q.rr[8] = r2.x; q.rr[9] = r2.y; q.rr[10] = r2.z; q.rr[11] = r2.w;
        q.qq[0] = q0.x; q.qq[1] = q0.y; q.qq[2] = q0.z; q.qq[3] = q0.w; q.qq[4] = q1.x; q.qq[5] = q1.y; q.qq[6] = q1.z; q.qq[7] = q1.w;
        q.qq[8] = q2.x; q.qq[9] = q2.y; q.qq[10] = q2.z; q.qq[11] = q2.w;
    }
    q.fi[0] = vf.x; q.fi[1] = vf.y; q.fi[2] = vf.z; q.fi[3] = vf.w;
    q.al[0] = va.x; q.al[1] = va.y; q.al[2] = va.z; q.al[3] = va.w;
    q.ga[0] = vg.x; q.ga[1] = vg.y; q.ga[2] = vg.z; q.ga[3] = vg.w;
    return q;
}

template <bool RGB, bool ALPHA, int NT>
__device__ __forceinline__ void fast_stage(const FastPx &px, const int32_t *__restrict__ fi_map,
                                           const float *__restrict__ rgb_map, const float *__restrict__ alpha_map,
                                           const float *__restrict__ g_rgb, const float *__restrict__ g_alpha, size_t img,
                                           int axis, int band_lo, int nld, int S, int SP)
{
    const int tid = threadIdx.x;
    // pixel d1 of band line ld.  The coverage bits (px.cov, zeroed by the caller before the barrier in front of this
    // function) let the out sweeps skip the face index: only the covered eighth of the pixels issues the atomic.
    auto put = [&](int ld, int d1, int fi, float al, float ga, float r, float g, float bl, float gr, float gg, float gb) {
        const int l = ld * SP + d1;
        px.fi[l] = fi;
        if (RGB) {
            *reinterpret_cast<float4 *>(px.g + 4 * (size_t)l) = make_float4(ga, gr, gg, gb);
            *reinterpret_cast<float4 *>(px.c + 4 * (size_t)l) = make_float4(al, r, g, bl);
            if (px.bg && fi < 0) *reinterpret_cast<float4 *>(px.bg) = make_float4(al, r, g, bl);  // same value from every such pixel
        } else {
            px.g[l] = ga;
            px.c[l] = al;
            if (px.bg && fi < 0) px.bg[0] = al;
        }
        if (px.cov && fi >= 0) atomicOr(px.cov + ld * px.CW + (d1 >> 5), 1u << (d1 & 31));  // (callers without coverage bits pass none)
    };
    // four adjacent pixels of a map row (load_px_quad): the 4 columns of a vertical band (one thread per row; pixel j -> line j,
    // d1 = y) or 4 consecutive pixels of a horizontal band's line (one thread per quad; pixel j -> line ld, d1 = x + j)
    auto put_quad = [&](size_t g, int ld0, int d10, int ld_step, int d1_step) {
        const PxQuad q = load_px_quad<RGB, ALPHA>(fi_map, rgb_map, alpha_map, g_rgb, g_alpha, g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            put(ld0 + j * ld_step, d10 + j * d1_step, q.fi[j], q.al[j], q.ga[j], q.rr[3 * j], q.rr[3 * j + 1], q.rr[3 * j + 2], q.qq[3 * j],
                q.qq[3 * j + 1], q.qq[3 * j + 2]);
    };
    // one pixel: coalesced 4- and 12-byte loads
    auto put_one = [&](int ld, int d1, size_t g) {
        float al = 0, ga = 0, r = 0, gn = 0, bl = 0, gr = 0, gg = 0, gb = 0;
        if (ALPHA) { al = alpha_map[g]; ga = g_alpha[g]; }
        if (RGB) {
            r = rgb_map[3 * g]; gn = rgb_map[3 * g + 1]; bl = rgb_map[3 * g + 2];
            gr = g_rgb[3 * g]; gg = g_rgb[3 * g + 1]; gb = g_rgb[3 * g + 2];
        }
        put(ld, d1, fi_map[g], al, ga, r, gn, bl, gr, gg, gb);
    };
    if (axis && (S & 3) == 0) {  // a band line is an image row: thread -> (line, quad of 4 consecutive pixels)
        const int quads = S >> 2;
        for (int i = tid; i < nld * quads; i += NT) {
            const int ld = i / quads, x = (i - ld * quads) << 2;
            put_quad(img + (size_t)(band_lo + ld) * S + x, ld, x, 0, 1);
        }
    } else if (axis) {  // thread -> (line, x), x fastest (coalesced 4- and 12-byte loads)
        for (int i = tid; i < nld * S; i += NT) {
            const int ld = i / S, x = i - ld * S;
            put_one(ld, x, img + (size_t)(band_lo + ld) * S + x);
        }
    } else if (nld == 4 && (S & 3) == 0) {  // 4 adjacent columns: one thread per row
        for (int y = tid; y < S; y += NT) put_quad(img + (size_t)y * S + band_lo, 0, y, 1, 0);
    } else {  // generic columns: thread -> (row d1, line ld) with ld fastest
        for (int i = tid; i < nld * S; i += NT) {
            const int d1 = i / nld, ld = i - d1 * nld;
            put_one(ld, d1, img + (size_t)d1 * S + band_lo + ld);
        }
    }
}

// --------------------------------------------------------------------------------------------------
// Step 3 of k_bpm_fast: the sweeps of the n_win line records in s_line, one PIECE (<= FSEG pixels of one sweep) per thread
// and round.  Pieces are sorted into classes, each walked by its own loop:
//   U  exactly FSEG pixels of an OUT sweep, none of them covered by a face (7 of 8 pixels of an out sweep are background, and
//      they come in long runs behind the silhouette): `I - ref` is the constant (background - reference colour), the visit
//      reads the four gradients and nothing else; unrolled over its 15 pixels with compile-time LDS offsets;
//   M  exactly FSEG pixels of an OUT sweep between the first and the last covered pixel of the sweep (the coverage bits say
//      where): every pixel's colour is read as well -- an uncovered one holds the background colour (K5);
//   G  everything else: the pieces (<= FSEG pixels) of the in sweeps -- ownership test :707, per-pixel sign of `+- eps` -- and
//      the remainder of the out sweep, the general loop; short pieces (<= G_SHORT pixels) are numbered apart from long ones.
// Piece -> thread without a search: the thread that owns line `tid` of the window classifies the line's pieces (coverage
// bits of the band, px.cov), one packed scan numbers the pieces of each class through (U first, then M, then G, every class
// starting on a multiple of 64 so that a wave never mixes classes), the owners write a (line | piece << 8) descriptor per
// piece into a queue, and after one barrier every thread walks the ids tid, tid + 512, ... of the queue.  The queue takes
// what the line window leaves of the workgroup's LDS (fast_band_config: ~2500 descriptors, a window's worth); a window with
// more pieces goes through it in rounds.  (The binary search over the lines' prefix sums that this replaced in round 3 cost
// ~100 instructions and 9 dependent LDS round trips per piece.)
// The two sums of a piece go to acc[2 * line + k] (ds_add_f64), k = 0 / 1 for the edge's first / second vertex.
//
// Arithmetic of a visit (rasterize.py:630-657 out sweep, :697-728 in sweep) by MODE:
//   K6_FAST   diff = sum_c (I_c - ref_c) * g_c in the reference's order, accumulated with fused multiply-adds; dist =
//      fma(c * 2/S, t, +-eps) in float, the sign of `+- eps` taken once per piece in U / M (t = d1 - d1_cross keeps its sign
//      beyond the crossing point, hence so do c0 * t and c1 * t, :650 / :655); diff * v_rcp_f32(dist); float sums over the
//      <= 15 terms of a piece and over the <= 16 pieces of a run of lanes, double from there on.  No branch in U / M:
//      dm = diff <= 0 ? 0 : diff (:647: a NaN diff is not `<= 0` and goes through).  nr_k6_tune.h holds the knobs.
//   K6_EXACT*   the reference's operations one by one (products and sums rounded separately, `x * 2. / is` and `dist +- eps`
//      in double as its literals make them, IEEE division), every sum in double.
// When a contribution is not taken (:648 / :653: d0 equals the vertex) its coefficient is +-Inf / NaN; the lane then
// accumulates garbage that is discarded after the loop (no per-visit test of the has0 / has1 flags).
static_assert(FSEG % k6::FB == 0, "batches must tile a piece");

// One pixel's four floats out of LDS as ONE 16-byte read.  In the colour-only instantiation the alpha slot is never used and the
// compiler narrows the load to ds_read2_b32 + ds_read_b32 (two LDS instructions at 4-byte granularity per pixel: that instance
// ran 15 % slower than the one that also handles alpha); keeping the first component formally alive keeps the b128 form.
__device__ __forceinline__ float4 lds_px4(const float *p)
{
    float4 v = *reinterpret_cast<const float4 *>(p);
    asm volatile("" : "+v"(v.x));
    return v;
}
constexpr int G_SHORT = 4;  // class G pieces up to this many pixels are numbered apart from the longer ones

// DPP moves inside a row of 16 lanes: value of the lane D places below / one place above; a lane without such a neighbour
// in its row, or whose neighbour is not executing, gets `old`
template <int D>
__device__ __forceinline__ int dpp_row_shr(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x110 + D, 0xf, 0xf, false); }
template <int D>
__device__ __forceinline__ float dpp_row_shr_v(float v)  // (0 where there is no such neighbour)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + D, 0xf, 0xf, false));
}
template <int D>
__device__ __forceinline__ double dpp_row_shr_v(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x110 + D, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x110 + D, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int dpp_row_shl1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x101, 0xf, 0xf, false); }

// The pieces of one line sit on neighbouring lanes (consecutive ids), and all of them add to the same two sums: 64 lanes on
// ~10 addresses make the LDS serialise an atomic per lane.  So the sums of each run of equal keys are formed with DPP moves
// first (a segmented scan inside the 16-lane rows; a run that crosses a row is flushed in two parts); on return only the last
// lane of a run holds a non-zero pair.  In float for the tolerance mode (<= 16 piece sums, a tree of depth 4; in double the
// moves and selects come in pairs: stage 249 vs 239 us at raster 256 in round 3), in double for the exact one.  Which pieces
// share a run depends on the order of the line records, so two calls of the tolerance mode agree to ~1e-6 of the largest
// gradient, not to the bit.  (All 64 lanes execute this: the id loop keeps the wave together.)
template <typename T>
__device__ __forceinline__ void run_sums(int key, T &p0, T &p1)
{
    const int k1 = dpp_row_shr<1>(-1, key), k2 = dpp_row_shr<2>(-1, key), k4 = dpp_row_shr<4>(-1, key),
              k8 = dpp_row_shr<8>(-1, key);
    T q0 = dpp_row_shr_v<1>(p0), q1 = dpp_row_shr_v<1>(p1);
    if (k1 == key) { p0 += q0; p1 += q1; }
    q0 = dpp_row_shr_v<2>(p0); q1 = dpp_row_shr_v<2>(p1);
    if (k2 == key) { p0 += q0; p1 += q1; }
    q0 = dpp_row_shr_v<4>(p0); q1 = dpp_row_shr_v<4>(p1);
    if (k4 == key) { p0 += q0; p1 += q1; }
    q0 = dpp_row_shr_v<8>(p0); q1 = dpp_row_shr_v<8>(p1);
    if (k8 == key) { p0 += q0; p1 += q1; }
    if (dpp_row_shl1(-1, key) == key) p0 = p1 = T(0);  // not the last lane of its run
}

// exclusive scan of one 64-bit word of four 16-bit counters per thread over the workgroup (no field overflows: every total
// is below 2^16); returns the exclusive prefix, *total = sum.  The two halves are scanned as ints with DPP moves: the LDS is
// the busiest unit of this kernel and a shuffle-based scan would go through its crossbar twelve times.
template <int NT>
__device__ __forceinline__ unsigned long long block_excl_scan64(unsigned long long v, unsigned long long *s_tmp,
                                                                unsigned long long *total)
{
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const int ilo = wave_incl_scan_dpp(lo), ihi = wave_incl_scan_dpp(hi);
    const unsigned long long inc = (unsigned long long)(unsigned)ilo | ((unsigned long long)(unsigned)ihi << 32);
    return block_excl_scan<NT>(v, inc, s_tmp, total);
}

template <bool RGB, bool ALPHA, int MODE, int NT>
__device__ __forceinline__ void fast_sweeps(const FastPx &px, const BandLine *s_line, int n_win, int SP, double eps, int S,
                                            double *acc, void *s_queue, int qcap, bool wide, unsigned long long *s_tmp)
{
    constexpr bool EXACT = MODE != K6_FAST;
    constexpr int FB = k6::FB;
    const int tid = threadIdx.x;
    // ---- owner of line `tid`: its pieces by class.  The covered pixels of an out sweep lie next to the edge it starts
    // from (the rest of the object), the background behind them: the full pieces from the one with the first covered pixel
    // to the one with the last are class M (pmin .. pmin + nM - 1; an uncovered gap between two covered stretches -- the
    // teapot's handle -- rides along), the others class U.  One pass over the line's coverage words finds both ends.
    int nF = 0, nM = 0, nG = 0, nS = 0, pmin = 0, nIn = 0, rin = 0, rem = 0;
    // (Owners are the first n_win threads.  Spreading them over all eight waves -- 24 lanes each instead of three full waves --
    // was measured and is slower, 261 vs 240 us: every LDS instruction of a sparsely filled wave costs the LDS what a full one
    // does, and the LDS is the unit these loops wait for.)
    const int my_line = tid;
    const bool owner = tid < n_win;
    if (owner) {
        const int in_rng = s_line[my_line].in_rng, out_rng = s_line[my_line].out_rng, geo = s_line[my_line].geo;
        const int il = (in_rng >> 16) - (in_rng & 0xffff) + 1, out_from = out_rng & 0xffff;
        const int ol = (out_rng >> 16) - out_from + 1;
        nF = ol > 0 ? ol / FSEG : 0;
        // class G pieces: nIn pieces of the in sweep (the last one rin pixels long) and the out remainder (rem pixels); the
        // short ones (<= G_SHORT pixels: nine in-sweeps in ten) are numbered apart from the long ones, so that the lanes of a
        // wave walk pieces of similar length
        nIn = il > 0 ? (il + FSEG - 1) / FSEG : 0;
        rin = il > 0 ? il - (nIn - 1) * FSEG : 0;
        rem = ol > 0 ? ol % FSEG : 0;
        nG = nIn + (rem > 0);
        nS = (rin > 0 && rin <= G_SHORT) + (rem > 0 && rem <= G_SHORT);
        if (nF > 0) {
            const int ld = (geo >> 16) & 0xff;
            const unsigned *cw = px.cov + ld * px.CW;
            // the pieces' pixels [out_from, last], clipped to the covered span of the band line
            const int last = out_from + nF * FSEG - 1;
            const int ca = max(out_from, px.span[2 * ld]), cb = min(last, px.span[2 * ld + 1]);
            // (four words per LDS read: the lines' word arrays start on 16 bytes and are padded to a multiple of four words)
            int cmin = 0x7fffffff, cmax = -1;
            if (ca <= cb) {
                for (int w4 = (ca >> 5) & ~3; w4 <= (cb >> 5); w4 += 4) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(cw + w4);
                    const unsigned qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int w = w4 + k;
                        unsigned m = qq[k];
                        if (w < (ca >> 5) || w > (cb >> 5)) m = 0u;
                        if (w == (ca >> 5)) m &= 0xffffffffu << (ca & 31);
                        if (w == (cb >> 5)) m &= 0xffffffffu >> (31 - (cb & 31));
                        if (m) {
                            cmin = min(cmin, 32 * w + __ffs((int)m) - 1);
                            cmax = max(cmax, 32 * w + 31 - __clz((int)m));
                        }
                    }
                }
            }
            if (cmax >= 0) {
                pmin = (cmin - out_from) / FSEG;
                nM = (cmax - out_from) / FSEG - pmin + 1;
            }
        }
    }
    // class U pieces travel in SUPER-PIECES of up to k6::U_GROUP consecutive pieces of one line (round 5): one descriptor, one
    // record decode and one flush for up to 45 pixels -- the pieces behind the silhouette come in long runs, and decode + flush
    // cost a piece about half of what its fifteen visits do.  The two runs of a line's U pieces (in front of its M pieces and
    // behind them) are grouped separately; a super-piece's count sits above its first piece number in the descriptor.
    // (tolerance mode only: with the exact mode's 62-slot visits the lanes of a wave that hold one piece wait three times as long
    // for those that hold three -- 342 -> 370 us)
    constexpr int UG = EXACT ? 1 : k6::U_GROUP;
    const int nUa = nF > 0 ? pmin : 0, nUb = nF - nM - nUa;  // U pieces in front of / behind the line's M pieces
    const int gUa = (nUa + UG - 1) / UG, gUb = (nUb + UG - 1) / UG;
    const int nU = gUa + gUb, nL = nG - nS;
    // one scan for the four numberings (16 bits each: a window holds < 2^16 pieces of every kind by the choice of win_lines)
    unsigned long long totals = 0;
    const unsigned long long offs = block_excl_scan64<NT>((unsigned long long)nU | ((unsigned long long)nM << 16) |
                                                          ((unsigned long long)nS << 32) | ((unsigned long long)nL << 48),
                                                      s_tmp, &totals);
    const int TU = (int)(totals & 0xffff), TM = (int)((totals >> 16) & 0xffff), TS = (int)((totals >> 32) & 0xffff),
              TL = (int)(totals >> 48);
    // class starts (multiples of 64): U at 0, M, G-short, G-long
    const int MA = (TU + 63) & ~63, SA = MA + ((TM + 63) & ~63), LA = SA + ((TS + 63) & ~63), total_ids = LA + TL;
    const int idU = (int)(offs & 0xffff), idM = MA + (int)((offs >> 16) & 0xffff), idS = SA + (int)((offs >> 32) & 0xffff),
              idL = LA + (int)(offs >> 48);
    unsigned short *q16 = reinterpret_cast<unsigned short *>(s_queue);
    unsigned *q32 = reinterpret_cast<unsigned *>(s_queue);
    // arithmetic constants of the mode
    const float eps_f = (float)eps;                                                      // K6_FAST
    const unsigned eps_hi = (unsigned)__double2hiint(eps), eps_lo = (unsigned)__double2loint(eps);  // K6_EXACT*
    const double s_d = (double)S;
    const float two_over_s_f = (float)(2.0 / (double)S);  // exact when S is a power of two
    // one term of the exact mode: :649-651 / :654-656 (x * 2. / S: an exact scaling when S is a power of two)
    auto exact_term = [&](float diff, float c, float t) {
        const float ct = c * t;
        float dist = MODE == K6_EXACT_POW2 ? ct * two_over_s_f : (float)((double)ct * 2.0 / s_d);
        dist = (float)((double)dist + signed_eps(dist, eps_hi, eps_lo));  // + eps when 0 < dist, - eps otherwise
        return diff / dist;
    };
    // rounds of qcap ids (qcap: a multiple of NT; most windows fit in one round)
    for (int lo = 0; lo < total_ids; lo += qcap) {
        const int hi = min(lo + qcap, total_ids);
        if (lo > 0) __syncthreads();  // the previous round's readers are done
        if (owner) {                  // descriptors (line | piece << 8) of this owner's pieces with ids in [lo, hi)
            auto put = [&](int id, int seg) {
                if (wide) q32[id - lo] = (unsigned)my_line | ((unsigned)seg << 8);
                else q16[id - lo] = (unsigned short)(my_line | (seg << 8));
            };
            for (int j = min(max(lo - idU, 0), nU), j1 = min(max(hi - idU, 0), nU); j < j1; ++j) {
                const int first = j < gUa ? j * UG : pmin + nM + (j - gUa) * UG;
                const int cnt = j < gUa ? min(UG, nUa - j * UG) : min(UG, nUb - (j - gUa) * UG);
                put(idU + j, first | ((cnt - 1) << (wide ? 22 : 6)));
            }
            for (int j = min(max(lo - idM, 0), nM), j1 = min(max(hi - idM, 0), nM); j < j1; ++j) put(idM + j, pmin + j);
            for (int j = 0, cs = 0, cl = 0; j < nG; ++j) {  // G piece j: in piece j (j < nIn) or the out remainder
                const int len = j < nIn - 1 ? FSEG : (j == nIn - 1 ? rin : rem);
                const int id = len <= G_SHORT ? idS + cs++ : idL + cl++;
                if (id >= lo && id < hi) put(id, j);
            }
        }
        __syncthreads();
        for (int id = lo + tid; rfl(id) < hi; id += NT) {  // (wave-uniform trip count: all 64 lanes stay together)
            const int wid = rfl(id);     // ids of a wave are 64 consecutive numbers from a multiple of 64: one class per wave
            const int cls = wid < MA ? 0 : (wid < SA ? 1 : 2);
            const int cls_end = min(hi, cls == 0 ? TU : (cls == 1 ? MA + TM : (wid < LA ? SA + TS : total_ids)));
            if (wid >= cls_end) continue;  // a wave of padding ids
            // a lane on a padding id behind its class walks piece 0 of line 0 (valid LDS addresses) and throws the result away
            const bool valid = id < cls_end;
            const unsigned desc = valid ? (wide ? q32[id - lo] : (unsigned)q16[id - lo]) : 0u;
            const int line = (int)(desc & 0xffu);
            int seg = (int)(desc >> 8), u_cnt = 1;
            if (cls == 0) {  // a super-piece of class U: count - 1 above the first piece number
                u_cnt = (wide ? (seg >> 22) : (seg >> 6)) + 1;
                seg &= wide ? 0x3fffff : 63;
            }
            const BandLine *L = &s_line[line];
            const int4 h = *reinterpret_cast<const int4 *>(L);
            const float4 c = *reinterpret_cast<const float4 *>(&L->cross);
            const int flags = (h.z >> 24) & 0xff;
            const int ld = (h.z >> 16) & 0xff, base = ld * SP;
            const int d1_in = h.z & 0xffff;
            const int out_from = h.y & 0xffff, out_to = h.y >> 16;
            // class G: which sweep and which pixels
            bool mode_in = false;
            int s_from = out_from + seg * FSEG, s_to = s_from + FSEG - 1;
            if (cls == 2) {
                const int in_from = h.x & 0xffff, in_to = h.x >> 16;
                const int il = in_to - in_from + 1;
                const int n_in = il > 0 ? (il + FSEG - 1) / FSEG : 0;
                mode_in = seg < n_in;
                if (mode_in) { s_from = in_from + seg * FSEG; s_to = min(s_from + FSEG - 1, in_to); }
                else { s_from = out_from + ((out_to - out_from + 1) / FSEG) * FSEG; s_to = out_to; }
            }
            // reference colour: the OUT sweep compares with the in pixel, the IN sweep with the out pixel
            const int lref = base + (mode_in ? d1_in + ((flags & 8) ? 1 : -1) : d1_in);
            float ra = 0.0f, rr = 0.0f, rg = 0.0f, rb = 0.0f;
            float ba = 0.0f, br = 0.0f, bgn = 0.0f, bb = 0.0f;  // colour of an uncovered pixel
            if (RGB) {
                const float4 q = *reinterpret_cast<const float4 *>(px.c + 4 * (size_t)lref);
                ra = q.x; rr = q.y; rg = q.z; rb = q.w;
                const float4 w = *reinterpret_cast<const float4 *>(px.bg);
                ba = w.x; br = w.y; bgn = w.z; bb = w.w;
            } else {
                ra = px.c[lref];
                ba = px.bg[0];
            }
            // diff = sum_c (I_c - ref_c) * g_c with the reference's operations in its order (:631-638 / :709-716; its leading
            // `0 +` only turns a -0 into +0, which no later step can tell apart).  An uncovered pixel has the background colour
            // (K5), whose difference to the reference colour is a constant of the piece.
            const float dba = ba - ra, dbr = br - rr, dbg = bgn - rg, dbb = bb - rb;
            const float cross = c.x, c0k = c.y, c1k = c.z;
            const int fnr = __float_as_int(c.w);
            // (tolerance mode: the dot product as fused multiply-adds -- 19 -> 13 VALU instructions per uncovered pixel with
            // the fused `c * t + eps` below, 23 -> 17 per covered one; `diff <= 0` may then decide differently from :647 where
            // diff is within ~3 roundings of 0, about a term of the size of a rounding.  The exact mode keeps the products and
            // sums apart.)
            // [fast-diff] bg_diff / own_diff: the colour difference, one product and three fused multiply-adds
            auto bg_diff = [&](const float4 &g4, float ga) {
                if (!RGB) return dba * ga;
                float d;
                if constexpr (!EXACT) {
                    d = ALPHA ? __builtin_fmaf(dbr, g4.y, dba * g4.x) : dbr * g4.y;
                    d = __builtin_fmaf(dbg, g4.z, d);
                    d = __builtin_fmaf(dbb, g4.w, d);
                } else {
                    d = ALPHA ? dba * g4.x + dbr * g4.y : dbr * g4.y;
                    d += dbg * g4.z;
                    d += dbb * g4.w;
                }
                return d;
            };
            auto own_diff = [&](const float4 &c4, float ca, const float4 &g4, float ga) {  // c4 / ca: the pixel's colour
                if (!RGB) return (ca - ra) * ga;
                float d;
                if constexpr (!EXACT) {
                    d = ALPHA ? __builtin_fmaf(c4.y - rr, g4.y, (c4.x - ra) * g4.x) : (c4.y - rr) * g4.y;
                    d = __builtin_fmaf(c4.z - rg, g4.z, d);
                    d = __builtin_fmaf(c4.w - rb, g4.w, d);
                } else {
                    d = ALPHA ? (c4.x - ra) * g4.x + (c4.y - rr) * g4.y : (c4.y - rr) * g4.y;
                    d += (c4.z - rg) * g4.z;
                    d += (c4.w - rb) * g4.w;
                }
                return d;
            };
            // the piece's two sums: double in the exact mode, float otherwise
            typename std::conditional<EXACT, double, float>::type f0 = 0, f1 = 0;
            if (cls < 2) {
                // ---- U / M: FSEG pixels of an out sweep, unrolled; one address register per array, compile-time offsets
                const int l0 = base + s_from;
                const float d1f0 = (float)s_from;
                const float t_first = d1f0 - cross;
                const float e0 = (0.0f < c0k * t_first) ? eps_f : -eps_f, e1 = (0.0f < c1k * t_first) ? eps_f : -eps_f;
                const float *gp = px.g + (RGB ? 4 : 1) * (size_t)l0, *cp = px.c + (RGB ? 4 : 1) * (size_t)l0;
                // One visit without a branch: the visits of a batch are independent instruction chains that the scheduler
                // interleaves.  Tolerance mode: y is never 0 (x and its eps have one sign), so the reciprocal is finite
                // wherever the contribution is taken (:648 / :653) and 0 * it adds nothing.
                // d1fb: t of the piece's first pixel (tolerance mode, dist = fma(c, t, +-eps): pixel k has t_first + k, both
                // of one sign: no cancellation) or its d1 (exact mode).  It is re-declared opaque per batch below: that keeps
                // the compiler from computing all FSEG values of t ahead of the loop, which costs a register each and pushed
                // the kernel into spilling.
                float d1fb = EXACT ? d1f0 : t_first;  // [fast-t] t = (d1 - cross) + k: here and in visit, two roundings of one sign
                auto visit = [&](float diff, int k) {
                    if constexpr (EXACT) {
                        const float t = (d1fb + (float)k) - cross;
                        const float q0 = exact_term(diff, c0k, t), q1 = exact_term(diff, c1k, t);
                        const bool skip = diff <= 0.0f;                            // :647 (a NaN diff goes through)
                        f0 -= (double)(skip ? 0.0f : q0);                          // :651
                        f1 -= (double)(skip ? 0.0f : q1);                          // :656
                    } else {
                        const float dm = (diff <= 0.0f) ? 0.0f : diff;
                        const float t = d1fb + (float)k;
                        const float y0 = __builtin_fmaf(c0k, t, e0), y1 = __builtin_fmaf(c1k, t, e1);  // :649-650 / :654-655
                        // [fast-rcp] v_rcp_f32 without a Newton step, the term added to the piece's float sum
                        f0 = __builtin_fmaf(-dm, __builtin_amdgcn_rcpf(y0), f0);                      // :651
                        f1 = __builtin_fmaf(-dm, __builtin_amdgcn_rcpf(y1), f1);                      // :656
                    }
                };
                if (cls == 0) {
                    // U: gradients only; the next batch's LDS reads are in flight while this one is evaluated.  The pieces of a
                    // super-piece one after the other: each piece's sums in a float of their own, added up like the run sums do
                    for (int u = 0; u < u_cnt; ++u) {
                    const auto p0 = f0, p1 = f1;
                    f0 = 0;
                    f1 = 0;
                    float4 gc[FB], gn[FB];
                    float ac[FB], an[FB];
#pragma unroll
                    for (int j = 0; j < FB; ++j) {
                        gc[j] = gn[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        ac[j] = an[j] = 0.0f;
                        if (RGB) gc[j] = lds_px4(gp + 4 * j);
                        else ac[j] = gp[j];
                    }
#pragma unroll
                    for (int kb = 0; kb < FSEG; kb += FB) {
                        asm volatile("" : "+v"(d1fb));
                        if (kb + FB < FSEG) {
#pragma unroll
                            for (int j = 0; j < FB; ++j) {
                                if (RGB) gn[j] = lds_px4(gp + 4 * (kb + FB + j));
                                else an[j] = gp[kb + FB + j];
                            }
                        }
#pragma unroll
                        for (int j = 0; j < FB; ++j) visit(bg_diff(gc[j], ac[j]), kb + j);
#pragma unroll
                        for (int j = 0; j < FB; ++j) { gc[j] = gn[j]; ac[j] = an[j]; }
                        __builtin_amdgcn_sched_barrier(0);  // (keeps the scheduler from hoisting every batch's reads to the top)
                    }
                    f0 += p0;
                    f1 += p1;
                    gp += (RGB ? 4 : 1) * FSEG;
                    d1fb += (float)FSEG;
                    }
                } else {
                    // M: every pixel's colour as well -- an uncovered one holds the background colour (K5), so the same
                    // expression serves both
#pragma unroll
                    for (int kb = 0; kb < FSEG; kb += FB) {
                        asm volatile("" : "+v"(d1fb));
                        float4 g4[FB], c4[FB];
                        float ga[FB], ca[FB];
#pragma unroll
                        for (int j = 0; j < FB; ++j) {
                            g4[j] = c4[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                            ga[j] = ca[j] = 0.0f;
                            if (RGB) {
                                g4[j] = lds_px4(gp + 4 * (kb + j));
                                c4[j] = lds_px4(cp + 4 * (kb + j));
                            } else {
                                ga[j] = gp[kb + j];
                                ca[j] = cp[kb + j];
                            }
                        }
#pragma unroll
                        for (int j = 0; j < FB; ++j) visit(own_diff(c4[j], ca[j], g4[j], ga[j]), kb + j);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
                // ---- G: a piece of an in sweep or the remainder of an out sweep, the general loop
                const int own_mask = mode_in ? -1 : 0;
                float d1f = (float)s_from;
                float b0 = 0.0f, b1 = 0.0f;
                for (int l = base + s_from; l <= base + s_to; ++l, d1f += 1.0f) {
                    // face index, gradients and colour are requested together (one LDS round trip)
                    const int fi = px.fi[l];
                    float4 g4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c4 = g4;
                    float ga = 0.0f, ca = 0.0f;
                    if (RGB) { g4 = lds_px4(px.g + 4 * (size_t)l); c4 = lds_px4(px.c + 4 * (size_t)l); }
                    else { ga = px.g[l]; ca = px.c[l]; }
                    const float diff = own_diff(c4, ca, g4, ga);  // (an uncovered pixel holds the background colour)
                    // :707 (only the in sweep tests ownership) and :647 / :717 (a NaN diff is not `<= 0`), without divergent
                    // control flow on the sweep kind
                    if ((((fi ^ fnr) & own_mask) != 0) | (diff <= 0.0f)) continue;
                    const float t = d1f - cross;
                    if constexpr (EXACT) {
                        f0 -= (double)exact_term(diff, c0k, t);                               // :649-651
                        f1 -= (double)exact_term(diff, c1k, t);                               // :654-656
                    } else {
                        const float x0 = c0k * t, x1 = c1k * t;                               // :649 / :654 (2 / S folded into c)
                        const float y0 = x0 + ((0.0f < x0) ? eps_f : -eps_f);                 // :650 / :655
                        const float y1 = x1 + ((0.0f < x1) ? eps_f : -eps_f);
                        b0 = __builtin_fmaf(-diff, __builtin_amdgcn_rcpf(y0), b0);            // :651
                        b1 = __builtin_fmaf(-diff, __builtin_amdgcn_rcpf(y1), b1);            // :656
                    }
                }
                if constexpr (!EXACT) { f0 += b0; f1 += b1; }
            }
            // :648 / :653: a contribution whose vertex sits on the line is not taken (its coefficient was Inf / NaN)
            using RunT = typename std::conditional<EXACT, double, float>::type;
            RunT p0 = (valid && (flags & 2)) ? (RunT)f0 : RunT(0), p1 = (valid && (flags & 4)) ? (RunT)f1 : RunT(0);
            const int key = valid ? line : -1 - (tid & 63);  // (a padding lane: a run of its own)
            run_sums(key, p0, p1);
            const double a0 = (double)p0, a1 = (double)p1;
            if (a0 != 0.0) atomicAdd(&acc[2 * line], a0);
            if (a1 != 0.0) atomicAdd(&acc[2 * line + 1], a1);
        }
    }
}

// The band kernel, NT threads per workgroup (band_shape below).  (launch bounds: what the LDS of a shape admits -- six waves
// per SIMD for three 512-thread workgroups per CU, four for four 256-thread ones; the generic exact form carries a double
// division: four)
// (the kernel's body as a function: the overflow-only form also runs on the first workgroups of k_big_overflow's launch.  block,
// n_blocks: the workgroup's number among the n_blocks that run the body -- blockIdx.x and gridDim.x of k_bpm_fast.  Returns whether
// the workgroup walked bands as part of an overflow pass, i.e. found an image over the line buffer.)
// (The inputs one by one: `__restrict__` works on a function's parameters only, and with one argument struct, read in the body or passed
// by value to the kernel, the 512-thread instances' scratch grew -- 84 -> 100 bytes in k_bpm_fast<true, true, 0, 512, true>.)
template <bool RGB, bool ALPHA, int MODE, int NT, bool OVF>
__device__ __forceinline__ bool bpm_fast_body(
    const float *__restrict__ faces, const int32_t *__restrict__ fi_map, const float *__restrict__ rgb_map,
    const float *__restrict__ alpha_map, const float *__restrict__ g_rgb, const float *__restrict__ g_alpha,
    const int *__restrict__ vis_list, const int *__restrict__ vis_count, const unsigned *__restrict__ rng,
    double *__restrict__ scratch, const int *__restrict__ band_lines, const int *__restrict__ band_start,
    const int *__restrict__ lines_ok, const BandLine *__restrict__ line_buf, size_t cap, int F, int S, int W, int SP,
    double eps, float k2s, int B, int win_lines, int qcap, uint4 *__restrict__ zero16, size_t n_zero16, const unsigned block,
    const unsigned n_blocks)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    // XCD-aware placement (nr_device.h): bands of one image share cache lines -- 8 adjacent 4-column bands sit in the same
    // 128-byte line of every map row, and the horizontal pass re-reads what the vertical pass just fetched -- so all
    // 2 * n_bands workgroups of an image are given ids that land on ONE XCD (one L2).  Measured in round 1: 613 -> 477 us.
    // (The same mapping on the forward and gather kernels changed nothing or cost 5 %: their reads are not shared.)
    const unsigned n_bands = (unsigned)(S + W - 1) / (unsigned)W;
    const unsigned total_wg = n_bands * 2u * (unsigned)B;
    // OVF: the launch behind k_bpm_row that serves the images whose records exceed the line buffer -- normally none -- by the scan
    // path: a small grid whose workgroups first take one cooperative look at the images' verdicts (none over the buffer: leave)
    // and otherwise walk the bands in strides.  (An instantiation of its own: with the band loop around it the ordinary kernel
    // came out at 116 registers instead of 89 and 7 % slower.)
    constexpr bool overflow_only = OVF;
    auto band_body = [&](const unsigned logical) {
    if (n_zero16) {
        // The fused backward's zero fill of grad_textures (the K7 gather behind this kernel stores only the listed faces'
        // cubes) rides along: every workgroup clears one slice before it looks at its band -- half of them have nothing
        // else to do -- instead of a launch of its own between this kernel and the gather.
        const size_t per = (n_zero16 + total_wg - 1) / total_wg, z_lo = (size_t)logical * per, z_hi = min(n_zero16, z_lo + per);
        for (size_t k = z_lo + tid; k < z_hi; k += NT) zero16[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    const int band = (int)(logical % n_bands), axis = (int)((logical / n_bands) & 1u), b = (int)(logical / (2u * n_bands));
    const int band_lo = band * W, band_hi = min(band_lo + W, S) - 1;
    const int nld = band_hi - band_lo + 1;
    const size_t bidx = ((size_t)b * 2 + axis) * n_bands + band;
    // overflow_only: this launch stands behind k_bpm_row and serves only the images whose records exceed the line buffer, by the
    // scan path; the band tables are k_bpm_row's (per line), not this kernel's shape
    if (overflow_only && lines_ok[b] != 0) return;
    const int n_band_lines = overflow_only ? 1 : band_lines[bidx];
    if (n_band_lines == 0) return;  // step 0: no visible face has a line here

    size_t off = 0;
    auto carve = [&](size_t bytes) { unsigned char *p = smem + off; off += (bytes + 15) & ~(size_t)15; return p; };
    constexpr int NC = RGB ? 4 : 1;  // floats per pixel in the gradient / colour arrays: (alpha, r, g, b) or alpha alone
    FastPx px;
    px.fi = (int *)carve((size_t)W * SP * 4);
    px.g = (float *)carve((size_t)W * SP * NC * 4);
    px.c = (float *)carve((size_t)W * SP * NC * 4);
    px.bg = (float *)carve(16);
    px.CW = (((SP + 31) >> 5) + 3) & ~3;  // words per line, a multiple of four (16-byte reads of the classification)
    px.cov = (unsigned *)carve((size_t)W * px.CW * 4);
    px.span = (int *)carve(4 * 2 * 4);  // (W <= 4 lines)
    const bool wide = S > 63 * FSEG;  // piece numbers beyond 6 bits (two more carry a class-U super-piece's count): 32-bit descriptors
    // The rest of the workgroup's LDS is split between the line window (32 B record + two double sums per line) and the piece
    // queue by the host (fast_band_config).  (A per-band split inside the kernel -- equal windows, as few as let a window's
    // pieces through the queue in one round -- was measured and lost to the fixed split, 258 vs 242 us: it trades windows of
    // 224 lines with two rounds for twice as many windows.)
    BandLine *s_line = (BandLine *)carve(sizeof(BandLine) * win_lines);
    double *s_lacc = (double *)carve(16 * (size_t)win_lines);  // [win_lines][2] sums of each line for its edge's two vertices
    void *s_queue = carve((size_t)qcap * (wide ? 4 : 2));     // piece descriptors of a window (or of a round of it)
    int *s_tmp = (int *)carve(4 * 16);

    // ---- 1. stage the band
    const size_t img = (size_t)b * S * S;
    for (int i = tid; i < W * px.CW; i += NT) px.cov[i] = 0u;
    __syncthreads();
    fast_stage<RGB, ALPHA, NT>(px, fi_map, rgb_map, alpha_map, g_rgb, g_alpha, img, axis, band_lo, nld, S, SP);
    __syncthreads();
    if (tid < nld) {  // covered span of each band line (the sweeps' classification looks no further)
        int first = 0x7fffffff, last = -1;
        for (int w = 0; w < px.CW; ++w) {
            const unsigned m = px.cov[tid * px.CW + w];
            if (m) { first = min(first, 32 * w + __ffs((int)m) - 1); last = 32 * w + 31 - __clz((int)m); }
        }
        px.span[2 * tid] = first;
        px.span[2 * tid + 1] = last;
    }

    // ---- 2. - 4. window by window.  Records path: the band's line records were written by k_line_setup.  Scan path (an image
    // with more lines than the record buffer holds, or NR_FLAG_K6_SCAN): the image's visible faces are scanned in chunks of
    // one face per thread and the lines of the chunk that fall into this band are set up in place.  The scan path keeps
    // nothing in registers across the sweeps -- it recomputes its chunk's line counts for every window -- so that the kernel's
    // register budget is the records path's.
    const bool use_rec = !overflow_only && lines_ok[b] != 0;
    const BandLine *recs = line_buf + (size_t)b * cap + (use_rec ? band_start[bidx] : 0);
    const int n_vis = use_rec ? 0 : vis_count[b];
    const unsigned *rng_ba = rng + ((size_t)b * 2 + axis) * F * 3;
    int chunk = 0, win = 0;  // (scan path) first list position of the chunk; (both) first line of the next window
    // the 2 * n_win line sums, one or two per thread (a window has at most NT lines)
    auto each_sum = [&](int n2, auto fn) {
        if (tid < n2) fn(tid);
        if (NT < 2 * BAND_WIN && tid + NT < n2) fn(tid + NT);
    };
    for (;;) {
        int n_win;
        if (use_rec) {
            if (win >= n_band_lines) break;
            n_win = min(n_band_lines - win, win_lines);
            if (tid < n_win) s_line[tid] = recs[win + tid];  // (win_lines <= NT)
            each_sum(2 * n_win, [&](int i) { s_lacc[i] = 0.0; });
            win += win_lines;
        } else {
            if (chunk >= n_vis) break;
            // one visible face per thread: lines of its 3 edges inside the band
            int nl = 0;
            int e_lo[3] = {0, 0, 0}, e_n[3] = {0, 0, 0};
            if (chunk + tid < n_vis) {
                const unsigned *r = rng_ba + (size_t)(chunk + tid) * 3;
#pragma unroll
                for (int e = 0; e < 3; e++) {
                    const unsigned pr = r[e];
                    const int lo = max((int)(pr & 0xffffu), band_lo), hi = min((int)(pr >> 16), band_hi);
                    if (hi >= lo) { e_lo[e] = lo; e_n[e] = hi - lo + 1; nl += e_n[e]; }
                }
            }
            int total_lines = 0;
            const int line_off = block_excl_scan<NT>(nl, wave_incl_scan(nl, (int)(threadIdx.x & 63)), s_tmp, &total_lines);
            if (win >= total_lines) {  // (uniform) this chunk is done
                chunk += NT;
                win = 0;
                continue;
            }
            n_win = min(total_lines - win, win_lines);
            // (list position | edge << 28, line) of the window's lines, parked where the line sums will be
            int2 *s_rec = reinterpret_cast<int2 *>(s_lacc);
            if (nl > 0 && line_off < win + win_lines && line_off + nl > win) {
                int k = line_off;
#pragma unroll
                for (int e = 0; e < 3; e++)
                    for (int j = 0; j < e_n[e]; j++, k++)
                        if (k >= win && k < win + win_lines) s_rec[k - win] = make_int2((chunk + tid) | (e << 28), e_lo[e] + j - band_lo);
            }
            __syncthreads();
            int2 rec = make_int2(0, 0);
            if (tid < n_win) rec = s_rec[tid];
            __syncthreads();
            if (tid < n_win) {  // line setup, one line per thread
                const int pos = rec.x & 0x0fffffff, e = (rec.x >> 28) & 3, ld = rec.y;
                const int rfn = vis_list[(size_t)b * F + pos];
                s_line[tid] = make_fast_line(faces + ((size_t)b * F + rfn) * 9, e, axis, band_lo + ld, ld, S, rfn,
                                             pos | (e << 28) | (((e + 1) % 3) << 30),
                                             [&](int d1) { return px.fi[ld * SP + d1]; }, k2s);
            }
            each_sum(2 * n_win, [&](int i) { s_lacc[i] = 0.0; });
            win += win_lines;
        }
        __syncthreads();
        fast_sweeps<RGB, ALPHA, MODE, NT>(px, s_line, n_win, SP, eps, S, s_lacc, s_queue, qcap, wide,
                                      reinterpret_cast<unsigned long long *>(s_tmp));
        __syncthreads();
        each_sum(2 * n_win, [&](int i) {  // line sums -> global double scratch [list position][vertex][x|y]
            const double a = s_lacc[i];
            if (a != 0.0) {
                const int tgt = s_line[i >> 1].tgt;
                const int pos = tgt & 0x0fffffff, v = (i & 1) ? (tgt >> 30) & 3 : (tgt >> 28) & 3;
                atomicAdd(scratch + ((size_t)b * F + pos) * 6 + 2 * v + (1 - axis), a);
            }
        });
        __syncthreads();
    }
    };
    if constexpr (!OVF) {
        const unsigned logical = xcd_block(total_wg);
        if (logical < total_wg) band_body(logical);
        return false;
    } else {
        int any = 0;
        for (int i = tid; i < B; i += NT) any |= lines_ok[i] == 0;
        if (!__syncthreads_or(any)) return false;
        for (unsigned logical = block; logical < total_wg; logical += n_blocks) {
            band_body(logical);
            __syncthreads();  // (the next band re-uses the LDS)
        }
        return true;
    }
}

template <bool RGB, bool ALPHA, int MODE, int NT, bool OVF = false>
__global__ __launch_bounds__(NT, MODE == K6_EXACT ? 4 : (NT == 256 ? k6::MINWAVES_256 : 6)) void k_bpm_fast(
    const float *__restrict__ faces, const int32_t *__restrict__ fi_map, const float *__restrict__ rgb_map,
    const float *__restrict__ alpha_map, const float *__restrict__ g_rgb, const float *__restrict__ g_alpha,
    const int *__restrict__ vis_list, const int *__restrict__ vis_count, const unsigned *__restrict__ rng,
    double *__restrict__ scratch, const int *__restrict__ band_lines, const int *__restrict__ band_start,
    const int *__restrict__ lines_ok, const BandLine *__restrict__ line_buf, size_t cap, int F, int S, int W, int SP,
    double eps, float k2s, int B, int win_lines, int qcap, uint4 *__restrict__ zero16, size_t n_zero16)
{
    bpm_fast_body<RGB, ALPHA, MODE, NT, OVF>(faces, fi_map, rgb_map, alpha_map, g_rgb, g_alpha, vis_list, vis_count, rng, scratch,
                                             band_lines, band_start, lines_ok, line_buf, cap, F, S, W, SP, eps, k2s, B, win_lines, qcap,
                                             zero16, n_zero16, blockIdx.x, gridDim.x);
}
