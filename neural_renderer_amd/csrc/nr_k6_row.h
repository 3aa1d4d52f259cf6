// nr_k6_row.h -- k_bpm_row, K6's band kernel for every call whose raster fits its band (both arithmetic modes), and
// k_band_gather, the same body with the K7 / K8 face gather's workgroups behind it in one grid.  Part of the translation unit
// nr_backward_pixel_map.hip (included there and nowhere else, behind nr_k6_lists.h and nr_k6_fast.h: signed_eps, lds_px4, and the
// images it leaves to k_bpm_fast's scan path).  The kernel's description stands in front of namespace rowk below.

// k_bpm_row: how many of a line's n_parts waves (a power of two) share one of its windows -- n_parts over the number of windows
// rounded up to a power of two, at least 1; lines of fewer than 32 segments (rasters below 481) keep a wave per window: their
// sweeps are too short for the members' repeated set-up to pay (64 views at 384^2: +1.7 % with teams, 512^2: -1.7 %)
__device__ __forceinline__ int window_team(int n_rec, int n_parts, int nsl)
{
    const int n_win = (n_rec + 63) >> 6;
    if (nsl < 32) return 1;
    int team = n_parts;
    while (team > 1 && n_parts / team < n_win) team >>= 1;
    return team;
}

// LDS hand-over between the lanes of ONE wave (its LDS operations execute in order; the fences keep the compiler from moving
// accesses across)
__device__ __forceinline__ void wave_lds_handover()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ==================================================================================================
// k_bpm_row (round 6): the band kernel of the default arithmetic mode.  A WAVE owns a band line, a BLOCK of 16 lanes a line
// record: four records per wave instruction.
//
// k_bpm_fast gives a lane a PIECE (15 pixels of one sweep) and walks it pixel by pixel out of LDS: every piece a descriptor, a
// record decode and a flush, every window a chain of barriers.  Round 5's k_bpm_px (gone) held a line's pixels in registers and
// visited ONE record at a time with all 64 lanes: 45 instructions of frame per record around its visits, and a sweep's last
// 64-lane chunk half empty.  Both ran at one third of the issued lanes useful.  Here:
//   * the band's pixels stay in LDS -- per pixel the four gradients g and ONE sum P = sum_c (I_c - K_c) g_c (formed in double at
//     the staging, rounded once), 24 bytes with the face index: five workgroups per CU.  K is the colour of the line's first
//     pixel, i.e. the background almost always: the sum of a background pixel is then exactly 0, and any colour NEAR the line's
//     colours serves -- with K = 0 a scene whose background is as bright as its faces (every term the small difference of
//     large products) came out 3 ... 6e-4 off in round 5;
//   * a block reads 16 consecutive pixels of its line per step, in segments ALIGNED to 16 pixels;
//   * an out sweep runs from the crossing point to the image border (:607-609), so "inside the sweep" is the sign of
//     td = direction * (d1 - d1_cross), a value the visit needs anyway: no range arithmetic, and a block may start segments
//     before its sweep or run on behind it -- those lanes are masked by the same comparison;
//   * the records of a window (64: a lane each in phase A) are SORTED by their number of segments (a counting sort in LDS) and
//     dealt to the blocks four at a time: the blocks of a group walk (nearly) the same number of steps (lane efficiency 0.89 at
//     raster 256, 0.92 at 512: scripts/row_stats.py), so the group is one loop with a uniform trip count and ONE reduction for
//     four records;
//   * that reduction is the matrix pipe's: a block is the 16 lanes of one block of v_mfma_f64_4x4x4_4b_f64 -- lanes
//     4 b .. 4 b + 3 of each of the wave's four rows -- and two of these instructions with a matrix of ones add up a block's 16
//     values in DOUBLE (the first contracts over the rows, the second over the four lanes), the sum arriving in every lane of
//     the block: no DPP tree in float (whose roundings of the TOTALS cost dense meshes a factor two in the error level),
//     no LDS atomics, and the vector pipe issues 4 conversions instead of 16 operations;
//   * a block's pixel quads are dealt to its four rows so that the 16-byte LDS reads stay conflict-free whatever segments the
//     four blocks are at (the LDS serves lanes {0-3, 12-15, 20-27}, ... together: quad = (row + 2 (b >> 1)) mod 4);
//   * a record's constants reach its block by ds_bpermute_b32 from the lane that prepared them in phase A.
// A visit (:630-657): diff = P - sum_c (ref_c - K_c) g_c (four fused multiply-adds), dist = |c| |t| + eps for the two vertices
// (t = d1 - d1_cross keeps its sign along an out sweep, so sigma = sign(c) sign(t) is a property of the record: the magnitudes
// are summed, the sign goes on once, at the flush), two v_rcp_f32 (a quarter-rate instruction on this part: a third of the
// visit's issue time, scripts/dev/valu_rate_probe.hip), two fused multiply-adds: 15 vector operations and two LDS reads for up
// to 64 useful lanes.
// Phase A (a lane per record): the record, its two reference colours straight from the maps (the in and the out pixel,
// :594-601 / :697-700 -- no colours in LDS), its in sweep (:665-728; nine in ten are <= 4 pixels) in the same two-sum form --
// and the two pixels next to the crossing point, which carry a record's largest terms, in the reference's DIRECT form
// sum_c (I_c - ref_c) g_c: their colours are the two reference colours (error levels, direct / centred sums for them: config 4
// 4.6e-5 / 5.9e-5, headline 3.3e-5 / 4.1e-5).
// Flush: one lane per record adds in sweep + out sweep to the double scratch (global_atomic_add_f64), as k_bpm_fast does.
// Images whose records exceed the line buffer (lines_ok == 0) are left to k_bpm_fast's scan path (launched behind this kernel
// with overflow_only set).
namespace rowk {
constexpr int NT = 256, NW = NT / 64;  // threads / waves per workgroup
constexpr int WIN = 64;            // records per window (a lane each in phase A)
constexpr int SEG = 16;            // pixels per step of a block
constexpr int MAX_SEGS = 64;       // segments of a line, at most (raster <= 1024): the sort's keys
constexpr int IN_SEG = 16;        // float terms per double addition of an in sweep (a piece of k_bpm_fast holds 15)
constexpr int IN_BATCH = 4;       // pixels of an in sweep whose LDS reads are requested together
constexpr int MAX_PX = 1024;       // pixels of a band, at most
// LDS of a workgroup, for the npx = W * SP pixels of its band: gradients [W][SP][NC] | sums P [W][SP] (the exact mode: colours
// [W][SP][NC]) | face indices [W][SP] | K of the band's lines (not in the exact mode) | a window per wave
constexpr int K_BYTES = 4 * 16, WAVE_BYTES = WIN * 16;
template <bool RGB> __host__ __device__ constexpr size_t g_bytes(size_t npx) { return npx * (RGB ? 16 : 4); }
template <bool RGB, bool EXACT> __host__ __device__ constexpr size_t c_bytes(size_t npx) { return EXACT ? g_bytes<RGB>(npx) : npx * 4; }
template <bool RGB, bool EXACT> __host__ __device__ constexpr size_t lds_bytes(size_t npx)
{
    return g_bytes<RGB>(npx) + c_bytes<RGB, EXACT>(npx) + npx * 4 + (EXACT ? 0 : K_BYTES) + NW * WAVE_BYTES;
}
}  // namespace rowk

#ifdef NR_ROW_STATS  // development builds (scripts/row_stats.py): work counters of k_bpm_row
__device__ unsigned long long g_row_stats[8];
NR_API int nr_dev_row_stats(unsigned long long *out8)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_row_stats), sizeof(unsigned long long) * 8) != hipSuccess) return 1;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_row_stats), z, sizeof(z)) == hipSuccess ? 0 : 1;
}
#define NR_ROW_STAT(i, v) do { if (lane == 0) atomicAdd(&g_row_stats[i], (unsigned long long)(v)); } while (0)
// (the records of the first NR_ROW_DUMP_WINDOWS windows -- segments of the out sweep | direction << 8 | has an out sweep << 9 |
// valid << 10 -- for studies of the grouping on the host: scripts/row_groupings.py)
constexpr unsigned NR_ROW_DUMP_WINDOWS = 1u << 16;
__device__ unsigned g_row_dump_n;
__device__ unsigned g_row_dump[NR_ROW_DUMP_WINDOWS * 64];
NR_API int nr_dev_row_dump(unsigned *out, unsigned *n_windows)
{
    if (hipMemcpyFromSymbol(n_windows, HIP_SYMBOL(g_row_dump_n), sizeof(unsigned)) != hipSuccess) return 1;
    const unsigned n = *n_windows < NR_ROW_DUMP_WINDOWS ? *n_windows : NR_ROW_DUMP_WINDOWS, zero = 0;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_row_dump), (size_t)n * 64 * sizeof(unsigned)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_row_dump_n), &zero, sizeof(unsigned)) == hipSuccess ? 0 : 1;
}
#else
#define NR_ROW_STAT(i, v) ((void)0)
#endif

// MODE: K6_FAST -- the default arithmetic, as described above -- or K6_EXACT / K6_EXACT_POW2 (NR_FLAG_EXACT_GRADIENT): the same
// groups of four records, every term with the reference's own operations: sum_c (I_c - ref_c) g_c rounded product by product
// (the colours, not the centred sums, are staged: 36 bytes per pixel, four workgroups per CU), `x * 2. / is` and `dist +- eps` in
// double, IEEE division, every sum in double -- a lane adds its terms to double accumulators, the matrix pipe adds the lanes.
// A masked lane divides 0 by 1 (the select sits in front of the division: no 0 / 0, no Inf * 0).
// The kernel's body is a device function: k_bpm_row below runs it alone, k_band_gather runs it in front of the K7 / K8 gather's
// workgroups in one grid.  It takes its workgroup from xcd_block, i.e. from blockIdx.x: the band workgroups are the first ids
// of either grid.  UNLISTED: the zero fill that rides along spares the cubes of the listed faces (zero_slot: K6's face -> list
// position table, n_zero16 / zero_epf entries), which the gather of the same launch stores.
struct BandRowArgs {
    const int32_t *fi_map;
    const float *rgb_map, *alpha_map, *g_rgb, *g_alpha;  // the forward's maps and their upstream gradients
    double *scratch;                                      // [B][list position][3 vertices][x|y] sums
    const int *band_lines, *band_start, *lines_ok;        // the per-line tables and the images' verdicts (k_line_setup)
    const BandLine *line_buf;
    size_t cap;       // records per image in line_buf
    int F, S, W, B;   // W: lines per band
    float eps_f;
    double eps_d;
    uint4 *zero16;    // the zero fill that rides along: n_zero16 16-byte words ...
    size_t n_zero16;
    const int *zero_slot;  // ... UNLISTED: but those of the listed faces (zero_slot[word / zero_epf] >= 0)
    unsigned zero_epf;
    int CH;           // pixels per chunk of a line (read by the CHUNKED instantiations only)
};

// (The body and k_bpm_row take their inputs one by one: `__restrict__` works on a function's parameters only.  With the body reading
// the struct every instance came out with other registers -- 70 -> 76 VGPRs in k_bpm_row<false, true, 2, true> --, with k_bpm_row taking
// it by value the uniform loads of the band tables became vector loads.  k_band_gather hands its block's fields over one by one.)
template <bool RGB, bool ALPHA, int MODE, bool CHUNKED, bool UNLISTED>
__device__ __forceinline__ void bpm_row_body(
    const int32_t *__restrict__ fi_map, const float *__restrict__ rgb_map, const float *__restrict__ alpha_map,
    const float *__restrict__ g_rgb, const float *__restrict__ g_alpha, double *__restrict__ scratch,
    const int *__restrict__ band_lines, const int *__restrict__ band_start, const int *__restrict__ lines_ok,
    const BandLine *__restrict__ line_buf, size_t cap, int F, int S, int W, int CH, float eps_f, double eps_d, int B,
    uint4 *__restrict__ zero16, size_t n_zero16, const int *__restrict__ zero_slot, unsigned zero_epf)
{
    using namespace rowk;
    constexpr bool EXACT = MODE != K6_FAST;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = rfl(tid >> 6);
    // A workgroup takes a band of W lines and, of those lines, a CHUNK of CH pixels (all of them up to raster 512, half a line
    // above): the sweeps of a record are sums over pixels, so the part of a sweep inside each chunk can be summed by a
    // workgroup of its own -- every term is formed exactly as in an unchunked line (t = d1 - d1_cross from the pixel's position
    // along the whole line), the chunks' sums meet in the double atomics of the flush.  What it buys on rasters above 512:
    // two-line bands instead of one-line ones.  A band of COLUMNS is staged in pieces of W pixels per image row, and with
    // one-line bands 4 of every 64 bytes fetched were used: the column bands' staging was over half of the kernel at raster
    // 1024 (k_bpm_row with the bands of one axis only, without sweeps, 32 views: columns 545 us, rows 125).  What it costs: a
    // record is set up once per chunk its sweeps reach -- which is why the chunks are not shorter: quarter lines with four-line
    // bands stage the columns in 310 us instead of 545 and lose it all again (K6 stage, us, chunks of <= 1024 / 512 / 256 pixels:
    // 32 views at 1024^2 1015 / 960 / 1138, 4 views 204 / 181 / 206, 64 views at 512^2 512 / 512 / 547).
    // (CHUNKED = false: whole lines -- an instantiation of its own, because the chunk's offset as a run-time zero cost the
    // headline launch 1.4 %: K6 stage 166.0 -> 168.4 us)
    const unsigned n_bands = (unsigned)(S + W - 1) / (unsigned)W, n_ch = CHUNKED ? (unsigned)(S + CH - 1) / (unsigned)CH : 1u;
    const unsigned total_wg = n_bands * 2u * (unsigned)B * n_ch;
    const unsigned logical = xcd_block(total_wg);  // all bands of an image on one XCD (see k_bpm_fast)
    if (logical >= total_wg) return;
    if (n_zero16) {  // the fused backward's zero fill of grad_textures rides along (see k_bpm_fast)
        const size_t per = (n_zero16 + total_wg - 1) / total_wg, z_lo = (size_t)logical * per, z_hi = min(n_zero16, z_lo + per);
        for (size_t k = z_lo + tid; k < z_hi; k += NT) {
            if constexpr (UNLISTED) { if (zero_slot[k / zero_epf] >= 0) continue; }
            zero16[k] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const unsigned bandidx = logical / n_ch;  // (the chunks of a band next to each other: they read the same records)
    const int c0 = CHUNKED ? (int)(logical - bandidx * n_ch) * CH : 0, SL = CHUNKED ? min(CH, S - c0) : S;  // the chunk: pixels [c0, c0 + SL) of the band's lines
    const int band = (int)(bandidx % n_bands), axis = (int)((bandidx / n_bands) & 1u);
    int b = (int)(bandidx / (2u * n_bands));
    // xcd_block gives XCD x the images x B / 8 ... (x + 1) B / 8 - 1: neighbouring views, whose line records rise and fall together
    // (edge extents of the headline's 64 views: the eight XCDs hold 0.955 ... 1.025 of the mean).  In the merged launch, when the
    // batch is a multiple of 8 and at least 16, the images are dealt across instead -- XCD x takes x, x + 8, ... (0.998 ... 1.001):
    // all bands of an image still on one XCD, in the same order, neighbouring bands on neighbouring ids.  (k_bpm_row's own launch,
    // which NR_FLAG_SERIAL_BACKWARD takes, keeps the mapping.)
    if constexpr (UNLISTED && k6::ROW_DEAL_IMAGES) {
        const int q = B >> 3;
        if ((B & 7) == 0 && q >= 2) b = (b % q) * 8 + b / q;
    }
    if (lines_ok[b] == 0) return;  // records beyond the buffer: k_bpm_fast's scan path serves this image
    const int band_lo = band * W, nld = min(W, S - band_lo);
    const size_t lt = ((size_t)b * 2 + axis) * S + band_lo;  // the band's lines in the per-line tables (band width 1)
    int n_tot = 0;
    for (int l = 0; l < nld; ++l) n_tot += band_lines[lt + l];
    if (n_tot == 0) return;  // no visible face has a line here

    constexpr int NC = RGB ? 4 : 1;  // floats per pixel in the gradient array: (alpha, r, g, b) or alpha alone
    // a line's chunk in LDS: SP pixels, a multiple of 32 (an even number of segments); the pixels behind the chunk hold zeros.
    // From here on pixel positions along a line are LOCAL: 0 is the chunk's first pixel.
    const int SP = (SL + 31) & ~31, nsl = SP / SEG;
    const unsigned npx = (unsigned)(W * SP), G_BYTES = (unsigned)g_bytes<RGB>(npx), C_BYTES = (unsigned)c_bytes<RGB, EXACT>(npx), FI_BYTES = npx * 4u;
    float *const s_g = (float *)smem;                                  // [W][SP][NC] gradients
    float *const s_p = (float *)(smem + G_BYTES);                      // [W][SP] sum_c (I_c - K_c) g_c; exact mode: [W][SP][NC] colours
    int *const s_fi = (int *)(smem + G_BYTES + C_BYTES);               // [W][SP] face index
    float4 *const s_k = (float4 *)(smem + G_BYTES + C_BYTES + FI_BYTES);  // [W] K of each line: (alpha, r, g, b) (not in the exact mode)
    unsigned char *wave_mem = smem + G_BYTES + C_BYTES + FI_BYTES + (EXACT ? 0u : (unsigned)K_BYTES) + (unsigned)wave * WAVE_BYTES;
    double2 *acc = (double2 *)wave_mem;  // [WIN] a record's two out-sweep sums (magnitudes) ...
    int *hist = (int *)wave_mem;         // ... after the sort's counters are done with the same bytes
    const int n_parts = max(1, NW / W);  // (a band narrower than the workgroup has waves: they share the windows of a line)
    const BandLine *recs_b = line_buf + (size_t)b * cap;
    const size_t img = (size_t)b * S * S;
    // map index of pixel d1 of band line ld (:587-593)
    auto map_index = [&](int ld, int d1) { return axis ? img + (size_t)(band_lo + ld) * S + (c0 + d1) : img + (size_t)(c0 + d1) * S + band_lo + ld; };
    // (alpha, r, g, b) of a pixel, straight from the maps
    auto map_colour = [&](size_t gi) {
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (!RGB || ALPHA) c.x = alpha_map[gi];
        if constexpr (RGB) { c.y = rgb_map[3 * gi]; c.z = rgb_map[3 * gi + 1]; c.w = rgb_map[3 * gi + 2]; }
        return c;
    };
    // K of a line: the colour of its first pixel (see above); not finite: 0
    auto line_k = [&](int ld) {
        if constexpr (EXACT) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 k = map_colour(map_index(ld, 0));
        const bool fin = fabsf(k.x) <= 3.0e38f && fabsf(k.y) <= 3.0e38f && fabsf(k.z) <= 3.0e38f && fabsf(k.w) <= 3.0e38f;
        if (!fin) k = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return k;
    };
    // (the first window of the wave's first line is requested in front of the staging loads: one global round trip less on the
    // workgroup's critical path)
    int4 hh_first = make_int4(1, 1, 0, 0);
    float4 qq_first = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (wave < nld * n_parts) {
        const int ld = wave / n_parts, part = wave - ld * n_parts;
        const int n_rec = band_lines[lt + ld], r = (part / window_team(n_rec, n_parts, nsl)) * WIN + lane;  // (shared windows: below)
        if (r < n_rec) {
            const BandLine *R = recs_b + band_start[lt + ld] + r;
            hh_first = *reinterpret_cast<const int4 *>(R);
            qq_first = *reinterpret_cast<const float4 *>(&R->cross);
        }
    }
    // ---- stage the band: gradients, sums, face indices
    {
        auto put = [&](int ld, int d1, int fi, const float4 &k, float al, float ga, float r, float g, float bl, float gr, float gg, float gb) {
            const int l = ld * SP + d1;
            s_fi[l] = fi;
            if constexpr (RGB) {
                *reinterpret_cast<float4 *>(s_g + 4 * (size_t)l) = make_float4(ga, gr, gg, gb);
                if constexpr (EXACT)
                    *reinterpret_cast<float4 *>(s_p + 4 * (size_t)l) = make_float4(al, r, g, bl);
                else
                    s_p[l] = (float)((ALPHA ? (double)(al - k.x) * (double)ga : 0.0) + (double)(r - k.y) * (double)gr +
                                     (double)(g - k.z) * (double)gg + (double)(bl - k.w) * (double)gb);
            } else {
                s_g[l] = ga;
                s_p[l] = EXACT ? al : (al - k.x) * ga;
            }
            if constexpr (!EXACT) { if (d1 == 0) s_k[ld] = k; }
        };
        // four adjacent pixels of a map row with one 16-byte load per field (load_px_quad, nr_k6_fast.h)
        auto put_quad = [&](size_t g, int ld0, int d10, int ld_step, int d1_step) {
            const PxQuad q = load_px_quad<RGB, ALPHA>(fi_map, rgb_map, alpha_map, g_rgb, g_alpha, g);
            float4 k = line_k(ld0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j > 0 && ld_step) k = line_k(ld0 + j * ld_step);
                put(ld0 + j * ld_step, d10 + j * d1_step, q.fi[j], k, q.al[j], q.ga[j], q.rr[3 * j], q.rr[3 * j + 1], q.rr[3 * j + 2],
                    q.qq[3 * j], q.qq[3 * j + 1], q.qq[3 * j + 2]);
            }
        };
        auto put_one = [&](int ld, int d1) {
            const size_t g = map_index(ld, d1);
            float al = 0, ga = 0, r = 0, gn = 0, bl = 0, gr = 0, gg = 0, gb = 0;
            if (ALPHA) { al = alpha_map[g]; ga = g_alpha[g]; }
            if (RGB) {
                r = rgb_map[3 * g]; gn = rgb_map[3 * g + 1]; bl = rgb_map[3 * g + 2];
                gr = g_rgb[3 * g]; gg = g_rgb[3 * g + 1]; gb = g_rgb[3 * g + 2];
            }
            put(ld, d1, fi_map[g], line_k(ld), al, ga, r, gn, bl, gr, gg, gb);
        };
        if (SP != SL) {  // the pixels behind the chunk: no gradient, nobody's
            const int pad = SP - SL;
            for (int i = tid; i < nld * pad; i += NT) {
                const int ld = i / pad, l = ld * SP + SL + (i - ld * pad);
                s_fi[l] = -1;
                if constexpr (EXACT && RGB) *reinterpret_cast<float4 *>(s_p + 4 * (size_t)l) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                else s_p[l] = 0.0f;
                if constexpr (RGB) *reinterpret_cast<float4 *>(s_g + 4 * (size_t)l) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                else s_g[l] = 0.0f;
            }
        }
        if (axis && (S & 3) == 0) {  // a band line is an image row: thread -> (line, quad of 4 consecutive pixels)
            const int quads = SL >> 2;  // (c0 and SL are multiples of 4 with S)
            for (int i = tid; i < nld * quads; i += NT) {
                const int ld = i / quads, x = (i - ld * quads) << 2;
                put_quad(img + (size_t)(band_lo + ld) * S + c0 + x, ld, x, 0, 1);
            }
        } else if (axis) {  // thread -> (line, x), x fastest (coalesced 4- and 12-byte loads)
            for (int i = tid; i < nld * SL; i += NT) put_one(i / SL, i % SL);
        } else if (nld == 4 && (S & 3) == 0 && (band_lo & 3) == 0) {  // 4 adjacent columns: one thread per row
            for (int y = tid; y < SL; y += NT) put_quad(img + (size_t)(c0 + y) * S + band_lo, 0, y, 1, 0);
        } else {  // generic columns: thread -> (row d1, line ld) with ld fastest
            for (int i = tid; i < nld * SL; i += NT) put_one(i % nld, i / nld);
        }
    }
    __syncthreads();

    float eps_v = eps_f;
    asm volatile("" : "+v"(eps_v));
    // the exact mode's term: :649-651 / :654-656 (x * 2. / S: an exact float scaling when S is a power of two); ct = c * t
    const unsigned eps_hi = (unsigned)__double2hiint(eps_d), eps_lo = (unsigned)__double2loint(eps_d);
    const double s_d = (double)S, two_over_s_d = 2.0 / (double)S;
    const float two_over_s_f = (float)(2.0 / (double)S);
    // `x * 2. / S` of a float x, rounded to float, without the double division when S is not a power of two: the double product
    // x * RN(2 / S) is within 2^-52 of the quotient, and so is the correctly rounded double quotient the reference's expression
    // forms; the quotient itself is at least 2^-36 away (relative) from every point where the rounding to float changes -- such
    // a point is M 2^f with M odd and of 25 bits, x = X 2^e with X below 2^24, S = 2^k s with s odd, >= 3 and below 2^11:
    // X 2^e = M s 2^(f+k) is impossible (M s is odd and has 26 bits or more), and two different multiples of 2^f differ by 2^f
    // at least, i.e. by 1 / (M S) > 2^-36 of the quotient -- so both doubles round to the same float.  The argument needs the
    // float's full 24 bits: a result below the normal range takes the division (c is a ratio of differences of pixel coordinates
    // and |t| a distance between them: such a product is 0 or far above 1e-38; the branch keeps the argument free of that).
    // k_bpm_fast keeps the division everywhere; tests/test_hip_parity.py compares the two kernels' exact modes bit for bit.
    auto exact_scale = [&](float ct) {
        if constexpr (MODE == K6_EXACT_POW2) return ct * two_over_s_f;
        float q = (float)((double)ct * two_over_s_d);
        if (__builtin_expect(!(fabsf(q) >= 1.17549435e-38f) && ct != 0.0f, 0)) q = (float)((double)ct * 2.0 / s_d);
        return q;
    };
    auto exact_dist = [&](float ct) {
        const float dist = exact_scale(ct);
        return (float)((double)dist + signed_eps(dist, eps_hi, eps_lo));  // + eps when 0 < dist, - eps otherwise
    };
    // The reciprocal of phase A's terms -- the in sweep and the out sweep's first pixel: the pixels next to the crossing point,
    // whose terms are a record's largest -- with one Newton step: v_rcp_f32's 1 ulp becomes ~0.5.  A full ulp on the largest
    // term of an entry that cancels down to the metric's floor (1e-3 of the largest gradient) reads as 2^-23 / 1e-3 = 1.2e-4:
    // round 5's soak found such a scene at 1.13e-4.  Two fused multiply-adds per term of a lane-per-record loop: not measurable;
    // on every visit of phase B they would be +25 % of the kernel's vector work.
    auto recip_n = [](float y) {  // [row-recip-n]
        const float r = __builtin_amdgcn_rcpf(y);
        return __builtin_fmaf(__builtin_fmaf(-y, r, 1.0f), r, r);
    };
    // sum_c (I_c - ref_c) g_c with the reference's operations in its order (:631-638 / :709-716)
    auto exact_diff = [&](const float4 &c4, const float4 &cr, const float4 &g4) {
        if constexpr (!RGB) return (c4.x - cr.x) * g4.x;
        float d = ALPHA ? (c4.x - cr.x) * g4.x + (c4.y - cr.y) * g4.y : (c4.y - cr.y) * g4.y;
        d += (c4.z - cr.z) * g4.z;
        d += (c4.w - cr.w) * g4.w;
        return d;
    };
    // the lane's block (record of a group) and its pixel inside a segment (see above)
    const int row = (lane >> 2) & 3, l16 = ((((lane >> 4) + ((lane >> 2) & 2)) & 3) << 2) | (lane & 3);
    for (int vt = wave; vt < nld * n_parts; vt += NW) {
        const int ld = vt / n_parts, part = vt - ld * n_parts;
        const int n_rec = band_lines[lt + ld];
        if (n_rec == 0) continue;
        const BandLine *recs = recs_b + band_start[lt + ld];
        const int base = ld * SP;
        float4 kc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (!EXACT) kc = s_k[ld];
        // A line with fewer windows than its band gives it waves (bands narrower than the workgroup: rasters above 256, small
        // launches; one or two windows of records per line are the rule on meshes of a few thousand faces): the waves form
        // TEAMS that share a window instead of idling -- every member repeats the lane-per-record set-up (the records, the
        // reference colours, the sort: the same result in each), member 0 walks the in sweeps and the out pixels, and the
        // groups of phase B are dealt out in turn; every member flushes what it summed (a record's in and out parts may then
        // arrive as two atomic additions instead of one).  The sums of a record are formed exactly as before, by whichever
        // wave takes its group.  (K6 stage, us, teams off / on: 4 views at 1024^2 235 / 204, 32 views 1165 / 1028, 64 views at
        // 768^2 1195 / 1154, at 512^2 508 / 500; the exact mode at 640^2 ... 1024^2 -15 ... -22 %.)
        const int team = window_team(n_rec, n_parts, nsl), member = part & (team - 1), n_teams = n_parts / team;
        const bool sweeps_mine = member == 0;
        const int w_first = (part / team) * WIN;
        for (int w0 = w_first; w0 < n_rec; w0 += WIN * n_teams) {
            const int nw = min(WIN, n_rec - w0);
            // ---- phase A: lane = record.  The lane keeps its record for the flush, walks the record's in sweep, and prepares what
            // its block will be handed in phase B: the reference colour of the OUT sweep (the in pixel, :594-601) minus K, |c0|
            // (carrying the direction in its sign bit), |c1|, -direction * crossing point, the number of segments of the sweep.
            int4 hh = hh_first;
            float4 qq = qq_first;
            if (!(vt == wave && w0 == w_first)) {  // (not the window requested in front of the staging)
                hh = make_int4(1, 1, 0, 0);
                qq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (lane < nw) {
                    const BandLine *R = recs + w0 + lane;
                    hh = *reinterpret_cast<const int4 *>(R);
                    qq = *reinterpret_cast<const float4 *>(&R->cross);
                }
            }
            // (local positions: the in pixel and the out pixel may lie outside the chunk.  The crossing point stays what it is: a
            // pixel's t = d1 - d1_cross is formed from its position along the WHOLE line, c0 + local -- the crossing point minus c0
            // would be rounded wherever c0 is the larger of the two)
            const int flags = (hh.z >> 24) & 0xff, d1_in = (hh.z & 0xffff) - c0;
            const int og_from = hh.y & 0xffff, og_to = hh.y >> 16;  // the out sweep along the whole line ...
            const int ig_from = hh.x & 0xffff, ig_to = hh.x >> 16;  // ... and the in sweep
            const bool has_out = og_from <= og_to;  // (:604: the in pixel is the face's)
            const bool has_in = ig_from <= ig_to;   // (every record whose in and out pixel lie inside the image)
            const bool dpos = (flags & 8) != 0;   // direction > 0: the sweep ends at the last pixel of the line, else it starts at pixel 0
            const int d1_out = d1_in + (dpos ? 1 : -1);
            // what of the record lies in this chunk: its in sweep's pixels, its out pixel (phase A's), and phase B's part of the
            // out sweep -- [out pixel + 1, end of the line] or [0, out pixel - 1]; the exact mode: with the out pixel
            const int in_from = max(ig_from, c0) - c0, in_to = min(ig_to, c0 + SL - 1) - c0;
            const bool out_px_here = has_out && d1_out >= 0 && d1_out < SL;
            const int bg_from = og_from + ((dpos && !EXACT) ? 1 : 0), bg_to = og_to - ((!dpos && !EXACT) ? 1 : 0);
            const int b_from = max(bg_from, c0) - c0, b_to = min(bg_to, c0 + SL - 1) - c0;
            const bool has_b = has_out && b_from <= b_to;
            const bool in_here = has_in && in_from <= in_to;
            // the two reference colours straight from the maps: the in pixel for the out sweep (:594-601), the out pixel for the
            // in sweep (:697-700); minus K for the two-sum form of the visits
            float4 c_in = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c_out = c_in;
            if (has_in && (has_b || in_here || out_px_here)) {  // (a record with a pixel in this chunk)
                c_in = map_colour(map_index(ld, d1_in));
                c_out = map_colour(map_index(ld, d1_out));
            }
            const float4 oref = make_float4(c_in.x - kc.x, c_in.y - kc.y, c_in.z - kc.z, c_in.w - kc.w);
            const float4 iref = make_float4(c_out.x - kc.x, c_out.y - kc.y, c_out.z - kc.z, c_out.w - kc.w);
            // The two pixels next to the crossing point carry a record's largest terms (|t| <= 1).  Their colours are the two
            // reference colours, so their colour differences are formed DIRECTLY here -- sum_c (I_c - ref_c) g_c, the reference's
            // own expression -- and only the pixels further out go through the centred sums P: the in pixel is the first pixel
            // of the in sweep (below), the out pixel the first one of the out sweep, which phase B then leaves out (td > 1).
            auto direct_diff = [&](const float4 &ci, const float4 &cr, int l) {
                float4 g4;
                if constexpr (RGB) g4 = lds_px4(s_g + 4 * (size_t)l);
                else g4 = make_float4(s_g[l], 0.0f, 0.0f, 0.0f);
                float d;
                if constexpr (EXACT) {
                    d = exact_diff(ci, cr, g4);
                } else if constexpr (RGB) {
                    d = ALPHA ? __builtin_fmaf(ci.y - cr.y, g4.y, (ci.x - cr.x) * g4.x) : (ci.y - cr.y) * g4.y;
                    d = __builtin_fmaf(ci.z - cr.z, g4.z, d);
                    d = __builtin_fmaf(ci.w - cr.w, g4.w, d);
                } else {
                    d = (ci.x - cr.x) * g4.x;
                }
                return d;
            };
            float f0 = 0.0f, f1 = 0.0f;  // the out pixel's terms (magnitudes: the sign goes on at the flush, with the out sweep's)
            if (out_px_here && !EXACT && sweeps_mine) {  // (the exact mode: phase B walks the whole out sweep)
                const float d = direct_diff(c_out, c_in, base + d1_out);                           // :631-638
                const float dm = !(d <= 0.0f) ? d : 0.0f;                                           // :647
                const float t = fabsf((float)(c0 + d1_out) - qq.x);
                f0 = dm * recip_n(__builtin_fmaf(fabsf(qq.y), t, eps_v));                          // :649-651
                f1 = dm * recip_n(__builtin_fmaf(fabsf(qq.z), t, eps_v));                          // :654-656
            }
            if constexpr (!EXACT) {
                // Phase B tells the out pixel from the rest of the sweep by |t| <= 1 -- exact for every pixel but one: with the
                // crossing point within half an ulp of the in pixel's centre (a vertex snapped onto a pixel centre, the cross
                // product a rounding below it) the SECOND pixel's |t| = 1 + 2^-24 rounds to 1 and phase B leaves it out as well.
                // It is taken here, by the same comparison on the same float, with the centred sums phase B would have used
                // (tests/test_fuzz_gpu.py, seed 118: the term of such a pixel was missing, 27 % of a corner face's gradient).
                const int d1_2 = d1_out + (dpos ? 1 : -1);
                const float t2 = fabsf((float)(c0 + d1_2) - qq.x);
                if (has_out && og_from < og_to && d1_2 >= 0 && d1_2 < SL && t2 <= 1.0f && sweeps_mine) {
                    const int l = base + d1_2;
                    float4 g4;
                    if constexpr (RGB) g4 = lds_px4(s_g + 4 * (size_t)l);
                    else g4 = make_float4(s_g[l], 0.0f, 0.0f, 0.0f);
                    float d = s_p[l];
                    if constexpr (!RGB || ALPHA) d = __builtin_fmaf(-oref.x, g4.x, d);
                    if constexpr (RGB) {
                        d = __builtin_fmaf(-oref.y, g4.y, d);
                        d = __builtin_fmaf(-oref.z, g4.z, d);
                        d = __builtin_fmaf(-oref.w, g4.w, d);
                    }
                    const float dm = !(d <= 0.0f) ? d : 0.0f;
                    f0 = __builtin_fmaf(dm, recip_n(__builtin_fmaf(fabsf(qq.y), t2, eps_v)), f0);
                    f1 = __builtin_fmaf(dm, recip_n(__builtin_fmaf(fabsf(qq.z), t2, eps_v)), f1);
                }
            }
            // segments of what phase B walks in this chunk: [b_from / 16, nsl) towards the end of the line, [0, b_to / 16] from pixel 0
            const int nseg = has_b ? (dpos ? nsl - (b_from >> 4) : (b_to >> 4) + 1) : 0;
            hist[lane] = 0;
            double in0 = 0.0, in1 = 0.0;
            if (in_here && sweeps_mine) {
                const float cross = qq.x, c0k = qq.y, c1k = qq.z;
                const int fnr = __float_as_int(qq.w);
                const float d_first = (EXACT || d1_in < 0 || d1_in >= SL) ? 0.0f : direct_diff(c_in, c_out, base + d1_in);
                // (batches of IN_BATCH pixels whose LDS reads are requested together -- nine in-sweeps in ten are one batch;
                // IN_SEG float terms per double addition, like a piece of k_bpm_fast)
                for (int s0 = in_from; s0 <= in_to; s0 += IN_SEG) {
                    const int s1 = min(s0 + IN_SEG - 1, in_to);
                    float b0 = 0.0f, b1 = 0.0f;
                    for (int q0 = s0; q0 <= s1; q0 += IN_BATCH) {
                        int fi[IN_BATCH];
                        float4 g4[IN_BATCH], c4[IN_BATCH];
                        float p4[IN_BATCH];
#pragma unroll
                        for (int k = 0; k < IN_BATCH; ++k) {
                            const int l = base + min(q0 + k, s1);
                            fi[k] = s_fi[l];
                            c4[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                            p4[k] = 0.0f;
                            if constexpr (EXACT) {
                                if constexpr (RGB) c4[k] = lds_px4(s_p + 4 * (size_t)l);
                                else c4[k].x = s_p[l];
                            } else {
                                p4[k] = s_p[l];
                            }
                            if constexpr (RGB) g4[k] = lds_px4(s_g + 4 * (size_t)l);
                            else g4[k] = make_float4(s_g[l], 0.0f, 0.0f, 0.0f);
                        }
#pragma unroll
                        for (int k = 0; k < IN_BATCH; ++k) {
                            float diff;                                                            // :709-716
                            if constexpr (EXACT) {
                                diff = exact_diff(c4[k], c_out, g4[k]);
                            } else {
                                diff = p4[k];
                                if constexpr (!RGB || ALPHA) diff = __builtin_fmaf(-iref.x, g4[k].x, diff);
                                if constexpr (RGB) {
                                    diff = __builtin_fmaf(-iref.y, g4[k].y, diff);
                                    diff = __builtin_fmaf(-iref.z, g4[k].z, diff);
                                    diff = __builtin_fmaf(-iref.w, g4[k].w, diff);
                                }
                                if (q0 + k == d1_in) diff = d_first;
                            }
                            // :707, :717 (a NaN diff goes through); a pixel beyond the batch's end repeats the last one: dropped
                            const bool take = (q0 + k <= s1) & (fi[k] == fnr) & !(diff <= 0.0f);
                            const float t = (float)(c0 + q0 + k) - cross;
                            if constexpr (EXACT) {
                                // (the select in front of the division: a pixel that is not taken divides 0 by 1)
                                const float dm = take ? diff : 0.0f;
                                const float y0 = take ? exact_dist(c0k * t) : 1.0f, y1 = take ? exact_dist(c1k * t) : 1.0f;
                                in0 -= (double)(dm / y0);                                            // :719-722
                                in1 -= (double)(dm / y1);                                            // :724-727
                            } else {
                                const float x0 = c0k * t, x1 = c1k * t;                               // :719 / :724 (2 / S folded into c)
                                const float y0 = x0 + ((0.0f < x0) ? eps_v : -eps_v);                 // :720-721 / :725-726
                                const float y1 = x1 + ((0.0f < x1) ? eps_v : -eps_v);
                                const float dm = take ? diff : 0.0f;
                                // (y is never 0 here: x and its eps have one sign, eps > 0 -- so 0 * (1 / y) adds nothing)
                                b0 = __builtin_fmaf(-dm, recip_n(y0), b0);                            // :722
                                b1 = __builtin_fmaf(-dm, recip_n(y1), b1);                            // :727
                            }
                        }
                    }
                    in0 += (double)b0;
                    in1 += (double)b1;
                }
            }
            // ---- the order of phase B: records by falling number of segments (counting sort: a counter per key in LDS; the
            // records without an out sweep behind the others, so that the positions are a permutation of the lanes, which one
            // ds_permute_b32 inverts: lane k then knows which lane holds the k-th record)
            wave_lds_handover();
            const int key = MAX_SEGS - nseg;  // (only of records phase B walks: 0 .. MAX_SEGS - 1)
            int rank = 0;
            if (has_b) rank = atomicAdd(&hist[key], 1);
            wave_lds_handover();
            const int cnt = hist[lane], incl = wave_incl_scan_dpp(cnt);
            const int n_out = __builtin_amdgcn_readlane(incl, 63);
            wave_lds_handover();
            hist[lane] = incl - cnt;
            wave_lds_handover();
            const unsigned long long no_out = __ballot(!has_b);
            int pos = n_out + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(no_out >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)no_out, 0u));
            if (has_b) pos = hist[key] + rank;
            const int inv = __builtin_amdgcn_ds_permute(pos << 2, lane);
            wave_lds_handover();
            NR_ROW_STAT(0, 1);        // windows
            NR_ROW_STAT(1, nw);       // records
            NR_ROW_STAT(2, n_out);    // records with an out sweep
#ifdef NR_ROW_STATS
            {
                unsigned wid = 0;
                if (lane == 0) wid = atomicAdd(&g_row_dump_n, 1u);
                wid = (unsigned)__builtin_amdgcn_readfirstlane((int)wid);
                if (wid < NR_ROW_DUMP_WINDOWS)
                    g_row_dump[(size_t)wid * 64 + lane] = lane < nw ? ((unsigned)nseg | (dpos ? 256u : 0u) | (has_b ? 512u : 0u) | 1024u) : 0u;
            }
            {
                int sn = nseg, si = has_b ? (b_to - b_from + 1) : 0;
                for (int o = 32; o > 0; o >>= 1) { sn += __shfl_xor(sn, o, WAVE); si += __shfl_xor(si, o, WAVE); }
                NR_ROW_STAT(3, sn);   // segments of the out sweeps
                NR_ROW_STAT(4, si);   // pixels of the out sweeps
            }
#endif
            // ---- phase B: four records at a time, one per block of 16 lanes
            // what a block is handed (from the lane that holds the record)
            const float v_ncd = dpos ? -qq.x : qq.x;
            // fast mode: |c0| carrying the direction in its sign bit, |c1|; exact mode: c0 * direction, c1 * direction (signed: a
            // product with +-1 is exact, so (c * direction) * (direction * t) is the reference's c * t bit for bit), and the
            // direction in the sign of the segment count
            const float v_ac0 = EXACT ? (dpos ? qq.y : -qq.y)
                                      : __uint_as_float((__float_as_uint(qq.y) & 0x7fffffffu) | (dpos ? 0u : 0x80000000u));
            const float v_ac1 = EXACT ? (dpos ? qq.z : -qq.z) : fabsf(qq.z);
            const int v_nseg = EXACT ? (dpos ? nseg : -nseg) : nseg;
            float4 oref_b = oref;  // the out sweep's reference colour as the blocks use it: minus K, or as it is (exact mode)
            if constexpr (EXACT) oref_b = c_in;
            const int g_first = 4 * member, g_step = 4 * team;  // (a shared window: every team-th group)
            int src_next = __builtin_amdgcn_ds_bpermute(((g_first + row) & 63) << 2, inv);
            for (int g0 = g_first; g0 < n_out; g0 += g_step) {
                const bool act = g0 + row < n_out;
                const int src = src_next;  // (of a block without a record: some lane; nothing of it is used)
                src_next = __builtin_amdgcn_ds_bpermute(((g0 + g_step + row) & 63) << 2, inv);
                const int sa = src << 2;
                const int r_nseg_s = __builtin_amdgcn_ds_bpermute(sa, v_nseg);
                const int r_nseg = EXACT ? abs(r_nseg_s) : r_nseg_s;
                float ncd = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(v_ncd)));
                const float ac0s = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(v_ac0)));
                const float ac1 = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(v_ac1)));
                float ra = 0.0f, rr = 0.0f, rg = 0.0f, rb = 0.0f;
                if constexpr (!RGB || ALPHA) ra = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(oref_b.x)));
                if constexpr (RGB) {
                    rr = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(oref_b.y)));
                    rg = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(oref_b.z)));
                    rb = __int_as_float(__builtin_amdgcn_ds_bpermute(sa, __float_as_int(oref_b.w)));
                }
                // (a block without a record: td = -Inf for every pixel, nothing is taken, nothing stored)
                if (!act) ncd = -__builtin_inff();
                const float sdir = EXACT ? (r_nseg_s < 0 ? -1.0f : 1.0f)
                                         : __uint_as_float(0x3f800000u | (__float_as_uint(ac0s) & 0x80000000u));
                // the group walks as many steps as its longest sweep has segments (the first block's: the order of the sort; the exact
                // mode, which walks in pairs, an even number of them); a sweep towards the end of the line ENDS with the group's last
                // step, one from pixel 0 starts with its first; pixels in front of a sweep or behind it are masked (td <= 0)
                const int steps = __builtin_amdgcn_readfirstlane(r_nseg), steps2 = EXACT ? (steps + 1) & ~1 : steps;
                NR_ROW_STAT(5, 1);       // groups
                NR_ROW_STAT(6, steps2);  // steps walked
                const bool rpos = EXACT ? r_nseg_s >= 0 : !(__float_as_uint(ac0s) >> 31);
                const int seg0 = rpos ? nsl - steps2 : 0;
                const int p0 = seg0 * SEG + l16;
                float pf = (float)(c0 + p0);  // (the position along the whole line: see the crossing point above)
                double A0 = 0.0, A1 = 0.0;
                if constexpr (EXACT) {
                    // ---- the exact mode: gradients and colours of a step (two 16-byte reads), the reference's term (rasterize.py
                    // :631-657) operation by operation, a double accumulator pair per lane; td = direction * (d1 - d1_cross) is the
                    // reference's t = d1 - d1_cross times +-1, and ac0s / ac1 are its c0 / c1 times the same +-1: the products
                    // c * t are the reference's bit for bit
                    const unsigned char *gp = (const unsigned char *)s_g + (size_t)(base + p0) * (NC * 4);
                    const unsigned char *cp = (const unsigned char *)s_p + (size_t)(base + p0) * (NC * 4);
                    const float4 cref = make_float4(ra, rr, rg, rb);
                    auto load_x = [&](int k, float4 &g4, float4 &c4) {
                        if constexpr (RGB) {
                            g4 = *reinterpret_cast<const float4 *>(gp + k * (SEG * NC * 4));
                            c4 = *reinterpret_cast<const float4 *>(cp + k * (SEG * NC * 4));
                        } else {
                            g4 = make_float4(*reinterpret_cast<const float *>(gp + k * (SEG * NC * 4)), 0.0f, 0.0f, 0.0f);
                            c4 = make_float4(*reinterpret_cast<const float *>(cp + k * (SEG * NC * 4)), 0.0f, 0.0f, 0.0f);
                        }
                    };
                    auto visit_x = [&](const float4 &g4, const float4 &c4, const float pfv) {
                        if constexpr (RGB && !ALPHA) asm volatile("" : : "v"(g4.x), "v"(c4.x));
                        const float d = exact_diff(c4, cref, g4);
                        const float td = __builtin_fmaf(sdir, pfv, ncd);    // > 0 exactly on the sweep's pixels
                        const bool keep = !(td <= 0.0f) && !(d <= 0.0f);   // (:647: a NaN diff goes through)
                        // (both distances are formed for every lane and the select sits in front of the division: a masked lane
                        // divides 0 by 1 -- and the loop has no branch)
                        const float e0 = exact_dist(ac0s * td), e1 = exact_dist(ac1 * td);
                        const float dm = keep ? d : 0.0f, y0 = keep ? e0 : 1.0f, y1 = keep ? e1 : 1.0f;
                        A0 -= (double)(dm / y0);                                                    // :649-651
                        A1 -= (double)(dm / y1);                                                    // :654-656
                    };
                    for (int s = 0; s < steps2; s += 2) {  // (two steps per iteration: their reads and their chains overlap)
                        float4 gA, cA, gB, cB;
                        load_x(0, gA, cA);
                        load_x(1, gB, cB);
                        visit_x(gA, cA, pf);
                        visit_x(gB, cB, pf + (float)SEG);
                        gp += 2 * SEG * NC * 4;
                        cp += 2 * SEG * NC * 4;
                        pf += (float)(2 * SEG);
                    }
                    A0 = __builtin_amdgcn_mfma_f64_4x4x4f64(A0, 1.0, 0.0, 0, 0, 0);
                    A1 = __builtin_amdgcn_mfma_f64_4x4x4f64(A1, 1.0, 0.0, 0, 0, 0);
                    A0 = __builtin_amdgcn_mfma_f64_4x4x4f64(A0, 1.0, 0.0, 0, 0, 0);
                    A1 = __builtin_amdgcn_mfma_f64_4x4x4f64(A1, 1.0, 0.0, 0, 0, 0);
                } else {
                    const unsigned char *gp = (const unsigned char *)s_g + (size_t)(base + p0) * (NC * 4);
                    const float *pp = s_p + base + p0;
                    auto visit = [&](const float4 &g4, const float pv, const float pfv, float &a0, float &a1) {
                        float d = pv;                                       // :631-638  [row-visit] diff: four fused multiply-adds
                        if constexpr (!RGB || ALPHA) d = __builtin_fmaf(-ra, g4.x, d);
                        if constexpr (RGB) {
                            d = __builtin_fmaf(-rr, g4.y, d);
                            d = __builtin_fmaf(-rg, g4.z, d);
                            d = __builtin_fmaf(-rb, g4.w, d);
                        }
                        // direction * (d1 - d1_cross): > 0 exactly on the sweep's pixels, in (0, 1] on its first one -- phase A's
                        const float td = __builtin_fmaf(sdir, pfv, ncd);
                        const bool keep = !(td <= 1.0f) && !(d <= 0.0f);  // (:647: a NaN diff goes through)
                        const float dm = keep ? d : 0.0f;
                        const float y0 = __builtin_fmaf(fabsf(ac0s), fabsf(td), eps_v), y1 = __builtin_fmaf(ac1, fabsf(td), eps_v);  // :649-650 / :654-655
                        // [row-rcp] v_rcp_f32 (<= 1 ulp), the term added to the lane's float sum
                        a0 = __builtin_fmaf(dm, __builtin_amdgcn_rcpf(y0), a0);                        // :651 (sign: the flush)
                        a1 = __builtin_fmaf(dm, __builtin_amdgcn_rcpf(y1), a1);                        // :656
                    };
                    // (plain 16-byte reads: lds_px4's barrier would make every read wait for its data on the spot; the instance without
                    // alpha keeps its first component formally alive BEHIND the visit instead, see lds_px4)
                    auto load = [&](int k, float4 &g4, float &pv) {
                        if constexpr (RGB) g4 = *reinterpret_cast<const float4 *>(gp + k * (SEG * NC * 4));
                        else g4 = make_float4(*reinterpret_cast<const float *>(gp + k * (SEG * NC * 4)), 0.0f, 0.0f, 0.0f);
                        pv = pp[k * SEG];
                    };
                    auto used = [&](const float4 &g4) {
                        if constexpr (RGB && !ALPHA) asm volatile("" : : "v"(g4.x));
                    };
                    // A lane adds the terms of its even and of its odd segments in float (<= 8 terms each at raster 256, 32 at 1024: the
                    // terms fall off like 1 / t); everything above is double: the matrix pipe adds the 2 x 16 sums of a block.  Steps
                    // alternate between the two sums, so a sweep's terms are always split into its even and its odd segments -- which
                    // of the two registers holds which depends on the group (seg0 may be odd), the two sets and their order do not, and
                    // the two sums meet in a double addition: a record's sums are the same bits whatever window, group or launch it is
                    // part of.  (Chains cut every 16 / 8 / 4 steps,
                    // each with a reduction of its own: +0 / +4 / +12 % kernel time at raster 256, error levels unchanged.)
                    float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
                    {
                        // Two steps per pair, two pairs of registers: while one pair is visited the other pair's reads are in flight
                        // (the scheduling barriers keep the compiler from gathering the reads at the top of the loop, where every
                        // iteration would wait for them).  Behind the group's last step the reads fetch what is never used (inside
                        // the workgroup's LDS: at most two segments past a line).
                        float4 gA, gB, gC, gD;
                        float pA, pB, pC, pD;
                        load(0, gA, pA);
                        load(1, gB, pB);
                        int s = 0;
                        for (; s + 4 <= steps2; s += 4) {
                            load(2, gC, pC);
                            load(3, gD, pD);
                            __builtin_amdgcn_sched_barrier(0);
                            visit(gA, pA, pf, a0, a1);
                            used(gA);
                            visit(gB, pB, pf + (float)SEG, b0, b1);
                            used(gB);
                            __builtin_amdgcn_sched_barrier(0);
                            load(4, gA, pA);
                            load(5, gB, pB);
                            __builtin_amdgcn_sched_barrier(0);
                            visit(gC, pC, pf + (float)(2 * SEG), a0, a1);
                            used(gC);
                            visit(gD, pD, pf + (float)(3 * SEG), b0, b1);
                            used(gD);
                            __builtin_amdgcn_sched_barrier(0);
                            gp += 4 * (SEG * NC * 4);
                            pp += 4 * SEG;
                            pf += (float)(4 * SEG);
                        }
                        if (const int rem = steps2 - s) {  // (the last one to three steps: two of them already requested)
                            if (rem == 3) load(2, gC, pC);
                            visit(gA, pA, pf, a0, a1);
                            used(gA);
                            if (rem >= 2) {
                                visit(gB, pB, pf + (float)SEG, b0, b1);
                                used(gB);
                            }
                            if (rem == 3) {
                                visit(gC, pC, pf + (float)(2 * SEG), a0, a1);
                                used(gC);
                            }
                        }
                    }
                    A0 = __builtin_amdgcn_mfma_f64_4x4x4f64((double)a0, 1.0, 0.0, 0, 0, 0);
                    A1 = __builtin_amdgcn_mfma_f64_4x4x4f64((double)a1, 1.0, 0.0, 0, 0, 0);
                    A0 = __builtin_amdgcn_mfma_f64_4x4x4f64((double)b0, 1.0, A0, 0, 0, 0);
                    A1 = __builtin_amdgcn_mfma_f64_4x4x4f64((double)b1, 1.0, A1, 0, 0, 0);
                    A0 = __builtin_amdgcn_mfma_f64_4x4x4f64(A0, 1.0, 0.0, 0, 0, 0);
                    A1 = __builtin_amdgcn_mfma_f64_4x4x4f64(A1, 1.0, 0.0, 0, 0, 0);
                }
                if (act && lane == (row << 2)) acc[src] = make_double2(A0, A1);  // (every lane of the block holds the sums)
            }
            wave_lds_handover();
            // ---- flush: in sweep + out sweep of each record -> global double scratch [list position][vertex][x|y].
            // Out sweep: grad -= diff / (sigma * |dist|), sigma = sign(c) * sign(t), sign(t) = the direction (t = d1 - d1_cross
            // keeps its sign beyond the crossing point): the magnitudes were summed, the sign goes on here.  :648 / :653 (and
            // :718 / :723): a contribution whose vertex sits on the line is not taken (its coefficient was Inf / NaN).
            if (lane < nw) {
                double2 a = make_double2(0.0, 0.0);
                if (has_b && ((pos >> 2) & (team - 1)) == member) a = acc[lane];  // (the wave that walked the record's group)
                a.x += (double)f0;
                a.y += (double)f1;
                const bool tneg = !dpos;
                // (the exact mode's sums carry their signs: -(diff / dist) term by term)
                const bool neg0 = EXACT || (((__float_as_uint(qq.y) >> 31) != 0) != tneg);
                const bool neg1 = EXACT || (((__float_as_uint(qq.z) >> 31) != 0) != tneg);
                const double t0 = (flags & 2) ? in0 + (neg0 ? a.x : -a.x) : 0.0;
                const double t1 = (flags & 4) ? in1 + (neg1 ? a.y : -a.y) : 0.0;
                const int tgt = hh.w, lpos = tgt & 0x0fffffff;
                double *dst = scratch + ((size_t)b * F + lpos) * 6 + (1 - axis);
                if (t0 != 0.0) atomicAdd(dst + 2 * ((tgt >> 28) & 3), t0);
                if (t1 != 0.0) atomicAdd(dst + 2 * ((tgt >> 30) & 3), t1);
            }
            wave_lds_handover();
        }
    }
}

template <bool RGB, bool ALPHA, int MODE, bool CHUNKED>
__global__ __launch_bounds__(rowk::NT, MODE == K6_FAST ? 5 : 4) void k_bpm_row(
    const int32_t *__restrict__ fi_map, const float *__restrict__ rgb_map, const float *__restrict__ alpha_map,
    const float *__restrict__ g_rgb, const float *__restrict__ g_alpha, double *__restrict__ scratch,
    const int *__restrict__ band_lines, const int *__restrict__ band_start, const int *__restrict__ lines_ok,
    const BandLine *__restrict__ line_buf, size_t cap, int F, int S, int W, int CH, float eps_f, double eps_d, int B,
    uint4 *__restrict__ zero16, size_t n_zero16)
{
    bpm_row_body<RGB, ALPHA, MODE, CHUNKED, false>(fi_map, rgb_map, alpha_map, g_rgb, g_alpha, scratch, band_lines, band_start, lines_ok,
                                                   line_buf, cap, F, S, W, CH, eps_f, eps_d, B, zero16, n_zero16, nullptr, 1u);
}

// --------------------------------------------------------------------------------------------------
// The fused backward's merged launch (plan_backward: gather_in_tail): k_bpm_row's workgroups and, BEHIND them in grid order, the
// K7 / K8 face gather's (nr_face_gather.h; static taps, texture_size 2).  Both kernels are bound by the workgroups the chip
// holds -- five per CU either way -- times a workgroup's life, and a kernel that runs in rounds ends with a tail: once the last
// band workgroup is handed out the chip empties over one workgroup life while a launch of its own could start nothing.  Here
// the dispatcher, which hands out workgroups in grid order, goes on with the gather's: they fill the slots the band kernel's
// last round frees and take no slot a band workgroup was waiting for, and one launch boundary goes.  (Round 5's "side job"
// interleaved the two in runs of 8 ids and paid k_bpm_fast's 40 KB of LDS per gather workgroup: it lost.)
// Nothing in the launch waits for anything: the gather reads nothing the band part writes.  K6's sums are rounded onto
// grad_faces by k_backward_big behind this launch (FINISH_BIG), the compaction stored grad_faces' zeros (FACE_ZEROS_ALL), and
// of grad_textures the band workgroups zero the unlisted faces' cubes only -- the gather stores every listed face's cube.
//   grid = [xcd_grid(band workgroups) | gather_x * B], gather id -> (bx, by) = (id / B, id % B): working-first order
//   (image_fastest, nr_device.h); gather_x = ceil(F / 16) slots over k6::SLOT_STRIDE, a workgroup looping over its slots.
template <bool RGB, bool ALPHA, bool DEPTH>
__global__ __launch_bounds__(rowk::NT, 5) void k_band_gather(BandRowArgs r, FaceGatherArgs g, unsigned band_grid, unsigned gather_x)
{
    if (blockIdx.x < band_grid) {
        bpm_row_body<RGB, ALPHA, K6_FAST, false, true>(r.fi_map, r.rgb_map, r.alpha_map, r.g_rgb, r.g_alpha, r.scratch, r.band_lines,
                                                       r.band_start, r.lines_ok, r.line_buf, r.cap, r.F, r.S, r.W, r.CH, r.eps_f, r.eps_d,
                                                       r.B, r.zero16, r.n_zero16, r.zero_slot, r.zero_epf);
    } else {
        // gather_x slots per image in the launch, fewer than the longest list may need: slot bx, bx + gather_x, ... while the
        // image's list lasts (a wave's four faces need nothing of the workgroup's other waves: no barrier between two slots)
        const SlotImage w = image_fastest(blockIdx.x - band_grid, (unsigned)r.B);
        const int n_vis = g.vis_count[w.by];
        for (int bx = w.bx; bx * 16 < n_vis; bx += (int)gather_x) face_gather_body<true, DEPTH, false>(g, bx, w.by);
    }
}
