// nr_k6_lists.h -- what K6's band kernels are handed: the lists of visible faces and the band tables.  Part of the translation
// unit nr_backward_pixel_map.hip (included there and nowhere else, behind `using namespace nr`).
//
//   [k_mark_visible]   only when the forward did not hand over its per-face "owns a pixel" flags (visible_faces)
//   k_compact_par | k_count_visible + k_compact_visible   per image, the sorted list of faces that own at least one
//          pixel.  A face that owns no pixel contributes nothing to K6 (the out sweep needs face_index[in] == fn,
//          :604, the in sweep only counts pixels owned by fn, :707), so ~2/3 of the front faces drop out.  The
//          compaction also stores, per listed face, the line range of each of its 3 edges along both axes, zeroes the
//          face's six double sums (indexed by list position: no fill launch), records face -> list position and counts the
//          lines of every (axis, band): a band workgroup whose count is zero leaves at once (more than half of the bands
//          of a teapot view: the object covers 12 % of the image).  The three kernels that rank faces share chunk_rank.
//   k_line_setup   every line's record (crossing point, in / out pixels, sweep ranges, the two distance coefficients:
//          rasterize.py:573-579, :606-609, :665-672), written band by band into one buffer.
//          (The records and the kernel's body live in nr_band_lines.h: in the fused backward of a small call the K7 / K8
//          gather shares this launch -- nr_backward_gather.hip, k_setup_gather, when plan_backward says so.)

__global__ __launch_bounds__(256) void k_mark_visible(const int32_t *__restrict__ fi_map,
                                                      unsigned char *__restrict__ flags, int F, int SS, size_t P)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int fi = fi_map[i];
    if (fi >= 0) flags[(i / SS) * F + fi] = 1;
}

// What the compaction records for the face at list position `pos` of image b: its index, the six edge line ranges
// rng[b][axis][pos][edge] (so that the 2 * n_bands band workgroups of an image scan 12 coalesced bytes per face instead of
// chasing list -> vertices each) and six zeroed double sums.
__device__ __forceinline__ void emit_visible(int b, int fn, int pos, int F, int S, const float *__restrict__ faces,
                                             int *__restrict__ vis_list, unsigned *__restrict__ rng,
                                             double *__restrict__ scratch, int *band_count, int n_bands, int W,
                                             int *line_diff = nullptr)
{
    vis_list[(size_t)b * F + pos] = fn;
    const float *f = faces + ((size_t)b * F + fn) * 9;
    const float fs = (float)S;
    float px[3], py[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { px[k] = to_pixel(f[3 * k], fs); py[k] = to_pixel(f[3 * k + 1], fs); }
    unsigned *r0 = rng + (((size_t)b * 2 + 0) * F + pos) * 3, *r1 = rng + (((size_t)b * 2 + 1) * F + pos) * 3;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const unsigned ra = edge_range(px[e], px[(e + 1) % 3], S), rb = edge_range(py[e], py[(e + 1) % 3], S);
        r0[e] = ra;
        r1[e] = rb;
        // lines per (axis, band of W lines): a band workgroup whose count is zero leaves at once
#pragma unroll
        for (int axis = 0; axis < 2; axis++) {
            const unsigned r = axis ? rb : ra;
            const int lo = (int)(r & 0xffffu), hi = (int)(r >> 16);
            if (line_diff) {
                // (k_compact_par: +1 where the edge's lines begin, -1 behind their end; the workgroup's prefix sum turns the
                // array into "edges on this line", whose sums over a band's lines are the counts -- two atomics per edge and
                // axis instead of one per band crossed, a loop of ~5 dependent LDS atomics on one-line bands)
                if (lo <= hi) {
                    atomicAdd(line_diff + axis * (S + 1) + lo, 1);
                    atomicAdd(line_diff + axis * (S + 1) + hi + 1, -1);
                }
                continue;
            }
            for (int band = lo / W; band * W <= hi; ++band)  // lo > hi (RNG_EMPTY): no iteration
                atomicAdd(band_count + axis * n_bands + band, min(hi, band * W + W - 1) - max(lo, band * W) + 1);
        }
    }
    double2 *z = reinterpret_cast<double2 *>(scratch + ((size_t)b * F + pos) * 6);
    z[0] = z[1] = z[2] = make_double2(0.0, 0.0);
}

// grad_faces of a face that owns no pixel (K6 contributes nothing, rasterize.py:604 / :707; K8 neither): when the fused
// backward finishes K6 inside its gather launch, the compaction -- which visits every face anyway -- stores these zeros
// (zero_listed: those of the listed faces too -- the fused backward whose gather runs BEFORE the band kernel and adds K8's sums)
__device__ __forceinline__ void zero_face(float *__restrict__ o)
{
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = 0.0f;
}

// Ordered compaction: every face gets slot_of = its position in the image's sorted list of visible faces, or -1.  One
// workgroup per chunk of 1024 faces.
//   Meshes of up to SMALL_CHUNKS chunks, one launch (k_compact_par): a workgroup counts the flags of the chunks in front of
//   its own (<= 15 coalesced bytes per thread) and leaves its lines-per-band counts as a dense row chunk_band[b][chunk][.];
//   the consumer (k_line_setup, or k_band_total when there is none) adds the rows up and takes the prefix.  (One workgroup
//   per image walking the chunks in order took 16 us for 5 chunks, 99 us for a 2048 x 2048 view with its 2 x 2048 bands.)
//   Larger meshes (config 5: 655 360 faces, B = 1), two launches + k_band_scan: k_count_visible counts the flags of each
//   chunk, k_compact_visible turns the counts of the preceding chunks into the chunk's offset and adds its band counts to
//   the image's global counters.
constexpr int VIS_CHUNK = 1024;
constexpr int SMALL_CHUNKS = 16;

// The rank of a chunk's faces, shared by the three compaction kernels (thread tid of workgroup (chunk, b): face chunk * VIS_CHUNK +
// tid; v: it exists and owns a pixel).  part: the wave's share of the visible faces in the chunks in front, however the kernel splits
// that count over its waves -- k_compact_par and k_list_visible count the flags (chunk_flags_before: <= SMALL_CHUNKS - 1 coalesced bytes
// per thread), k_compact_visible adds up k_count_visible's counts.  s_part / s_wcnt: [VIS_CHUNK / 64] ints of LDS.  Returns the wave's
// ballot of v; off + its set bits below the lane is the face's list position, own the chunk's number of visible faces.
__device__ __forceinline__ int chunk_flags_before(const unsigned char *flags, int b, int F, int chunk)
{
    int part = 0;
    for (int c = 0, tid = threadIdx.x; c < chunk; ++c) part += __popcll(__ballot(flags[(size_t)b * F + c * VIS_CHUNK + tid] != 0));
    return part;
}
__device__ __forceinline__ unsigned long long chunk_rank(bool v, int part, int *s_part, int *s_wcnt, int &off, int &own)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long m = __ballot(v);
    if (lane == 0) { s_part[wave] = part; s_wcnt[wave] = __popcll(m); }
    __syncthreads();
    off = own = 0;
    for (int w = 0; w < VIS_CHUNK / 64; ++w) {
        off += s_part[w];
        if (w < wave) off += s_wcnt[w];
        own += s_wcnt[w];
    }
    return m;
}
// vis_count[b], for thread 0 of the image's last chunk: the faces in front of the chunk and its own
__device__ __forceinline__ int chunk_rank_total(int own, const int *s_part)
{
    int base = 0;
    for (int w = 0; w < VIS_CHUNK / 64; ++w) base += s_part[w];
    return base + own;
}

__global__ __launch_bounds__(VIS_CHUNK) void k_compact_par(const unsigned char *__restrict__ flags,
                                                           int *__restrict__ vis_list, int *__restrict__ vis_count,
                                                           int *__restrict__ slot_of, int F, int n_chunks,
                                                           const float *__restrict__ faces, unsigned *__restrict__ rng,
                                                           double *__restrict__ scratch, int S,
                                                           int *__restrict__ chunk_band, int n_bands, int W,
                                                           int *__restrict__ band_cursor, float *__restrict__ zero_faces,
                                                           int zero_listed, int use_diff, int *__restrict__ ticket)
{
    extern __shared__ int s_band[];  // [2][n_bands] lines per band of this chunk's faces; use_diff: + [2][S + 1] line differences
    __shared__ int s_wcnt[VIS_CHUNK / 64];
    __shared__ int s_part[VIS_CHUNK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 2 * n_bands; i += VIS_CHUNK) s_band[i] = 0;
    int *s_diff = use_diff ? s_band + 2 * n_bands : nullptr;
    if (use_diff)
        for (int i = tid; i < 2 * (S + 1); i += VIS_CHUNK) s_diff[i] = 0;
    const int part = chunk_flags_before(flags, b, F, chunk), fn = chunk * VIS_CHUNK + tid;
    const bool v = fn < F && flags[(size_t)b * F + fn] != 0;
    int off, own;
    const unsigned long long m = chunk_rank(v, part, s_part, s_wcnt, off, own);
    if (fn < F) {
        const int before = off + __popcll(m & ((1ull << lane) - 1ull));  // visible faces in front of fn
        slot_of[(size_t)b * F + fn] = v ? before : -1;
        if (v) emit_visible(b, fn, before, F, S, faces, vis_list, rng, scratch, s_band, n_bands, W, s_diff);
        if (zero_faces && (!v || zero_listed)) zero_face(zero_faces + ((size_t)b * F + fn) * 9);
    }
    __syncthreads();
    if (use_diff) {
        // line differences -> edges per line (inclusive prefix over the 2 (S + 1) entries; the entry behind an axis' last line
        // takes the closing -1s, so the running sum is back at 0 where the second axis begins) -> lines per band
        const int n2 = 2 * (S + 1), per = (n2 + VIS_CHUNK - 1) / VIS_CHUNK, i0 = tid * per, i1 = min(n2, i0 + per);
        int local = 0;
        for (int i = i0; i < i1; ++i) local += s_diff[i];
        const int inc = wave_incl_scan(local, lane);
        __syncthreads();  // (s_part / s_wcnt were read above by every thread: reuse s_wcnt for the wave totals)
        if (lane == 63) s_wcnt[wave] = inc;
        __syncthreads();
        int run = inc - local;
        for (int w = 0; w < wave; ++w) run += s_wcnt[w];
        for (int i = i0; i < i1; ++i) {
            run += s_diff[i];
            s_diff[i] = run;
        }
        __syncthreads();
        for (int i = tid; i < 2 * n_bands; i += VIS_CHUNK) {
            const int axis = i >= n_bands, band = i - axis * n_bands;
            int c = 0;
            for (int l = band * W; l < min(S, band * W + W); ++l) c += s_diff[axis * (S + 1) + l];
            s_band[i] = c;
        }
        __syncthreads();
    }
    int *row = chunk_band + ((size_t)b * n_chunks + chunk) * 2 * n_bands;
    for (int i = tid; i < 2 * n_bands; i += VIS_CHUNK) row[i] = s_band[i];
    if (chunk == 0)  // the fill cursors of k_line_setup (it runs after this kernel)
        for (int i = tid; i < 2 * n_bands; i += VIS_CHUNK) band_cursor[(size_t)b * 2 * n_bands + i] = 0;
    if (chunk == n_chunks - 1 && tid == 0) vis_count[b] = chunk_rank_total(own, s_part);
    if (chunk == 0 && b == 0 && tid == 0) *ticket = 0;  // (the overflow pass's ticket counter: k_big_overflow)
}

// the lists alone (depth-only backward: no K6, but the K8 gather still wants to visit only the faces that own a pixel)
__global__ __launch_bounds__(VIS_CHUNK) void k_list_visible(const unsigned char *__restrict__ flags,
                                                            int *__restrict__ vis_list, int *__restrict__ vis_count, int F,
                                                            int n_chunks)
{
    __shared__ int s_wcnt[VIS_CHUNK / 64];
    __shared__ int s_part[VIS_CHUNK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int part = chunk_flags_before(flags, b, F, chunk), fn = chunk * VIS_CHUNK + tid;
    const bool v = fn < F && flags[(size_t)b * F + fn] != 0;
    int off, own;
    const unsigned long long m = chunk_rank(v, part, s_part, s_wcnt, off, own);
    if (v) vis_list[(size_t)b * F + off + __popcll(m & ((1ull << lane) - 1ull))] = fn;
    if (chunk == n_chunks - 1 && tid == 0) vis_count[b] = chunk_rank_total(own, s_part);
}

__global__ __launch_bounds__(VIS_CHUNK) void k_count_visible(const unsigned char *__restrict__ flags,
                                                             int *__restrict__ chunk_count, int F, int n_chunks,
                                                             int *__restrict__ band_lines, int n_bands)
{
    __shared__ int s_wcnt[VIS_CHUNK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the image's band counters are accumulated with global atomics by k_compact_visible: zero them here (one launch earlier)
    for (int i = chunk * VIS_CHUNK + tid; i < 2 * n_bands; i += n_chunks * VIS_CHUNK) band_lines[(size_t)b * 2 * n_bands + i] = 0;
    const int fn = chunk * VIS_CHUNK + tid;
    const bool v = fn < F && flags[(size_t)b * F + fn] != 0;
    const unsigned long long m = __ballot(v);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < VIS_CHUNK / 64; ++w) tot += s_wcnt[w];
        chunk_count[(size_t)b * n_chunks + chunk] = tot;
    }
}

__global__ __launch_bounds__(VIS_CHUNK) void k_compact_visible(const unsigned char *__restrict__ flags,
                                                               const int *__restrict__ chunk_count,
                                                               int *__restrict__ vis_list, int *__restrict__ vis_count,
                                                               int *__restrict__ slot_of, int F, int n_chunks,
                                                               const float *__restrict__ faces,
                                                               unsigned *__restrict__ rng, double *__restrict__ scratch,
                                                               int S, int *__restrict__ band_lines, int n_bands, int W,
                                                               int lds_counters, float *__restrict__ zero_faces,
                                                               int zero_listed)
{
    // This workgroup's lines per band are counted in LDS and only the non-zero counters go to the image's global ones:
    // one device-wide atomic per (face, edge, band) cost 315 us on config 5 (same-address atomics from all 8 XCDs).
    extern __shared__ int s_band[];  // [2 * n_bands] when lds_counters
    __shared__ int s_wcnt[VIS_CHUNK / 64];
    __shared__ int s_part[VIS_CHUNK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    if (lds_counters)
        for (int i = tid; i < 2 * n_bands; i += VIS_CHUNK) s_band[i] = 0;
    // offset of this chunk = sum of the counts of the chunks before it
    int part = 0;
    for (int c = tid; c < chunk; c += VIS_CHUNK) part += chunk_count[(size_t)b * n_chunks + c];
    part = wave_sum(part);
    const int fn = chunk * VIS_CHUNK + tid;
    const bool v = fn < F && flags[(size_t)b * F + fn] != 0;
    int off, own;
    const unsigned long long m = chunk_rank(v, part, s_part, s_wcnt, off, own);
    if (fn < F) {
        const int before = off + __popcll(m & ((1ull << (tid & 63)) - 1ull));  // visible faces in front of fn
        slot_of[(size_t)b * F + fn] = v ? before : -1;
        if (zero_faces && (!v || zero_listed)) zero_face(zero_faces + ((size_t)b * F + fn) * 9);
        if (v)
            emit_visible(b, fn, before, F, S, faces, vis_list, rng, scratch,
                         lds_counters ? s_band : band_lines + (size_t)b * 2 * n_bands, n_bands, W);
    }
    if (lds_counters) {
        __syncthreads();
        for (int i = tid; i < 2 * n_bands; i += VIS_CHUNK) {
            const int c = s_band[i];
            if (c) atomicAdd(band_lines + (size_t)b * 2 * n_bands + i, c);
        }
    }
    if (chunk == n_chunks - 1 && tid == 0) vis_count[b] = chunk_rank_total(own, s_part);
}

// rasterize.py:651 / :656 / :722 / :727: `dist += eps` when 0 < dist, `dist -= eps` otherwise (eps is a double literal there).
// Returns +-eps; only the high dword depends on the comparison (one v_cndmask instead of two selects on 64-bit values).
__device__ __forceinline__ double signed_eps(float dist, unsigned eps_hi, unsigned eps_lo)
{
    return __hiloint2double((int)((0.0f < dist) ? eps_hi : (eps_hi ^ 0x80000000u)), (int)eps_lo);
}

// (ids in working-first order: image_fastest, nr_device.h)
__global__ __launch_bounds__(256, 8) void k_line_setup(LineSetupArgs a)
{
    const SlotImage w = image_fastest(blockIdx.x, a.grid_y);
    line_setup_body(a, w.bx, w.by);
}

// exclusive prefix of an image's 2 * n_bands line counts (first wave of the block), the image's total and the verdict
// whether its records fit the buffer; zeroes the fill cursors
__device__ __forceinline__ void band_prefix(const int *cnt, int n2, int *__restrict__ start_out, int *__restrict__ cursor_out,
                                            int *__restrict__ ok_out, size_t cap)
{
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x, per = (n2 + 63) / 64;
    int local = 0;
    for (int i = lane * per; i < min(n2, (lane + 1) * per); ++i) local += cnt[i];
    const int inc = wave_incl_scan(local, lane);
    int run = inc - local;
    for (int i = lane * per; i < min(n2, (lane + 1) * per); ++i) {
        start_out[i] = run;
        cursor_out[i] = 0;
        run += cnt[i];
    }
    const int total = __shfl(inc, 63, WAVE);
    if (lane == 0) *ok_out = ((size_t)total <= cap) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_band_scan(const int *__restrict__ band_lines, int *__restrict__ band_start,
                                                   int *__restrict__ band_cursor, int *__restrict__ lines_ok, int n_bands,
                                                   size_t cap, int force_scan, int *__restrict__ ticket)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0;  // (the overflow pass's ticket counter: k_big_overflow)
    const size_t o = (size_t)blockIdx.x * 2 * n_bands;
    band_prefix(band_lines + o, 2 * n_bands, band_start + o, band_cursor + o, lines_ok + blockIdx.x, force_scan ? 0 : cap);
}

// the same table from the chunk rows of k_compact_par when no k_line_setup follows (NR_FLAG_K6_SCAN): every
// image is told to take the scan path
__global__ __launch_bounds__(256) void k_band_total(const int *__restrict__ chunk_band, int n_sum, int *__restrict__ band_lines,
                                                    int *__restrict__ band_start, int *__restrict__ lines_ok, int n_bands)
{
    const int b = blockIdx.x, n2 = 2 * n_bands;
    const int *rows = chunk_band + (size_t)b * n_sum * n2;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        int t = 0;
        for (int c = 0; c < n_sum; ++c) t += rows[(size_t)c * n2 + i];
        band_lines[(size_t)b * n2 + i] = t;
        band_start[(size_t)b * n2 + i] = 0;
    }
    if (threadIdx.x == 0) lines_ok[b] = 0;
}
