// nr_soft_silhouette.hip -- soft silhouettes: distance-based coverage with its exact gradient (include/nr_hip.h; DESIGN
// "Soft silhouettes").
//
// Per contributing face f and pixel p: d2 = the squared distance of p to the nearest of the three edge segments (lowest
// segment on a tie), s = +1 strictly inside the triangle, else -1, x = s d2 / sigma, D = 1 / (1 + e^-x);
// Q_p = the product of 1 / (1 + e^x) in ascending f, alpha_p = 1 - Q_p.  A face contributes iff its nine coordinates are
// finite and near <= z <= far at its three vertices.  A (pixel, face) pair is taken iff the pixel lies in the face's BOX:
// the pixel range of the triangle's bounding box grown by sqrt(17 sigma); a pair outside it is outside the triangle with
// d2 > 17 sigma (D < 2^-24) and is left out of both directions.
//   k_soft_setup     (image, face) -> a 48-byte record: the six xy, the box, the flag (soft_record, nr_soft_pair.h)
//   k_soft_forward   a workgroup of four waves owns a 16 x 16 pixel tile, a wave an 8 x 8 quarter of it, a lane a pixel
//                    (soft_tile).  The records go through LDS in chunks of 256 (one per thread); those whose box meets the
//                    tile are kept in a compact list in ascending f (ballot + prefix count, no atomics), which every wave
//                    walks with a wave-uniform trip count.  Stores alpha and Q.
//   k_soft_backward  a wave owns an (image, face): it walks the pixels of the box in row-major order, lanes strided,
//                    recomputes D, takes G = g Q, sums the six xy gradients per lane, reduces them over the lanes in a
//                    fixed tree and stores the nine entries (z: 0).
// The float32 operation sequence of a pair (soft_pair) is the one tests/soft_ref.py counts its bounds from.  No atomics, no
// host synchronisation, every output element stored; the same bits in every run and for an image alone or inside a batch:
// a pixel's product depends on the boxes alone, never on the tile or the chunk a face arrives in.  The record, the box, the
// tile and the pair are nr_soft_pair.h's, one definition with nr_soft_render.hip.
#include "nr_soft_pair.h"

using namespace nr;

namespace {

// --------------------------------------------------------------------------------------------------------------------
// set-up

__global__ __launch_bounds__(256) void k_soft_setup(const float *__restrict__ faces, float4 *__restrict__ rec, int F, int S,
                                                    float reach, double near, double far)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    float c[9];
    soft_record<false>(faces + ((size_t)b * F + f) * 9, rec + ((size_t)b * F + f) * SOFT_REC, S, reach, near, far, c);
}

// --------------------------------------------------------------------------------------------------------------------
// forward

__global__ __launch_bounds__(256) void k_soft_forward(const float4 *__restrict__ rec, float *__restrict__ alpha,
                                                      float *__restrict__ trans, int F, int S, int tiles_x, float inv_sigma)
{
    __shared__ float4 list[SOFT_CHUNK * SOFT_REC];
    __shared__ int wave_count[4];
    const int b = blockIdx.y;
    const SoftTile T = soft_tile(S, tiles_x);
    const float4 *rb = rec + (size_t)b * F * SOFT_REC;
    float Q = 1.0f;
    for (int c0 = 0; c0 < F; c0 += SOFT_CHUNK) {
        // soft_filter_chunk<SOFT_REC>'s statements (nr_soft_pair.h), written out: as a call the compiler reuses r0's registers
        // in the walk below and waits for its load (vmcnt) once per listed face -- 0.4 to 0.8 % of the 64 x 64 rows, measured
        const int f = c0 + T.tid;
        float4 r0, r1, r2;
        bool hit = false;
        if (f < F) {
            r0 = rb[(size_t)f * SOFT_REC]; r1 = rb[(size_t)f * SOFT_REC + 1]; r2 = rb[(size_t)f * SOFT_REC + 2];
            const SoftFace s = unpack(r0, r1, r2);
            hit = s.on != 0 && s.ix_lo <= T.tx1 && s.ix_hi >= T.tx0 && s.iy_lo <= T.ty1 && s.iy_hi >= T.ty0;
        }
        const unsigned long long m = __ballot(hit);
        const int before = __popcll(m & ((1ull << T.lane) - 1ull));
        if (T.lane == 0) wave_count[T.wave] = __popcll(m);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int cnt = wave_count[w];
            base += w < T.wave ? cnt : 0;
            n += cnt;
        }
        if (hit) {   // thread order is face order: the list stays ascending in f
            const int at = (base + before) * SOFT_REC;   // < SOFT_CHUNK * SOFT_REC: at most one entry per thread
            list[at] = r0; list[at + 1] = r1; list[at + 2] = r2;
        }
        __syncthreads();
        n = rfl(n);
        for (int j = 0; j < n; j++) {
            const SoftFace s = unpack(list[j * SOFT_REC], list[j * SOFT_REC + 1], list[j * SOFT_REC + 2]);
            const SoftPair p = soft_pair(T.px, T.py, s, inv_sigma);
            const float q = Q * (1.0f / (1.0f + expf(p.x)));   // 1 - D as 1 / (1 + e^x), never as a subtraction
            Q = in_box(s, T.xi, T.yi) ? q : Q;
        }
        __syncthreads();   // the list and the counts are rewritten by the next chunk
    }
    if (T.xi < S && T.yi < S) {
        const size_t o = ((size_t)b * S + T.yi) * S + T.xi;
        alpha[o] = 1.0f - Q;
        trans[o] = Q;
    }
}

// --------------------------------------------------------------------------------------------------------------------
// backward

__global__ __launch_bounds__(256) void k_soft_backward(const float4 *__restrict__ rec, const float *__restrict__ trans,
                                                       const float *__restrict__ grad_alpha, float *__restrict__ grad_faces,
                                                       int F, int S, float inv_sigma)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int f = rfl(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (f >= F) return;
    const float4 *r = rec + ((size_t)b * F + f) * SOFT_REC;
    const SoftFace s = unpack(r[0], r[1], r[2]);
    float g0x = 0.0f, g0y = 0.0f, g1x = 0.0f, g1y = 0.0f, g2x = 0.0f, g2y = 0.0f;
    // the record's box lies inside the raster or is empty (k_soft_setup); clamped again, the workspace being the caller's
    const int x_lo = max(s.ix_lo, 0), x_hi = min(s.ix_hi, S - 1), y_lo = max(s.iy_lo, 0), y_hi = min(s.iy_hi, S - 1);
    if (s.on != 0 && x_lo <= x_hi && y_lo <= y_hi) {
        const int bw = x_hi - x_lo + 1, n = bw * (y_hi - y_lo + 1);   // <= S * S <= 2^28
        const float *qb = trans + (size_t)b * S * S, *gb = grad_alpha + (size_t)b * S * S;
        for (int i = lane; i < n; i += WAVE) {
            const int row = i / bw, xi = x_lo + (i - row * bw), yi = y_lo + row;
            const SoftPair p = soft_pair(pixel_center(xi, S), pixel_center(yi, S), s, inv_sigma);
            const size_t o = (size_t)yi * S + xi;
            const float G = gb[o] * qb[o];
            const float D = 1.0f / (1.0f + expf(-p.x));
            float C = (G * D) * inv_sigma;   // dL/dx / sigma; dx/dd2 = s / sigma
            C = p.inside ? C : -C;
            const float ca = (-2.0f * (1.0f - p.t)) * C, cb = (-2.0f * p.t) * C;
            const float ax = ca * p.rx, ay = ca * p.ry, bx = cb * p.rx, by = cb * p.ry;
            // one addition per entry and pixel (of an exact 0 for the third vertex): segment k runs from vertex k to k + 1
            const int k = p.k;
            g0x += k == 0 ? ax : (k == 2 ? bx : 0.0f);
            g0y += k == 0 ? ay : (k == 2 ? by : 0.0f);
            g1x += k == 1 ? ax : (k == 0 ? bx : 0.0f);
            g1y += k == 1 ? ay : (k == 0 ? by : 0.0f);
            g2x += k == 2 ? ax : (k == 1 ? bx : 0.0f);
            g2y += k == 2 ? ay : (k == 1 ? by : 0.0f);
        }
    }
    g0x = wave_sum(g0x); g0y = wave_sum(g0y);
    g1x = wave_sum(g1x); g1y = wave_sum(g1y);
    g2x = wave_sum(g2x); g2y = wave_sum(g2y);
    if (lane == 0) {
        float *o = grad_faces + ((size_t)b * F + f) * 9;
        o[0] = g0x; o[1] = g0y; o[2] = 0.0f;
        o[3] = g1x; o[4] = g1y; o[5] = 0.0f;
        o[6] = g2x; o[7] = g2y; o[8] = 0.0f;
    }
}

// --------------------------------------------------------------------------------------------------------------------
// host

size_t soft_workspace(int B, int F) { return (size_t)B * (size_t)F * SOFT_REC * sizeof(float4); }

int soft_args(int B, int F, int S, double sigma, double near, double far, const void *workspace, size_t workspace_bytes)
{
    if (!soft_sizes_ok(B, F, S)) return NR_E_SIZE;
    if (!(sigma >= 1.0e-30 && sigma <= 1.0e30) || near != near || far != far) return NR_E_MODE;   // (1 / sigma is a float)
    if (!workspace || workspace_bytes < soft_workspace(B, F)) return NR_E_WORKSPACE;
    return 0;
}

int soft_setup(const float *faces, int B, int F, int S, double sigma, double near, double far, void *workspace, hipStream_t st)
{
    hipLaunchKernelGGL(k_soft_setup, dim3((unsigned)((F + 255) / 256), (unsigned)B), dim3(256), 0, st, faces, (float4 *)workspace,
                       F, S, soft_reach(sigma), near, far);
    return launch_status();
}

}  // namespace

NR_API size_t nr_soft_silhouette_workspace_bytes(int32_t B, int32_t F, int32_t S)
{
    return soft_sizes_ok(B, F, S) ? soft_workspace(B, F) : 0;
}

NR_API int nr_soft_silhouette_forward(const float *faces, float *alpha, float *transmittance, int32_t B, int32_t F, int32_t S,
                                      double sigma, double near, double far, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    if (!faces || !alpha || !transmittance) return NR_E_NULL;
    if (int e = soft_args(B, F, S, sigma, near, far, workspace, workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = soft_setup(faces, B, F, S, sigma, near, far, workspace, st)) return rc;
    const int tiles = (S + SOFT_TILE - 1) / SOFT_TILE;
    hipLaunchKernelGGL(k_soft_forward, dim3((unsigned)(tiles * tiles), (unsigned)B), dim3(256), 0, st,
                       (const float4 *)workspace, alpha, transmittance, F, S, tiles, (float)(1.0 / sigma));
    return launch_status();
}

NR_API int nr_soft_silhouette_backward(const float *faces, const float *transmittance, const float *grad_alpha,
                                       float *grad_faces, int32_t B, int32_t F, int32_t S, double sigma, double near, double far,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (!faces || !transmittance || !grad_alpha || !grad_faces) return NR_E_NULL;
    if (int e = soft_args(B, F, S, sigma, near, far, workspace, workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = soft_setup(faces, B, F, S, sigma, near, far, workspace, st)) return rc;   // the caller's workspace holds nothing
    hipLaunchKernelGGL(k_soft_backward, dim3((unsigned)((F + 3) / 4), (unsigned)B), dim3(256), 0, st,
                       (const float4 *)workspace, transmittance, grad_alpha, grad_faces, F, S, (float)(1.0 / sigma));
    return launch_status();
}
