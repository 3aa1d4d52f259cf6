// nr_soft_silhouette.hip -- soft silhouettes: distance-based coverage with its exact gradient (include/nr_hip.h; DESIGN
// "Soft silhouettes").
//
// Per contributing face f and pixel p: d2 = the squared distance of p to the nearest of the three edge segments (lowest
// segment on a tie), s = +1 strictly inside the triangle, else -1, x = s d2 / sigma, D = 1 / (1 + e^-x);
// Q_p = the product of 1 / (1 + e^x) in ascending f, alpha_p = 1 - Q_p.  A face contributes iff its nine coordinates are
// finite and near <= z <= far at its three vertices.  A (pixel, face) pair is taken iff the pixel lies in the face's BOX:
// the pixel range of the triangle's bounding box grown by sqrt(17 sigma); a pair outside it is outside the triangle with
// d2 > 17 sigma (D < 2^-24) and is left out of both directions.
//   k_soft_setup     (image, face) -> a 48-byte record: the six xy, the box, the flag
//   k_soft_forward   a workgroup of four waves owns a 16 x 16 pixel tile, a wave an 8 x 8 quarter of it, a lane a pixel.
//                    The records go through LDS in chunks of 256 (one per thread); those whose box meets the tile are kept
//                    in a compact list in ascending f (ballot + prefix count, no atomics), which every wave walks with a
//                    wave-uniform trip count.  Stores alpha and Q.
//   k_soft_backward  a wave owns an (image, face): it walks the pixels of the box in row-major order, lanes strided,
//                    recomputes D, takes G = g Q, sums the six xy gradients per lane, reduces them over the lanes in a
//                    fixed tree and stores the nine entries (z: 0).
// The float32 operation sequence of a pair (soft_pair) is the one tests/soft_ref.py counts its bounds from.  No atomics, no
// host synchronisation, every output element stored; the same bits in every run and for an image alone or inside a batch:
// a pixel's product depends on the boxes alone, never on the tile or the chunk a face arrives in.
#include "nr_soft_pair.h"

using namespace nr;

namespace {

constexpr int SOFT_TILE = 16;      // pixels per side of a workgroup's tile (a wave: 8 x 8)
constexpr int SOFT_CHUNK = 256;    // face records per LDS chunk, one per thread
constexpr int SOFT_REC = 3;        // float4 per record
constexpr float SOFT_REACH = 17.0f;  // the box reaches sqrt(SOFT_REACH sigma) beyond the triangle's bounding box
constexpr int SOFT_MAX_F = 1 << 24;

// SoftFace / unpack / soft_segment / soft_pair / in_box: nr_soft_pair.h, shared with nr_soft_render.hip

// --------------------------------------------------------------------------------------------------------------------
// set-up

__global__ __launch_bounds__(256) void k_soft_setup(const float *__restrict__ faces, float4 *__restrict__ rec, int F, int S,
                                                    float reach, double near, double far)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const float *v = faces + ((size_t)b * F + f) * 9;
    float c[9];
#pragma unroll
    for (int k = 0; k < 9; k++) c[k] = v[k];
    bool on = true;
#pragma unroll
    for (int k = 0; k < 9; k++) on = on && (fabsf(c[k]) < __builtin_inff());   // false for a NaN too
#pragma unroll
    for (int k = 2; k < 9; k += 3) on = on && (double)c[k] >= near && (double)c[k] <= far;
    int ix_lo = S, iy_lo = S, ix_hi = -1, iy_hi = -1;   // empty
    if (on) {
        const float fs = (float)S;
        const float xmin = fminf(fminf(c[0], c[3]), c[6]) - reach, xmax = fmaxf(fmaxf(c[0], c[3]), c[6]) + reach;
        const float ymin = fminf(fminf(c[1], c[4]), c[7]) - reach, ymax = fmaxf(fmaxf(c[1], c[4]), c[7]) + reach;
        // pixel i has its centre at NDC (2 i + 1 - S) / S, i.e. NDC v lies at pixel coordinate to_pixel(v); floor below and
        // ceil above keep up to a pixel more than needed, which only adds pairs.  Clamped before the conversion to int.
        const float lo_c = -1.0f, hi_c = fs;
        ix_lo = max((int)floorf(fminf(fmaxf(to_pixel(xmin, fs), lo_c), hi_c)), 0);
        ix_hi = min((int)ceilf(fminf(fmaxf(to_pixel(xmax, fs), lo_c), hi_c)), S - 1);
        iy_lo = max((int)floorf(fminf(fmaxf(to_pixel(ymin, fs), lo_c), hi_c)), 0);
        iy_hi = min((int)ceilf(fminf(fmaxf(to_pixel(ymax, fs), lo_c), hi_c)), S - 1);
        if (ix_lo > ix_hi || iy_lo > iy_hi) { ix_lo = iy_lo = S; ix_hi = iy_hi = -1; }
    }
    float4 *o = rec + ((size_t)b * F + f) * SOFT_REC;
    o[0] = make_float4(c[0], c[1], c[3], c[4]);
    o[1] = make_float4(c[6], c[7], __int_as_float(ix_lo), __int_as_float(iy_lo));
    o[2] = make_float4(__int_as_float(ix_hi), __int_as_float(iy_hi), __int_as_float(on ? 1 : 0), 0.0f);
}

// --------------------------------------------------------------------------------------------------------------------
// forward

__global__ __launch_bounds__(256) void k_soft_forward(const float4 *__restrict__ rec, float *__restrict__ alpha,
                                                      float *__restrict__ trans, int F, int S, int tiles_x, float inv_sigma)
{
    __shared__ float4 list[SOFT_CHUNK * SOFT_REC];
    __shared__ int wave_count[4];
    const int b = blockIdx.y, tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx0 = tile_x * SOFT_TILE, ty0 = tile_y * SOFT_TILE;
    const int tx1 = min(tx0 + SOFT_TILE - 1, S - 1), ty1 = min(ty0 + SOFT_TILE - 1, S - 1);
    const int xi = tx0 + (wave & 1) * 8 + (lane & 7), yi = ty0 + (wave >> 1) * 8 + (lane >> 3);
    const float px = pixel_center(min(xi, S - 1), S), py = pixel_center(min(yi, S - 1), S);
    const float4 *rb = rec + (size_t)b * F * SOFT_REC;
    float Q = 1.0f;
    for (int c0 = 0; c0 < F; c0 += SOFT_CHUNK) {
        const int f = c0 + tid;
        float4 r0, r1, r2;
        bool hit = false;
        if (f < F) {
            r0 = rb[(size_t)f * SOFT_REC];
            r1 = rb[(size_t)f * SOFT_REC + 1];
            r2 = rb[(size_t)f * SOFT_REC + 2];
            const SoftFace s = unpack(r0, r1, r2);
            hit = s.on != 0 && s.ix_lo <= tx1 && s.ix_hi >= tx0 && s.iy_lo <= ty1 && s.iy_hi >= ty0;
        }
        const unsigned long long m = __ballot(hit);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_count[wave] = __popcll(m);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int cnt = wave_count[w];
            base += w < wave ? cnt : 0;
            n += cnt;
        }
        if (hit) {   // thread order is face order: the list stays ascending in f
            const int at = (base + before) * SOFT_REC;   // < SOFT_CHUNK * SOFT_REC: at most one entry per thread
            list[at] = r0;
            list[at + 1] = r1;
            list[at + 2] = r2;
        }
        __syncthreads();
        n = rfl(n);
        for (int j = 0; j < n; j++) {
            const SoftFace s = unpack(list[j * SOFT_REC], list[j * SOFT_REC + 1], list[j * SOFT_REC + 2]);
            const SoftPair p = soft_pair(px, py, s, inv_sigma);
            const float q = Q * (1.0f / (1.0f + expf(p.x)));   // 1 - D as 1 / (1 + e^x), never as a subtraction
            Q = in_box(s, xi, yi) ? q : Q;
        }
        __syncthreads();   // the list and the counts are rewritten by the next chunk
    }
    if (xi < S && yi < S) {
        const size_t o = ((size_t)b * S + yi) * S + xi;
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

bool soft_sizes_ok(int B, int F, int S) { return check_sizes(B, F, S) == 0 && F <= SOFT_MAX_F; }

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
    const float reach = sqrtf(SOFT_REACH * (float)sigma) * 1.0001f;   // (the margin covers the roundings of this line)
    hipLaunchKernelGGL(k_soft_setup, dim3((unsigned)((F + 255) / 256), (unsigned)B), dim3(256), 0, st, faces, (float4 *)workspace,
                       F, S, reach, near, far);
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
