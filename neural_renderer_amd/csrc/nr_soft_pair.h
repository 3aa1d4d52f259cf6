// nr_soft_pair.h -- what nr_soft_silhouette.hip and nr_soft_render.hip share, one definition each so that the two cannot drift
// apart: the constants, the base record with the contribution rules and the BOX (soft_record: "the same bits for an image alone
// or inside a batch" rests on the boxes being one rule), the forward's tile (soft_tile) and chunk filter (soft_filter_chunk),
// the (pixel, face) pair (soft_pair: its float32 operation sequence is the one tests/soft_ref.py and tests/soft_render_ref.py
// count their bounds from) and the host's soft_reach and soft_sizes_ok.
#pragma once
#include "nr_device.h"

namespace nr {

constexpr int SOFT_TILE = 16;        // pixels per side of a forward workgroup's tile (a wave: 8 x 8)
constexpr int SOFT_CHUNK = 256;      // face records per LDS chunk, one per thread
constexpr int SOFT_REC = 3;          // float4 of the base record, which every soft record starts with
constexpr float SOFT_REACH = 17.0f;  // the box reaches sqrt(SOFT_REACH sigma) beyond the bounding box (the colours' cutoff in d2)
constexpr int SOFT_MAX_F = 1 << 24;

// a face's base record: (x0, y0, x1, y1), (x2, y2, ix_lo, iy_lo), (ix_hi, iy_hi, contributes, 0); the box in pixel indices,
// clamped to the raster, lo > hi = empty
struct SoftFace {
    float x0, y0, x1, y1, x2, y2;
    int ix_lo, iy_lo, ix_hi, iy_hi, on;
};

__device__ __forceinline__ SoftFace unpack(const float4 &a, const float4 &b, const float4 &c)
{
    SoftFace r;
    r.x0 = a.x; r.y0 = a.y; r.x1 = a.z; r.y1 = a.w;
    r.x2 = b.x; r.y2 = b.y;
    r.ix_lo = __float_as_int(b.z); r.iy_lo = __float_as_int(b.w);
    r.ix_hi = __float_as_int(c.x); r.iy_hi = __float_as_int(c.y);
    r.on = __float_as_int(c.z);
    return r;
}

// the base record of the face at v (nine floats, handed back in c) into o[0..2]: it contributes iff the nine are finite, near
// <= z <= far at the three vertices and, with AREA_RULE, the doubled area is not 0; the box is the bounding box grown by reach
template <bool AREA_RULE>
__device__ __forceinline__ void soft_record(const float *__restrict__ v, float4 *__restrict__ o, int S, float reach, double near,
                                            double far, float (&c)[9])
{
#pragma unroll
    for (int k = 0; k < 9; k++) c[k] = v[k];
    bool on = true;
#pragma unroll
    for (int k = 0; k < 9; k++) on = on && (fabsf(c[k]) < __builtin_inff());   // false for a NaN too
#pragma unroll
    for (int k = 2; k < 9; k += 3) on = on && (double)c[k] >= near && (double)c[k] <= far;
    if constexpr (AREA_RULE) {
        // the doubled area in double: the differences and products of floats are exact there, one rounding in the subtraction
        const double area = ((double)c[3] - (double)c[0]) * ((double)c[7] - (double)c[1]) -
                            ((double)c[6] - (double)c[0]) * ((double)c[4] - (double)c[1]);
        on = on && area != 0.0;
    }
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
    o[0] = make_float4(c[0], c[1], c[3], c[4]);
    o[1] = make_float4(c[6], c[7], __int_as_float(ix_lo), __int_as_float(iy_lo));
    o[2] = make_float4(__int_as_float(ix_hi), __int_as_float(iy_hi), __int_as_float(on ? 1 : 0), 0.0f);
}

// a forward workgroup of four waves owns the tile blockIdx.x of tiles_x per row, [tx0, tx1] x [ty0, ty1] clipped to the raster,
// a wave an 8 x 8 quarter, a lane the pixel (xi, yi) with the centre (px, py) -- clamped: a lane beyond the raster stores nothing
struct SoftTile {
    int tid, wave, lane, tx0, ty0, tx1, ty1, xi, yi;
    float px, py;
};

__device__ __forceinline__ SoftTile soft_tile(int S, int tiles_x)
{
    SoftTile T;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    T.tid = threadIdx.x; T.wave = T.tid >> 6; T.lane = T.tid & 63;
    T.tx0 = tile_x * SOFT_TILE; T.ty0 = tile_y * SOFT_TILE;
    T.tx1 = min(T.tx0 + SOFT_TILE - 1, S - 1); T.ty1 = min(T.ty0 + SOFT_TILE - 1, S - 1);
    T.xi = T.tx0 + (T.wave & 1) * 8 + (T.lane & 7); T.yi = T.ty0 + (T.wave >> 1) * 8 + (T.lane >> 3);
    T.px = pixel_center(min(T.xi, S - 1), S); T.py = pixel_center(min(T.yi, S - 1), S);
    return T;
}

// the records c0 .. c0 + SOFT_CHUNK - 1 of rb (REC float4 each, one per thread) into the compact LDS list of those whose box
// meets the tile, ascending in f -> their number.  k_soft_forward holds the same statements written out (the reason is there)
template <int REC>
__device__ __forceinline__ int soft_filter_chunk(const float4 *__restrict__ rb, int c0, int F, const SoftTile &T, float4 *list,
                                                 int *wave_count)
{
    const int f = c0 + T.tid;
    float4 r0, r1, r2, r3, r4, r5, r6;   // (named, not an array: an array indexed in a loop ends up in scratch or LDS)
    bool hit = false;
    if (f < F) {
        const float4 *src = rb + (size_t)f * REC;
        r0 = src[0]; r1 = src[1]; r2 = src[2];
        if constexpr (REC > 3) r3 = src[3];
        if constexpr (REC > 4) r4 = src[4];
        if constexpr (REC > 5) r5 = src[5];
        if constexpr (REC > 6) r6 = src[6];
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
        const int at = (base + before) * REC;   // < SOFT_CHUNK * REC: at most one entry per thread
        list[at] = r0; list[at + 1] = r1; list[at + 2] = r2;
        if constexpr (REC > 3) list[at + 3] = r3;
        if constexpr (REC > 4) list[at + 4] = r4;
        if constexpr (REC > 5) list[at + 5] = r5;
        if constexpr (REC > 6) list[at + 6] = r6;
    }
    __syncthreads();
    return rfl(n);
}

// one segment a -> b against the pixel p: the clamped parameter t of the nearest point c = a + t (b - a), r = p - c taken as
// (1 - t) (p - a) + t (p - b) -- the roundings stay relative to the distances to the two ends, not to the coordinates, and
// an end takes its share of the gradient, (1 - t) or t, without a cancellation --, d2 = |r|^2, and the edge function cr of p
__device__ __forceinline__ void soft_segment(float px, float py, float ax, float ay, float bx, float by, float &d2, float &t,
                                             float &rx, float &ry, float &cr)
{
    const float ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay, vx = px - bx, vy = py - by;
    const float dot = wx * ex + wy * ey, ee = ex * ex + ey * ey;
    t = ee > 0.0f ? dot / ee : 0.0f;   // a zero-length segment gives its endpoint
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float t1 = 1.0f - t;
    rx = t1 * wx + t * vx;
    ry = t1 * wy + t * vy;
    d2 = rx * rx + ry * ry;
    cr = ex * wy - ey * wx;
}

// the pair (p, face): x = s d2 / sigma, the side itself (d2 / sigma may underflow to 0 and lose the sign), the chosen segment
// k (the lowest on a tie), its t and r
struct SoftPair {
    float x, t, rx, ry;
    int k;
    bool inside;
};

__device__ __forceinline__ SoftPair soft_pair(float px, float py, const SoftFace &f, float inv_sigma)
{
    float d0, t0, rx0, ry0, c0, d1, t1, rx1, ry1, c1, d2, t2, rx2, ry2, c2;
    soft_segment(px, py, f.x0, f.y0, f.x1, f.y1, d0, t0, rx0, ry0, c0);
    soft_segment(px, py, f.x1, f.y1, f.x2, f.y2, d1, t1, rx1, ry1, c1);
    soft_segment(px, py, f.x2, f.y2, f.x0, f.y0, d2, t2, rx2, ry2, c2);
    SoftPair p;
    const bool s1 = d1 < d0;   // strict: the lowest segment wins a tie
    const float da = s1 ? d1 : d0;
    const bool s2 = d2 < da;
    const float d = s2 ? d2 : da;
    p.k = s2 ? 2 : (s1 ? 1 : 0);
    p.t = s2 ? t2 : (s1 ? t1 : t0);
    p.rx = s2 ? rx2 : (s1 ? rx1 : rx0);
    p.ry = s2 ? ry2 : (s1 ? ry1 : ry0);
    const bool inside = (c0 > 0.0f && c1 > 0.0f && c2 > 0.0f) || (c0 < 0.0f && c1 < 0.0f && c2 < 0.0f);
    const float v = d * inv_sigma;
    p.inside = inside;
    p.x = inside ? v : -v;
    return p;
}

__device__ __forceinline__ bool in_box(const SoftFace &f, int xi, int yi)
{
    return xi >= f.ix_lo && xi <= f.ix_hi && yi >= f.iy_lo && yi <= f.iy_hi;
}

// host: the box's reach in NDC (the margin covers the roundings of this line), and the sizes every soft entry takes
inline float soft_reach(double sigma) { return sqrtf(SOFT_REACH * (float)sigma) * 1.0001f; }

inline bool soft_sizes_ok(int B, int F, int S) { return check_sizes(B, F, S) == 0 && F <= SOFT_MAX_F; }

}  // namespace nr
