// nr_soft_pair.h -- the (pixel, face) pair of the soft operators: the face record's first 48 bytes, the nearest segment, the
// side and x = s d2 / sigma.  One definition for nr_soft_silhouette.hip and nr_soft_render.hip, so that the two cannot drift
// apart: the float32 operation sequence here is the one tests/soft_ref.py and tests/soft_render_ref.py count their bounds from.
#pragma once
#include "nr_device.h"

namespace nr {

// a face's record: (x0, y0, x1, y1), (x2, y2, ix_lo, iy_lo), (ix_hi, iy_hi, contributes, 0); the box in pixel indices,
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

}  // namespace nr
