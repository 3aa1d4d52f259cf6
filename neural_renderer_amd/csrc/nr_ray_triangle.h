// nr_ray_triangle.h -- whether and where a ray meets a triangle: ONE definition for the sweep, the merge and the finish of
// nr_ray_mesh.hip (DESIGN "Ray casting"), so that a (ray, face) pair has the same bits wherever it is evaluated.  It is restated
// in torch (neural_renderer_amd/ray_mesh.py `_pair_torch`) and in float64 NumPy (tests/ray_ref.py).
//
// Moeller-Trumbore with the sign taken out and the division put last.  For the ray o + t d (d NOT normalised, so t counts in
// lengths of d) and the face (v0, v1, v2):
//   e1 = v1 - v0;  e2 = v2 - v0;                       (the record: v0, e1, e2 -- three 16-byte words, one spare float each)
//   pvec = d x e2;  det = e1 . pvec;  tvec = o - v0;  qvec = tvec x e1;
//   s = sign(det);  D = |det|;  U = s (tvec . pvec);  V = s (d . qvec);  T = s (e2 . qvec).
// The pair is a hit iff  D > 0,  U >= 0,  V >= 0,  U + V <= D  (all on the undivided numerators), with `cull` det > 0, and
// near <= t < far for t = T / D.  The one division per quantity is made only for pairs that passed the inside test.  The
// weights of the hit point are w1 = U / D, w2 = V / D, w0 = max((1 - w1) - w2, 0): they sum to 1 within 3 ulp.
// Every comparison fails for a NaN, so a NaN ray misses everything; a face with a non-finite corner gets v0.x = NaN, which
// makes tvec.x, hence U (tvec.x enters it as a product, and NaN * 0 is NaN), NaN: it is never hit.  A collapsed face, or one
// parallel to the ray, has D = 0 and is never hit.  Shared edges are NOT watertight: U, V and D of the two faces of an edge
// are rounded independently, so a ray through the edge may hit both (the lower t, then the lower face, wins) or neither.
//
// The float32 operation order (no contraction): dot(p, q) = (p0 q0 + p1 q1) + p2 q2;  (p x q)_0 = p1 q2 - p2 q1, cyclic.
#pragma once
#include "nr_device.h"

namespace nr {

struct RayRecord {
    float4 v0;  // v0 (x = NaN on a face with a non-finite corner), spare
    float4 e1;  // v1 - v0, spare
    float4 e2;  // v2 - v0, spare
};
constexpr int RAY_RECORD_WORDS = 3;

__device__ __forceinline__ float rt_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ RayRecord ray_record(const float w[3][3])
{
    RayRecord R;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) finite = finite && (fabsf(w[k][c]) <= 3.402823466e38f);
    R.v0 = make_float4(finite ? w[0][0] : __builtin_nanf(""), w[0][1], w[0][2], 0.0f);
    R.e1 = make_float4(w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2], 0.0f);
    R.e2 = make_float4(w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2], 0.0f);
    return R;
}

struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

// t of the pair when it is a hit within [near, far), else +inf (which never wins a strict <).  WEIGHTS: also the barycentric
// weights of the hit point (left alone on a miss).
template <bool WEIGHTS>
__device__ __forceinline__ float ray_triangle(const RayRecord &R, const Ray &r, float near, float far, bool cull, float *wout)
{
    const float px = r.dy * R.e2.z - r.dz * R.e2.y, py = r.dz * R.e2.x - r.dx * R.e2.z, pz = r.dx * R.e2.y - r.dy * R.e2.x;
    const float det = rt_dot(R.e1.x, R.e1.y, R.e1.z, px, py, pz);
    const float tx = r.ox - R.v0.x, ty = r.oy - R.v0.y, tz = r.oz - R.v0.z;
    const float qx = ty * R.e1.z - tz * R.e1.y, qy = tz * R.e1.x - tx * R.e1.z, qz = tx * R.e1.y - ty * R.e1.x;
    const float u = rt_dot(tx, ty, tz, px, py, pz), v = rt_dot(r.dx, r.dy, r.dz, qx, qy, qz);
    const bool neg = det < 0.0f;
    const float D = fabsf(det), U = neg ? -u : u, V = neg ? -v : v;
    const float inf = __builtin_inff();
    if (!(D > 0.0f && U >= 0.0f && V >= 0.0f && U + V <= D) || (cull && neg)) return inf;
    const float tt = rt_dot(R.e2.x, R.e2.y, R.e2.z, qx, qy, qz);
    const float t = (neg ? -tt : tt) / D;
    if (!(t >= near && t < far)) return inf;
    if (WEIGHTS) {
        const float w1 = U / D, w2 = V / D;
        wout[0] = fmaxf((1.0f - w1) - w2, 0.0f);
        wout[1] = w1;
        wout[2] = w2;
    }
    return t;
}

}  // namespace nr
