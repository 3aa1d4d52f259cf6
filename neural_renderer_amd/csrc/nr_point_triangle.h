// nr_point_triangle.h -- the closest point of a triangle to a point: ONE definition for both sweeps of nr_point_mesh.hip
// (DESIGN "Point-to-mesh distance"), so that a (point, face) pair has the same bits whichever sweep evaluates it.
//
// Not the textbook region walk: on a face with a repeated vertex or collinear vertices that walk returns a corner where the
// closest point lies inside a segment.  Here a face is a record of per-face invariants, and a pair takes the smallest of four
// candidates, every one the honest distance to a point OF the triangle, with no divergent regions and no division:
//   the three edge segments   t = clamp(e . (p - u) * inv|e|^2, 0, 1), inv|e|^2 = 0 when |e|^2 = 0 (then t = 0);
//   the in-plane projection   y = (g . ap) inv|g|^2,  x = (ab . ap - y (ab . ac)) inv|ab|^2,  g = ac - ((ab . ac) inv|ab|^2) ab
//                             (Gram-Schmidt: the point is x ab + y ac), taken only when x >= 0, y >= 0, x + y <= 1 hold --
//                             they fail for a NaN, and inv|g|^2 = 0 puts the candidate on segment ab when the Gram
//                             determinant |ab|^2 |g|^2 is not positive.
// The candidates are compared with a strict < in the order ab, ac, bc, plane.  On a face without area this is exactly the
// distance to its segment or point.  The reciprocals are IEEE divisions made once per face (build flags: correctly rounded
// division); on the lattice case of the tests they are powers of two, so the products are the quotients.
//
// The float32 operation order (no contraction): dot(p, q) = (p0 q0 + p1 q1) + p2 q2;
//   record: ab = v1 - v0; ac = v2 - v0; e = v2 - v1; aa, cc, ee, bb = dot(ab, ab), dot(ac, ac), dot(e, e), dot(ab, ac);
//           inv_x = x > 0 ? 1 / x : 0;  g = ac - (bb inv_aa) ab;  gg = dot(g, g).  A face with a non-finite coordinate gets
//           a[0] = NaN: every candidate of every pair with it is then NaN, and a NaN never wins a strict <.
//   pair:   ap = p - a;  d1 = dot(ab, ap);  d2 = dot(ac, ap);
//           t1 = clamp(d1 inv_aa);  r = ap - t1 ab;                       s1 = dot(r, r)    weights (1 - t1, t1, 0)
//           t2 = clamp(d2 inv_cc);  r = ap - t2 ac;                       s2                (1 - t2, 0, t2)
//           bp = ap - ab;  t3 = clamp(dot(e, bp) inv_ee);  r = bp - t3 e; s3                (0, 1 - t3, t3)
//           y = dot(g, ap) inv_gg;  x = (d1 - y bb) inv_aa;  r = (ap - x ab) - y ac;  s4    (max((1 - x) - y, 0), x, y)
//   clamp(t) = fminf(fmaxf(t, 0), 1): 0 for a NaN.
// The residual of a pair for the gradients, from the weights the forward stored (envelope theorem: they carry no gradient):
//   r = ((p - v0) - w1 (v1 - v0)) - w2 (v2 - v0).
#pragma once
#include "nr_device.h"

namespace nr {

// 20 floats = five 16-byte words: read from LDS as five broadcast ds_read_b128 (a three-float read would be a ds_read_b96)
struct TriRecord {
    float4 a_iaa;   // a = v0,        1 / |ab|^2
    float4 ab_icc;  // ab,            1 / |ac|^2
    float4 ac_iee;  // ac,            1 / |e|^2
    float4 g_igg;   // g,             1 / |g|^2
    float4 e_bb;    // e = v2 - v1,   ab . ac
};
constexpr int TRI_RECORD_WORDS = 5;

__device__ __forceinline__ float pt_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}
__device__ __forceinline__ float pt_inv(float x) { return x > 0.0f ? 1.0f / x : 0.0f; }
__device__ __forceinline__ float pt_clamp01(float t) { return fminf(fmaxf(t, 0.0f), 1.0f); }

__device__ __forceinline__ TriRecord tri_record(const float w[3][3])
{
    TriRecord R;
    const float abx = w[1][0] - w[0][0], aby = w[1][1] - w[0][1], abz = w[1][2] - w[0][2];
    const float acx = w[2][0] - w[0][0], acy = w[2][1] - w[0][1], acz = w[2][2] - w[0][2];
    const float ex = w[2][0] - w[1][0], ey = w[2][1] - w[1][1], ez = w[2][2] - w[1][2];
    const float aa = pt_dot(abx, aby, abz, abx, aby, abz), cc = pt_dot(acx, acy, acz, acx, acy, acz);
    const float ee = pt_dot(ex, ey, ez, ex, ey, ez), bb = pt_dot(abx, aby, abz, acx, acy, acz);
    const float iaa = pt_inv(aa), m = bb * iaa;
    const float gx = acx - m * abx, gy = acy - m * aby, gz = acz - m * abz;
    const float gg = pt_dot(gx, gy, gz, gx, gy, gz);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) finite = finite && (fabsf(w[k][c]) <= 3.402823466e38f);
    R.a_iaa = make_float4(finite ? w[0][0] : __builtin_nanf(""), w[0][1], w[0][2], iaa);
    R.ab_icc = make_float4(abx, aby, abz, pt_inv(cc));
    R.ac_iee = make_float4(acx, acy, acz, pt_inv(ee));
    R.g_igg = make_float4(gx, gy, gz, pt_inv(gg));
    R.e_bb = make_float4(ex, ey, ez, bb);
    return R;
}

// dist2 of point p to the face of record R; with WEIGHTS also the barycentric weights of the closest point
template <bool WEIGHTS>
__device__ __forceinline__ float point_triangle(const TriRecord &R, float px, float py, float pz, float *wout)
{
    const float apx = px - R.a_iaa.x, apy = py - R.a_iaa.y, apz = pz - R.a_iaa.z;
    const float abx = R.ab_icc.x, aby = R.ab_icc.y, abz = R.ab_icc.z;
    const float acx = R.ac_iee.x, acy = R.ac_iee.y, acz = R.ac_iee.z;
    const float ex = R.e_bb.x, ey = R.e_bb.y, ez = R.e_bb.z;
    const float d1 = pt_dot(abx, aby, abz, apx, apy, apz), d2 = pt_dot(acx, acy, acz, apx, apy, apz);
    float rx, ry, rz;
    // segment ab
    const float t1 = pt_clamp01(d1 * R.a_iaa.w);
    rx = apx - t1 * abx; ry = apy - t1 * aby; rz = apz - t1 * abz;
    const float s1 = pt_dot(rx, ry, rz, rx, ry, rz);
    // segment ac
    const float t2 = pt_clamp01(d2 * R.ab_icc.w);
    rx = apx - t2 * acx; ry = apy - t2 * acy; rz = apz - t2 * acz;
    const float s2 = pt_dot(rx, ry, rz, rx, ry, rz);
    // segment bc
    const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const float t3 = pt_clamp01(pt_dot(ex, ey, ez, bpx, bpy, bpz) * R.ac_iee.w);
    rx = bpx - t3 * ex; ry = bpy - t3 * ey; rz = bpz - t3 * ez;
    const float s3 = pt_dot(rx, ry, rz, rx, ry, rz);
    // the projection onto the plane
    const float y = pt_dot(R.g_igg.x, R.g_igg.y, R.g_igg.z, apx, apy, apz) * R.g_igg.w;
    const float x = (d1 - y * R.e_bb.w) * R.a_iaa.w;
    rx = (apx - x * abx) - y * acx; ry = (apy - x * aby) - y * acy; rz = (apz - x * abz) - y * acz;
    const float s4 = pt_dot(rx, ry, rz, rx, ry, rz);
    const bool inside = x >= 0.0f && y >= 0.0f && x + y <= 1.0f;
    float best = s1;
    int which = 0;
    if (s2 < best) { best = s2; which = 1; }
    if (s3 < best) { best = s3; which = 2; }
    if (inside && s4 < best) { best = s4; which = 3; }
    if (WEIGHTS) {
        wout[0] = which == 0 ? 1.0f - t1 : (which == 1 ? 1.0f - t2 : (which == 2 ? 0.0f : fmaxf((1.0f - x) - y, 0.0f)));
        wout[1] = which == 0 ? t1 : (which == 1 ? 0.0f : (which == 2 ? 1.0f - t3 : x));
        wout[2] = which == 0 ? 0.0f : (which == 1 ? t2 : (which == 2 ? t3 : y));
    }
    return best;
}

// r = ((p - v0) - w1 (v1 - v0)) - w2 (v2 - v0), per component
__device__ __forceinline__ void point_triangle_residual(const float w[3][3], const float *p, float w1, float w2, float r[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = ((p[c] - w[0][c]) - w1 * (w[1][c] - w[0][c])) - w2 * (w[2][c] - w[0][c]);
}

}  // namespace nr
