// nr_solid_angle.h -- the signed solid angle of a triangle seen from a point: ONE definition for the three sweeps of
// nr_winding.hip (DESIGN "Winding numbers"), so that a (point, face) pair has the same bits whichever kernel evaluates it.
//
//   A = v0 - p, B = v1 - p, C = v2 - p, la, lb, lc their lengths
//   num = A . (B x C)
//   den = la lb lc + (A . B) lc + (B . C) la + (C . A) lb
//   Omega = 2 atan2(num, den)                                  (van Oosterom-Strackee)
// and its exact derivative, with s = num^2 + den^2:
//   dOmega = 2 (den dnum - num dden) / s
//   dnum/dA = B x C, dnum/dB = C x A, dnum/dC = A x B
//   dden/dA = (A / la) (lb lc + B . C) + B lc + C lb, cyclic for B and C;  d/dp = -(d/dA + d/dB + d/dC)
// Edge rules: num = den = 0 (the point on a vertex) gives Omega = 0 and a zero gradient; la = 0 uses A / la := 0; a face with two
// corners equal as positions is marked in its record and is skipped by the sweeps (exactly 0 to the value and to every
// gradient); a face or a point with a non-finite coordinate gets x = NaN, so every pair with it is NaN.  No epsilon anywhere:
// a scene scaled by a power of two has the same num / den ratio bits.
//
// The float32 operation order (no contraction): dot(p, q) = (p0 q0 + p1 q1) + p2 q2; cross(p, q) = (p1 q2 - p2 q1, p2 q0 - p0 q2,
// p0 q1 - p1 q0); length = sqrtf(dot) (correctly rounded: build flags);
//   den = (((la lb) lc + ab lc) + bc la) + ca lb,  ab = dot(A, B), bc = dot(B, C), ca = dot(C, A)
//   gradient: kn = (2 den) / s, kd = (2 num) / s, s = num num + den den;  ila = la > 0 ? 1 / la : 0;
//             ddenA = ((A ila) (lb lc + bc) + B lc) + C lb;  gA = kn (B x C) - kd ddenA;  gp = -((gA + gB) + gC).
#pragma once
#include "nr_device.h"
#include "nr_shade.h"

namespace nr {

// 12 floats = three 16-byte words: read from LDS as three broadcast ds_read_b128 (a three-float read would be a ds_read_b96)
struct SaRecord {
    float4 v0_skip;  // v0 (x = NaN when a corner is not finite), w != 0: the face is skipped
    float4 v1;       // v1, 0
    float4 v2;       // v2, 0
};
constexpr int SA_RECORD_WORDS = 3;

struct SaPair {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    float la, lb, lc, ab, bc, ca;
    float num, den;
};

__device__ __forceinline__ float sa_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ bool sa_finite(float x) { return fabsf(x) <= 3.402823466e38f; }

// the x coordinate of a point, NaN when one of its coordinates is not finite
__device__ __forceinline__ float sa_point_x(float x, float y, float z)
{
    return sa_finite(x) && sa_finite(y) && sa_finite(z) ? x : __builtin_nanf("");
}

__device__ __forceinline__ SaRecord sa_record(const float w[3][3])
{
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) finite = finite && sa_finite(w[k][c]);
    const bool e01 = w[0][0] == w[1][0] && w[0][1] == w[1][1] && w[0][2] == w[1][2];
    const bool e12 = w[1][0] == w[2][0] && w[1][1] == w[2][1] && w[1][2] == w[2][2];
    const bool e20 = w[2][0] == w[0][0] && w[2][1] == w[0][1] && w[2][2] == w[0][2];
    SaRecord R;
    R.v0_skip = make_float4(finite ? w[0][0] : __builtin_nanf(""), w[0][1], w[0][2], e01 || e12 || e20 ? 1.0f : 0.0f);
    R.v1 = make_float4(w[1][0], w[1][1], w[1][2], 0.0f);
    R.v2 = make_float4(w[2][0], w[2][1], w[2][2], 0.0f);
    return R;
}

__device__ __forceinline__ SaPair sa_pair(const SaRecord &R, float px, float py, float pz)
{
    SaPair P;
    P.ax = R.v0_skip.x - px; P.ay = R.v0_skip.y - py; P.az = R.v0_skip.z - pz;
    P.bx = R.v1.x - px; P.by = R.v1.y - py; P.bz = R.v1.z - pz;
    P.cx = R.v2.x - px; P.cy = R.v2.y - py; P.cz = R.v2.z - pz;
    P.la = sqrtf(sa_dot(P.ax, P.ay, P.az, P.ax, P.ay, P.az));
    P.lb = sqrtf(sa_dot(P.bx, P.by, P.bz, P.bx, P.by, P.bz));
    P.lc = sqrtf(sa_dot(P.cx, P.cy, P.cz, P.cx, P.cy, P.cz));
    const float nx = P.by * P.cz - P.bz * P.cy, ny = P.bz * P.cx - P.bx * P.cz, nz = P.bx * P.cy - P.by * P.cx;
    P.num = sa_dot(P.ax, P.ay, P.az, nx, ny, nz);
    P.ab = sa_dot(P.ax, P.ay, P.az, P.bx, P.by, P.bz);
    P.bc = sa_dot(P.bx, P.by, P.bz, P.cx, P.cy, P.cz);
    P.ca = sa_dot(P.cx, P.cy, P.cz, P.ax, P.ay, P.az);
    P.den = (((P.la * P.lb) * P.lc + P.ab * P.lc) + P.bc * P.la) + P.ca * P.lb;
    return P;
}

__device__ __forceinline__ float sa_omega(const SaPair &P)
{
    return P.num == 0.0f && P.den == 0.0f ? 0.0f : 2.0f * atan2f(P.num, P.den);
}

__device__ __forceinline__ float sa_inv_length(float l) { return l > 0.0f ? 1.0f / l : 0.0f; }

// dOmega/dv0, dOmega/dv1, dOmega/dv2 of a pair; dOmega/dp = -((g0 + g1) + g2) per component
__device__ __forceinline__ void sa_gradient(const SaPair &P, float g0[3], float g1[3], float g2[3])
{
    const float s = P.num * P.num + P.den * P.den;
    const bool zero = s == 0.0f;
    const float kn = zero ? 0.0f : (2.0f * P.den) / s, kd = zero ? 0.0f : (2.0f * P.num) / s;
    const float A[3] = {P.ax, P.ay, P.az}, B[3] = {P.bx, P.by, P.bz}, C[3] = {P.cx, P.cy, P.cz};
    const float ila = sa_inv_length(P.la), ilb = sa_inv_length(P.lb), ilc = sa_inv_length(P.lc);
    const float ma = P.lb * P.lc + P.bc, mb = P.lc * P.la + P.ca, mc = P.la * P.lb + P.ab;
    float nA[3], nB[3], nC[3];
    cross3(B, C, nA);
    cross3(C, A, nB);
    cross3(A, B, nC);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float dA = ((A[c] * ila) * ma + B[c] * P.lc) + C[c] * P.lb;
        const float dB = ((B[c] * ilb) * mb + C[c] * P.la) + A[c] * P.lc;
        const float dC = ((C[c] * ilc) * mc + A[c] * P.lb) + B[c] * P.la;
        g0[c] = zero ? 0.0f : kn * nA[c] - kd * dA;
        g1[c] = zero ? 0.0f : kn * nB[c] - kd * dB;
        g2[c] = zero ? 0.0f : kn * nC[c] - kd * dC;
    }
}

}  // namespace nr
