// nr_mesh_losses.hip -- the two shape priors of a mesh fit (include/nr_hip.h; DESIGN "Mesh losses"): the uniform Laplacian
// loss and the flatness (dihedral angle) loss on world-space vertices [B, Nv, 3], one topology for the whole call.
//
// Every sum over the neighbourhood of a vertex is a GATHER through a host-built table in ascending order, and every sum
// over an image is reduced in the fixed order of nr_reduce.h: no float or double atomics in either direction, the same bits in
// every run.
//   k_laplacian_forward    (image, vertex): delta_v, stored for the backward; |delta_v|^2 summed per block in double
//   k_laplacian_backward   (image, vertex): the gather over N(v)
//   k_flatness_forward     (image, quad): (cos + 1)^2 summed per block in double
//   k_flatness_backward    (image, vertex): for each incident (quad, slot) in table order the quad's derivative is recomputed
//                          from its four vertices and the slot's share added -- no per-quad gradient buffer
//   k_loss_finish          (image): the blocks' partial sums in block order (ordered_sum), rounded once to loss[b]
//
// The float32 operation order (no contraction, correctly rounded division and square root: _build.HIPCC_FLAGS).
// dot(p, q) = (p0 q0 + p1 q1) + p2 q2 throughout.
//   Laplacian.  s = 0; s += x_u for u in N(v) in table order (per component); m = s / (float)deg; delta = x_v - m
//     (deg = 0: delta = 0).  The image's loss: (double)d0 d0 + (double)d1 d1 + (double)d2 d2 per vertex, in double.
//     Backward: t = 0; t += delta_u / (float)deg_u for u in N(v) in table order; grad = (2 g_b) * (delta_v - t).
//   Flatness, per quad (x0, x1 the edge, x2, x3 the opposite vertices), eps rounded to float once:
//     a = x1 - x0; b1 = x2 - x0; b2 = x3 - x0; A = dot(a, a) + eps; ab_i = dot(a, b_i); t_i = ab_i / A; c_i = b_i - t_i a;
//     n_i = dot(c_i, c_i); l_i = sqrt(n_i + eps); d = dot(c1, c2); D = l1 l2 + eps; cos = d / D; p = cos + 1;
//     the image's loss: (double)p p per quad, in double.
//     Backward, G = (2 g_b) p:  gd = G / D;  gD = -(G cos) / D;  h1 = (gD l2) / l1;  h2 = (gD l1) / l2  (= 2 d/dn_i);
//       gc1 = gd c2 + h1 c1;  gc2 = gd c1 + h2 c2;  gt_i = -dot(gc_i, a);  gab_i = gt_i / A;
//       gA = -(gt1 t1) / A - (gt2 t2) / A;
//       ga = ((((-t1) gc1 - t2 gc2) + gab1 b1) + gab2 b2) + (2 gA) a;   gb_i = gc_i + gab_i a;
//       slots: x1 <- ga, x2 <- gb1, x3 <- gb2, x0 <- -((ga + gb1) + gb2).
//     A vertex's gradient: 0, then += its slot's share of each incident quad in table order (ascending 4 q + slot).
//
// The edge-length loss and the cotangent Laplacian loss (DESIGN "Mesh losses: edge length and cotangent Laplacian"), on the same
// block sums and k_loss_finish:
//   k_edge_length_forward  (image, edge): (l - t)^2 summed per block in double
//   k_edge_length_backward (image, vertex): the gather over N(v); every edge recomputed from its two vertices, its target read
//                          through nbr_edge -- no per-edge gradient buffer
//   k_cot_weights          (image, face): the three cotangents of a face, cot [B, F, 3]
//   k_cot_apply            (image, vertex): L applied to a field [B, Nv, 3] through the vertex -> (face, corner) table with the
//                          stored weights; the forward's field is x (|H|^2 summed per block in double), the backward's is H
//   Edge length, per edge (v0 < v1) with target t:  d = x_v1 - x_v0;  n = dot(d, d);
//     no target tensor and t = 0: the image's loss adds (double)n;  else l = sqrt(n); r = l - t; the loss adds (double)r r.
//     Backward, vertex v: s = 0; for u in N(v) in table order: d = x_v - x_u; n = dot(d, d);
//       t = 0: s += d;  else l = sqrt(n); k = l > 0 ? (l - t) / l : 0; s += k d;     grad = (2 g_b) s.
//   Cotangents of face (i0, i1, i2) at corner c, eps rounded to float once:  a = x_(c+1) - x_c;  b = x_(c+2) - x_c;
//     n = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0);  cot_c = dot(a, b) / sqrt(dot(n, n) + eps);  a face with a repeated
//     index stores three zeros.
//   L(phi)_v: h = 0; for each (face, corner c) entry of v in table order (ascending 3 f + c), w = cot of that face:
//       p = phi_(c+1) - phi_v;  q = phi_(c+2) - phi_v;  h += w_(c+2) p + w_(c+1) q  (per component);
//     out = 0.5 h, or (0.5 h) (2 s_b) with a scale s.  Forward: H = L(x), the loss adds (double)H0 H0 + (double)H1 H1 +
//     (double)H2 H2 per vertex.  Backward: grad = L(H) with s = g: the weights are constants of the step, L is symmetric.
#include "nr_device.h"

using namespace nr;

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ float dot3f(const float *p, const float *q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

// block b's sum of v (nr_reduce.h: block_sum) into partial [B, gridDim.x]; every thread of the block must call it
__device__ __forceinline__ void store_block_sum(double v, double *__restrict__ partial, int b)
{
    const double s = block_sum<BLOCK>(v);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// partial [B, n_blocks] -> loss [B]: one thread per image adds its blocks in block order (n_blocks may be 0: loss = 0)
__global__ __launch_bounds__(BLOCK) void k_loss_finish(const double *__restrict__ partial, float *__restrict__ loss, int B,
                                                       int n_blocks)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    loss[b] = (float)ordered_sum(partial + (size_t)b * n_blocks, n_blocks, 1);
}

// --------------------------------------------------------------------------------------------------------------------
// Laplacian

// the neighbours of vertex v: [e0, e1) into nbr (clamped for memory safety; the host builds the table)
__device__ __forceinline__ void nbr_range(const int32_t *__restrict__ off, int v, int total, int &e0, int &e1)
{
    e0 = clampi(off[v], 0, total);
    e1 = clampi(off[v + 1], e0, total);
}

__global__ __launch_bounds__(BLOCK) void k_laplacian_forward(const float *__restrict__ x, const int32_t *__restrict__ off,
                                                             const int32_t *__restrict__ nbr, float *__restrict__ delta,
                                                             double *__restrict__ partial, int Nv, int total)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    double sq = 0.0;
    if (v < Nv) {
        const float *xb = x + (size_t)b * Nv * 3;
        int e0, e1;
        nbr_range(off, v, total, e0, e1);
        float s[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
        for (int e = e0; e < e1; e++) {
            const float *xu = xb + (size_t)clampi(nbr[e], 0, Nv - 1) * 3;
            s[0] += xu[0];
            s[1] += xu[1];
            s[2] += xu[2];
        }
        if (e1 > e0) {
            const float deg = (float)(e1 - e0);
            const float *xv = xb + (size_t)v * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) d[c] = xv[c] - s[c] / deg;
        }
        if (delta) {
            float *o = delta + ((size_t)b * Nv + v) * 3;
            o[0] = d[0];
            o[1] = d[1];
            o[2] = d[2];
        }
        sq = ((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1]) + (double)d[2] * (double)d[2];
    }
    store_block_sum(sq, partial, b);
}

__global__ __launch_bounds__(BLOCK) void k_laplacian_backward(const float *__restrict__ delta, const int32_t *__restrict__ off,
                                                              const int32_t *__restrict__ nbr,
                                                              const float *__restrict__ grad_loss,
                                                              float *__restrict__ grad_vertices, int Nv, int total)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= Nv) return;
    const float *db = delta + (size_t)b * Nv * 3;
    int e0, e1;
    nbr_range(off, v, total, e0, e1);
    float t[3] = {0.0f, 0.0f, 0.0f};
    for (int e = e0; e < e1; e++) {
        const int u = clampi(nbr[e], 0, Nv - 1);
        int u0, u1;
        nbr_range(off, u, total, u0, u1);
        const float deg = (float)max(u1 - u0, 1);  // (u has v as a neighbour: >= 1 in a table the host built)
        const float *du = db + (size_t)u * 3;
        t[0] += du[0] / deg;
        t[1] += du[1] / deg;
        t[2] += du[2] / deg;
    }
    const float g2 = 2.0f * grad_loss[b];
    const float *dv = db + (size_t)v * 3;
    float *o = grad_vertices + ((size_t)b * Nv + v) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = g2 * (dv[c] - t[c]);
}

// --------------------------------------------------------------------------------------------------------------------
// flatness

struct Quad {
    float a[3], b1[3], b2[3], c1[3], c2[3];
    float A, t1, t2, l1, l2, D, cosv;
};

// the forward of quad q of an image whose vertices are xb
__device__ __forceinline__ void quad_forward(const float *__restrict__ xb, const int32_t *__restrict__ quads, int q, int Nv,
                                             float eps, Quad &Q)
{
    const int32_t *qi = quads + (size_t)q * 4;
    const float *x0 = xb + (size_t)clampi(qi[0], 0, Nv - 1) * 3, *x1 = xb + (size_t)clampi(qi[1], 0, Nv - 1) * 3;
    const float *x2 = xb + (size_t)clampi(qi[2], 0, Nv - 1) * 3, *x3 = xb + (size_t)clampi(qi[3], 0, Nv - 1) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float p0 = x0[c];
        Q.a[c] = x1[c] - p0;
        Q.b1[c] = x2[c] - p0;
        Q.b2[c] = x3[c] - p0;
    }
    Q.A = dot3f(Q.a, Q.a) + eps;
    Q.t1 = dot3f(Q.a, Q.b1) / Q.A;
    Q.t2 = dot3f(Q.a, Q.b2) / Q.A;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        Q.c1[c] = Q.b1[c] - Q.t1 * Q.a[c];
        Q.c2[c] = Q.b2[c] - Q.t2 * Q.a[c];
    }
    Q.l1 = sqrtf(dot3f(Q.c1, Q.c1) + eps);
    Q.l2 = sqrtf(dot3f(Q.c2, Q.c2) + eps);
    Q.D = Q.l1 * Q.l2 + eps;
    Q.cosv = dot3f(Q.c1, Q.c2) / Q.D;
}

// the gradient of slot `slot` (0, 1: the edge; 2, 3: the opposite vertices) of a quad for the upstream g2 = 2 g_b
__device__ __forceinline__ void quad_backward(const Quad &Q, float g2, int slot, float out[3])
{
    const float G = g2 * (Q.cosv + 1.0f);
    const float gd = G / Q.D;
    const float gD = -(G * Q.cosv) / Q.D;
    const float gn1x2 = (gD * Q.l2) / Q.l1, gn2x2 = (gD * Q.l1) / Q.l2;  // 2 gn_i
    float gc1[3], gc2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        gc1[c] = gd * Q.c2[c] + gn1x2 * Q.c1[c];
        gc2[c] = gd * Q.c1[c] + gn2x2 * Q.c2[c];
    }
    const float gt1 = -dot3f(gc1, Q.a), gt2 = -dot3f(gc2, Q.a);
    const float gab1 = gt1 / Q.A, gab2 = gt2 / Q.A;
    const float gAx2 = 2.0f * (-(gt1 * Q.t1) / Q.A - (gt2 * Q.t2) / Q.A);
    float ga[3], gb1[3], gb2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        ga[c] = ((((-Q.t1) * gc1[c] - Q.t2 * gc2[c]) + gab1 * Q.b1[c]) + gab2 * Q.b2[c]) + gAx2 * Q.a[c];
        gb1[c] = gc1[c] + gab1 * Q.a[c];
        gb2[c] = gc2[c] + gab2 * Q.a[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
        out[c] = slot == 1 ? ga[c] : (slot == 2 ? gb1[c] : (slot == 3 ? gb2[c] : -((ga[c] + gb1[c]) + gb2[c])));
}

__global__ __launch_bounds__(BLOCK) void k_flatness_forward(const float *__restrict__ x, const int32_t *__restrict__ quads,
                                                            double *__restrict__ partial, int Nv, int E2, float eps)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    double term = 0.0;
    if (q < E2) {
        Quad Q;
        quad_forward(x + (size_t)b * Nv * 3, quads, q, Nv, eps, Q);
        const float p = Q.cosv + 1.0f;
        term = (double)p * (double)p;
    }
    store_block_sum(term, partial, b);
}

__global__ __launch_bounds__(BLOCK) void k_flatness_backward(const float *__restrict__ x, const int32_t *__restrict__ quads,
                                                             const int32_t *__restrict__ inc_off,
                                                             const int32_t *__restrict__ inc,
                                                             const float *__restrict__ grad_loss,
                                                             float *__restrict__ grad_vertices, int Nv, int E2, float eps)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= Nv) return;
    const float *xb = x + (size_t)b * Nv * 3;
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (E2 > 0) {
        const int total = 4 * E2;
        const int e0 = clampi(inc_off[v], 0, total), e1 = clampi(inc_off[v + 1], e0, total);
        const float g2 = 2.0f * grad_loss[b];
        for (int e = e0; e < e1; e++) {
            const int qs = clampi(inc[e], 0, total - 1);
            Quad Q;
            float o[3];
            quad_forward(xb, quads, qs >> 2, Nv, eps, Q);
            quad_backward(Q, g2, qs & 3, o);
            g[0] += o[0];
            g[1] += o[1];
            g[2] += o[2];
        }
    }
    float *out = grad_vertices + ((size_t)b * Nv + v) * 3;
    out[0] = g[0];
    out[1] = g[1];
    out[2] = g[2];
}

#ifdef NR_FLATNESS_BUFFER
// A measurement build only (-DNR_FLATNESS_BUFFER through _build.build_variant; scripts/mesh_losses_timing.py picks the library
// up from NR_HIP_LIB): the alternative the product does not take -- every quad's four gradients stored once, [B, E2, 4, 3],
// and gathered per vertex through the same table -- so that the two can be timed side by side.  The same bits as the
// recomputing kernel.  Its buffer is a process-wide allocation grown on demand, which is why this is no product path.
__global__ __launch_bounds__(BLOCK) void k_flatness_quad_grads(const float *__restrict__ x, const int32_t *__restrict__ quads,
                                                               const float *__restrict__ grad_loss, float *__restrict__ buf,
                                                               int Nv, int E2, float eps)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (q >= E2) return;
    Quad Q;
    quad_forward(x + (size_t)b * Nv * 3, quads, q, Nv, eps, Q);
    const float g2 = 2.0f * grad_loss[b];
    float *o = buf + ((size_t)b * E2 + q) * 12;
#pragma unroll
    for (int slot = 0; slot < 4; slot++) quad_backward(Q, g2, slot, o + 3 * slot);
}

__global__ __launch_bounds__(BLOCK) void k_flatness_gather(const int32_t *__restrict__ inc_off, const int32_t *__restrict__ inc,
                                                           const float *__restrict__ buf, float *__restrict__ grad_vertices,
                                                           int Nv, int E2)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= Nv) return;
    const int total = 4 * E2;
    const int e0 = clampi(inc_off[v], 0, total), e1 = clampi(inc_off[v + 1], e0, total);
    const float *bb = buf + (size_t)b * total * 3;
    float g[3] = {0.0f, 0.0f, 0.0f};
    for (int e = e0; e < e1; e++) {
        const float *o = bb + (size_t)clampi(inc[e], 0, total - 1) * 3;
        g[0] += o[0];
        g[1] += o[1];
        g[2] += o[2];
    }
    float *out = grad_vertices + ((size_t)b * Nv + v) * 3;
    out[0] = g[0];
    out[1] = g[1];
    out[2] = g[2];
}

float *quad_buffer(size_t bytes)
{
    static float *buf = nullptr;
    static size_t have = 0;
    if (bytes > have) {
        if (buf) (void)hipFree(buf);
        have = 0;
        if (hipMalloc((void **)&buf, bytes) != hipSuccess) return buf = nullptr;
        have = bytes;
    }
    return buf;
}
#endif

// --------------------------------------------------------------------------------------------------------------------
// edge length

// the target of edge e of image b: the tensor's entry ([E], or [B, E] with per_batch), or the call's number
__device__ __forceinline__ float edge_target(const float *__restrict__ target, int per_batch, float value, int b, int e, int E)
{
    return target ? target[(per_batch ? (size_t)b * E : (size_t)0) + e] : value;
}

__global__ __launch_bounds__(BLOCK) void k_edge_length_forward(const float *__restrict__ x, const int32_t *__restrict__ edges,
                                                               const float *__restrict__ target, double *__restrict__ partial,
                                                               int Nv, int E, int per_batch, float value)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    double term = 0.0;
    if (e < E) {
        const float *xb = x + (size_t)b * Nv * 3;
        const float *x0 = xb + (size_t)clampi(edges[2 * (size_t)e], 0, Nv - 1) * 3;
        const float *x1 = xb + (size_t)clampi(edges[2 * (size_t)e + 1], 0, Nv - 1) * 3;
        const float d[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]};
        const float n = dot3f(d, d);
        if (!target && value == 0.0f) {
            term = (double)n;
        } else {
            const float r = sqrtf(n) - edge_target(target, per_batch, value, b, e, E);
            term = (double)r * (double)r;
        }
    }
    store_block_sum(term, partial, b);
}

__global__ __launch_bounds__(BLOCK) void k_edge_length_backward(const float *__restrict__ x, const int32_t *__restrict__ off,
                                                                const int32_t *__restrict__ nbr,
                                                                const int32_t *__restrict__ nbr_edge,
                                                                const float *__restrict__ target,
                                                                const float *__restrict__ grad_loss,
                                                                float *__restrict__ grad_vertices, int Nv, int total, int E,
                                                                int per_batch, float value)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= Nv) return;
    const float *xb = x + (size_t)b * Nv * 3;
    const float *xv = xb + (size_t)v * 3;
    const bool squared = !target && value == 0.0f;
    int e0, e1;
    nbr_range(off, v, total, e0, e1);
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int e = e0; e < e1; e++) {
        const float *xu = xb + (size_t)clampi(nbr[e], 0, Nv - 1) * 3;
        const float d[3] = {xv[0] - xu[0], xv[1] - xu[1], xv[2] - xu[2]};
        if (squared) {
            s[0] += d[0];
            s[1] += d[1];
            s[2] += d[2];
        } else {
            const float l = sqrtf(dot3f(d, d));
            const float t = edge_target(target, per_batch, value, b, target ? clampi(nbr_edge[e], 0, E - 1) : 0, E);
            const float k = l > 0.0f ? (l - t) / l : 0.0f;
            s[0] += k * d[0];
            s[1] += k * d[1];
            s[2] += k * d[2];
        }
    }
    const float g2 = 2.0f * grad_loss[b];
    float *o = grad_vertices + ((size_t)b * Nv + v) * 3;
    o[0] = g2 * s[0];
    o[1] = g2 * s[1];
    o[2] = g2 * s[2];
}

// --------------------------------------------------------------------------------------------------------------------
// cotangent Laplacian

__global__ __launch_bounds__(BLOCK) void k_cot_weights(const float *__restrict__ x, const int32_t *__restrict__ faces,
                                                       float *__restrict__ cot, int Nv, int F, float eps)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const float *xb = x + (size_t)b * Nv * 3;
    const int32_t *fi = faces + (size_t)f * 3;
    const int i[3] = {clampi(fi[0], 0, Nv - 1), clampi(fi[1], 0, Nv - 1), clampi(fi[2], 0, Nv - 1)};
    float w[3] = {0.0f, 0.0f, 0.0f};
    if (i[0] != i[1] && i[1] != i[2] && i[0] != i[2]) {
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float *src = xb + (size_t)i[k] * 3;
            p[k][0] = src[0];
            p[k][1] = src[1];
            p[k][2] = src[2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            const float a[3] = {p[c1][0] - p[c][0], p[c1][1] - p[c][1], p[c1][2] - p[c][2]};
            const float q[3] = {p[c2][0] - p[c][0], p[c2][1] - p[c][1], p[c2][2] - p[c][2]};
            const float n[3] = {a[1] * q[2] - a[2] * q[1], a[2] * q[0] - a[0] * q[2], a[0] * q[1] - a[1] * q[0]};
            w[c] = dot3f(a, q) / sqrtf(dot3f(n, n) + eps);
        }
    }
    float *o = cot + ((size_t)b * F + f) * 3;
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
}

// out[b, v] = L(field)_v (times 2 scale[b] with a scale; out may be NULL); with `partial`, |L(field)_v|^2 goes into the block's
// sum, and every thread of the block stays to the end
__global__ __launch_bounds__(BLOCK) void k_cot_apply(const float *__restrict__ field, const float *__restrict__ cot,
                                                     const int32_t *__restrict__ faces, const int32_t *__restrict__ adj_off,
                                                     const int32_t *__restrict__ adj_ent, const float *__restrict__ scale,
                                                     float *__restrict__ out, double *__restrict__ partial, int Nv, int F)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    double sq = 0.0;
    if (v < Nv) {
        const float *pb = field + (size_t)b * Nv * 3;
        const float *wb = cot + (size_t)b * F * 3;
        const float *pv = pb + (size_t)v * 3;
        const int total = 3 * F;
        const int e0 = clampi(adj_off[v], 0, total), e1 = clampi(adj_off[v + 1], e0, total);
        float h[3] = {0.0f, 0.0f, 0.0f};
        for (int e = e0; e < e1; e++) {
            const int fc = clampi(adj_ent[e], 0, total - 1), f = fc / 3, c = fc - 3 * f;
            const int c1 = c == 2 ? 0 : c + 1, c2 = c == 0 ? 2 : c - 1;
            const int32_t *fi = faces + (size_t)f * 3;
            const float *p1 = pb + (size_t)clampi(fi[c1], 0, Nv - 1) * 3, *p2 = pb + (size_t)clampi(fi[c2], 0, Nv - 1) * 3;
            const float w1 = wb[(size_t)f * 3 + c1], w2 = wb[(size_t)f * 3 + c2];
#pragma unroll
            for (int k = 0; k < 3; k++) h[k] += w2 * (p1[k] - pv[k]) + w1 * (p2[k] - pv[k]);
        }
        float H[3] = {0.5f * h[0], 0.5f * h[1], 0.5f * h[2]};
        if (scale) {
            const float s2 = 2.0f * scale[b];
#pragma unroll
            for (int k = 0; k < 3; k++) H[k] *= s2;
        }
        if (out) {
            float *o = out + ((size_t)b * Nv + v) * 3;
            o[0] = H[0];
            o[1] = H[1];
            o[2] = H[2];
        }
        sq = ((double)H[0] * (double)H[0] + (double)H[1] * (double)H[1]) + (double)H[2] * (double)H[2];
    }
    if (partial) store_block_sum(sq, partial, b);
}

// --------------------------------------------------------------------------------------------------------------------
// host

inline int n_blocks_of(int n) { return (n + BLOCK - 1) / BLOCK; }

// B images of N >= 0 items each
int loss_sizes(int B, int Nv, int N)
{
    if (B < 1 || B > 65535 || Nv < 1 || N < 0) return NR_E_SIZE;
    if ((size_t)B * (size_t)Nv > 0x7fffffffull / 3 || (size_t)N > 0x7fffffffull / 4) return NR_E_SIZE;
    return 0;
}

size_t partial_bytes(int B, int N) { return (size_t)B * (size_t)(N > 0 ? n_blocks_of(N) : 1) * sizeof(double); }

int finish(const double *partial, float *loss, int B, int n_blocks, hipStream_t st)
{
    hipLaunchKernelGGL(k_loss_finish, dim3((unsigned)n_blocks_of(B)), dim3(BLOCK), 0, st, partial, loss, B, n_blocks);
    return launch_status();
}

}  // namespace

NR_API size_t nr_mesh_loss_workspace_bytes(int32_t B, int32_t N)
{
    if (B < 1 || B > 65535 || N < 0) return 0;
    return partial_bytes(B, N);
}

NR_API int nr_laplacian_forward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr, float *delta, float *loss,
                                int32_t B, int32_t Nv, int32_t num_nbr, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!vertices || !nbr_offsets || !loss || (num_nbr > 0 && !nbr)) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, 0)) return e;
    if (num_nbr < 0) return NR_E_SIZE;
    if (!workspace || workspace_bytes < partial_bytes(B, Nv)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int nb = n_blocks_of(Nv);
    hipLaunchKernelGGL(k_laplacian_forward, dim3((unsigned)nb, (unsigned)B), dim3(BLOCK), 0, st, vertices, nbr_offsets, nbr, delta,
                       partial, Nv, num_nbr);
    if (int rc = launch_status()) return rc;
    return finish(partial, loss, B, nb, st);
}

NR_API int nr_laplacian_backward(const float *delta, const int32_t *nbr_offsets, const int32_t *nbr, const float *grad_loss,
                                 float *grad_vertices, int32_t B, int32_t Nv, int32_t num_nbr, void *stream)
{
    if (!delta || !nbr_offsets || !grad_loss || !grad_vertices || (num_nbr > 0 && !nbr)) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, 0)) return e;
    if (num_nbr < 0) return NR_E_SIZE;
    hipLaunchKernelGGL(k_laplacian_backward, dim3((unsigned)n_blocks_of(Nv), (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream,
                       delta, nbr_offsets, nbr, grad_loss, grad_vertices, Nv, num_nbr);
    return launch_status();
}

NR_API int nr_flatness_forward(const float *vertices, const int32_t *quads, float *loss, int32_t B, int32_t Nv, int32_t E2,
                               double eps, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!vertices || !loss || (E2 > 0 && !quads)) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, E2)) return e;
    if ((size_t)B * (size_t)E2 > 0x7fffffffull) return NR_E_SIZE;
    if (!workspace || workspace_bytes < partial_bytes(B, E2)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int nb = n_blocks_of(E2);
    if (nb > 0) {
        hipLaunchKernelGGL(k_flatness_forward, dim3((unsigned)nb, (unsigned)B), dim3(BLOCK), 0, st, vertices, quads, partial, Nv,
                           E2, (float)eps);
        if (int rc = launch_status()) return rc;
    }
    return finish(partial, loss, B, nb, st);
}

NR_API int nr_flatness_backward(const float *vertices, const int32_t *quads, const int32_t *inc_offsets, const int32_t *inc,
                                const float *grad_loss, float *grad_vertices, int32_t B, int32_t Nv, int32_t E2, double eps,
                                void *stream)
{
    if (!vertices || !grad_loss || !grad_vertices || (E2 > 0 && (!quads || !inc_offsets || !inc))) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, E2)) return e;
#ifdef NR_FLATNESS_BUFFER
    if (E2 > 0) {
        float *buf = quad_buffer((size_t)B * E2 * 12 * sizeof(float));
        if (!buf) return NR_E_WORKSPACE;
        hipLaunchKernelGGL(k_flatness_quad_grads, dim3((unsigned)n_blocks_of(E2), (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream,
                           vertices, quads, grad_loss, buf, Nv, E2, (float)eps);
        if (int rc = launch_status()) return rc;
        hipLaunchKernelGGL(k_flatness_gather, dim3((unsigned)n_blocks_of(Nv), (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream,
                           inc_offsets, inc, buf, grad_vertices, Nv, E2);
        return launch_status();
    }
#endif
    hipLaunchKernelGGL(k_flatness_backward, dim3((unsigned)n_blocks_of(Nv), (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream,
                       vertices, quads, inc_offsets, inc, grad_loss, grad_vertices, Nv, E2, (float)eps);
    return launch_status();
}

NR_API int nr_edge_length_forward(const float *vertices, const int32_t *edges, const float *target, float *loss, int32_t B,
                                  int32_t Nv, int32_t E, int32_t target_per_batch, double target_value, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    if (!vertices || !loss || (E > 0 && !edges)) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, E)) return e;
    if ((size_t)B * (size_t)E > 0x7fffffffull || !(target_value >= 0.0) || target_value > 3.0e38) return NR_E_SIZE;
    if (!workspace || workspace_bytes < partial_bytes(B, E)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int nb = n_blocks_of(E);
    if (nb > 0) {
        hipLaunchKernelGGL(k_edge_length_forward, dim3((unsigned)nb, (unsigned)B), dim3(BLOCK), 0, st, vertices, edges, target,
                           partial, Nv, E, target_per_batch != 0, (float)target_value);
        if (int rc = launch_status()) return rc;
    }
    return finish(partial, loss, B, nb, st);
}

NR_API int nr_edge_length_backward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr, const int32_t *nbr_edge,
                                   const float *target, const float *grad_loss, float *grad_vertices, int32_t B, int32_t Nv,
                                   int32_t num_nbr, int32_t E, int32_t target_per_batch, double target_value, void *stream)
{
    if (!vertices || !nbr_offsets || !grad_loss || !grad_vertices || (num_nbr > 0 && !nbr)) return NR_E_NULL;
    if (target && num_nbr > 0 && !nbr_edge) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, E)) return e;
    if (num_nbr < 0 || (size_t)B * (size_t)E > 0x7fffffffull || !(target_value >= 0.0) || target_value > 3.0e38) return NR_E_SIZE;
    if (target && num_nbr > 0 && E < 1) return NR_E_SIZE;
    hipLaunchKernelGGL(k_edge_length_backward, dim3((unsigned)n_blocks_of(Nv), (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream,
                       vertices, nbr_offsets, nbr, nbr_edge, target, grad_loss, grad_vertices, Nv, num_nbr, E,
                       target_per_batch != 0, (float)target_value);
    return launch_status();
}

NR_API int nr_cot_weights(const float *vertices, const int32_t *faces, float *cot, int32_t B, int32_t Nv, int32_t F, double eps,
                          void *stream)
{
    if (!vertices || !faces || !cot) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, F)) return e;
    if (F < 1 || (size_t)B * (size_t)F > 0x7fffffffull / 3) return NR_E_SIZE;
    hipLaunchKernelGGL(k_cot_weights, dim3((unsigned)n_blocks_of(F), (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream, vertices,
                       faces, cot, Nv, F, (float)eps);
    return launch_status();
}

NR_API int nr_cot_apply(const float *field, const float *cot, const int32_t *faces, const int32_t *adj_offsets,
                        const int32_t *adj_entries, const float *scale, float *out, float *loss, int32_t B, int32_t Nv, int32_t F,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (!field || !cot || !faces || !adj_offsets || !adj_entries || (!out && !loss)) return NR_E_NULL;
    if (int e = loss_sizes(B, Nv, F)) return e;
    if (F < 1 || (size_t)B * (size_t)F > 0x7fffffffull / 3) return NR_E_SIZE;
    if (loss && (!workspace || workspace_bytes < partial_bytes(B, Nv))) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = loss ? (double *)workspace : nullptr;
    const int nb = n_blocks_of(Nv);
    hipLaunchKernelGGL(k_cot_apply, dim3((unsigned)nb, (unsigned)B), dim3(BLOCK), 0, st, field, cot, faces, adj_offsets,
                       adj_entries, scale, out, partial, Nv, F);
    if (int rc = launch_status()) return rc;
    return loss ? finish(partial, loss, B, nb, st) : 0;
}
