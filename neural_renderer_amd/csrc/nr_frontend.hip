// nr_frontend.hip -- the caller immediately in front of the rasterizer, fused.
//
// One kernel replaces the chain `Renderer.render*` runs before `rasterize` (reference neural_renderer/renderer.py:35-107):
//   fill_back          faces ++ reversed faces, textures ++ transposed textures               renderer.py:37-38, 77-79
//   lighting           per-face ambient + Lambert factor multiplied into the textures          lighting.py:8-51
//   look_at / look     camera rotation built from eye / at (or direction) / up                 look_at.py:7-46, look.py:7-45
//   perspective        x/z/tan, y/z/tan, z                                                      perspective.py:5-19
//   vertices_to_faces  the gather into [B, F, 3, 3]                                             vertices_to_faces.py:4-21
// and one kernel (plus a per-image camera kernel) replaces its whole backward, including the gradient that flows from
// the lit textures back into the vertices through the face normals, the face->vertex scatter (hardware float atomics)
// and the gradient of a learnable camera position (example4 optimises `eye`).
//
// Not in the reference: camera_mode 'projection' (NR_CAMERA_PROJECTION, nr_hip.h: nr_projection) -- intrinsics K, pose R | t
// and OpenCV lens distortion read from device arrays -- replaces look_at / look + perspective in the same kernels
// (template argument PROJ); its backward also yields per-image sums for grad_K / grad_R / grad_t (k_projection_backward).
//
// Why: in stock torch this chain is ~60 small launches forward and ~100 backward on [B,3]- to [B,Nv,3]-sized tensors,
// i.e. ~1.1 ms of host launch latency around a 0.9 ms rasterizer step at the headline size (scripts/renderer_e2e.py),
// plus three full passes over the [B, 2F, ts^3, 3] texture tensor (concat, multiply, and their backward).
//
// Host side: the six entry points (forward / backward, each with lit textures, with light colours `_light`, and for the
// projection camera `_projection`) only fill one FrontendCall.  check_call applies every argument check and builds the
// kernels' parameters; launch_forward / launch_backward then launch the PROJ instantiation the call names, and the
// backward's zero fills and its camera kernel (k_camera_backward or k_projection_backward).
//
// Work decomposition: LANES = 8 consecutive lanes per (image, face).  Every lane recomputes the (cheap) camera basis and
// the face's light colour; the lanes stride over the ts^3 texels, lanes 0/1 write the front/back copies of the face.
//
// Arithmetic follows the reference's float32 operation order where it is defined by the Python source
// (normalize = x / (|x| + 1e-5), light = ia*ca + id*(cd*cos), x / z / width); the 3x3 rotation is applied as
// ((t0*r0 + t1*r1) + t2*r2), which is one valid evaluation order of the reference's BLAS matmul.
#include "nr_device.h"
#include "nr_shade.h"

using namespace nr;

namespace {

constexpr int FE_LANES = 8;
constexpr int FE_THREADS = 256;
struct CameraBasis {
    float r[9];  // rows: x axis, y axis, z axis
    float eye[3];
    float d[3], cx[3], cy[3];  // pre-normalisation vectors (needed by the backward)
};

__device__ __forceinline__ void camera_basis(const FrontendParams &P, const float *__restrict__ eye, int b, CameraBasis &C)
{
    const float *e = eye + (P.eye_per_batch ? 3 * b : 0);
    C.eye[0] = e[0];
    C.eye[1] = e[1];
    C.eye[2] = e[2];
    if (P.camera_mode == NR_CAMERA_LOOK_AT) {  // look_at.py:30
        C.d[0] = P.target[0] - C.eye[0];
        C.d[1] = P.target[1] - C.eye[1];
        C.d[2] = P.target[2] - C.eye[2];
    } else {  // look.py:29
        C.d[0] = P.target[0];
        C.d[1] = P.target[1];
        C.d[2] = P.target[2];
    }
    normalize3(C.d, C.r + 6);
    cross3(P.up, C.r + 6, C.cx);  // look_at.py:31
    normalize3(C.cx, C.r + 0);
    cross3(C.r + 6, C.r + 0, C.cy);  // look_at.py:32
    normalize3(C.cy, C.r + 3);
}

// world vertex -> rasterizer input (x, y in NDC, z = camera depth); `cam` receives the camera-space point
__device__ __forceinline__ void project(const FrontendParams &P, const CameraBasis &C, const float *w, float *cam, float *out)
{
    const float t0 = w[0] - C.eye[0], t1 = w[1] - C.eye[1], t2 = w[2] - C.eye[2];  // look_at.py:42-43
#pragma unroll
    for (int i = 0; i < 3; i++) cam[i] = (t0 * C.r[3 * i] + t1 * C.r[3 * i + 1]) + t2 * C.r[3 * i + 2];  // :44
    if (P.perspective) {  // perspective.py:15-17
        out[0] = cam[0] / cam[2] / P.width;
        out[1] = cam[1] / cam[2] / P.width;
    } else {
        out[0] = cam[0];
        out[1] = cam[1];
    }
    out[2] = cam[2];
}

// ---- NR_CAMERA_PROJECTION: intrinsics K, pose R | t and OpenCV lens distortion (nr_hip.h: nr_projection) ----
// The camera parameters are DEVICE arrays (the host never reads them); every lane that projects loads its image's copy.
constexpr int PROJ_ACC = 18;  // per-image sums of the backward: [0..8] g_R, [9..11] g_t, [12..17] g_K rows 0-1

struct ProjParams {
    const float *K, *R, *t, *dist;  // [B,3,3] | [3,3], [B,3,3] | [3,3], [B,3] | [3], [B,5] | [5] | NULL
    int K_per_batch, R_per_batch, t_per_batch, dist_per_batch;
    float size;  // orig_size
};

struct ProjCamera {
    float R[9], t[3], K[6], d[5];  // K: rows 0 and 1 only; d = (k1, k2, p1, p2, k3)
};

__device__ __forceinline__ void proj_camera(const ProjParams &Q, int b, ProjCamera &C)
{
    const float *K = Q.K + (Q.K_per_batch ? 9 * b : 0);
    const float *R = Q.R + (Q.R_per_batch ? 9 * b : 0);
    const float *t = Q.t + (Q.t_per_batch ? 3 * b : 0);
#pragma unroll
    for (int i = 0; i < 9; i++) C.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 6; i++) C.K[i] = K[i];
#pragma unroll
    for (int i = 0; i < 3; i++) C.t[i] = t[i];
    if (Q.dist) {
        const float *d = Q.dist + (Q.dist_per_batch ? 5 * b : 0);
#pragma unroll
        for (int i = 0; i < 5; i++) C.d[i] = d[i];
    }
}

// The intermediate values of the camera model, kept for the backward
struct ProjPoint {
    float c[3];         // camera space: c = R w + t
    float xp, yp;       // x' = c.x / c.z, y' = c.y / c.z
    float r2, rad;      // (distortion only)
    float xd, yd;       // x'', y''
};

// world vertex -> (NDC x, NDC y, depth): the contract of nr_hip.h, in its float32 operation order
__device__ __forceinline__ void project_projection(const ProjParams &Q, const ProjCamera &C, const float *w, ProjPoint &p,
                                                   float *out)
{
#pragma unroll
    for (int i = 0; i < 3; i++) p.c[i] = ((C.R[3 * i] * w[0] + C.R[3 * i + 1] * w[1]) + C.R[3 * i + 2] * w[2]) + C.t[i];
    p.xp = p.c[0] / p.c[2];
    p.yp = p.c[1] / p.c[2];
    if (Q.dist) {
        const float k1 = C.d[0], k2 = C.d[1], p1 = C.d[2], p2 = C.d[3], k3 = C.d[4];
        const float x = p.xp, y = p.yp;
        p.r2 = x * x + y * y;
        const float r4 = p.r2 * p.r2, r6 = r4 * p.r2;
        p.rad = ((1.0f + k1 * p.r2) + k2 * r4) + k3 * r6;
        p.xd = (x * p.rad + 2.0f * p1 * x * y) + p2 * (p.r2 + 2.0f * x * x);
        p.yd = (y * p.rad + p1 * (p.r2 + 2.0f * y * y)) + 2.0f * p2 * x * y;
    } else {
        p.r2 = 0.0f;
        p.rad = 1.0f;
        p.xd = p.xp;
        p.yd = p.yp;
    }
    const float u = (C.K[0] * p.xd + C.K[1] * p.yd) + C.K[2];
    const float v = (C.K[3] * p.xd + C.K[4] * p.yd) + C.K[5];
    out[0] = (2.0f * u - Q.size) / Q.size;
    out[1] = (Q.size - 2.0f * v) / Q.size;
    out[2] = p.c[2];
}

// backward of project_projection for one vertex: g = d loss / d out -> gw (world vertex, added), acc (PROJ_ACC sums, added)
__device__ __forceinline__ void project_projection_bwd(const ProjParams &Q, const ProjCamera &C, const float *w, const float *g,
                                                       float *gw, float *acc)
{
    ProjPoint p;
    float o[3];
    project_projection(Q, C, w, p, o);
    const float gu = 2.0f * g[0] / Q.size;  // out.x = (2u - S) / S
    const float gv = -2.0f * g[1] / Q.size; // out.y = (S - 2v) / S
    acc[12] += gu * p.xd;
    acc[13] += gu * p.yd;
    acc[14] += gu;
    acc[15] += gv * p.xd;
    acc[16] += gv * p.yd;
    acc[17] += gv;
    const float gxd = gu * C.K[0] + gv * C.K[3];
    const float gyd = gu * C.K[1] + gv * C.K[4];
    float gxp = gxd, gyp = gyd;
    if (Q.dist) {  // the Jacobian of (x'', y'') by (x', y'); it is symmetric
        const float k1 = C.d[0], k2 = C.d[1], p1 = C.d[2], p2 = C.d[3], k3 = C.d[4];
        const float x = p.xp, y = p.yp;
        const float drad = (k1 + 2.0f * k2 * p.r2) + 3.0f * k3 * (p.r2 * p.r2);  // d rad / d r2
        const float jxx = ((p.rad + 2.0f * x * x * drad) + 2.0f * p1 * y) + 6.0f * p2 * x;
        const float jxy = ((2.0f * x * y * drad) + 2.0f * p1 * x) + 2.0f * p2 * y;
        const float jyy = ((p.rad + 2.0f * y * y * drad) + 6.0f * p1 * y) + 2.0f * p2 * x;
        gxp = gxd * jxx + gyd * jxy;
        gyp = gxd * jxy + gyd * jyy;
    }
    const float gc[3] = {gxp / p.c[2], gyp / p.c[2], g[2] - (gxp * p.xp + gyp * p.yp) / p.c[2]};
    // c = R w + t:  g_w = R^T g_c,  g_R[i][j] += g_c[i] w[j],  g_t += g_c
#pragma unroll
    for (int j = 0; j < 3; j++) gw[j] += (gc[0] * C.R[j] + gc[1] * C.R[3 + j]) + gc[2] * C.R[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) acc[3 * i + j] += gc[i] * w[j];
        acc[9 + i] += gc[i];
    }
}

// PROJ: the NR_CAMERA_PROJECTION model of `Q` (eye unused) instead of look_at / look + perspective
template <bool PROJ>
__global__ __launch_bounds__(FE_THREADS) void k_frontend_forward(const float *__restrict__ vertices,
                                                                 const int32_t *__restrict__ faces_idx,
                                                                 const float *__restrict__ textures,
                                                                 const float *__restrict__ eye, float *__restrict__ faces_out,
                                                                 float *__restrict__ textures_out, int Nv, int Nf, int ts,
                                                                 FrontendParams P, float *__restrict__ light_out, ProjParams Q)
{
    const int b = blockIdx.y;
    const int f = (blockIdx.x * FE_THREADS + threadIdx.x) / FE_LANES;
    const int lane = threadIdx.x % FE_LANES;
    if (f >= Nf) return;
    const int Fout = P.fill_back ? 2 * Nf : Nf;
    const int32_t *idx = faces_idx + ((size_t)(P.idx_per_batch ? b : 0) * Nf + f) * 3;
    const float *vb = vertices + (size_t)b * Nv * 3;
    float w[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *src = vb + (size_t)min(max(idx[k], 0), Nv - 1) * 3;  // validated on the host; clamped for memory safety
        w[k][0] = src[0];
        w[k][1] = src[1];
        w[k][2] = src[2];
    }

    if (lane < 2 && (lane == 0 || P.fill_back)) {
        float *dst = faces_out + ((size_t)b * Fout + (lane == 0 ? f : Nf + f)) * 9;
        if constexpr (PROJ) {
            ProjCamera C;
            proj_camera(Q, b, C);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ProjPoint p;
                float *d = dst + 3 * (lane == 0 ? k : 2 - k);
                project_projection(Q, C, w[k], p, d);
            }
        } else {
            CameraBasis C;
            camera_basis(P, eye, b, C);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float cam[3], o[3];
                project(P, C, w[k], cam, o);
                float *d = dst + 3 * (lane == 0 ? k : 2 - k);  // reversed vertex order for the back copy
                d[0] = o[0];
                d[1] = o[1];
                d[2] = o[2];
            }
        }
    }

    if (light_out && lane == 0) {  // the colours only: the rasterizer multiplies its samples by them (nr_hip.h: nr_face_light)
        float n[3], dotn, lf[3], lb[3];
        face_light(P, w[0], w[1], w[2], n, dotn, lf, lb);
        float *of = light_out + ((size_t)b * Fout + f) * 3;
        float *ob = light_out + ((size_t)b * Fout + Nf + f) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            of[c] = lf[c];
            if (P.fill_back) ob[c] = lb[c];
        }
    }
    if (textures) {
        float n[3], dotn, lf[3], lb[3];
        face_light(P, w[0], w[1], w[2], n, dotn, lf, lb);
        const int T = ts * ts * ts;
        const float *tex = textures + ((size_t)b * Nf + f) * T * 3;
        float *of = textures_out + ((size_t)b * Fout + f) * T * 3;
        float *ob = textures_out + ((size_t)b * Fout + Nf + f) * T * 3;
        for (int t = lane; t < T; t += FE_LANES) {
            const float t0 = tex[3 * t], t1 = tex[3 * t + 1], t2 = tex[3 * t + 2];
            of[3 * t] = t0 * lf[0];  // lighting.py:50-51
            of[3 * t + 1] = t1 * lf[1];
            of[3 * t + 2] = t2 * lf[2];
            if (P.fill_back) {
                const int u = transpose_texel(t, ts);
                ob[3 * u] = t0 * lb[0];
                ob[3 * u + 1] = t1 * lb[1];
                ob[3 * u + 2] = t2 * lb[2];
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------
// backward
// cam_acc: per-image camera sums, NACC doubles per image (12 for eye: sum of g_w, g_R; PROJ_ACC for PROJ)
template <bool PROJ>
__global__ __launch_bounds__(FE_THREADS) void k_frontend_backward(
    const float *__restrict__ vertices, const int32_t *__restrict__ faces_idx, const float *__restrict__ textures,
    const float *__restrict__ eye, const float *__restrict__ g_faces, const float *__restrict__ g_tex_out,
    float *__restrict__ grad_vertices, float *__restrict__ grad_textures, double *__restrict__ cam_acc, int Nv, int Nf, int ts,
    FrontendParams P, const float *__restrict__ g_light, ProjParams Q)
{
    constexpr int NACC = PROJ ? PROJ_ACC : 12;
    __shared__ double s_acc[FE_THREADS / 64][NACC];
    const int b = blockIdx.y;
    const int f = (blockIdx.x * FE_THREADS + threadIdx.x) / FE_LANES;
    const int lane = threadIdx.x % FE_LANES;
    const bool live = f < Nf;
    const int Fout = P.fill_back ? 2 * Nf : Nf;
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; k++) acc[k] = 0.0f;

    if (live) {
        const int32_t *idx = faces_idx + ((size_t)(P.idx_per_batch ? b : 0) * Nf + f) * 3;
        const float *vb = vertices + (size_t)b * Nv * 3;
        const int vi[3] = {min(max(idx[0], 0), Nv - 1), min(max(idx[1], 0), Nv - 1), min(max(idx[2], 0), Nv - 1)};
        float w[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float *src = vb + (size_t)vi[k] * 3;
            w[k][0] = src[0];
            w[k][1] = src[1];
            w[k][2] = src[2];
        }
        float gw[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // gradient w.r.t. the face's three world-space vertices

        // ---- textures / lighting ----
        if ((textures && g_tex_out) || g_light) {
            float n[3], dotn, lf[3], lb[3];
            face_light(P, w[0], w[1], w[2], n, dotn, lf, lb);
            const int T = g_light ? 0 : ts * ts * ts;
            const float *tex = textures + ((size_t)b * Nf + f) * T * 3;
            const float *gf = g_tex_out + ((size_t)b * Fout + f) * T * 3;
            const float *gb = g_tex_out + ((size_t)b * Fout + Nf + f) * T * 3;
            float *gt = grad_textures ? grad_textures + ((size_t)b * Nf + f) * T * 3 : nullptr;
            float glf[3] = {0, 0, 0}, glb[3] = {0, 0, 0};
            if (g_light && lane == 0) {  // the colours' gradient arrives summed (the other lanes add zeros below)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    glf[c] = g_light[((size_t)b * Fout + f) * 3 + c];
                    if (P.fill_back) glb[c] = g_light[((size_t)b * Fout + Nf + f) * 3 + c];
                }
            }
            for (int t = lane; t < T; t += FE_LANES) {
                const int u = P.fill_back ? transpose_texel(t, ts) : 0;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float x = tex[3 * t + c];
                    const float a = gf[3 * t + c];
                    const float bb = P.fill_back ? gb[3 * u + c] : 0.0f;
                    if (gt) gt[3 * t + c] = P.fill_back ? a * lf[c] + bb * lb[c] : a * lf[c];
                    glf[c] += a * x;
                    glb[c] += bb * x;
                }
            }
            if (P.has_directional && grad_vertices) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
#pragma unroll
                    for (int m = 1; m < FE_LANES; m <<= 1) {
                        glf[c] += __shfl_xor(glf[c], m);
                        glb[c] += __shfl_xor(glb[c], m);
                    }
                }
                if (lane == 0) {
                    // light = amb + id * (cd * cos): d loss / d cos
                    const float gcf = P.id * (P.cd[0] * glf[0] + P.cd[1] * glf[1] + P.cd[2] * glf[2]);
                    const float gcb = P.id * (P.cd[0] * glb[0] + P.cd[1] * glb[1] + P.cd[2] * glb[2]);
                    float gdot = 0.0f;  // relu: the front copy sees dotn, the back copy -dotn
                    if (dotn > 0.0f) gdot += gcf;
                    if (-dotn > 0.0f) gdot -= gcb;
                    if (gdot != 0.0f) {
                        const float gnh[3] = {gdot * P.ldir[0], gdot * P.ldir[1], gdot * P.ldir[2]};
                        float gn[3];
                        normalize3_bwd(n, gnh, gn);
                        // n = v10 x v12:  g_v10 = v12 x g_n,  g_v12 = g_n x v10
                        const float v10[3] = {w[0][0] - w[1][0], w[0][1] - w[1][1], w[0][2] - w[1][2]};
                        const float v12[3] = {w[2][0] - w[1][0], w[2][1] - w[1][1], w[2][2] - w[1][2]};
                        float ga[3], gb2[3];
                        cross3(v12, gn, ga);
                        cross3(gn, v10, gb2);
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            gw[0][c] += ga[c];
                            gw[2][c] += gb2[c];
                            gw[1][c] -= ga[c] + gb2[c];
                        }
                    }
                }
            }
        }

        // ---- geometry: perspective, rotation, gather ----
        if constexpr (PROJ) {
            if (lane == 0 && grad_vertices) {
                ProjCamera C;
                proj_camera(Q, b, C);
                const float *g0 = g_faces + ((size_t)b * Fout + f) * 9;
                const float *g1 = g_faces + ((size_t)b * Fout + Nf + f) * 9;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    float g[3] = {g0[3 * k], g0[3 * k + 1], g0[3 * k + 2]};
                    if (P.fill_back) {
                        g[0] += g1[3 * (2 - k)];
                        g[1] += g1[3 * (2 - k) + 1];
                        g[2] += g1[3 * (2 - k) + 2];
                    }
                    project_projection_bwd(Q, C, w[k], g, gw[k], acc);
                }
            }
        } else if (lane == 0 && grad_vertices) {
            CameraBasis C;
            camera_basis(P, eye, b, C);
            const float *g0 = g_faces + ((size_t)b * Fout + f) * 9;
            const float *g1 = g_faces + ((size_t)b * Fout + Nf + f) * 9;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float g[3] = {g0[3 * k], g0[3 * k + 1], g0[3 * k + 2]};
                if (P.fill_back) {
                    g[0] += g1[3 * (2 - k)];
                    g[1] += g1[3 * (2 - k) + 1];
                    g[2] += g1[3 * (2 - k) + 2];
                }
                float cam[3], o[3];
                project(P, C, w[k], cam, o);
                float gc[3];  // gradient w.r.t. the camera-space point
                if (P.perspective) {
                    const float zw = cam[2] * P.width;
                    gc[0] = g[0] / zw;
                    gc[1] = g[1] / zw;
                    gc[2] = g[2] - (g[0] * cam[0] + g[1] * cam[1]) / (cam[2] * zw);
                } else {
                    gc[0] = g[0];
                    gc[1] = g[1];
                    gc[2] = g[2];
                }
                // cam = R (w - eye):  g_w = R^T g_cam,  g_eye -= g_w,  g_R[i][j] += g_cam[i] * (w - eye)[j]
                float gwk[3];
#pragma unroll
                for (int j = 0; j < 3; j++) gwk[j] = (gc[0] * C.r[j] + gc[1] * C.r[3 + j]) + gc[2] * C.r[6 + j];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    gw[k][j] += gwk[j];
                    acc[j] += gwk[j];
                }
                if (cam_acc) {
                    const float t[3] = {w[k][0] - C.eye[0], w[k][1] - C.eye[1], w[k][2] - C.eye[2]};
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++) acc[3 + 3 * i + j] += gc[i] * t[j];
                }
            }
        }

        if (lane == 0 && grad_vertices) {  // face -> vertex scatter (get_item backward)
            float *gv = grad_vertices + (size_t)b * Nv * 3;
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int c = 0; c < 3; c++)
                    if (gw[k][c] != 0.0f) atomicAdd(gv + (size_t)vi[k] * 3 + c, gw[k][c]);
        }
    }

    if (cam_acc) {  // per-image sums for the camera backward (eye: [0..2] = sum of g_w, [3..11] = g_R; PROJ: PROJ_ACC)
        const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
#pragma unroll
        for (int k = 0; k < NACC; k++) {
            double v = (double)acc[k];
#pragma unroll
            for (int m = FE_LANES; m < 64; m <<= 1) v += __shfl_xor(v, m);
            if (wl == 0) s_acc[wave][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < NACC) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < FE_THREADS / 64; q++) v += s_acc[q][threadIdx.x];
            if (v != 0.0) atomicAdd(cam_acc + (size_t)b * NACC + threadIdx.x, v);
        }
    }
}

// one thread per image: the gradient of the camera position through `cam = R(eye) (w - eye)`
__global__ void k_camera_backward(const float *__restrict__ eye, const double *__restrict__ cam_acc,
                                  float *__restrict__ grad_eye, int B, FrontendParams P)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    CameraBasis C;
    camera_basis(P, eye, b, C);
    const double *a = cam_acc + (size_t)b * 12;
    float ge[3] = {-(float)a[0], -(float)a[1], -(float)a[2]};  // direct term: cam = R (w - eye)
    if (P.camera_mode == NR_CAMERA_LOOK_AT) {                  // R depends on eye only in look_at mode
        const float gx[3] = {(float)a[3], (float)a[4], (float)a[5]};
        const float gy[3] = {(float)a[6], (float)a[7], (float)a[8]};
        float gz[3] = {(float)a[9], (float)a[10], (float)a[11]};
        // y = N(cy), cy = z x x
        float gcy[3], t[3], gxt[3];
        normalize3_bwd(C.cy, gy, gcy);
        cross3(C.r + 0, gcy, t);  // g_z += x x g_cy
        gz[0] += t[0];
        gz[1] += t[1];
        gz[2] += t[2];
        cross3(gcy, C.r + 6, t);  // g_x += g_cy x z
        gxt[0] = gx[0] + t[0];
        gxt[1] = gx[1] + t[1];
        gxt[2] = gx[2] + t[2];
        // x = N(cx), cx = up x z
        float gcx[3];
        normalize3_bwd(C.cx, gxt, gcx);
        cross3(gcx, P.up, t);  // g_z += g_cx x up
        gz[0] += t[0];
        gz[1] += t[1];
        gz[2] += t[2];
        // z = N(d), d = at - eye
        float gd[3];
        normalize3_bwd(C.d, gz, gd);
        ge[0] -= gd[0];
        ge[1] -= gd[1];
        ge[2] -= gd[2];
    }
    if (P.eye_per_batch) {
        grad_eye[3 * b] = ge[0];
        grad_eye[3 * b + 1] = ge[1];
        grad_eye[3 * b + 2] = ge[2];
    } else {  // one camera shared by the batch: grad_eye [3] zero-filled by the host call
        atomicAdd(grad_eye + 0, ge[0]);
        atomicAdd(grad_eye + 1, ge[1]);
        atomicAdd(grad_eye + 2, ge[2]);
    }
}

// one thread per image: the per-image sums -> grad_K (rows 0-1; row 2 is 0), grad_R, grad_t.  A parameter shared by the
// batch receives every image's sum through a float atomic (its output is zero-filled by the host call).
__global__ void k_projection_backward(const double *__restrict__ cam_acc, float *__restrict__ grad_K, float *__restrict__ grad_R,
                                      float *__restrict__ grad_t, int B, ProjParams Q)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *a = cam_acc + (size_t)b * PROJ_ACC;
    if (grad_R) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            if (Q.R_per_batch)
                grad_R[9 * b + i] = (float)a[i];
            else
                atomicAdd(grad_R + i, (float)a[i]);
        }
    }
    if (grad_t) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (Q.t_per_batch)
                grad_t[3 * b + i] = (float)a[9 + i];
            else
                atomicAdd(grad_t + i, (float)a[9 + i]);
        }
    }
    if (grad_K) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const float v = i < 6 ? (float)a[12 + i] : 0.0f;
            if (Q.K_per_batch)
                grad_K[9 * b + i] = v;
            else if (i < 6)
                atomicAdd(grad_K + i, v);
        }
    }
}

// ---- host: each entry point fills one FrontendCall; check_call and the two runners serve all six ----

// One call of any entry point.  proj: the NR_CAMERA_PROJECTION model (`projection`), else look_at / look (`camera`, `eye`).
// A forward call sets the forward outputs, a backward call the gradients; the rest stays NULL.
struct FrontendCall {
    bool proj;
    const nr_camera *camera;
    const nr_projection *projection;
    const float *vertices, *textures, *eye;
    const int32_t *faces_idx;
    float *faces_out, *textures_out, *light_out;
    const float *grad_faces, *grad_textures_out, *grad_light;
    float *grad_vertices, *grad_textures, *grad_eye, *grad_K, *grad_R, *grad_t;
    int32_t B, Nv, Nf, ts, idx_per_batch, eye_per_batch, fill_back;
    const nr_light *light;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t st;
};

// the per-image camera sums of the backward: 12 doubles for eye, PROJ_ACC for the projection camera
size_t cam_acc_bytes(int32_t B, bool proj) { return B < 1 ? 0 : (size_t)B * (proj ? PROJ_ACC : 12) * sizeof(double); }

bool wants_camera(const FrontendCall &c) { return c.grad_eye || c.grad_K || c.grad_R || c.grad_t; }

// Every argument check of a call, in the order the entry points apply them, then the kernels' parameters
int check_call(const FrontendCall &c, bool backward, FrontendParams &P, ProjParams &Q)
{
    if (!c.vertices || !c.faces_idx || (!c.proj && !c.eye)) return NR_E_NULL;
    const bool want_cam = wants_camera(c);
    if (backward) {
        if (!c.grad_faces) return NR_E_NULL;
        if (!c.grad_vertices && !c.grad_textures && !want_cam) return NR_E_MODE;
        if (want_cam && !c.grad_vertices) return NR_E_MODE;  // the camera sums are produced by the vertex pass
        if (c.grad_textures && !(c.textures && c.grad_textures_out)) return NR_E_MODE;
        if (c.grad_textures_out && !c.textures) return NR_E_MODE;
        if (c.grad_light && c.textures) return NR_E_MODE;
        if (c.grad_light && !c.light) return NR_E_NULL;
    } else {
        if (!c.faces_out) return NR_E_NULL;
        if ((c.textures == nullptr) != (c.textures_out == nullptr)) return NR_E_MODE;
        if (c.textures_out && c.light_out) return NR_E_MODE;
    }
    if (c.B < 1 || c.Nv < 1 || c.Nf < 1 || c.B > 65535) return NR_E_SIZE;
    if (c.textures && c.ts < 1) return NR_E_SIZE;
    if ((size_t)c.B * (size_t)c.Nf > 0x7fffffffull / 18) return NR_E_SIZE;
    P = {};
    Q = {};
    if (c.proj) {
        const nr_projection *p = c.projection;
        if (!p || !p->K || !p->R || !p->t) return NR_E_NULL;
        if (!(p->orig_size > 0.0f && p->orig_size < __builtin_inff())) return NR_E_SIZE;
        P.camera_mode = NR_CAMERA_PROJECTION;  // (no look_at / perspective parameters: they stay 0)
        Q = {p->K, p->R, p->t, p->dist_coeffs, p->K_per_batch != 0, p->R_per_batch != 0, p->t_per_batch != 0,
             p->dist_per_batch != 0, p->orig_size};
    } else {
        const nr_camera *cam = c.camera;
        if (!cam) return NR_E_NULL;
        if (cam->mode != NR_CAMERA_LOOK_AT && cam->mode != NR_CAMERA_LOOK) return NR_E_MODE;
        P.camera_mode = cam->mode;
        P.perspective = cam->perspective != 0;
        for (int k = 0; k < 3; k++) {
            P.target[k] = cam->target[k];
            P.up[k] = cam->up[k];
        }
        P.width = cam->width;
    }
    if ((c.textures || c.light_out || c.grad_light) && !c.light) return NR_E_NULL;
    P.eye_per_batch = c.eye_per_batch != 0;
    P.idx_per_batch = c.idx_per_batch != 0;
    P.fill_back = c.fill_back != 0;
    if (c.light) {
        P.ia = c.light->intensity_ambient;
        P.id = c.light->intensity_directional;
        P.has_directional = c.light->intensity_directional != 0.0f;
        for (int k = 0; k < 3; k++) {
            P.ca[k] = c.light->color_ambient[k];
            P.cd[k] = c.light->color_directional[k];
            P.ldir[k] = c.light->direction[k];
        }
    }
    if (want_cam && (!c.workspace || c.workspace_bytes < cam_acc_bytes(c.B, c.proj))) return NR_E_WORKSPACE;
    return 0;
}

dim3 face_grid(const FrontendCall &c)
{
    return dim3((unsigned)(((size_t)c.Nf * FE_LANES + FE_THREADS - 1) / FE_THREADS), (unsigned)c.B);
}

int launch_forward(const FrontendCall &c)
{
    FrontendParams P;
    ProjParams Q;
    if (int rc = check_call(c, false, P, Q)) return rc;
    hipLaunchKernelGGL(c.proj ? k_frontend_forward<true> : k_frontend_forward<false>, face_grid(c), dim3(FE_THREADS), 0, c.st,
                       c.vertices, c.faces_idx, c.textures, c.eye, c.faces_out, c.textures_out, c.Nv, c.Nf,
                       c.light_out ? 0 : c.ts, P, c.light_out, Q);
    return launch_status();
}

int launch_backward(const FrontendCall &c)
{
    FrontendParams P;
    ProjParams Q;
    if (int rc = check_call(c, true, P, Q)) return rc;
    double *cam_acc = nullptr;
    if (wants_camera(c)) {  // zeros for the camera sums and for the camera gradients the batch shares (float atomics)
        cam_acc = (double *)c.workspace;
        int e = fill_bytes(cam_acc, 0, cam_acc_bytes(c.B, c.proj), c.st);
        if (e == 0 && c.grad_eye && !P.eye_per_batch) e = fill_bytes(c.grad_eye, 0, 3 * sizeof(float), c.st);
        if (e == 0 && c.grad_K && !Q.K_per_batch) e = fill_bytes(c.grad_K, 0, 9 * sizeof(float), c.st);
        if (e == 0 && c.grad_R && !Q.R_per_batch) e = fill_bytes(c.grad_R, 0, 9 * sizeof(float), c.st);
        if (e == 0 && c.grad_t && !Q.t_per_batch) e = fill_bytes(c.grad_t, 0, 3 * sizeof(float), c.st);
        if (e != 0) return e;
    }
    if (c.grad_vertices)
        if (int e = fill_bytes(c.grad_vertices, 0, (size_t)c.B * c.Nv * 3 * sizeof(float), c.st)) return e;
    hipLaunchKernelGGL(c.proj ? k_frontend_backward<true> : k_frontend_backward<false>, face_grid(c), dim3(FE_THREADS), 0, c.st,
                       c.vertices, c.faces_idx, c.textures, c.eye, c.grad_faces, c.grad_textures_out, c.grad_vertices,
                       c.grad_textures, cam_acc, c.Nv, c.Nf, c.grad_light ? 0 : c.ts, P, c.grad_light, Q);
    if (int rc = launch_status()) return rc;
    if (!cam_acc) return 0;
    const dim3 grid((unsigned)((c.B + 63) / 64));
    if (c.proj)
        hipLaunchKernelGGL(k_projection_backward, grid, dim3(64), 0, c.st, cam_acc, c.grad_K, c.grad_R, c.grad_t, c.B, Q);
    else
        hipLaunchKernelGGL(k_camera_backward, grid, dim3(64), 0, c.st, c.eye, cam_acc, c.grad_eye, c.B, P);
    return launch_status();
}

}  // namespace

NR_API size_t nr_frontend_workspace_bytes(int32_t B) { return cam_acc_bytes(B, false); }

NR_API size_t nr_frontend_projection_workspace_bytes(int32_t B) { return cam_acc_bytes(B, true); }

NR_API int nr_frontend_forward(const float *vertices, const int32_t *faces_idx, const float *textures, const float *eye,
                               float *faces_out, float *textures_out, int32_t B, int32_t Nv, int32_t Nf, int32_t ts,
                               int32_t idx_per_batch, int32_t eye_per_batch, int32_t fill_back, const nr_camera *camera,
                               const nr_light *light, void *stream)
{
    FrontendCall c = {};
    c.camera = camera, c.eye = eye, c.eye_per_batch = eye_per_batch;
    c.vertices = vertices, c.faces_idx = faces_idx, c.textures = textures;
    c.faces_out = faces_out, c.textures_out = textures_out;
    c.B = B, c.Nv = Nv, c.Nf = Nf, c.ts = ts, c.idx_per_batch = idx_per_batch, c.fill_back = fill_back;
    c.light = light, c.st = (hipStream_t)stream;
    return launch_forward(c);
}

NR_API int nr_frontend_forward_light(const float *vertices, const int32_t *faces_idx, const float *eye, float *faces_out,
                                     float *light_out, int32_t B, int32_t Nv, int32_t Nf, int32_t idx_per_batch,
                                     int32_t eye_per_batch, int32_t fill_back, const nr_camera *camera,
                                     const nr_light *light, void *stream)
{
    if (!light_out) return NR_E_NULL;
    FrontendCall c = {};
    c.camera = camera, c.eye = eye, c.eye_per_batch = eye_per_batch;
    c.vertices = vertices, c.faces_idx = faces_idx, c.faces_out = faces_out, c.light_out = light_out;
    c.B = B, c.Nv = Nv, c.Nf = Nf, c.idx_per_batch = idx_per_batch, c.fill_back = fill_back;
    c.light = light, c.st = (hipStream_t)stream;
    return launch_forward(c);
}

NR_API int nr_frontend_backward(const float *vertices, const int32_t *faces_idx, const float *textures, const float *eye,
                                const float *grad_faces, const float *grad_textures_out, float *grad_vertices,
                                float *grad_textures, float *grad_eye, int32_t B, int32_t Nv, int32_t Nf, int32_t ts,
                                int32_t idx_per_batch, int32_t eye_per_batch, int32_t fill_back, const nr_camera *camera,
                                const nr_light *light, void *workspace, size_t workspace_bytes, void *stream)
{
    FrontendCall c = {};
    c.camera = camera, c.eye = eye, c.eye_per_batch = eye_per_batch, c.grad_eye = grad_eye;
    c.vertices = vertices, c.faces_idx = faces_idx, c.textures = textures;
    c.grad_faces = grad_faces, c.grad_textures_out = grad_textures_out;
    c.grad_vertices = grad_vertices, c.grad_textures = grad_textures;
    c.B = B, c.Nv = Nv, c.Nf = Nf, c.ts = ts, c.idx_per_batch = idx_per_batch, c.fill_back = fill_back;
    c.light = light, c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.st = (hipStream_t)stream;
    return launch_backward(c);
}

NR_API int nr_frontend_backward_light(const float *vertices, const int32_t *faces_idx, const float *eye,
                                      const float *grad_faces, const float *grad_light, float *grad_vertices,
                                      float *grad_eye, int32_t B, int32_t Nv, int32_t Nf, int32_t idx_per_batch,
                                      int32_t eye_per_batch, int32_t fill_back, const nr_camera *camera,
                                      const nr_light *light, void *workspace, size_t workspace_bytes, void *stream)
{
    if (grad_light && !light) return NR_E_NULL;  // (ahead of every other check, as it always was here)
    FrontendCall c = {};
    c.camera = camera, c.eye = eye, c.eye_per_batch = eye_per_batch, c.grad_eye = grad_eye;
    c.vertices = vertices, c.faces_idx = faces_idx;
    c.grad_faces = grad_faces, c.grad_light = grad_light, c.grad_vertices = grad_vertices;
    c.B = B, c.Nv = Nv, c.Nf = Nf, c.idx_per_batch = idx_per_batch, c.fill_back = fill_back;
    c.light = light, c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.st = (hipStream_t)stream;
    return launch_backward(c);
}

NR_API int nr_frontend_forward_projection(const float *vertices, const int32_t *faces_idx, const float *textures,
                                          float *faces_out, float *textures_out, float *light_out, int32_t B, int32_t Nv,
                                          int32_t Nf, int32_t ts, int32_t idx_per_batch, int32_t fill_back,
                                          const nr_projection *projection, const nr_light *light, void *stream)
{
    FrontendCall c = {};
    c.proj = true, c.projection = projection;
    c.vertices = vertices, c.faces_idx = faces_idx, c.textures = textures;
    c.faces_out = faces_out, c.textures_out = textures_out, c.light_out = light_out;
    c.B = B, c.Nv = Nv, c.Nf = Nf, c.ts = ts, c.idx_per_batch = idx_per_batch, c.fill_back = fill_back;
    c.light = light, c.st = (hipStream_t)stream;
    return launch_forward(c);
}

NR_API int nr_frontend_backward_projection(const float *vertices, const int32_t *faces_idx, const float *textures,
                                           const float *grad_faces, const float *grad_textures_out, const float *grad_light,
                                           float *grad_vertices, float *grad_textures, float *grad_K, float *grad_R,
                                           float *grad_t, int32_t B, int32_t Nv, int32_t Nf, int32_t ts,
                                           int32_t idx_per_batch, int32_t fill_back, const nr_projection *projection,
                                           const nr_light *light, void *workspace, size_t workspace_bytes, void *stream)
{
    FrontendCall c = {};
    c.proj = true, c.projection = projection, c.grad_K = grad_K, c.grad_R = grad_R, c.grad_t = grad_t;
    c.vertices = vertices, c.faces_idx = faces_idx, c.textures = textures;
    c.grad_faces = grad_faces, c.grad_textures_out = grad_textures_out, c.grad_light = grad_light;
    c.grad_vertices = grad_vertices, c.grad_textures = grad_textures;
    c.B = B, c.Nv = Nv, c.Nf = Nf, c.ts = ts, c.idx_per_batch = idx_per_batch, c.fill_back = fill_back;
    c.light = light, c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.st = (hipStream_t)stream;
    return launch_backward(c);
}
