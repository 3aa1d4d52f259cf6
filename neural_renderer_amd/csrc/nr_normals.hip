// nr_normals.hip -- vertex, face and corner normals as operators of their own (include/nr_hip.h; DESIGN "Normal maps").
//
// The normals are the ones the light kernels already form and fold away (nr_vertex_colors.hip: k_vertex_light; nr_shade.h:
// face_light), in the same float32 operation order, so that the two agree bit for bit:
//   N_f = cross(v0 - v1, v2 - v1), n_f = normalize3(N_f); m_v = the sum of N_f over the (face, corner) pairs of v in ascending
//   3 f + k order, n_v = normalize3(m_v); a vertex without a face, a zero m_v or a zero-area face gives exactly 0.
// Every sum around a vertex or a face is a GATHER through the vertex -> (face, corner) table: no atomics in either direction,
// every output element stored, the same bits in every run and for an image alone or inside a batch.
//   k_vertex_normals          forward: (image, vertex) -> n_v
//   k_face_normals            forward: (image, face) -> n_f
//   k_corner_normals<SMOOTH>  forward: (image, face) -> the nine numbers of the face and of its reversed copy (negated, in
//                             its own flipped corner order: corner[Nf + f][k] = -corner[f][2 - k])
//   k_vertex_stage<CORNER>    backward 1, smooth: (image, vertex) -> g_m, the gradient of the vertex's normal sum, from
//                             grad_normals or from the corner gradients around the vertex (front minus flipped back)
//   k_face_stage<CORNER>      backward 1, flat: (image, face) -> g_N, the gradient of the face's unnormalised normal
//   k_normals_gather<SMOOTH>  backward 2 (nr_mesh_gather.h): (image, vertex) -> grad_vertices, corner k's share of g_N(f)
//                             summed over the faces around the vertex; smooth: g_N(f) = (g_m(v0) + g_m(v1)) + g_m(v2)
// The mesh arguments, the geometry helpers and k_normals_gather are nr_mesh_gather.h's, shared with nr_vertex_colors.hip and
// nr_lights.hip.
#include "nr_mesh_gather.h"

using namespace nr;

namespace {

// the gradient of corner k of face f's normal from grad_corner of image b: the front copy's minus the reversed copy's, which
// carries the negated normal at corner 2 - k
__device__ __forceinline__ void corner_grad(const MeshArgs &a, const float *__restrict__ gcb, int f, int k, float *g)
{
    const float *gf = gcb + (size_t)f * 9 + 3 * k;
    g[0] = gf[0];
    g[1] = gf[1];
    g[2] = gf[2];
    if (a.fill_back) {
        const float *gb = gcb + ((size_t)a.Nf + f) * 9 + 3 * (2 - k);
        g[0] -= gb[0];
        g[1] -= gb[1];
        g[2] -= gb[2];
    }
}

// --------------------------------------------------------------------------------------------------------------------
// forward

__global__ __launch_bounds__(256) void k_vertex_normals(MeshArgs a, float *__restrict__ normals)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    float m[3], n[3];
    normal_sum(a, b, v, m);
    normalize3(m, n);
    float *o = normals + ((size_t)b * a.Nv + v) * 3;
    o[0] = n[0];
    o[1] = n[1];
    o[2] = n[2];
}

__global__ __launch_bounds__(256) void k_face_normals(MeshArgs a, float *__restrict__ normals)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= a.Nf) return;
    int vi[3];
    float w[3][3], v10[3], v12[3], N[3], n[3];
    load_face(a, b, f, vi, w);
    face_normal(w, v10, v12, N);
    normalize3(N, n);
    float *o = normals + ((size_t)b * a.Nf + f) * 3;
    o[0] = n[0];
    o[1] = n[1];
    o[2] = n[2];
}

// vn: the vertex normals [B, Nv, 3] of k_vertex_normals (SMOOTH)
template <bool SMOOTH>
__global__ __launch_bounds__(256) void k_corner_normals(MeshArgs a, const float *__restrict__ vn, float *__restrict__ corner)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= a.Nf) return;
    int vi[3];
    float w[3][3], n[3][3];  // per corner
    load_face(a, b, f, vi, w);
    if (SMOOTH) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float *src = vn + ((size_t)b * a.Nv + vi[k]) * 3;
            n[k][0] = src[0];
            n[k][1] = src[1];
            n[k][2] = src[2];
        }
    } else {
        float v10[3], v12[3], N[3];
        face_normal(w, v10, v12, N);
        normalize3(N, n[0]);
#pragma unroll
        for (int c = 0; c < 3; c++) n[1][c] = n[2][c] = n[0][c];
    }
    const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
    float *of = corner + ((size_t)b * Fout + f) * 9;
    float *ob = corner + ((size_t)b * Fout + a.Nf + f) * 9;
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            of[3 * k + c] = n[k][c];
            if (a.fill_back) ob[3 * (2 - k) + c] = -n[k][c];  // reversed corner order, negated normal
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------
// backward

// g_m [B, Nv, 3]; g: grad_normals [B, Nv, 3], or (CORNER) grad_corner [B, F, 3, 3]
template <bool CORNER>
__global__ __launch_bounds__(256) void k_vertex_stage(MeshArgs a, const float *__restrict__ g, float *__restrict__ gm)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    float s[3] = {0.0f, 0.0f, 0.0f};
    if (CORNER) {
        const float *gcb = g + (size_t)b * (a.fill_back ? 2 * a.Nf : a.Nf) * 9;
        int e0, e1;
        const int32_t *ent = adjacency(a, b, v, e0, e1);
        for (int e = e0; e < e1; e++) {
            const int fk = clampi(ent[e], 0, 3 * a.Nf - 1), f = fk / 3, k = fk - 3 * f;
            float t[3];
            corner_grad(a, gcb, f, k, t);
            s[0] += t[0];
            s[1] += t[1];
            s[2] += t[2];
        }
    } else {
        const float *src = g + ((size_t)b * a.Nv + v) * 3;
        s[0] = src[0];
        s[1] = src[1];
        s[2] = src[2];
    }
    float m[3], o[3];
    normal_sum(a, b, v, m);
    normalize3_bwd(m, s, o);
    float *out = gm + ((size_t)b * a.Nv + v) * 3;
    out[0] = o[0];
    out[1] = o[1];
    out[2] = o[2];
}

// g_N [B, Nf, 3]; g: grad_normals [B, Nf, 3], or (CORNER) grad_corner [B, F, 3, 3]: (g_0 + g_1) + g_2 over the corners
template <bool CORNER>
__global__ __launch_bounds__(256) void k_face_stage(MeshArgs a, const float *__restrict__ g, float *__restrict__ gN)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= a.Nf) return;
    float s[3];
    if (CORNER) {
        const float *gcb = g + (size_t)b * (a.fill_back ? 2 * a.Nf : a.Nf) * 9;
        float t0[3], t1[3], t2[3];
        corner_grad(a, gcb, f, 0, t0);
        corner_grad(a, gcb, f, 1, t1);
        corner_grad(a, gcb, f, 2, t2);
#pragma unroll
        for (int c = 0; c < 3; c++) s[c] = (t0[c] + t1[c]) + t2[c];
    } else {
        const float *src = g + ((size_t)b * a.Nf + f) * 3;
        s[0] = src[0];
        s[1] = src[1];
        s[2] = src[2];
    }
    int vi[3];
    float w[3][3], v10[3], v12[3], N[3], o[3];
    load_face(a, b, f, vi, w);
    face_normal(w, v10, v12, N);
    normalize3_bwd(N, s, o);
    float *out = gN + ((size_t)b * a.Nf + f) * 3;
    out[0] = o[0];
    out[1] = o[1];
    out[2] = o[2];
}

// --------------------------------------------------------------------------------------------------------------------
// host

size_t n_workspace(int B, int Nv, int Nf) { return (size_t)B * (size_t)(Nv > Nf ? Nv : Nf) * 3 * sizeof(float); }

}  // namespace

NR_API size_t nr_normals_workspace_bytes(int32_t B, int32_t Nv, int32_t Nf)
{
    return mesh_sizes_ok(B, Nv, Nf) ? n_workspace(B, Nv, Nf) : 0;
}

NR_API int nr_vertex_normals_forward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                     const int32_t *adj_entries, float *normals, int32_t B, int32_t Nv, int32_t Nf,
                                     int32_t idx_per_batch, void *stream)
{
    MeshArgs a;
    if (!normals) return NR_E_NULL;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, 0, true, a)) return e;
    hipLaunchKernelGGL(k_vertex_normals, grid_of(Nv, B), dim3(256), 0, (hipStream_t)stream, a, normals);
    return launch_status();
}

NR_API int nr_vertex_normals_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                      const int32_t *adj_entries, const float *grad_normals, float *grad_vertices,
                                      int32_t B, int32_t Nv, int32_t Nf, int32_t idx_per_batch, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    MeshArgs a;
    if (!grad_normals || !grad_vertices) return NR_E_NULL;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, 0, true, a)) return e;
    if (!workspace || workspace_bytes < n_workspace(B, Nv, Nf)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *gm = (float *)workspace;
    hipLaunchKernelGGL(k_vertex_stage<false>, grid_of(Nv, B), dim3(256), 0, st, a, grad_normals, gm);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_normals_gather<true>, grid_of(Nv, B), dim3(256), 0, st, a, gm, grad_vertices);
    return launch_status();
}

NR_API int nr_face_normals_forward(const float *vertices, const int32_t *faces_idx, float *normals, int32_t B, int32_t Nv,
                                   int32_t Nf, int32_t idx_per_batch, void *stream)
{
    MeshArgs a;
    if (!normals) return NR_E_NULL;
    if (int e = mesh_args(vertices, faces_idx, nullptr, nullptr, B, Nv, Nf, idx_per_batch, 0, false, a)) return e;
    hipLaunchKernelGGL(k_face_normals, grid_of(Nf, B), dim3(256), 0, (hipStream_t)stream, a, normals);
    return launch_status();
}

NR_API int nr_face_normals_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                    const int32_t *adj_entries, const float *grad_normals, float *grad_vertices, int32_t B,
                                    int32_t Nv, int32_t Nf, int32_t idx_per_batch, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    MeshArgs a;
    if (!grad_normals || !grad_vertices) return NR_E_NULL;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, 0, true, a)) return e;
    if (!workspace || workspace_bytes < n_workspace(B, Nv, Nf)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *gN = (float *)workspace;
    hipLaunchKernelGGL(k_face_stage<false>, grid_of(Nf, B), dim3(256), 0, st, a, grad_normals, gN);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_normals_gather<false>, grid_of(Nv, B), dim3(256), 0, st, a, gN, grad_vertices);
    return launch_status();
}

NR_API int nr_corner_normals_forward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                     const int32_t *adj_entries, float *corner, int32_t B, int32_t Nv, int32_t Nf,
                                     int32_t idx_per_batch, int32_t fill_back, int32_t smooth, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    MeshArgs a;
    if (!corner) return NR_E_NULL;
    if (smooth != 0 && smooth != 1) return NR_E_MODE;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, fill_back, smooth != 0, a)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (!smooth) {
        hipLaunchKernelGGL(k_corner_normals<false>, grid_of(Nf, B), dim3(256), 0, st, a, nullptr, corner);
        return launch_status();
    }
    if (!workspace || workspace_bytes < n_workspace(B, Nv, Nf)) return NR_E_WORKSPACE;
    float *vn = (float *)workspace;
    hipLaunchKernelGGL(k_vertex_normals, grid_of(Nv, B), dim3(256), 0, st, a, vn);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_corner_normals<true>, grid_of(Nf, B), dim3(256), 0, st, a, vn, corner);
    return launch_status();
}

NR_API int nr_corner_normals_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                      const int32_t *adj_entries, const float *grad_corner, float *grad_vertices, int32_t B,
                                      int32_t Nv, int32_t Nf, int32_t idx_per_batch, int32_t fill_back, int32_t smooth,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    MeshArgs a;
    if (!grad_corner || !grad_vertices) return NR_E_NULL;
    if (smooth != 0 && smooth != 1) return NR_E_MODE;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, fill_back, true, a)) return e;
    if (!workspace || workspace_bytes < n_workspace(B, Nv, Nf)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    if (smooth) {
        hipLaunchKernelGGL(k_vertex_stage<true>, grid_of(Nv, B), dim3(256), 0, st, a, grad_corner, ws);
        if (int rc = launch_status()) return rc;
        hipLaunchKernelGGL(k_normals_gather<true>, grid_of(Nv, B), dim3(256), 0, st, a, ws, grad_vertices);
        return launch_status();
    }
    hipLaunchKernelGGL(k_face_stage<true>, grid_of(Nf, B), dim3(256), 0, st, a, grad_corner, ws);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_normals_gather<false>, grid_of(Nv, B), dim3(256), 0, st, a, ws, grad_vertices);
    return launch_status();
}
