// nr_mesh_gather.h -- the geometry that every operator on the vertex -> (face, corner) table shares (nr_normals.hip,
// nr_vertex_colors.hip, nr_lights.hip): a face's vertices, a vertex's table entries, the unnormalised face normal, the normal
// sum around a vertex, a corner's share of a normal's gradient, and the gather of grad_vertices from the normals' gradients.
// One definition, in one float32 operation order, so that the operators agree bit for bit (DESIGN "Normal maps"):
//   N_f = cross(v0 - v1, v2 - v1); m_v = the sum of N_f over the (face, corner) pairs of v in ascending 3 f + k order.
// Every sum around a vertex is a GATHER through the table: no atomics, every output element stored, the same bits in every run.
#pragma once
#include "nr_device.h"
#include "nr_shade.h"

namespace nr {

// the mesh of a call; the operators' own argument structs derive from it
struct MeshArgs {
    const float *vertices;     // [B, Nv, 3] world space
    const int32_t *idx;        // [Bt, Nf, 3]
    const int32_t *adj_off;    // [Bt, Nv + 1]
    const int32_t *adj_ent;    // [Bt, 3 Nf]: 3 f + k, ascending within a vertex
    int B, Nv, Nf;
    int idx_per_batch, fill_back;
};

// face f of image b: its vertex numbers (clamped for memory safety; the host validates them) and world-space vertices
__device__ __forceinline__ void load_face(const MeshArgs &a, int b, int f, int vi[3], float w[3][3])
{
    const int32_t *idx = a.idx + ((size_t)(a.idx_per_batch ? b : 0) * a.Nf + f) * 3;
    const float *vb = a.vertices + (size_t)b * a.Nv * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        vi[k] = clampi(idx[k], 0, a.Nv - 1);
        const float *src = vb + (size_t)vi[k] * 3;
        w[k][0] = src[0];
        w[k][1] = src[1];
        w[k][2] = src[2];
    }
}

// the table entries of vertex v in image b: [e0, e1) into the returned array
__device__ __forceinline__ const int32_t *adjacency(const MeshArgs &a, int b, int v, int &e0, int &e1)
{
    const size_t t = a.idx_per_batch ? b : 0;
    const int32_t *off = a.adj_off + t * ((size_t)a.Nv + 1);
    e0 = clampi(off[v], 0, 3 * a.Nf);
    e1 = clampi(off[v + 1], e0, 3 * a.Nf);
    return a.adj_ent + t * 3 * (size_t)a.Nf;
}

// unnormalised face normal cross(v0 - v1, v2 - v1) (lighting.py:36-39), and the two edges
__device__ __forceinline__ void face_normal(const float w[3][3], float *v10, float *v12, float *n)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v10[c] = w[0][c] - w[1][c];
        v12[c] = w[2][c] - w[1][c];
    }
    cross3(v10, v12, n);
}

// m_v: the face normals around vertex v, summed in float32 in ascending (face, corner) order (area-weighted)
__device__ __forceinline__ void normal_sum(const MeshArgs &a, int b, int v, float *m)
{
    m[0] = m[1] = m[2] = 0.0f;
    int e0, e1;
    const int32_t *ent = adjacency(a, b, v, e0, e1);
    for (int e = e0; e < e1; e++) {
        int vi[3];
        float w[3][3], v10[3], v12[3], n[3];
        load_face(a, b, clampi(ent[e], 0, 3 * a.Nf - 1) / 3, vi, w);
        face_normal(w, v10, v12, n);
        m[0] += n[0];
        m[1] += n[1];
        m[2] += n[2];
    }
}

// gradient of corner k of a face from the gradient gn of its unnormalised normal n = v10 x v12
__device__ __forceinline__ void normal_to_corner(const float *v10, const float *v12, const float *gn, int k, float *o)
{
    float ga[3], gb[3];
    cross3(v12, gn, ga);  // g_v10
    cross3(gn, v10, gb);  // g_v12
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = k == 0 ? ga[c] : (k == 2 ? gb[c] : -(ga[c] + gb[c]));
}

// grad_vertices[b, v] = the sum over the faces around v, in table order, of corner k's share of g_N(f); ws: g_N [B, Nf, 3], or
// (SMOOTH) g_m [B, Nv, 3] with g_N(f) = (g_m(v0) + g_m(v1)) + g_m(v2): every face around a vertex takes part in the normal
// sums of its three vertices.  The last launch of every backward to the vertices that goes through normals.
template <bool SMOOTH>
static __global__ __launch_bounds__(256) void k_normals_gather(MeshArgs a, const float *__restrict__ ws,
                                                               float *__restrict__ grad_vertices)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    float g[3] = {0.0f, 0.0f, 0.0f};
    int e0, e1;
    const int32_t *ent = adjacency(a, b, v, e0, e1);
    const float *wsb = ws + (size_t)b * (SMOOTH ? a.Nv : a.Nf) * 3;
    for (int e = e0; e < e1; e++) {
        const int fk = clampi(ent[e], 0, 3 * a.Nf - 1), f = fk / 3, k = fk - 3 * f;
        int vi[3];
        float w[3][3], v10[3], v12[3], n[3], gn[3], o[3];
        load_face(a, b, f, vi, w);
        face_normal(w, v10, v12, n);
#pragma unroll
        for (int c = 0; c < 3; c++)
            gn[c] = SMOOTH ? (wsb[(size_t)vi[0] * 3 + c] + wsb[(size_t)vi[1] * 3 + c]) + wsb[(size_t)vi[2] * 3 + c]
                           : wsb[(size_t)f * 3 + c];
        normal_to_corner(v10, v12, gn, k, o);
        g[0] += o[0];
        g[1] += o[1];
        g[2] += o[2];
    }
    float *out = grad_vertices + ((size_t)b * a.Nv + v) * 3;
    out[0] = g[0];
    out[1] = g[1];
    out[2] = g[2];
}

// --------------------------------------------------------------------------------------------------------------------
// host

// B on grid.y; int32 indexing of the [B, 2 Nf, 3, 3] corner and the [B, Nv, 6] light arrays inside the kernels
inline bool mesh_sizes_ok(int B, int Nv, int Nf)
{
    if (B < 1 || B > 65535 || Nv < 1 || Nf < 1) return false;
    return (size_t)B * (size_t)Nf <= 0x7fffffffull / 18 && (size_t)B * (size_t)Nv <= 0x7fffffffull / 6;
}

// the argument checks that every call on a mesh shares (NR_E_NULL before NR_E_SIZE), then the mesh's part of the arguments
inline int mesh_args(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets, const int32_t *adj_entries,
                     int B, int Nv, int Nf, int idx_per_batch, int fill_back, bool need_adjacency, MeshArgs &a)
{
    if (!vertices || !faces_idx) return NR_E_NULL;
    if (need_adjacency && (!adj_offsets || !adj_entries)) return NR_E_NULL;
    if (!mesh_sizes_ok(B, Nv, Nf)) return NR_E_SIZE;
    a.vertices = vertices; a.idx = faces_idx; a.adj_off = adj_offsets; a.adj_ent = adj_entries;
    a.B = B; a.Nv = Nv; a.Nf = Nf;
    a.idx_per_batch = idx_per_batch != 0;
    a.fill_back = fill_back != 0;
    return 0;
}

// one thread per item (vertex or face) of every image, 256 to a block
inline dim3 grid_of(int n, int B) { return dim3((unsigned)((n + 255) / 256), (unsigned)B); }

}  // namespace nr
