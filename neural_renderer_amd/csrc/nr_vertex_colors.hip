// nr_vertex_colors.hip -- vertex colours and smooth shading (include/nr_hip.h; DESIGN K10 "Vertex colours").
//
// The rasterizer side.  The forward is the corner instantiation of the resolve pass (nr_forward.hip: shade_pixel<SHADE_CORNER>):
// three lit colours per face, interpolated perspective-correctly at every covered pixel.  Its backward to the colours:
//   k_corner_gather       4 lanes per face: faces of up to CORNER_BIG candidate pixels scan their candidates (K7's gather:
//                         face_candidates / cand_pixel), recompute the forward's weights d_k at the pixels they own and sum
//                         g_c * d_k in double in a fixed order -- no atomics, every element stored (zeros without a pixel);
//                         larger faces are flagged and get their nine double sums zeroed
//   k_corner_backward     one thread per pixel, flagged faces only: adds g_c * d_k into the face's double sums (the lanes of a
//                         wave that share a face sum first: one atomic per run and sum)
//   k_corner_round        the flagged faces' double sums -> grad_corner, rounded once
// grad_faces is the rasterizer's own backward (K6 + K8 read the maps), as for per-pixel UV images.
//
// The vertex side (nr_vertex_shade_forward / _backward): corner colours = vertex colours times light, the light per face
// (flat, exactly the front-end's face_light) or per vertex from area-weighted vertex normals (smooth, Gouraud).  Every sum
// over the faces around a vertex is a GATHER through a vertex -> (face, corner) table in ascending (face, corner) order: no
// atomics in either direction, the same bits in every run.
//   k_vertex_light          smooth forward 1: (image, vertex) -> the light colours seen by the front and the reversed copies
//   k_corner_colors<SMOOTH> forward: (image, face) -> the nine numbers of the face and of its reversed copy
//   k_vs_backward<SMOOTH>   (image, vertex): grad_colors of a batch of colours; flat: grad_vertices; smooth: g_m, the
//                           gradient of the vertex's normal sum, into the workspace
//   k_vs_backward_shared<SMOOTH>  colours shared by the batch: a wave per vertex, the lanes take the images, double sums
//                           combined in the fixed order of the butterfly
//   k_normals_gather<true>  smooth 2 (nr_mesh_gather.h): (image, vertex) -> grad_vertices from g_N(f) = g_m(v0) + g_m(v1) + g_m(v2)
// The mesh arguments and the geometry helpers (load_face, adjacency, face_normal, normal_sum, normal_to_corner) are
// nr_mesh_gather.h's, shared with nr_normals.hip and nr_lights.hip.
#include "nr_mesh_gather.h"

using namespace nr;

namespace {

// --------------------------------------------------------------------------------------------------------------------
// rasterizer: backward to the corner colours

// lanes per face in k_corner_gather: a face owns ~5 pixels of ~20 candidates at the shapes that matter, and the cross-lane
// sums cost more than the scan (16 lanes: 99 us at the headline shape, the nine double butterflies of every wave)
constexpr int CORNER_LANES = 4;
constexpr int CORNER_BIG = 1024;   // candidate pixels above which a face goes to the per-pixel kernel (256 trips per lane)

// the forward's weights of pixel p owned by `face`
__device__ __forceinline__ void corner_weights(const float *__restrict__ face, const float *__restrict__ weight_map,
                                               const float *__restrict__ depth_map, size_t p, float d[3])
{
    const float zp = depth_map[p];
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = fminf(fmaxf(weight_map[3 * p + k] * (zp / face[3 * k + 2]), 0.0f), 1.0f);
}

// visible: the forward's per-face "owns a pixel" flags, or NULL (every face scans its candidates)
__global__ __launch_bounds__(256) void k_corner_gather(const float *__restrict__ faces,
                                                       const int32_t *__restrict__ face_index_map,
                                                       const float *__restrict__ weight_map,
                                                       const float *__restrict__ depth_map,
                                                       const float *__restrict__ grad_rgb_map,
                                                       const unsigned char *__restrict__ visible,
                                                       float *__restrict__ grad_corner, double *__restrict__ acc,
                                                       unsigned char *__restrict__ big, int F, int S, size_t n_faces)
{
    const size_t gf = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / CORNER_LANES;  // b * F + f
    const int sub = threadIdx.x % CORNER_LANES;
    const bool live = gf < n_faces;
    double s9[9];
#pragma unroll
    for (int j = 0; j < 9; j++) s9[j] = 0.0;
    bool is_big = false;
    if (live && (!visible || visible[gf])) {
        const float *face = faces + gf * 9;
        const int b = (int)(gf / F), f = (int)(gf - (size_t)b * F);
        const Cand cd = face_candidates(face[0], face[1], face[3], face[4], face[6], face[7], S);
        is_big = cd.n > CORNER_BIG;
        const size_t img = (size_t)b * S * S;
        for (int i = sub; !is_big && i < cd.n; i += CORNER_LANES) {
            int x, y;
            if (!cand_pixel(cd, i, S, x, y)) continue;
            const size_t p = img + (size_t)y * S + x;
            if (face_index_map[p] != f) continue;
            float d[3];
            corner_weights(face, weight_map, depth_map, p, d);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double g = (double)grad_rgb_map[3 * p + c];
#pragma unroll
                for (int k = 0; k < 3; k++) s9[3 * k + c] += g * (double)d[k];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 9; j++)
#pragma unroll
        for (int o = CORNER_LANES / 2; o > 0; o >>= 1) s9[j] += __shfl_xor(s9[j], o, CORNER_LANES);
    if (!live) return;
    if (sub == 0) big[gf] = is_big ? 1 : 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {  // the nine stores dealt to the face's lanes
        if (j % CORNER_LANES != sub) continue;
        if (is_big) acc[gf * 9 + j] = 0.0;
        else grad_corner[gf * 9 + j] = (float)s9[j];
    }
}

__global__ __launch_bounds__(256) void k_corner_backward(const float *__restrict__ faces,
                                                         const int32_t *__restrict__ face_index_map,
                                                         const float *__restrict__ weight_map,
                                                         const float *__restrict__ depth_map,
                                                         const float *__restrict__ grad_rgb_map, double *__restrict__ acc,
                                                         const unsigned char *__restrict__ big, int F, int S,
                                                         size_t n_pixels)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int fi = i < n_pixels ? face_index_map[i] : -1;
    int key = -1;  // b * F + fi of a covered pixel of a flagged face
    float g[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    if (fi >= 0 && fi < F && big[(size_t)(i / ((size_t)S * S)) * F + fi]) {
        const int b = (int)(i / ((size_t)S * S));
        key = b * F + fi;
        corner_weights(faces + (size_t)key * 9, weight_map, depth_map, i, d);
#pragma unroll
        for (int k = 0; k < 3; k++) g[k] = grad_rgb_map[3 * i + k];
    }
    // The pixels of a wave are consecutive in a row, so the lanes that share a face form runs (a face may have several: a
    // wave can span rows).  A segmented doubling sum adds up every run at once -- lane l takes lane l + o while that lane
    // lies in its run, o = 1 .. 32 -- and the first lane of each run sends the run's nine sums as double atomics.  Float: a
    // product and a tree of depth 6 are 7 roundings, 4.2e-7 of the sum of |terms| at most, whatever the number of pixels;
    // everything beyond a run is summed in double.
    if (__ballot(key >= 0) == 0) return;  // (wave-uniform: no pixel of a flagged face)
    const int lane = threadIdx.x & (WAVE - 1);
    const int prev = __shfl_up(key, 1, WAVE);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
    const int run_end = above ? lane + __ffsll(above) : WAVE;  // one past the last lane of this lane's run
    float s9[9];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) s9[3 * k + c] = g[c] * d[k];
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const bool take = lane + o < run_end;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const float v = __shfl_down(s9[j], o, WAVE);
            if (take) s9[j] += v;
        }
    }
    if (key >= 0 && head) {
#pragma unroll
        for (int j = 0; j < 9; j++)
            if (s9[j] != 0.0f) atomicAdd(acc + (size_t)key * 9 + j, (double)s9[j]);
    }
}

__global__ __launch_bounds__(256) void k_corner_round(const double *__restrict__ acc, const unsigned char *__restrict__ big,
                                                      float *__restrict__ grad_corner, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && big[i / 9]) grad_corner[i] = (float)acc[i];
}

// --------------------------------------------------------------------------------------------------------------------
// vertex shading

struct VSArgs : MeshArgs {
    const float *colors;       // [Bc, Nv, 3]
    int colors_shared;
    FrontendParams P;          // the light (the camera fields stay 0)
};

__device__ __forceinline__ const float *color_of(const VSArgs &a, int b, int v)
{
    return a.colors + ((size_t)(a.colors_shared ? 0 : b) * a.Nv + v) * 3;
}

// face_light's arithmetic on a vertex's normal sum m: the colours seen by the faces and by their reversed copies
__device__ __forceinline__ void vertex_light(const FrontendParams &P, const float *m, float &dotn, float *light_f,
                                             float *light_b)
{
    float cos_f = 0.0f, cos_b = 0.0f;
    dotn = 0.0f;
    if (P.has_directional) {
        float nh[3];
        normalize3(m, nh);
        dotn = dot3(nh, P.ldir);
        cos_f = fmaxf(dotn, 0.0f);
        cos_b = fmaxf(-dotn, 0.0f);  // the reversed copy sees the negated normal
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float amb = P.ia != 0.0f ? P.ia * P.ca[c] : 0.0f;
        light_f[c] = P.has_directional ? amb + P.id * (P.cd[c] * cos_f) : amb;
        light_b[c] = P.has_directional ? amb + P.id * (P.cd[c] * cos_b) : amb;
    }
}

// d loss / d (n_hat . direction) from the gradients of the two light colours
__device__ __forceinline__ float light_dot_bwd(const FrontendParams &P, float dotn, const float *glf, const float *glb)
{
    const float gcf = P.id * (P.cd[0] * glf[0] + P.cd[1] * glf[1] + P.cd[2] * glf[2]);
    const float gcb = P.id * (P.cd[0] * glb[0] + P.cd[1] * glb[1] + P.cd[2] * glb[2]);
    float gdot = 0.0f;  // relu: the front copy sees dotn, the back copy -dotn
    if (dotn > 0.0f) gdot += gcf;
    if (-dotn > 0.0f) gdot -= gcb;
    return gdot;
}

__global__ __launch_bounds__(256) void k_vertex_light(VSArgs a, float *__restrict__ vlight)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    float m[3] = {0.0f, 0.0f, 0.0f}, dotn, lf[3], lb[3];
    if (a.P.has_directional) normal_sum(a, b, v, m);
    vertex_light(a.P, m, dotn, lf, lb);
    float *o = vlight + ((size_t)b * a.Nv + v) * 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[c] = lf[c];
        o[3 + c] = lb[c];
    }
}

template <bool SMOOTH>
__global__ __launch_bounds__(256) void k_corner_colors(VSArgs a, const float *__restrict__ vlight, float *__restrict__ corner)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= a.Nf) return;
    int vi[3];
    float w[3][3];
    load_face(a, b, f, vi, w);
    float lf[3][3], lb[3][3];  // per corner
    if (SMOOTH) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float *l = vlight + ((size_t)b * a.Nv + vi[k]) * 6;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                lf[k][c] = l[c];
                lb[k][c] = l[3 + c];
            }
        }
    } else {
        float n[3], dotn;
        face_light(a.P, w[0], w[1], w[2], n, dotn, lf[0], lb[0]);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lf[1][c] = lf[2][c] = lf[0][c];
            lb[1][c] = lb[2][c] = lb[0][c];
        }
    }
    const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
    float *of = corner + ((size_t)b * Fout + f) * 9;
    float *ob = corner + ((size_t)b * Fout + a.Nf + f) * 9;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *col = color_of(a, b, vi[k]);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            of[3 * k + c] = col[c] * lf[k][c];
            if (a.fill_back) ob[3 * (2 - k) + c] = col[c] * lb[k][c];  // reversed corner order
        }
    }
}

// What vertex v of image b contributes: gcol = the gradient of its colour (double), and -- when `geom` -- gout = its
// gradient (flat) or the gradient of its normal sum (smooth) from the light terms.
template <bool SMOOTH>
__device__ __forceinline__ void vertex_backward(const VSArgs &a, const float *__restrict__ gc, int b, int v, bool geom,
                                                double gcol[3], float gout[3])
{
    const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
    const float *gcb = gc + (size_t)b * Fout * 9;
    gcol[0] = gcol[1] = gcol[2] = 0.0;
    gout[0] = gout[1] = gout[2] = 0.0f;
    int e0, e1;
    const int32_t *ent = adjacency(a, b, v, e0, e1);
    if (SMOOTH) {
        double sf[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};  // the corner gradients around the vertex
        for (int e = e0; e < e1; e++) {
            const int fk = clampi(ent[e], 0, 3 * a.Nf - 1), f = fk / 3, k = fk - 3 * f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                sf[c] += (double)gcb[(size_t)f * 9 + 3 * k + c];
                if (a.fill_back) sb[c] += (double)gcb[((size_t)a.Nf + f) * 9 + 3 * (2 - k) + c];
            }
        }
        float m[3] = {0.0f, 0.0f, 0.0f}, dotn, lf[3], lb[3];
        if (a.P.has_directional) normal_sum(a, b, v, m);
        vertex_light(a.P, m, dotn, lf, lb);
#pragma unroll
        for (int c = 0; c < 3; c++) gcol[c] = sf[c] * (double)lf[c] + sb[c] * (double)lb[c];
        if (geom && a.P.has_directional) {
            const float *col = color_of(a, b, v);
            const float glf[3] = {(float)((double)col[0] * sf[0]), (float)((double)col[1] * sf[1]), (float)((double)col[2] * sf[2])};
            const float glb[3] = {(float)((double)col[0] * sb[0]), (float)((double)col[1] * sb[1]), (float)((double)col[2] * sb[2])};
            const float gdot = light_dot_bwd(a.P, dotn, glf, glb);
            if (gdot != 0.0f) {
                const float gnh[3] = {gdot * a.P.ldir[0], gdot * a.P.ldir[1], gdot * a.P.ldir[2]};
                normalize3_bwd(m, gnh, gout);
            }
        }
        return;
    }
    for (int e = e0; e < e1; e++) {
        const int fk = clampi(ent[e], 0, 3 * a.Nf - 1), f = fk / 3, k = fk - 3 * f;
        int vi[3];
        float w[3][3], n[3] = {0.0f, 0.0f, 0.0f}, dotn, lf[3], lb[3];
        load_face(a, b, f, vi, w);
        face_light(a.P, w[0], w[1], w[2], n, dotn, lf, lb);
        const float *gf = gcb + (size_t)f * 9, *gb = gcb + ((size_t)a.Nf + f) * 9;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            gcol[c] += (double)gf[3 * k + c] * (double)lf[c];
            if (a.fill_back) gcol[c] += (double)gb[3 * (2 - k) + c] * (double)lb[c];
        }
        if (geom && a.P.has_directional) {
            float glf[3] = {0.0f, 0.0f, 0.0f}, glb[3] = {0.0f, 0.0f, 0.0f};  // the gradients of the face's two light colours
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float *col = color_of(a, b, vi[j]);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    glf[c] += gf[3 * j + c] * col[c];
                    if (a.fill_back) glb[c] += gb[3 * (2 - j) + c] * col[c];
                }
            }
            const float gdot = light_dot_bwd(a.P, dotn, glf, glb);
            if (gdot != 0.0f) {
                const float gnh[3] = {gdot * a.P.ldir[0], gdot * a.P.ldir[1], gdot * a.P.ldir[2]};
                float gn[3], v10[3], v12[3], nn[3], o[3];
                normalize3_bwd(n, gnh, gn);
                face_normal(w, v10, v12, nn);
                normal_to_corner(v10, v12, gn, k, o);
                gout[0] += o[0];
                gout[1] += o[1];
                gout[2] += o[2];
            }
        }
    }
}

// grad_colors [B, Nv, 3] (or NULL) and gout [B, Nv, 3] (or NULL): grad_vertices (flat) / g_m (smooth)
template <bool SMOOTH>
__global__ __launch_bounds__(256) void k_vs_backward(VSArgs a, const float *__restrict__ gc, float *__restrict__ grad_colors,
                                                     float *__restrict__ gout)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    double gcol[3];
    float g[3];
    vertex_backward<SMOOTH>(a, gc, b, v, gout != nullptr, gcol, g);
    const size_t o = ((size_t)b * a.Nv + v) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (grad_colors) grad_colors[o + c] = (float)gcol[c];
        if (gout) gout[o + c] = g[c];
    }
}

// colours shared by the batch: grad_colors [Nv, 3] = the sum over the images.  A wave per vertex; lane l takes the images l,
// l + 64, ... in ascending order, the lanes' double sums are combined by the butterfly: one fixed order, rounded once.
template <bool SMOOTH>
__global__ __launch_bounds__(256) void k_vs_backward_shared(VSArgs a, const float *__restrict__ gc, float *__restrict__ grad_colors)
{
    const int v = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (v >= a.Nv) return;  // (whole waves leave)
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = lane; b < a.B; b += WAVE) {
        double gcol[3];
        float unused[3];
        vertex_backward<SMOOTH>(a, gc, b, v, false, gcol, unused);
        s[0] += gcol[0];
        s[1] += gcol[1];
        s[2] += gcol[2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] = wave_sum(s[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) grad_colors[(size_t)v * 3 + c] = (float)s[c];
    }
}

// every argument check of the two vertex-shading calls, then the kernels' arguments
int vs_args(const float *vertices, const int32_t *faces_idx, const float *colors, const int32_t *adj_offsets,
            const int32_t *adj_entries, int B, int Nv, int Nf, int color_batch, int idx_per_batch, int fill_back,
            const nr_light *light, bool need_adjacency, VSArgs &a)
{
    if (!colors || !light) return NR_E_NULL;
    a = {};
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, fill_back, need_adjacency, a))
        return e;
    if (color_batch != 1 && color_batch != B) return NR_E_SIZE;
    a.colors = colors;
    a.colors_shared = (color_batch == 1 && B > 1) ? 1 : 0;
    a.P.fill_back = a.fill_back;
    a.P.ia = light->intensity_ambient;
    a.P.id = light->intensity_directional;
    a.P.has_directional = light->intensity_directional != 0.0f;
    for (int k = 0; k < 3; k++) {
        a.P.ca[k] = light->color_ambient[k];
        a.P.cd[k] = light->color_directional[k];
        a.P.ldir[k] = light->direction[k];
    }
    return 0;
}

size_t vs_workspace(int B, int Nv) { return (size_t)B * Nv * 6 * sizeof(float); }

}  // namespace

NR_API size_t nr_backward_corner_colors_workspace_bytes(int32_t B, int32_t F)
{
    if (check_sizes(B, F, 1)) return 0;
    return (size_t)B * F * 9 * sizeof(double) + (size_t)B * F;  // the double sums, then a flag per face
}

NR_API int nr_backward_corner_colors(const float *faces, const int32_t *face_index_map, const float *weight_map,
                                     const float *depth_map, const float *grad_rgb_map, const uint8_t *visible_faces,
                                     float *grad_corner, int32_t B, int32_t F, int32_t S, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    if (!faces || !face_index_map || !weight_map || !depth_map || !grad_rgb_map || !grad_corner) return NR_E_NULL;
    if (int e = check_sizes(B, F, S)) return e;
    const size_t n = (size_t)B * S * S, n_faces = (size_t)B * F, n_sums = n_faces * 9;
    if (n > 0xffffff00ull || n_faces * CORNER_LANES > 0xffffff00ull) return NR_E_SIZE;  // (1-D grids)
    if (!workspace || workspace_bytes < n_sums * sizeof(double) + n_faces) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *acc = (double *)workspace;
    unsigned char *big = (unsigned char *)(acc + n_sums);
    hipLaunchKernelGGL(k_corner_gather, dim3((unsigned)((n_faces * CORNER_LANES + 255) / 256)), dim3(256), 0, st, faces,
                       face_index_map, weight_map, depth_map, grad_rgb_map, visible_faces, grad_corner, acc, big, F, S, n_faces);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_corner_backward, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, faces, face_index_map,
                       weight_map, depth_map, grad_rgb_map, acc, big, F, S, n);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_corner_round, dim3((unsigned)((n_sums + 255) / 256)), dim3(256), 0, st, acc, big, grad_corner, n_sums);
    return launch_status();
}

NR_API size_t nr_vertex_shade_workspace_bytes(int32_t B, int32_t Nv)
{
    if (B < 1 || B > 65535 || Nv < 1 || (size_t)B * (size_t)Nv > 0x7fffffffull / 6) return 0;
    return vs_workspace(B, Nv);
}

NR_API int nr_vertex_shade_forward(const float *vertices, const int32_t *faces_idx, const float *colors,
                                   const int32_t *adj_offsets, const int32_t *adj_entries, float *corner_colors, int32_t B,
                                   int32_t Nv, int32_t Nf, int32_t color_batch, int32_t idx_per_batch, int32_t fill_back,
                                   int32_t smooth, const nr_light *light, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    VSArgs a;
    if (!corner_colors) return NR_E_NULL;
    if (smooth != 0 && smooth != 1) return NR_E_MODE;
    if (int e = vs_args(vertices, faces_idx, colors, adj_offsets, adj_entries, B, Nv, Nf, color_batch, idx_per_batch,
                        fill_back, light, smooth != 0, a))
        return e;
    hipStream_t st = (hipStream_t)stream;
    if (!smooth) {
        hipLaunchKernelGGL(k_corner_colors<false>, grid_of(Nf, B), dim3(256), 0, st, a, nullptr, corner_colors);
        return launch_status();
    }
    if (!workspace || workspace_bytes < vs_workspace(B, Nv)) return NR_E_WORKSPACE;
    float *vlight = (float *)workspace;
    hipLaunchKernelGGL(k_vertex_light, grid_of(Nv, B), dim3(256), 0, st, a, vlight);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_corner_colors<true>, grid_of(Nf, B), dim3(256), 0, st, a, vlight, corner_colors);
    return launch_status();
}

NR_API int nr_vertex_shade_backward(const float *vertices, const int32_t *faces_idx, const float *colors,
                                    const int32_t *adj_offsets, const int32_t *adj_entries, const float *grad_corner,
                                    float *grad_colors, float *grad_vertices, int32_t B, int32_t Nv, int32_t Nf,
                                    int32_t color_batch, int32_t idx_per_batch, int32_t fill_back, int32_t smooth,
                                    const nr_light *light, void *workspace, size_t workspace_bytes, void *stream)
{
    VSArgs a;
    if (!grad_corner) return NR_E_NULL;
    if (!grad_colors && !grad_vertices) return NR_E_MODE;
    if (smooth != 0 && smooth != 1) return NR_E_MODE;
    if (int e = vs_args(vertices, faces_idx, colors, adj_offsets, adj_entries, B, Nv, Nf, color_batch, idx_per_batch,
                        fill_back, light, true, a))
        return e;
    if (smooth && grad_vertices && (!workspace || workspace_bytes < vs_workspace(B, Nv))) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *per_image_colors = a.colors_shared ? nullptr : grad_colors;
    if (grad_colors && a.colors_shared) {
        const dim3 grid((unsigned)((Nv + 256 / WAVE - 1) / (256 / WAVE)));
        if (smooth) hipLaunchKernelGGL(k_vs_backward_shared<true>, grid, dim3(256), 0, st, a, grad_corner, grad_colors);
        else hipLaunchKernelGGL(k_vs_backward_shared<false>, grid, dim3(256), 0, st, a, grad_corner, grad_colors);
        if (int rc = launch_status()) return rc;
    }
    if (!per_image_colors && !grad_vertices) return 0;
    if (!smooth) {
        hipLaunchKernelGGL(k_vs_backward<false>, grid_of(Nv, B), dim3(256), 0, st, a, grad_corner, per_image_colors, grad_vertices);
        return launch_status();
    }
    float *gm = grad_vertices ? (float *)workspace : nullptr;
    hipLaunchKernelGGL(k_vs_backward<true>, grid_of(Nv, B), dim3(256), 0, st, a, grad_corner, per_image_colors, gm);
    if (int rc = launch_status()) return rc;
    if (!grad_vertices) return 0;
    hipLaunchKernelGGL(k_normals_gather<true>, grid_of(Nv, B), dim3(256), 0, st, (const MeshArgs &)a, gm, grad_vertices);
    return launch_status();
}
