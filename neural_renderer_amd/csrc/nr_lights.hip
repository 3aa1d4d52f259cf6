// nr_lights.hip -- learnable lights (include/nr_hip.h: nr_light_colors_forward / _backward; DESIGN "Learnable lights"): the
// light colour of every face (flat) or face corner (smooth) from light parameters in DEVICE memory -- an ambient term, one
// directional lamp and nine spherical-harmonics irradiance coefficients, each shared by the batch or one per image -- with
// gradients to the vertices and to every parameter.  The result feeds the rasterizer's face_light input.
//
// Every sum around a vertex is a GATHER through the vertex -> (face, corner) table of nr_vertex_colors.hip, every sum over an
// image is reduced in the fixed order of nr_reduce.h: no atomics, the same bits in every run.
//   k_face_light           flat forward: (image, face) -> the colours of the face and of its reversed copy
//   k_vertex_light         smooth forward 1: (image, vertex) -> both colours into the workspace
//   k_corner_light         smooth forward 2: (image, face) -> the colours of its corners (the reversed copy's flipped)
//   k_vertex_grad<SMOOTH>  (image, vertex): flat: grad_vertices; smooth: g_m, the gradient of the vertex's normal sum
//   k_normals_gather<true> smooth 2 (nr_mesh_gather.h): (image, vertex): grad_vertices from g_N(f) = (g_m(v0) + g_m(v1)) + g_m(v2)
//   k_light_sums<SMOOTH>   (image, block of 256 faces / vertices): the 36 double sums of the block into the workspace
//   k_light_finish         (image, gradient element): the blocks in block order (ordered_sum; a shared parameter: the images in
//                          image order), the gradient formed in double and rounded once
//
// The mesh arguments and the geometry helpers (load_face, adjacency, face_normal, normal_sum, normal_to_corner) are
// nr_mesh_gather.h's, shared with nr_vertex_colors.hip and nr_normals.hip.  With sh = NULL the forward is bit for bit
// nr_vertex_shade_forward's light of a white mesh and grad_vertices nr_vertex_shade_backward's: the light's own arithmetic
// (light_eval, normal_bwd) follows nr_shade.h's face_light and nr_vertex_colors.hip's light_dot_bwd term by term
// (tests/test_lights_gpu.py compares them).
#include "nr_mesh_gather.h"

using namespace nr;

namespace {

constexpr int BLOCK = 256;
constexpr float SH_C0 = 0.282095f, SH_C1 = 0.488603f, SH_C2 = 1.092548f, SH_C3 = 0.315392f, SH_C4 = 0.546274f;

// the 36 sums of an image: S[1, c], S[cos, c], S[Y_k, c] (k = 0 .. 8), T
constexpr int SUM_ONE = 0, SUM_COS = 3, SUM_SH = 6, SUM_DIR = 33, NSUM = 36;
enum { NEED_ONE = 1, NEED_COS = 2, NEED_SH = 4, NEED_DIR = 8 };
// the gradient elements of an image: g_Ia, g_Id, g_Ca[3], g_Cd[3], g_dir[3], g_sh[27]
constexpr int NELEM = 38;

struct LArgs : MeshArgs {
    nr_lights lights;        // device pointers
};

// the light of one image in registers (sh: only with a.lights.sh)
struct Lamp {
    float ia, id, ca[3], cd[3], d[3], sh[27];
};

__device__ __forceinline__ const float *param(const LArgs &a, const float *p, int bit, int b, int n)
{
    return p + (((a.lights.per_image >> bit) & 1) ? (size_t)b * n : 0);
}

__device__ __forceinline__ void load_lamp(const LArgs &a, int b, Lamp &L)
{
    L.ia = *param(a, a.lights.intensity_ambient, 0, b, 1);
    L.id = *param(a, a.lights.intensity_directional, 1, b, 1);
    const float *ca = param(a, a.lights.color_ambient, 2, b, 3), *cd = param(a, a.lights.color_directional, 3, b, 3);
    const float *d = param(a, a.lights.direction, 4, b, 3);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        L.ca[c] = ca[c];
        L.cd[c] = cd[c];
        L.d[c] = d[c];
    }
    if (a.lights.sh) {
        const float *sh = param(a, a.lights.sh, 5, b, 27);
#pragma unroll
        for (int j = 0; j < 27; j++) L.sh[j] = sh[j];
    }
}

// Y_0 .. Y_8 at the unit vector u
__device__ __forceinline__ void sh_basis(const float *u, float *Y)
{
    const float x = u[0], y = u[1], z = u[2];
    Y[0] = SH_C0;
    Y[1] = SH_C1 * y;
    Y[2] = SH_C1 * z;
    Y[3] = SH_C1 * x;
    Y[4] = SH_C2 * x * y;
    Y[5] = SH_C2 * y * z;
    Y[6] = SH_C3 * (3.0f * z * z - 1.0f);
    Y[7] = SH_C2 * x * z;
    Y[8] = SH_C4 * (x * x - y * y);
}

// the light seen along the unit vector u, cosv = max(u . d, 0): face_light's two terms, then the SH terms one by one
__device__ __forceinline__ void light_eval(const Lamp &L, bool has_sh, const float *u, float cosv, float *out)
{
    float Y[9];
    if (has_sh) sh_basis(u, Y);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float amb = L.ia * L.ca[c];
        float l = amb + L.id * (L.cd[c] * cosv);
        if (has_sh) {
#pragma unroll
            for (int k = 0; k < 9; k++) l = l + L.sh[3 * k + c] * Y[k];
        }
        out[c] = l;
    }
}

// both colours from an unnormalised normal (sum) n: nh = normalize3(n), dotn = nh . d; the reversed copy sees -nh
__device__ __forceinline__ void both_lights(const Lamp &L, bool has_sh, const float *n, float *nh, float &dotn, float *lf,
                                            float *lb)
{
    normalize3(n, nh);
    dotn = dot3(nh, L.d);
    light_eval(L, has_sh, nh, fmaxf(dotn, 0.0f), lf);
    const float nb[3] = {-nh[0], -nh[1], -nh[2]};
    light_eval(L, has_sh, nb, fmaxf(-dotn, 0.0f), lb);
}

// d (sum_c G_c sum_k sh[k, c] Y_k(u)) / d u
__device__ __forceinline__ void sh_bwd(const Lamp &L, const float *u, const float *G, float *gu)
{
    float a[9];
#pragma unroll
    for (int k = 1; k < 9; k++) a[k] = (G[0] * L.sh[3 * k] + G[1] * L.sh[3 * k + 1]) + G[2] * L.sh[3 * k + 2];
    const float x = u[0], y = u[1], z = u[2];
    gu[0] = ((SH_C1 * a[3] + (SH_C2 * y) * a[4]) + (SH_C2 * z) * a[7]) + ((2.0f * SH_C4) * x) * a[8];
    gu[1] = ((SH_C1 * a[1] + (SH_C2 * x) * a[4]) + (SH_C2 * z) * a[5]) - ((2.0f * SH_C4) * y) * a[8];
    gu[2] = ((SH_C1 * a[2] + (SH_C2 * y) * a[5]) + ((6.0f * SH_C3) * z) * a[6]) + (SH_C2 * x) * a[7];
}

// The gradient gn of an unnormalised normal (sum) n from the gradients glf / glb of the two colours it lights (glb: only with
// `back`).  The lamp's part is nr_vertex_colors.hip's light_dot_bwd and g_nh = gdot d; the SH part of the reversed copy
// comes back through u = -nh.  n = 0: no gradient.
__device__ __forceinline__ void normal_bwd(const Lamp &L, bool has_sh, bool back, const float *n, const float *glf,
                                           const float *glb, float *gn)
{
    float nh[3];
    normalize3(n, nh);
    const float dotn = dot3(nh, L.d);
    const float gcf = L.id * (L.cd[0] * glf[0] + L.cd[1] * glf[1] + L.cd[2] * glf[2]);
    float gdot = 0.0f;  // relu: the front copy sees dotn, the back copy -dotn
    if (dotn > 0.0f) gdot += gcf;
    if (back) {
        const float gcb = L.id * (L.cd[0] * glb[0] + L.cd[1] * glb[1] + L.cd[2] * glb[2]);
        if (-dotn > 0.0f) gdot -= gcb;
    }
    float gnh[3] = {gdot * L.d[0], gdot * L.d[1], gdot * L.d[2]};
    if (has_sh) {
        float gu[3];
        sh_bwd(L, nh, glf, gu);
#pragma unroll
        for (int c = 0; c < 3; c++) gnh[c] += gu[c];
        if (back) {
            const float nb[3] = {-nh[0], -nh[1], -nh[2]};
            sh_bwd(L, nb, glb, gu);
#pragma unroll
            for (int c = 0; c < 3; c++) gnh[c] -= gu[c];
        }
    }
    gn[0] = gn[1] = gn[2] = 0.0f;
    if (sqrtf(dot3(n, n)) > 0.0f) normalize3_bwd(n, gnh, gn);
}

// the corner gradients around vertex v, summed in double in table order: front copies, reversed copies
__device__ __forceinline__ void gather_corner_grads(const LArgs &a, const float *__restrict__ g, int b, int v, double sf[3],
                                                    double sb[3])
{
    const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
    const float *gb = g + (size_t)b * Fout * 9;
    sf[0] = sf[1] = sf[2] = sb[0] = sb[1] = sb[2] = 0.0;
    int e0, e1;
    const int32_t *ent = adjacency(a, b, v, e0, e1);
    for (int e = e0; e < e1; e++) {
        const int fk = clampi(ent[e], 0, 3 * a.Nf - 1), f = fk / 3, k = fk - 3 * f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            sf[c] += (double)gb[(size_t)f * 9 + 3 * k + c];
            if (a.fill_back) sb[c] += (double)gb[((size_t)a.Nf + f) * 9 + 3 * (2 - k) + c];
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------
// forward

__global__ __launch_bounds__(BLOCK) void k_face_light(LArgs a, float *__restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= a.Nf) return;
    Lamp L;
    load_lamp(a, b, L);
    int vi[3];
    float w[3][3], v10[3], v12[3], n[3], nh[3], dotn, lf[3], lb[3];
    load_face(a, b, f, vi, w);
    face_normal(w, v10, v12, n);
    both_lights(L, a.lights.sh != nullptr, n, nh, dotn, lf, lb);
    const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
    float *of = out + ((size_t)b * Fout + f) * 3, *ob = out + ((size_t)b * Fout + a.Nf + f) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        of[c] = lf[c];
        if (a.fill_back) ob[c] = lb[c];
    }
}

__global__ __launch_bounds__(BLOCK) void k_vertex_light(LArgs a, float *__restrict__ vlight)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    Lamp L;
    load_lamp(a, b, L);
    float m[3], nh[3], dotn, lf[3], lb[3];
    normal_sum(a, b, v, m);
    both_lights(L, a.lights.sh != nullptr, m, nh, dotn, lf, lb);
    float *o = vlight + ((size_t)b * a.Nv + v) * 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[c] = lf[c];
        o[3 + c] = lb[c];
    }
}

__global__ __launch_bounds__(BLOCK) void k_corner_light(LArgs a, const float *__restrict__ vlight, float *__restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= a.Nf) return;
    const int32_t *idx = a.idx + ((size_t)(a.idx_per_batch ? b : 0) * a.Nf + f) * 3;
    const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
    float *of = out + ((size_t)b * Fout + f) * 9, *ob = out + ((size_t)b * Fout + a.Nf + f) * 9;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *l = vlight + ((size_t)b * a.Nv + clampi(idx[k], 0, a.Nv - 1)) * 6;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            of[3 * k + c] = l[c];
            if (a.fill_back) ob[3 * (2 - k) + c] = l[3 + c];  // reversed corner order
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------
// backward to the vertices

// g [B, F, 3] (flat) or [B, F, 3, 3] (smooth); gout [B, Nv, 3]: grad_vertices (flat) / g_m (smooth)
template <bool SMOOTH>
__global__ __launch_bounds__(BLOCK) void k_vertex_grad(LArgs a, const float *__restrict__ g, float *__restrict__ gout)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    Lamp L;
    load_lamp(a, b, L);
    const bool has_sh = a.lights.sh != nullptr;
    float o3[3] = {0.0f, 0.0f, 0.0f};
    if (SMOOTH) {
        double sf[3], sb[3];
        gather_corner_grads(a, g, b, v, sf, sb);
        const float glf[3] = {(float)sf[0], (float)sf[1], (float)sf[2]}, glb[3] = {(float)sb[0], (float)sb[1], (float)sb[2]};
        float m[3];
        normal_sum(a, b, v, m);
        normal_bwd(L, has_sh, a.fill_back != 0, m, glf, glb, o3);
    } else {
        const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
        const float *gb = g + (size_t)b * Fout * 3;
        int e0, e1;
        const int32_t *ent = adjacency(a, b, v, e0, e1);
        for (int e = e0; e < e1; e++) {
            const int fk = clampi(ent[e], 0, 3 * a.Nf - 1), f = fk / 3, k = fk - 3 * f;
            int vi[3];
            float w[3][3], v10[3], v12[3], n[3], gn[3], o[3];
            load_face(a, b, f, vi, w);
            face_normal(w, v10, v12, n);
            normal_bwd(L, has_sh, a.fill_back != 0, n, gb + (size_t)f * 3, gb + ((size_t)a.Nf + f) * 3, gn);
            normal_to_corner(v10, v12, gn, k, o);
            o3[0] += o[0];
            o3[1] += o[1];
            o3[2] += o[2];
        }
    }
    float *out = gout + ((size_t)b * a.Nv + v) * 3;
    out[0] = o3[0];
    out[1] = o3[1];
    out[2] = o3[2];
}

// --------------------------------------------------------------------------------------------------------------------
// backward to the light

// what one copy (u = +-nh, dots = u . d, G the gradient of its colour) adds to the item's 36 sums
__device__ __forceinline__ void add_copy(const Lamp &L, bool has_sh, int need, const float *u, float dots, const double *G,
                                         double *s)
{
    if (need & NEED_ONE) {
#pragma unroll
        for (int c = 0; c < 3; c++) s[SUM_ONE + c] += G[c];
    }
    if (need & NEED_COS) {
        const double cosv = (double)fmaxf(dots, 0.0f);
#pragma unroll
        for (int c = 0; c < 3; c++) s[SUM_COS + c] += cosv * G[c];
    }
    if ((need & NEED_SH) && has_sh) {
        float Y[9];
        sh_basis(u, Y);
#pragma unroll
        for (int k = 0; k < 9; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) s[SUM_SH + 3 * k + c] += (double)Y[k] * G[c];
    }
    if ((need & NEED_DIR) && dots > 0.0f) {
        const double gcd = (G[0] * (double)L.cd[0] + G[1] * (double)L.cd[1]) + G[2] * (double)L.cd[2];
#pragma unroll
        for (int c = 0; c < 3; c++) s[SUM_DIR + c] += (double)u[c] * gcd;
    }
}

// partial [B, n_blocks, NSUM]: the sums of every block of 256 faces (flat) / vertices (smooth); the sums that `need` leaves
// out are stored as 0.  The block's sums are nr_reduce.h's block_sums written out in its two steps (wave_sum, waves_sum),
// because a group of sums that `need` leaves out -- all zeros -- skips its butterflies, which block_sums has no word for.
template <bool SMOOTH>
__global__ __launch_bounds__(BLOCK) void k_light_sums(LArgs a, const float *__restrict__ g, double *__restrict__ partial, int need)
{
    __shared__ double wave_sums[NSUM][BLOCK / WAVE];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const bool has_sh = a.lights.sh != nullptr;
    double s[NSUM];
#pragma unroll
    for (int j = 0; j < NSUM; j++) s[j] = 0.0;
    if (i < (SMOOTH ? a.Nv : a.Nf)) {
        Lamp L;
        load_lamp(a, b, L);
        float n[3];
        double Gf[3], Gb[3] = {0.0, 0.0, 0.0};
        if (SMOOTH) {
            gather_corner_grads(a, g, b, i, Gf, Gb);
            normal_sum(a, b, i, n);
        } else {
            int vi[3];
            float w[3][3], v10[3], v12[3];
            load_face(a, b, i, vi, w);
            face_normal(w, v10, v12, n);
            const int Fout = a.fill_back ? 2 * a.Nf : a.Nf;
            const float *gf = g + ((size_t)b * Fout + i) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Gf[c] = (double)gf[c];
                if (a.fill_back) Gb[c] = (double)gf[(size_t)a.Nf * 3 + c];
            }
        }
        float nh[3];
        normalize3(n, nh);
        const float dotn = dot3(nh, L.d);
        add_copy(L, has_sh, need, nh, dotn, Gf, s);
        if (a.fill_back) {
            const float nb[3] = {-nh[0], -nh[1], -nh[2]};
            add_copy(L, has_sh, need, nb, -dotn, Gb, s);
        }
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int j = 0; j < NSUM; j++) {
        const int group = j < SUM_COS ? NEED_ONE : (j < SUM_SH ? NEED_COS : (j < SUM_DIR ? NEED_SH : NEED_DIR));
        const double v = (need & group) ? wave_sum(s[j]) : s[j];  // (uniform)
        if (lane == 0) wave_sums[j][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSUM)
        partial[((size_t)b * gridDim.x + blockIdx.x) * NSUM + threadIdx.x] = waves_sum(wave_sums[threadIdx.x]);
}

// what image b adds to gradient element e (see NELEM)
__device__ __forceinline__ double element_of(const LArgs &a, const double *__restrict__ partial, int n_blocks, int b, int e)
{
    auto S = [&](int j) {  // sum j of image b: its blocks in block order
        return ordered_sum(partial + (size_t)b * n_blocks * NSUM + j, n_blocks, NSUM);
    };
    if (e < 2) {  // g_Ia = sum_c S[1, c] Ca_c, g_Id = sum_c S[cos, c] Cd_c
        const float *col = e == 0 ? param(a, a.lights.color_ambient, 2, b, 3) : param(a, a.lights.color_directional, 3, b, 3);
        const int j = e == 0 ? SUM_ONE : SUM_COS;
        return (S(j) * (double)col[0] + S(j + 1) * (double)col[1]) + S(j + 2) * (double)col[2];
    }
    if (e < 5) return (double)*param(a, a.lights.intensity_ambient, 0, b, 1) * S(SUM_ONE + e - 2);
    if (e < 8) return (double)*param(a, a.lights.intensity_directional, 1, b, 1) * S(SUM_COS + e - 5);
    if (e < 11) return (double)*param(a, a.lights.intensity_directional, 1, b, 1) * S(SUM_DIR + e - 8);
    return S(SUM_SH + e - 11);
}

// one thread per (image, gradient element); a shared parameter is summed over the images, in image order, by image 0's thread
__global__ __launch_bounds__(BLOCK) void k_light_finish(LArgs a, const double *__restrict__ partial, int n_blocks, nr_lights_grad out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.B * NELEM) return;
    const int b = t / NELEM, e = t - b * NELEM;
    float *dst;
    int bit, n, off;
    if (e == 0) { dst = out.intensity_ambient; bit = 0; n = 1; off = 0; }
    else if (e == 1) { dst = out.intensity_directional; bit = 1; n = 1; off = 0; }
    else if (e < 5) { dst = out.color_ambient; bit = 2; n = 3; off = e - 2; }
    else if (e < 8) { dst = out.color_directional; bit = 3; n = 3; off = e - 5; }
    else if (e < 11) { dst = out.direction; bit = 4; n = 3; off = e - 8; }
    else { dst = out.sh; bit = 5; n = 27; off = e - 11; }
    if (!dst) return;
    if ((a.lights.per_image >> bit) & 1) {
        dst[(size_t)b * n + off] = (float)element_of(a, partial, n_blocks, b, e);
        return;
    }
    if (b != 0) return;
    double s = 0.0;
    for (int i = 0; i < a.B; i++) s += element_of(a, partial, n_blocks, i, e);
    dst[off] = (float)s;
}

// --------------------------------------------------------------------------------------------------------------------
// host

inline int n_blocks_of(int n) { return (n + BLOCK - 1) / BLOCK; }

// the workspace: the blocks' sums, then (smooth) six floats per vertex -- the forward's two colours, the backward's g_m
size_t partial_bytes(int B, int Nv, int Nf, int smooth)
{
    return (size_t)B * n_blocks_of(smooth ? Nv : Nf) * NSUM * sizeof(double);
}
size_t workspace_bytes_of(int B, int Nv, int Nf, int smooth)
{
    return partial_bytes(B, Nv, Nf, smooth) + (smooth ? (size_t)B * Nv * 6 * sizeof(float) : 0);
}

// every argument check the two calls share, then the kernels' arguments
int light_args(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets, const int32_t *adj_entries,
               const nr_lights *lights, int B, int Nv, int Nf, int idx_per_batch, int fill_back, int smooth, bool need_adjacency,
               LArgs &a)
{
    a = {};
    // every NR_E_NULL, then every NR_E_MODE, in front of the mesh's NR_E_SIZE
    const int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, Nf, idx_per_batch, fill_back, need_adjacency, a);
    if (e == NR_E_NULL || !lights) return NR_E_NULL;
    if (!lights->intensity_ambient || !lights->intensity_directional || !lights->color_ambient || !lights->color_directional ||
        !lights->direction)
        return NR_E_NULL;
    if (smooth != 0 && smooth != 1) return NR_E_MODE;
    if (lights->per_image < 0 || lights->per_image > 63) return NR_E_MODE;
    if (e) return e;
    a.lights = *lights;
    return 0;
}

}  // namespace

NR_API size_t nr_light_colors_workspace_bytes(int32_t B, int32_t Nv, int32_t Nf, int32_t smooth)
{
    if (!mesh_sizes_ok(B, Nv, Nf) || (smooth != 0 && smooth != 1)) return 0;
    return workspace_bytes_of(B, Nv, Nf, smooth);
}

NR_API int nr_light_colors_forward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                   const int32_t *adj_entries, const nr_lights *lights, float *light_out, int32_t B, int32_t Nv,
                                   int32_t Nf, int32_t idx_per_batch, int32_t fill_back, int32_t smooth, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    LArgs a;
    if (!light_out) return NR_E_NULL;
    if (int e = light_args(vertices, faces_idx, adj_offsets, adj_entries, lights, B, Nv, Nf, idx_per_batch, fill_back, smooth,
                           smooth == 1, a))
        return e;
    hipStream_t st = (hipStream_t)stream;
    if (!smooth) {
        hipLaunchKernelGGL(k_face_light, grid_of(Nf, B), dim3(BLOCK), 0, st, a, light_out);
        return launch_status();
    }
    if (!workspace || workspace_bytes < workspace_bytes_of(B, Nv, Nf, 1)) return NR_E_WORKSPACE;
    float *vlight = (float *)((char *)workspace + partial_bytes(B, Nv, Nf, 1));
    hipLaunchKernelGGL(k_vertex_light, grid_of(Nv, B), dim3(BLOCK), 0, st, a, vlight);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_corner_light, grid_of(Nf, B), dim3(BLOCK), 0, st, a, vlight, light_out);
    return launch_status();
}

NR_API int nr_light_colors_backward(const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                                    const int32_t *adj_entries, const nr_lights *lights, const float *grad_light,
                                    float *grad_vertices, const nr_lights_grad *grads, int32_t B, int32_t Nv, int32_t Nf,
                                    int32_t idx_per_batch, int32_t fill_back, int32_t smooth, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    LArgs a;
    if (!grad_light) return NR_E_NULL;
    if (int e = light_args(vertices, faces_idx, adj_offsets, adj_entries, lights, B, Nv, Nf, idx_per_batch, fill_back, smooth,
                           true, a))
        return e;
    nr_lights_grad out = {};
    if (grads) out = *grads;
    if (!a.lights.sh) out.sh = nullptr;  // (no SH term: nothing to differentiate)
    int need = 0;
    if (out.intensity_ambient || out.color_ambient) need |= NEED_ONE;
    if (out.intensity_directional || out.color_directional) need |= NEED_COS;
    if (out.sh) need |= NEED_SH;
    if (out.direction) need |= NEED_DIR;
    if (!need && !grad_vertices) return NR_E_MODE;
    if ((need || (smooth && grad_vertices)) && (!workspace || workspace_bytes < workspace_bytes_of(B, Nv, Nf, smooth)))
        return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (need) {
        double *partial = (double *)workspace;
        const int n_items = smooth ? Nv : Nf, nb = n_blocks_of(n_items);
        if (smooth) hipLaunchKernelGGL(k_light_sums<true>, grid_of(n_items, B), dim3(BLOCK), 0, st, a, grad_light, partial, need);
        else hipLaunchKernelGGL(k_light_sums<false>, grid_of(n_items, B), dim3(BLOCK), 0, st, a, grad_light, partial, need);
        if (int rc = launch_status()) return rc;
        hipLaunchKernelGGL(k_light_finish, dim3((unsigned)n_blocks_of(B * NELEM)), dim3(BLOCK), 0, st, a, partial, nb, out);
        if (int rc = launch_status()) return rc;
    }
    if (!grad_vertices) return 0;
    if (!smooth) {
        hipLaunchKernelGGL(k_vertex_grad<false>, grid_of(Nv, B), dim3(BLOCK), 0, st, a, grad_light, grad_vertices);
        return launch_status();
    }
    float *gm = (float *)((char *)workspace + partial_bytes(B, Nv, Nf, 1));
    hipLaunchKernelGGL(k_vertex_grad<true>, grid_of(Nv, B), dim3(BLOCK), 0, st, a, grad_light, gm);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_normals_gather<true>, grid_of(Nv, B), dim3(BLOCK), 0, st, (const MeshArgs &)a, gm, grad_vertices);
    return launch_status();
}
