// nr_winding.hip -- the generalized winding number of a mesh at a cloud of points (include/nr_hip.h; DESIGN "Winding numbers"):
// w(p) = (1 / 4 pi) sum_f Omega_f(p), the signed solid angles of nr_solid_angle.h, by a dense points x faces sweep, and its
// exact gradients to the points and the vertices.  One topology per call; world-space vertices [B, Nv, 3].
//
//   k_sweep<1>     (image, Q points per thread in registers): the faces stream through LDS in tiles of T records (three 16-byte
//                  words, read as broadcast ds_read_b128s; a collapsed face carries its skip flag in the padding), built by the
//                  tile loader from `vertices` and `faces`
//   k_sweep<3>     the same sweep with dOmega/dp in three accumulators per point, times g / (4 pi)
//   k_faces        (image, one face record and nine accumulators per thread): the points and their upstream g stream through
//                  LDS as float4 (x, y, z, g) tiles; per corner sum_i g_i dOmega_i/dv_k, times 1 / (4 pi), to the workspace
//   k_gather       (image, vertex): the corner gradients of the vertex's table entries (f, k), ascending, summed in float32
//   k_merge<C>     small calls: the streamed side is cut at tile boundaries over S workgroups, each storing its tiles' sums
// The sums are a two-level definition: the streamed side in fixed tiles of T; a tile's terms added in double, ascending, from 0;
// the tile sums added in double, ascending, from 0; the total scaled in double and rounded once.  A split call stores the tile
// sums and k_merge adds them in that order, so the result does not depend on the split, to the bit.
// No atomics and no scratch: every output stored once, the same bits in every run and for an image alone or inside a batch.
#include "nr_pair_sweep.h"
#include "nr_solid_angle.h"

using namespace nr;

namespace {

// measurement builds set other values: python -m neural_renderer_amd._build <tag> NR_WN_Q=4 builds a variant library, and
// NR_HIP_LIB points scripts/winding_timing.py at it
#ifndef NR_WN_Q
#define NR_WN_Q 2
#endif
#ifndef NR_WN_T
#define NR_WN_T 256
#endif
#ifndef NR_WN_SPLIT_BELOW
#define NR_WN_SPLIT_BELOW 1024
#endif

constexpr int BLOCK = 256;
constexpr int Q = NR_WN_Q;                      // points per thread, k_sweep
constexpr int T = NR_WN_T;                      // records (points) per LDS tile: the first level of the sums
constexpr int SPLIT_BELOW = NR_WN_SPLIT_BELOW;  // fewer workgroups than this: split the streamed side
constexpr size_t PART_CAP = (size_t)256 << 20;  // tile sums above this many bytes: the call is not split
constexpr double INV_4PI = 0.079577471545947667884;

struct SweepArgs {
    MeshArgs mesh;
    const float *points;  // [B or 1, N, 3]
    const float *grad;    // [B, N] upstream (not k_sweep<1>)
    int N, points_per_batch;
    int S, chunk, tiles;  // the streamed side in S parts of `chunk` items (a multiple of T); `tiles` tiles in all
    double *part;         // [B, tiles, C, rows] when S > 1
    float *out;           // winding [B, N] | grad_points [B, N, 3] | corner gradients [B, F, 3, 3]
};

__device__ __forceinline__ const float *points_of(const SweepArgs &a, int b)
{
    return a.points + (a.points_per_batch ? (size_t)b * a.N * 3 : 0);
}

template <int C>
__device__ __forceinline__ size_t part_at(const SweepArgs &a, int b, int t, int c, int rows, int row)
{
    return (((size_t)b * a.tiles + t) * C + c) * rows + row;
}

// C = 1: the winding number; C = 3: its gradient to the points
template <int C>
__global__ __launch_bounds__(BLOCK) void k_sweep(SweepArgs a)
{
    __shared__ float4 tile[T][SA_RECORD_WORDS];
    const int b = blockIdx.y, s = blockIdx.x % a.S, blk = blockIdx.x / a.S, tid = threadIdx.x;
    const int F = a.mesh.Nf, N = a.N;
    const float *pb = points_of(a, b);
    float px[Q], py[Q], pz[Q];
    double total[Q][C];
    int pi[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        pi[q] = (blk * Q + q) * BLOCK + tid;
        const float *p = pb + (size_t)min(pi[q], N - 1) * 3;
        px[q] = sa_point_x(p[0], p[1], p[2]); py[q] = p[1]; pz[q] = p[2];
#pragma unroll
        for (int c = 0; c < C; c++) total[q][c] = 0.0;
    }
    const int f_begin = s * a.chunk, f_end = min(F, f_begin + a.chunk);
    for (int f0 = f_begin; f0 < f_end; f0 += T) {
        __syncthreads();
        for (int t = tid; t < T; t += BLOCK) {
            if (f0 + t < f_end) {
                int vi[3];
                float w[3][3];
                load_face(a.mesh, b, f0 + t, vi, w);
                const SaRecord R = sa_record(w);
                tile[t][0] = R.v0_skip; tile[t][1] = R.v1; tile[t][2] = R.v2;
            }
        }
        __syncthreads();
        const int nf = min(T, f_end - f0);
        double acc[Q][C];
#pragma unroll
        for (int q = 0; q < Q; q++)
#pragma unroll
            for (int c = 0; c < C; c++) acc[q][c] = 0.0;
        for (int j = 0; j < nf; j++) {
            SaRecord R;
            R.v0_skip = tile[j][0]; R.v1 = tile[j][1]; R.v2 = tile[j][2];
            asm volatile("" ::"v"(R.v1.w), "v"(R.v2.w));  // the padding counts as used: ds_read_b128s, not ds_read_b96s
            if (R.v0_skip.w != 0.0f) continue;             // a collapsed face (the same for every lane)
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const SaPair P = sa_pair(R, px[q], py[q], pz[q]);
                if (C == 1) {
                    acc[q][0] += (double)sa_omega(P);
                } else {
                    float g0[3], g1[3], g2[3];
                    sa_gradient(P, g0, g1, g2);
#pragma unroll
                    for (int c = 0; c < C; c++) acc[q][c] += (double)(-((g0[c] + g1[c]) + g2[c]));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < Q; q++)
#pragma unroll
            for (int c = 0; c < C; c++) {
                if (a.S == 1) total[q][c] += acc[q][c];
                else if (pi[q] < N) a.part[part_at<C>(a, b, f0 / T, c, N, pi[q])] = acc[q][c];
            }
    }
    if (a.S != 1) return;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        if (pi[q] >= N) continue;
        const size_t o = (size_t)b * N + pi[q];
        const double scale = C == 1 ? INV_4PI : (double)a.grad[o] * INV_4PI;
#pragma unroll
        for (int c = 0; c < C; c++) a.out[o * C + c] = (float)(total[q][c] * scale);
    }
}

// one face per thread, the points streamed: sum_i g_i dOmega_i/dv_k per corner k
__global__ __launch_bounds__(BLOCK) void k_faces(SweepArgs a)
{
    __shared__ float4 tile[T];
    const int b = blockIdx.y, s = blockIdx.x % a.S, blk = blockIdx.x / a.S, tid = threadIdx.x;
    const int F = a.mesh.Nf, N = a.N;
    const int f = blk * BLOCK + tid;
    const float *pb = points_of(a, b);
    const float *gb = a.grad + (size_t)b * N;
    int vi[3];
    float w[3][3];
    load_face(a.mesh, b, min(f, F - 1), vi, w);
    const SaRecord R = sa_record(w);
    const bool skip = R.v0_skip.w != 0.0f;
    double total[9];
#pragma unroll
    for (int k = 0; k < 9; k++) total[k] = 0.0;
    const int i_begin = s * a.chunk, i_end = min(N, i_begin + a.chunk);
    for (int i0 = i_begin; i0 < i_end; i0 += T) {
        __syncthreads();
        for (int t = tid; t < T; t += BLOCK) {
            if (i0 + t < i_end) {
                const float *p = pb + (size_t)(i0 + t) * 3;
                tile[t] = make_float4(sa_point_x(p[0], p[1], p[2]), p[1], p[2], gb[i0 + t]);
            }
        }
        __syncthreads();
        const int np = skip ? 0 : min(T, i_end - i0);
        double acc[9];
#pragma unroll
        for (int k = 0; k < 9; k++) acc[k] = 0.0;
        for (int j = 0; j < np; j++) {
            const float4 p = tile[j];
            const SaPair P = sa_pair(R, p.x, p.y, p.z);
            float g0[3], g1[3], g2[3];
            sa_gradient(P, g0, g1, g2);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                acc[c] += (double)(p.w * g0[c]);
                acc[3 + c] += (double)(p.w * g1[c]);
                acc[6 + c] += (double)(p.w * g2[c]);
            }
        }
#pragma unroll
        for (int k = 0; k < 9; k++) {
            if (a.S == 1) total[k] += acc[k];
            else if (f < F) a.part[part_at<9>(a, b, i0 / T, k, F, f)] = acc[k];
        }
    }
    if (a.S != 1 || f >= F) return;
    float *out = a.out + ((size_t)b * F + f) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = (float)(total[k] * INV_4PI);
}

// the tile sums of every row in ascending order; C = 9: the rows are faces
template <int C>
__global__ __launch_bounds__(BLOCK) void k_merge(SweepArgs a)
{
    const int rows = C == 9 ? a.mesh.Nf : a.N;
    const int row = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (row >= rows) return;
    const size_t o = (size_t)b * rows + row;
    const double scale = C == 3 ? (double)a.grad[o] * INV_4PI : INV_4PI;
#pragma unroll
    for (int c = 0; c < C; c++) {
        double total = 0.0;
        for (int t = 0; t < a.tiles; t++) total += a.part[part_at<C>(a, b, t, c, rows, row)];
        a.out[o * C + c] = (float)(total * scale);
    }
}

// grad_vertices[b, v] = the corner gradients [B, F, 3, 3] of the vertex's table entries, ascending, in float32
__global__ __launch_bounds__(BLOCK) void k_gather(MeshArgs a, const float *__restrict__ corners, float *__restrict__ grad_vertices)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= a.Nv) return;
    float g[3] = {0.0f, 0.0f, 0.0f};
    int e0, e1;
    const int32_t *ent = adjacency(a, b, v, e0, e1);
    const float *cb = corners + (size_t)b * a.Nf * 9;
    for (int e = e0; e < e1; e++) {
        const float *src = cb + (size_t)clampi(ent[e], 0, 3 * a.Nf - 1) * 3;
        g[0] += src[0];
        g[1] += src[1];
        g[2] += src[2];
    }
    float *out = grad_vertices + ((size_t)b * a.Nv + v) * 3;
    out[0] = g[0];
    out[1] = g[1];
    out[2] = g[2];
}

// --------------------------------------------------------------------------------------------------------------------
// host

enum { FORWARD = 0, BACKWARD_POINTS = 1, BACKWARD_VERTICES = 2 };

size_t corner_bytes(int B, int F) { return ((size_t)B * F * 9 * sizeof(float) + 15) / 16 * 16; }

// The split of call `which` -> the sweep's workgroups along x, 0: the split asks for more than a grid holds (judged on the
// split that was asked for, before the cap).  A split call stores 1, 3 or 9 doubles per row and tile, `bytes` in all; above
// PART_CAP bytes it is not split.
unsigned plan(int which, int B, int N, int F, int split, SplitPlan &p, size_t &bytes)
{
    const bool faces = which == BACKWARD_VERTICES;
    const int rows = faces ? F : N, per_block = faces ? BLOCK : BLOCK * Q, values = faces ? 9 : (which == FORWARD ? 1 : 3);
    p = plan_split(B, rows, per_block, faces ? N : F, T, SPLIT_BELOW, split);
    const unsigned groups_x = grid_x(rows, per_block, p.S);
    bytes = (size_t)B * p.tiles * rows * values * sizeof(double);
    if (!groups_x || (p.S > 1 && bytes <= PART_CAP)) return groups_x;
    p.S = 1;
    p.chunk = p.tiles * T;
    bytes = 0;
    return grid_x(rows, per_block, 1);
}

int run(int which, const float *points, const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
        const int32_t *adj_entries, const float *grad, float *out, int B, int N, int Nv, int F, int points_per_batch, int split,
        void *workspace, size_t workspace_bytes, void *stream)
{
    if (!points || !out || (which != FORWARD && !grad)) return NR_E_NULL;
    SweepArgs a;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, F, 0, 0, which == BACKWARD_VERTICES, a.mesh)) return e;
    if (!sweep_sizes_ok(B, N, Nv, F) || split < 0) return NR_E_SIZE;
    if (points_per_batch != 0 && points_per_batch != 1) return NR_E_MODE;
    SplitPlan p;
    size_t parts;
    const unsigned groups_x = plan(which, B, N, F, split, p, parts);
    if (!groups_x) return NR_E_SIZE;
    a.S = p.S; a.chunk = p.chunk; a.tiles = p.tiles;
    const size_t corners = which == BACKWARD_VERTICES ? corner_bytes(B, F) : 0;
    if (parts + corners && (!workspace || workspace_bytes < parts + corners)) return NR_E_WORKSPACE;
    a.points = points; a.grad = grad; a.N = N; a.points_per_batch = points_per_batch;
    a.part = parts ? (double *)((char *)workspace + corners) : nullptr;
    a.out = which == BACKWARD_VERTICES ? (float *)workspace : out;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(groups_x, (unsigned)B), per_row = grid_of(which == BACKWARD_VERTICES ? F : N, B);
    void (*const sweep[])(SweepArgs) = {k_sweep<1>, k_sweep<3>, k_faces};  // by `which`
    void (*const merge[])(SweepArgs) = {k_merge<1>, k_merge<3>, k_merge<9>};
    if (int rc = launch_sweep(a.S, [&] { hipLaunchKernelGGL(sweep[which], grid, dim3(BLOCK), 0, st, a); },
                              [&] { hipLaunchKernelGGL(merge[which], per_row, dim3(BLOCK), 0, st, a); }))
        return rc;
    if (which == BACKWARD_VERTICES) {
        hipLaunchKernelGGL(k_gather, grid_of(Nv, B), dim3(BLOCK), 0, st, a.mesh, (const float *)a.out, out);
        return launch_status();
    }
    return 0;
}

}  // namespace

NR_API size_t nr_winding_workspace_bytes(int32_t B, int32_t N, int32_t F, int32_t which, int32_t split)
{
    if (!sweep_sizes_ok(B, N, 1, F) || split < 0 || which < FORWARD || which > BACKWARD_VERTICES) return 0;
    SplitPlan p;
    size_t parts;
    if (!plan(which, B, N, F, split, p, parts)) return 0;  // (the call itself returns NR_E_SIZE)
    return parts + (which == BACKWARD_VERTICES ? corner_bytes(B, F) : 0);
}

NR_API int nr_winding_forward(const float *points, const float *vertices, const int32_t *faces, float *winding, int32_t B, int32_t N,
                              int32_t Nv, int32_t F, int32_t points_per_batch, int32_t split, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    return run(FORWARD, points, vertices, faces, nullptr, nullptr, nullptr, winding, B, N, Nv, F, points_per_batch, split, workspace,
               workspace_bytes, stream);
}

NR_API int nr_winding_backward_points(const float *points, const float *vertices, const int32_t *faces, const float *grad_winding,
                                      float *grad_points, int32_t B, int32_t N, int32_t Nv, int32_t F, int32_t split,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    return run(BACKWARD_POINTS, points, vertices, faces, nullptr, nullptr, grad_winding, grad_points, B, N, Nv, F, 1, split,
               workspace, workspace_bytes, stream);
}

NR_API int nr_winding_backward_vertices(const float *points, const float *vertices, const int32_t *faces,
                                        const int32_t *adj_offsets, const int32_t *adj_entries, const float *grad_winding,
                                        float *grad_vertices, int32_t B, int32_t N, int32_t Nv, int32_t F,
                                        int32_t points_per_batch, int32_t split, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    return run(BACKWARD_VERTICES, points, vertices, faces, adj_offsets, adj_entries, grad_winding, grad_vertices, B, N, Nv, F,
               points_per_batch, split, workspace, workspace_bytes, stream);
}
