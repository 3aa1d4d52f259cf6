// nr_point_mesh.hip -- the point-to-mesh distance (include/nr_hip.h; DESIGN "Point-to-mesh distance"): for every point of a
// cloud the nearest triangle of a mesh, for every triangle the nearest point, both by a brute-force sweep, and the gradients
// of the squared distances to the points and the vertices.  One topology per call; world-space vertices [B, Nv, 3].
//
//   k_points_to_faces  (image, Q points per thread in registers): the faces stream through LDS in tiles of T records
//                      (nr_point_triangle.h: five 16-byte words, read as broadcast ds_read_b128s), built by the tile loader
//                      from `vertices` and `faces`; the running minimum takes a strict < in ascending face order
//   k_faces_to_points  (image, one face record per thread in registers): the points stream through LDS as float4 tiles
//   k_merge            small calls: the streamed side is split over S workgroups, each writing its minimum and id; the
//                      parts are merged in ascending order with the same strict <, so the result does not depend on S
//   finish             the winning pair is evaluated once more WITH its weights (the same function, the same bits) and
//                      dist2, the id and the barycentric weights are stored -- every output element exactly once
//   k_loss             (image): the sums of both directions in double -- per thread elements t, t + 256, .. in index order from
//                      0.0, then the workgroup in the fixed order of nr_reduce.h (block_sum) -- weighted, added, rounded once
//   k_backward_points  (image, point): its own pair's 2 g r, then the faces that chose the point through a list sorted by
//                      point id, in list order
//   k_backward_vertices (image, vertex): the table entries (f, k) of the vertex ascending; per entry face f's own pair,
//                      then the points assigned to f through a list sorted by face id; each term -(2 g w_k) r
// No atomics and no scratch: the same bits in every run, for an image alone or inside a batch.
//
// A NaN distance never wins a strict <; the minimum starts at +inf with id 0, so ids are always in range and a row whose
// pairs are all NaN (or +inf) reports id 0 and that pair's own, non-finite, dist2.
#include "nr_pair_sweep.h"
#include "nr_point_triangle.h"

using namespace nr;

namespace {

// measurement builds set other values (scripts/point_mesh_timing.py --variants); LAB-NOTEBOOK has the table
#ifndef NR_PM_Q
#define NR_PM_Q 2
#endif
#ifndef NR_PM_T
#define NR_PM_T 256
#endif
#ifndef NR_PM_SPLIT_BELOW
#define NR_PM_SPLIT_BELOW 1024
#endif

constexpr int BLOCK = 256;
constexpr int Q = NR_PM_Q;                      // points per thread, points -> faces
constexpr int T = NR_PM_T;                      // records (points) per LDS tile
constexpr int SPLIT_BELOW = NR_PM_SPLIT_BELOW;  // fewer workgroups than this: split the streamed side

struct SweepArgs {
    MeshArgs mesh;
    const float *points;  // [B or 1, N, 3]
    int N, points_per_batch;
    int S, chunk;         // the streamed side in S parts of `chunk` items (a multiple of T)
    float *part_d;        // [B, S, rows] when S > 1
    int32_t *part_id;
    float *dist2;         // [B, rows]
    int32_t *ids;         // [B, rows]
    float *bary;          // [B, rows, 3]
};

__device__ __forceinline__ const float *points_of(const SweepArgs &a, int b)
{
    return a.points + (a.points_per_batch ? (size_t)b * a.N * 3 : 0);
}

// the pair (point i, face f) once more with its weights: row `row` of the outputs
__device__ __forceinline__ void finish(const SweepArgs &a, int b, int rows, int row, int i, int f, int id)
{
    int vi[3];
    float w[3][3], bw[3];
    load_face(a.mesh, b, f, vi, w);
    const TriRecord R = tri_record(w);
    const float *p = points_of(a, b) + (size_t)i * 3;
    const float d = point_triangle<true>(R, p[0], p[1], p[2], bw);
    const size_t o = (size_t)b * rows + row;
    a.dist2[o] = d;
    a.ids[o] = id;
    a.bary[o * 3] = bw[0];
    a.bary[o * 3 + 1] = bw[1];
    a.bary[o * 3 + 2] = bw[2];
}

__device__ __forceinline__ void store_part(const SweepArgs &a, int b, int s, int rows, int row, float d, int id)
{
    const size_t o = ((size_t)b * a.S + s) * rows + row;
    a.part_d[o] = d;
    a.part_id[o] = id;
}

__global__ __launch_bounds__(BLOCK) void k_points_to_faces(SweepArgs a)
{
    __shared__ float4 tile[T][TRI_RECORD_WORDS];
    const int b = blockIdx.y, s = blockIdx.x % a.S, blk = blockIdx.x / a.S, tid = threadIdx.x;
    const int F = a.mesh.Nf, N = a.N;
    const float *pb = points_of(a, b);
    float px[Q], py[Q], pz[Q], best[Q];
    int id[Q], pi[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        pi[q] = (blk * Q + q) * BLOCK + tid;
        const float *p = pb + (size_t)min(pi[q], N - 1) * 3;
        px[q] = p[0]; py[q] = p[1]; pz[q] = p[2];
        best[q] = __builtin_inff();
        id[q] = 0;
    }
    const int f_begin = s * a.chunk, f_end = min(F, f_begin + a.chunk);
    for (int f0 = f_begin; f0 < f_end; f0 += T) {
        __syncthreads();
        for (int t = tid; t < T; t += BLOCK) {
            if (f0 + t < f_end) {
                int vi[3];
                float w[3][3];
                load_face(a.mesh, b, f0 + t, vi, w);
                const TriRecord R = tri_record(w);
                tile[t][0] = R.a_iaa; tile[t][1] = R.ab_icc; tile[t][2] = R.ac_iee; tile[t][3] = R.g_igg; tile[t][4] = R.e_bb;
            }
        }
        __syncthreads();
        const int nf = min(T, f_end - f0);
        for (int j = 0; j < nf; j++) {
            TriRecord R;
            R.a_iaa = tile[j][0]; R.ab_icc = tile[j][1]; R.ac_iee = tile[j][2]; R.g_igg = tile[j][3]; R.e_bb = tile[j][4];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const float d = point_triangle<false>(R, px[q], py[q], pz[q], nullptr);
                if (d < best[q]) { best[q] = d; id[q] = f0 + j; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
        if (pi[q] >= N) continue;
        if (a.S == 1) finish(a, b, N, pi[q], pi[q], id[q], id[q]);
        else store_part(a, b, s, N, pi[q], best[q], id[q]);
    }
}

__global__ __launch_bounds__(BLOCK) void k_faces_to_points(SweepArgs a)
{
    __shared__ float4 tile[T];
    const int b = blockIdx.y, s = blockIdx.x % a.S, blk = blockIdx.x / a.S, tid = threadIdx.x;
    const int F = a.mesh.Nf, N = a.N;
    const int f = blk * BLOCK + tid;
    const float *pb = points_of(a, b);
    int vi[3];
    float w[3][3];
    load_face(a.mesh, b, min(f, F - 1), vi, w);
    const TriRecord R = tri_record(w);
    float best = __builtin_inff();
    int id = 0;
    const int i_begin = s * a.chunk, i_end = min(N, i_begin + a.chunk);
    for (int i0 = i_begin; i0 < i_end; i0 += T) {
        __syncthreads();
        for (int t = tid; t < T; t += BLOCK) {
            if (i0 + t < i_end) {
                const float *p = pb + (size_t)(i0 + t) * 3;
                tile[t] = make_float4(p[0], p[1], p[2], 0.0f);
            }
        }
        __syncthreads();
        const int np = min(T, i_end - i0);
        for (int j = 0; j < np; j++) {
            const float4 p = tile[j];
            asm volatile("" ::"v"(p.w));  // the fourth float counts as used: one ds_read_b128, not a ds_read_b96 at twice the cycles
            const float d = point_triangle<false>(R, p.x, p.y, p.z, nullptr);
            if (d < best) { best = d; id = i0 + j; }
        }
    }
    if (f >= F) return;
    if (a.S == 1) finish(a, b, F, f, id, f, id);
    else store_part(a, b, s, F, f, best, id);
}

// the S parts of every row in ascending order, then finish; FACES: the rows are faces (ids are points)
template <bool FACES>
__global__ __launch_bounds__(BLOCK) void k_merge(SweepArgs a)
{
    const int rows = FACES ? a.mesh.Nf : a.N;
    const int row = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (row >= rows) return;
    const int id = merge_argmin(a.part_d, a.part_id, b, a.S, rows, row, 0, (FACES ? a.N : a.mesh.Nf) - 1);
    if (FACES) finish(a, b, rows, row, id, row, id);
    else finish(a, b, rows, row, row, id, id);
}

// --------------------------------------------------------------------------------------------------------------------
// loss

// the sum of d[0 .. n), valid in thread 0; every thread of the block must call it
__device__ __forceinline__ double strided_sum(const float *__restrict__ d, int n)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) s += (double)d[i];
    const double t = block_sum<BLOCK>(s);
    __syncthreads();  // k_loss calls twice: block_sum's LDS has been read
    return t;
}

__global__ __launch_bounds__(BLOCK) void k_loss(const float *__restrict__ dist2_points, const float *__restrict__ dist2_faces,
                                                float *__restrict__ loss, int N, int F, double wp, double wf)
{
    const int b = blockIdx.x;
    double total = 0.0;
    if (dist2_points) total = wp * strided_sum(dist2_points + (size_t)b * N, N);
    if (dist2_faces) {
        const double t = wf * strided_sum(dist2_faces + (size_t)b * F, F);
        total = dist2_points ? total + t : t;
    }
    if (threadIdx.x == 0) loss[b] = (float)total;
}

// --------------------------------------------------------------------------------------------------------------------
// backward

struct BackwardArgs {
    MeshArgs mesh;
    const float *points;
    int N, points_per_batch;
    // points -> mesh pairs (NULL face_ids: none): per point its face, weights and upstream; the points sorted by face
    const int32_t *face_ids;   // [B, N]
    const float *bary_p;       // [B, N, 3]
    const float *grad_p;       // [B, N]
    const int32_t *order_p;    // [B, N]: point numbers, by face id (stable)
    const int32_t *offsets_f;  // [B, F + 1]
    // mesh -> points pairs (NULL point_ids: none)
    const int32_t *point_ids;  // [B, F]
    const float *bary_f;       // [B, F, 3]
    const float *grad_f;       // [B, F]
    const int32_t *order_f;    // [B, F]: face numbers, by point id (stable)
    const int32_t *offsets_p;  // [B, N + 1]
};

// acc += sign * coef * r of the pair (point i, face with vertices w, weights bw)
__device__ __forceinline__ void add_pair(const BackwardArgs &a, int b, int i, const float w[3][3], const float *bw, float coef,
                                         bool subtract, float acc[3])
{
    const float *p = a.points + ((a.points_per_batch ? (size_t)b * a.N : 0) + (size_t)i) * 3;
    float r[3];
    point_triangle_residual(w, p, bw[1], bw[2], r);
#pragma unroll
    for (int c = 0; c < 3; c++) acc[c] = subtract ? acc[c] - coef * r[c] : acc[c] + coef * r[c];
}

__global__ __launch_bounds__(BLOCK) void k_backward_points(BackwardArgs a, float *__restrict__ grad_points)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const int N = a.N, F = a.mesh.Nf;
    if (i >= N) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int vi[3];
    float w[3][3];
    if (a.face_ids) {
        const size_t o = (size_t)b * N + i;
        load_face(a.mesh, b, clampi(a.face_ids[o], 0, F - 1), vi, w);
        add_pair(a, b, i, w, a.bary_p + o * 3, 2.0f * a.grad_p[o], false, acc);
    }
    if (a.point_ids) {
        const int32_t *off = a.offsets_p + (size_t)b * (N + 1);
        const int e0 = clampi(off[i], 0, F), e1 = clampi(off[i + 1], e0, F);
        for (int e = e0; e < e1; e++) {
            const int f = clampi(a.order_f[(size_t)b * F + e], 0, F - 1);
            const size_t o = (size_t)b * F + f;
            load_face(a.mesh, b, f, vi, w);
            add_pair(a, b, i, w, a.bary_f + o * 3, 2.0f * a.grad_f[o], false, acc);
        }
    }
    float *out = grad_points + ((size_t)b * N + i) * 3;
    out[0] = acc[0];
    out[1] = acc[1];
    out[2] = acc[2];
}

__global__ __launch_bounds__(BLOCK) void k_backward_vertices(BackwardArgs a, float *__restrict__ grad_vertices)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const int N = a.N, F = a.mesh.Nf;
    if (v >= a.mesh.Nv) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int e0, e1;
    const int32_t *ent = adjacency(a.mesh, b, v, e0, e1);
    for (int e = e0; e < e1; e++) {
        const int fk = clampi(ent[e], 0, 3 * F - 1), f = fk / 3, k = fk - 3 * f;
        int vi[3];
        float w[3][3];
        load_face(a.mesh, b, f, vi, w);
        if (a.point_ids) {
            const size_t o = (size_t)b * F + f;
            const float *bw = a.bary_f + o * 3;
            add_pair(a, b, clampi(a.point_ids[o], 0, N - 1), w, bw, (2.0f * a.grad_f[o]) * bw[k], true, acc);
        }
        if (a.face_ids) {
            const int32_t *off = a.offsets_f + (size_t)b * (F + 1);
            const int j0 = clampi(off[f], 0, N), j1 = clampi(off[f + 1], j0, N);
            for (int j = j0; j < j1; j++) {
                const int i = clampi(a.order_p[(size_t)b * N + j], 0, N - 1);
                const size_t o = (size_t)b * N + i;
                const float *bw = a.bary_p + o * 3;
                add_pair(a, b, i, w, bw, (2.0f * a.grad_p[o]) * bw[k], true, acc);
            }
        }
    }
    float *out = grad_vertices + ((size_t)b * a.mesh.Nv + v) * 3;
    out[0] = acc[0];
    out[1] = acc[1];
    out[2] = acc[2];
}

// --------------------------------------------------------------------------------------------------------------------
// host

// the split of a direction (faces: the rows are faces) -> the sweep's workgroups along x, 0: more than a grid holds
unsigned plan(bool faces, int B, int N, int F, int split, SplitPlan &p)
{
    const int rows = faces ? F : N, per_block = faces ? BLOCK : BLOCK * Q;
    p = plan_split(B, rows, per_block, faces ? N : F, T, SPLIT_BELOW, split);
    return grid_x(rows, per_block, p.S);
}

size_t part_bytes(int B, int S, int rows) { return S > 1 ? (size_t)B * S * rows * (sizeof(float) + sizeof(int32_t)) : 0; }

int sweep(bool faces, const float *points, const float *vertices, const int32_t *faces_idx, float *dist2, int32_t *ids, float *bary,
          int B, int N, int Nv, int F, int points_per_batch, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!points || !dist2 || !ids || !bary) return NR_E_NULL;
    SweepArgs a;
    if (int e = mesh_args(vertices, faces_idx, nullptr, nullptr, B, Nv, F, 0, 0, false, a.mesh)) return e;
    if (!sweep_sizes_ok(B, N, Nv, F) || split < 0) return NR_E_SIZE;
    SplitPlan p;
    const unsigned groups_x = plan(faces, B, N, F, split, p);
    if (!groups_x) return NR_E_SIZE;
    a.S = p.S; a.chunk = p.chunk;
    const int rows = faces ? F : N;
    const size_t need = part_bytes(B, a.S, rows);
    if (need && (!workspace || workspace_bytes < need)) return NR_E_WORKSPACE;
    a.points = points; a.N = N; a.points_per_batch = points_per_batch != 0;
    a.part_d = need ? (float *)workspace : nullptr;
    a.part_id = need ? (int32_t *)((float *)workspace + (size_t)B * a.S * rows) : nullptr;
    a.dist2 = dist2; a.ids = ids; a.bary = bary;
    hipStream_t st = (hipStream_t)stream;
    void (*const sweep)(SweepArgs) = faces ? k_faces_to_points : k_points_to_faces;
    void (*const merge)(SweepArgs) = faces ? k_merge<true> : k_merge<false>;
    return launch_sweep(a.S, [&] { hipLaunchKernelGGL(sweep, dim3(groups_x, (unsigned)B), dim3(BLOCK), 0, st, a); },
                        [&] { hipLaunchKernelGGL(merge, grid_of(rows, B), dim3(BLOCK), 0, st, a); });
}

int backward_args(const float *points, const float *vertices, const int32_t *faces_idx, const int32_t *adj_offsets,
                  const int32_t *adj_entries, bool need_adjacency, const int32_t *face_ids, const float *bary_p,
                  const float *grad_p, const int32_t *order_p, const int32_t *offsets_f, bool need_order_p,
                  const int32_t *point_ids, const float *bary_f, const float *grad_f, const int32_t *order_f,
                  const int32_t *offsets_p, bool need_order_f, int B, int N, int Nv, int F, int points_per_batch, BackwardArgs &a)
{
    if (!points) return NR_E_NULL;
    if (int e = mesh_args(vertices, faces_idx, adj_offsets, adj_entries, B, Nv, F, 0, 0, need_adjacency, a.mesh)) return e;
    if (face_ids && (!bary_p || !grad_p || (need_order_p && (!order_p || !offsets_f)))) return NR_E_NULL;
    if (point_ids && (!bary_f || !grad_f || (need_order_f && (!order_f || !offsets_p)))) return NR_E_NULL;
    if (!sweep_sizes_ok(B, N, Nv, F)) return NR_E_SIZE;
    if (!face_ids && !point_ids) return NR_E_MODE;
    a.points = points; a.N = N; a.points_per_batch = points_per_batch != 0;
    a.face_ids = face_ids; a.bary_p = bary_p; a.grad_p = grad_p; a.order_p = order_p; a.offsets_f = offsets_f;
    a.point_ids = point_ids; a.bary_f = bary_f; a.grad_f = grad_f; a.order_f = order_f; a.offsets_p = offsets_p;
    return 0;
}

}  // namespace

NR_API size_t nr_point_mesh_workspace_bytes(int32_t B, int32_t N, int32_t F, int32_t faces_to_points, int32_t split)
{
    SplitPlan p;
    if (!sweep_sizes_ok(B, N, 1, F) || split < 0 || !plan(faces_to_points != 0, B, N, F, split, p)) return 0;
    return part_bytes(B, p.S, faces_to_points ? F : N);
}

NR_API int nr_point_mesh_points_to_faces(const float *points, const float *vertices, const int32_t *faces, float *dist2,
                                         int32_t *face_ids, float *barycentric, int32_t B, int32_t N, int32_t Nv, int32_t F,
                                         int32_t points_per_batch, int32_t split, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return sweep(false, points, vertices, faces, dist2, face_ids, barycentric, B, N, Nv, F, points_per_batch, split, workspace,
                 workspace_bytes, stream);
}

NR_API int nr_point_mesh_faces_to_points(const float *points, const float *vertices, const int32_t *faces, float *dist2,
                                         int32_t *point_ids, float *barycentric, int32_t B, int32_t N, int32_t Nv, int32_t F,
                                         int32_t points_per_batch, int32_t split, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return sweep(true, points, vertices, faces, dist2, point_ids, barycentric, B, N, Nv, F, points_per_batch, split, workspace,
                 workspace_bytes, stream);
}

NR_API int nr_point_mesh_loss(const float *dist2_points, const float *dist2_faces, float *loss, int32_t B, int32_t N, int32_t F,
                              double weight_points, double weight_faces, void *stream)
{
    if (!loss) return NR_E_NULL;
    if (!dist2_points && !dist2_faces) return NR_E_MODE;
    if (!rows_ok(B, dist2_points ? N : 1) || !rows_ok(B, dist2_faces ? F : 1)) return NR_E_SIZE;
    hipLaunchKernelGGL(k_loss, dim3((unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream, dist2_points, dist2_faces, loss, N, F,
                       weight_points, weight_faces);
    return launch_status();
}

NR_API int nr_point_mesh_backward_points(const float *points, const float *vertices, const int32_t *faces, const int32_t *face_ids,
                                         const float *barycentric_points, const float *grad_dist2_points,
                                         const int32_t *point_ids, const float *barycentric_faces, const float *grad_dist2_faces,
                                         const int32_t *order_faces, const int32_t *offsets_points, float *grad_points, int32_t B,
                                         int32_t N, int32_t Nv, int32_t F, void *stream)
{
    if (!grad_points) return NR_E_NULL;
    BackwardArgs a;
    if (int e = backward_args(points, vertices, faces, nullptr, nullptr, false, face_ids, barycentric_points, grad_dist2_points,
                              nullptr, nullptr, false, point_ids, barycentric_faces, grad_dist2_faces, order_faces, offsets_points,
                              true, B, N, Nv, F, 1, a))
        return e;
    hipLaunchKernelGGL(k_backward_points, grid_of(N, B), dim3(BLOCK), 0, (hipStream_t)stream, a, grad_points);
    return launch_status();
}

NR_API int nr_point_mesh_backward_vertices(const float *points, const float *vertices, const int32_t *faces,
                                           const int32_t *adj_offsets, const int32_t *adj_entries, const int32_t *face_ids,
                                           const float *barycentric_points, const float *grad_dist2_points,
                                           const int32_t *order_points, const int32_t *offsets_faces, const int32_t *point_ids,
                                           const float *barycentric_faces, const float *grad_dist2_faces, float *grad_vertices,
                                           int32_t B, int32_t N, int32_t Nv, int32_t F, int32_t points_per_batch, void *stream)
{
    if (!grad_vertices) return NR_E_NULL;
    BackwardArgs a;
    if (int e = backward_args(points, vertices, faces, adj_offsets, adj_entries, true, face_ids, barycentric_points,
                              grad_dist2_points, order_points, offsets_faces, true, point_ids, barycentric_faces, grad_dist2_faces,
                              nullptr, nullptr, false, B, N, Nv, F, points_per_batch, a))
        return e;
    hipLaunchKernelGGL(k_backward_vertices, grid_of(Nv, B), dim3(BLOCK), 0, (hipStream_t)stream, a, grad_vertices);
    return launch_status();
}
