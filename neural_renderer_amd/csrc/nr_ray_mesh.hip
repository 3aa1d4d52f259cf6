// nr_ray_mesh.hip -- ray casting (include/nr_hip.h; DESIGN "Ray casting"): for every ray of a bundle the first face of a mesh it
// hits -- its parameter t, the face and the barycentric weights of the hit point -- or whether it hits any face at all, by a
// brute-force rays x faces sweep.  One topology per call; world-space vertices [B, Nv, 3]; no gradients here (the
// differentiable t is a few lines of torch on the gathered winners, neural_renderer_amd/ray_mesh.py).
//
//   k_sweep<false>  first hit: (image, Q rays per thread in registers): the faces stream through LDS in tiles of T records
//                   (nr_ray_triangle.h: three 16-byte words, read as broadcast ds_read_b128s), built by the tile loader from
//                   `vertices` and `faces`; the running minimum of t takes a strict < in ascending face order
//   k_sweep<true>   any hit: the same sweep with one flag per ray; a workgroup leaves the tile loop once all its rays are
//                   occluded -- decided by the whole workgroup at the tile barrier (__syncthreads_and)
//   k_merge<ANY>    small calls: the faces are split over S workgroups, each writing its minimum and id (its flag); the parts
//                   are merged in ascending order with the same strict < (with OR), so the result does not depend on S
//   finish          the winning pair is evaluated once more WITH its weights (the same function, the same bits) and t, the id
//                   and the weights are stored -- every output element exactly once; a miss stores +inf, -1 and zeros
// No atomics and no scratch beyond the split's parts: the same bits in every run, for an image alone or inside a batch, split
// or not.  A NaN never wins a strict < and fails the inside test, so ids are always in [-1, F).
#include "nr_pair_sweep.h"
#include "nr_ray_triangle.h"

using namespace nr;

namespace {

// measurement builds set other values (python -m neural_renderer_amd._build <tag> NR_RAY_Q=4; scripts/ray_mesh_timing.py)
#ifndef NR_RAY_Q
#define NR_RAY_Q 2
#endif
#ifndef NR_RAY_T
#define NR_RAY_T 256
#endif
#ifndef NR_RAY_SPLIT_BELOW
#define NR_RAY_SPLIT_BELOW 1024
#endif

constexpr int BLOCK = 256;
constexpr int Q = NR_RAY_Q;                      // rays per thread
constexpr int T = NR_RAY_T;                      // face records per LDS tile
constexpr int SPLIT_BELOW = NR_RAY_SPLIT_BELOW;  // fewer workgroups than this: split the faces

struct SweepArgs {
    MeshArgs mesh;
    const float *origins;     // [B or 1, R, 3]
    const float *directions;  // [B or 1, R, 3]
    int R, rays_per_batch;
    float near, far;
    int cull;
    int S, chunk;             // the faces in S parts of `chunk` faces (a multiple of T)
    float *part_t;            // [B, S, R] when S > 1 (first hit)
    int32_t *part_id;         // [B, S, R] when S > 1 (first hit: the id; any hit: the flag)
    float *t;                 // [B, R]
    int32_t *ids;             // [B, R]
    float *bary;              // [B, R, 3]
    unsigned char *occluded;  // [B, R] (any hit)
};

__device__ __forceinline__ Ray ray_of(const SweepArgs &a, int b, int i)
{
    const size_t o = ((a.rays_per_batch ? (size_t)b * a.R : 0) + (size_t)i) * 3;
    const float *p = a.origins + o, *d = a.directions + o;
    Ray r;
    r.ox = p[0]; r.oy = p[1]; r.oz = p[2];
    r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
    return r;
}

// row i of the first-hit outputs: the pair (ray i, face id) once more with its weights, or a miss for id < 0
__device__ __forceinline__ void finish(const SweepArgs &a, int b, int i, int id)
{
    float t = __builtin_inff(), bw[3] = {0.0f, 0.0f, 0.0f};
    if (id >= 0) {
        int vi[3];
        float w[3][3];
        load_face(a.mesh, b, id, vi, w);
        const RayRecord R = ray_record(w);
        t = ray_triangle<true>(R, ray_of(a, b, i), a.near, a.far, a.cull != 0, bw);
    }
    const size_t o = (size_t)b * a.R + i;
    a.t[o] = t;
    a.ids[o] = id;
    a.bary[o * 3] = bw[0];
    a.bary[o * 3 + 1] = bw[1];
    a.bary[o * 3 + 2] = bw[2];
}

template <bool ANY>
__global__ __launch_bounds__(BLOCK) void k_sweep(SweepArgs a)
{
    __shared__ float4 tile[T][RAY_RECORD_WORDS];
    const int b = blockIdx.y, s = blockIdx.x % a.S, blk = blockIdx.x / a.S, tid = threadIdx.x;
    const int F = a.mesh.Nf, N = a.R;
    const float near = a.near, far = a.far;
    const bool cull = a.cull != 0;
    Ray ray[Q];
    float best[Q];
    int id[Q], ri[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        ri[q] = (blk * Q + q) * BLOCK + tid;
        ray[q] = ray_of(a, b, min(ri[q], N - 1));
        best[q] = __builtin_inff();
        id[q] = ANY ? (ri[q] >= N ? 1 : 0) : -1;  // (any hit: a thread without a ray does not keep the workgroup in the loop)
    }
    const int f_begin = s * a.chunk, f_end = min(F, f_begin + a.chunk);
    for (int f0 = f_begin; f0 < f_end; f0 += T) {
        if (ANY) {
            int done = 1;
#pragma unroll
            for (int q = 0; q < Q; q++) done &= id[q];
            if (__syncthreads_and(done)) break;  // the same answer in every thread of the workgroup
        } else {
            __syncthreads();
        }
        for (int t = tid; t < T; t += BLOCK) {
            if (f0 + t < f_end) {
                int vi[3];
                float w[3][3];
                load_face(a.mesh, b, f0 + t, vi, w);
                const RayRecord R = ray_record(w);
                tile[t][0] = R.v0; tile[t][1] = R.e1; tile[t][2] = R.e2;
            }
        }
        __syncthreads();
        const int nf = min(T, f_end - f0);
        for (int j = 0; j < nf; j++) {
            RayRecord R;
            R.v0 = tile[j][0]; R.e1 = tile[j][1]; R.e2 = tile[j][2];
            // the padding counts as used: ds_read_b128s, not ds_read_b96s.  This leans on the compiler; after a toolchain change
            // compile this file alone with --save-temps and look for ds_read_b128 (three per sweep) and no ds_read_b96 in the .s
            asm volatile("" ::"v"(R.v0.w), "v"(R.e1.w), "v"(R.e2.w));
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const float t = ray_triangle<false>(R, ray[q], near, far, cull, nullptr);
                if (ANY) {
                    if (t < __builtin_inff()) id[q] = 1;
                } else if (t < best[q]) {
                    best[q] = t;
                    id[q] = f0 + j;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
        if (ri[q] >= N) continue;
        if (a.S > 1) {
            const size_t o = ((size_t)b * a.S + s) * N + ri[q];
            if (!ANY) a.part_t[o] = best[q];
            a.part_id[o] = id[q];
        } else if (ANY) {
            a.occluded[(size_t)b * N + ri[q]] = (unsigned char)id[q];
        } else {
            finish(a, b, ri[q], id[q]);
        }
    }
}

// the S parts of every ray in ascending order
template <bool ANY>
__global__ __launch_bounds__(BLOCK) void k_merge(SweepArgs a)
{
    const int N = a.R, i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    if (ANY) {
        int flag = 0;
        for (int s = 0; s < a.S; s++) flag |= a.part_id[((size_t)b * a.S + s) * N + i];
        a.occluded[(size_t)b * N + i] = (unsigned char)(flag != 0);
    } else {
        finish(a, b, i, merge_argmin(a.part_t, a.part_id, b, a.S, N, i, -1, a.mesh.Nf - 1));
    }
}

// --------------------------------------------------------------------------------------------------------------------
// host

// the split of the faces for N rays, BLOCK * Q to a workgroup -> the sweep's workgroups along x, 0: more than a grid holds
unsigned plan(int B, int N, int F, int split, SplitPlan &p)
{
    p = plan_split(B, N, BLOCK * Q, F, T, SPLIT_BELOW, split);
    return grid_x(N, BLOCK * Q, p.S);
}

size_t part_bytes(int B, int S, int N, bool any)
{
    return S > 1 ? (size_t)B * S * N * (any ? sizeof(int32_t) : sizeof(float) + sizeof(int32_t)) : 0;
}

int run(bool any, const float *origins, const float *directions, const float *vertices, const int32_t *faces_idx, float *t,
        int32_t *ids, float *bary, unsigned char *occluded, int B, int N, int Nv, int F, int rays_per_batch, double near, double far,
        int cull, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!origins || !directions) return NR_E_NULL;
    if (any ? !occluded : (!t || !ids || !bary)) return NR_E_NULL;
    SweepArgs a;
    if (int e = mesh_args(vertices, faces_idx, nullptr, nullptr, B, Nv, F, 0, 0, false, a.mesh)) return e;
    if (!sweep_sizes_ok(B, N, Nv, F) || split < 0) return NR_E_SIZE;
    if ((rays_per_batch != 0 && rays_per_batch != 1) || (cull != 0 && cull != 1) || near != near || far != far) return NR_E_MODE;
    SplitPlan p;
    const unsigned groups_x = plan(B, N, F, split, p);
    if (!groups_x) return NR_E_SIZE;  // (a forced split near the tile count on a very large bundle)
    a.S = p.S; a.chunk = p.chunk;
    const size_t need = part_bytes(B, a.S, N, any);
    if (need && (!workspace || workspace_bytes < need)) return NR_E_WORKSPACE;
    a.origins = origins; a.directions = directions; a.R = N; a.rays_per_batch = rays_per_batch;
    a.near = (float)near; a.far = (float)far; a.cull = cull;
    a.part_id = need ? (int32_t *)workspace : nullptr;
    a.part_t = need && !any ? (float *)((int32_t *)workspace + (size_t)B * a.S * N) : nullptr;
    a.t = t; a.ids = ids; a.bary = bary; a.occluded = occluded;
    hipStream_t st = (hipStream_t)stream;
    void (*const sweep)(SweepArgs) = any ? k_sweep<true> : k_sweep<false>;
    void (*const merge)(SweepArgs) = any ? k_merge<true> : k_merge<false>;
    return launch_sweep(a.S, [&] { hipLaunchKernelGGL(sweep, dim3(groups_x, (unsigned)B), dim3(BLOCK), 0, st, a); },
                        [&] { hipLaunchKernelGGL(merge, grid_of(N, B), dim3(BLOCK), 0, st, a); });
}

}  // namespace

NR_API size_t nr_ray_mesh_workspace_bytes(int32_t B, int32_t R, int32_t F, int32_t any_hit, int32_t split)
{
    SplitPlan p;
    if (!sweep_sizes_ok(B, R, 1, F) || split < 0 || !plan(B, R, F, split, p)) return 0;  // (the call itself: NR_E_SIZE)
    return part_bytes(B, p.S, R, any_hit != 0);
}

NR_API int nr_ray_mesh_first_hit(const float *origins, const float *directions, const float *vertices, const int32_t *faces,
                                 float *t, int32_t *face_ids, float *barycentric, int32_t B, int32_t R, int32_t Nv, int32_t F,
                                 int32_t rays_per_batch, double near, double far, int32_t cull, int32_t split, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return run(false, origins, directions, vertices, faces, t, face_ids, barycentric, nullptr, B, R, Nv, F, rays_per_batch, near, far,
               cull, split, workspace, workspace_bytes, stream);
}

NR_API int nr_ray_mesh_any_hit(const float *origins, const float *directions, const float *vertices, const int32_t *faces,
                               unsigned char *occluded, int32_t B, int32_t R, int32_t Nv, int32_t F, int32_t rays_per_batch,
                               double near, double far, int32_t cull, int32_t split, void *workspace, size_t workspace_bytes,
                               void *stream)
{
    return run(true, origins, directions, vertices, faces, nullptr, nullptr, nullptr, occluded, B, R, Nv, F, rays_per_batch, near, far,
               cull, split, workspace, workspace_bytes, stream);
}
