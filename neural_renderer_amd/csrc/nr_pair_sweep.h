// nr_pair_sweep.h -- what the dense pair sweeps share (nr_point_mesh.hip, nr_winding.hip, nr_ray_mesh.hip; DESIGN "Pair
// sweeps"): every row (a point, a ray or a face, in registers) meets every item of the streamed side, which goes through LDS in
// tiles of T records; small calls cut the streamed side at tile boundaries into S parts over more workgroups, and a second
// launch merges a row's parts in ascending order.  Shared: the sizes check, the split plan, the 64-bit workgroup count, the
// sweep-then-merge launch sequence and the ordered arg-min merge.  The sweep kernels with their tile loops stay in the
// operators' files: a shared tile loop gave the same bits but slower kernels (LAB-NOTEBOOK).
#pragma once
#include "nr_mesh_gather.h"

namespace nr {

// the streamed side in S parts of `chunk` items (a multiple of T); `tiles` tiles in all
struct SplitPlan {
    int S, chunk, tiles;
};

// the S parts (value, id) of a row, laid out [B, S, rows], in ascending order under a strict <, so the winner does not depend
// on S; the id starts at `none` (0 where a row always has a pair, -1 where it may have none) and is clamped to [none, last]
// for memory safety
__device__ __forceinline__ int merge_argmin(const float *part_value, const int32_t *part_id, int b, int S, int rows, int row,
                                            int none, int last)
{
    float best = __builtin_inff();
    int id = none;
    for (int s = 0; s < S; s++) {
        const size_t o = ((size_t)b * S + s) * rows + row;
        const float v = part_value[o];
        if (v < best) { best = v; id = part_id[o]; }
    }
    return clampi(id, none, last);
}

// --------------------------------------------------------------------------------------------------------------------
// host

// B on grid.y; int32 indexing of [B, n, 3] inside the kernels: n rows (or streamed items) per image
inline bool rows_ok(int B, int n) { return B >= 1 && B <= 65535 && n >= 1 && (size_t)B * (size_t)n <= 0x7fffffffull / 3; }

// the sizes of a sweep of N points or rays against a mesh
inline bool sweep_sizes_ok(int B, int N, int Nv, int F) { return rows_ok(B, N) && mesh_sizes_ok(B, Nv, F); }

// The streamed side (cols items, tiles of T) for `rows` rows handled `per_block` to a workgroup: one part when the grid fills
// the machine (or split == 1), else enough parts to reach split_below workgroups (split > 1: that many), never more than there
// are tiles, and no part empty.
inline SplitPlan plan_split(int B, int rows, int per_block, int cols, int T, int split_below, int split)
{
    const long long groups = (long long)((rows + per_block - 1) / per_block) * B;
    const int tiles = (cols + T - 1) / T;
    long long want = split > 0 ? split : (groups >= split_below ? 1 : (split_below + groups - 1) / groups);
    if (want > tiles) want = tiles;
    const int per_part = (tiles + (int)want - 1) / (int)want;
    return {(tiles + per_part - 1) / per_part, per_part * T, tiles};
}

// the sweep's workgroups along x, counted in 64 bits -> 0 above 2^31 - 1 (a forced split near the tile count on a very large
// call): the entry points then return NR_E_SIZE, before they look at the workspace
inline unsigned grid_x(int rows, int per_block, int S)
{
    const long long n = (long long)((rows + per_block - 1) / per_block) * S;
    return n > 0x7fffffffll ? 0u : (unsigned)n;
}

// the launch sequence: sweep(), and merge() when the call is split, each followed by its status
template <class Sweep, class Merge>
inline int launch_sweep(int S, Sweep sweep, Merge merge)
{
    sweep();
    const int rc = launch_status();
    if (rc || S == 1) return rc;
    merge();
    return launch_status();
}

}  // namespace nr
