// nr_isosurface.hip -- isosurface extraction by marching tetrahedra (include/nr_hip.h; DESIGN "Isosurface extraction"): from
// values [B, D, H, W] to, per image, the crossing edges `edge_nodes` (one vertex each) and the triangles `faces` over them, in the
// order that nr_marching_tets.h defines.  Topology only: the positions are a few lines of torch on the gathered nodes
// (neural_renderer_amd/isosurface.py).
//
// A workgroup owns a RUN of `run` consecutive nodes of one image (blockIdx.y) and walks it in rounds of BLOCK, thread order =
// node order, so a scan over the threads is a scan over the nodes.
//   k_count   per node the 8 values of its cell (indices clamped at the grid's end) -> the 8-bit inside mask; the 7 owned edges
//             cross where a corner's bit differs from bit 0; the cell's triangles from the table.  Both counts are scanned
//             in one word (vertices in the low half, triangles in the high half: 7 x 4096 and 12 x 4096 fit 16 bits) -- a wave
//             scan, the waves through LDS, a carry from round to round.  Stored per node: `info` = exclusive vertex prefix
//             << 8 | crossing bits 1..7 | inside bit of the node, and the triangle prefix (16 bits).  Per workgroup its totals
//             and whether it saw a non-finite value.
//   k_scan    one workgroup per image walks the workgroups' totals in passes of BLOCK: exclusive offsets per workgroup, the
//             image's totals (vertices, triangles, non-finite) -- which the host reads back, its one synchronisation -- and
//             once more over the images (64-bit) for the rows at which an image's outputs begin.
//   k_emit    the same mapping, from `info` alone -- the values are not read again, so what is written is what was counted: a
//             node stores its crossing edges (a, b) from its own offset; a cell looks up the vertex of each table entry at
//             the edge's owner (a corner of the cell): offset[workgroup of the owner] + prefix[owner] + popcount(owner's
//             crossing bits below the edge code).  No barrier; every store is checked against the rows the caller allocated.
// No atomics, no workgroup waits for another: the same bits in every run, for an image alone or inside a batch, for any run.
#include "nr_device.h"
#include "nr_marching_tets.h"

using namespace nr;

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / WAVE;
constexpr int RUN_DEFAULT = 1024;
constexpr int RUN_MAX = 4096;  // 7 x RUN_MAX and 12 x RUN_MAX fit the scan's 16-bit halves

struct IsoArgs {
    const float *values;          // [B, N]
    int B, D, H, W, N;
    float iso;
    int above;
    int run, nwg;                 // nodes per workgroup, workgroups per image
    uint32_t *info;               // [B, N]
    uint16_t *fpre;               // [B, N]
    uint32_t *wg_tot;             // [B, nwg, 3]
    uint32_t *wg_off;             // [B, nwg, 2]
    uint32_t *totals;             // [B, 3] (the caller's)
    unsigned long long *img_off;  // [B, 2]
    int32_t *edge_nodes;          // [cap_v, 2]
    int32_t *faces;               // [cap_f, 3]
    unsigned long long cap_v, cap_f;
};

// exclusive prefix of v over the workgroup's threads and the workgroup's total; `part` is WAVES words of LDS (nr_reduce.h)
template <typename T>
__device__ __forceinline__ T excl_scan(T v, T *part, T &total)
{
    return block_excl_scan<BLOCK>(v, wave_incl_scan(v, (int)(threadIdx.x & (WAVE - 1))), part, &total);
}

// node n + the step of corner / edge `code` (4 di + 2 dj + dk) with the strides of the axes
__device__ __forceinline__ int step_of(int code, int si, int sj, int sk)
{
    return ((code & 4) ? si : 0) + ((code & 2) ? sj : 0) + ((code & 1) ? sk : 0);
}

__global__ __launch_bounds__(BLOCK) void k_count(IsoArgs a)
{
    __shared__ unsigned part[WAVES];
    const int b = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x;
    const int HW = a.H * a.W;
    const float *val = a.values + (size_t)b * a.N;
    unsigned carry = 0;
    int bad = 0;
    for (int r0 = 0; r0 < a.run; r0 += BLOCK) {
        const int local = r0 + tid;
        const long long n64 = (long long)wg * a.run + local;
        const bool valid = local < a.run && n64 < a.N;
        unsigned pack = 0, word = 0;
        if (valid) {
            const int n = (int)n64;
            const int i = n / HW, rem = n - i * HW, j = rem / a.W, k = rem - j * a.W;
            // a step beyond the grid's end stays where it is: every load is inside the image, and the edge does not count
            const int si = i + 1 < a.D ? HW : 0, sj = j + 1 < a.H ? a.W : 0, sk = k + 1 < a.W ? 1 : 0;
            unsigned in = 0, ok = 0;
#pragma unroll
            for (int code = 0; code < 8; code++) {
                const float v = val[n + step_of(code, si, sj, sk)];
                if (code == 0 && !__builtin_isfinite(v)) bad = 1;
                in |= (unsigned)(a.above ? v > a.iso : v < a.iso) << code;
                ok |= (unsigned)((!(code & 4) || si) && (!(code & 2) || sj) && (!(code & 1) || sk)) << code;
            }
            const unsigned cm = (in ^ ((in & 1u) ? 0xffu : 0u)) & ok & 0xfeu;  // owned edges with one inside end
            const unsigned nf = ok == 0xffu ? cell_triangles(in) : 0u;
            pack = __popc(cm) | nf << 16;
            word = cm | (in & 1u);
        }
        unsigned total;
        const unsigned excl = carry + excl_scan(pack, part, total);
        if (valid) {
            const size_t g = (size_t)b * a.N + (size_t)n64;
            a.info[g] = (excl & 0xffffu) << 8 | word;
            a.fpre[g] = (uint16_t)(excl >> 16);
        }
        carry += total;
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        uint32_t *t = a.wg_tot + ((size_t)b * a.nwg + wg) * 3;
        t[0] = carry & 0xffffu;
        t[1] = carry >> 16;
        t[2] = (uint32_t)(bad != 0);
    }
}

// rows of n triples (count, count, flag): exclusive offsets of the two counts per entry, and per row the sums and the flags' OR
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_scan(const uint32_t *in, T *off, uint32_t *sums, int n)
{
    __shared__ T part[WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    in += (size_t)row * n * 3;
    off += (size_t)row * n * 2;
    T c0 = 0, c1 = 0;
    int flag = 0;
    for (int p0 = 0; p0 < n; p0 += BLOCK) {
        const int i = p0 + tid;
        const bool valid = i < n;
        const T v0 = valid ? in[(size_t)i * 3] : 0, v1 = valid ? in[(size_t)i * 3 + 1] : 0;
        if (valid && in[(size_t)i * 3 + 2]) flag = 1;
        T t0, t1;
        const T e0 = excl_scan(v0, part, t0), e1 = excl_scan(v1, part, t1);
        if (valid) {
            off[(size_t)i * 2] = c0 + e0;
            off[(size_t)i * 2 + 1] = c1 + e1;
        }
        c0 += t0;
        c1 += t1;
    }
    flag = __syncthreads_or(flag);
    if (sums && tid == 0) {
        sums[(size_t)row * 3] = (uint32_t)c0;
        sums[(size_t)row * 3 + 1] = (uint32_t)c1;
        sums[(size_t)row * 3 + 2] = (uint32_t)(flag != 0);
    }
}

__global__ __launch_bounds__(BLOCK) void k_emit(IsoArgs a)
{
    // per thread the seven possible owners of its cell's vertices (corner codes 0 .. 6): vertex offset and crossing bits
    __shared__ unsigned s_base[7][BLOCK], s_cm[7][BLOCK];
    const int b = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x;
    const int HW = a.H * a.W;
    const uint32_t *info = a.info + (size_t)b * a.N;
    const uint32_t *wg_off = a.wg_off + (size_t)b * a.nwg * 2;
    for (int r0 = 0; r0 < a.run; r0 += BLOCK) {
        const int local = r0 + tid;
        const long long n64 = (long long)wg * a.run + local;
        if (!(local < a.run && n64 < a.N)) continue;
        const int n = (int)n64;
        const unsigned word = info[n], cm = word & 0xfeu;
        if (!cm) continue;  // no crossing edge: no vertex, and a cell with eight equal corners
        const int i = n / HW, rem = n - i * HW, j = rem / a.W, k = rem - j * a.W;
        const unsigned first = wg_off[(size_t)wg * 2] + (word >> 8);
        unsigned long long row = a.img_off[(size_t)b * 2] + first;
#pragma unroll
        for (int code = 1; code < 8; code++) {
            if ((cm >> code) & 1u) {
                if (row < a.cap_v) {
                    a.edge_nodes[row * 2] = n;
                    a.edge_nodes[row * 2 + 1] = n + step_of(code, HW, a.W, 1);
                }
                row++;
            }
        }
        if (!(i + 1 < a.D && j + 1 < a.H && k + 1 < a.W)) continue;
        const unsigned in = ((word & 1u) ? 0xffu : 0u) ^ cm;  // the cell's inside mask (all 7 edges exist here)
        s_base[0][tid] = first;
        s_cm[0][tid] = cm;
#pragma unroll
        for (int o = 1; o < 7; o++) {
            const int no = n + step_of(o, HW, a.W, 1);
            const unsigned w2 = info[no];
            s_base[o][tid] = wg_off[(size_t)(no / a.run) * 2] + (w2 >> 8);
            s_cm[o][tid] = w2 & 0xfeu;
        }
        unsigned long long frow = a.img_off[(size_t)b * 2 + 1] + wg_off[(size_t)wg * 2 + 1] + a.fpre[(size_t)b * a.N + n];
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const unsigned tm = tet_mask(in, t);
            const int nt = TET_TRIANGLES[tm];
            for (int s = 0; s < nt; s++) {
                int id[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const unsigned entry = TET_TABLE[t][tm][3 * s + c], o = entry >> 3, e = entry & 7u;
                    id[c] = (int)(s_base[o][tid] + __popc(s_cm[o][tid] & ((1u << e) - 1u)));
                }
                if (frow < a.cap_f) {
                    a.faces[frow * 3] = id[0];
                    a.faces[frow * 3 + 1] = id[1];
                    a.faces[frow * 3 + 2] = id[2];
                }
                frow++;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------
// host

// B on grid.y; 7 N < 2^31: a vertex number and a node number fit int32, 12 N triangles fit uint32
bool sizes_ok(int B, int D, int H, int W, int run)
{
    if (B < 1 || B > 65535 || D < 2 || H < 2 || W < 2 || run < 0 || run > RUN_MAX) return false;
    return (unsigned long long)D * (unsigned long long)H * (unsigned long long)W * 7ull < 0x80000000ull;
}

struct Layout {
    size_t info, fpre, wg_tot, wg_off, img_off, bytes;
    int run, nwg;
};

Layout layout_of(int B, int D, int H, int W, int run)
{
    Layout l;
    const size_t N = (size_t)D * H * W;
    l.run = run > 0 ? run : RUN_DEFAULT;
    l.nwg = (int)((N + l.run - 1) / l.run);
    size_t at = 0;
    l.info = at;    at = align_up(at + (size_t)B * N * sizeof(uint32_t), 16);
    l.fpre = at;    at = align_up(at + (size_t)B * N * sizeof(uint16_t), 16);
    l.wg_tot = at;  at = align_up(at + (size_t)B * l.nwg * 3 * sizeof(uint32_t), 16);
    l.wg_off = at;  at = align_up(at + (size_t)B * l.nwg * 2 * sizeof(uint32_t), 16);
    l.img_off = at; at = align_up(at + (size_t)B * 2 * sizeof(unsigned long long), 16);
    l.bytes = at;
    return l;
}

int args_of(int B, int D, int H, int W, int run, void *workspace, size_t workspace_bytes, IsoArgs &a)
{
    if (!sizes_ok(B, D, H, W, run)) return NR_E_SIZE;
    const Layout l = layout_of(B, D, H, W, run);
    if (!workspace || workspace_bytes < l.bytes) return NR_E_WORKSPACE;
    unsigned char *ws = (unsigned char *)workspace;
    a.B = B; a.D = D; a.H = H; a.W = W; a.N = D * H * W;
    a.run = l.run; a.nwg = l.nwg;
    a.info = (uint32_t *)(ws + l.info);
    a.fpre = (uint16_t *)(ws + l.fpre);
    a.wg_tot = (uint32_t *)(ws + l.wg_tot);
    a.wg_off = (uint32_t *)(ws + l.wg_off);
    a.img_off = (unsigned long long *)(ws + l.img_off);
    a.values = nullptr; a.totals = nullptr; a.edge_nodes = nullptr; a.faces = nullptr;
    a.iso = 0.0f; a.above = 0; a.cap_v = a.cap_f = 0;
    return 0;
}

}  // namespace

NR_API size_t nr_isosurface_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W, int32_t run)
{
    return sizes_ok(B, D, H, W, run) ? layout_of(B, D, H, W, run).bytes : 0;
}

NR_API int nr_isosurface_count(const float *values, int32_t *totals, int32_t B, int32_t D, int32_t H, int32_t W, double iso,
                               int32_t above, int32_t run, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!values || !totals) return NR_E_NULL;
    IsoArgs a;
    if (int e = args_of(B, D, H, W, run, workspace, workspace_bytes, a)) return e;
    if ((above != 0 && above != 1) || !(iso - iso == 0.0)) return NR_E_MODE;
    a.values = values; a.totals = (uint32_t *)totals; a.iso = (float)iso; a.above = above;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_count, dim3((unsigned)a.nwg, (unsigned)B), dim3(BLOCK), 0, st, a);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_scan<uint32_t>, dim3((unsigned)B), dim3(BLOCK), 0, st, (const uint32_t *)a.wg_tot, a.wg_off, a.totals, a.nwg);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_scan<unsigned long long>, dim3(1), dim3(BLOCK), 0, st, (const uint32_t *)a.totals, a.img_off,
                       (uint32_t *)nullptr, B);
    return launch_status();
}

NR_API int nr_isosurface_emit(int32_t *edge_nodes, int32_t *faces, size_t num_vertices, size_t num_faces, int32_t B, int32_t D,
                              int32_t H, int32_t W, int32_t run, void *workspace, size_t workspace_bytes, void *stream)
{
    if ((num_vertices && !edge_nodes) || (num_faces && !faces)) return NR_E_NULL;
    IsoArgs a;
    if (int e = args_of(B, D, H, W, run, workspace, workspace_bytes, a)) return e;
    if (!num_vertices && !num_faces) return 0;
    a.edge_nodes = edge_nodes; a.faces = faces; a.cap_v = num_vertices; a.cap_f = num_faces;
    hipLaunchKernelGGL(k_emit, dim3((unsigned)a.nwg, (unsigned)B), dim3(BLOCK), 0, (hipStream_t)stream, a);
    return launch_status();
}
