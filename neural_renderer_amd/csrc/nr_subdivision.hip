// nr_subdivision.hip -- mesh subdivision as a sparse linear operator (include/nr_hip.h; DESIGN "Mesh subdivision"): one level
// of Loop or midpoint refinement is a table with a row per OUTPUT vertex, applied to per-vertex data [B, num_in, C]; its
// backward is the transposed table -- a row per INPUT vertex -- applied to the incoming gradient by the same kernel.  The
// tables are built on the host (neural_renderer_amd/subdivision.py) and shared by the images of a call.
//
// One level, on faces [F, 3] over Nv vertices:
//   edges: every unordered pair {p < q} that is a side of a face, E of them, ordered by (p, q); edge e owns new vertex
//     Nv + e, old vertices keep their indices: Nv' = Nv + E.  m(e): the (face, side) occurrences of e, duplicate faces
//     counted; e is SHARP when m(e) != 2 (a boundary edge, an edge in three or more faces).
//   children of f = (a, b, c): 4 f .. 4 f + 3 = (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca); the winding is kept.
//   midpoint: old vertex v: {v: 1}; edge vertex: {p: 1/2, q: 1/2}.
//   loop (Loop's rules, Warren's weights, the usual boundary and crease rules); N(v): the distinct vertices joined to v by an
//     edge, n = |N(v)|, s(v): the sharp edges at v.
//       old vertex, n = 0:        {v: 1}
//       old vertex, s = 0:        beta = 3/16 if n = 3 else 3 / (8 n); {v: 1 - n beta, u: beta for u in N(v)}
//       old vertex, s = 2:        {v: 3/4, the two sharp neighbours: 1/8 each}
//       old vertex, any other s:  {v: 1}                                   (a corner, a non-manifold point)
//       edge vertex, sharp:       {p: 1/2, q: 1/2}
//       edge vertex, m = 2:       {p: 3/8, q: 3/8, o1: 1/8, o2: 1/8}, o1 / o2 the opposite vertices
//   The weights are evaluated in float64, entries of a row with one column added in float64 (o1 = o2), rounded to float32
//   once.  Every row sums to 1.
//
// The float32 operation order of a row (k_stencil_apply): its entries in table order -- ascending column --, x_k the input of
// the k-th entry:  acc = w_0 * x_0 (one rounding);  acc = fmaf(w_k, x_k, acc) for k = 1, 2, ...  The fmaf is written out
// (the build has -ffp-contract=off).  A row {v: 1} copies its input bit for bit; a row without entries stores 0.
//
// No atomics, every output element is stored, one launch per call: the same bits in every run, and an image alone gives the
// bits it has inside a batch (every image has its own accumulator and its own fmaf chain; nothing is reduced across images).
//
// Lane mapping: a thread owns ONE output element (row, channel) of IMAGES = 4 consecutive images (grid.y = ceil(B / 4));
// consecutive lanes own consecutive elements of an image's [num_out, C] block, so a wave stores 256 contiguous bytes per
// image.  The lanes of a row read the row's offsets, columns and weights from the same addresses (one request, served from
// cache: the table is shared by all images), once for the four images, and gather 4 C contiguous bytes of each source vertex
// between them.  A row is a chain of dependent loads -- the column, then the input it points to -- and with one entry of one
// image in flight per thread the kernel waits for memory latency, not bandwidth: UNROLL = 4 entries times 4 images are
// requested before the first is used.  Measured on the MI355X (LAB-NOTEBOOK "mesh subdivision"): 1.84 x less kernel time
// than one image and one entry at a time, and ahead of (1, 4), (4, 1), (2, 4) and (8, 2).  At most 64 VGPRs, no LDS, no
// scratch: eight waves per SIMD.
#include "nr_device.h"

using namespace nr;

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_CHANNELS = 16;

// Images per thread (a row's offsets, columns and weights are read once for that many images) and entries of a row whose
// columns, weights and inputs are requested together: measured against their alternatives (LAB-NOTEBOOK "mesh subdivision").
// A call of more than IMAGES images spans several groups on grid.y, the last one possibly partial
// (tests/test_subdivision_gpu.py sizes its batches from this value).
constexpr int IMAGES = 4, UNROLL = 4;

// CC: the channel count when it is known at compile time (the division by it becomes a multiplication), 0: `channels`.
// A thread walks its row once for IMAGES images, blockIdx.y * IMAGES onwards; the row's loads are a chain -- column, then
// the input it points to -- so UNROLL entries times IMAGES images are requested before the first is used.  The fmaf chain
// of every image keeps the table's order.
template <int CC>
__global__ __launch_bounds__(BLOCK) void k_stencil_apply(const float *__restrict__ x, const int32_t *__restrict__ row_offsets,
                                                         const int32_t *__restrict__ cols, const float *__restrict__ weights,
                                                         float *__restrict__ y, int B, int num_in, int num_out, int channels,
                                                         int num_entries)
{
    const int C = CC ? CC : channels;
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b0 = blockIdx.y * IMAGES;  // i: element of an image's [num_out, C] block
    if (i >= num_out * C) return;
    const int row = i / C, c = i - row * C;
    // (offsets, columns clamped for memory safety; the host builds the table)
    const int e0 = clampi(row_offsets[row], 0, num_entries), e1 = clampi(row_offsets[row + 1], e0, num_entries);
    const size_t in_stride = (size_t)num_in * C, out_stride = (size_t)num_out * C;
    const int n_img = min(IMAGES, B - b0);  // >= 1; the slots behind the batch's end read its last image and store nothing
    const float *xb = x + (size_t)b0 * in_stride + c;
    size_t img[IMAGES];
    float acc[IMAGES];
#pragma unroll
    for (int k = 0; k < IMAGES; k++) {
        img[k] = (size_t)min(k, n_img - 1) * in_stride;
        acc[k] = 0.0f;
    }
    if (e1 > e0) {
        {
            const int s = clampi(cols[e0], 0, num_in - 1) * C;
            const float w = weights[e0];
#pragma unroll
            for (int k = 0; k < IMAGES; k++) acc[k] = w * xb[img[k] + s];
        }
        int e = e0 + 1;
        for (; e + UNROLL <= e1; e += UNROLL) {
            int s[UNROLL];
            float w[UNROLL], v[UNROLL][IMAGES];
#pragma unroll
            for (int j = 0; j < UNROLL; j++) {
                s[j] = clampi(cols[e + j], 0, num_in - 1) * C;
                w[j] = weights[e + j];
            }
#pragma unroll
            for (int j = 0; j < UNROLL; j++)
#pragma unroll
                for (int k = 0; k < IMAGES; k++) v[j][k] = xb[img[k] + s[j]];
#pragma unroll
            for (int j = 0; j < UNROLL; j++)
#pragma unroll
                for (int k = 0; k < IMAGES; k++) acc[k] = fmaf(w[j], v[j][k], acc[k]);
        }
        for (; e < e1; e++) {
            const int s = clampi(cols[e], 0, num_in - 1) * C;
            const float w = weights[e];
#pragma unroll
            for (int k = 0; k < IMAGES; k++) acc[k] = fmaf(w, xb[img[k] + s], acc[k]);
        }
    }
    float *yb = y + (size_t)b0 * out_stride + i;
#pragma unroll
    for (int k = 0; k < IMAGES; k++)
        if (k < n_img) yb[(size_t)k * out_stride] = acc[k];
}

}  // namespace

NR_API int nr_stencil_apply(const float *x, const int32_t *row_offsets, const int32_t *cols, const float *weights, float *y,
                            int32_t B, int32_t num_in, int32_t num_out, int32_t channels, int32_t num_entries, void *stream)
{
    if (!x || !row_offsets || !cols || !weights || !y) return NR_E_NULL;
    if (B < 1 || B > 65535 || num_in < 1 || num_out < 1 || num_entries < 1) return NR_E_SIZE;
    if (channels < 1 || channels > MAX_CHANNELS) return NR_E_SIZE;
    // an image's element index is an int inside the kernel
    if ((size_t)num_in * (size_t)channels > 0x7fffffffull - BLOCK || (size_t)num_out * (size_t)channels > 0x7fffffffull - BLOCK)
        return NR_E_SIZE;
    const unsigned nb = (unsigned)(((size_t)num_out * (size_t)channels + BLOCK - 1) / BLOCK);
    const dim3 grid(nb, (unsigned)((B + IMAGES - 1) / IMAGES)), block(BLOCK);
    hipStream_t st = (hipStream_t)stream;
    if (channels == 3)
        hipLaunchKernelGGL(k_stencil_apply<3>, grid, block, 0, st, x, row_offsets, cols, weights, y, B, num_in, num_out, channels,
                           num_entries);
    else if (channels == 1)
        hipLaunchKernelGGL(k_stencil_apply<1>, grid, block, 0, st, x, row_offsets, cols, weights, y, B, num_in, num_out, channels,
                           num_entries);
    else
        hipLaunchKernelGGL(k_stencil_apply<0>, grid, block, 0, st, x, row_offsets, cols, weights, y, B, num_in, num_out, channels,
                           num_entries);
    return launch_status();
}
