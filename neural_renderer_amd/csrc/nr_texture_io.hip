// nr_texture_io.hip -- the data formats either side of the path: the two one-shot kernels of the reference's
// OBJ/MTL texture pipeline.
//
//   k_bake_textures        K10, neural_renderer/load_obj.py:87-144: texture image + per-face uv triangles -> the
//                          [Nf, ts, ts, ts, 3] texture cubes the rasterizer samples (bilinear lookup at the barycentric
//                          point of every texel).
//   k_texture_atlas        K11, neural_renderer/save_obj.py:32-113: texture cubes -> one atlas image of 16x16-pixel tiles
//   k_texture_atlas_seam        (save_obj.py:115-146: the column right of each tile's diagonal repeats its left neighbour).
//
// Both are pure gathers, one thread per output element, run once per mesh; they exist so that textured meshes enter and
// leave the rasterizer in exactly the reference's encoding.
//
// Not in the reference: the same bake as a differentiable step of an optimisation (learnable UV texture images, DESIGN K10):
//   k_bake_uv              forward, every step: Bi x F x ts^3 texels from all M images of a layout in one launch
//   k_uv_map_keys / _rows / _finish   once per layout: the inverse map pixel -> (texel, weight), CSR, stably sorted
//   k_bake_uv_backward     backward, every step: one thread per (b, pixel) walks its map entries (double sums, no atomics)
// All of them take a texel's reads from texel_reads(), the arithmetic of k_bake_textures, so forward and adjoint agree.  Arithmetic: float32 in the reference's operation order, with
// its double literals (`ts - 1.`, `max(tif, 0.)`, the pasted eps) evaluated in double.
//
// Undefined behaviour of the reference that is given a definition here: image reads outside the image (uv exactly 1, or
// negative uv) are clamped to the nearest valid flat pixel index -- such reads carry weight 0 whenever the reference's
// own result is defined; atlas tiles beyond the last face stay 0.
#include "nr_device.h"

#include <rocprim/device/device_radix_sort.hpp>

using namespace nr;

namespace {

// The barycentric point of texel t = (i0*ts + i1)*ts + i2 of a face (load_obj.py:98-106): (i0,i1,i2)/(ts-1) in double,
// rounded to float, divided by its float sum.  At texel (0,0,0) the sum is 0 and the point NaN, as in the reference.
__device__ __forceinline__ void texel_point(int t, int ts, float d[3])
{
    float dim0 = (float)((double)(t / (ts * ts)) / (ts - 1.));  // :98-100
    float dim1 = (float)((double)((t / ts) % ts) / (ts - 1.));
    float dim2 = (float)((double)(t % ts) / (ts - 1.));
    const float sum = dim0 + dim1 + dim2;  // :103
    d[0] = dim0 / sum;
    d[1] = dim1 / sum;
    d[2] = dim2 / sum;
}

// The learnable bake's point: texel_point, except that texel (0,0,0) -- NaN in the reference -- is the uv centroid, with
// weights 1/3 in float (include/nr_hip.h, nr_bake_uv_textures).
__device__ __forceinline__ void uv_texel_point(int t, int ts, float d[3])
{
    if (t == 0) {
        d[0] = d[1] = d[2] = 1.0f / 3.0f;
        return;
    }
    texel_point(t, ts, d);
}

// (texel_reads, mirror_row and f2i live in nr_device.h: one definition for the bakes, the inverse map and per-pixel UV shading)

__global__ __launch_bounds__(256) void k_bake_textures(const float *__restrict__ image, const float *__restrict__ faces_uv,
                                                       const int32_t *__restrict__ is_update, float *__restrict__ textures,
                                                       size_t n, int ts, int H, int W)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int T = ts * ts * ts;
    const int fn = (int)(i / T);
    if (is_update[fn] == 0) return;  // load_obj.py:110
    float d[3];
    texel_point((int)(i % T), ts, d);
    long long p[4];
    float w[4];
    texel_reads(faces_uv + (size_t)fn * 6, d, H, W, p, w);
    float *texture = textures + i * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {  // :123-128
        float c = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) c += image[p[r] * 3 + k] * w[r];
        texture[k] = c;
    }
}

// ---- learnable UV textures -------------------------------------------------------------------------------------------
// images [Bi, P, 3]: the M images of a layout packed one after another, each [H_m, W_m, 3] top row first; table [M, 3] =
// (first pixel, H_m, W_m).  Texels of faces without an image (face_image outside [0, M)) copy `base`.
__global__ __launch_bounds__(256) void k_bake_uv(const float *__restrict__ images, const int32_t *__restrict__ table,
                                                 const float *__restrict__ faces_uv, const int32_t *__restrict__ face_image,
                                                 const float *__restrict__ base, float *__restrict__ textures, size_t n,
                                                 int num_faces, int ts, int M, int P)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int T = ts * ts * ts;
    const size_t per_image = (size_t)num_faces * T;
    const int b = (int)(i / per_image);
    const int ft = (int)(i - (size_t)b * per_image);
    const int f = ft / T;
    const int m = face_image[f];
    float *out = textures + i * 3;
    if (m < 0 || m >= M) {
        const float *src = base + (size_t)ft * 3;
        out[0] = src[0];
        out[1] = src[1];
        out[2] = src[2];
        return;
    }
    const int off = table[3 * m], H = table[3 * m + 1], W = table[3 * m + 2];
    float d[3];
    uv_texel_point(ft - f * T, ts, d);
    long long p[4];
    float w[4];
    texel_reads(faces_uv + (size_t)f * 6, d, H, W, p, w);
    const float *image = images + ((size_t)b * P + off) * 3;
    int q[4];
#pragma unroll
    for (int r = 0; r < 4; r++) q[r] = mirror_row(p[r], H, W);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float c = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) c += image[(size_t)q[r] * 3 + k] * w[r];
        out[k] = c;
    }
}

// map build 1/3: entry e = 4 * (f*T + t) + r is read r of texel t of face f; its key is the packed pixel it reads, or P
// (after every pixel) when the face has no image
__global__ __launch_bounds__(256) void k_uv_map_keys(const int32_t *__restrict__ table, const float *__restrict__ faces_uv,
                                                     const int32_t *__restrict__ face_image, uint32_t *__restrict__ keys,
                                                     uint32_t *__restrict__ entries, int n, int ts, int M, int P)
{
    const int ft = blockIdx.x * blockDim.x + threadIdx.x;
    if (ft >= n) return;
    const int T = ts * ts * ts;
    const int f = ft / T;
    const int m = face_image[f];
    uint32_t key[4] = {(uint32_t)P, (uint32_t)P, (uint32_t)P, (uint32_t)P};
    if (m >= 0 && m < M) {
        const int off = table[3 * m], H = table[3 * m + 1], W = table[3 * m + 2];
        float d[3];
        uv_texel_point(ft - f * T, ts, d);
        long long p[4];
        float w[4];
        texel_reads(faces_uv + (size_t)f * 6, d, H, W, p, w);
#pragma unroll
        for (int r = 0; r < 4; r++) key[r] = (uint32_t)(off + mirror_row(p[r], H, W));
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        keys[4 * ft + r] = key[r];
        entries[4 * ft + r] = (uint32_t)(4 * ft + r);
    }
}

// map build 2/3 (after the stable sort by key): row_ptr[p] = first sorted entry with key >= p, for p in [0, P]
__global__ __launch_bounds__(256) void k_uv_map_rows(const uint32_t *__restrict__ keys, int32_t *__restrict__ row_ptr, int n,
                                                     int P)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > P) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < (uint32_t)p)
            lo = mid + 1;
        else
            hi = mid;
    }
    row_ptr[p] = lo;
}

// map build 3/3: each sorted entry -> (texel f*T + t, the weight texel_reads gives its read)
__global__ __launch_bounds__(256) void k_uv_map_finish(const int32_t *__restrict__ table, const float *__restrict__ faces_uv,
                                                       const int32_t *__restrict__ face_image,
                                                       const uint32_t *__restrict__ keys, const uint32_t *__restrict__ entries,
                                                       int32_t *__restrict__ entry_texel, float *__restrict__ entry_weight,
                                                       int n, int ts, int M, int P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = entries[i];
    const int ft = (int)(e >> 2), r = (int)(e & 3);
    float weight = 0.0f;
    if (keys[i] < (uint32_t)P) {
        const int T = ts * ts * ts;
        const int f = ft / T;
        const int m = face_image[f];
        const int H = table[3 * m + 1], W = table[3 * m + 2];
        float d[3];
        uv_texel_point(ft - f * T, ts, d);
        long long p[4];
        float w[4];
        texel_reads(faces_uv + (size_t)f * 6, d, H, W, p, w);
        weight = w[r];
    }
    entry_texel[i] = ft;
    entry_weight[i] = weight;
}

// grad_images[b, p, :] = sum over p's entries, in map order, of grad_textures[b, texel, :] * weight: products exact in
// double, one rounding at the end.  Every pixel is written (0 without entries).
__global__ __launch_bounds__(256) void k_bake_uv_backward(const float *__restrict__ grad_textures,
                                                          const int32_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ entry_texel,
                                                          const float *__restrict__ entry_weight,
                                                          float *__restrict__ grad_images, size_t n, size_t per_image, int P)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t b = i / P;
    const int p = (int)(i - b * P);
    const float *g = grad_textures + b * per_image * 3;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    const int end = row_ptr[p + 1];
    for (int j = row_ptr[p]; j < end; j++) {
        const double w = (double)entry_weight[j];
        const float *gt = g + (size_t)entry_texel[j] * 3;
        acc0 += (double)gt[0] * w;
        acc1 += (double)gt[1] * w;
        acc2 += (double)gt[2] * w;
    }
    float *out = grad_images + i * 3;
    out[0] = (float)acc0;
    out[1] = (float)acc1;
    out[2] = (float)acc2;
}

// one thread per atlas pixel (x, y); tile (x / tso, y / tso) belongs to face fn = x / tso + (y / tso) * tile_width
__global__ __launch_bounds__(256) void k_texture_atlas(float *__restrict__ image, const float *__restrict__ vertices_all,
                                                       const float *__restrict__ textures, size_t n, int num_faces, int tsi,
                                                       int tso, int tile_width)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int width = tile_width * tso;
    const int x = (int)(i % width);
    const int y = (int)(i / width);
    const int fn = x / tso + (y / tso) * tile_width;  // save_obj.py:39-41
    float *out = image + i * 3;
    if (fn >= num_faces) {
        out[0] = out[1] = out[2] = 0.0f;
        return;
    }
    const float *texture = textures + (size_t)fn * tsi * tsi * tsi * 3;
    const float *p0 = vertices_all + (size_t)fn * 6, *p1 = p0 + 2, *p2 = p0 + 4;

    float face_inv[9] = {p1[1] - p2[1], p2[0] - p1[0], p1[0] * p2[1] - p2[0] * p1[1],   // :54-57
                         p2[1] - p0[1], p0[0] - p2[0], p2[0] * p0[1] - p0[0] * p2[1],
                         p0[1] - p1[1], p1[0] - p0[0], p0[0] * p1[1] - p1[0] * p0[1]};
    const float den = p2[0] * (p0[1] - p1[1]) + p0[0] * (p1[1] - p2[1]) + p1[0] * (p2[1] - p0[1]);  // :58-61
#pragma unroll
    for (int k = 0; k < 9; k++) face_inv[k] /= den;

    float weight[3];
    float weight_sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {  // :65-69
        weight[k] = face_inv[3 * k + 0] * (float)x + face_inv[3 * k + 1] * (float)y + face_inv[3 * k + 2];
        weight_sum += weight[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) weight[k] = (float)((double)weight[k] / ((double)weight_sum + 1e-5));  // :70

    float tif[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {  // :73-79
        float t = weight[k] * (float)(tsi - 1);
        t = (float)fmax((double)t, 0.);
        t = (float)fmin((double)t, (double)(tsi - 1) - 1e-5);
        tif[k] = t;
    }

    float new_pixel[3] = {0.0f, 0.0f, 0.0f};
    for (int pn = 0; pn < 8; pn++) {  // :82-97
        float w = 1.0f;
        int idx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int ti = f2i(tif[k]);
            if ((pn >> k) % 2 == 0) {
                w *= 1.0f - (tif[k] - (float)ti);
                idx[k] = ti;
            } else {
                w *= tif[k] - (float)ti;
                idx[k] = ti + 1;
            }
        }
        const int isc = idx[0] * tsi * tsi + idx[1] * tsi + idx[2];
#pragma unroll
        for (int k = 0; k < 3; k++) new_pixel[k] += w * texture[isc * 3 + k];
    }
    out[0] = new_pixel[0];
    out[1] = new_pixel[1];
    out[2] = new_pixel[2];
}

// save_obj.py:115-146: pixels one step right of a tile's diagonal copy their left neighbour
__global__ __launch_bounds__(256) void k_texture_atlas_seam(float *__restrict__ image, size_t n, int tso, int tile_width)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int width = tile_width * tso;
    const int x = (int)(i % width);
    const int y = (int)(i / width);
    if ((y % tso + 1) == (x % tso)) {
        const size_t src = (size_t)y * width + (x - 1);  // never itself a seam pixel: no race
#pragma unroll
        for (int k = 0; k < 3; k++) image[i * 3 + k] = image[src * 3 + k];
    }
}

}  // namespace

NR_API int nr_load_textures(const float *image, const float *faces_uv, const int32_t *is_update, float *textures,
                            int32_t num_faces, int32_t texture_size, int32_t image_height, int32_t image_width, void *stream)
{
    if (!image || !faces_uv || !is_update || !textures) return NR_E_NULL;
    if (num_faces < 1 || texture_size < 2 || image_height < 1 || image_width < 1) return NR_E_SIZE;
    const size_t n = (size_t)num_faces * texture_size * texture_size * texture_size;
    if (n > 0x7fffffffull * 64) return NR_E_SIZE;
    hipLaunchKernelGGL(k_bake_textures, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, image, faces_uv,
                       is_update, textures, n, texture_size, image_height, image_width);
    return launch_status();
}

namespace {

// the four sort buffers of the map build, then rocPRIM's own scratch, each 256-byte aligned
constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

int uv_sizes_ok(int32_t num_faces, int32_t texture_size, int32_t num_images, int32_t num_pixels)
{
    if (num_faces < 1 || texture_size < 2 || num_images < 1 || num_pixels < 1) return 0;
    if (num_pixels > 0x7ffffffe) return 0;
    const long long entries = 4ll * num_faces * texture_size * texture_size * texture_size;  // int32 entry numbers
    return entries <= 0x7fffffffll;
}

unsigned key_bits(int32_t num_pixels)  // keys run from 0 to num_pixels (the key of faces without an image)
{
    unsigned bits = 1;
    while (bits < 32 && ((uint64_t)num_pixels >> bits) != 0) bits++;
    return bits;
}

size_t uv_sort_bytes(int32_t n, int32_t num_pixels)
{
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)n, 0u, key_bits(num_pixels), (hipStream_t)0) != hipSuccess)
        return 0;
    return bytes;
}

}  // namespace

NR_API int nr_bake_uv_textures(const float *images, const int32_t *image_table, const float *faces_uv,
                               const int32_t *face_image, const float *base, float *textures, int32_t batch_size,
                               int32_t num_faces, int32_t texture_size, int32_t num_images, int32_t num_pixels, void *stream)
{
    if (!images || !image_table || !faces_uv || !face_image || !base || !textures) return NR_E_NULL;
    if (batch_size < 1 || !uv_sizes_ok(num_faces, texture_size, num_images, num_pixels)) return NR_E_SIZE;
    const size_t n = (size_t)batch_size * num_faces * texture_size * texture_size * texture_size;
    if (n > 0x7fffffffull * 64) return NR_E_SIZE;
    hipLaunchKernelGGL(k_bake_uv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images, image_table,
                       faces_uv, face_image, base, textures, n, num_faces, texture_size, num_images, num_pixels);
    return launch_status();
}

NR_API size_t nr_uv_texture_map_workspace_bytes(int32_t num_faces, int32_t texture_size, int32_t num_images,
                                                int32_t num_pixels)
{
    if (!uv_sizes_ok(num_faces, texture_size, num_images, num_pixels)) return 0;
    const int32_t n = 4 * num_faces * texture_size * texture_size * texture_size;
    const size_t sort = uv_sort_bytes(n, num_pixels);
    if (sort == 0) return 0;
    return 4 * align_up((size_t)n * 4) + align_up(sort);
}

NR_API int nr_uv_texture_map(const int32_t *image_table, const float *faces_uv, const int32_t *face_image, int32_t *row_ptr,
                             int32_t *entry_texel, float *entry_weight, int32_t num_faces, int32_t texture_size,
                             int32_t num_images, int32_t num_pixels, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!image_table || !faces_uv || !face_image || !row_ptr || !entry_texel || !entry_weight) return NR_E_NULL;
    if (!uv_sizes_ok(num_faces, texture_size, num_images, num_pixels)) return NR_E_SIZE;
    const size_t need = nr_uv_texture_map_workspace_bytes(num_faces, texture_size, num_images, num_pixels);
    if (!workspace || need == 0 || workspace_bytes < need) return NR_E_WORKSPACE;
    const int T = texture_size * texture_size * texture_size;
    const int nft = num_faces * T, n = 4 * nft;
    const size_t slot = align_up((size_t)n * 4);
    char *ws = (char *)workspace;
    uint32_t *keys_in = (uint32_t *)ws, *keys_out = (uint32_t *)(ws + slot);
    uint32_t *entries_in = (uint32_t *)(ws + 2 * slot), *entries_out = (uint32_t *)(ws + 3 * slot);
    void *sort_ws = ws + 4 * slot;
    size_t sort_bytes = workspace_bytes - 4 * slot;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_uv_map_keys, dim3((unsigned)((nft + 255) / 256)), dim3(256), 0, st, image_table, faces_uv, face_image,
                       keys_in, entries_in, nft, texture_size, num_images, num_pixels);
    int rc = launch_status();
    if (rc) return rc;
    const hipError_t e = rocprim::radix_sort_pairs(sort_ws, sort_bytes, keys_in, keys_out, entries_in, entries_out, (size_t)n,
                                                   0u, key_bits(num_pixels), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_uv_map_rows, dim3((unsigned)(((size_t)num_pixels + 1 + 255) / 256)), dim3(256), 0, st, keys_out,
                       row_ptr, n, num_pixels);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_uv_map_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, image_table, faces_uv, face_image,
                       keys_out, entries_out, entry_texel, entry_weight, n, texture_size, num_images, num_pixels);
    return launch_status();
}

NR_API int nr_bake_uv_textures_backward(const float *grad_textures, const int32_t *row_ptr, const int32_t *entry_texel,
                                        const float *entry_weight, float *grad_images, int32_t batch_size, int32_t num_faces,
                                        int32_t texture_size, int32_t num_pixels, void *stream)
{
    if (!grad_textures || !row_ptr || !entry_texel || !entry_weight || !grad_images) return NR_E_NULL;
    if (batch_size < 1 || !uv_sizes_ok(num_faces, texture_size, 1, num_pixels)) return NR_E_SIZE;
    const size_t n = (size_t)batch_size * num_pixels;
    if (n > 0x7fffffffull * 64) return NR_E_SIZE;
    const size_t per_image = (size_t)num_faces * texture_size * texture_size * texture_size;
    hipLaunchKernelGGL(k_bake_uv_backward, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_textures,
                       row_ptr, entry_texel, entry_weight, grad_images, n, per_image, num_pixels);
    return launch_status();
}

NR_API int nr_create_texture_image(const float *textures, const float *tile_vertices, float *image, int32_t num_faces,
                                   int32_t texture_size_in, int32_t texture_size_out, int32_t tile_width, int32_t tile_height,
                                   void *stream)
{
    if (!textures || !tile_vertices || !image) return NR_E_NULL;
    if (num_faces < 1 || texture_size_in < 2 || texture_size_out < 2 || tile_width < 1 || tile_height < 1) return NR_E_SIZE;
    if ((long long)tile_width * tile_height < num_faces) return NR_E_SIZE;
    const size_t n = (size_t)tile_width * texture_size_out * (size_t)tile_height * texture_size_out;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_texture_atlas, grid, block, 0, st, image, tile_vertices, textures, n, num_faces, texture_size_in,
                       texture_size_out, tile_width);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_texture_atlas_seam, grid, block, 0, st, image, n, texture_size_out, tile_width);
    return launch_status();
}
