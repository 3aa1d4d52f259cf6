// nr_uv_pixel.hip -- the backward of per-pixel UV texture images (nr_backward_uv_images, include/nr_hip.h; DESIGN K10
// "Per-pixel UV images").  The forward is the UV instantiation of the resolve pass (nr_forward.hip: shade_pixel<true>).
//
//   k_uv_pixel_backward   one thread per pixel: recomputes the forward's reads (uv_locate) and colour (uv_color) and adds
//                         g * light * omega into the double sums of the image pixels it read, g * c into those of its face's
//                         light colour (the lanes of a wave that share a face sum first: one atomic per face and wave)
//   k_uv_round            the double sums -> grad_images / grad_light, rounded once
//
// The double scratch makes the result independent of how many pixels read one image pixel (1x1 images, heavy magnification):
// float atomics in arrival order lose that bound after a few dozen terms.
#include "nr_device.h"

using namespace nr;

namespace {

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

__global__ __launch_bounds__(256) void k_uv_pixel_backward(UVShade uv, const float *__restrict__ faces,
                                                           const int32_t *__restrict__ face_index_map,
                                                           const float *__restrict__ weight_map,
                                                           const float *__restrict__ depth_map,
                                                           const float *__restrict__ grad_rgb_map,
                                                           const float *__restrict__ light, double *__restrict__ acc_images,
                                                           double *__restrict__ acc_light, int F, int S, int tex_faces,
                                                           double eps, size_t n_pixels)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int fi = i < n_pixels ? face_index_map[i] : -1;
    int key = -1;  // b * F + fi of a covered pixel
    double gl[3] = {0.0, 0.0, 0.0};
    if (fi >= 0) {
        const int b = (int)(i / ((size_t)S * S));
        key = b * F + fi;
        const float g[3] = {grad_rgb_map[3 * i], grad_rgb_map[3 * i + 1], grad_rgb_map[3 * i + 2]};
        UVSample s;
        uv_locate(uv, fi, tex_faces, faces + (size_t)key * 9, weight_map[3 * i], weight_map[3 * i + 1],
                  weight_map[3 * i + 2], depth_map[i], eps, s);
        if (acc_light) {
            float c[3];
            uv_color(uv, s, b, c);
#pragma unroll
            for (int k = 0; k < 3; k++) gl[k] = (double)g[k] * (double)c[k];
        }
        if (acc_images && s.m >= 0) {
            const float *lc = light + (size_t)key * 3;
            const double gk[3] = {(double)g[0] * (double)lc[0], (double)g[1] * (double)lc[1], (double)g[2] * (double)lc[2]};
            double *a = acc_images + (uv.shared ? 0 : (size_t)b * uv.P * 3);
            // (the reads of neighbouring lanes are neighbouring image pixels: the atomics of a wave hit few cache lines)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                double *q = a + (size_t)s.q[r] * 3;
                const double w = (double)s.w[r];
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (gk[k] != 0.0 && w != 0.0) atomicAdd(q + k, gk[k] * w);
            }
        }
    }
    if (!acc_light) return;
    // The light sums: the lanes of the wave that share the leader's face add up first, the leader sends one atomic per
    // channel -- a large face otherwise sends thousands of atomics to one address.  (Uniform loop: one trip per distinct face
    // among the wave's covered pixels.)
    unsigned long long pending = __ballot(key >= 0);
    while (pending) {
        const int leader = __ffsll(pending) - 1;
        const int k0 = bcast_i(key, leader);
        const bool mine = key == k0;
        double s3[3];
#pragma unroll
        for (int k = 0; k < 3; k++) s3[k] = wave_sum_d(mine ? gl[k] : 0.0);
        if ((int)(threadIdx.x & (WAVE - 1)) == leader) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (s3[k] != 0.0) atomicAdd(acc_light + (size_t)k0 * 3 + k, s3[k]);
        }
        pending &= ~__ballot(mine);
    }
}

// [0, n_images): grad_images, [n_images, n_images + n_light): grad_light -- each double sum rounded once
__global__ __launch_bounds__(256) void k_uv_round(const double *__restrict__ acc, float *__restrict__ grad_images,
                                                  size_t n_images, size_t light_off, float *__restrict__ grad_light,
                                                  size_t n_light)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_images) {
        grad_images[i] = (float)acc[i];
    } else if (i - n_images < n_light) {
        grad_light[i - n_images] = (float)acc[light_off + i - n_images];
    }
}

struct UVScratch {
    size_t n_images, n_light, light_off, total;  // elements, elements, element offset, bytes
};

UVScratch uv_scratch(int B, int F, int P, int image_batch)
{
    UVScratch L;
    L.n_images = (size_t)image_batch * P * 3;
    L.n_light = (size_t)B * F * 3;
    L.light_off = align_up(L.n_images, 32);  // 256-byte aligned
    L.total = (L.light_off + L.n_light) * sizeof(double);
    return L;
}

}  // namespace

NR_API size_t nr_backward_uv_images_workspace_bytes(int32_t B, int32_t F, int32_t num_pixels, int32_t image_batch)
{
    if (check_sizes(B, F, 1) || num_pixels < 1 || num_pixels > 0x7ffffffe || (image_batch != 1 && image_batch != B))
        return 0;
    return uv_scratch(B, F, num_pixels, image_batch).total;
}

NR_API int nr_backward_uv_images(const nr_face_light *lit, const nr_uv_images *uv, const float *faces,
                                 const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                 const float *grad_rgb_map, float *grad_images, int32_t B, int32_t F, int32_t S,
                                 double eps, void *workspace, size_t workspace_bytes, void *stream)
{
    FaceLight fl;
    UVShade us;
    if (int e = uv_images_args(lit, uv, B, F, fl, us)) return e;
    if (!faces || !face_index_map || !weight_map || !depth_map || !grad_rgb_map) return NR_E_NULL;
    if (!grad_images && !fl.grad_light) return NR_E_MODE;
    if (int e = check_sizes(B, F, S)) return e;
    const UVScratch L = uv_scratch(B, F, us.P, uv->image_batch);
    if ((size_t)B * S * S > 0xffffff00ull || L.n_images + L.n_light > 0xffffff00ull) return NR_E_SIZE;  // (1-D grids)
    if (!workspace || workspace_bytes < L.total) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *acc = (double *)workspace;
    if (int he = fill_bytes(acc, 0, L.total, st)) return he;  // (nr_device.h: not a memset node)
    const size_t n = (size_t)B * S * S;
    hipLaunchKernelGGL(k_uv_pixel_backward, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, us, faces, face_index_map,
                       weight_map, depth_map, grad_rgb_map, fl.light, grad_images ? acc : nullptr,
                       fl.grad_light ? acc + L.light_off : nullptr, F, S, fl.tex_faces, eps, n);
    if (int rc = launch_status()) return rc;
    const size_t n_img = grad_images ? L.n_images : 0, n_light = fl.grad_light ? L.n_light : 0;
    hipLaunchKernelGGL(k_uv_round, dim3((unsigned)((n_img + n_light + 255) / 256)), dim3(256), 0, st, acc, grad_images,
                       n_img, L.light_off, fl.grad_light, n_light);
    return launch_status();
}
