// nr_uv_pixel.hip -- the backward of per-pixel UV texture images (nr_backward_uv_images, include/nr_hip.h; DESIGN K10
// "Per-pixel UV images").  The forward is the UV instantiation of the resolve pass (nr_forward.hip: shade_pixel<true>).
//
//   k_uv_pixel_backward   one thread per pixel: recomputes the forward's reads (uv_locate) and colour (uv_color) and adds
//                         g * light * omega into the double sums of the image pixels it read, g * c into those of its face's
//                         light colour (the lanes of a wave that share a face sum first: one atomic per face and wave)
//   k_uv_pixel_backward<true>  the same pass with a light colour per corner (nr_backward_uv_images_smooth): the image terms
//                         take the pixel's interpolated light, and g * c * e_k goes into the NINE light sums of the face (the
//                         runs of consecutive lanes that share a face are summed in double first: one atomic per run and sum)
//   k_uv_round            the double sums -> grad_images / grad_light, rounded once
//
// The double scratch makes the result independent of how many pixels read one image pixel (1x1 images, heavy magnification):
// float atomics in arrival order lose that bound after a few dozen terms.
#include "nr_device.h"

using namespace nr;

namespace {

// SMOOTH (nr_backward_uv_images_smooth): `light` is [B, F, 3, 3], a colour per corner, and acc_light holds nine sums per face.
template <bool SMOOTH>
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
    float e[3] = {0.0f, 0.0f, 0.0f};  // SMOOTH: the forward's corner weights
    if (fi >= 0) {
        const int b = (int)(i / ((size_t)S * S));
        key = b * F + fi;
        const float g[3] = {grad_rgb_map[3 * i], grad_rgb_map[3 * i + 1], grad_rgb_map[3 * i + 2]};
        UVSample s;
        uv_locate(uv, fi, tex_faces, faces + (size_t)key * 9, weight_map[3 * i], weight_map[3 * i + 1],
                  weight_map[3 * i + 2], depth_map[i], eps, s);
        if (SMOOTH) {
            const float *face = faces + (size_t)key * 9;
            const float w[3] = {weight_map[3 * i], weight_map[3 * i + 1], weight_map[3 * i + 2]};
            const float fz[3] = {face[2], face[5], face[8]};
            corner_weights(fz, w, depth_map[i], e);
        }
        if (acc_light) {
            float c[3];
            uv_color(uv, s, b, c);
#pragma unroll
            for (int k = 0; k < 3; k++) gl[k] = (double)g[k] * (double)c[k];
        }
        if (acc_images && s.m >= 0) {
            const float *lc = light + (size_t)key * 3;
            float lp[3];
            if (SMOOTH) {  // the forward's float32 light of this pixel
                const float *l9 = light + (size_t)key * 9;
#pragma unroll
                for (int k = 0; k < 3; k++) lp[k] = (l9[k] * e[0] + l9[3 + k] * e[1]) + l9[6 + k] * e[2];
                lc = lp;
            }
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
    if (SMOOTH) {
        // Nine sums per face, and at the sizes that matter a wave holds a dozen faces of a few pixels each: one butterfly
        // per distinct face (below) would cost 9 x 6 double shuffles a dozen times over.  The pixels of a wave are
        // consecutive in a row, so the lanes that share a face form runs; a segmented doubling sum adds up every run at once
        // (the scheme of k_corner_backward in nr_vertex_colors.hip -- the per-pixel kernel behind k_corner_gather for faces
        // beyond its 1 024-candidate limit -- here in double: lane l takes lane l + o while that lane lies in its run), and the
        // first lane of each run sends the run's nine sums.  A face has few runs per wave (a wave rarely spans rows).
        if (__ballot(key >= 0) == 0) return;  // (wave-uniform)
        const int lane = threadIdx.x & (WAVE - 1);
        const int prev = __shfl_up(key, 1, WAVE);
        const bool head = lane == 0 || prev != key;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
        const int run_end = above ? lane + __ffsll(above) : WAVE;  // one past the last lane of this lane's run
        double s9[9];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) s9[3 * k + c] = gl[c] * (double)e[k];
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const bool take = lane + o < run_end;
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const double v = __shfl_down(s9[j], o, WAVE);
                if (take) s9[j] += v;
            }
        }
        if (key >= 0 && head) {
#pragma unroll
            for (int j = 0; j < 9; j++)
                if (s9[j] != 0.0) atomicAdd(acc_light + (size_t)key * 9 + j, s9[j]);
        }
        return;
    }
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
        for (int k = 0; k < 3; k++) s3[k] = wave_sum(mine ? gl[k] : 0.0);
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

// light_sums: per face, 3 (a colour) or 9 (a colour per corner)
UVScratch uv_scratch(int B, int F, int P, int image_batch, int light_sums = 3)
{
    UVScratch L;
    L.n_images = (size_t)image_batch * P * 3;
    L.n_light = (size_t)B * F * light_sums;
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

namespace {
// both backwards behind their argument structs: the checks, the zero fill, the pixel pass, the rounding pass
int run_uv_backward(bool smooth, const FaceLight &fl, const UVShade &us, int image_batch, const float *faces,
                    const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                    const float *grad_rgb_map, float *grad_images, int B, int F, int S, double eps, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    if (!faces || !face_index_map || !weight_map || !depth_map || !grad_rgb_map) return NR_E_NULL;
    if (!grad_images && !fl.grad_light) return NR_E_MODE;
    if (int e = check_sizes(B, F, S)) return e;
    const UVScratch L = uv_scratch(B, F, us.P, image_batch, smooth ? 9 : 3);
    if ((size_t)B * S * S > 0xffffff00ull || L.n_images + L.n_light > 0xffffff00ull) return NR_E_SIZE;  // (1-D grids)
    if (!workspace || workspace_bytes < L.total) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *acc = (double *)workspace;
    if (int he = fill_bytes(acc, 0, L.total, st)) return he;  // (nr_device.h: not a memset node)
    const size_t n = (size_t)B * S * S;
    const dim3 grid((unsigned)((n + 255) / 256));
    double *acc_images = grad_images ? acc : nullptr, *acc_light = fl.grad_light ? acc + L.light_off : nullptr;
    if (smooth)
        hipLaunchKernelGGL(k_uv_pixel_backward<true>, grid, dim3(256), 0, st, us, faces, face_index_map, weight_map, depth_map,
                           grad_rgb_map, fl.light, acc_images, acc_light, F, S, fl.tex_faces, eps, n);
    else
        hipLaunchKernelGGL(k_uv_pixel_backward<false>, grid, dim3(256), 0, st, us, faces, face_index_map, weight_map, depth_map,
                           grad_rgb_map, fl.light, acc_images, acc_light, F, S, fl.tex_faces, eps, n);
    if (int rc = launch_status()) return rc;
    const size_t n_img = grad_images ? L.n_images : 0, n_light = fl.grad_light ? L.n_light : 0;
    hipLaunchKernelGGL(k_uv_round, dim3((unsigned)((n_img + n_light + 255) / 256)), dim3(256), 0, st, acc, grad_images,
                       n_img, L.light_off, fl.grad_light, n_light);
    return launch_status();
}
}  // namespace

NR_API int nr_backward_uv_images(const nr_face_light *lit, const nr_uv_images *uv, const float *faces,
                                 const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                 const float *grad_rgb_map, float *grad_images, int32_t B, int32_t F, int32_t S,
                                 double eps, void *workspace, size_t workspace_bytes, void *stream)
{
    FaceLight fl;
    UVShade us;
    if (int e = uv_images_args(lit, uv, B, F, fl, us)) return e;
    return run_uv_backward(false, fl, us, uv->image_batch, faces, face_index_map, weight_map, depth_map, grad_rgb_map,
                           grad_images, B, F, S, eps, workspace, workspace_bytes, stream);
}

NR_API size_t nr_backward_uv_images_smooth_workspace_bytes(int32_t B, int32_t F, int32_t num_pixels, int32_t image_batch)
{
    if (check_sizes(B, F, 1) || num_pixels < 1 || num_pixels > 0x7ffffffe || (image_batch != 1 && image_batch != B))
        return 0;
    return uv_scratch(B, F, num_pixels, image_batch, 9).total;
}

NR_API int nr_backward_uv_images_smooth(const nr_corner_light *lit, const nr_uv_images *uv, const float *faces,
                                        const int32_t *face_index_map, const float *weight_map, const float *depth_map,
                                        const float *grad_rgb_map, float *grad_images, int32_t B, int32_t F, int32_t S,
                                        double eps, void *workspace, size_t workspace_bytes, void *stream)
{
    FaceLight fl;
    UVShade us;
    if (int e = uv_smooth_args(lit, uv, B, F, fl, us)) return e;
    return run_uv_backward(true, fl, us, uv->image_batch, faces, face_index_map, weight_map, depth_map, grad_rgb_map,
                           grad_images, B, F, S, eps, workspace, workspace_bytes, stream);
}
