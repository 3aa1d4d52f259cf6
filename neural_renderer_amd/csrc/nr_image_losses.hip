// nr_image_losses.hip -- the objective of a mesh fit on images (include/nr_hip.h; DESIGN "Image losses"): the silhouette
// IoU loss on alpha [B, H, W] and the masked squared error on images [B, C, H, W], both on an image pyramid of 1 .. 5
// levels, level l the 2 x 2 mean of level l - 1.
//
// The tile-to-workgroup map.  An image is cut into tiles of 64 x 16 pixels (TW x TH), row-major; workgroup (tile, image) of
// 256 threads owns one tile, thread (tx, ty) = (tid % 16, tid / 16) the four pixels x0 + 4 tx .. + 3 of row y0 + ty -- one
// 16-byte load when W is a multiple of 4 and the pointers are 16-byte aligned (VEC), four guarded loads otherwise.  H and W
// are multiples of 2^(levels - 1) and so are TW and TH: every block of every level lies inside one tile, and a tile that
// hangs over the image's edge is cut along block borders.  Pixels outside read as 0 and add exactly 0 to every sum.  The
// levels of a tile are formed in LDS: level 0 [16][64] from the registers, level l [16 >> l][64 >> l] by the first
// 1024 >> 2 l threads, one value each.
//   k_iou_forward / k_se_forward   (tile, image): every level's sums of the tile in double, reduced over the workgroup in the
//                                  fixed order of nr_reduce.h (block_sums), one partial per (image, tile, sum)
//   k_iou_finish / k_se_finish     (image): the tiles' partials in tile order (ordered_sum), the loss evaluated in double
//                                  and rounded once; the IoU's I_l, U_l are left as doubles for the backward
//   k_iou_backward / k_se_backward (tile, image): elementwise over the tile.  The IoU reads the target and the saved sums, not
//                                  alpha; the squared error recomputes its differences
// No atomics in any kernel: the same bits in every run, and an image alone gives the bits it has inside a batch.
//
// The float operation order (no contraction, correctly rounded division: _build.HIPCC_FLAGS).
//   P_l(z) at a block = (((p00 + p01) + p10) + p11) * 0.25f in float32 from level l - 1, upper row first (as nr_image.hip).
//   IoU, per level element (a, t): in double, p = a t (exact), I += p, U += (a + t) - p.  A thread adds its four level-0
//     pixels left to right, then its element of level 1, 2, ... into sums of their own.
//     finish: Ue_l = U_l + eps; loss = 0; loss += w_l (1 - I_l / Ue_l) for l ascending; (float)loss.
//     backward, in double: k_l = -((g_b w_l) 4^-l) / (Ue_l Ue_l);  s = 0;  s += k_l (t_l Ue_l - I_l (1 - t_l)) for l ascending
//     with t_l the float32 pyramid of the target;  grad = (float)s.
//   Squared error: e = x - t, d = m e (float32; without a mask d = e), d_l = P_l(d); per level element S_l += (double)d_l d_l,
//     the channels one after the other into the same sums.  finish: loss += w_l S_l for l ascending; (float)loss.
//     backward, in double: k_l = ((2 g_b) w_l) 4^-l;  s = 0;  s += k_l d_l for l ascending;  grad = (float)(m s).
#include "nr_device.h"

using namespace nr;

namespace {

constexpr int BLOCK = 256;
constexpr int TW = 64, TH = 16;   // a tile; BLOCK threads of four pixels each
constexpr int MAXL = 5;           // levels: TW and TH are multiples of 2^(MAXL - 1)
constexpr int PYR = 1364;         // floats of a tile's pyramid: 1024 + 256 + 64 + 16 + 4

struct LevelWeights {
    double w[MAXL];
};

// where level l of a tile's pyramid starts: 0, 1024, 1280, 1344, 1360
__device__ __forceinline__ constexpr int level_offset(int l) { return (4096 - (4096 >> (2 * l))) / 3; }
__device__ __forceinline__ constexpr int level_count(int l) { return (TW * TH) >> (2 * l); }

struct Pixel4 {
    int x, y;      // the thread's first pixel
    int tx4, ty;   // ... inside the tile
};

__device__ __forceinline__ Pixel4 my_pixels(int tiles_x)
{
    const int tile = blockIdx.x, row = tile / tiles_x, col = tile - row * tiles_x;
    Pixel4 p;
    p.tx4 = 4 * (threadIdx.x & 15);
    p.ty = threadIdx.x >> 4;
    p.x = col * TW + p.tx4;
    p.y = row * TH + p.ty;
    return p;
}

// the thread's four pixels of an [H, W] plane; 0 outside
template <bool VEC>
__device__ __forceinline__ void load4(const float *__restrict__ plane, int H, int W, const Pixel4 &p, float v[4])
{
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (p.y >= H || p.x >= W) return;
    const float *src = plane + (size_t)p.y * W + p.x;
    if (VEC) {  // W % 4 == 0 and p.x % 4 == 0: all four inside
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p.x + j < W) v[j] = src[j];
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ plane, int H, int W, const Pixel4 &p, const float v[4])
{
    if (p.y >= H || p.x >= W) return;
    float *dst = plane + (size_t)p.y * W + p.x;
    if (VEC) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p.x + j < W) dst[j] = v[j];
    }
}

__device__ __forceinline__ void put_level0(float *__restrict__ s, const Pixel4 &p, const float v[4])
{
    *reinterpret_cast<float4 *>(s + p.ty * TW + p.tx4) = make_float4(v[0], v[1], v[2], v[3]);
}

// element e of level l >= 1 from level l - 1 of the pyramid s
__device__ __forceinline__ float pool(const float *__restrict__ s, int l, int e)
{
    const int wl = TW >> l, ly = e / wl, lx = e - ly * wl;
    const float *q = s + level_offset(l - 1) + (2 * ly) * (2 * wl) + 2 * lx;
    return (((q[0] + q[1]) + q[2 * wl]) + q[2 * wl + 1]) * 0.25f;
}

// level l's value at pixel (tx, ty) of the tile
__device__ __forceinline__ float level_at(const float *__restrict__ s, int l, int tx, int ty)
{
    return s[level_offset(l) + (ty >> l) * (TW >> l) + (tx >> l)];
}

// --------------------------------------------------------------------------------------------------------------------
// IoU

__device__ __forceinline__ void iou_add(double &I, double &U, float a, float t)
{
    const double da = (double)a, dt = (double)t, p = da * dt;
    I += p;
    U += (da + dt) - p;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_iou_forward(const float *__restrict__ alpha, const float *__restrict__ target,
                                                       size_t target_stride, double *__restrict__ partial, int H, int W,
                                                       int tiles_x, int levels)
{
    __shared__ __align__(16) float sa[PYR], st[PYR];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Pixel4 p = my_pixels(tiles_x);
    float a[4], t[4];
    load4<VEC>(alpha + (size_t)b * H * W, H, W, p, a);
    load4<VEC>(target + (size_t)b * target_stride, H, W, p, t);
    double acc[2 * MAXL];
#pragma unroll
    for (int k = 0; k < 2 * MAXL; k++) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) iou_add(acc[0], acc[1], a[j], t[j]);
    if (levels > 1) {
        put_level0(sa, p, a);
        put_level0(st, p, t);
    }
#pragma unroll
    for (int l = 1; l < MAXL; l++) {
        if (l < levels) {
            __syncthreads();
            if (tid < level_count(l)) {
                const float va = pool(sa, l, tid), vt = pool(st, l, tid);
                sa[level_offset(l) + tid] = va;
                st[level_offset(l) + tid] = vt;
                iou_add(acc[2 * l], acc[2 * l + 1], va, vt);
            }
        }
    }
    const int n = 2 * levels;
    const double sum = block_sums<BLOCK>(acc, n);
    if (tid < n) partial[((size_t)b * gridDim.x + blockIdx.x) * n + tid] = sum;
}

// partial [B, n_tiles, 2 levels] -> loss [B], sums [B, 2 levels] (or NULL)
__global__ __launch_bounds__(BLOCK) void k_iou_finish(const double *__restrict__ partial, float *__restrict__ loss,
                                                      double *__restrict__ sums, LevelWeights lw, double eps, int B,
                                                      int n_tiles, int levels)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = 2 * levels;
    const double *p = partial + (size_t)b * n_tiles * n;
    double total = 0.0;
#pragma unroll
    for (int l = 0; l < MAXL; l++) {
        if (l < levels) {
            const double I = ordered_sum(p + 2 * l, n_tiles, n), U = ordered_sum(p + 2 * l + 1, n_tiles, n);
            total += lw.w[l] * (1.0 - I / (U + eps));
            if (sums) {
                sums[(size_t)b * n + 2 * l] = I;
                sums[(size_t)b * n + 2 * l + 1] = U;
            }
        }
    }
    loss[b] = (float)total;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_iou_backward(const float *__restrict__ target, size_t target_stride,
                                                        const double *__restrict__ sums,
                                                        const float *__restrict__ grad_loss, float *__restrict__ grad_alpha,
                                                        LevelWeights lw, double eps, int H, int W, int tiles_x, int levels)
{
    __shared__ __align__(16) float st[PYR];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Pixel4 p = my_pixels(tiles_x);
    float t[4];
    load4<VEC>(target + (size_t)b * target_stride, H, W, p, t);
    if (levels > 1) put_level0(st, p, t);
#pragma unroll
    for (int l = 1; l < MAXL; l++) {
        if (l < levels) {
            __syncthreads();
            if (tid < level_count(l)) st[level_offset(l) + tid] = pool(st, l, tid);
        }
    }
    if (levels > 1) __syncthreads();
    const double g = (double)grad_loss[b];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int l = 0; l < MAXL; l++) {
        if (l < levels) {
            const double I = sums[(size_t)b * 2 * levels + 2 * l], Ue = sums[(size_t)b * 2 * levels + 2 * l + 1] + eps;
            const double k = -((g * lw.w[l]) * (1.0 / (double)(1 << (2 * l)))) / (Ue * Ue);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double tl = (double)(l == 0 ? t[j] : level_at(st, l, p.tx4 + j, p.ty));
                s[j] += k * (tl * Ue - I * (1.0 - tl));
            }
        }
    }
    const float out[4] = {(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
    store4<VEC>(grad_alpha + (size_t)b * H * W, H, W, p, out);
}

// --------------------------------------------------------------------------------------------------------------------
// squared error

// d = m (x - t) of the thread's four pixels of channel c (mask NULL: d = x - t)
template <bool VEC>
__device__ __forceinline__ void masked_difference(const float *__restrict__ images, const float *__restrict__ target,
                                                  const float m[4], bool masked, int H, int W, const Pixel4 &p, float d[4])
{
    float x[4], t[4];
    load4<VEC>(images, H, W, p, x);
    load4<VEC>(target, H, W, p, t);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float e = x[j] - t[j];
        d[j] = masked ? m[j] * e : e;
    }
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_se_forward(const float *__restrict__ images, const float *__restrict__ target,
                                                      size_t target_stride, const float *__restrict__ mask, size_t mask_stride,
                                                      double *__restrict__ partial, int C, int H, int W, int tiles_x,
                                                      int levels)
{
    __shared__ __align__(16) float sd[PYR];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Pixel4 p = my_pixels(tiles_x);
    const size_t plane = (size_t)H * W;
    float m[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (mask) load4<VEC>(mask + (size_t)b * mask_stride, H, W, p, m);
    double acc[MAXL];
#pragma unroll
    for (int k = 0; k < MAXL; k++) acc[k] = 0.0;
    for (int c = 0; c < C; c++) {
        float d[4];
        masked_difference<VEC>(images + ((size_t)b * C + c) * plane, target + (size_t)b * target_stride + (size_t)c * plane, m,
                               mask != nullptr, H, W, p, d);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[0] += (double)d[j] * (double)d[j];
        if (levels > 1) {
            if (c > 0) __syncthreads();  // the previous channel's pyramid has been read
            put_level0(sd, p, d);
        }
#pragma unroll
        for (int l = 1; l < MAXL; l++) {
            if (l < levels) {
                __syncthreads();
                if (tid < level_count(l)) {
                    const float v = pool(sd, l, tid);
                    sd[level_offset(l) + tid] = v;
                    acc[l] += (double)v * (double)v;
                }
            }
        }
    }
    const double sum = block_sums<BLOCK>(acc, levels);
    if (tid < levels) partial[((size_t)b * gridDim.x + blockIdx.x) * levels + tid] = sum;
}

// partial [B, n_tiles, levels] -> loss [B]
__global__ __launch_bounds__(BLOCK) void k_se_finish(const double *__restrict__ partial, float *__restrict__ loss,
                                                     LevelWeights lw, int B, int n_tiles, int levels)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *p = partial + (size_t)b * n_tiles * levels;
    double total = 0.0;
#pragma unroll
    for (int l = 0; l < MAXL; l++) {
        if (l < levels) {
            total += lw.w[l] * ordered_sum(p + l, n_tiles, levels);
        }
    }
    loss[b] = (float)total;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_se_backward(const float *__restrict__ images, const float *__restrict__ target,
                                                       size_t target_stride, const float *__restrict__ mask,
                                                       size_t mask_stride, const float *__restrict__ grad_loss,
                                                       float *__restrict__ grad_images, LevelWeights lw, int C, int H, int W,
                                                       int tiles_x, int levels)
{
    __shared__ __align__(16) float sd[PYR];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Pixel4 p = my_pixels(tiles_x);
    const size_t plane = (size_t)H * W;
    float m[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (mask) load4<VEC>(mask + (size_t)b * mask_stride, H, W, p, m);
    const double g2 = 2.0 * (double)grad_loss[b];
    double k[MAXL];
#pragma unroll
    for (int l = 0; l < MAXL; l++) k[l] = l < levels ? (g2 * lw.w[l]) * (1.0 / (double)(1 << (2 * l))) : 0.0;
    for (int c = 0; c < C; c++) {
        float d[4];
        masked_difference<VEC>(images + ((size_t)b * C + c) * plane, target + (size_t)b * target_stride + (size_t)c * plane, m,
                               mask != nullptr, H, W, p, d);
        if (levels > 1) {
            if (c > 0) __syncthreads();
            put_level0(sd, p, d);
        }
#pragma unroll
        for (int l = 1; l < MAXL; l++) {
            if (l < levels) {
                __syncthreads();
                if (tid < level_count(l)) sd[level_offset(l) + tid] = pool(sd, l, tid);
            }
        }
        if (levels > 1) __syncthreads();
        float out[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < MAXL; l++)
                if (l < levels) s += k[l] * (double)(l == 0 ? d[j] : level_at(sd, l, p.tx4 + j, p.ty));
            out[j] = (float)(mask ? (double)m[j] * s : s);
        }
        store4<VEC>(grad_images + ((size_t)b * C + c) * plane, H, W, p, out);
    }
}

// --------------------------------------------------------------------------------------------------------------------
// host

inline int tiles_x_of(int W) { return (W + TW - 1) / TW; }
inline int n_tiles_of(int H, int W) { return tiles_x_of(W) * ((H + TH - 1) / TH); }

// B images of C planes [H, W] on `levels` levels
int loss_sizes(int B, int C, int H, int W, int levels)
{
    if (B < 1 || B > 65535 || C < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || levels < 1 || levels > MAXL) return NR_E_SIZE;
    const int step = 1 << (levels - 1);
    if (H % step || W % step) return NR_E_SIZE;
    if ((size_t)C * (size_t)H * (size_t)W > 0x7fffffffull) return NR_E_SIZE;
    return 0;
}

size_t partial_bytes(int B, int H, int W, int levels) { return (size_t)B * n_tiles_of(H, W) * 2 * levels * sizeof(double); }

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

LevelWeights weights_of(const double *level_weights, int levels)
{
    LevelWeights lw;
    for (int l = 0; l < MAXL; l++) lw.w[l] = l < levels ? level_weights[l] : 0.0;
    return lw;
}

inline dim3 finish_grid(int B) { return dim3((unsigned)((B + BLOCK - 1) / BLOCK)); }

}  // namespace

NR_API size_t nr_image_loss_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t levels)
{
    if (loss_sizes(B, 1, H, W, levels)) return 0;
    return partial_bytes(B, H, W, levels);
}

NR_API int nr_iou_loss_forward(const float *alpha, const float *target, int32_t target_per_image, const double *level_weights,
                               float *loss, double *sums, int32_t B, int32_t H, int32_t W, int32_t levels, double eps,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (!alpha || !target || !level_weights || !loss) return NR_E_NULL;
    if (int e = loss_sizes(B, 1, H, W, levels)) return e;
    if (!workspace || workspace_bytes < partial_bytes(B, H, W, levels)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const LevelWeights lw = weights_of(level_weights, levels);
    const size_t ts = target_per_image ? (size_t)H * W : 0;
    const int nt = n_tiles_of(H, W);
    const dim3 grid((unsigned)nt, (unsigned)B), block(BLOCK);
    if (W % 4 == 0 && aligned16(alpha) && aligned16(target))
        hipLaunchKernelGGL(k_iou_forward<true>, grid, block, 0, st, alpha, target, ts, partial, H, W, tiles_x_of(W), levels);
    else
        hipLaunchKernelGGL(k_iou_forward<false>, grid, block, 0, st, alpha, target, ts, partial, H, W, tiles_x_of(W), levels);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_iou_finish, finish_grid(B), block, 0, st, partial, loss, sums, lw, eps, B, nt, levels);
    return launch_status();
}

NR_API int nr_iou_loss_backward(const float *target, int32_t target_per_image, const double *sums, const double *level_weights,
                                const float *grad_loss, float *grad_alpha, int32_t B, int32_t H, int32_t W, int32_t levels,
                                double eps, void *stream)
{
    if (!target || !sums || !level_weights || !grad_loss || !grad_alpha) return NR_E_NULL;
    if (int e = loss_sizes(B, 1, H, W, levels)) return e;
    const LevelWeights lw = weights_of(level_weights, levels);
    const size_t ts = target_per_image ? (size_t)H * W : 0;
    const dim3 grid((unsigned)n_tiles_of(H, W), (unsigned)B), block(BLOCK);
    if (W % 4 == 0 && aligned16(target) && aligned16(grad_alpha))
        hipLaunchKernelGGL(k_iou_backward<true>, grid, block, 0, (hipStream_t)stream, target, ts, sums, grad_loss, grad_alpha, lw,
                           eps, H, W, tiles_x_of(W), levels);
    else
        hipLaunchKernelGGL(k_iou_backward<false>, grid, block, 0, (hipStream_t)stream, target, ts, sums, grad_loss, grad_alpha, lw,
                           eps, H, W, tiles_x_of(W), levels);
    return launch_status();
}

NR_API int nr_squared_error_forward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                                    int32_t mask_per_image, const double *level_weights, float *loss, int32_t B, int32_t C,
                                    int32_t H, int32_t W, int32_t levels, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!images || !target || !level_weights || !loss) return NR_E_NULL;
    if (int e = loss_sizes(B, C, H, W, levels)) return e;
    if (!workspace || workspace_bytes < partial_bytes(B, H, W, levels)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const LevelWeights lw = weights_of(level_weights, levels);
    const size_t ts = target_per_image ? (size_t)C * H * W : 0, ms = mask_per_image ? (size_t)H * W : 0;
    const int nt = n_tiles_of(H, W);
    const dim3 grid((unsigned)nt, (unsigned)B), block(BLOCK);
    if (W % 4 == 0 && aligned16(images) && aligned16(target) && aligned16(mask))
        hipLaunchKernelGGL(k_se_forward<true>, grid, block, 0, st, images, target, ts, mask, ms, partial, C, H, W, tiles_x_of(W),
                           levels);
    else
        hipLaunchKernelGGL(k_se_forward<false>, grid, block, 0, st, images, target, ts, mask, ms, partial, C, H, W, tiles_x_of(W),
                           levels);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_se_finish, finish_grid(B), block, 0, st, partial, loss, lw, B, nt, levels);
    return launch_status();
}

NR_API int nr_squared_error_backward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                                     int32_t mask_per_image, const double *level_weights, const float *grad_loss,
                                     float *grad_images, int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, void *stream)
{
    if (!images || !target || !level_weights || !grad_loss || !grad_images) return NR_E_NULL;
    if (int e = loss_sizes(B, C, H, W, levels)) return e;
    const LevelWeights lw = weights_of(level_weights, levels);
    const size_t ts = target_per_image ? (size_t)C * H * W : 0, ms = mask_per_image ? (size_t)H * W : 0;
    const dim3 grid((unsigned)n_tiles_of(H, W), (unsigned)B), block(BLOCK);
    if (W % 4 == 0 && aligned16(images) && aligned16(target) && aligned16(mask) && aligned16(grad_images))
        hipLaunchKernelGGL(k_se_backward<true>, grid, block, 0, (hipStream_t)stream, images, target, ts, mask, ms, grad_loss,
                           grad_images, lw, C, H, W, tiles_x_of(W), levels);
    else
        hipLaunchKernelGGL(k_se_backward<false>, grid, block, 0, (hipStream_t)stream, images, target, ts, mask, ms, grad_loss,
                           grad_images, lw, C, H, W, tiles_x_of(W), levels);
    return launch_status();
}
