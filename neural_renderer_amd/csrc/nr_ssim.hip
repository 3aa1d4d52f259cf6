// nr_ssim.hip -- the structural similarity of two images as a loss (include/nr_hip.h; DESIGN "Image losses: SSIM"): per
// channel and window centre q
//   mu_x = G*x, mu_y = G*y, sxx = G*(x x) - mu_x^2, syy = G*(y y) - mu_y^2, sxy = G*(x y) - mu_x mu_y,
//   S = (2 mu_x mu_y + C1)(2 sxy + C2) / ((mu_x^2 + mu_y^2 + C1)(sxx + syy + C2)),   loss_b = k sum_{c,q} m_b(q) (1 - S_c(q))
// with G the separable window w (x) w of n = 2 R + 1 taps, n odd in 3 .. 11.  'same': z reads as 0 outside the image and every
// pixel is a window centre; 'valid': only the windows inside the image, (H - 2R) x (W - 2R) centres.  Below, the MAP is the
// grid of window centres [Hq, Wq] and off = 0 ('same') or R ('valid'): centre q of the map is pixel q + off of the image.
//
// The tile-to-workgroup map.  The forward cuts the map, the backward the image, into tiles of 64 x 16 (TW x TH), row-major;
// workgroup (tile, image) of 256 threads owns one tile and walks the channels one after the other; thread (tx, ty) =
// (tid % 16, tid / 16) owns the four elements x0 + 4 tx .. + 3 of row y0 + ty.  Per channel:
//   stage     the tile plus a halo of R on every side, (TH + 2R) rows of 64 + 2R floats at a pitch of PITCH = 64 + 2R rounded
//             up to 4, one LDS plane per input, 0 outside the source: 16-byte loads over the 16-byte cells that cover the rows
//             when the source's width is a multiple of 4 and its pointer is 16-byte aligned, guarded scalar loads otherwise
//             (the same values either way);
//   rows      item (row, s), s in 0 .. 15, of the (TH + 2R) x 16 items: 16-byte LDS reads of the staged floats
//             4 s .. 4 s + 4 + 2R of the row, the products, and the horizontal filter of every plane at the four columns
//             4 s .. 4 s + 3, left as one float4 per plane in LDS planes [TH + 2R][64];
//   columns   thread (tx, ty): the vertical filter over rows ty .. ty + 2R of those planes at its four columns (16-byte
//             LDS reads; at a pitch of 64 floats the 16 lanes of a read's group cover the 64 banks once), then the pixel
//             arithmetic in registers.
//   k_ssim_forward  (tile of the map, image): planes x, y; filters mu_x, mu_y, G*(xx), G*(yy), G*(xy); S and, when a gradient
//                   can follow, M1, M2, M3 (below) as three float maps; the tile's sums of m (1 - S) and of m in double --
//                   the thread's own order (channel by channel, its four pixels left to right), then the workgroup in the
//                   fixed order of nr_reduce.h (block_sums) --, one partial per (image, tile, sum)
//   k_ssim_finish   (image): the tiles' partials in tile order (ordered_sum), k and the loss evaluated in double, the loss
//                   rounded once; k left as a double for the backward
//   k_ssim_backward (tile of the image, image): planes M1, M2, M3 and the mask over the map; a gather -- the thread sums
//                   over the windows q that contain its pixels p --: F_i = sum_q w(q - p) m(q) M_i(q), then
//                   grad(p) = -(g_b k_b) (F_1 + 2 x(p) F_2 + y(p) F_3)
// No atomics in any kernel: the same bits in every run, and an image alone gives the bits it has inside a batch.
//
// The float operation order (float32; no contraction, correctly rounded division: _build.HIPCC_FLAGS; the filters' fused
// multiply-adds are written out as fmaf).
//   a filter of z with taps w: acc = w_0 z_0 (one rounding; the columns: acc = fmaf(w_0, z_0, 0), the same value), then
//     acc = fmaf(w_k, z_k, acc) for k ascending; rows first (k = column), then columns (k = row).  The products x x, y y,
//     x y are rounded once each before their filter.  The backward filters m(q) M_i(q) (one rounding; without a mask M_i
//     itself) with the taps reversed, w(q - p) = w[R - (q - p)].
//   pxx = mu_x mu_x, pyy = mu_y mu_y, pxy = mu_x mu_y;  sxx = G*(xx) - pxx, syy = G*(yy) - pyy, sxy = G*(xy) - pxy;
//   a1 = (pxy + pxy) + C1, b1 = (pxx + pyy) + C1, a2 = (sxy + sxy) + C2, b2 = (sxx + syy) + C2   (C1, C2 rounded to float32),
//   num = a1 a2, den = b1 b2, S = num / den.  Bit-equal x and y give bit-equal sums in numerator and denominator: S = 1
//     and a loss of exactly 0.
//   M3 = (a1 + a1) / den,  M2 = -(S / b2),
//   M1 = ((((mu_y + mu_y) a2) / den - ((mu_x + mu_x) S) / b1) - (mu_x + mu_x) M2) - mu_y M3.
//   sums: per pixel in double, loss += (double)m (1.0 - (double)S), mask += (double)m (no mask: m = 1).
//   finish: 'sum' k = 1; 'mean' k = 1 / ((double)C mask) when mask != 0, else 0; loss = (float)(k loss).
//   backward, in double: coef = -((double)g_b k_b);  s = ((double)F1 + (2.0 (double)x) (double)F2) + (double)y (double)F3;
//     grad = (float)(coef s).
#include "nr_device.h"

using namespace nr;

namespace {

constexpr int BLOCK = 256;
constexpr int TW = 64, TH = 16;  // a tile; BLOCK threads of four elements each
constexpr int MAXN = 11;         // taps

struct Window {
    float w[MAXN];
};

__host__ __device__ constexpr int pitch_of(int R) { return (TW + 2 * R + 3) / 4 * 4; }
__host__ __device__ constexpr int rows_of(int R) { return TH + 2 * R; }

// `rows` x (TW + 2R) floats of the plane src [Hs, Ws] from (oy, ox) (which may lie outside: 0 there) into dst at `pitch`.
// vec: Ws % 4 == 0 and src 16-byte aligned -- 16-byte loads over the aligned cells that cover a row.
__device__ __forceinline__ void stage_plane(float *__restrict__ dst, const float *__restrict__ src, int Hs, int Ws, int oy, int ox,
                                            int rows, int cols, int pitch, bool vec)
{
    if (vec) {
        const int a0 = ox & ~3;                         // (two's complement: rounds down for negative ox too)
        const int cells = (ox + cols - a0 + 3) >> 2;    // 16-byte cells of a row
        for (int i = threadIdx.x; i < rows * cells; i += BLOCK) {
            const int r = i / cells, j = i - r * cells;
            const int y = oy + r, x = a0 + 4 * j;
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (y >= 0 && y < Hs && x >= 0 && x < Ws) q = *reinterpret_cast<const float4 *>(src + (size_t)y * Ws + x);
            const float v[4] = {q.x, q.y, q.z, q.w};
            float *d = dst + r * pitch + (x - ox);
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (x - ox + e >= 0 && x - ox + e < cols) d[e] = v[e];
        }
    } else {
        for (int i = threadIdx.x; i < rows * cols; i += BLOCK) {
            const int r = i / cols, c = i - r * cols;
            const int y = oy + r, x = ox + c;
            dst[r * pitch + c] = (y >= 0 && y < Hs && x >= 0 && x < Ws) ? src[(size_t)y * Ws + x] : 0.0f;
        }
    }
}

// floats [0, 4 + 2R) of a staged row from its 16-byte aligned start
template <int R>
__device__ __forceinline__ void read_row(const float *__restrict__ s, float (&v)[(4 + 2 * R + 3) / 4 * 4])
{
#pragma unroll
    for (int c = 0; c < (4 + 2 * R + 3) / 4; c++) {
        const float4 q = *reinterpret_cast<const float4 *>(s + 4 * c);
        v[4 * c] = q.x; v[4 * c + 1] = q.y; v[4 * c + 2] = q.z; v[4 * c + 3] = q.w;
    }
}

// the horizontal filter at four neighbouring columns: out_j = sum_k w_k z_(j + k)
template <int R, int NV>
__device__ __forceinline__ float4 filter_row(const float (&z)[NV], const Window &win)
{
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float acc = win.w[0] * z[j];
#pragma unroll
        for (int k = 1; k <= 2 * R; k++) acc = fmaf(win.w[k], z[j + k], acc);
        o[j] = acc;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// the vertical filters of NP planes [TH + 2R][TW] at rows ty .. ty + 2R, columns tx4 .. tx4 + 3, from 0: tap by tap, every
// plane's four sums advancing together.  The tap loop stays a loop: unrolled, the scheduler issues all NP (2R + 1) reads
// ahead of the sums and holds them in registers (256 VGPRs, one wave per SIMD at R = 5, or spills under a register limit).
template <int R, int NP>
__device__ __forceinline__ void filter_columns(const float (*planes)[(TH + 2 * R) * TW], int tx4, int ty, const Window &win,
                                               float (&o)[NP][4])
{
#pragma unroll
    for (int f = 0; f < NP; f++) o[f][0] = o[f][1] = o[f][2] = o[f][3] = 0.0f;
#pragma unroll 1
    for (int k = 0; k <= 2 * R; k++) {
        const float w = win.w[k];
#pragma unroll
        for (int f = 0; f < NP; f++) {
            const float4 q = *reinterpret_cast<const float4 *>(planes[f] + (ty + k) * TW + tx4);
            o[f][0] = fmaf(w, q.x, o[f][0]);
            o[f][1] = fmaf(w, q.y, o[f][1]);
            o[f][2] = fmaf(w, q.z, o[f][2]);
            o[f][3] = fmaf(w, q.w, o[f][3]);
        }
    }
}

// four floats of row y of a plane [Hs, Ws] from column x; nothing outside
__device__ __forceinline__ void store_row4(float *__restrict__ plane, int Hs, int Ws, int y, int x, const float v[4], bool vec)
{
    if (y >= Hs || x >= Ws) return;
    float *dst = plane + (size_t)y * Ws + x;
    if (vec) {  // Ws % 4 == 0 and x % 4 == 0: all four inside
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (x + j < Ws) dst[j] = v[j];
    }
}

__device__ __forceinline__ void load_row4(const float *__restrict__ plane, int Hs, int Ws, int y, int x, float v[4], bool vec)
{
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (y >= Hs || x >= Ws) return;
    const float *src = plane + (size_t)y * Ws + x;
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (x + j < Ws) v[j] = src[j];
    }
}

struct ForwardArgs {
    const float *images, *target, *mask;  // mask may be NULL
    size_t target_stride, mask_stride;    // per image (0: shared)
    float *ssim_map;                      // [B, C, Hq, Wq] or NULL
    float *grad_maps;                     // [3, B, C, Hq, Wq] or NULL
    double *partial;                      // [B, n_tiles, 2]
    int B, C, H, W, Hq, Wq, off, tiles_x;
    float c1, c2;
    int vec_in, vec_out;
};

// (three waves per SIMD: what the LDS of R = 5 allows)
template <int R>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(3)))
void k_ssim_forward(ForwardArgs a, Window win)
{
    constexpr int PITCH = pitch_of(R), ROWS = rows_of(R), NV = (4 + 2 * R + 3) / 4 * 4;
    __shared__ __align__(16) float sx[ROWS * PITCH], sy[ROWS * PITCH];
    __shared__ __align__(16) float hp[5][ROWS * TW];  // mu_x, mu_y, xx, yy, xy after the rows
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tile = blockIdx.x, trow = tile / a.tiles_x, tcol = tile - trow * a.tiles_x;
    const int x0 = tcol * TW, y0 = trow * TH;            // the tile's first window centre
    const int tx4 = 4 * (tid & 15), ty = tid >> 4;
    const int qx = x0 + tx4, qy = y0 + ty;               // the thread's first centre
    const size_t plane = (size_t)a.H * a.W, qplane = (size_t)a.Hq * a.Wq;
    float m[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (a.mask) {
        const float *mp = a.mask + (size_t)b * a.mask_stride;
#pragma unroll
        for (int j = 0; j < 4; j++)
            m[j] = (qy < a.Hq && qx + j < a.Wq) ? mp[(size_t)(qy + a.off) * a.W + (qx + j + a.off)] : 0.0f;
    }
    double loss = 0.0, msum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (qy < a.Hq && qx + j < a.Wq) msum += (double)m[j];
    for (int c = 0; c < a.C; c++) {
        const float *xp = a.images + ((size_t)b * a.C + c) * plane;
        const float *yp = a.target + (size_t)b * a.target_stride + (size_t)c * plane;
        stage_plane(sx, xp, a.H, a.W, y0 + a.off - R, x0 + a.off - R, ROWS, TW + 2 * R, PITCH, a.vec_in);
        stage_plane(sy, yp, a.H, a.W, y0 + a.off - R, x0 + a.off - R, ROWS, TW + 2 * R, PITCH, a.vec_in);
        __syncthreads();  // staged; and the previous channel's columns have been read
        for (int i = tid; i < ROWS * 16; i += BLOCK) {
            const int r = i >> 4, s4 = 4 * (i & 15);
            float xs[NV], ys[NV], pr[NV];
            read_row<R>(sx + r * PITCH + s4, xs);
            read_row<R>(sy + r * PITCH + s4, ys);
            *reinterpret_cast<float4 *>(&hp[0][r * TW + s4]) = filter_row<R>(xs, win);
            *reinterpret_cast<float4 *>(&hp[1][r * TW + s4]) = filter_row<R>(ys, win);
#pragma unroll
            for (int k = 0; k < NV; k++) pr[k] = xs[k] * xs[k];
            *reinterpret_cast<float4 *>(&hp[2][r * TW + s4]) = filter_row<R>(pr, win);
#pragma unroll
            for (int k = 0; k < NV; k++) pr[k] = ys[k] * ys[k];
            *reinterpret_cast<float4 *>(&hp[3][r * TW + s4]) = filter_row<R>(pr, win);
#pragma unroll
            for (int k = 0; k < NV; k++) pr[k] = xs[k] * ys[k];
            *reinterpret_cast<float4 *>(&hp[4][r * TW + s4]) = filter_row<R>(pr, win);
        }
        __syncthreads();  // the rows are there; the staged planes are free for the next channel
        float o[5][4];
        filter_columns<R, 5>(hp, tx4, ty, win, o);
        const float (&mux)[4] = o[0], (&muy)[4] = o[1], (&gxx)[4] = o[2], (&gyy)[4] = o[3], (&gxy)[4] = o[4];
        float S[4], M1[4], M2[4], M3[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float pxx = mux[j] * mux[j], pyy = muy[j] * muy[j], pxy = mux[j] * muy[j];
            const float sxx = gxx[j] - pxx, syy = gyy[j] - pyy, sxy = gxy[j] - pxy;
            const float a1 = (pxy + pxy) + a.c1, b1 = (pxx + pyy) + a.c1;
            const float a2 = (sxy + sxy) + a.c2, b2 = (sxx + syy) + a.c2;
            const float num = a1 * a2, den = b1 * b2;
            S[j] = num / den;
            if (a.grad_maps) {
                const float mx2 = mux[j] + mux[j], my2 = muy[j] + muy[j];
                M3[j] = (a1 + a1) / den;
                M2[j] = -(S[j] / b2);
                M1[j] = (((my2 * a2) / den - (mx2 * S[j]) / b1) - mx2 * M2[j]) - muy[j] * M3[j];
            }
            if (qy < a.Hq && qx + j < a.Wq) loss += (double)m[j] * (1.0 - (double)S[j]);
        }
        const size_t at = ((size_t)b * a.C + c) * qplane;
        if (a.ssim_map) store_row4(a.ssim_map + at, a.Hq, a.Wq, qy, qx, S, a.vec_out);
        if (a.grad_maps) {
            const size_t each = (size_t)a.B * a.C * qplane;
            store_row4(a.grad_maps + at, a.Hq, a.Wq, qy, qx, M1, a.vec_out);
            store_row4(a.grad_maps + each + at, a.Hq, a.Wq, qy, qx, M2, a.vec_out);
            store_row4(a.grad_maps + 2 * each + at, a.Hq, a.Wq, qy, qx, M3, a.vec_out);
        }
    }
    const double both[2] = {loss, msum};
    const double sum = block_sums<BLOCK>(both, 2);
    if (tid < 2) a.partial[((size_t)b * gridDim.x + blockIdx.x) * 2 + tid] = sum;
}

// partial [B, n_tiles, 2] -> loss [B], scales [B] (or NULL)
__global__ __launch_bounds__(BLOCK) void k_ssim_finish(const double *__restrict__ partial, float *__restrict__ loss,
                                                       double *__restrict__ scales, int B, int C, int n_tiles, int mean)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *p = partial + (size_t)b * n_tiles * 2;
    const double L = ordered_sum(p, n_tiles, 2), M = ordered_sum(p + 1, n_tiles, 2);
    const double k = mean ? (M != 0.0 ? 1.0 / ((double)C * M) : 0.0) : 1.0;
    loss[b] = (float)(k * L);
    if (scales) scales[b] = k;
}

struct BackwardArgs {
    const float *images, *target, *mask;
    size_t target_stride, mask_stride;
    const float *grad_maps;   // [3, B, C, Hq, Wq]
    const double *scales;     // [B]
    const float *grad_loss;   // [B]
    float *grad_images;       // [B, C, H, W]
    int B, C, H, W, Hq, Wq, off, tiles_x;
    int vec_img, vec_map, vec_mask;
};

template <int R>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(3)))
void k_ssim_backward(BackwardArgs a, Window win)  // win: the taps reversed
{
    constexpr int PITCH = pitch_of(R), ROWS = rows_of(R), NV = (4 + 2 * R + 3) / 4 * 4;
    __shared__ __align__(16) float sm[3][ROWS * PITCH], smask[ROWS * PITCH];
    __shared__ __align__(16) float hp[3][ROWS * TW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tile = blockIdx.x, trow = tile / a.tiles_x, tcol = tile - trow * a.tiles_x;
    const int x0 = tcol * TW, y0 = trow * TH;            // the tile's first pixel
    const int tx4 = 4 * (tid & 15), ty = tid >> 4;
    const int px = x0 + tx4, py = y0 + ty;
    const size_t plane = (size_t)a.H * a.W, qplane = (size_t)a.Hq * a.Wq, each = (size_t)a.B * a.C * qplane;
    const double coef = -((double)a.grad_loss[b] * a.scales[b]);
    // staged element (r, c) is window centre (y0 - off - R + r, x0 - off - R + c) of the map, pixel (y0 - R + r, x0 - R + c)
    if (a.mask)
        stage_plane(smask, a.mask + (size_t)b * a.mask_stride, a.H, a.W, y0 - R, x0 - R, ROWS, TW + 2 * R, PITCH, a.vec_mask);
    for (int c = 0; c < a.C; c++) {
        const size_t at = ((size_t)b * a.C + c) * qplane;
#pragma unroll
        for (int f = 0; f < 3; f++)
            stage_plane(sm[f], a.grad_maps + f * each + at, a.Hq, a.Wq, y0 - a.off - R, x0 - a.off - R, ROWS, TW + 2 * R, PITCH,
                        a.vec_map);
        __syncthreads();
        for (int i = tid; i < ROWS * 16; i += BLOCK) {
            const int r = i >> 4, s4 = 4 * (i & 15);
            float mk[NV], v[NV];
            if (a.mask) read_row<R>(smask + r * PITCH + s4, mk);
#pragma unroll
            for (int f = 0; f < 3; f++) {
                read_row<R>(sm[f] + r * PITCH + s4, v);
                if (a.mask) {
#pragma unroll
                    for (int k = 0; k < NV; k++) v[k] = mk[k] * v[k];
                }
                *reinterpret_cast<float4 *>(&hp[f][r * TW + s4]) = filter_row<R>(v, win);
            }
        }
        __syncthreads();
        float o[3][4], x[4], y[4], out[4];
        filter_columns<R, 3>(hp, tx4, ty, win, o);
        const float (&F1)[4] = o[0], (&F2)[4] = o[1], (&F3)[4] = o[2];
        load_row4(a.images + ((size_t)b * a.C + c) * plane, a.H, a.W, py, px, x, a.vec_img);
        load_row4(a.target + (size_t)b * a.target_stride + (size_t)c * plane, a.H, a.W, py, px, y, a.vec_img);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double s = ((double)F1[j] + (2.0 * (double)x[j]) * (double)F2[j]) + (double)y[j] * (double)F3[j];
            out[j] = (float)(coef * s);
        }
        store_row4(a.grad_images + ((size_t)b * a.C + c) * plane, a.H, a.W, py, px, out, a.vec_img);
    }
}

// --------------------------------------------------------------------------------------------------------------------
// host

inline int tiles_x_of(int W) { return (W + TW - 1) / TW; }
inline int n_tiles_of(int H, int W) { return tiles_x_of(W) * ((H + TH - 1) / TH); }

// B images of C planes [H, W], windows of n taps; -> Hq, Wq
int ssim_sizes(int B, int C, int H, int W, int n, int valid, int &Hq, int &Wq)
{
    if (B < 1 || B > 65535 || C < 1 || H < 1 || W < 1 || H > 32768 || W > 32768) return NR_E_SIZE;
    if (n < 3 || n > MAXN || n % 2 == 0) return NR_E_SIZE;
    if ((size_t)C * (size_t)H * (size_t)W > 0x7fffffffull) return NR_E_SIZE;
    Hq = valid ? H - (n - 1) : H;
    Wq = valid ? W - (n - 1) : W;
    return (Hq < 1 || Wq < 1) ? NR_E_SIZE : 0;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <typename Args>
void launch_forward(int R, dim3 grid, hipStream_t st, const Args &a, const Window &w)
{
    switch (R) {
    case 1: hipLaunchKernelGGL(k_ssim_forward<1>, grid, dim3(BLOCK), 0, st, a, w); break;
    case 2: hipLaunchKernelGGL(k_ssim_forward<2>, grid, dim3(BLOCK), 0, st, a, w); break;
    case 3: hipLaunchKernelGGL(k_ssim_forward<3>, grid, dim3(BLOCK), 0, st, a, w); break;
    case 4: hipLaunchKernelGGL(k_ssim_forward<4>, grid, dim3(BLOCK), 0, st, a, w); break;
    default: hipLaunchKernelGGL(k_ssim_forward<5>, grid, dim3(BLOCK), 0, st, a, w); break;
    }
}

template <typename Args>
void launch_backward(int R, dim3 grid, hipStream_t st, const Args &a, const Window &w)
{
    switch (R) {
    case 1: hipLaunchKernelGGL(k_ssim_backward<1>, grid, dim3(BLOCK), 0, st, a, w); break;
    case 2: hipLaunchKernelGGL(k_ssim_backward<2>, grid, dim3(BLOCK), 0, st, a, w); break;
    case 3: hipLaunchKernelGGL(k_ssim_backward<3>, grid, dim3(BLOCK), 0, st, a, w); break;
    case 4: hipLaunchKernelGGL(k_ssim_backward<4>, grid, dim3(BLOCK), 0, st, a, w); break;
    default: hipLaunchKernelGGL(k_ssim_backward<5>, grid, dim3(BLOCK), 0, st, a, w); break;
    }
}

}  // namespace

NR_API size_t nr_ssim_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t window_size, int32_t valid)
{
    int Hq, Wq;
    if (ssim_sizes(B, 1, H, W, window_size, valid, Hq, Wq)) return 0;
    return (size_t)B * n_tiles_of(Hq, Wq) * 2 * sizeof(double);
}

NR_API int nr_ssim_loss_forward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                                int32_t mask_per_image, const float *window, float *loss, float *ssim_map, float *grad_maps,
                                double *scales, int32_t B, int32_t C, int32_t H, int32_t W, int32_t window_size, int32_t valid,
                                int32_t mean, double c1, double c2, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!images || !target || !window || !loss || (grad_maps != nullptr) != (scales != nullptr)) return NR_E_NULL;
    int Hq, Wq;
    if (int e = ssim_sizes(B, C, H, W, window_size, valid, Hq, Wq)) return e;
    const int nt = n_tiles_of(Hq, Wq);
    if (!workspace || workspace_bytes < (size_t)B * nt * 2 * sizeof(double)) return NR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int R = window_size / 2;
    Window win;
    for (int k = 0; k < MAXN; k++) win.w[k] = k < window_size ? window[k] : 0.0f;
    ForwardArgs a;
    a.images = images; a.target = target; a.mask = mask;
    a.target_stride = target_per_image ? (size_t)C * H * W : 0;
    a.mask_stride = mask_per_image ? (size_t)H * W : 0;
    a.ssim_map = ssim_map; a.grad_maps = grad_maps;
    a.partial = (double *)workspace;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Hq = Hq; a.Wq = Wq; a.off = valid ? R : 0; a.tiles_x = tiles_x_of(Wq);
    a.c1 = (float)c1; a.c2 = (float)c2;
    a.vec_in = W % 4 == 0 && aligned16(images) && aligned16(target);
    a.vec_out = Wq % 4 == 0 && aligned16(ssim_map) && aligned16(grad_maps);
    launch_forward(R, dim3((unsigned)nt, (unsigned)B), st, a, win);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_ssim_finish, dim3((unsigned)((B + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, a.partial, loss, scales, B, C,
                       nt, mean);
    return launch_status();
}

NR_API int nr_ssim_loss_backward(const float *images, const float *target, const float *mask, int32_t target_per_image,
                                 int32_t mask_per_image, const float *window, const float *grad_maps, const double *scales,
                                 const float *grad_loss, float *grad_images, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t window_size, int32_t valid, void *stream)
{
    if (!images || !target || !window || !grad_maps || !scales || !grad_loss || !grad_images) return NR_E_NULL;
    int Hq, Wq;
    if (int e = ssim_sizes(B, C, H, W, window_size, valid, Hq, Wq)) return e;
    const int R = window_size / 2;
    Window win;
    for (int k = 0; k < MAXN; k++) win.w[k] = k < window_size ? window[window_size - 1 - k] : 0.0f;
    BackwardArgs a;
    a.images = images; a.target = target; a.mask = mask;
    a.target_stride = target_per_image ? (size_t)C * H * W : 0;
    a.mask_stride = mask_per_image ? (size_t)H * W : 0;
    a.grad_maps = grad_maps; a.scales = scales; a.grad_loss = grad_loss; a.grad_images = grad_images;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Hq = Hq; a.Wq = Wq; a.off = valid ? R : 0; a.tiles_x = tiles_x_of(W);
    a.vec_img = W % 4 == 0 && aligned16(images) && aligned16(target) && aligned16(grad_images);
    a.vec_map = Wq % 4 == 0 && aligned16(grad_maps);
    a.vec_mask = W % 4 == 0 && aligned16(mask);
    launch_backward(R, dim3((unsigned)n_tiles_of(H, W), (unsigned)B), (hipStream_t)stream, a, win);
    return launch_status();
}
