// nr_soft_render.hip -- soft colour rendering: the soft silhouette's coverage, aggregated over the faces with a depth-weighted
// softmax, and the exact gradient of that definition to x, y, z and the face colours (include/nr_hip.h; DESIGN "Soft colour
// rendering").
//
// A face contributes iff its nine coordinates are finite, near <= z <= far at its three vertices and its doubled area
// (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0), taken in double, is not 0.  Per contributing face f and pixel p: d2, the chosen
// segment k, its clamped t, r, the side s and x = s d2 / sigma are soft_pair's (nr_soft_pair.h); c_0, c_1, c_2 are the edge
// functions of the segments v0v1, v1v2, v2v0 at p.  The pair is TAKEN iff s = +1 or d2 <= 17 sigma (the box of the record,
// the bounding box grown by sqrt(17 sigma), is the coarse filter in front of this test).  Inverse depth at the pixel:
//   inside   A = c_0 + c_1 + c_2, lambda_0 = c_1 / A, lambda_1 = c_2 / A, lambda_2 = c_0 / A
//   outside  lambda = 1 - t at the first vertex of segment k, t at its second, 0 at the third
//   iz = lambda_0 / z0 + lambda_1 / z1 + lambda_2 / z2,  zp = 1 / iz,  zn = (far - zp) / (far - near)
// Over the taken pairs of p in ascending f, with m = max(eps, max_f zn_f), D = 1 / (1 + e^-x):
//   w_f = D_f exp((zn_f - m) / gamma),  w_b = exp((eps - m) / gamma),  Z = w_b + sum w_f
//   rgb = (w_b C_b + sum w_f C_f) / Z,  Q = prod 1 / (1 + e^x_f),  alpha = 1 - Q
//   k_render_setup     (image, face) -> an 80-byte record: the base record's 48 bytes (soft_record, nr_soft_pair.h: the flag
//                      with the area rule, the silhouette's box), 1 / z_k, the colour
//   k_render_forward   a workgroup of four waves owns a 16 x 16 pixel tile, a lane a pixel (soft_tile); the records go
//                      through LDS in chunks of 256 (20 KiB), the compact list ascending in f by soft_filter_chunk, a
//                      wave-uniform trip count.  TWO walks of the image's records: the first finds m, the second sums.
//                      Stores rgba, Q, (m, Z).
//   k_render_backward  a wave owns an (image, face): it walks the pixels of the box, lanes strided, recomputes the pair, sums
//                      six xy, three z and three colour gradients per lane, reduces them in the fixed xor tree, one store
//                      per entry.
//   k_render_colors    shared colours: the B partial colour gradients added in ascending b in double.
// Corner colours (nr_soft_corners_*; DESIGN "Soft colour rendering", Corner colours): colors carry nine floats per face,
// (corner, rgb), and the colour of a taken pair is interpolated at the pixel with the depth's own weights,
//   u_k = lambda_k / z_k,  mu_k = u_k zp,  C_f(p) = (mu_0 C_f0 + mu_1 C_f1) + mu_2 C_f2   per channel
// -- perspective-correct inside, the colour of the nearest boundary point outside.  The three kernels are the <true>
// instantiations of the same templates: a 96-byte record (the 48 bytes, 1 / z_k, nine colour floats; 24 KiB per chunk), nine
// colour sums per lane next to the nine of the coordinates.  Backward, with E_k = (W zp) (g_rgb . (C_fk - C_f(p))):
//   dL/dC_fk += (W g_rgb) mu_k,  dL/dz_k = -((diz + E_k) lambda_k) / z_k^2,
//   free t on a -> b   T = (diz (iz_b - iz_a) + (E_b iz_b - E_a iz_a)) / ee
//   inside             q_j = (diz / A) (iz_v(j) - iz) + (E_v(j) iz_v(j)) / A,  v(0) = 2, v(1) = 0, v(2) = 1
// the flat terms plus one addition each (sum_k lambda_k dL/dlambda_k taken as diz iz: sum_k u_k E_k = 0 in exact arithmetic).
// The <false> instantiations are the flat kernels, instruction for instruction.
// No atomics, no host synchronisation, every output element stored; the same bits in every run and for an image alone or
// inside a batch: a pixel's sums depend on the set of its taken pairs and their order in f alone.  The base record, the box, the
// tile, the filter, the pair and the constants are nr_soft_pair.h's, one definition with nr_soft_silhouette.hip.
// UV images (nr_soft_uv_*; DESIGN "Soft colour rendering", UV images): the colour of a taken pair is a light colour per face
// times the bake's bilinear lookup of the face's image at the pair's own weights,
//   d_k = min(max(mu_k, 0), 1),  T_f(p) = texel_reads' four reads of image face_image[f] at d (uv_texel),  C_f(p) = L_f T_f(p)
// -- the texture render() shows inside, the texture of the nearest boundary point outside; a face without an image shows L_f
// times the mean of its base cube.  The forward and the backward are the <UV> instantiations of the same two templates (the
// flat and corner ones are <FLAT> and <CORNER>: the former <false> and <true>, their instructions unchanged), k_uv_setup
// writes a 112-byte record (the 48 bytes, 1 / z_k, the light colour, six uv floats, the image's first pixel, H and W; 28 KiB
// per chunk).  Backward, with Tx_c = sum_r (dw_r / dwx1) I[q_r]_c, Ty_c likewise, G_k = sum_c g_c L_c (Tx_c uvx_k (W - 1) +
// Ty_c uvy_k (H - 1)):  E_k = (W zp) (G_k - sum_j mu_j G_j) stands where the corner colours' E_k stands and every line after it
// is shared; dL/dL_fc += (W g_c) T_c takes the three colour sums.  These outputs keep the paragraph above: fixed order, the
// same bits in every run.  The IMAGE gradient does not: dL/dI[q_r]_c += W g_c L_c w_r is formed in double and added with
// double atomics into a zero-filled scratch (many pairs land on one image pixel; the scheme of nr_uv_pixel.hip, for its
// reason), zero terms skipped, and k_uv_image_round rounds every sum once -- a double sum whose additions arrive in no fixed
// order.
// Texture cubes (nr_soft_cubes_*; DESIGN "Soft colour rendering", Texture cubes): the colour of a taken pair is a light colour
// per face times the rasterizer's trilinear lookup of the face's cube [ts, ts, ts, 3] at the pair's own weights,
//   v_k = min(max(mu_k (ts - 1), 0), (ts - 1) - texture_eps),  T_f(p) = the eight taps of cube_texel,  C_f(p) = L_f T_f(p)
// -- compute_taps' sequence and sum_taps' sum (nr_device.h) with mu_k where the rasterizer has w_k (zp / z_k).  The <CUBE>
// instantiations of the two templates; k_cube_setup writes an 80-byte record (the flat one, with the face's index where the
// flat record has a 0: the forward's compact list loses a record's position).  Backward, with D_kc = sum_pn (dw_pn / dfr_k)
// tex[tap_pn]_c (cube_slopes) and G_k = (ts - 1) sum_c g_c L_c D_kc:  E_k = (W zp) (G_k - sum_j mu_j G_j) and everything after it
// as above; dL/dL_fc += (W g_c) T_c.  THE CUBE GRADIENT TAKES NO ATOMICS: the wave that owns (image, face) owns the face's
// cube, keeps ts^3 * 3 double sums in LDS that no other wave touches and adds the terms ((W g_c) L_c) w_pn of its taken pairs
// one pair after the other in the order of its walk (k_render_backward has the scheme); every entry is rounded once and
// stored, zeros included.  Fixed order, the same bits in every run and for an image alone or inside a batch.
#include <type_traits>

#include "nr_soft_pair.h"

using namespace nr;

namespace {

constexpr int RENDER_REC = 5;         // float4 per record: the base record's SOFT_REC and two more
constexpr int CORNER_REC = 6;         // ... with corner colours

// what a record holds beyond the base record: (1 / z0, 1 / z1, 1 / z2, red), (green, blue, 0, 0)
struct FaceShade {
    float iz0, iz1, iz2, cr, cg, cb;
};

__device__ __forceinline__ FaceShade unpack_shade(const float4 &d, const float4 &e)
{
    FaceShade r;
    r.iz0 = d.x; r.iz1 = d.y; r.iz2 = d.z; r.cr = d.w;
    r.cg = e.x; r.cb = e.y;
    return r;
}

// the edge function of segment a -> b at p, in soft_segment's own operations
__device__ __forceinline__ float edge_function(float px, float py, float ax, float ay, float bx, float by)
{
    const float ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay;
    return ex * wy - ey * wx;
}

// the depth of a pair: the weights lambda of the three vertices (perspective-correct barycentric inside, the nearest point's
// outside), 1 / A, iz, zp and zn
struct PairDepth {
    float l0, l1, l2, rA, iz, zp, zn;
    bool taken;
};

__device__ __forceinline__ PairDepth pair_depth(float px, float py, const SoftFace &f, const FaceShade &h, const SoftPair &p,
                                                float cut, float far, float inv_range)
{
    PairDepth q;
    const float c0 = edge_function(px, py, f.x0, f.y0, f.x1, f.y1);
    const float c1 = edge_function(px, py, f.x1, f.y1, f.x2, f.y2);
    const float c2 = edge_function(px, py, f.x2, f.y2, f.x0, f.y0);
    q.rA = 1.0f / ((c0 + c1) + c2);   // (used inside only, where the three have one sign)
    const float t1 = 1.0f - p.t;
    const int k = p.k;
    const float o0 = k == 0 ? t1 : (k == 2 ? p.t : 0.0f);
    const float o1 = k == 1 ? t1 : (k == 0 ? p.t : 0.0f);
    const float o2 = k == 2 ? t1 : (k == 1 ? p.t : 0.0f);
    q.l0 = p.inside ? c1 * q.rA : o0;
    q.l1 = p.inside ? c2 * q.rA : o1;
    q.l2 = p.inside ? c0 * q.rA : o2;
    q.iz = (q.l0 * h.iz0 + q.l1 * h.iz1) + q.l2 * h.iz2;
    q.zp = 1.0f / q.iz;
    q.zn = (far - q.zp) * inv_range;
    q.taken = p.inside || (p.rx * p.rx + p.ry * p.ry) <= cut;   // (soft_segment's own d2)
    return q;
}

// what a corner record holds beyond FaceShade's 1 / z_k: (., ., ., c00), (c01, c02, c10, c11), (c12, c20, c21, c22) -- c[corner][rgb]
struct CornerColor {
    float c00, c01, c02, c10, c11, c12, c20, c21, c22;
};

__device__ __forceinline__ CornerColor unpack_corners(const float4 &d, const float4 &e, const float4 &g)
{
    CornerColor r;
    r.c00 = d.w; r.c01 = e.x; r.c02 = e.y; r.c10 = e.z; r.c11 = e.w;
    r.c12 = g.x; r.c20 = g.y; r.c21 = g.z; r.c22 = g.w;
    return r;
}

// the perspective-correct weights of a pair and its colour at the pixel; u_k are pair_depth's own products
struct PairColor {
    float mu0, mu1, mu2, r, g, b;
};

__device__ __forceinline__ PairColor pair_color(const PairDepth &q, const FaceShade &h, const CornerColor &c)
{
    PairColor o;
    o.mu0 = (q.l0 * h.iz0) * q.zp;
    o.mu1 = (q.l1 * h.iz1) * q.zp;
    o.mu2 = (q.l2 * h.iz2) * q.zp;
    o.r = (o.mu0 * c.c00 + o.mu1 * c.c10) + o.mu2 * c.c20;
    o.g = (o.mu0 * c.c01 + o.mu1 * c.c11) + o.mu2 * c.c21;
    o.b = (o.mu0 * c.c02 + o.mu1 * c.c12) + o.mu2 * c.c22;
    return o;
}

struct RenderArgs {
    float inv_sigma, inv_gamma, cut, far, inv_range, eps;
    float bg_r, bg_g, bg_b;
};

// the colour of a pair: one per face, three corner colours, a light colour times a UV image sample, or times a cube sample
constexpr int FLAT = 0, CORNER = 1, UV = 2, CUBE = 3;
constexpr int UV_REC = 7;             // float4 per record with a UV sample
constexpr int mode_rec(int mode) { return mode == UV ? UV_REC : (mode == CORNER ? CORNER_REC : RENDER_REC); }
constexpr int CUBE_MIN_TS = 2, CUBE_MAX_TS = 8;   // the texture sizes of the cube kernels (48 KiB of LDS per backward workgroup at 8)

// what the UV kernels take beyond RenderArgs (the flat and corner kernels keep RenderArgs itself: their signatures stay)
struct UVArgs : RenderArgs {
    const float *images;     // [image_batch, P, 3], each image top row first
    size_t image_stride;     // floats between the images of two batch elements, 0 for shared images
    double *acc;             // backward: the double sums of the image gradient, or nullptr when it is not asked for
    size_t acc_stride;       // doubles, 0 for shared images
};
// ... and the cube kernels
struct CubeArgs : RenderArgs {
    const float *cubes;      // [cube_batch, F, ts, ts, ts, 3]
    size_t cube_stride;      // floats between the cubes of two batch elements, 0 for shared cubes
    int ts;
    double hi;               // the upper clamp of a sample position, (ts - 1) - texture_eps
    float *grad;             // backward: the cube gradient of every image [B, F, ts^3, 3], or nullptr when it is not asked for
};
template <int MODE>
using ModeArgs = std::conditional_t<MODE == UV, UVArgs, std::conditional_t<MODE == CUBE, CubeArgs, RenderArgs>>;

// what a UV record holds beyond FaceShade's 1 / z_k and the light colour (FaceShade's cr, cg, cb):
// (., ., uvx0, uvy0), (uvx1, uvy1, uvx2, uvy2), (first pixel, H, W, 0); a face without an image has H = 0 and the mean of its
// base cube in the first three uv slots
struct UVFace {
    float uv[6];
    int off, H, W;
};

__device__ __forceinline__ UVFace unpack_uv(const float4 &e, const float4 &g, const float4 &i)
{
    UVFace u;
    u.uv[0] = e.z; u.uv[1] = e.w; u.uv[2] = g.x; u.uv[3] = g.y; u.uv[4] = g.z; u.uv[5] = g.w;
    u.off = __float_as_int(i.x); u.H = __float_as_int(i.y); u.W = __float_as_int(i.z);
    return u;
}

// the sample of a taken pair: the four reads q (packed pixels) with their weights w, the weights' factors ax = (wx0, wx1,
// wy0, wy1), the texels i[read][rgb] and the sum (r, g, b)
struct UVTexel {
    int q[4];
    float w[4], ax[4], i[4][3], r, g, b;
};

// T_f(p): the bake's own bilinear lookup (texel_reads, nr_device.h) at d_k = min(max(mu_k, 0), 1), the reads summed in read
// order from 0 as uv_color sums them; the mean base colour for a face without an image.  NO READ LEAVES THE FACE'S IMAGE,
// whatever uv and mu hold (uv outside [0, 1], infinite, NaN): texel_reads clamps the flat index to [0, H W - 1], mirror_row
// maps that range onto itself, and k_uv_setup admits an image only when [off, off + H W) lies inside the packed pixels.
__device__ __forceinline__ void uv_texel(const UVFace &u, const PairColor &pc, const float *__restrict__ images, UVTexel &s)
{
    if (u.H == 0) {
        s.r = u.uv[0]; s.g = u.uv[1]; s.b = u.uv[2];
        return;
    }
    const float d[3] = {fminf(fmaxf(pc.mu0, 0.0f), 1.0f), fminf(fmaxf(pc.mu1, 0.0f), 1.0f), fminf(fmaxf(pc.mu2, 0.0f), 1.0f)};
    long long p[4];
    texel_reads(u.uv, d, u.H, u.W, p, s.w, s.ax);
#pragma unroll
    for (int r = 0; r < 4; r++) {   // the four texels are requested together
        s.q[r] = u.off + mirror_row(p[r], u.H, u.W);
        const float *px = images + (size_t)s.q[r] * 3;
        s.i[r][0] = px[0]; s.i[r][1] = px[1]; s.i[r][2] = px[2];
    }
    s.r = s.g = s.b = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        s.r += s.i[r][0] * s.w[r];
        s.g += s.i[r][1] * s.w[r];
        s.b += s.i[r][2] * s.w[r];
    }
}

// the sample of a taken pair in its face's cube: the cell i, the fractions fr, the eight taps' weights w and texels tx[tap][rgb]
// (bit pn of `inside`: tap pn lies inside the cube; the texels of the others are handed back as zeros) and the sum (r, g, b)
struct CubeTexel {
    int i[3];
    float fr[3], w[8], tx[8][3], r, g, b;
    unsigned inside;
};

// T_f(p): compute_taps' sequence (nr_device.h) at v_k = mu_k (ts - 1) -- max with 0, which also takes a NaN to 0, then the min
// with hi in double, rounded --, summed as sum_taps sums: the eight texels requested together, from 0 in tap order, a tap whose
// flat index leaves the cube skipped (its weight is an exact 0) and its address replaced by the cube's last texel.  NO READ
// LEAVES THE FACE'S CUBE whatever mu holds: 0 <= v_k <= hi <= ts - 1, so every i_k lies in [0, ts - 1] and every flat index
// read in [0, ts^3 - 1].
__device__ __forceinline__ void cube_texel(const float *__restrict__ cube, int ts, double hi, const PairColor &pc, CubeTexel &s)
{
    const float mu[3] = {pc.mu0, pc.mu1, pc.mu2};
    const int T = ts * ts * ts;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v = mu[k] * (float)(ts - 1);
        v = fmaxf(v, 0.0f);
        v = (float)fmin((double)v, hi);
        s.i[k] = (int)v;
        s.fr[k] = v - (float)s.i[k];
    }
    s.inside = 0;
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        float w = 1.0f;
        int idx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (((pn >> k) & 1) == 0) {
                w *= 1.0f - s.fr[k];
                idx[k] = s.i[k];
            } else {
                w *= s.fr[k];
                idx[k] = s.i[k] + 1;
            }
        }
        const int flat = (idx[0] * ts + idx[1]) * ts + idx[2];
        s.w[pn] = w;
        s.inside |= (unsigned)(flat < T) << pn;
        const float *p = cube + min(flat, T - 1) * 3;
        s.tx[pn][0] = p[0]; s.tx[pn][1] = p[1]; s.tx[pn][2] = p[2];
    }
    float c[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        const bool in = (s.inside >> pn) & 1u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float sum = c[k] + s.w[pn] * s.tx[pn][k];
            c[k] = in ? sum : c[k];
            s.tx[pn][k] = in ? s.tx[pn][k] : 0.0f;
        }
    }
    s.r = c[0]; s.g = c[1]; s.b = c[2];
}

// D_k: the derivative of the sum above to fr_k, per channel -- the four differences of the taps with and without bit k, each
// times the product of the other two dimensions' factors, added in ascending tap order from the first
__device__ __forceinline__ void cube_slopes(const CubeTexel &s, int k, float d[3])
{
    const int ka = k == 0 ? 1 : 0, kb = k == 2 ? 1 : 2;   // the other two dimensions, ascending
    const float fa[2] = {1.0f - s.fr[ka], s.fr[ka]}, fb[2] = {1.0f - s.fr[kb], s.fr[kb]};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float sum = 0.0f;
#pragma unroll
        for (int jb = 0; jb < 2; jb++)
#pragma unroll
            for (int ja = 0; ja < 2; ja++) {
                const int lo = (ja << ka) | (jb << kb), up = lo | (1 << k);
                const float term = (fa[ja] * fb[jb]) * (s.tx[up][c] - s.tx[lo][c]);
                sum = (ja | jb) == 0 ? term : sum + term;
            }
        d[c] = sum;
    }
}

// --------------------------------------------------------------------------------------------------------------------
// set-up

// texture cubes: the base record, 1 / z_k and the light colour as the flat record holds its colour, then the face's own index:
// the forward's compact list loses a record's position
__global__ __launch_bounds__(256) void k_cube_setup(const float *__restrict__ faces, const float *__restrict__ light,
                                                    float4 *__restrict__ rec, int F, int S, size_t light_stride, float reach,
                                                    double near, double far)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const float *L = light + (size_t)b * light_stride + (size_t)f * 3;
    float4 *o = rec + ((size_t)b * F + f) * RENDER_REC;
    float c[9];
    soft_record<true>(faces + ((size_t)b * F + f) * 9, o, S, reach, near, far, c);
    o[3] = make_float4(1.0f / c[2], 1.0f / c[5], 1.0f / c[8], L[0]);
    o[4] = make_float4(L[1], L[2], __int_as_float(f), 0.0f);
}

template <bool CORNERS>
__global__ __launch_bounds__(256) void k_render_setup(const float *__restrict__ faces, const float *__restrict__ colors,
                                                      float4 *__restrict__ rec, int F, int S, size_t color_stride, float reach,
                                                      double near, double far)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const float *col = colors + (size_t)b * color_stride + (size_t)f * (CORNERS ? 9 : 3);
    float4 *o = rec + ((size_t)b * F + f) * (CORNERS ? CORNER_REC : RENDER_REC);
    float c[9];
    soft_record<true>(faces + ((size_t)b * F + f) * 9, o, S, reach, near, far, c);   // the flag with the area rule
    o[3] = make_float4(1.0f / c[2], 1.0f / c[5], 1.0f / c[8], col[0]);
    if constexpr (CORNERS) {
        o[4] = make_float4(col[1], col[2], col[3], col[4]);
        o[5] = make_float4(col[5], col[6], col[7], col[8]);
    } else {
        o[4] = make_float4(col[1], col[2], 0.0f, 0.0f);
    }
}

// UV images: the base record, 1 / z_k and the light colour as above, then the face's uv triangle and its image's place in the
// packing.  A face whose face_image lies outside [0, M), or whose table row does not lie inside the P packed pixels, is a face
// without an image: H = 0 and the mean of its base cube (summed in double, rounded once) in the first three uv slots.
__global__ __launch_bounds__(256) void k_uv_setup(const float *__restrict__ faces, const float *__restrict__ light, UVShade uv,
                                                  float4 *__restrict__ rec, int F, int S, size_t light_stride, float reach,
                                                  double near, double far)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const float *L = light + (size_t)b * light_stride + (size_t)f * 3;
    float4 *o = rec + ((size_t)b * F + f) * UV_REC;
    float c[9];
    soft_record<true>(faces + ((size_t)b * F + f) * 9, o, S, reach, near, far, c);
    o[3] = make_float4(1.0f / c[2], 1.0f / c[5], 1.0f / c[8], L[0]);
    const int m = uv.face_image[f];
    int off = 0, H = 0, W = 0;
    if (m >= 0 && m < uv.M) {
        off = uv.table[3 * m]; H = uv.table[3 * m + 1]; W = uv.table[3 * m + 2];
        if (off < 0 || H < 1 || W < 1 || (long long)off + (long long)H * W > (long long)uv.P) H = 0;
    }
    if (H != 0) {
        const float *t = uv.faces_uv + (size_t)f * 6;
        o[4] = make_float4(L[1], L[2], t[0], t[1]);
        o[5] = make_float4(t[2], t[3], t[4], t[5]);
        o[6] = make_float4(__int_as_float(off), __int_as_float(H), __int_as_float(W), 0.0f);
    } else {
        const int T = uv.ts * uv.ts * uv.ts;
        const float *tx = uv.base + (size_t)f * T * 3;
        double sr = 0.0, sg = 0.0, sb = 0.0;
        for (int i = 0; i < T; i++) {
            sr += (double)tx[3 * i]; sg += (double)tx[3 * i + 1]; sb += (double)tx[3 * i + 2];
        }
        o[4] = make_float4(L[1], L[2], (float)(sr / T), (float)(sg / T));
        o[5] = make_float4((float)(sb / T), 0.0f, 0.0f, 0.0f);
        o[6] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// --------------------------------------------------------------------------------------------------------------------
// forward

template <int MODE>
__global__ __launch_bounds__(256) void k_render_forward(const float4 *__restrict__ rec, float *__restrict__ rgba,
                                                        float *__restrict__ trans, float *__restrict__ norm, int F, int S,
                                                        int tiles_x, ModeArgs<MODE> a)
{
    constexpr bool CORNERS = MODE == CORNER;
    constexpr int REC = mode_rec(MODE);
    __shared__ float4 list[SOFT_CHUNK * REC];
    __shared__ int wave_count[4];
    const int b = blockIdx.y;
    const SoftTile T = soft_tile(S, tiles_x);
    const int xi = T.xi, yi = T.yi;
    const float px = T.px, py = T.py;
    const float4 *rb = rec + (size_t)b * F * REC;
    // the first walk: m = max(eps, the zn of the taken pairs) -- a maximum of the very floats the second walk subtracts it from
    float m = a.eps;
    for (int c0 = 0; c0 < F; c0 += SOFT_CHUNK) {
        const int n = soft_filter_chunk<REC>(rb, c0, F, T, list, wave_count);
        for (int j = 0; j < n; j++) {
            const float4 *l = list + j * REC;
            const SoftFace s = unpack(l[0], l[1], l[2]);
            const FaceShade h = unpack_shade(l[3], l[4]);
            const SoftPair p = soft_pair(px, py, s, a.inv_sigma);
            const PairDepth q = pair_depth(px, py, s, h, p, a.cut, a.far, a.inv_range);
            m = (q.taken && in_box(s, xi, yi)) ? fmaxf(m, q.zn) : m;
        }
        __syncthreads();   // the list and the counts are rewritten by the next chunk
    }
    // the second walk
    const float wb = expf((a.eps - m) * a.inv_gamma);
    float Z = wb, cr = wb * a.bg_r, cg = wb * a.bg_g, cb = wb * a.bg_b, Q = 1.0f;
    for (int c0 = 0; c0 < F; c0 += SOFT_CHUNK) {
        const int n = soft_filter_chunk<REC>(rb, c0, F, T, list, wave_count);
        for (int j = 0; j < n; j++) {
            const float4 *l = list + j * REC;
            const SoftFace s = unpack(l[0], l[1], l[2]);
            const FaceShade h = unpack_shade(l[3], l[4]);
            const SoftPair p = soft_pair(px, py, s, a.inv_sigma);
            const PairDepth q = pair_depth(px, py, s, h, p, a.cut, a.far, a.inv_range);
            const bool take = q.taken && in_box(s, xi, yi);
            const float D = 1.0f / (1.0f + expf(-p.x));
            const float w = D * expf((q.zn - m) * a.inv_gamma);
            const float q1 = Q * (1.0f / (1.0f + expf(p.x)));   // 1 - D as 1 / (1 + e^x), never as a subtraction
            Z = take ? Z + w : Z;
            if constexpr (CORNERS) {
                const PairColor pc = pair_color(q, h, unpack_corners(l[3], l[4], l[5]));
                cr = take ? cr + w * pc.r : cr;
                cg = take ? cg + w * pc.g : cg;
                cb = take ? cb + w * pc.b : cb;
            } else if constexpr (MODE == UV) {   // the image is read for taken pairs only
                const PairColor pc = pair_color(q, h, CornerColor{});   // (its mu; the colour part folds away)
                UVTexel t = {};
                if (take) uv_texel(unpack_uv(l[4], l[5], l[6]), pc, a.images + (size_t)b * a.image_stride, t);
                cr = take ? cr + w * (h.cr * t.r) : cr;
                cg = take ? cg + w * (h.cg * t.g) : cg;
                cb = take ? cb + w * (h.cb * t.b) : cb;
            } else if constexpr (MODE == CUBE) {   // the cube is read for taken pairs only
                const PairColor pc = pair_color(q, h, CornerColor{});   // (its mu)
                CubeTexel t = {};
                if (take) {
                    const int f = min(max(__float_as_int(l[4].z), 0), F - 1);   // (the record's own; clamped, the workspace being the caller's)
                    cube_texel(a.cubes + (size_t)b * a.cube_stride + (size_t)f * (a.ts * a.ts * a.ts * 3), a.ts, a.hi, pc, t);
                }
                cr = take ? cr + w * (h.cr * t.r) : cr;
                cg = take ? cg + w * (h.cg * t.g) : cg;
                cb = take ? cb + w * (h.cb * t.b) : cb;
            } else {
                cr = take ? cr + w * h.cr : cr;
                cg = take ? cg + w * h.cg : cg;
                cb = take ? cb + w * h.cb : cb;
            }
            Q = take ? q1 : Q;
        }
        __syncthreads();
    }
    if (xi < S && yi < S) {
        const size_t SS = (size_t)S * S, o = (size_t)yi * S + xi;
        float *img = rgba + (size_t)b * 4 * SS;
        img[o] = cr / Z;
        img[SS + o] = cg / Z;
        img[2 * SS + o] = cb / Z;
        img[3 * SS + o] = 1.0f - Q;
        trans[(size_t)b * SS + o] = Q;
        norm[(size_t)b * 2 * SS + o] = m;
        norm[(size_t)b * 2 * SS + SS + o] = Z;
    }
}

// --------------------------------------------------------------------------------------------------------------------
// backward

// between LDS accesses of different lanes of ONE wave to the same address: the hardware keeps a wave's LDS operations in order,
// this keeps the compiler from moving them across
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE>
__global__ __launch_bounds__(256) void k_render_backward(const float4 *__restrict__ rec, const float *__restrict__ rgba,
                                                         const float *__restrict__ trans, const float *__restrict__ norm,
                                                         const float *__restrict__ grad_rgba, float *__restrict__ grad_faces,
                                                         float *__restrict__ grad_colors, int F, int S, ModeArgs<MODE> a)
{
    constexpr bool CORNERS = MODE == CORNER, VARIES = MODE != FLAT;   // VARIES: the colour moves with the pixel, E_k below
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int f = rfl(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (f >= F) return;
    const float4 *r = rec + ((size_t)b * F + f) * mode_rec(MODE);
    const SoftFace s = unpack(r[0], r[1], r[2]);
    const FaceShade h = unpack_shade(r[3], r[4]);
    CornerColor cc = {};
    if constexpr (CORNERS) cc = unpack_corners(r[3], r[4], r[5]);
    UVFace uvf = {};
    if constexpr (MODE == UV) uvf = unpack_uv(r[4], r[5], r[6]);
    // texture cubes: the wave owns its face's cube, so it sums the cube's gradient itself -- in double, in LDS that no other
    // wave touches, one taken pair after the other in the order of the walk (k_render_backward's comment has the scheme)
    [[maybe_unused]] double *sums = nullptr;
    [[maybe_unused]] const float *cube = nullptr;
    [[maybe_unused]] int T3 = 0;
    if constexpr (MODE == CUBE) {
        extern __shared__ double cube_sums[];
        T3 = a.ts * a.ts * a.ts * 3;
        cube = a.cubes + (size_t)b * a.cube_stride + (size_t)f * T3;
        if (a.grad) {
            sums = cube_sums + (threadIdx.x >> 6) * T3;
            for (int e = lane; e < T3; e += WAVE) sums[e] = 0.0;
            wave_lds_order();
        }
    }
    float g0x = 0.0f, g0y = 0.0f, g1x = 0.0f, g1y = 0.0f, g2x = 0.0f, g2y = 0.0f;
    float g0z = 0.0f, g1z = 0.0f, g2z = 0.0f, gcr = 0.0f, gcg = 0.0f, gcb = 0.0f;
    float g1r = 0.0f, g1g = 0.0f, g1b = 0.0f, g2r = 0.0f, g2g = 0.0f, g2b = 0.0f;   // (corners 1 and 2; gcr, gcg, gcb are corner 0's)
    // the record's box lies inside the raster or is empty (k_render_setup); clamped again, the workspace being the caller's
    const int x_lo = max(s.ix_lo, 0), x_hi = min(s.ix_hi, S - 1), y_lo = max(s.iy_lo, 0), y_hi = min(s.iy_hi, S - 1);
    if (s.on != 0 && x_lo <= x_hi && y_lo <= y_hi) {
        const int bw = x_hi - x_lo + 1, n = bw * (y_hi - y_lo + 1);   // <= S * S <= 2^28
        const size_t SS = (size_t)S * S;
        const float *img = rgba + (size_t)b * 4 * SS, *gi = grad_rgba + (size_t)b * 4 * SS;
        const float *qb = trans + (size_t)b * SS, *nb = norm + (size_t)b * 2 * SS;
        const float e0x = s.x1 - s.x0, e0y = s.y1 - s.y0, e1x = s.x2 - s.x1, e1y = s.y2 - s.y1, e2x = s.x0 - s.x2, e2y = s.y0 - s.y2;
        const float ee0 = e0x * e0x + e0y * e0y, ee1 = e1x * e1x + e1y * e1y, ee2 = e2x * e2x + e2y * e2y;   // soft_segment's ee
        const float s0 = h.iz0 * h.iz0, s1 = h.iz1 * h.iz1, s2 = h.iz2 * h.iz2;   // 1 / z_k^2
        // (texture cubes: every lane makes every trip, a lane past the last pixel on the last pixel again with nothing taken)
        const int n_walk = MODE == CUBE ? (n + WAVE - 1) / WAVE * WAVE : n;
        for (int i0 = lane; i0 < n_walk; i0 += WAVE) {
            const int i = MODE == CUBE ? min(i0, n - 1) : i0;
            const int row = i / bw, xi = x_lo + (i - row * bw), yi = y_lo + row;
            const float px = pixel_center(xi, S), py = pixel_center(yi, S);
            const SoftPair p = soft_pair(px, py, s, a.inv_sigma);
            const PairDepth q = pair_depth(px, py, s, h, p, a.cut, a.far, a.inv_range);
            const size_t o = (size_t)yi * S + xi;
            const float R = img[o], G = img[SS + o], Bl = img[2 * SS + o];
            const float gr = gi[o], gg = gi[SS + o], gb = gi[2 * SS + o], ga = gi[3 * SS + o];
            const float Qp = qb[o], m = nb[o], Z = nb[SS + o];
            const float D = 1.0f / (1.0f + expf(-p.x)), D1 = 1.0f / (1.0f + expf(p.x));
            float W = (D * expf((q.zn - m) * a.inv_gamma)) / Z;
            const bool taken = MODE == CUBE ? (q.taken && i0 < n) : q.taken;
            W = taken ? W : 0.0f;                          // a pair not taken: every term below is an exact 0
            const float Ga = taken ? ga * Qp : 0.0f;
            float hh, E0 = 0.0f, E1 = 0.0f, E2 = 0.0f;   // E_k: what corner k's colour adds to diz, 0 for a flat colour
            if constexpr (CORNERS) {
                const PairColor pc = pair_color(q, h, cc);
                hh = (gr * (pc.r - R) + gg * (pc.g - G)) + gb * (pc.b - Bl);
                const float wr = W * gr, wg = W * gg, wb = W * gb, Wz = W * q.zp;
                gcr += wr * pc.mu0; gcg += wg * pc.mu0; gcb += wb * pc.mu0;
                g1r += wr * pc.mu1; g1g += wg * pc.mu1; g1b += wb * pc.mu1;
                g2r += wr * pc.mu2; g2g += wg * pc.mu2; g2b += wb * pc.mu2;
                E0 = Wz * ((gr * (cc.c00 - pc.r) + gg * (cc.c01 - pc.g)) + gb * (cc.c02 - pc.b));
                E1 = Wz * ((gr * (cc.c10 - pc.r) + gg * (cc.c11 - pc.g)) + gb * (cc.c12 - pc.b));
                E2 = Wz * ((gr * (cc.c20 - pc.r) + gg * (cc.c21 - pc.g)) + gb * (cc.c22 - pc.b));
            } else if constexpr (MODE == UV) {
                const PairColor pc = pair_color(q, h, CornerColor{});   // (its mu)
                UVTexel t = {};
                if (taken) uv_texel(uvf, pc, a.images + (size_t)b * a.image_stride, t);
                hh = (gr * (h.cr * t.r - R) + gg * (h.cg * t.g - G)) + gb * (h.cb * t.b - Bl);
                gcr += (W * gr) * t.r;    // the light colour's sums
                gcg += (W * gg) * t.g;
                gcb += (W * gb) * t.b;
                if (taken && uvf.H != 0) {
                    // the sample moves with wx1 and wy1 alone (the read indices carry no gradient): Tx, Ty per channel, then
                    // G_k = sum_c g_c L_c (Tx_c uvx_k (W - 1) + Ty_c uvy_k (H - 1)) and E_k = (W zp) (G_k - sum_j mu_j G_j)
                    const float ar = gr * h.cr, ag = gg * h.cg, ab = gb * h.cb;
                    const float txr = t.ax[2] * (t.i[2][0] - t.i[0][0]) + t.ax[3] * (t.i[3][0] - t.i[1][0]);
                    const float txg = t.ax[2] * (t.i[2][1] - t.i[0][1]) + t.ax[3] * (t.i[3][1] - t.i[1][1]);
                    const float txb = t.ax[2] * (t.i[2][2] - t.i[0][2]) + t.ax[3] * (t.i[3][2] - t.i[1][2]);
                    const float tyr = t.ax[0] * (t.i[1][0] - t.i[0][0]) + t.ax[1] * (t.i[3][0] - t.i[2][0]);
                    const float tyg = t.ax[0] * (t.i[1][1] - t.i[0][1]) + t.ax[1] * (t.i[3][1] - t.i[2][1]);
                    const float tyb = t.ax[0] * (t.i[1][2] - t.i[0][2]) + t.ax[1] * (t.i[3][2] - t.i[2][2]);
                    const float X = ((ar * txr + ag * txg) + ab * txb) * (float)(uvf.W - 1);
                    const float Y = ((ar * tyr + ag * tyg) + ab * tyb) * (float)(uvf.H - 1);
                    const float G0 = X * uvf.uv[0] + Y * uvf.uv[1], G1 = X * uvf.uv[2] + Y * uvf.uv[3];
                    const float G2 = X * uvf.uv[4] + Y * uvf.uv[5];
                    const float Gm = (pc.mu0 * G0 + pc.mu1 * G1) + pc.mu2 * G2, Wz = W * q.zp;
                    E0 = Wz * (G0 - Gm);
                    E1 = Wz * (G1 - Gm);
                    E2 = Wz * (G2 - Gm);
                    if (a.acc) {   // the image terms W g_c L_c w_r, formed and added in double; zero terms are skipped
                        double *acc = a.acc + (size_t)b * a.acc_stride;
                        const double gk[3] = {(double)W * ((double)gr * (double)h.cr), (double)W * ((double)gg * (double)h.cg),
                                              (double)W * ((double)gb * (double)h.cb)};
#pragma unroll
                        for (int rd = 0; rd < 4; rd++) {
                            double *at = acc + (size_t)t.q[rd] * 3;
#pragma unroll
                            for (int c = 0; c < 3; c++) {
                                const double term = gk[c] * (double)t.w[rd];
                                if (term != 0.0) atomicAdd(at + c, term);
                            }
                        }
                    }
                }
            } else if constexpr (MODE == CUBE) {
                const PairColor pc = pair_color(q, h, CornerColor{});   // (its mu)
                CubeTexel t = {};
                if (taken) cube_texel(cube, a.ts, a.hi, pc, t);
                hh = (gr * (h.cr * t.r - R) + gg * (h.cg * t.g - G)) + gb * (h.cb * t.b - Bl);
                gcr += (W * gr) * t.r;    // the light colour's sums
                gcg += (W * gg) * t.g;
                gcb += (W * gb) * t.b;
                if (taken) {
                    // the sample moves with fr alone (the cell carries no gradient, both clamps are taken with derivative 1):
                    // G_k = (ts - 1) sum_c g_c L_c D_kc and E_k = (W zp) (G_k - sum_j mu_j G_j)
                    const float ar = gr * h.cr, ag = gg * h.cg, ab = gb * h.cb, sc = (float)(a.ts - 1);
                    float d0[3], d1[3], d2[3];
                    cube_slopes(t, 0, d0);
                    cube_slopes(t, 1, d1);
                    cube_slopes(t, 2, d2);
                    const float G0 = ((ar * d0[0] + ag * d0[1]) + ab * d0[2]) * sc;
                    const float G1 = ((ar * d1[0] + ag * d1[1]) + ab * d1[2]) * sc;
                    const float G2 = ((ar * d2[0] + ag * d2[1]) + ab * d2[2]) * sc;
                    const float Gm = (pc.mu0 * G0 + pc.mu1 * G1) + pc.mu2 * G2, Wz = W * q.zp;
                    E0 = Wz * (G0 - Gm);
                    E1 = Wz * (G1 - Gm);
                    E2 = Wz * (G2 - Gm);
                }
                if (sums) {
                    // the cube terms (W g_c L_c) w_pn.  The taken pairs of this trip one after the other in ascending lane order:
                    // the pair's cell, fractions and three factors go to every lane, lane 3 pn + c forms tap pn's weight with the
                    // forward's own operations and adds channel c's term, an exact double product, to its entry.  A pair's eight
                    // taps are eight different texels, so no two lanes meet; a tap outside the cube is skipped as in the forward.
                    const float vr = (W * gr) * h.cr, vg = (W * gg) * h.cg, vb = (W * gb) * h.cb;
                    const int pn = lane / 3, ch = lane - pn * 3, T = T3 / 3;
                    unsigned long long todo = __ballot(taken);
                    while (todo != 0) {
                        const int src = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        const int c0 = bcast_i(t.i[0], src), c1 = bcast_i(t.i[1], src), c2 = bcast_i(t.i[2], src);
                        const float fr0 = bcast_f(t.fr[0], src), fr1 = bcast_f(t.fr[1], src), fr2 = bcast_f(t.fr[2], src);
                        const float v0 = bcast_f(vr, src), v1 = bcast_f(vg, src), v2 = bcast_f(vb, src);
                        if (lane < 24) {
                            float w = 1.0f;
                            w *= (pn & 1) ? fr0 : 1.0f - fr0;
                            w *= (pn & 2) ? fr1 : 1.0f - fr1;
                            w *= (pn & 4) ? fr2 : 1.0f - fr2;
                            const int flat = ((c0 + (pn & 1)) * a.ts + (c1 + ((pn >> 1) & 1))) * a.ts + (c2 + (pn >> 2));
                            const float v = ch == 0 ? v0 : (ch == 1 ? v1 : v2);
                            if (flat < T) sums[flat * 3 + ch] += (double)v * (double)w;
                        }
                        wave_lds_order();
                    }
                }
            } else {
                hh = (gr * (h.cr - R) + gg * (h.cg - G)) + gb * (h.cb - Bl);
                gcr += W * gr;
                gcg += W * gg;
                gcb += W * gb;
            }
            const float hW = hh * W;
            // x -> d2 -> the two ends of the chosen segment, as k_soft_backward
            float C = (hW * D1 + Ga * D) * a.inv_sigma;
            C = p.inside ? C : -C;
            const float t1 = 1.0f - p.t;
            const float ca = (-2.0f * t1) * C, cb = (-2.0f * p.t) * C;
            // zn -> zp -> iz
            const float diz = ((hW * a.inv_gamma) * a.inv_range) * (q.zp * q.zp);
            if constexpr (VARIES) {
                g0z += -((diz + E0) * q.l0) * s0;
                g1z += -((diz + E1) * q.l1) * s1;
                g2z += -((diz + E2) * q.l2) * s2;
            } else {
                g0z += -(diz * q.l0) * s0;
                g1z += -(diz * q.l1) * s1;
                g2z += -(diz * q.l2) * s2;
            }
            // iz -> x, y.  Outside, through a free t of segment a -> b: iz = (1 - t) / z_a + t / z_b, dt/da = (-(1 - t) e - r) / ee,
            // dt/db = (r - t e) / ee
            const int k = p.k;
            const float iza = k == 0 ? h.iz0 : (k == 1 ? h.iz1 : h.iz2), izb = k == 0 ? h.iz1 : (k == 1 ? h.iz2 : h.iz0);
            const float ex = k == 0 ? e0x : (k == 1 ? e1x : e2x), ey = k == 0 ? e0y : (k == 1 ? e1y : e2y);
            const float ee = k == 0 ? ee0 : (k == 1 ? ee1 : ee2);
            const bool free_t = !p.inside && p.t > 0.0f && p.t < 1.0f;
            float T;
            if constexpr (VARIES) {   // ... and the colour moves along the segment with t
                const float Ea = k == 0 ? E0 : (k == 1 ? E1 : E2), Eb = k == 0 ? E1 : (k == 1 ? E2 : E0);
                T = free_t ? (diz * (izb - iza) + (Eb * izb - Ea * iza)) / ee : 0.0f;
            } else {
                T = free_t ? (diz * (izb - iza)) / ee : 0.0f;
            }
            const float ra = ca - T, rb = cb + T, ea = -(t1 * T), eb = -(p.t * T);
            const float ax = ra * p.rx + ea * ex, ay = ra * p.ry + ea * ey;
            const float bx = rb * p.rx + eb * ex, by = rb * p.ry + eb * ey;
            // inside, through lambda: d iz / d c_j = (iz of the vertex that c_j weighs - iz) / A, and c_j moves with its two ends
            const float dA = p.inside ? diz * q.rA : 0.0f;
            float q0 = dA * (h.iz2 - q.iz), q1 = dA * (h.iz0 - q.iz), q2 = dA * (h.iz1 - q.iz);
            if constexpr (VARIES) {   // ... and the colour with lambda: c_j weighs vertex v(j) = 2, 0, 1
                const float rA = p.inside ? q.rA : 0.0f;
                q0 += (E2 * h.iz2) * rA;
                q1 += (E0 * h.iz0) * rA;
                q2 += (E1 * h.iz1) * rA;
            }
            const float p0x = px - s.x0, p0y = py - s.y0, p1x = px - s.x1, p1y = py - s.y1, p2x = px - s.x2, p2y = py - s.y2;
            g0x += (k == 0 ? ax : (k == 2 ? bx : 0.0f)) + (q2 * p2y - q0 * p1y);
            g0y += (k == 0 ? ay : (k == 2 ? by : 0.0f)) + (q0 * p1x - q2 * p2x);
            g1x += (k == 1 ? ax : (k == 0 ? bx : 0.0f)) + (q0 * p0y - q1 * p2y);
            g1y += (k == 1 ? ay : (k == 0 ? by : 0.0f)) + (q1 * p2x - q0 * p0x);
            g2x += (k == 2 ? ax : (k == 1 ? bx : 0.0f)) + (q1 * p1y - q2 * p0y);
            g2y += (k == 2 ? ay : (k == 1 ? by : 0.0f)) + (q2 * p0x - q1 * p1x);
        }
    }
    g0x = wave_sum(g0x); g0y = wave_sum(g0y); g0z = wave_sum(g0z);
    g1x = wave_sum(g1x); g1y = wave_sum(g1y); g1z = wave_sum(g1z);
    g2x = wave_sum(g2x); g2y = wave_sum(g2y); g2z = wave_sum(g2z);
    gcr = wave_sum(gcr); gcg = wave_sum(gcg); gcb = wave_sum(gcb);
    if constexpr (CORNERS) {
        g1r = wave_sum(g1r); g1g = wave_sum(g1g); g1b = wave_sum(g1b);
        g2r = wave_sum(g2r); g2g = wave_sum(g2g); g2b = wave_sum(g2b);
    }
    if (lane == 0) {
        float *o = grad_faces + ((size_t)b * F + f) * 9;
        o[0] = g0x; o[1] = g0y; o[2] = g0z;
        o[3] = g1x; o[4] = g1y; o[5] = g1z;
        o[6] = g2x; o[7] = g2y; o[8] = g2z;
        float *c = grad_colors + ((size_t)b * F + f) * (CORNERS ? 9 : 3);
        c[0] = gcr; c[1] = gcg; c[2] = gcb;
        if constexpr (CORNERS) {
            c[3] = g1r; c[4] = g1g; c[5] = g1b;
            c[6] = g2r; c[7] = g2g; c[8] = g2b;
        }
    }
    if constexpr (MODE == CUBE) {   // every entry of the face's cube stored, each sum rounded once; zeros for a dropped face
        if (sums) {
            float *o = a.grad + ((size_t)b * F + f) * T3;
            for (int e = lane; e < T3; e += WAVE) o[e] = (float)sums[e];
        }
    }
}

// shared colours: the B partial gradients of an entry in ascending b, in double, rounded once
__global__ __launch_bounds__(256) void k_render_colors(const float *__restrict__ part, float *__restrict__ grad_colors, int B,
                                                       int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    for (int b = 0; b < B; b++) sum += (double)part[(size_t)b * n + i];
    grad_colors[i] = (float)sum;
}

// --------------------------------------------------------------------------------------------------------------------
// host

// corners = 0: one colour per face, 1: one per corner
size_t render_records(int B, int F, int corners)
{
    return (size_t)B * (size_t)F * (corners ? CORNER_REC : RENDER_REC) * sizeof(float4);
}

// the records, then the per-image colour gradients of a call with shared colours
size_t render_workspace(int B, int F, int corners)
{
    return render_records(B, F, corners) + align_up((size_t)B * (size_t)F * (corners ? 9 : 3) * sizeof(float), 16);
}

struct RenderCall {
    const float *faces, *colors;
    int B, F, S, colors_per_batch;
    double sigma, gamma, near, far, eps;
    const double *bg;
    void *workspace;
    size_t workspace_bytes;
    int corners;
};

int render_check(const RenderCall &c)
{
    if (!c.faces || !c.colors) return NR_E_NULL;
    if (!soft_sizes_ok(c.B, c.F, c.S)) return NR_E_SIZE;
    const auto finite = [](double v) { return v - v == 0.0; };
    if (!(c.sigma >= 1.0e-30 && c.sigma <= 1.0e30) || !(c.gamma >= 1.0e-30 && c.gamma <= 1.0e30)) return NR_E_MODE;
    if (!finite(c.near) || !finite(c.far) || !(c.far > c.near) || !finite(c.eps)) return NR_E_MODE;
    if (!finite(c.bg[0]) || !finite(c.bg[1]) || !finite(c.bg[2])) return NR_E_MODE;
    if (c.colors_per_batch != 0 && c.colors_per_batch != 1) return NR_E_MODE;
    if (!c.workspace || c.workspace_bytes < render_workspace(c.B, c.F, c.corners)) return NR_E_WORKSPACE;
    return 0;
}

RenderArgs render_args(const RenderCall &c)
{
    RenderArgs a;
    a.inv_sigma = (float)(1.0 / c.sigma);
    a.inv_gamma = (float)(1.0 / c.gamma);
    a.cut = (float)((double)SOFT_REACH * c.sigma);
    a.far = (float)c.far;
    a.inv_range = (float)(1.0 / (c.far - c.near));
    a.eps = (float)c.eps;
    a.bg_r = (float)c.bg[0]; a.bg_g = (float)c.bg[1]; a.bg_b = (float)c.bg[2];
    return a;
}

template <bool CORNERS>
int render_setup(const RenderCall &c, hipStream_t st)
{
    hipLaunchKernelGGL(k_render_setup<CORNERS>, dim3((unsigned)((c.F + 255) / 256), (unsigned)c.B), dim3(256), 0, st, c.faces,
                       c.colors, (float4 *)c.workspace, c.F, c.S, c.colors_per_batch ? (size_t)c.F * (CORNERS ? 9 : 3) : (size_t)0,
                       soft_reach(c.sigma), c.near, c.far);
    return launch_status();
}

template <bool CORNERS>
int render_forward(const RenderCall &c, float *rgba, float *transmittance, float *normaliser, void *stream)
{
    if (!rgba || !transmittance || !normaliser) return NR_E_NULL;
    if (int e = render_check(c)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = render_setup<CORNERS>(c, st)) return rc;
    const int tiles = (c.S + SOFT_TILE - 1) / SOFT_TILE;
    hipLaunchKernelGGL(k_render_forward<CORNERS>, dim3((unsigned)(tiles * tiles), (unsigned)c.B), dim3(256), 0, st,
                       (const float4 *)c.workspace, rgba, transmittance, normaliser, c.F, c.S, tiles, render_args(c));
    return launch_status();
}

template <bool CORNERS>
int render_backward(const RenderCall &c, const float *rgba, const float *transmittance, const float *normaliser,
                    const float *grad_rgba, float *grad_faces, float *grad_colors, void *stream)
{
    if (!rgba || !transmittance || !normaliser || !grad_rgba || !grad_faces || !grad_colors) return NR_E_NULL;
    if (int e = render_check(c)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = render_setup<CORNERS>(c, st)) return rc;   // the caller's workspace holds nothing
    float *part = c.colors_per_batch ? grad_colors : (float *)((char *)c.workspace + render_records(c.B, c.F, c.corners));
    hipLaunchKernelGGL(k_render_backward<CORNERS>, dim3((unsigned)((c.F + 3) / 4), (unsigned)c.B), dim3(256), 0, st,
                       (const float4 *)c.workspace, rgba, transmittance, normaliser, grad_rgba, grad_faces, part, c.F, c.S,
                       render_args(c));
    if (int rc = launch_status()) return rc;
    if (!c.colors_per_batch) {
        const int n = c.F * (CORNERS ? 9 : 3);
        hipLaunchKernelGGL(k_render_colors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, grad_colors, c.B, n);
    }
    return launch_status();
}

// UV images: the double sums of the image gradient -> grad_images, each rounded once
__global__ __launch_bounds__(256) void k_uv_image_round(const double *__restrict__ acc, float *__restrict__ grad_images, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) grad_images[i] = (float)acc[i];
}

// the workspace of the UV entries: the records, the per-image light gradients of a call with shared light, the double sums
struct UVWorkspace {
    size_t part_off, acc_off, acc_bytes, total;
};

UVWorkspace uv_workspace(int B, int F, int P, int image_batch)
{
    UVWorkspace w;
    w.part_off = (size_t)B * (size_t)F * UV_REC * sizeof(float4);
    w.acc_off = align_up(w.part_off + (size_t)B * (size_t)F * 3 * sizeof(float), 256);
    w.acc_bytes = (size_t)image_batch * (size_t)P * 3 * sizeof(double);
    w.total = w.acc_off + w.acc_bytes;
    return w;
}

// render_check's codes in render_check's order, with uv_images_args' checks (nr_forward.hip) in front of the workspace's
int uv_check(const nr_uv_images *uv, const RenderCall &c, UVShade &us)
{
    if (!uv || !c.faces || !c.colors) return NR_E_NULL;
    if (!soft_sizes_ok(c.B, c.F, c.S)) return NR_E_SIZE;
    const nr_face_light lit = {c.colors, c.F, nullptr, nullptr};
    FaceLight fl;
    if (int e = uv_images_args(&lit, uv, c.B, c.F, fl, us)) return e;
    if ((size_t)uv->image_batch * (size_t)uv->num_pixels * 3 > 0xffffff00ull) return NR_E_SIZE;   // (k_uv_image_round's 1-D grid)
    RenderCall flat = c;   // the numbers; the flat workspace is the smaller one
    flat.workspace_bytes = c.workspace ? render_workspace(c.B, c.F, 0) : 0;
    if (int e = render_check(flat)) return e;
    if (c.workspace_bytes < uv_workspace(c.B, c.F, uv->num_pixels, uv->image_batch).total) return NR_E_WORKSPACE;
    return 0;
}

UVArgs uv_args(const RenderCall &c, const UVShade &us, double *acc)
{
    UVArgs a;
    static_cast<RenderArgs &>(a) = render_args(c);
    a.images = us.images;
    a.image_stride = us.shared ? 0 : (size_t)us.P * 3;
    a.acc = acc;
    a.acc_stride = a.image_stride;
    return a;
}

int uv_setup(const RenderCall &c, const UVShade &us, hipStream_t st)
{
    hipLaunchKernelGGL(k_uv_setup, dim3((unsigned)((c.F + 255) / 256), (unsigned)c.B), dim3(256), 0, st, c.faces, c.colors, us,
                       (float4 *)c.workspace, c.F, c.S, c.colors_per_batch ? (size_t)c.F * 3 : (size_t)0, soft_reach(c.sigma),
                       c.near, c.far);
    return launch_status();
}

int uv_forward(const nr_uv_images *uv, const RenderCall &c, float *rgba, float *transmittance, float *normaliser, void *stream)
{
    if (!rgba || !transmittance || !normaliser) return NR_E_NULL;
    UVShade us;
    if (int e = uv_check(uv, c, us)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = uv_setup(c, us, st)) return rc;
    const int tiles = (c.S + SOFT_TILE - 1) / SOFT_TILE;
    hipLaunchKernelGGL(k_render_forward<UV>, dim3((unsigned)(tiles * tiles), (unsigned)c.B), dim3(256), 0, st,
                       (const float4 *)c.workspace, rgba, transmittance, normaliser, c.F, c.S, tiles, uv_args(c, us, nullptr));
    return launch_status();
}

int uv_backward(const nr_uv_images *uv, const RenderCall &c, const float *rgba, const float *transmittance,
                const float *normaliser, const float *grad_rgba, float *grad_faces, float *grad_light, float *grad_images,
                void *stream)
{
    if (!rgba || !transmittance || !normaliser || !grad_rgba || !grad_faces || !grad_light) return NR_E_NULL;
    UVShade us;
    if (int e = uv_check(uv, c, us)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = uv_setup(c, us, st)) return rc;   // the caller's workspace holds nothing
    const UVWorkspace w = uv_workspace(c.B, c.F, us.P, uv->image_batch);
    double *acc = grad_images ? (double *)((char *)c.workspace + w.acc_off) : nullptr;
    if (acc)
        if (int he = fill_bytes(acc, 0, w.acc_bytes, st)) return he;   // (nr_device.h: not a memset node)
    float *part = c.colors_per_batch ? grad_light : (float *)((char *)c.workspace + w.part_off);
    hipLaunchKernelGGL(k_render_backward<UV>, dim3((unsigned)((c.F + 3) / 4), (unsigned)c.B), dim3(256), 0, st,
                       (const float4 *)c.workspace, rgba, transmittance, normaliser, grad_rgba, grad_faces, part, c.F, c.S,
                       uv_args(c, us, acc));
    if (int rc = launch_status()) return rc;
    if (!c.colors_per_batch) {
        const int n = c.F * 3;
        hipLaunchKernelGGL(k_render_colors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, grad_light, c.B, n);
        if (int rc = launch_status()) return rc;
    }
    if (acc) {
        const size_t n = w.acc_bytes / sizeof(double);
        hipLaunchKernelGGL(k_uv_image_round, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc, grad_images, n);
    }
    return launch_status();
}

// the workspace of the cube entries: the records, the per-image light gradients of a call with shared light, the per-image
// cube gradients of a call with shared cubes
struct CubeWorkspace {
    size_t light_off, cubes_off, total;
};

CubeWorkspace cube_workspace(int B, int F, int ts, int textures_per_batch)
{
    CubeWorkspace w;
    w.light_off = (size_t)B * (size_t)F * RENDER_REC * sizeof(float4);
    w.cubes_off = align_up(w.light_off + (size_t)B * (size_t)F * 3 * sizeof(float), 256);
    w.total = w.cubes_off + (textures_per_batch ? 0 : (size_t)B * (size_t)F * (size_t)(ts * ts * ts * 3) * sizeof(float));
    return w;
}

bool cube_sizes_ok(int B, int F, int S, int ts)
{
    // (F ts^3 3 is k_render_colors' int n)
    return soft_sizes_ok(B, F, S) && ts >= CUBE_MIN_TS && ts <= CUBE_MAX_TS && (size_t)F * (size_t)(ts * ts * ts * 3) <= 0x7fffff00ull;
}

struct CubeCall {
    const float *textures;
    int ts, textures_per_batch;
    double texture_eps;
};

// render_check's codes in render_check's order, the texture size with the sizes and texture_eps with the numbers
int cube_check(const CubeCall &t, const RenderCall &c)
{
    if (!t.textures || !c.faces || !c.colors) return NR_E_NULL;
    if (!cube_sizes_ok(c.B, c.F, c.S, t.ts)) return NR_E_SIZE;
    RenderCall flat = c;   // the numbers; the flat workspace is the smaller one
    flat.workspace_bytes = c.workspace ? render_workspace(c.B, c.F, 0) : 0;
    const int e = render_check(flat);
    if (e != 0 && e != NR_E_WORKSPACE) return e;
    if (!(t.texture_eps >= 0.0 && t.texture_eps < 1.0)) return NR_E_MODE;
    if (t.textures_per_batch != 0 && t.textures_per_batch != 1) return NR_E_MODE;
    if (e != 0 || c.workspace_bytes < cube_workspace(c.B, c.F, t.ts, t.textures_per_batch).total) return NR_E_WORKSPACE;
    return 0;
}

CubeArgs cube_args(const CubeCall &t, const RenderCall &c, float *grad)
{
    CubeArgs a;
    static_cast<RenderArgs &>(a) = render_args(c);
    a.cubes = t.textures;
    a.cube_stride = t.textures_per_batch ? (size_t)c.F * (size_t)(t.ts * t.ts * t.ts * 3) : (size_t)0;
    a.ts = t.ts;
    a.hi = (double)(t.ts - 1) - t.texture_eps;
    a.grad = grad;
    return a;
}

int cube_setup(const RenderCall &c, hipStream_t st)
{
    hipLaunchKernelGGL(k_cube_setup, dim3((unsigned)((c.F + 255) / 256), (unsigned)c.B), dim3(256), 0, st, c.faces, c.colors,
                       (float4 *)c.workspace, c.F, c.S, c.colors_per_batch ? (size_t)c.F * 3 : (size_t)0, soft_reach(c.sigma),
                       c.near, c.far);
    return launch_status();
}

int cube_forward(const CubeCall &t, const RenderCall &c, float *rgba, float *transmittance, float *normaliser, void *stream)
{
    if (!rgba || !transmittance || !normaliser) return NR_E_NULL;
    if (int e = cube_check(t, c)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = cube_setup(c, st)) return rc;
    const int tiles = (c.S + SOFT_TILE - 1) / SOFT_TILE;
    hipLaunchKernelGGL(k_render_forward<CUBE>, dim3((unsigned)(tiles * tiles), (unsigned)c.B), dim3(256), 0, st,
                       (const float4 *)c.workspace, rgba, transmittance, normaliser, c.F, c.S, tiles, cube_args(t, c, nullptr));
    return launch_status();
}

int cube_backward(const CubeCall &t, const RenderCall &c, const float *rgba, const float *transmittance, const float *normaliser,
                  const float *grad_rgba, float *grad_faces, float *grad_light, float *grad_textures, void *stream)
{
    if (!rgba || !transmittance || !normaliser || !grad_rgba || !grad_faces || !grad_light) return NR_E_NULL;
    if (int e = cube_check(t, c)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = cube_setup(c, st)) return rc;   // the caller's workspace holds nothing
    const CubeWorkspace w = cube_workspace(c.B, c.F, t.ts, t.textures_per_batch);
    const int T3 = t.ts * t.ts * t.ts * 3;
    float *part_light = c.colors_per_batch ? grad_light : (float *)((char *)c.workspace + w.light_off);
    float *part_cubes = !grad_textures ? nullptr : (t.textures_per_batch ? grad_textures : (float *)((char *)c.workspace + w.cubes_off));
    // the cube sums: ts^3 * 3 doubles per wave, four waves
    hipLaunchKernelGGL(k_render_backward<CUBE>, dim3((unsigned)((c.F + 3) / 4), (unsigned)c.B), dim3(256),
                       (size_t)4 * T3 * sizeof(double), st, (const float4 *)c.workspace, rgba, transmittance, normaliser,
                       grad_rgba, grad_faces, part_light, c.F, c.S, cube_args(t, c, part_cubes));
    if (int rc = launch_status()) return rc;
    if (!c.colors_per_batch) {
        const int n = c.F * 3;
        hipLaunchKernelGGL(k_render_colors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part_light, grad_light, c.B, n);
        if (int rc = launch_status()) return rc;
    }
    if (part_cubes && !t.textures_per_batch) {
        const int n = c.F * T3;
        hipLaunchKernelGGL(k_render_colors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part_cubes, grad_textures, c.B, n);
    }
    return launch_status();
}

}  // namespace

NR_API size_t nr_soft_cubes_workspace_bytes(int32_t B, int32_t F, int32_t S, int32_t ts, int32_t textures_per_batch)
{
    if (!cube_sizes_ok(B, F, S, ts) || (textures_per_batch != 0 && textures_per_batch != 1)) return 0;
    return cube_workspace(B, F, ts, textures_per_batch).total;
}

NR_API int nr_soft_cubes_forward(const float *faces, const float *textures, const float *light, float *rgba, float *transmittance,
                                 float *normaliser, int32_t B, int32_t F, int32_t S, int32_t ts, int32_t textures_per_batch,
                                 int32_t light_per_batch, double sigma, double gamma, double near, double far, double eps,
                                 double background_r, double background_g, double background_b, double texture_eps,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, light, B, F, S, light_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 0};
    const CubeCall t = {textures, ts, textures_per_batch, texture_eps};
    return cube_forward(t, c, rgba, transmittance, normaliser, stream);
}

NR_API int nr_soft_cubes_backward(const float *faces, const float *textures, const float *light, const float *rgba,
                                  const float *transmittance, const float *normaliser, const float *grad_rgba, float *grad_faces,
                                  float *grad_light, float *grad_textures, int32_t B, int32_t F, int32_t S, int32_t ts,
                                  int32_t textures_per_batch, int32_t light_per_batch, double sigma, double gamma, double near,
                                  double far, double eps, double background_r, double background_g, double background_b,
                                  double texture_eps, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, light, B, F, S, light_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 0};
    const CubeCall t = {textures, ts, textures_per_batch, texture_eps};
    return cube_backward(t, c, rgba, transmittance, normaliser, grad_rgba, grad_faces, grad_light, grad_textures, stream);
}

NR_API size_t nr_soft_uv_workspace_bytes(const nr_uv_images *uv, int32_t B, int32_t F, int32_t S)
{
    if (!uv || !soft_sizes_ok(B, F, S) || uv->num_pixels < 1 || uv->num_pixels > 0x7ffffffe ||
        (uv->image_batch != 1 && uv->image_batch != B))
        return 0;
    return uv_workspace(B, F, uv->num_pixels, uv->image_batch).total;
}

NR_API int nr_soft_uv_forward(const nr_uv_images *uv, const float *faces, const float *light, float *rgba, float *transmittance,
                              float *normaliser, int32_t B, int32_t F, int32_t S, int32_t light_per_batch, double sigma,
                              double gamma, double near, double far, double eps, double background_r, double background_g,
                              double background_b, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, light, B, F, S, light_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 0};
    return uv_forward(uv, c, rgba, transmittance, normaliser, stream);
}

NR_API int nr_soft_uv_backward(const nr_uv_images *uv, const float *faces, const float *light, const float *rgba,
                               const float *transmittance, const float *normaliser, const float *grad_rgba, float *grad_faces,
                               float *grad_light, float *grad_images, int32_t B, int32_t F, int32_t S, int32_t light_per_batch,
                               double sigma, double gamma, double near, double far, double eps, double background_r,
                               double background_g, double background_b, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, light, B, F, S, light_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 0};
    return uv_backward(uv, c, rgba, transmittance, normaliser, grad_rgba, grad_faces, grad_light, grad_images, stream);
}

NR_API size_t nr_soft_render_workspace_bytes(int32_t B, int32_t F, int32_t S)
{
    return soft_sizes_ok(B, F, S) ? render_workspace(B, F, 0) : 0;
}

NR_API int nr_soft_render_forward(const float *faces, const float *colors, float *rgba, float *transmittance, float *normaliser,
                                  int32_t B, int32_t F, int32_t S, int32_t colors_per_batch, double sigma, double gamma,
                                  double near, double far, double eps, double background_r, double background_g,
                                  double background_b, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, colors, B, F, S, colors_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 0};
    return render_forward<false>(c, rgba, transmittance, normaliser, stream);
}

NR_API int nr_soft_render_backward(const float *faces, const float *colors, const float *rgba, const float *transmittance,
                                   const float *normaliser, const float *grad_rgba, float *grad_faces, float *grad_colors,
                                   int32_t B, int32_t F, int32_t S, int32_t colors_per_batch, double sigma, double gamma,
                                   double near, double far, double eps, double background_r, double background_g,
                                   double background_b, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, colors, B, F, S, colors_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 0};
    return render_backward<false>(c, rgba, transmittance, normaliser, grad_rgba, grad_faces, grad_colors, stream);
}

NR_API size_t nr_soft_corners_workspace_bytes(int32_t B, int32_t F, int32_t S)
{
    return soft_sizes_ok(B, F, S) ? render_workspace(B, F, 1) : 0;
}

NR_API int nr_soft_corners_forward(const float *faces, const float *colors, float *rgba, float *transmittance, float *normaliser,
                                   int32_t B, int32_t F, int32_t S, int32_t colors_per_batch, double sigma, double gamma,
                                   double near, double far, double eps, double background_r, double background_g,
                                   double background_b, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, colors, B, F, S, colors_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 1};
    return render_forward<true>(c, rgba, transmittance, normaliser, stream);
}

NR_API int nr_soft_corners_backward(const float *faces, const float *colors, const float *rgba, const float *transmittance,
                                    const float *normaliser, const float *grad_rgba, float *grad_faces, float *grad_colors,
                                    int32_t B, int32_t F, int32_t S, int32_t colors_per_batch, double sigma, double gamma,
                                    double near, double far, double eps, double background_r, double background_g,
                                    double background_b, void *workspace, size_t workspace_bytes, void *stream)
{
    const double bg[3] = {background_r, background_g, background_b};
    const RenderCall c = {faces, colors, B, F, S, colors_per_batch, sigma, gamma, near, far, eps, bg, workspace, workspace_bytes, 1};
    return render_backward<true>(c, rgba, transmittance, normaliser, grad_rgba, grad_faces, grad_colors, stream);
}
