// nr_device.h -- device helpers shared by the gfx950 kernels of libnr_hip.so.
//
// Numerics contract (DESIGN.md "Numerics"): float32 IEEE arithmetic in the operation order of the reference
// source (neural_renderer/rasterize.py), double promotion where the reference's CUDA text has a double
// literal, NO multiply-add contraction (-ffp-contract=off), correctly rounded division.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/nr_hip.h"

#define NR_API extern "C" __attribute__((visibility("default")))

namespace nr {

constexpr int WAVE = 64;

// --------------------------------------------------------------------------------------------------
// shared device helpers

// back-face test: rasterize.py:252 / :306 / :540
__device__ __forceinline__ bool is_backside(float x0, float y0, float x1, float y1, float x2, float y2)
{
    return (y2 - y0) * (x1 - x0) < (y1 - y0) * (x2 - x0);
}

// NDC -> pixel units: 0.5 * (v * is + is - 1), rasterize.py:258 / :549 (the 0.5 scaling is exact in f32)
__device__ __forceinline__ float to_pixel(float v, float fs) { return 0.5f * (v * fs + fs - 1.0f); }

// inverse of [[p0x,p1x,p2x],[p0y,p1y,p2y],[1,1,1]]: rasterize.py:261-269
__device__ __forceinline__ void compute_face_inv(const float px[3], const float py[3], float inv[9])
{
    inv[0] = py[1] - py[2];
    inv[1] = px[2] - px[1];
    inv[2] = px[1] * py[2] - px[2] * py[1];
    inv[3] = py[2] - py[0];
    inv[4] = px[0] - px[2];
    inv[5] = px[2] * py[0] - px[0] * py[2];
    inv[6] = py[0] - py[1];
    inv[7] = px[1] - px[0];
    inv[8] = px[0] * py[1] - px[1] * py[0];
    const float den = px[2] * (py[0] - py[1]) + px[0] * (py[1] - py[2]) + px[1] * (py[2] - py[0]);
#pragma unroll
    for (int k = 0; k < 9; k++) inv[k] /= den;
}

// pixel centre in NDC: (2. * i + 1 - is) / is evaluated in double, rasterize.py:291-292
__device__ __forceinline__ float pixel_center(int i, int S) { return (float)((2.0 * i + 1 - S) / S); }

// (wave_sum, wave_incl_scan and the other fixed-order sums and scans: nr_reduce.h, included below)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int bcast_i(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float bcast_f(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}


// --------------------------------------------------------------------------------------------------
// Candidate pixels of a face: the only pixels the forward needs to test and the backward gathers need to scan (they MUST
// agree: a pixel the forward could give to a face has to be among the candidates the backward visits).
//   * none: back faces (rasterize.py:306), off-screen faces, faces whose three vertices coincide (their barycentric weights
//     are NaN for every pixel, so `zp < depth_min` never holds, :322-334);
//   * a BOX: the exact pixel range of the triangle plus a guard band of BBOX_GUARD pixels -- the inside test (:310-312) runs
//     on rounded NDC floats, whose rounding moves an edge by ~1e-6 pixel, so 0.25 pixel is conservative;
//   * a STRIP along the longest edge for needles and degenerate (collinear) faces.  The inside test compares rounded
//     products of NDC differences; its rounding error is a relative 2^-22 or so of |p - a| * |b - a|, i.e. every edge line is
//     accepted within an ANGLE of ~5e-7 rad at any distance.  Beyond a vertex whose interior angle is below twice that, the
//     wedges of the two adjacent edges overlap and the reference accepts pixels far outside the triangle, along its axis
//     (found by fuzzing: micro-triangles of a few ulps through pixel centres).  Faces that thin -- 2 * area <= 2^-18 *
//     (longest edge)^2 in NDC, the coordinates the test works with -- lie within 4e-6 of their longest edge's line, and so does
//     everything the test can accept: the candidates are the STRIP_W pixels around that line in every row (or column);
//   * the whole image when nothing better can be said (non-finite or astronomically large coordinates).
struct Cand {
    int x_lo, y_lo, bw;  // box: origin and width
    int n;               // number of candidates, 0 = none
    int strip;           // 0 box, 1 strip stepping through rows (x = a * y + b), 2 strip stepping through columns
    float a, b;
};
constexpr float BBOX_GUARD = 0.25f;
constexpr int STRIP_W = 4;  // floor(line) - 1 .. floor(line) + 2

__device__ __forceinline__ Cand face_candidates(float x0, float y0, float x1, float y1, float x2, float y2, int S)
{
    Cand c;
    c.x_lo = c.y_lo = 0; c.bw = 1; c.n = 0; c.strip = 0; c.a = c.b = 0.0f;
    if (is_backside(x0, y0, x1, y1, x2, y2)) return c;
    if ((x0 == x1) && (x1 == x2) && (y0 == y1) && (y1 == y2)) return c;
    const float fs = (float)S;
    const float px[3] = {to_pixel(x0, fs), to_pixel(x1, fs), to_pixel(x2, fs)};
    const float py[3] = {to_pixel(y0, fs), to_pixel(y1, fs), to_pixel(y2, fs)};
    const float den = px[2] * (py[0] - py[1]) + px[0] * (py[1] - py[2]) + px[1] * (py[2] - py[0]);
    const float e0x = x1 - x0, e0y = y1 - y0, e1x = x2 - x1, e1y = y2 - y1, e2x = x0 - x2, e2y = y0 - y2;
    const float area2 = fabsf(e0x * e1y - e0y * e1x);
    const float l0 = e0x * e0x + e0y * e0y, l1 = e1x * e1x + e1y * e1y, l2 = e2x * e2x + e2y * e2y;
    const float len2 = fmaxf(fmaxf(l0, l1), l2);
    const bool thin = !(area2 > 0x1p-18f * len2) || !(fabsf(den) > 0.0f);
    const float big = 1.0e6f;  // pixel coordinates beyond this make the strip arithmetic meaningless
    const bool wild = !(len2 < __builtin_inff()) || !(fabsf(den) < __builtin_inff()) ||
                      !(fmaxf(fmaxf(fabsf(px[0]), fabsf(px[1])), fabsf(px[2])) < big) ||
                      !(fmaxf(fmaxf(fabsf(py[0]), fabsf(py[1])), fabsf(py[2])) < big);
    // A face is "thin" relative to its longest edge; with vertices far off-screen (a perspective division by z near 0) that
    // edge can be 10^5 pixels long and the face still several pixels high on screen.  The 4-pixel strip is only conservative
    // while 2^-18 * (longest edge in pixels) stays below half a pixel; beyond that the whole image is the candidate set.
    const bool strip_ok = len2 * fs * fs * 0.25f * 0x1p-36f <= 0.25f;
    if (thin && !wild && strip_ok) {
        // the longest edge: its direction from the NDC differences (exact for close vertices -- in pixel units a
        // micro-triangle's edge would be a few ulps of noise), its position from one endpoint in pixel units
        const int k = (l0 >= l1 && l0 >= l2) ? 0 : (l1 >= l2 ? 1 : 2);
        const float ax = px[k], ay = py[k];
        const float dx = k == 0 ? e0x : (k == 1 ? e1x : e2x), dy = k == 0 ? e0y : (k == 1 ? e1y : e2y);
        if (fabsf(dy) >= fabsf(dx) && dy != 0.0f) {
            c.strip = 1; c.a = dx / dy; c.b = ax - c.a * ay;
        } else if (dx != 0.0f) {
            c.strip = 2; c.a = dy / dx; c.b = ay - c.a * ax;
        }
        if (c.strip) { c.n = S * STRIP_W; return c; }
    }
    if (thin || wild) {  // the whole image
        c.bw = S; c.n = S * S;
        return c;
    }
    const float xmin = fminf(fminf(px[0], px[1]), px[2]), xmax = fmaxf(fmaxf(px[0], px[1]), px[2]);
    const float ymin = fminf(fminf(py[0], py[1]), py[2]), ymax = fmaxf(fmaxf(py[0], py[1]), py[2]);
    const float lo_c = -2.0f, hi_c = (float)S + 1.0f;  // clamp before the int conversion
    const int xl = max((int)ceilf(fminf(fmaxf(xmin - BBOX_GUARD, lo_c), hi_c)), 0);
    const int xh = min((int)floorf(fminf(fmaxf(xmax + BBOX_GUARD, lo_c), hi_c)), S - 1);
    const int yl = max((int)ceilf(fminf(fmaxf(ymin - BBOX_GUARD, lo_c), hi_c)), 0);
    const int yh = min((int)floorf(fminf(fmaxf(ymax + BBOX_GUARD, lo_c), hi_c)), S - 1);
    if (xl <= xh && yl <= yh) {
        c.x_lo = xl; c.y_lo = yl; c.bw = xh - xl + 1; c.n = c.bw * (yh - yl + 1);
    }
    return c;
}

// i-th candidate -> pixel (x, y); false when it falls outside the image (strips only)
__device__ __forceinline__ bool cand_pixel(const Cand &c, int i, int S, int &x, int &y)
{
    if (c.strip == 0) {
        const int yy = i / c.bw;
        x = c.x_lo + (i - yy * c.bw);
        y = c.y_lo + yy;
        return true;
    }
    const int m = i / STRIP_W, j = i - m * STRIP_W;
    const int o = (int)floorf(c.a * (float)m + c.b) - 1 + j;
    if (c.strip == 1) { y = m; x = o; } else { x = m; y = o; }
    return o >= 0 && o < S;
}

// --------------------------------------------------------------------------------------------------
// Per-face light colours (nr_face_light in include/nr_hip.h): instead of textures that were multiplied by the
// light colour of their face and duplicated for the fill_back copy in front of the rasterizer (lighting.py:50-51,
// renderer.py:79: 2 x B x Nf x ts^3 x 3 floats written, read, and the same again for the gradient), the kernels read the
// ORIGINAL cubes [B, tex_faces, ts^3, 3] and multiply the sampled colour by light[b, f, :].  Face f >= tex_faces is the
// reversed copy of face f - tex_faces and reads its cube with the first and the third axis exchanged.
struct FaceLight {
    const float *light = nullptr;     // [B, F, 3]; NULL = off: textures are [B, F, ts^3, 3], sampled as they are
    int tex_faces = 0;                // Nf (F == Nf or F == 2 * Nf)
    const float *textures = nullptr;  // backward only: the cubes, for the gradient of `light`
    float *grad_light = nullptr;      // backward only: [B, F, 3] or NULL
};

// texel (i, j, k) -> (k, j, i) of a ts^3 cube, flattened (renderer.py:79)
__device__ __forceinline__ int transpose_texel(int t, int ts)
{
    const int k = t % ts, j = (t / ts) % ts, i = t / (ts * ts);
    return (k * ts + j) * ts + i;
}

// texture taps shared by F3 (forward) and B2 (backward recompute): rasterize.py:398-425
struct Taps {
    int isc[8];
    float w[8];
};

// The eight trilinear taps of a pixel (rasterize.py:398-421).  When an index float reaches ts - 1 exactly (eps too small to
// survive the float32 rounding of :402, or eps = 0) the "upper" corner of that dimension has index ts and weight exactly 0;
// its flattened index can then leave the face's cube (isc >= ts^3).  The reference multiplies whatever lies there by 0 /
// adds 0 to it; consumers here skip such taps instead of touching memory outside the cube.
// z: the face's three vertex depths; flip: flatten the taps of the cube with axes 0 and 2 exchanged (FaceLight: the
// reversed copy of a face reads the original cube transposed)
__device__ __forceinline__ void compute_taps(const float *__restrict__ z, const float *__restrict__ weight,
                                             float depth, int ts, double eps, Taps &t, bool flip = false)
{
    float tif[3];
    int ti[3];
    float fr[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v = weight[k] * (float)(ts - 1) * (depth / z[k]);  // :400
        v = fmaxf(v, 0.0f);                                                 // :401
        v = (float)fmin((double)v, (double)(ts - 1) - eps);                 // :402 (double min, then rounded)
        tif[k] = v;
        ti[k] = (int)v;
        fr[k] = v - (float)ti[k];
    }
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        float w = 1.0f;
        int idx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (((pn >> k) & 1) == 0) {
                w *= 1.0f - fr[k];
                idx[k] = ti[k];
            } else {
                w *= fr[k];
                idx[k] = ti[k] + 1;
            }
        }
        t.isc[pn] = (flip ? idx[2] : idx[0]) * ts * ts + idx[1] * ts + (flip ? idx[0] : idx[2]);
        t.w[pn] = w;
    }
}

// The trilinear sum of a cube of T texels at taps t, from 0 in tap order.  The eight texels are requested together -- a tap
// outside the cube (compute_taps) at the cube's last texel, for the address alone -- and summed once they are all there: a
// load under its own condition is a basic block of its own that waits for its data before the next one is issued, eight
// round trips one behind the other.  A tap outside the cube is skipped by keeping the sums as they are (not by its zero
// weight: a NaN or Inf texel must not come in).
__device__ __forceinline__ void sum_taps(const float *__restrict__ texture, const Taps &t, int T, float c[3])
{
    float tx[8][3];
    unsigned inside = 0;  // bit pn: tap pn lies inside the cube
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        inside |= (unsigned)(t.isc[pn] < T) << pn;
        const float *p = texture + min(t.isc[pn], T - 1) * 3;
        tx[pn][0] = p[0];
        tx[pn][1] = p[1];
        tx[pn][2] = p[2];
    }
    c[0] = c[1] = c[2] = 0.0f;
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        const bool in = (inside >> pn) & 1u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float s = c[k] + t.w[pn] * tx[pn][k];
            c[k] = in ? s : c[k];
        }
    }
}

// --------------------------------------------------------------------------------------------------
// Bilinear reads of texture images (K10).  One definition for the load_obj bake, the learnable bake, its inverse map and
// per-pixel UV shading (nr_texture_io.hip, nr_uv_pixel.hip, the UV branch of shade_pixel).

__device__ __forceinline__ int f2i(float x) { return (int)x; }  // v_cvt_i32_f32: truncates, saturates, NaN -> 0 (as CUDA)

// The four bilinear reads of an [H,W] image stored bottom row first at the barycentric point d of a face's uv triangle
// (load_obj.py:112-128): the flat pixel indices in the order the sum takes them -- (yi,xi), (yi1,xi), (yi,xi+1), (yi1,xi+1),
// with the reference's yi1 = (int)(pos_y + 1) -- clamped to [0, H*W-1], and their weights.
// ax: the weights' factors (wx0, wx1, wy0, wy1), for a caller that differentiates the sample (nr_soft_render.hip).
__device__ __forceinline__ void texel_reads(const float *face, const float d[3], int H, int W, long long p[4], float w[4],
                                            float ax[4])
{
    const float pos_x = (face[0] * d[0] + face[2] * d[1] + face[4] * d[2]) * (float)(W - 1);  // :112-113
    const float pos_y = (face[1] * d[0] + face[3] * d[1] + face[5] * d[2]) * (float)(H - 1);  // :114-115
    const int xi = f2i(pos_x), yi = f2i(pos_y), yi1 = f2i(pos_y + 1.0f);
    const float wx1 = pos_x - (float)xi, wx0 = 1.0f - wx1;  // :118-121
    const float wy1 = pos_y - (float)yi, wy0 = 1.0f - wy1;
    const long long last = (long long)H * W - 1;
    auto clampi = [&](int row, int col) -> long long {
        const long long q = (long long)row * W + col;
        return q < 0 ? 0 : (q > last ? last : q);
    };
    p[0] = clampi(yi, xi);
    p[1] = clampi(yi1, xi);
    p[2] = clampi(yi, xi + 1);
    p[3] = clampi(yi1, xi + 1);
    w[0] = wx0 * wy0;
    w[1] = wx0 * wy1;
    w[2] = wx1 * wy0;
    w[3] = wx1 * wy1;
    ax[0] = wx0; ax[1] = wx1; ax[2] = wy0; ax[3] = wy1;
}

__device__ __forceinline__ void texel_reads(const float *face, const float d[3], int H, int W, long long p[4], float w[4])
{
    float ax[4];
    texel_reads(face, d, H, W, p, w, ax);
}

// texel_reads' index (bottom row first) -> the same pixel in an image stored top row first (file orientation)
__device__ __forceinline__ int mirror_row(long long p, int H, int W)
{
    const int row = (int)(p / W), col = (int)(p - (long long)row * W);
    return (H - 1 - row) * W + col;
}

// Per-pixel sampling of UV texture images (nr_uv_images in include/nr_hip.h): the layout and images of
// nr_bake_uv_textures, read at the pixel instead of at the texels of a cube.
struct UVShade {
    const float *images = nullptr;      // [Bi, P, 3], each image top row first
    const int32_t *table = nullptr;     // [M, 3]: first pixel, H, W
    const float *faces_uv = nullptr;    // [Nf, 3, 2]
    const int32_t *face_image = nullptr;  // [Nf]; outside [0, M): the face samples `base`
    const float *base = nullptr;        // [Nf, ts^3, 3]
    int ts = 0, M = 0, P = 0;
    int shared = 0;                     // 1: one set of images for the whole batch (image batch stride 0)
};

// Where the pixel of face fi (batch element b, weights w, depth zp) reads.  `face` = face fi of batch element b itself.  The
// reversed copy fi >= tex_faces of face f0 = fi - tex_faces takes its weights in reversed corner order, as the cube path
// transposes the cube.  m >= 0: four reads q (packed pixels) with weights w of image m; m < 0: the cube taps of `base`.
struct UVSample {
    int m, f0;
    int q[4];
    float w[4];
    Taps t;
};

// The perspective-correct corner weights of a pixel (weights w, depth zp) of a face with vertex depths z, in the face's own
// corner order: d_k = fminf(fmaxf(w_k * (zp / z_k), 0), 1) -- compute_taps' product without the ts - 1 factor.  Used by
// the resolve pass's corner mode (shade_pixel<SHADE_CORNER>) and by smooth UV shading in both directions.  NOT the only place
// that states the product: uv_locate below and nr_vertex_colors.hip's backward (its own corner_weights) keep their own line
// of it, because routing them through here changed the code generated for those existing kernels (DESIGN K10 "Smooth light
// on UV images").  A change to the formula has to be made in all three.
__device__ __forceinline__ void corner_weights(const float (&z)[3], const float (&w)[3], float zp, float (&d)[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = fminf(fmaxf(w[k] * (zp / z[k]), 0.0f), 1.0f);
}

__device__ __forceinline__ void uv_locate(const UVShade &uv, int fi, int tex_faces, const float *face, float w0, float w1,
                                          float w2, float zp, double eps, UVSample &s)
{
    const bool flip = fi >= tex_faces;
    s.f0 = flip ? fi - tex_faces : fi;
    const int m = uv.face_image[s.f0];
    s.m = (m >= 0 && m < uv.M) ? m : -1;
    const float fz[3] = {face[2], face[5], face[8]};
    const float w[3] = {w0, w1, w2};
    if (s.m < 0) {
        compute_taps(fz, w, zp, uv.ts, eps, s.t, flip);
        return;
    }
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = fminf(fmaxf(w[k] * (zp / fz[k]), 0.0f), 1.0f);  // compute_taps' product, no ts - 1
    if (flip) {
        const float d0 = d[0];
        d[0] = d[2];
        d[2] = d0;
    }
    const int off = uv.table[3 * s.m], H = uv.table[3 * s.m + 1], W = uv.table[3 * s.m + 2];
    long long p[4];
    texel_reads(uv.faces_uv + (size_t)s.f0 * 6, d, H, W, p, s.w);
#pragma unroll
    for (int r = 0; r < 4; r++) s.q[r] = off + mirror_row(p[r], H, W);
}

// The sampled colour before the light factor: the reads summed in read order from 0 (as k_bake_uv sums a texel), or the
// cube path's trilinear sum on `base` (as shade_pixel sums a cube).
__device__ __forceinline__ void uv_color(const UVShade &uv, const UVSample &s, int b, float c[3])
{
    c[0] = c[1] = c[2] = 0.0f;
    if (s.m >= 0) {
        const float *img = uv.images + (uv.shared ? 0 : (size_t)b * uv.P * 3);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float *px = img + (size_t)s.q[r] * 3;
            c[0] += px[0] * s.w[r];
            c[1] += px[1] * s.w[r];
            c[2] += px[2] * s.w[r];
        }
        return;
    }
    const int T = uv.ts * uv.ts * uv.ts;
    const float *texture = uv.base + (size_t)s.f0 * T * 3;
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        if (s.t.isc[pn] >= T) continue;  // outside the cube: weight 0 (see compute_taps)
        const float *tx = texture + s.t.isc[pn] * 3;
        c[0] += s.t.w[pn] * tx[0];
        c[1] += s.t.w[pn] * tx[1];
        c[2] += s.t.w[pn] * tx[2];
    }
}


// --------------------------------------------------------------------------------------------------
// host side helpers
// XCD-aware workgroup placement.  MI355X has 8 accelerator dies (XCDs), each with a private L2; the hardware deals
// consecutive workgroup ids of a launch round-robin to them.  Work items that share data (the faces, maps and textures of one
// image) should therefore NOT have consecutive ids: a 1-D grid of xcd_grid(n) workgroups is launched and the kernel uses
// xcd_block(n) instead of blockIdx.x, which makes each XCD walk one contiguous 1/8 of the logical range.
constexpr unsigned NUM_XCD = 8;
inline unsigned xcd_grid(size_t n_blocks) { return (unsigned)((n_blocks + NUM_XCD - 1) / NUM_XCD * NUM_XCD); }
#ifdef __HIPCC__
// logical block id in [0, n_blocks), or n_blocks (= "no work") for the padding blocks
__device__ __forceinline__ unsigned xcd_block(unsigned n_blocks)
{
    const unsigned chunk = (n_blocks + NUM_XCD - 1) / NUM_XCD;
    const unsigned logical = (blockIdx.x % NUM_XCD) * chunk + blockIdx.x / NUM_XCD;
    return logical < n_blocks ? logical : n_blocks;
}

// Working-first order for the sparse launches over (list slots, image): a grid of gx workgroups for each of B images whose
// workgroup (bx, by) has work only while bx is below a count of image by (the length of its visible-face list over the
// workgroup's share: about one in six at the headline size) and otherwise reads that count and leaves.  With bx fastest --
// the order of a 2-D grid -- every image is a run of working workgroups followed by a long run of leaving ones, and a slot
// a working workgroup frees is handed to several leaving ones in turn before the next working one gets it.  The launch is
// 1-D instead, gx * B ids, and the image is fastest: (bx, by) = (id / B, id % B).  Every workgroup that can have work (bx
// below the longest list's share) is handed out before the first that cannot.  Nothing waits for anything: it is the same
// set of workgroups in another order.  (With B a multiple of 8 an image's workgroups all land on one XCD.)
// Used where it measured (profiles/sparse_grid_ab.md, profiles/idle_workgroups_ab.md): k_line_setup, the gather part of
// k_band_gather and k_setup_gather.
struct SlotImage { int bx, by; };
__device__ __forceinline__ SlotImage image_fastest(unsigned id, unsigned B)
{
    const unsigned bx = id / B;
    return {(int)bx, (int)(id - bx * B)};
}
#endif

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#ifdef __HIPCC__
// Fills of the library's own instead of hipMemsetAsync: a captured HIP graph that holds a memset node on memory from outside
// the graph's pool misbehaves on replay on ROCm 7.2 (the 0xff fill of the z-buffer faults on the second replay, the zero
// fill of grad_textures leaves garbage) -- found with the operator's graph-replay mode.  Kernel nodes replay fine.
static __global__ __launch_bounds__(256) void k_fill_bytes(unsigned char *__restrict__ dst, size_t bytes, unsigned value32)
{
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i0 >= bytes) return;
    if (i0 + 16 <= bytes && ((size_t)(dst + i0) & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst + i0) = make_uint4(value32, value32, value32, value32);
    } else {
        for (size_t i = i0; i < bytes && i < i0 + 16; ++i) dst[i] = (unsigned char)value32;
    }
}
// every byte of [dst, dst + bytes) = byte; returns a hipError_t as int (0 = ok)
inline int fill_bytes(void *dst, int byte, size_t bytes, hipStream_t st)
{
    if (bytes == 0) return 0;
    const unsigned b = (unsigned)(byte & 0xff), v = b | (b << 8) | (b << 16) | (b << 24);
    hipLaunchKernelGGL(k_fill_bytes, dim3((unsigned)((bytes + 4095) / 4096)), dim3(256), 0, st, (unsigned char *)dst, bytes, v);
    return (int)hipGetLastError();
}
#endif

inline int check_sizes(int B, int F, int S)
{
    if (B < 1 || B > 65535 || F < 1 || S < 1 || S > 16384) return NR_E_SIZE;  // B: several kernels put the image on grid.y
    if ((size_t)B * (size_t)F > 0x7fffffffull / 9) return NR_E_SIZE;  // int32 face indexing inside kernels
    return 0;
}

inline int launch_status()
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}


// --------------------------------------------------------------------------------------------------
// The backward of one ABI call (nr_backward.hip): K6 (grad_faces from the rgb / alpha maps), K7 (grad_textures) and K8
// (grad_faces from the depth map).  The entry point describes the call (BackwardCall); plan_backward checks it and decides
// every launch before the first one goes out (BackwardPlan); run_backward launches the plan's steps in order.  The steps are
// the host sides of K6 (nr_backward_pixel_map.hip) and of the gathers (nr_backward_gather.hip).
enum { STAGE_K6 = 1, STAGE_K7 = 2, STAGE_K8 = 4, STAGE_ALL = 7 };  // what the entry point computes (all: the fused backward)

struct BackwardCall {
    int stages;                        // STAGE_*
    bool rgb, alpha;                   // K6 takes these maps
    const float *faces, *faces_z_ref;
    const int32_t *face_index_map;
    const float *weight_map, *depth_map, *rgb_map, *alpha_map, *grad_rgb_map, *grad_alpha_map, *grad_depth_map;
    const float *sampling_weight_map;  // nr_backward_textures: the forward's taps (or NULL)
    const int32_t *sampling_index_map;
    const float *face_inv_map;         // nr_backward_depth_map: the reference's per-pixel residual (or NULL)
    float *grad_faces, *grad_textures;
    int B, F, S, ts;
    double eps;
    int flags;
    const unsigned char *visible_faces;  // the forward's per-face flags (or NULL)
    void *workspace;
    size_t workspace_bytes;
    FaceLight lit;  // lit.light given: grad_textures is [B, lit.tex_faces, ts^3, 3], lit.grad_light receives [B, F, 3]
    hipStream_t st;
};

// Which band kernel K6 takes, and how it is shaped: decided from the call's shape alone (plan_k6, nr_backward_pixel_map.hip).
struct BandShape {
    int threads;     // 256 | 512
    int w_max;       // widest band (lines)
    size_t budget;   // LDS per workgroup
};
enum K6Kernel { K6_KERNEL_FAST = 0, K6_KERNEL_ROW = 1, K6_KERNEL_GLOBAL = 2 };  // (0 / 1: nr_profile_band_kernel_which)
struct K6Plan {
    int kernel;           // K6Kernel
    int mode;             // K6_FAST | K6_EXACT_POW2 | K6_EXACT
    BandShape shape;      // k_bpm_fast: workgroup shape,
    int W_fast;           // ... band width (lines; 0: no LDS band fits -- the global kernel),
    size_t fast_lds;      // ... LDS bytes,
    int win_lines, qcap;  // ... line records per window and piece-queue capacity
    int W_row;            // k_bpm_row: band width (0: not taken)
    size_t row_lds;       // ... LDS bytes
    int W, n_bands;       // the band tables: lines per band, bands per image
    bool use_records;     // line records from k_line_setup (false: every image takes k_bpm_fast's face scan)
    bool overflow_pass;   // k_bpm_fast's overflow-only launch follows k_bpm_row
    bool row_chunked;     // k_bpm_row cuts its lines into chunks (rasters above 512 on meshes below 2^15 faces)
    size_t fill_max;      // the largest zero fill (bytes) that the band kernel takes along
};
K6Plan plan_k6(int B, int F, int S, bool rgb, double eps, int flags);

enum FaceZeros { FACE_ZEROS_NONE, FACE_ZEROS_UNLISTED, FACE_ZEROS_ALL };     // the compaction's stores of grad_faces
// who zeroes grad_textures (TEX_ZEROS_BAND_UNLISTED: the band workgroups of the merged launch, the unlisted faces' cubes only)
enum TexZeros { TEX_ZEROS_NONE, TEX_ZEROS_BAND, TEX_ZEROS_SETUP, TEX_ZEROS_FILL, TEX_ZEROS_BAND_UNLISTED };
enum K6Finish { FINISH_NONE, FINISH_KERNEL, FINISH_GATHER, FINISH_BIG, FINISH_ADD };  // who rounds K6's sums into grad_faces
enum Gather { GATHER_NONE, GATHER_FACE, GATHER_ATOMIC };                   // K7's gather

struct BackwardPlan {
    bool k6;               // K6 runs, as k6p says
    K6Plan k6p;
    bool bands;            // ... through the band pipeline (not k_bpm_global): K6's lists, scratch and face -> position table
    int face_zeros;        // FaceZeros
    bool gather_first;     // small calls: the K7 gather goes out between the compaction and the band kernel
    bool gather_in_tail;   // large calls: the K7 / K8 gather's workgroups behind k_bpm_row's in one grid (k_band_gather)
    bool setup_alone;      // k_line_setup as a launch of its own (behind the gather when gather_first)
    bool setup_in_gather;  // k_line_setup's workgroups inside the gather's launch (k_setup_gather)
    int tex_zeros;         // TexZeros (TEX_ZEROS_SETUP: the unlisted faces' cubes, in k_setup_gather)
    size_t tex_bytes;      // grad_textures' bytes (the original cubes with per-face light colours)
    bool light_fill;       // grad_light zero-filled in front of the gather
    int gather;            // Gather
    bool listed;           // the face gather and k_backward_big walk K6's lists
    bool static_taps;      // texture_size 2 with static taps (TS2 kernels)
    int lanes;             // face gather: lanes per face (16 / 64 / 256)
    size_t gather_lds;     // ... its dynamic LDS
    bool depth_in_gather;  // K8 rides in the K7 gather (and its k_backward_big)
    bool big;              // k_backward_big behind the face gather (texture_size <= 8)
    bool big_overflow;     // ... with K6's overflow pass in its launch (k_big_overflow) instead of behind the band kernel
    int finish;            // K6Finish
    bool depth;            // K8 as launches of its own (k_backward_depth_face + k_backward_big)
    bool fill_faces;       // depth-only fused call: grad_faces zero-filled
    bool depth_lists;      // ... and K8's lists from the forward's flags (k_list_visible)
};
int plan_backward(const BackwardCall &c, BackwardPlan &p);  // 0 or an NR_E_* code; launches nothing
int run_backward(const BackwardCall &c);  // plan_backward, then the plan's steps in order

// K6's buffers in the workspace: per image the sorted list of the faces that own a pixel ([B][F] ints, [B] counts), face ->
// list position or -1 ([B][F]), and the six double sums of each list position
struct K6Lists {
    const int *vis_list, *vis_count, *slot_of;
    double *scratch;
    int *ticket;  // the overflow pass's ticket counter (k_big_overflow), zeroed by the compaction
};
struct LineSetupArgs;  // nr_band_lines.h

// K6's steps (nr_backward_pixel_map.hip)
int k6_compact(const BackwardCall &c, const K6Plan &p, int face_zeros, K6Lists &out);  // [k_mark_visible] + compaction
LineSetupArgs k6_line_setup_args(const BackwardCall &c, const K6Plan &p);
int run_line_setup(const LineSetupArgs &a, hipStream_t st);
int k6_band(const BackwardCall &c, const K6Plan &p, const K6Lists &l, const LineSetupArgs &ls, void *fill, size_t fill_bytes,
            const BackwardPlan *tail, bool overflow_later);  // k_bpm_global, or band kernel (tail: with the gather behind it) [+ overflow]
int k6_big_overflow(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l, const LineSetupArgs &ls);  // overflow + k_backward_big
void k6_finalize(const BackwardCall &c, const K6Lists &l, bool add);
bool k6_lists_fit(int B, int F, size_t workspace_bytes);  // k_list_visible's lists fit the workspace and one launch
K6Lists k6_list_visible(const BackwardCall &c);
// the gathers' steps (nr_backward_gather.hip)
int gather_faces(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l, const LineSetupArgs *ls);
void gather_big(const BackwardCall &c, const BackwardPlan &p, const K6Lists &l);
void gather_atomic(const BackwardCall &c);
void gather_depth(const BackwardCall &c, const K6Lists &l);

int face_light_args(const nr_face_light *lit, int F, bool backward, FaceLight &out);  // nr_forward.hip
// nr_uv_images + its nr_face_light (lit->grad_light copied into fl) -> the kernels' arguments; nr_forward.hip
int uv_images_args(const nr_face_light *lit, const nr_uv_images *uv, int B, int F, FaceLight &fl, UVShade &out);
// the same for an nr_corner_light (smooth UV shading): fl.light is then [B, F, 3, 3] and fl.grad_light likewise
int uv_smooth_args(const nr_corner_light *lit, const nr_uv_images *uv, int B, int F, FaceLight &fl, UVShade &out);

}  // namespace nr

#include "nr_reduce.h"  // fixed-order sums and scans: every kernel file gets them with this header
