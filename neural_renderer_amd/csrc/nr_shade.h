// nr_shade.h -- the light model shared by the geometry front-end (nr_frontend.hip) and vertex shading (nr_vertex_colors.hip):
// the small vector helpers, chainer's normalize with its backward, the front-end's parameter block and the light colours of
// a face and of its reversed copy (lighting.py:28-47).  One definition, so that both files round alike.
#pragma once
#include "nr_device.h"

namespace nr {

constexpr float NORM_EPS = 1e-5f;  // chainer.functions.normalize default eps

struct FrontendParams {
    int camera_mode;  // NR_CAMERA_LOOK_AT / NR_CAMERA_LOOK / NR_CAMERA_PROJECTION
    int perspective;
    int eye_per_batch;
    int idx_per_batch;
    int fill_back;
    int has_directional;
    float target[3];  // `at` (look_at) or `direction` (look)
    float up[3];
    float width;  // tan(viewing angle)
    float ia, id;
    float ca[3], cd[3], ldir[3];
};

__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const float *a, const float *b, float *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// chainer normalize: v / (|v| + eps)
__device__ __forceinline__ void normalize3(const float *v, float *o)
{
    const float s = sqrtf(dot3(v, v)) + NORM_EPS;
    o[0] = v[0] / s;
    o[1] = v[1] / s;
    o[2] = v[2] / s;
}

// backward of normalize3: g_v = g / (r + eps) - v * (g.v) / ((r + eps)^2 * r)
__device__ __forceinline__ void normalize3_bwd(const float *v, const float *g, float *o)
{
    const float r = sqrtf(dot3(v, v));
    const float s = r + NORM_EPS;
    const float k = r > 0.0f ? dot3(g, v) / (s * s * r) : 0.0f;
    o[0] = g[0] / s - v[0] * k;
    o[1] = g[1] / s - v[1] * k;
    o[2] = g[2] / s - v[2] * k;
}

// light colours of a face and of its reversed copy (lighting.py:31-47); n = unnormalised normal, dotn = n_hat . direction
__device__ __forceinline__ void face_light(const FrontendParams &P, const float *w0, const float *w1, const float *w2, float *n,
                                           float &dotn, float *light_f, float *light_b)
{
    float cos_f = 0.0f, cos_b = 0.0f;
    dotn = 0.0f;
    if (P.has_directional) {
        const float v10[3] = {w0[0] - w1[0], w0[1] - w1[1], w0[2] - w1[2]};  // lighting.py:37-38
        const float v12[3] = {w2[0] - w1[0], w2[1] - w1[1], w2[2] - w1[2]};
        cross3(v10, v12, n);
        float nh[3];
        normalize3(n, nh);  // :40
        dotn = dot3(nh, P.ldir);
        cos_f = fmaxf(dotn, 0.0f);   // relu, :45
        cos_b = fmaxf(-dotn, 0.0f);  // the reversed face has exactly the negated normal
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float amb = P.ia != 0.0f ? P.ia * P.ca[c] : 0.0f;                       // :28-29
        light_f[c] = P.has_directional ? amb + P.id * (P.cd[c] * cos_f) : amb;        // :46
        light_b[c] = P.has_directional ? amb + P.id * (P.cd[c] * cos_b) : amb;
    }
}

}  // namespace nr
