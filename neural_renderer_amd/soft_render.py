"""Soft colour rendering (not in the reference): the soft silhouette's coverage aggregated over the faces by Soft Rasterizer's
depth-weighted softmax, with the exact gradient of its definition -- to x, y, z and the face colours.  The hard rasterizer's
approximate gradient knows nothing about occlusion: a face hidden behind another gets none, and no z ever receives one from
the image.  Here the image can pull a hidden face forward and push an occluder back.

`faces` [B,F,3,3] are the rasterizer's own input -- x, y in NDC with y up, z the positive camera depth -- WITHOUT fill_back
copies, exactly as soft_silhouettes takes them; `colors` [B,F,3], or [1,F,3] shared by the batch and read in place, one RGB
colour per face -- or corner colours [B,F,3,3] / [1,F,3,3], indexed (image, face, corner, rgb), interpolated at every pixel
(below).  The output is rgba [B,4,S,S], row 0 the top row, rendered at S directly (no anti-aliasing); pixel centres
(2 i + 1 - S) / S.

    A face contributes iff its nine coordinates are finite, near <= z_k <= far at its three vertices and its doubled area
    (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0), evaluated in float64, is not 0: a zero-area face has no plane to take a depth
    from.
    Per contributing face f and pixel p: d2, the chosen segment k (the lowest on a tie), its clamped t, r, the side s,
    x = s d2 / sigma, D = 1 / (1 + e^-x) and 1 - D = 1 / (1 + e^x) are the soft silhouette's (soft_silhouette.py); c_0, c_1,
    c_2 are the edge functions of the segments v0v1, v1v2, v2v0 at p.
    The pair is TAKEN iff s = +1 or d2 <= 17 sigma.  The cutoff is part of the definition: a far pair with D < 2^-24 could
    still carry weight once multiplied by exp(zn / gamma).
    Inverse depth: inside, A = c_0 + c_1 + c_2, lambda_0 = c_1 / A, lambda_1 = c_2 / A, lambda_2 = c_0 / A (the
    rasterizer's perspective-correct form); outside, at the nearest point of the chosen segment a -> b, lambda_a = 1 - t,
    lambda_b = t and the third 0 -- continuous with the inside form across every edge.
    iz = lambda_0 / z0 + lambda_1 / z1 + lambda_2 / z2,  zp = 1 / iz,  zn = (far - zp) / (far - near) in [0, 1].
    Over the taken pairs of p in ascending f, with m = max(eps, max_f zn_f):
      w_f = D_f exp((zn_f - m) / gamma),  w_b = exp((eps - m) / gamma),  Z = w_b + sum w_f
      rgb = (w_b background + sum w_f C_f) / Z,  Q = prod 1 / (1 + e^x_f),  alpha = 1 - Q
    Gradient (exact, once-differentiable), per taken pair, with W = D exp((zn - m) / gamma) / Z and h = g_rgb . (C_f - rgb):
      dL/dC_f += W g_rgb,  dL/dx = h W (1 - D) + g_alpha Q D,  dL/dzn = h W / gamma
    dx goes to the two ends of the chosen segment as in the soft silhouette (the t inside d2 carries no gradient);
    dzn/dzp = -1 / (far - near), dzp/diz = -zp^2, diz/dz_k = -lambda_k / z_k^2; diz also reaches x and y, through lambda
    inside and through t outside where 0 < t < 1 -- a clamped t has derivative 0.

    Corner colours: for a taken pair u_k = lambda_k / z_k, mu_k = u_k zp (the perspective-correct weights, sum 1) and
      C_f(p) = (mu_0 C_f0 + mu_1 C_f1) + mu_2 C_f2 per channel
    stands where C_f stood: inside the colour the rasterizer would interpolate, outside the colour at the nearest boundary
    point -- continuous across every edge, single-valued because the nearest point of a triangle is unique.  Gradient: with
    h = g_rgb . (C_f(p) - rgb), dL/dC_fk += W mu_k g_rgb; with E_k = W zp (g_rgb . (C_fk - C_f(p))) and d_k = diz + E_k,
    dL/dlambda_k = d_k / z_k and dL/dz_k = -d_k lambda_k / z_k^2; inside dL/dc_i = (dL/dlambda_v(i) - diz iz) / A with
    v(0) = 2, v(1) = 0, v(2) = 1; outside with a free t on a -> b, dL/dt = d_b / z_b - d_a / z_a.  Three equal corner colours
    give E_k = 0 and the flat gradient.

sigma, gamma, eps, near, far and the background colour are host numbers without gradients.  On float32 CUDA tensors inside
the ranges of include/nr_hip.h both directions are HIP kernels (nr_soft_render_*, for corner colours nr_soft_corners_*);
`soft_render_torch` serves everything else in plain torch with the same definition.  No host tables: a first call may be
captured (graph.capture) -- but capture before any eager backward on the same leaves, or make the eager calls under no_grad,
as for soft_silhouettes (DESIGN "Soft silhouettes", Stream capture).

Not done: textures sampled at the pixel, a learnable sigma / gamma, anti-aliasing, a spatial index.
"""
import math

import torch

from . import _lib, _util

_CHUNK_ELEMENTS = 2 ** 24   # soft_render_torch: the most elements of one temporary
REACH = 17.0                # an outside pair is taken up to d2 = REACH sigma


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def soft_render_torch(faces, colors, image_size=256, sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3,
                      background_color=(0, 0, 0)):
    """rgba [B,4,S,S] in plain torch (any device, any float dtype), differentiable by autograd in faces and colors; the
    module docstring's definition over every (pixel, face) pair, in chunks of pixel rows."""
    B, F, S = int(faces.shape[0]), int(faces.shape[1]), int(image_size)
    one, zero = torch.ones((), dtype=faces.dtype, device=faces.device), torch.zeros((), dtype=faces.dtype, device=faces.device)
    z = faces[:, :, :, 2]
    f64 = faces.detach().double()
    area = ((f64[:, :, 1, 0] - f64[:, :, 0, 0]) * (f64[:, :, 2, 1] - f64[:, :, 0, 1])
            - (f64[:, :, 2, 0] - f64[:, :, 0, 0]) * (f64[:, :, 1, 1] - f64[:, :, 0, 1]))
    on = torch.isfinite(faces).all(3).all(2) & (z >= near).all(2) & (z <= far).all(2) & (area != 0)   # [B,F]
    xy = torch.where(on[:, :, None, None], faces[..., :2], zero)
    iz = 1 / torch.where(on[:, :, None], z, one)
    v = [[xy[:, None, None, :, k, c] for c in range(2)] for k in range(3)]   # [B,1,1,F]
    izv = [iz[:, None, None, :, k] for k in range(3)]
    corners = colors.dim() == 4
    if corners:
        col = colors.to(faces.dtype).expand(B, F, 3, 3)[:, None, None]       # [B,1,1,F,3 corners,3]
    else:
        col = colors.to(faces.dtype).expand(B, F, 3)[:, None, None]          # [B,1,1,F,3]
    on = on[:, None, None, :]
    centre = (2 * torch.arange(S, device=faces.device, dtype=torch.float64) + 1 - S) / S
    centre = centre.to(faces.dtype)
    px = centre[None, None, :, None]
    bg = [float(c) for c in background_color]
    rows = max(1, _CHUNK_ELEMENTS // max(1, B * S * F))
    out = []
    for r0 in range(0, S, rows):
        py = centre[None, r0:r0 + rows, None, None]
        d0, c0, t0 = _util.soft_segment(px, py, v[0][0], v[0][1], v[1][0], v[1][1])
        d1, c1, t1 = _util.soft_segment(px, py, v[1][0], v[1][1], v[2][0], v[2][1])
        d2, c2, t2 = _util.soft_segment(px, py, v[2][0], v[2][1], v[0][0], v[0][1])
        s1 = d1 < d0   # strict: the lowest segment wins a tie
        da = torch.where(s1, d1, d0)
        s2 = d2 < da
        d = torch.where(s2, d2, da)
        t = torch.where(s2, t2, torch.where(s1, t1, t0))
        k0, k1 = ~s1 & ~s2, s1 & ~s2
        inside = ((c0 > 0) & (c1 > 0) & (c2 > 0)) | ((c0 < 0) & (c1 < 0) & (c2 < 0))
        A = torch.where(inside, c0 + c1 + c2, one)
        l0 = torch.where(inside, c1 / A, torch.where(k0, 1 - t, torch.where(s2, t, zero)))
        l1 = torch.where(inside, c2 / A, torch.where(k1, 1 - t, torch.where(k0, t, zero)))
        l2 = torch.where(inside, c0 / A, torch.where(s2, 1 - t, torch.where(k1, t, zero)))
        u0, u1, u2 = l0 * izv[0], l1 * izv[1], l2 * izv[2]
        zp = 1 / (u0 + u1 + u2)
        zn = (far - zp) / (far - near)
        taken = on & (inside | (d.detach() <= REACH * sigma))
        x = torch.where(inside, d, -d) / sigma
        m = torch.where(taken, zn.detach(), torch.full_like(zn, -math.inf)).amax(3).clamp(min=eps)   # [B,rows,S]
        w = torch.where(taken, torch.sigmoid(x) * torch.exp(torch.where(taken, (zn - m[..., None]) / gamma, zero)), zero)
        wb = torch.exp((eps - m) / gamma)
        Z = wb + w.sum(3)
        if corners:   # the colour at the pixel: the perspective-correct weights mu_k = u_k zp
            mu0, mu1, mu2 = u0 * zp, u1 * zp, u2 * zp
            at = [mu0 * col[..., 0, c] + mu1 * col[..., 1, c] + mu2 * col[..., 2, c] for c in range(3)]
        else:
            at = [col[..., c] for c in range(3)]
        rgb = [(wb * bg[c] + (w * at[c]).sum(3)) / Z for c in range(3)]
        # alpha = 1 - Q as in soft_silhouettes_torch: the value from the product, the derivative from Q times the logarithms
        q = torch.where(taken, torch.sigmoid(-x), torch.ones_like(x)).prod(3).detach()
        ln_q = torch.where(taken, torch.nn.functional.logsigmoid(-x), torch.zeros_like(x)).sum(3)
        alpha = (1 - q) + q * torch.where(q > 0, ln_q.detach() - ln_q, torch.zeros_like(ln_q))
        out.append(torch.stack(rgb + [alpha], 1))
    return torch.cat(out, 2).flip(2)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

class _SoftRender(torch.autograd.Function):
    """forward(ctx, faces [B,F,3,3], colors [B|1,F,3] or [B|1,F,3,3], image_size, sigma, gamma, near, far, eps, background)
    -> rgba [B,4,S,S], row 0 the top row.  4-dim colours take the nr_soft_corners_* entries, 3-dim ones nr_soft_render_*."""

    @staticmethod
    def forward(ctx, faces, colors, image_size, sigma, gamma, near, far, eps, background):
        f, c = _lib.dense(faces.detach()), _lib.dense(colors.detach())
        B, F, S = int(f.shape[0]), int(f.shape[1]), image_size
        per_batch = 1 if int(c.shape[0]) == B else 0   # else [1,F,3]: one set for the batch, read in place
        entry = 'nr_soft_corners' if c.dim() == 4 else 'nr_soft_render'
        rgba = torch.empty((B, 4, S, S), dtype=torch.float32, device=f.device)
        q = torch.empty((B, S, S), dtype=torch.float32, device=f.device)
        norm = torch.empty((B, 2, S, S), dtype=torch.float32, device=f.device)
        _lib.launch(entry + '_forward', f.device, f.data_ptr(), c.data_ptr(), rgba.data_ptr(), q.data_ptr(), norm.data_ptr(),
                    B, F, S, per_batch, sigma, gamma, near, far, eps, background[0], background[1], background[2],
                    workspace_bytes=_lib.workspace_bytes(entry + '_workspace_bytes', B, F, S))
        ctx.save_for_backward(f, c, rgba, q, norm)
        ctx.args = (S, per_batch, sigma, gamma, near, far, eps, background, entry)
        return rgba.flip(2)

    @staticmethod
    def backward(ctx, grad_rgba):
        f, c, rgba, q, norm = ctx.saved_tensors
        S, per_batch, sigma, gamma, near, far, eps, background, entry = ctx.args
        B, F = int(f.shape[0]), int(f.shape[1])
        g = _lib.dense(grad_rgba.flip(2))
        grad_faces, grad_colors = torch.empty_like(f), torch.empty_like(c)
        _lib.launch(entry + '_backward', f.device, f.data_ptr(), c.data_ptr(), rgba.data_ptr(), q.data_ptr(), norm.data_ptr(),
                    g.data_ptr(), grad_faces.data_ptr(), grad_colors.data_ptr(), B, F, S, per_batch, sigma, gamma, near, far,
                    eps, background[0], background[1], background[2],
                    workspace_bytes=_lib.workspace_bytes(entry + '_workspace_bytes', B, F, S))
        return (grad_faces, grad_colors) + (None,) * 7


# ---------------------------------------------------------------------------------------------------------------------
# the public function

def _check(name, faces, colors, image_size, sigma, gamma, near, far, eps, background_color, implementation):
    """Argument checks shared by both implementations -> (image_size, sigma, gamma, near, far, eps, background, takes the
    HIP path)."""
    B, F = _util.soft_check_faces(name, faces)
    if not (torch.is_tensor(colors) and colors.is_floating_point() and colors.dim() in (3, 4)
            and tuple(colors.shape[1:]) in ((F, 3), (F, 3, 3)) and colors.shape[0] in (1, B)):
        raise ValueError('%s: colors must be a float tensor [batch size or 1, num of faces (%d), 3], or [batch size or 1, '
                         'num of faces, 3, 3] for corner colours' % (name, F))
    if colors.device != faces.device:
        raise ValueError('%s: colors on %s, faces on %s' % (name, colors.device, faces.device))
    _util.soft_check_image_size(name, image_size)
    sigma, gamma = _util.number(name, 'sigma', sigma), _util.number(name, 'gamma', gamma)
    for what, v in (('sigma', sigma), ('gamma', gamma)):
        if not (0 < v < float('inf')):
            raise ValueError('%s: %s must be a finite number greater than 0, got %r' % (name, what, v))
    near, far, eps = _util.number(name, 'near', near), _util.number(name, 'far', far), _util.number(name, 'eps', eps)
    if not (math.isfinite(near) and math.isfinite(far) and near < far):
        raise ValueError('%s: near and far must be finite numbers with near < far, got %r and %r' % (name, near, far))
    if not math.isfinite(eps):
        raise ValueError('%s: eps must be a finite number, got %r' % (name, eps))
    try:
        background = tuple(background_color)
    except TypeError:
        background = ()
    if len(background) != 3:
        raise ValueError('%s: background_color must be three numbers, got %r' % (name, background_color))
    background = tuple(_util.number(name, 'background_color', float(c) if torch.is_tensor(c) else c) for c in background)
    if not all(math.isfinite(c) for c in background):
        raise ValueError('%s: background_color must be finite, got %r' % (name, background_color))
    fits = _util.soft_fits(faces, image_size) and colors.dtype == faces.dtype and 1e-30 <= sigma <= 1e30 and 1e-30 <= gamma <= 1e30
    return image_size, sigma, gamma, near, far, eps, background, _util.takes_hip(
        name, implementation, fits, 'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most, at most 2^24 '
        'faces (batch size * faces * 9 < 2^31), an image_size of 16384 at most and sigma, gamma in [1e-30, 1e30]')


def soft_render(faces, colors, image_size=256, sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3,
                background_color=(0, 0, 0), implementation=None):
    """rgba [B,4,S,S] (row 0 the top row): faces [B,F,3,3] -- the rasterizer's input, without fill_back copies -- with one
    colour per face, colors [B,F,3] or [1,F,3] -- or one per corner, [B,F,3,3] or [1,F,3,3], interpolated
    perspective-correctly at every pixel --, aggregated by coverage and depth (module docstring).  Differentiable in
    faces (x, y and z) and colors, once.  sigma (squared NDC units) sets the width of the coverage's transition, gamma the
    sharpness of the depth order (in units of the normalised depth), eps the background's place in that order; host floats
    without gradients, like near, far and background_color.  `implementation`: None picks the HIP kernels for float32 CUDA
    tensors inside their ranges, 'torch' / 'hip' force one ('hip' raises when the call does not fit)."""
    S, sigma, gamma, near, far, eps, background, hip = _check('soft_render', faces, colors, image_size, sigma, gamma, near, far,
                                                              eps, background_color, implementation)
    if hip:
        return _SoftRender.apply(faces, colors, S, sigma, gamma, near, far, eps, background)
    return soft_render_torch(faces, colors, S, sigma, gamma, near, far, eps, background)
