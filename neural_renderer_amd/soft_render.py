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

UV texture images sampled at the pixel: soft_render_uv below (its docstring has the colour of a pair and its gradient).
Texture cubes sampled at the pixel: soft_render_cubes below, likewise.

Not done: a light per corner with UV images or cubes, fill_back-transposed cubes, cubes larger than 8 in HIP, gradients to
faces_uv, a learnable sigma / gamma, anti-aliasing, a spatial index.
"""
import math

import torch

from . import _lib, _util

_CHUNK_ELEMENTS = 2 ** 24   # soft_render_torch: the most elements of one temporary
REACH = 17.0                # an outside pair is taken up to d2 = REACH sigma


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _render_torch(faces, shade, per_pair, image_size, sigma, gamma, near, far, eps, background_color):
    """The module docstring's definition over every (pixel, face) pair, in chunks of pixel rows, up to the colour of a pair:
    `shade(u0, u1, u2, zp)` -- u_k = lambda_k / z_k and zp, each [B,rows,S,F] -- gives the pair's colour as three channel
    tensors that broadcast against them; `per_pair`: how many elements of that size shade's largest temporary holds."""
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
    on = on[:, None, None, :]
    centre = (2 * torch.arange(S, device=faces.device, dtype=torch.float64) + 1 - S) / S
    centre = centre.to(faces.dtype)
    px = centre[None, None, :, None]
    bg = [float(c) for c in background_color]
    rows = max(1, _CHUNK_ELEMENTS // max(1, B * S * F * per_pair))
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
        at = shade(u0, u1, u2, zp)
        rgb = [(wb * bg[c] + (w * at[c]).sum(3)) / Z for c in range(3)]
        # alpha = 1 - Q as in soft_silhouettes_torch: the value from the product, the derivative from Q times the logarithms
        q = torch.where(taken, torch.sigmoid(-x), torch.ones_like(x)).prod(3).detach()
        ln_q = torch.where(taken, torch.nn.functional.logsigmoid(-x), torch.zeros_like(x)).sum(3)
        alpha = (1 - q) + q * torch.where(q > 0, ln_q.detach() - ln_q, torch.zeros_like(ln_q))
        out.append(torch.stack(rgb + [alpha], 1))
    return torch.cat(out, 2).flip(2)


def soft_render_torch(faces, colors, image_size=256, sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3,
                      background_color=(0, 0, 0)):
    """rgba [B,4,S,S] in plain torch (any device, any float dtype), differentiable by autograd in faces and colors; the
    module docstring's definition over every (pixel, face) pair, in chunks of pixel rows."""
    B, F = int(faces.shape[0]), int(faces.shape[1])
    if colors.dim() == 4:   # the colour at the pixel: the perspective-correct weights mu_k = u_k zp
        col = colors.to(faces.dtype).expand(B, F, 3, 3)[:, None, None]       # [B,1,1,F,3 corners,3]

        def shade(u0, u1, u2, zp):
            mu0, mu1, mu2 = u0 * zp, u1 * zp, u2 * zp
            return [mu0 * col[..., 0, c] + mu1 * col[..., 1, c] + mu2 * col[..., 2, c] for c in range(3)]
    else:
        col = colors.to(faces.dtype).expand(B, F, 3)[:, None, None]          # [B,1,1,F,3]

        def shade(u0, u1, u2, zp):
            return [col[..., c] for c in range(3)]
    return _render_torch(faces, shade, 1, image_size, sigma, gamma, near, far, eps, background_color)


def soft_render_uv_torch(faces, faces_uv, face_image, base_color, image_table, packed_images, light, image_size=256,
                         sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3, background_color=(0, 0, 0)):
    """rgba [B,4,S,S] in plain torch (any device, any float dtype) with UV images, on plain tensors: faces [B,F,3,3]; faces_uv
    [F,3,2]; face_image [F] integers (outside [0, M): no image); base_color [F,3], the colour of a face without an image, or
    [F,...,3], averaged over the middle dimensions (a base cube); image_table [M,3] integers (first pixel, H, W);
    packed_images [Bi,P,3] (Bi 1 or B), each image top row first; light [B|1,F,3] or None (ones).  The module docstring's
    definition with the UV colour of a pair, differentiable by autograd in faces, packed_images and light; in chunks of pixel
    rows."""
    B, F = int(faces.shape[0]), int(faces.shape[1])
    dt, dev = faces.dtype, faces.device
    uv = torch.as_tensor(faces_uv, device=dev).to(dt)
    fi = torch.as_tensor(face_image, device=dev).long()
    table = torch.as_tensor(image_table, device=dev).long().reshape(-1, 3)
    base = torch.as_tensor(base_color, device=dev).to(dt)
    base = base.reshape(F, -1, 3).mean(1)                                       # [F,3]
    packed = packed_images.to(dt)
    Bi, P = int(packed.shape[0]), int(packed.shape[1])
    has = (fi >= 0) & (fi < table.shape[0])
    row = table[torch.where(has, fi, torch.zeros_like(fi))]                     # [F,3]
    off, H, W = row[:, 0], row[:, 1], row[:, 2]
    has = has & (off >= 0) & (H >= 1) & (W >= 1) & (off + H * W <= P)
    off, H, W = [torch.where(has, v, torch.ones_like(v) if i else torch.zeros_like(v)) for i, v in enumerate((off, H, W))]
    lit = (torch.ones((1, F, 3), dtype=dt, device=dev) if light is None else light.to(dt)).expand(B, F, 3)[:, None, None]
    Wf, Hf = (W - 1).to(dt), (H - 1).to(dt)
    last = H * W - 1
    images = packed.expand(B, P, 3)
    bidx = torch.arange(B, device=dev)[:, None, None, None]

    def shade(u0, u1, u2, zp):
        d = []
        for u in (u0, u1, u2):   # the clamp removes rounding excess only: its derivative is taken as 1
            mu = u * zp
            d.append(mu + (mu.clamp(0, 1) - mu).detach())
        pos_x = (uv[:, 0, 0] * d[0] + uv[:, 1, 0] * d[1] + uv[:, 2, 0] * d[2]) * Wf
        pos_y = (uv[:, 0, 1] * d[0] + uv[:, 1, 1] * d[1] + uv[:, 2, 1] * d[2]) * Hf
        xi, yi = pos_x.detach().trunc(), pos_y.detach().trunc()                 # (int): towards 0; no gradient
        yi1 = (pos_y.detach() + 1).trunc()
        wx1, wy1 = pos_x - xi, pos_y - yi
        wx0, wy0 = 1 - wx1, 1 - wy1
        xi, yi, yi1 = [torch.nan_to_num(v, nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31).long() for v in (xi, yi, yi1)]
        total = None
        for r_, c_, w in ((yi, xi, wx0 * wy0), (yi1, xi, wx0 * wy1), (yi, xi + 1, wx1 * wy0), (yi1, xi + 1, wx1 * wy1)):
            flat = torch.minimum((r_ * W + c_).clamp(min=0), last)               # rows from the bottom, clamped into the image
            rr = flat // W
            q = off + (H - 1 - rr) * W + (flat - rr * W)                        # the image is stored top row first
            term = images[bidx, q] * w[..., None]                               # [B,rows,S,F,3]
            total = term if total is None else total + term
        T = torch.where(has[:, None], total, base)
        return [lit[..., c] * T[..., c] for c in range(3)]
    return _render_torch(faces, shade, 8, image_size, sigma, gamma, near, far, eps, background_color)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

@_util.once_differentiable
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

def _check(name, faces, colors, image_size, sigma, gamma, near, far, eps, background_color, implementation, light=False):
    """Argument checks shared by both implementations -> (image_size, sigma, gamma, near, far, eps, background, takes the
    HIP path).  light: `colors` is soft_render_uv's `light`, one colour per face only."""
    B, F = _util.soft_check_faces(name, faces)
    if light:
        if not (torch.is_tensor(colors) and colors.is_floating_point() and colors.dim() == 3
                and tuple(colors.shape[1:]) == (F, 3) and colors.shape[0] in (1, B)):
            raise ValueError('%s: light must be a float tensor [batch size or 1, num of faces (%d), 3]' % (name, F))
    elif not (torch.is_tensor(colors) and colors.is_floating_point() and colors.dim() in (3, 4)
              and tuple(colors.shape[1:]) in ((F, 3), (F, 3, 3)) and colors.shape[0] in (1, B)):
        raise ValueError('%s: colors must be a float tensor [batch size or 1, num of faces (%d), 3], or [batch size or 1, '
                         'num of faces, 3, 3] for corner colours' % (name, F))
    if colors.device != faces.device:
        raise ValueError('%s: %s on %s, faces on %s' % (name, 'light' if light else 'colors', colors.device, faces.device))
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


# ---------------------------------------------------------------------------------------------------------------------
# UV images

@_util.once_differentiable
class _SoftRenderUV(torch.autograd.Function):
    """forward(ctx, uv (a UVImages), args, faces [B,F,3,3], light [B|1,F,3], *uv.images) -> rgba [B,4,S,S], row 0 the top
    row: the nr_soft_uv_* entries."""

    @staticmethod
    def _struct(layout, packed, device):
        st = layout._tensors(device)
        return _lib.UVImagesStruct(packed.data_ptr(), st['table'].data_ptr(), st['faces_uv'].data_ptr(),
                                   st['face_image'].data_ptr(), st['base'].data_ptr(), layout.texture_size, layout.num_images,
                                   layout.num_pixels, int(packed.shape[0]))

    @staticmethod
    def forward(ctx, uv, args, faces, light, *images):
        from .uv_textures import pack_images
        S, sigma, gamma, near, far, eps, background = args
        f, lt = _lib.dense(faces.detach()), _lib.dense(light.detach())
        packed = pack_images([im.detach() for im in images], uv.batch)
        B, F = int(f.shape[0]), int(f.shape[1])
        per_batch = 1 if int(lt.shape[0]) == B else 0   # else [1,F,3]: one set for the batch, read in place
        rgba = torch.empty((B, 4, S, S), dtype=torch.float32, device=f.device)
        q = torch.empty((B, S, S), dtype=torch.float32, device=f.device)
        norm = torch.empty((B, 2, S, S), dtype=torch.float32, device=f.device)
        st = _SoftRenderUV._struct(uv.layout, packed, f.device)
        _lib.launch('nr_soft_uv_forward', f.device, st, f.data_ptr(), lt.data_ptr(), rgba.data_ptr(), q.data_ptr(),
                    norm.data_ptr(), B, F, S, per_batch, sigma, gamma, near, far, eps, background[0], background[1],
                    background[2], workspace_bytes=_lib.workspace_bytes('nr_soft_uv_workspace_bytes', st, B, F, S))
        ctx.save_for_backward(f, lt, packed, rgba, q, norm)
        ctx.uv, ctx.args, ctx.per_batch = uv, args, per_batch
        return rgba.flip(2)

    @staticmethod
    def backward(ctx, grad_rgba):
        from .uv_textures import unpack_image_gradients
        f, lt, packed, rgba, q, norm = ctx.saved_tensors
        uv, per_batch = ctx.uv, ctx.per_batch
        S, sigma, gamma, near, far, eps, background = ctx.args
        B, F = int(f.shape[0]), int(f.shape[1])
        g = _lib.dense(grad_rgba.flip(2))
        want_images = True in ctx.needs_input_grad[4:]
        grad_faces, grad_light = torch.empty_like(f), torch.empty_like(lt)
        grad_packed = torch.empty_like(packed) if want_images else None
        st = _SoftRenderUV._struct(uv.layout, packed, f.device)
        _lib.launch('nr_soft_uv_backward', f.device, st, f.data_ptr(), lt.data_ptr(), rgba.data_ptr(), q.data_ptr(),
                    norm.data_ptr(), g.data_ptr(), grad_faces.data_ptr(), grad_light.data_ptr(), _lib.ptr(grad_packed), B, F, S,
                    per_batch, sigma, gamma, near, far, eps, background[0], background[1], background[2],
                    workspace_bytes=_lib.workspace_bytes('nr_soft_uv_workspace_bytes', st, B, F, S))
        grads = [None] * len(uv.images)
        if want_images:
            for m, (gi, im) in enumerate(zip(unpack_image_gradients(uv.layout, grad_packed), uv.images)):
                if ctx.needs_input_grad[4 + m]:   # an image shared by the batch: one row when every image is shared, else the rows summed
                    grads[m] = gi if im.dim() == 4 else (gi[0] if uv.batch is None else gi.sum(0))
        return (None, None, grad_faces, grad_light) + tuple(grads)


def soft_render_uv(faces, uv_images, light=None, image_size=256, sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3,
                   background_color=(0, 0, 0), implementation=None):
    """rgba [B,4,S,S] (row 0 the top row): faces [B,F,3,3] -- the rasterizer's input, without fill_back copies -- coloured by
    the images of a UVImages (uv_textures.py: images [H_m,W_m,3] shared by the batch or [B,H_m,W_m,3] per render), sampled at
    every taken pair with the bake's bilinear lookup at the pair's perspective-correct weights, times one light colour per
    face, light [B,F,3] or [1,F,3] (None: ones); aggregated by coverage and depth as soft_render does.

        C_f(p)_c = L_fc T_f(p)_c.  A face with an image m = face_image[f]: d_k = min(max(mu_k, 0), 1) (the clamp only removes
        rounding excess; its derivative is taken as 1), pos_x = (sum_k uvx_fk d_k)(W_m - 1), pos_y = (sum_k uvy_fk d_k)(H_m - 1),
        the four reads (yi,xi), (yi1,xi), (yi,xi+1), (yi1,xi+1) with xi = (int)pos_x, yi = (int)pos_y, yi1 = (int)(pos_y + 1),
        rows counted from the bottom of an image stored top row first, the flat index clamped into the image, weights wx0 wy0,
        wx0 wy1, wx1 wy0, wx1 wy1, summed in that order from 0.  A face without an image: the mean of its base cube, a constant.
        Inside a face this is the texture render() shows, outside the texture at the nearest boundary point: continuous
        across every edge.  Gradient, exact wherever the definition is differentiable (the read indices carry none; wx1 and
        wy1 move with pos): per taken pair dL/dI[q_r]_c += W g_c L_c w_r, dL/dL_fc += W g_c T_f(p)_c, and with G_k = sum_c g_c
        L_c (Tx_c uvx_fk (W - 1) + Ty_c uvy_fk (H - 1)), E_k = W zp (G_k - sum_j mu_j G_j) stands where the corner colours' E_k
        stands (module docstring).

    Differentiable, once, in faces (x, y and z), in every image tensor and in light; faces_uv, face_image and base receive no
    gradient.  On float32 CUDA tensors inside the ranges of include/nr_hip.h both directions are HIP kernels (nr_soft_uv_*):
    the gradients of faces and light are summed in a fixed order and repeat bit for bit; each entry of an image's gradient
    is rounded once from a double sum whose additions arrive in no fixed order -- its last bit may differ between runs.
    Everything else (`implementation='torch'`, sigma or gamma outside [1e-30, 1e30]) is soft_render_uv_torch on the layout's
    tensors.  No host tables beyond the layout's (uploaded on first use): a call may be captured (graph.capture) once one
    eager call has run -- but capture before any eager backward on the same leaves, or make the eager calls under no_grad, as
    for soft_silhouettes (DESIGN "Soft silhouettes", Stream capture).  The other arguments are soft_render's."""
    from .uv_textures import UVImages, pack_images
    name = 'soft_render_uv'
    B, F = _util.soft_check_faces(name, faces)
    if not isinstance(uv_images, UVImages):
        raise ValueError('%s: uv_images must be a UVImages' % name)
    if uv_images.layout.num_faces != F:
        raise ValueError('%s: the layout has %d faces, the call %d (the soft renderer takes no fill_back copies)'
                         % (name, uv_images.layout.num_faces, F))
    if uv_images.image_batch not in (1, B):
        raise ValueError('%s: batched images must have the batch size of the faces (%d), got %d' % (name, B, uv_images.image_batch))
    if uv_images.device != faces.device:
        raise ValueError('%s: images on %s, faces on %s' % (name, uv_images.device, faces.device))
    if light is None:
        light = torch.ones((1, F, 3), dtype=faces.dtype, device=faces.device)
    S, sigma, gamma, near, far, eps, background, hip = _check(name, faces, light, image_size, sigma, gamma, near, far, eps,
                                                              background_color, implementation, light=True)
    if hip:
        return _SoftRenderUV.apply(uv_images, (S, sigma, gamma, near, far, eps, background), faces, light, *uv_images.images)
    layout = uv_images.layout
    st = layout._tensors(faces.device)
    return soft_render_uv_torch(faces, st['faces_uv'], st['face_image'], st['base'], st['table'],
                                pack_images(uv_images.images, uv_images.batch), light, S, sigma, gamma, near, far, eps, background)


# ---------------------------------------------------------------------------------------------------------------------
# texture cubes

CUBE_MIN_TS, CUBE_MAX_TS = 2, 8   # the texture sizes of the HIP kernels (nr_soft_cubes_*)


class TextureCubes(object):
    """Texture cubes [B|1,F,ts,ts,ts,3] (ts >= 2, no fill_back copies) to be SAMPLED AT EVERY PIXEL by the soft renderer:
    Renderer.render_soft(vertices, faces, TextureCubes(t), per_pixel=True).  A bare 6-dim tensor keeps its meaning there (the
    mean of each cube); this wrapper only names the tensor, which stays the leaf that receives the gradient."""

    def __init__(self, textures):
        if not (torch.is_tensor(textures) and textures.is_floating_point() and textures.dim() == 6 and textures.shape[5] == 3
                and textures.shape[2] == textures.shape[3] == textures.shape[4] and textures.shape[2] >= 2):
            raise ValueError('TextureCubes: textures must be a float tensor [batch size or 1, num of faces, ts, ts, ts, 3] with '
                             'ts >= 2, got %s' % (tuple(textures.shape) if torch.is_tensor(textures) else type(textures).__name__,))
        self.textures = textures

    @property
    def texture_size(self):
        return int(self.textures.shape[2])


def soft_render_cubes_torch(faces, textures, light=None, image_size=256, sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3,
                            background_color=(0, 0, 0), texture_eps=1e-3):
    """rgba [B,4,S,S] in plain torch (any device, any float dtype) with texture cubes sampled at the pixel: faces [B,F,3,3],
    textures [B|1,F,ts,ts,ts,3], light [B|1,F,3] or None (ones).  soft_render_cubes' definition, differentiable by autograd in
    faces, textures and light; in chunks of pixel rows."""
    B, F = int(faces.shape[0]), int(faces.shape[1])
    dt, dev = faces.dtype, faces.device
    ts = int(textures.shape[2])
    T = ts ** 3
    tex = textures.to(dt).expand(B, F, ts, ts, ts, 3).reshape(B, F, T, 3)
    lit = (torch.ones((1, F, 3), dtype=dt, device=dev) if light is None else light.to(dt)).expand(B, F, 3)[:, None, None]
    hi = float(ts - 1) - float(texture_eps)
    bidx = torch.arange(B, device=dev)[:, None, None, None]
    fidx = torch.arange(F, device=dev)[None, None, None, :]

    def shade(u0, u1, u2, zp):
        cell, fr = [], []
        for u in (u0, u1, u2):   # both clamps with derivative 1; the cell carries no gradient
            v = (u * zp) * (ts - 1)
            c = torch.nan_to_num(v.detach(), nan=0.0).clamp(min=0)
            c = torch.clamp(c.double(), max=hi).to(dt)                         # (the min in double, then rounded)
            v = v + (c - v).detach()
            i = c.trunc()
            cell.append(i.long())
            fr.append(v - i)
        total = None
        for pn in range(8):
            w, idx = None, []
            for k in range(3):
                up = (pn >> k) & 1
                f_ = fr[k] if up else 1 - fr[k]
                w = f_ if w is None else w * f_
                idx.append(cell[k] + up)
            flat = (idx[0] * ts + idx[1]) * ts + idx[2]
            inside = flat < T                                                  # a tap outside the cube is skipped
            texel = tex[bidx, fidx, flat.clamp(max=T - 1)]                     # [B,rows,S,F,3]
            term = torch.where(inside[..., None], texel * w[..., None], torch.zeros((), dtype=dt, device=dev))
            total = term if total is None else total + term
        return [lit[..., c] * total[..., c] for c in range(3)]
    return _render_torch(faces, shade, 16, image_size, sigma, gamma, near, far, eps, background_color)


@_util.once_differentiable
class _SoftRenderCubes(torch.autograd.Function):
    """forward(ctx, faces [B,F,3,3], textures [B|1,F,ts,ts,ts,3], light [B|1,F,3], args) -> rgba [B,4,S,S], row 0 the top row:
    the nr_soft_cubes_* entries."""

    @staticmethod
    def forward(ctx, faces, textures, light, args):
        S, sigma, gamma, near, far, eps, background, texture_eps = args
        f, t, lt = _lib.dense(faces.detach()), _lib.dense(textures.detach()), _lib.dense(light.detach())
        B, F, ts = int(f.shape[0]), int(f.shape[1]), int(t.shape[2])
        tex_per_batch = 1 if int(t.shape[0]) == B else 0     # else [1,F,...]: one set for the batch, read in place
        light_per_batch = 1 if int(lt.shape[0]) == B else 0
        rgba = torch.empty((B, 4, S, S), dtype=torch.float32, device=f.device)
        q = torch.empty((B, S, S), dtype=torch.float32, device=f.device)
        norm = torch.empty((B, 2, S, S), dtype=torch.float32, device=f.device)
        _lib.launch('nr_soft_cubes_forward', f.device, f.data_ptr(), t.data_ptr(), lt.data_ptr(), rgba.data_ptr(), q.data_ptr(),
                    norm.data_ptr(), B, F, S, ts, tex_per_batch, light_per_batch, sigma, gamma, near, far, eps, background[0],
                    background[1], background[2], texture_eps,
                    workspace_bytes=_lib.workspace_bytes('nr_soft_cubes_workspace_bytes', B, F, S, ts, tex_per_batch))
        ctx.save_for_backward(f, t, lt, rgba, q, norm)
        ctx.args, ctx.per_batch = args, (tex_per_batch, light_per_batch)
        return rgba.flip(2)

    @staticmethod
    def backward(ctx, grad_rgba):
        f, t, lt, rgba, q, norm = ctx.saved_tensors
        S, sigma, gamma, near, far, eps, background, texture_eps = ctx.args
        tex_per_batch, light_per_batch = ctx.per_batch
        B, F, ts = int(f.shape[0]), int(f.shape[1]), int(t.shape[2])
        g = _lib.dense(grad_rgba.flip(2))
        grad_faces, grad_light = torch.empty_like(f), torch.empty_like(lt)
        grad_textures = torch.empty_like(t) if ctx.needs_input_grad[1] else None   # (every entry is stored by the kernels)
        _lib.launch('nr_soft_cubes_backward', f.device, f.data_ptr(), t.data_ptr(), lt.data_ptr(), rgba.data_ptr(), q.data_ptr(),
                    norm.data_ptr(), g.data_ptr(), grad_faces.data_ptr(), grad_light.data_ptr(), _lib.ptr(grad_textures), B, F, S,
                    ts, tex_per_batch, light_per_batch, sigma, gamma, near, far, eps, background[0], background[1],
                    background[2], texture_eps,
                    workspace_bytes=_lib.workspace_bytes('nr_soft_cubes_workspace_bytes', B, F, S, ts, tex_per_batch))
        return grad_faces, grad_textures, grad_light, None


def soft_render_cubes(faces, textures, light=None, image_size=256, sigma=1e-4, gamma=1e-4, near=0.1, far=100, eps=1e-3,
                      background_color=(0, 0, 0), texture_eps=1e-3, implementation=None):
    """rgba [B,4,S,S] (row 0 the top row): faces [B,F,3,3] -- the rasterizer's input, without fill_back copies -- coloured by
    the rasterizer's texture cubes, textures [B,F,ts,ts,ts,3] or [1,F,ts,ts,ts,3] shared by the batch (ts >= 2, no fill_back
    copies), sampled at every taken pair with the rasterizer's trilinear lookup at the pair's perspective-correct weights, times
    one light colour per face, light [B,F,3] or [1,F,3] (None: ones); aggregated by coverage and depth as soft_render does.
    Everything in the module docstring stands -- u_k, zp, mu_k = u_k zp, m, w_f, Z, Q and alpha -- except the colour of a
    taken pair:

        C_f(p)_c = L_fc T_f(p)_c.  v_k = mu_k (ts - 1); v_k = max(v_k, 0); v_k = (float)min((double)v_k, (double)(ts - 1) -
        texture_eps): the rasterizer's sequence with mu_k where it has w_k (zp / z_k).  i_k = (int)v_k, fr_k = v_k - i_k; eight
        taps pn = 0..7, bit k of pn picks (i_k + 1, fr_k), else (i_k, 1 - fr_k); the weight is the product over k in that
        order, the flat index (i_0 ts + i_1) ts + i_2 of the picked indices.  A tap whose flat index is >= ts^3 is skipped,
        never read: its weight is an exact 0, and nothing from outside the cube comes in.  T is the sum from 0 in tap order.
        Inside a face this is the texture render() shows, outside the texture at the nearest boundary point: continuous
        across every edge, as the corner colours are.
        Gradient, exact wherever the definition is differentiable.  The tap indices carry none.  Both clamps are taken with
        derivative 1, as soft_render_uv takes its clamp: the lower one removes rounding excess only; THE UPPER ONE ACTS ON A
        SLIVER OF RELATIVE WIDTH texture_eps / (ts - 1) AT A VERTEX, WHERE THE GRADIENT IS THE UNCLAMPED DERIVATIVE; where an
        outside pair's nearest point is a vertex, mu = (1, 0, 0) and every term that would differ is multiplied by an exact
        0.  Per taken pair dL/dtex[f][tap_pn]_c += W g_c L_c w_pn, dL/dL_fc += W g_c T_f(p)_c, and with D_kc = sum_pn
        (dw_pn / dfr_k) tex[tap_pn]_c and G_k = (ts - 1) sum_c g_c L_c D_kc, E_k = W zp (G_k - sum_j mu_j G_j) stands where the
        corner colours' E_k stands (module docstring).

    texture_eps (the rasterizer's `eps`; a finite host number with 0 <= texture_eps < 1) is not `eps`, which places the
    background in the depth order.  Differentiable, once, in faces (x, y and z), textures and light.  On float32 CUDA tensors
    inside the ranges of include/nr_hip.h and with 2 <= ts <= 8 both directions are HIP kernels (nr_soft_cubes_*): every
    gradient, the cubes' included, is summed in a fixed order without atomics and repeats bit for bit, for an image alone or
    inside a batch.  Everything else (`implementation='torch'`, a larger ts, sigma or gamma outside [1e-30, 1e30]) is
    soft_render_cubes_torch.  No host tables: a call may be captured (graph.capture) -- but capture before any eager backward on
    the same leaves, or make the eager calls under no_grad, as for soft_silhouettes (DESIGN "Soft silhouettes", Stream
    capture).  Not done: a light per corner, fill_back-transposed cubes, cubes larger than 8 in HIP.  The other arguments are
    soft_render's."""
    name = 'soft_render_cubes'
    B, F = _util.soft_check_faces(name, faces)
    if isinstance(textures, TextureCubes):
        textures = textures.textures
    if not (torch.is_tensor(textures) and textures.is_floating_point() and textures.dim() == 6 and textures.shape[5] == 3
            and textures.shape[2] == textures.shape[3] == textures.shape[4] and textures.shape[2] >= 2
            and textures.shape[1] == F and textures.shape[0] in (1, B)):
        raise ValueError('%s: textures must be a float tensor [batch size or 1, num of faces (%d), ts, ts, ts, 3] with ts >= 2 '
                         '(the soft renderer takes no fill_back copies), got %s'
                         % (name, F, tuple(textures.shape) if torch.is_tensor(textures) else type(textures).__name__))
    if textures.device != faces.device:
        raise ValueError('%s: textures on %s, faces on %s' % (name, textures.device, faces.device))
    texture_eps = _util.number(name, 'texture_eps', texture_eps)
    if not (0 <= texture_eps < 1):
        raise ValueError('%s: texture_eps must be a finite number with 0 <= texture_eps < 1, got %r' % (name, texture_eps))
    if light is None:
        light = torch.ones((1, F, 3), dtype=faces.dtype, device=faces.device)
    ts = int(textures.shape[2])
    fits = textures.dtype == faces.dtype and CUBE_MIN_TS <= ts <= CUBE_MAX_TS and F * ts ** 3 * 3 < 2 ** 31 - 256
    S, sigma, gamma, near, far, eps, background, hip = _check(name, faces, light, image_size, sigma, gamma, near, far, eps,
                                                              background_color, implementation if fits else
                                                              _cubes_do_not_fit(name, implementation), light=True)
    if hip and fits:
        return _SoftRenderCubes.apply(faces, textures, light, (S, sigma, gamma, near, far, eps, background, texture_eps))
    return soft_render_cubes_torch(faces, textures, light, S, sigma, gamma, near, far, eps, background, texture_eps)


def _cubes_do_not_fit(name, implementation):
    """takes_hip's sentence for cubes outside the HIP kernels' range -> 'torch' for every implementation that may take it."""
    _util.takes_hip(name, implementation, False, 'the HIP kernels take float32 CUDA cubes of the faces\' dtype with a texture size '
                    'from %d to %d (larger cubes run in torch) and num of faces * ts^3 * 3 < 2^31 - 256' % (CUBE_MIN_TS, CUBE_MAX_TS))
    return 'torch'
