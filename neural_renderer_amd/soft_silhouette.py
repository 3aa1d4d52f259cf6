"""Soft silhouettes (not in the reference): a probabilistic silhouette of the Soft Rasterizer family with the exact gradient
of its definition, next to the hard rasterizer whose approximate gradient exists only where an edge sweeps across a pixel.

`faces` [B,F,3,3] are the rasterizer's own input -- x, y in NDC with y up, z the positive camera depth (Renderer._frontend,
Renderer._project) -- WITHOUT fill_back copies: a duplicated face would count twice.  The output is alpha [B,S,S], row 0 the
top row, rendered at S directly (no anti-aliasing).  The pixel centre of column xi and internal row yi (row 0 at the bottom)
is (2 i + 1 - S) / S, as in the rasterizer.

    A face contributes iff its nine coordinates are finite and near <= z_k <= far at its three vertices; any other face is
    absent from every product and has a zero gradient.  Orientation plays no role.
    Per contributing face f and pixel p, with the segments 0, 1, 2 = v0v1, v1v2, v2v0:
      c_k   the nearest point of segment k to p, parameter clamped to [0, 1]; a zero-length segment gives its endpoint
      d2    min_k |p - c_k|^2, the lowest k on a tie
      s     +1 if the three edge functions of p are all > 0 or all < 0, else -1 (a zero-area face has no inside)
      x     s d2 / sigma,  D = 1 / (1 + e^-x)
    Q_p = the product over f, ascending, of 1 - D_pf evaluated as 1 / (1 + e^x);  alpha_p = 1 - Q_p.
    Gradient, with G_p = g_p Q_p: dL/dx_pf = G_p D_pf (no division by 1 - D).  For the chosen segment a -> b with nearest
    point c = a + t (b - a) and r = p - c: d d2 / da = -2 (1 - t) r, d d2 / db = -2 t r -- a clamped t hands the whole of -2 r
    to that endpoint --, times s / sigma, summed over the pixels.  The third vertex and every z receive 0.

sigma is a host float > 0 without a gradient; the operator is once-differentiable.  On float32 CUDA tensors inside the
ranges of include/nr_hip.h the two directions are HIP kernels (nr_soft_silhouette_*), which leave out the (pixel, face) pairs
outside the face's bounding box grown by sqrt(17 sigma) (there D < 2^-24); `soft_silhouettes_torch` serves everything else in
plain torch with the same definition and tie rule, and leaves nothing out.  No host tables: a first call may be captured
(graph.capture) -- but capture before any eager backward on the same leaves, or make the eager calls under no_grad: a
capture after a whole eager step ended the process inside torch's capture_end (DESIGN "Soft silhouettes", Stream capture).
"""
import torch

from . import _lib, _util

_CHUNK_ELEMENTS = 2 ** 26   # soft_silhouettes_torch: the most elements of one temporary


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def soft_silhouettes_torch(faces, image_size=256, sigma=1e-4, near=0.1, far=100):
    """alpha [B,S,S] in plain torch (any device, any float dtype), differentiable by autograd; the module docstring's
    definition over every (pixel, face) pair, in chunks of pixel rows."""
    B, F, S = int(faces.shape[0]), int(faces.shape[1]), int(image_size)
    z = faces[:, :, :, 2]
    on = (torch.isfinite(faces).all(3).all(2) & (z >= near).all(2) & (z <= far).all(2))   # [B,F]
    xy = torch.where(on[:, :, None, None], faces[..., :2], torch.zeros_like(faces[..., :2]))
    v = [[xy[:, None, None, :, k, c] for c in range(2)] for k in range(3)]   # [B,1,1,F]
    on = on[:, None, None, :]
    centre = (2 * torch.arange(S, device=faces.device, dtype=torch.float64) + 1 - S) / S
    centre = centre.to(faces.dtype)
    px = centre[None, None, :, None]
    rows = max(1, _CHUNK_ELEMENTS // max(1, B * S * F))
    out = []
    for r0 in range(0, S, rows):
        py = centre[None, r0:r0 + rows, None, None]
        d0, c0, _ = _util.soft_segment(px, py, v[0][0], v[0][1], v[1][0], v[1][1])
        d1, c1, _ = _util.soft_segment(px, py, v[1][0], v[1][1], v[2][0], v[2][1])
        d2, c2, _ = _util.soft_segment(px, py, v[2][0], v[2][1], v[0][0], v[0][1])
        d = torch.where(d1 < d0, d1, d0)   # strict: the lowest segment wins a tie
        d = torch.where(d2 < d, d2, d)
        inside = ((c0 > 0) & (c1 > 0) & (c2 > 0)) | ((c0 < 0) & (c1 < 0) & (c2 < 0))
        x = torch.where(inside, d, -d) / sigma
        q = torch.where(on, torch.sigmoid(-x), torch.ones_like(x)).prod(3).detach()   # 1 - D = 1 / (1 + e^x)
        # the gradient in the definition's form, G D: alpha = 1 - Q with d alpha / dx = Q D = -Q d ln(1 - D) / dx, so the
        # value comes from the product and the derivative from Q times the sum of the logarithms (which adds an exact 0)
        ln_q = torch.where(on, torch.nn.functional.logsigmoid(-x), torch.zeros_like(x)).sum(3)
        out.append((1 - q) + q * torch.where(q > 0, ln_q.detach() - ln_q, torch.zeros_like(ln_q)))
    return torch.cat(out, 1).flip(1)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

@_util.once_differentiable
class _SoftSilhouettes(torch.autograd.Function):
    """forward(ctx, faces [B,F,3,3], image_size, sigma, near, far) -> alpha [B,S,S], row 0 the top row."""

    @staticmethod
    def forward(ctx, faces, image_size, sigma, near, far):
        f = _lib.dense(faces.detach())
        B, F, S = int(f.shape[0]), int(f.shape[1]), image_size
        alpha = torch.empty((B, S, S), dtype=torch.float32, device=f.device)
        q = torch.empty_like(alpha)
        _lib.launch('nr_soft_silhouette_forward', f.device, f.data_ptr(), alpha.data_ptr(), q.data_ptr(), B, F, S, sigma, near,
                    far, workspace_bytes=_lib.workspace_bytes('nr_soft_silhouette_workspace_bytes', B, F, S))
        ctx.save_for_backward(f, q)
        ctx.args = (S, sigma, near, far)
        return alpha.flip(1)

    @staticmethod
    def backward(ctx, grad_alpha):
        f, q = ctx.saved_tensors
        S, sigma, near, far = ctx.args
        B, F = int(f.shape[0]), int(f.shape[1])
        g = _lib.dense(grad_alpha.flip(1))
        grad_faces = torch.empty_like(f)
        _lib.launch('nr_soft_silhouette_backward', f.device, f.data_ptr(), q.data_ptr(), g.data_ptr(), grad_faces.data_ptr(),
                    B, F, S, sigma, near, far,
                    workspace_bytes=_lib.workspace_bytes('nr_soft_silhouette_workspace_bytes', B, F, S))
        return grad_faces, None, None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# the public function

def _check(name, faces, image_size, sigma, near, far, implementation):
    """Argument checks shared by both implementations -> (image_size, sigma, near, far, takes the HIP path)."""
    _util.soft_check_faces(name, faces)
    _util.soft_check_image_size(name, image_size)
    sigma = _util.number(name, 'sigma', sigma)
    if not (0 < sigma < float('inf')):
        raise ValueError('%s: sigma must be a finite number greater than 0, got %r' % (name, sigma))
    near, far = _util.number(name, 'near', near), _util.number(name, 'far', far)
    fits = _util.soft_fits(faces, image_size) and 1e-30 <= sigma <= 1e30
    return image_size, sigma, near, far, _util.takes_hip(
        name, implementation, fits, 'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most, at most 2^24 '
        'faces (batch size * faces * 9 < 2^31), an image_size of 16384 at most and 1e-30 <= sigma <= 1e30')


def soft_silhouettes(faces, image_size=256, sigma=1e-4, near=0.1, far=100, implementation=None):
    """alpha [B,S,S] (row 0 the top row): the soft silhouette of faces [B,F,3,3] -- the rasterizer's input, without
    fill_back copies -- at image_size S (module docstring).  Differentiable in faces (x and y; z gets 0), once.  sigma, in
    squared NDC units, sets the width of the transition: a host float > 0 without a gradient.  `implementation`: None picks
    the HIP kernels for float32 CUDA tensors inside their ranges, 'torch' / 'hip' force one ('hip' raises when the call does
    not fit)."""
    S, sigma, near, far, hip = _check('soft_silhouettes', faces, image_size, sigma, near, far, implementation)
    if hip:
        return _SoftSilhouettes.apply(faces, S, sigma, near, far)
    return soft_silhouettes_torch(faces, S, sigma, near, far)
