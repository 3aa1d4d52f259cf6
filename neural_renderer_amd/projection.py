"""Projection camera: intrinsics K, pose R | t and OpenCV lens distortion (not in the reference).

`projection(vertices, K, R, t, dist_coeffs, orig_size)` maps world-space vertices [B, Nv, 3] to the rasterizer's input:
NDC x and y (y up) and camera depth.  For vertex w of image b, in float32:

    c   = R[b] @ w + t[b]                   camera space, OpenCV axes: x right, y down, z forward
    x'  = c.x / c.z,  y' = c.y / c.z
    r2  = x'^2 + y'^2
    rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3     dist_coeffs = (k1, k2, p1, p2, k3), OpenCV order
    x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2)
    y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y'
    u   = K[0,0] x'' + K[0,1] y'' + K[0,2]  (row 2 of K is ignored)
    v   = K[1,0] x'' + K[1,1] y'' + K[1,2]
    out = ((2u - orig_size) / orig_size, (orig_size - 2v) / orig_size, c.z)

u and v are continuous pixel coordinates of an orig_size x orig_size image in which pixel i spans [i, i+1): with
orig_size == image_size, a point at u = i + 0.5, v = j + 0.5 lands on the centre of column i and of row j counted from the
TOP of the rendered image -- the photo's own row, so renders overlay the photo without flipping.  OpenCV intrinsics put
pixel centres at integers: add 0.5 to cx and cy when you take K from OpenCV.

K [3,3] or [B,3,3]; R [3,3] or [B,3,3] (world -> camera); t [3], [B,3] or [B,1,3]; dist_coeffs None (no distortion) or
[5] / [B,5]; orig_size a positive number (square images only).  Nothing is clamped: points at c.z <= near are culled by
the rasterizer.  Works on any device and dtype with autograd; Renderer(camera_mode='projection') runs the same model in the
fused HIP front-end (csrc/nr_frontend.hip) on CUDA float32 inputs.
"""
import torch

from ._util import as_tensor_like


def _param(value, ref, batch_size, shape):
    """list / ndarray / tensor of shape `shape` or [B] + shape -> [B] + shape tensor in ref's dtype and device."""
    p = as_tensor_like(value, ref, dtype=ref.dtype)
    if tuple(p.shape) == shape:
        return p[None].expand((batch_size,) + shape)
    if p.dim() == len(shape) + 1 and tuple(p.shape[1:]) == shape:
        return p
    raise ValueError('expected a parameter of shape %s or [B, %s], got %s' % (list(shape), ', '.join(map(str, shape)),
                                                                             list(p.shape)))


def projection(vertices, K, R, t, dist_coeffs=None, orig_size=None):
    assert vertices.dim() == 3 and vertices.shape[2] == 3
    if orig_size is None:
        raise ValueError('projection needs orig_size')
    B = vertices.shape[0]
    K = _param(K, vertices, B, (3, 3))
    R = _param(R, vertices, B, (3, 3))
    t = as_tensor_like(t, vertices, dtype=vertices.dtype)
    if t.dim() == 3 and t.shape[1] == 1:
        t = t[:, 0]
    t = _param(t, vertices, B, (3,))

    c = torch.matmul(vertices, R.transpose(1, 2)) + t[:, None, :]
    x = c[..., 0] / c[..., 2]
    y = c[..., 1] / c[..., 2]
    if dist_coeffs is not None:
        d = _param(dist_coeffs, vertices, B, (5,))
        k1, k2, p1, p2, k3 = [d[:, i, None] for i in range(5)]
        r2 = x * x + y * y
        r4 = r2 * r2
        rad = 1 + k1 * r2 + k2 * r4 + k3 * (r4 * r2)
        x, y = (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x),
                y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
    u = K[:, 0, 0, None] * x + K[:, 0, 1, None] * y + K[:, 0, 2, None]
    v = K[:, 1, 0, None] * x + K[:, 1, 1, None] * y + K[:, 1, 2, None]
    return torch.stack(((2 * u - orig_size) / orig_size, (orig_size - 2 * v) / orig_size, c[..., 2]), dim=2)
