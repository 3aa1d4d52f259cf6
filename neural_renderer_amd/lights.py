"""Learnable lights (not in the reference): light parameters as tensors -- shared by the batch or one per image, possibly
learnable -- and nine spherical-harmonics (SH) coefficients per colour channel next to the reference's ambient term and
directional lamp.

With n = N / (|N| + 1e-5) = (x, y, z) the unit normal of a face (flat) or of a vertex (smooth: N is the sum of the normals of
the faces around it, area-weighted), the light colour is

    L_c(n) = Ia Ca_c + Id (Cd_c max(n . d, 0)) + sum_k sh[k, c] Y_k(n)          k = 0 .. 8, added in ascending order
    Y0 = c0   Y1 = c1 y   Y2 = c1 z   Y3 = c1 x   Y4 = c2 x y   Y5 = c2 y z   Y6 = c3 (3 z^2 - 1)   Y7 = c2 x z   Y8 = c4 (x^2 - y^2)
    c0 = 0.282095  c1 = 0.488603  c2 = 1.092548  c3 = 0.315392  c4 = 0.546274

The first two terms are lighting()'s, in its operation order.  `d` is not normalised (as in the reference) and L is not
clamped: the `sh` rows are IRRADIANCE coefficients -- the cosine lobe is already folded into them, they are what a fit to
images recovers -- not the radiance coefficients of an environment map.  The reversed copy of a face (fill_back) sees -n.
A zero normal (a degenerate face, a vertex without a face) gives n = 0: the light is Ia Ca + c0 sh[0] - c3 sh[6] and nothing
flows back to the vertices; the derivative of max(., 0) is taken for n . d > 0 strictly.

`light_colors` evaluates this for a mesh: [B,F,3] (flat) or [B,F,3,3] (smooth, per corner), exactly what the rasterizer takes as
`face_light`.  On CUDA float32 tensors it runs as HIP kernels in both directions (include/nr_hip.h: nr_light_colors_forward /
_backward; csrc/nr_lights.hip): the parameters stay on the device, so a call never synchronises and can be captured into a graph
-- after one eager call with the same index tensor, which builds the vertex adjacency table (vertex_colors.py).  Neither
direction uses atomics: every output repeats bit for bit.  `Renderer.lights = Lights(...)` makes render() take its light from
here instead of the host attributes `light_*`.
"""
import numpy as np
import torch
from torch import nn

from . import _lib, _util
from .vertex_colors import _adjacency

NAMES = ('intensity_ambient', 'intensity_directional', 'color_ambient', 'color_directional', 'direction', 'sh')
_SHAPES = {'intensity_ambient': (), 'intensity_directional': (), 'color_ambient': (3,), 'color_directional': (3,),
           'direction': (3,), 'sh': (9, 3)}
# c0 .. c4 as the float32 numbers the kernels hold, also in a float64 evaluation
SH_C = tuple(float(np.float32(c)) for c in (0.282095, 0.488603, 1.092548, 0.315392, 0.546274))


def _per_image(name, value):
    """False / True: `value` is shared / one per image; raises for any other shape.  A [1] intensity counts as shared."""
    shape, want = tuple(value.shape), _SHAPES[name]
    if shape == want or (want == () and shape == (1,)):
        return False
    if len(shape) == len(want) + 1 and shape[1:] == want and shape[0] >= 1:
        return True
    raise ValueError('Lights.%s must have shape %s (shared) or %s (one per image), got %s'
                     % (name, list(want), ['batch size'] + list(want), list(shape)))


class Lights(nn.Module):
    """The light of a render as tensors: intensities (numbers, or [B]), colours and the lamp's direction ([3] or [B,3]) and
    `sh`, nine SH irradiance coefficients per colour channel ([9,3] or [B,9,3]; None: no SH term) -- see the module
    docstring for the formula.  Values are numbers, sequences or tensors.  The names in `learnable` become nn.Parameters
    (copies of the values given), the others buffers; a buffer may be assigned any tensor later, also one that carries a
    gradient (`lights.sh = net(x)`).  Float32 on the CPU unless tensors say otherwise: move it with `.to(device)`."""

    def __init__(self, intensity_ambient=0.5, intensity_directional=0.5, color_ambient=(1, 1, 1), color_directional=(1, 1, 1),
                 direction=(0, 1, 0), sh=None, learnable=()):
        super(Lights, self).__init__()
        learnable = (learnable,) if isinstance(learnable, str) else tuple(learnable)
        unknown = [n for n in learnable if n not in NAMES]
        if unknown:
            raise ValueError('Lights: learnable names must be among %s, got %s' % (', '.join(NAMES), unknown))
        values = dict(zip(NAMES, (intensity_ambient, intensity_directional, color_ambient, color_directional, direction, sh)))
        for name in NAMES:
            value = values[name]
            if value is None:
                if name != 'sh':
                    raise ValueError('Lights.%s is required (only sh may be None)' % name)
                if 'sh' in learnable:
                    raise ValueError("Lights: a learnable sh needs start values (e.g. torch.zeros(9, 3))")
                self.register_buffer('sh', None)
                continue
            if not torch.is_tensor(value):
                value = torch.as_tensor(np.asarray(value, dtype=np.float32))
            if not value.is_floating_point():
                value = value.to(torch.float32)
            _per_image(name, value)
            if name in learnable:
                self.register_parameter(name, nn.Parameter(value.detach().clone()))
            else:
                self.register_buffer(name, value)

    @classmethod
    def from_renderer(cls, renderer, sh=None, learnable=()):
        """The host light attributes of a Renderer (`light_*`) as a Lights."""
        return cls(renderer.light_intensity_ambient, renderer.light_intensity_directional, renderer.light_color_ambient,
                   renderer.light_color_directional, renderer.light_direction, sh=sh, learnable=learnable)

    def tensors(self):
        """The six parameters in the C ABI's order (sh may be None)."""
        return tuple(getattr(self, n) for n in NAMES)


def _check(vertices, faces, lights):
    """Shape / dtype / device checks shared by both implementations -> (B, Nv, Nf, the six tensors, per-image flags)."""
    if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3 and vertices.is_floating_point()):
        raise ValueError('light_colors: vertices must be a float tensor [batch size, num of vertices, 3]')
    B, Nv = int(vertices.shape[0]), int(vertices.shape[1])
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dim() in (2, 3) and faces.shape[-1] == 3
            and faces.shape[-2] >= 1):
        raise ValueError('light_colors: faces must be an integer tensor [num of faces, 3] or [batch size, num of faces, 3]')
    if faces.dim() == 3 and faces.shape[0] != B:
        raise ValueError('light_colors: faces have batch size %d, vertices %d' % (faces.shape[0], B))
    if faces.device != vertices.device:
        raise ValueError('light_colors: faces are on %s, vertices on %s' % (faces.device, vertices.device))
    if not isinstance(lights, Lights):
        raise ValueError('light_colors: lights must be a Lights, got %s' % type(lights).__name__)
    params, flags = lights.tensors(), []
    for name, p in zip(NAMES, params):
        if p is None:
            flags.append(False)
            continue
        if not torch.is_tensor(p):
            raise ValueError('Lights.%s must be a tensor' % name)
        per_image = _per_image(name, p)
        if per_image and p.shape[0] != B:
            raise ValueError('Lights.%s holds %d images, vertices %d' % (name, p.shape[0], B))
        if p.dtype != vertices.dtype:
            raise ValueError('Lights.%s is %s, vertices %s' % (name, p.dtype, vertices.dtype))
        if p.device != vertices.device:
            raise ValueError('Lights.%s is on %s, vertices on %s' % (name, p.device, vertices.device))
        flags.append(per_image)
    return B, Nv, int(faces.shape[-2]), params, flags


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _sh_basis(u):
    """Y_0 .. Y_8 at unit vectors u [...,3] -> [...,9], in the kernels' operation order."""
    c0, c1, c2, c3, c4 = SH_C
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    return torch.stack((torch.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0),
                        c2 * x * z, c4 * (x * x - y * y)), dim=-1)


def light_colors_torch(vertices, faces, lights, fill_back=True, smooth=False):
    """light_colors in plain torch: any device, any float dtype."""
    B, Nv, Nf, params, flags = _check(vertices, faces, lights)
    ia, idir, ca, cd, d, sh = (None if p is None else (p if f else p.reshape((1,) + _SHAPES[n]).expand((B,) + _SHAPES[n]))
                               for n, p, f in zip(NAMES, params, flags))
    idx = faces.long()
    if idx.dim() == 2:
        idx = idx[None].expand(B, -1, -1)
    batch = torch.arange(B, device=vertices.device)[:, None, None]
    fv = vertices[batch, idx]  # [B,Nf,3,3]
    n = torch.cross(fv[:, :, 0] - fv[:, :, 1], fv[:, :, 2] - fv[:, :, 1], dim=2)
    if smooth:
        m = torch.zeros((B, Nv, 3), dtype=vertices.dtype, device=vertices.device)
        for k in range(3):
            m = m.scatter_add(1, idx[:, :, k, None].expand(B, Nf, 3), n)
        n = m
    sq = (n * n).sum(2, keepdim=True)
    zero = sq == 0  # n = 0: n_hat = 0 and no gradient (sqrt's derivative at 0 would make it NaN)
    nh = torch.where(zero, torch.zeros_like(n), n / (torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)) + 1e-5))
    dot = (nh[:, :, 0] * d[:, None, 0] + nh[:, :, 1] * d[:, None, 1]) + nh[:, :, 2] * d[:, None, 2]
    amb = (ia[:, None] * ca)[:, None, :]

    def seen(u, cosv):
        light = amb + idir[:, None, None] * (cd[:, None, :] * cosv[:, :, None])
        if sh is not None:
            Y = _sh_basis(u)  # [B,N,9]
            for k in range(9):
                light = light + sh[:, None, k, :] * Y[:, :, k, None]
        return light

    front = seen(nh, torch.relu(dot))
    back = seen(-nh, torch.relu(-dot)) if fill_back else None
    if smooth:
        front = front[batch, idx]  # [B,Nf,3,3]
        return torch.cat((front, torch.flip(back[batch, idx], dims=[2])), dim=1) if fill_back else front
    return torch.cat((front, back), dim=1) if fill_back else front


# ---------------------------------------------------------------------------------------------------------------------
# HIP

def _lights_struct(params, flags):
    s = _lib.Lights()
    for name, p in zip(NAMES, params):
        setattr(s, name, _lib.ptr(p))
    s.per_image = sum(1 << j for j, f in enumerate(flags) if f)
    return s


@_util.once_differentiable
class _LightColors(torch.autograd.Function):
    """forward(ctx, setup, vertices [B,Nv,3], ia, id, ca, cd, direction, sh | None) -> [B,F,3] | [B,F,3,3];
    setup = (indices, offsets, entries, idx_per_batch, per-image flags, fill_back, smooth)."""

    @staticmethod
    def forward(ctx, setup, vertices, *params):
        idx, off, ent, per_batch, flags, fill_back, smooth = setup
        v = _lib.dense(vertices.detach())
        params = tuple(None if p is None else _lib.dense(p.detach()) for p in params)
        dev = v.device
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        F = 2 * Nf if fill_back else Nf
        out = torch.empty((B, F, 3, 3) if smooth else (B, F, 3), dtype=torch.float32, device=dev)
        _lib.launch('nr_light_colors_forward', dev, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    _lights_struct(params, flags), out.data_ptr(), B, Nv, Nf, int(per_batch), int(fill_back), int(smooth),
                    workspace_bytes=_lib.workspace_bytes('nr_light_colors_workspace_bytes', B, Nv, Nf, 1) if smooth else 0)
        ctx.save_for_backward(v, *params)
        ctx.setup = setup
        return out

    @staticmethod
    def backward(ctx, grad_light):
        v, *params = ctx.saved_tensors
        idx, off, ent, per_batch, flags, fill_back, smooth = ctx.setup
        need = ctx.needs_input_grad[1:]
        if not any(need):
            return (None,) * (2 + len(params))
        dev = v.device
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        g = _lib.dense(grad_light)
        grad_v = torch.empty_like(v) if need[0] else None
        grads = tuple(torch.empty_like(p) if (n and p is not None) else None for p, n in zip(params, need[1:]))
        out = _lib.LightsGrad()
        for name, t in zip(NAMES, grads):
            setattr(out, name, _lib.ptr(t))
        _lib.launch('nr_light_colors_backward', dev, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    _lights_struct(params, flags), g.data_ptr(), _lib.ptr(grad_v), out, B, Nv, Nf, int(per_batch), int(fill_back),
                    int(smooth), workspace_bytes=_lib.workspace_bytes('nr_light_colors_workspace_bytes', B, Nv, Nf, int(smooth)))
        return (None, grad_v) + grads


def light_colors(vertices, faces, lights, fill_back=True, smooth=False, implementation=None):
    """The light colour of every face, [B,F,3] (smooth = False), or of every face corner, [B,F,3,3] (smooth = True: computed
    at the vertices from their area-weighted normals; the corners of a reversed copy in its own, flipped order), from
    world-space vertices [B,Nv,3], faces [Nf,3] | [B,Nf,3] and a Lights; F = Nf, or 2 Nf with fill_back.  Differentiable in
    the vertices and in every light tensor that requires a gradient.  `implementation`: None picks the HIP kernels for float32
    CUDA tensors, 'torch' is plain torch on any device and float dtype, 'hip' raises when the call does not fit the kernels.
    The HIP path builds the vertex adjacency table of an index tensor on the host the first time it sees it: inside a graph
    capture an unknown index tensor raises -- call once eagerly first."""
    B, Nv, Nf, params, flags = _check(vertices, faces, lights)
    fits = vertices.is_cuda and vertices.dtype == torch.float32 and B <= 65535
    if not _util.takes_hip('light_colors', implementation, fits, 'the HIP kernels take float32 CUDA tensors and at most 65535 '
                           'images'):
        return light_colors_torch(vertices, faces, lights, fill_back, smooth)
    _util.check_face_indices(faces, Nv, vertices.device)
    idx, off, ent, per_batch = _adjacency(faces, Nv)
    setup = (idx, off, ent, per_batch, tuple(flags), bool(fill_back), bool(smooth))
    return _LightColors.apply(setup, vertices, *params)
