"""Per-vertex colours and smooth shading (not in the reference).

`Renderer.render(vertices, faces, VertexColors(colors))` colours a mesh by its vertices: `vertex_shade` turns the vertex
colours and the light into three lit colours per face, one per corner (`CornerColors`), and the rasterizer interpolates them
perspective-correctly at every covered pixel (include/nr_hip.h: nr_forward_rasterize_corner).  `Renderer.shading` picks the
light: 'flat' is the reference's one colour per face (lighting.py), 'smooth' computes it at the vertices from area-weighted
vertex normals (Gouraud shading), so a coarse sphere stops looking faceted and the light's gradient becomes a smooth function
of the vertex positions.

On CUDA float32 tensors with host light parameters (`frontend.light_fusable`) `vertex_shade` runs as HIP kernels in both
directions (nr_vertex_shade_forward / _backward).  Every sum over the faces around a vertex is a gather through a
vertex -> (face, corner) table, so neither direction uses atomics and the results repeat bit for bit.  The table is built on
the host from the index tensor the first time a topology is seen and cached on that tensor: the build reads the indices back,
so it must happen BEFORE a graph capture -- run one eager step with the same index tensor first (inside a capture an
unknown topology raises).  An index tensor [B,Nf,3] whose images differ gets one table per image; one whose images are all
equal (the usual `faces[None].expand(B, ...)`) shares a single table.  CPU tensors, other dtypes and per-image light tensors
take the plain-torch implementation `vertex_shade_torch`, which is also the kernels' second yardstick in the tests.
"""
import numpy as np
import torch

from . import _lib, _util
from ._util import as_tensor_like
from .frontend import _is_number, _vec3


class VertexColors(object):
    """Per-vertex colours for Renderer.render: a float32 tensor [Nv,3] (shared by the batch) or [B,Nv,3], possibly learnable.
    Holds a reference, no copy."""

    def __init__(self, colors):
        if not torch.is_tensor(colors):
            raise ValueError('VertexColors: a tensor [num of vertices, 3] or [batch size, num of vertices, 3] expected')
        if colors.dtype != torch.float32 or colors.dim() not in (2, 3) or colors.shape[-1] != 3 or colors.shape[-2] < 1:
            raise ValueError('VertexColors: colors must be float32 [num of vertices, 3] or [batch size, num of vertices, 3], '
                             'got %s %s' % (colors.dtype, tuple(colors.shape)))
        self.colors = colors

    @property
    def color_batch(self):
        return 1 if self.colors.dim() == 2 else int(self.colors.shape[0])

    @property
    def num_vertices(self):
        return int(self.colors.shape[-2])

    @property
    def device(self):
        return self.colors.device


class CornerColors(object):
    """Three lit colours per face, one per corner, for the rasterizer: a float32 tensor [B,F,3,3] indexed (batch, face,
    corner, rgb), F the rasterizer's face count (a fill_back copy carries its own nine numbers in its own corner order).
    Accepted as `textures` by rasterize, rasterize_rgbad and Rasterize.__call__; gradients reach the tensor."""

    def __init__(self, colors):
        if not torch.is_tensor(colors):
            raise ValueError('CornerColors: a tensor [batch size, num of faces, 3, 3] expected')
        if colors.dtype != torch.float32 or colors.dim() != 4 or tuple(colors.shape[2:]) != (3, 3) or colors.shape[1] < 1:
            raise ValueError('CornerColors: colors must be float32 [batch size, num of faces, 3, 3], got %s %s'
                             % (colors.dtype, tuple(colors.shape)))
        self.colors = colors

    @property
    def device(self):
        return self.colors.device


# ---------------------------------------------------------------------------------------------------------------------
# the vertex -> (face, corner) table

_ADJ_ATTR = '_nr_vertex_adjacency'  # stashed on the index tensor OBJECT (see _util._INDEX_ATTR for why not on data_ptr alone)


def build_adjacency(faces_idx, num_vertices):
    """Host arrays (offsets [T,Nv+1], entries [T,3Nf]) int32 for indices [T,Nf,3]: the entries of vertex v,
    entries[t, offsets[t,v]:offsets[t,v+1]], are its (face, corner) pairs 3f + k in ascending order."""
    idx = np.asarray(faces_idx, dtype=np.int64)
    T, Nf = idx.shape[:2]
    flat = idx.reshape(T, 3 * Nf)
    if flat.size and (flat.min() < 0 or flat.max() >= num_vertices):
        raise IndexError('a vertex index outside [0, %d)' % num_vertices)
    entries = np.argsort(flat, axis=1, kind='stable').astype(np.int32)
    offsets = np.zeros((T, num_vertices + 1), np.int32)
    for t in range(T):
        offsets[t, 1:] = np.cumsum(np.bincount(flat[t], minlength=num_vertices))
    return offsets, entries


def _adjacency(faces, num_vertices):
    """-> (indices int32 [T,Nf,3], offsets, entries, per_batch) on faces' device, cached on the index tensor (and for a view
    on the tensor it is a view of) under its identity: data_ptr, shape, strides, version counter and the vertex count."""
    def build():
        host = faces.detach().cpu().numpy()
        if host.ndim == 2:
            host = host[None]
        if host.shape[0] > 1 and (host == host[0:1]).all():
            host = host[0:1]  # one topology for the whole batch
        offsets, entries = build_adjacency(host, num_vertices)
        dev = faces.device
        return (torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(dev), torch.from_numpy(offsets).to(dev),
                torch.from_numpy(entries).to(dev), host.shape[0] > 1)

    return _util.cached_on_index(faces, _ADJ_ATTR, (int(num_vertices),), build,
                           'the vertex adjacency table of this index tensor is not built yet, and building it reads the '
                           'indices on the host: call vertex_shade / Renderer.render once with it before the capture')


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _light_vec(value, ref, batch_size):
    v = as_tensor_like(value, ref, ref.dtype)
    return v[None, :].expand(batch_size, 3) if v.dim() == 1 else v


def vertex_shade_torch(vertices, faces, colors, intensity_ambient=0.5, intensity_directional=0.5, color_ambient=(1, 1, 1),
                       color_directional=(1, 1, 1), direction=(0, 1, 0), fill_back=True, smooth=False):
    """corner colours [B,F,3,3] in plain torch (any device, any float dtype; light colours and direction [3] or [B,3])."""
    B, Nv = vertices.shape[:2]
    idx = faces.long()
    if idx.dim() == 2:
        idx = idx[None].expand(B, -1, -1)
    Nf = idx.shape[1]
    if colors.dim() == 2:
        colors = colors[None]
    colors = colors.expand(B, Nv, 3)
    batch = torch.arange(B, device=vertices.device)[:, None, None]
    fv = vertices[batch, idx]  # [B,Nf,3,3]
    cf = colors[batch, idx]
    ca, cd, direction = (_light_vec(x, vertices, B) for x in (color_ambient, color_directional, direction))
    n = torch.cross(fv[:, :, 0] - fv[:, :, 1], fv[:, :, 2] - fv[:, :, 1], dim=2)  # lighting.py:36-39
    amb = intensity_ambient * ca if intensity_ambient != 0 else torch.zeros_like(ca)

    def lights(normal_sum):  # [B,N,3] -> the light seen by the faces and by their reversed copies, [B,N,3] each
        if intensity_directional == 0:
            a = amb[:, None, :].expand_as(normal_sum)
            return a, a
        nh = normal_sum / (torch.sqrt((normal_sum * normal_sum).sum(2, keepdim=True)) + 1e-5)
        dot = (nh * direction[:, None, :]).sum(2)
        front = amb[:, None, :] + intensity_directional * (cd[:, None, :] * torch.relu(dot)[:, :, None])
        back = amb[:, None, :] + intensity_directional * (cd[:, None, :] * torch.relu(-dot)[:, :, None])
        return front, back

    if smooth:
        m = torch.zeros((B, Nv, 3), dtype=vertices.dtype, device=vertices.device)
        for k in range(3):
            m = m.scatter_add(1, idx[:, :, k, None].expand(B, Nf, 3), n)
        lf, lb = lights(m)
        lf, lb = lf[batch, idx], lb[batch, idx]  # [B,Nf,3,3]
    else:
        lf, lb = lights(n)
        lf, lb = lf[:, :, None, :], lb[:, :, None, :]
    front = cf * lf
    if not fill_back:
        return front
    return torch.cat((front, torch.flip(cf * lb, dims=[2])), dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

def _light_struct(ia, idir, ca, cd, direction):
    light = _lib.Light()
    light.intensity_ambient, light.intensity_directional = float(ia), float(idir)
    for name, src in (('color_ambient', ca), ('color_directional', cd), ('direction', direction)):
        v = np.asarray(src, dtype=np.float32)
        for k in range(3):
            getattr(light, name)[k] = float(v[k])
    return light


@_util.once_differentiable
class _VertexShade(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], colors [Nv,3] | [Bc,Nv,3], setup) -> corner colours [B,F,3,3];
    setup = (indices, offsets, entries, idx_per_batch, nr_light, fill_back, smooth)."""

    @staticmethod
    def forward(ctx, vertices, colors, setup):
        idx, off, ent, per_batch, light, fill_back, smooth = setup
        v = _lib.dense(vertices.detach())
        c = _lib.dense(colors.detach())
        dev = v.device
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        Bc = 1 if c.dim() == 2 else int(c.shape[0])
        F = 2 * Nf if fill_back else Nf
        out = torch.empty((B, F, 3, 3), dtype=torch.float32, device=dev)
        _lib.launch('nr_vertex_shade_forward', dev, v.data_ptr(), idx.data_ptr(), c.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    out.data_ptr(), B, Nv, Nf, Bc, int(per_batch), int(fill_back), int(smooth), light,
                    workspace_bytes=_lib.workspace_bytes('nr_vertex_shade_workspace_bytes', B, Nv) if smooth else 0)
        ctx.save_for_backward(v, c)
        ctx.setup = setup
        ctx.colors_dim = colors.dim()
        return out

    @staticmethod
    def backward(ctx, grad_corner):
        v, c = ctx.saved_tensors
        idx, off, ent, per_batch, light, fill_back, smooth = ctx.setup
        need_v, need_c = ctx.needs_input_grad[:2]
        if not (need_v or need_c):
            return None, None, None
        dev = v.device
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        Bc = 1 if c.dim() == 2 else int(c.shape[0])
        g = _lib.dense(grad_corner)
        grad_v = torch.empty_like(v) if need_v else None
        grad_c = torch.empty_like(c) if need_c else None
        _lib.launch('nr_vertex_shade_backward', dev, v.data_ptr(), idx.data_ptr(), c.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    g.data_ptr(), _lib.ptr(grad_c), _lib.ptr(grad_v), B, Nv, Nf, Bc, int(per_batch), int(fill_back), int(smooth),
                    light, workspace_bytes=(_lib.workspace_bytes('nr_vertex_shade_workspace_bytes', B, Nv)
                                            if (smooth and need_v) else 0))
        return grad_v, grad_c, None


def _host_light(ia, idir, ca, cd, direction):
    """The light as host numbers (nr_light), or None when a parameter is a tensor / per-image array."""
    if not (_is_number(ia) and _is_number(idir)):
        return None
    vecs = [_vec3(x) for x in (ca, cd, direction)]
    if any(x is None for x in vecs):
        return None
    return _light_struct(ia, idir, *vecs)


def check_vertex_shade(vertices, faces, colors):
    """Shape / dtype / device checks shared by both implementations.  Returns (B, Nv, Nf, Bc)."""
    if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3 and vertices.is_floating_point()):
        raise ValueError('vertex_shade: vertices must be a float tensor [batch size, num of vertices, 3]')
    B, Nv = int(vertices.shape[0]), int(vertices.shape[1])
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dim() in (2, 3) and faces.shape[-1] == 3
            and faces.shape[-2] >= 1):
        raise ValueError('vertex_shade: faces must be an integer tensor [num of faces, 3] or [batch size, num of faces, 3]')
    if faces.dim() == 3 and faces.shape[0] != B:
        raise ValueError('vertex_shade: faces have batch size %d, vertices %d' % (faces.shape[0], B))
    if isinstance(colors, VertexColors):
        colors = colors.colors
    if not (torch.is_tensor(colors) and colors.dim() in (2, 3) and colors.shape[-1] == 3):
        raise ValueError('vertex_shade: colors must be a tensor [num of vertices, 3] or [batch size, num of vertices, 3]')
    if colors.dtype != vertices.dtype:
        raise ValueError('vertex_shade: colors are %s, vertices %s' % (colors.dtype, vertices.dtype))
    if colors.shape[-2] != Nv:
        raise ValueError('vertex_shade: %d vertex colours for %d vertices' % (colors.shape[-2], Nv))
    Bc = 1 if colors.dim() == 2 else int(colors.shape[0])
    if Bc not in (1, B):
        raise ValueError('vertex_shade: batched colours must have the batch size of the vertices (%d), got %d' % (B, Bc))
    if colors.device != vertices.device or faces.device != vertices.device:
        raise ValueError('vertex_shade: vertices, faces and colors must be on one device (%s, %s, %s)'
                         % (vertices.device, faces.device, colors.device))
    return B, Nv, int(faces.shape[-2]), Bc


def vertex_shade(vertices, faces, colors, intensity_ambient=0.5, intensity_directional=0.5, color_ambient=(1, 1, 1),
                 color_directional=(1, 1, 1), direction=(0, 1, 0), fill_back=True, smooth=False, implementation=None):
    """CornerColors [B,F,3,3] (F = Nf, or 2 Nf with fill_back) from world-space vertices [B,Nv,3], faces [Nf,3] | [B,Nf,3],
    vertex colours [Nv,3] | [B,Nv,3] (or a VertexColors) and lighting()'s light parameters.  smooth = False: the light of a
    face is lighting()'s; smooth = True: the light is computed at the vertices from the area-weighted sum of the normals of
    their faces.  Differentiable in vertices and colors.  `implementation`: None picks the HIP kernels when the call fits
    them (see the module docstring), 'torch' / 'hip' force one ('hip' raises when the call does not fit)."""
    if isinstance(colors, VertexColors):
        colors = colors.colors
    B, Nv, Nf, Bc = check_vertex_shade(vertices, faces, colors)
    _util.check_implementation('vertex_shade', implementation)
    light = _host_light(intensity_ambient, intensity_directional, color_ambient, color_directional, direction)
    fits = vertices.is_cuda and vertices.dtype == torch.float32 and light is not None and B <= 65535
    if not _util.takes_hip('vertex_shade', implementation, fits, 'the HIP kernels take float32 CUDA tensors and host light '
                           'parameters'):
        if vertices.dtype != torch.float32:
            raise ValueError('vertex_shade: float32 tensors expected (vertex_shade_torch takes other float types)')
        return CornerColors(vertex_shade_torch(vertices, faces, colors, intensity_ambient, intensity_directional,
                                               color_ambient, color_directional, direction, fill_back, smooth))
    _util.check_face_indices(faces, Nv, vertices.device)
    idx, off, ent, per_batch = _adjacency(faces, Nv)
    setup = (idx, off, ent, per_batch, light, bool(fill_back), bool(smooth))
    return CornerColors(_VertexShade.apply(vertices, colors, setup))


def vertex_light(vertices, faces, intensity_ambient=0.5, intensity_directional=0.5, color_ambient=(1, 1, 1),
                 color_directional=(1, 1, 1), direction=(0, 1, 0), fill_back=True, smooth=True, implementation=None):
    """The light of every face corner, a float32 tensor [B,F,3,3] (F = Nf, or 2 Nf with fill_back; the corners of a reversed
    copy in its own, flipped order): the corner colours vertex_shade gives a white mesh.  It is what the rasterizer takes as
    `face_light` next to a UVImages for smooth light (Renderer.shading = 'smooth').  Differentiable in vertices.  The HIP
    path runs nr_vertex_shade_* with one row of ones shared by the batch and asks for no colour gradient; `implementation`
    as in vertex_shade."""
    if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3 and vertices.is_floating_point()):
        raise ValueError('vertex_light: vertices must be a float tensor [batch size, num of vertices, 3]')
    ones = torch.ones((int(vertices.shape[1]), 3), dtype=vertices.dtype, device=vertices.device)
    return vertex_shade(vertices, faces, ones, intensity_ambient, intensity_directional, color_ambient, color_directional,
                        direction, fill_back, smooth, implementation).colors
