"""Vertex, face and corner normals, and the camera rotation of a Renderer (not in the reference).

The normals are the ones the light already uses (vertex_colors.py, lighting.py), as tensors of their own:

    N_f = cross(v0 - v1, v2 - v1)                      the unnormalised normal of face f (lighting.py:36-39)
    n_f = N_f / (|N_f| + 1e-5)                          face_normals   [B,Nf,3]
    m_v = the sum of N_f over the faces around v       (area-weighted; once per corner of f that is v)
    n_v = m_v / (|m_v| + 1e-5)                          vertex_normals [B,Nv,3]

A vertex without a face, a zero normal sum and a zero-area face give exactly 0.  `corner_normals` lays them out as the
rasterizer's CornerColors [B,F,3,3]: corner k of face f carries n_f (flat) or the normal of its vertex (smooth), and the
reversed copy of a face (fill_back) the negated normal in its own flipped corner order, corner[Nf + f][k] = -corner[f][2 - k].
`Renderer.render_normals` rasterizes them into a normal map.

On CUDA float32 tensors the three functions run as HIP kernels in both directions (include/nr_hip.h: nr_vertex_normals_*,
nr_face_normals_*, nr_corner_normals_*), in the float32 operation order of vertex shading: the normals equal the ones inside
`vertex_light` bit for bit.  Every sum around a vertex or a face is a gather through the vertex -> (face, corner) table of
vertex_colors.py, so neither direction uses atomics and the results repeat bit for bit; the table is built on the host the
first time an index tensor is seen (inside a graph capture an unseen index tensor raises: run one eager step first).  CPU
tensors, other float types and implementation='torch' take the plain-torch functions `*_torch` with the same formulas.
"""
import torch

from . import _lib, _util
from ._util import normalize
from .cross import cross
from .vertex_colors import CornerColors, _adjacency

NORM_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _normalize(v):
    """v / (|v| + eps) on the last axis, written so that autograd gives g / eps, not NaN, where |v| = 0."""
    d = (v * v).sum(-1, keepdim=True)
    pos = d > 0
    r = torch.where(pos, torch.sqrt(torch.where(pos, d, torch.ones_like(d))), torch.zeros_like(d))
    return v / (r + NORM_EPS)


def _index(vertices, faces):
    B = vertices.shape[0]
    idx = faces.long()
    if idx.dim() == 2:
        idx = idx[None].expand(B, -1, -1)
    return idx


def _raw_face_normals(vertices, idx):
    batch = torch.arange(vertices.shape[0], device=vertices.device)[:, None, None]
    fv = vertices[batch, idx]  # [B,Nf,3,3]
    return torch.cross(fv[:, :, 0] - fv[:, :, 1], fv[:, :, 2] - fv[:, :, 1], dim=2)


def face_normals_torch(vertices, faces):
    """n_f [B,Nf,3] in plain torch (any device, any float dtype)."""
    return _normalize(_raw_face_normals(vertices, _index(vertices, faces)))


def vertex_normals_torch(vertices, faces):
    """n_v [B,Nv,3] in plain torch (any device, any float dtype); on the CPU the normal sums run in ascending (face, corner)
    order like the kernels', on a GPU in the arrival order of scatter_add's atomics."""
    B, Nv = vertices.shape[:2]
    idx = _index(vertices, faces)
    Nf = idx.shape[1]
    n = _raw_face_normals(vertices, idx)
    m = torch.zeros((B, Nv, 3), dtype=vertices.dtype, device=vertices.device)
    m = m.scatter_add(1, idx.reshape(B, 3 * Nf, 1).expand(B, 3 * Nf, 3), n[:, :, None, :].expand(B, Nf, 3, 3).reshape(B, 3 * Nf, 3))
    return _normalize(m)


def corner_normals_torch(vertices, faces, smooth=False, fill_back=True):
    """corner normals [B,F,3,3] in plain torch (any device, any float dtype)."""
    idx = _index(vertices, faces)
    if smooth:
        batch = torch.arange(vertices.shape[0], device=vertices.device)[:, None, None]
        front = vertex_normals_torch(vertices, faces)[batch, idx]
    else:
        front = face_normals_torch(vertices, faces)[:, :, None, :].expand(-1, -1, 3, -1)
    if not fill_back:
        return front.contiguous()
    return torch.cat((front, -torch.flip(front, dims=[2])), dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

@_util.once_differentiable
class _VertexNormals(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], setup) -> n_v [B,Nv,3]; setup = (indices, offsets, entries, idx_per_batch)."""

    @staticmethod
    def forward(ctx, vertices, setup):
        idx, off, ent, per_batch = setup
        v = _lib.dense(vertices.detach())
        B, Nv = v.shape[:2]
        out = torch.empty_like(v)
        _lib.launch('nr_vertex_normals_forward', v.device, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    out.data_ptr(), B, Nv, idx.shape[1], int(per_batch))
        ctx.save_for_backward(v)
        ctx.setup = setup
        return out

    @staticmethod
    def backward(ctx, grad_normals):
        v, = ctx.saved_tensors
        idx, off, ent, per_batch = ctx.setup
        B, Nv = v.shape[:2]
        g = _lib.dense(grad_normals)
        grad_v = torch.empty_like(v)
        _lib.launch('nr_vertex_normals_backward', v.device, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    g.data_ptr(), grad_v.data_ptr(), B, Nv, idx.shape[1], int(per_batch),
                    workspace_bytes=_lib.workspace_bytes('nr_normals_workspace_bytes', B, Nv, idx.shape[1]))
        return grad_v, None


@_util.once_differentiable
class _FaceNormals(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], setup) -> n_f [B,Nf,3]; setup as in _VertexNormals."""

    @staticmethod
    def forward(ctx, vertices, setup):
        idx, off, ent, per_batch = setup
        v = _lib.dense(vertices.detach())
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        out = torch.empty((B, Nf, 3), dtype=torch.float32, device=v.device)
        _lib.launch('nr_face_normals_forward', v.device, v.data_ptr(), idx.data_ptr(), out.data_ptr(), B, Nv, Nf,
                    int(per_batch))
        ctx.save_for_backward(v)
        ctx.setup = setup
        return out

    @staticmethod
    def backward(ctx, grad_normals):
        v, = ctx.saved_tensors
        idx, off, ent, per_batch = ctx.setup
        B, Nv = v.shape[:2]
        g = _lib.dense(grad_normals)
        grad_v = torch.empty_like(v)
        _lib.launch('nr_face_normals_backward', v.device, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    g.data_ptr(), grad_v.data_ptr(), B, Nv, idx.shape[1], int(per_batch),
                    workspace_bytes=_lib.workspace_bytes('nr_normals_workspace_bytes', B, Nv, idx.shape[1]))
        return grad_v, None


@_util.once_differentiable
class _CornerNormals(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], setup) -> corner normals [B,F,3,3];
    setup = (indices, offsets, entries, idx_per_batch, fill_back, smooth)."""

    @staticmethod
    def forward(ctx, vertices, setup):
        idx, off, ent, per_batch, fill_back, smooth = setup
        v = _lib.dense(vertices.detach())
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        out = torch.empty((B, 2 * Nf if fill_back else Nf, 3, 3), dtype=torch.float32, device=v.device)
        _lib.launch('nr_corner_normals_forward', v.device, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    out.data_ptr(), B, Nv, Nf, int(per_batch), int(fill_back), int(smooth),
                    workspace_bytes=_lib.workspace_bytes('nr_normals_workspace_bytes', B, Nv, Nf) if smooth else 0)
        ctx.save_for_backward(v)
        ctx.setup = setup
        return out

    @staticmethod
    def backward(ctx, grad_corner):
        v, = ctx.saved_tensors
        idx, off, ent, per_batch, fill_back, smooth = ctx.setup
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        g = _lib.dense(grad_corner)
        grad_v = torch.empty_like(v)
        _lib.launch('nr_corner_normals_backward', v.device, v.data_ptr(), idx.data_ptr(), off.data_ptr(), ent.data_ptr(),
                    g.data_ptr(), grad_v.data_ptr(), B, Nv, Nf, int(per_batch), int(fill_back), int(smooth),
                    workspace_bytes=_lib.workspace_bytes('nr_normals_workspace_bytes', B, Nv, Nf))
        return grad_v, None


# ---------------------------------------------------------------------------------------------------------------------
# the public functions

def _check(name, vertices, faces, implementation):
    """Shape / dtype / device checks shared by both implementations -> (vertices [B,Nv,3], unbatched, takes the HIP path)."""
    if not (torch.is_tensor(vertices) and vertices.dim() in (2, 3) and vertices.shape[-1] == 3 and vertices.shape[-2] >= 1
            and vertices.is_floating_point()):
        raise ValueError('%s: vertices must be a float tensor [batch size, num of vertices, 3] or [num of vertices, 3]' % name)
    unbatched = vertices.dim() == 2
    if unbatched:
        vertices = vertices[None]
    B = int(vertices.shape[0])
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dtype != torch.bool and faces.dim() in (2, 3)
            and faces.shape[-1] == 3 and faces.shape[-2] >= 1):
        raise ValueError('%s: faces must be an integer tensor [num of faces, 3] or [batch size, num of faces, 3]' % name)
    if faces.dim() == 3 and faces.shape[0] != B:
        raise ValueError('%s: faces have batch size %d, vertices %d' % (name, faces.shape[0], B))
    if faces.device != vertices.device:
        raise ValueError('%s: vertices and faces must be on one device (%s, %s)' % (name, vertices.device, faces.device))
    fits = vertices.is_cuda and vertices.dtype == torch.float32 and 1 <= B <= 65535
    return vertices, unbatched, _util.takes_hip(name, implementation, fits, 'the HIP kernels take float32 CUDA tensors with a '
                                                'batch size of at most 65535')


def _setup(vertices, faces):
    _util.check_face_indices(faces, vertices.shape[1], vertices.device)
    return _adjacency(faces, vertices.shape[1])


def vertex_normals(vertices, faces, implementation=None):
    """n_v [B,Nv,3] (or [Nv,3] for vertices [Nv,3]): the area-weighted vertex normals of world-space vertices and faces
    [Nf,3] | [B,Nf,3] (module docstring).  Differentiable in vertices.  `implementation`: None picks the HIP kernels for
    float32 CUDA tensors, 'torch' / 'hip' force one ('hip' raises when the call does not fit)."""
    v, unbatched, hip = _check('vertex_normals', vertices, faces, implementation)
    out = _VertexNormals.apply(v, _setup(v, faces)) if hip else vertex_normals_torch(v, faces)
    return out[0] if unbatched else out


def face_normals(vertices, faces, implementation=None):
    """n_f [B,Nf,3] (or [Nf,3] for vertices [Nv,3]): the face normals, lighting()'s sign.  Otherwise as vertex_normals."""
    v, unbatched, hip = _check('face_normals', vertices, faces, implementation)
    out = _FaceNormals.apply(v, _setup(v, faces)) if hip else face_normals_torch(v, faces)
    return out[0] if unbatched else out


def corner_normals(vertices, faces, smooth=False, fill_back=True, implementation=None):
    """CornerColors [B,F,3,3] (F = Nf, or 2 Nf with fill_back) holding a normal per face corner, for the rasterizer: the
    face's (smooth = False) or its vertex's (smooth = True); the reversed copies carry the negated normals in their own
    flipped corner order.  The values are signed -- the rasterizer interpolates CornerColors without a clamp.  Vertices
    [B,Nv,3]; otherwise as vertex_normals."""
    if torch.is_tensor(vertices) and vertices.dim() != 3:
        raise ValueError('corner_normals: vertices must be a float tensor [batch size, num of vertices, 3]')
    v, _, hip = _check('corner_normals', vertices, faces, implementation)
    if hip:
        return CornerColors(_CornerNormals.apply(v, _setup(v, faces) + (bool(fill_back), bool(smooth))))
    if v.dtype != torch.float32:
        raise ValueError('corner_normals: float32 tensors expected (corner_normals_torch takes other float types)')
    return CornerColors(corner_normals_torch(v, faces, smooth, fill_back))


# ---------------------------------------------------------------------------------------------------------------------
# the camera's rotation

def camera_rotation(renderer, batch_size, like):
    """The rotation [B,3,3] of the renderer's camera, world -> camera, in `like`'s dtype and on its device: the rows x, y, z
    that look_at (look_at.py:22-24) builds from `eye`, or look (look.py) from `camera_direction`, with up = (0, 1, 0); in
    'projection' mode `renderer.R`.  look_at(v, eye) = (v - eye) @ R^T.  Plain torch: a learnable eye or R gets its
    gradient."""
    from .projection import _param
    mode = renderer.camera_mode
    if mode == 'projection':
        if renderer.R is None:
            raise ValueError("camera_mode 'projection' needs Renderer.R")
        return _param(renderer.R, like, batch_size, (3, 3))
    if mode not in ('look_at', 'look'):
        raise ValueError("camera_rotation: camera_mode must be 'look_at', 'look' or 'projection', got %r" % (mode,))
    up = _util.as_tensor_like([0, 1, 0], like, like.dtype)[None, :]
    if mode == 'look_at':
        eye = _util.as_tensor_like(renderer.eye, like, like.dtype)
        if eye.dim() == 1:
            eye = eye[None, :]
        z_axis = normalize(torch.zeros_like(eye) - eye)  # at = (0, 0, 0)
    else:
        direction = _util.as_tensor_like(renderer.camera_direction, like, like.dtype)
        if direction.dim() == 1:
            direction = direction[None, :]
        z_axis = normalize(direction)
    x_axis = normalize(cross(up.expand_as(z_axis), z_axis))
    y_axis = normalize(cross(z_axis, x_axis))
    r = torch.stack((x_axis, y_axis, z_axis), dim=1)
    return r.expand(batch_size, 3, 3) if r.shape[0] != batch_size else r
