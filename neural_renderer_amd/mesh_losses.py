"""Laplacian and flatness losses on a mesh's vertices (not in the reference's library: the two shape priors of its paper,
Neural 3D Mesh Renderer, section 5).

`laplacian_loss(vertices, faces)` keeps every vertex near the centroid of its neighbours (uniform umbrella operator);
`flatness_loss(vertices, faces)` penalises the dihedral angle across every interior edge.  Both take world-space vertices
[B,Nv,3] (or [Nv,3]) and ONE topology `faces` [Nf,3] for the whole call, return one loss per image, and are
once-differentiable in the vertices.

Definitions.  N(v) is the set of distinct u != v that share a face with v (duplicate faces and repeated indices inside a
face add nothing), deg v = |N(v)|.
    delta_v = x_v - (1 / deg v) sum_{u in N(v)} x_u   (0 with deg v = 0),      laplacian loss_b = sum_v |delta_{b,v}|^2
A quad is an undirected edge {v0 < v1} that lies in exactly two faces, counted after removing the faces with a repeated
index (edges in one face or in more than two are skipped); v2 and v3 are the opposite vertices, v2 from the lower-numbered
face; the quads are ordered by (v0, v1).  Per quad
    a = x1 - x0;  b1 = x2 - x0;  b2 = x3 - x0;  c_i = b_i - ((a . b_i) / (a . a + eps)) a;  l_i = sqrt(c_i . c_i + eps)
    cos = (c1 . c2) / (l1 l2 + eps),                                            flatness loss_b = sum_quads (cos + 1)^2
which is 0 (up to eps) on a flat mesh and finite for every finite input.

On CUDA float32 tensors with B <= 65535 both run as HIP kernels in both directions (nr_laplacian_* / nr_flatness_*,
csrc/nr_mesh_losses.hip): every sum around a vertex is a gather through one of the tables below and every loss is reduced
in a fixed order, so no direction uses atomics and the results repeat bit for bit.  Everything else takes the plain-torch
implementations `laplacian_loss_torch` / `flatness_loss_torch` (any device, any float dtype), which are also the kernels'
second yardstick in the tests.

The tables are built on the host in vectorised NumPy the first time a topology is seen and cached on the index tensor, as
vertex_colors._adjacency caches its table: the build reads the indices back, so it must happen BEFORE a graph capture --
run one eager step with the same index tensor first (inside a capture an unknown topology raises)."""
import numpy as np
import torch

from . import _lib, _util

_TABLES_ATTR = '_nr_mesh_loss_tables'  # stashed on the index tensor OBJECT (see _util._INDEX_ATTR for why not on data_ptr alone)


class MeshTables(object):
    """The int32 tables of one topology, on one device:
    nbr_offsets [Nv+1], nbr [sum deg]: N(v) = nbr[nbr_offsets[v]:nbr_offsets[v+1]], ascending;
    quads [E2,4]: (v0, v1, v2, v3) ordered by (v0, v1);
    inc_offsets [Nv+1], inc [4 E2]: the (quad, slot) pairs 4 q + slot in which vertex v occurs, ascending."""

    def __init__(self, nbr_offsets, nbr, quads, inc_offsets, inc):
        self.nbr_offsets, self.nbr, self.quads, self.inc_offsets, self.inc = nbr_offsets, nbr, quads, inc_offsets, inc
        self.num_vertices = int(nbr_offsets.shape[0]) - 1
        self.num_quads = int(quads.shape[0])


def build_tables(faces_idx, num_vertices):
    """Host arrays (nbr_offsets, nbr, quads, inc_offsets, inc), all int32, for indices [Nf,3] (see MeshTables)."""
    f = np.asarray(faces_idx, dtype=np.int64).reshape(-1, 3)
    Nv = int(num_vertices)
    if f.size and (f.min() < 0 or f.max() >= Nv):
        raise IndexError('a vertex index outside [0, %d)' % Nv)
    # neighbours: the six ordered pairs of every face, without v == u, each distinct pair once; the keys v * Nv + u sort
    # by vertex, then by neighbour
    v = f[:, (0, 0, 1, 1, 2, 2)].reshape(-1)
    u = f[:, (1, 2, 0, 2, 0, 1)].reshape(-1)
    keys = np.unique((v * Nv + u)[v != u])
    nbr = (keys % Nv).astype(np.int32)
    nbr_offsets = np.zeros(Nv + 1, np.int64)
    nbr_offsets[1:] = np.cumsum(np.bincount(keys // Nv, minlength=Nv))
    # quads: the three edges of every face without a repeated index, face-major, so that a stable sort by the edge's key
    # keeps the faces of an edge in ascending order
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    g = f[ok]
    e0, e1, opp = g[:, (0, 1, 2)].reshape(-1), g[:, (1, 2, 0)].reshape(-1), g[:, (2, 0, 1)].reshape(-1)
    lo, hi = np.minimum(e0, e1), np.maximum(e0, e1)
    ekey = lo * Nv + hi
    order = np.argsort(ekey, kind='stable')
    ekey, opp = ekey[order], opp[order]
    uniq, first, count = np.unique(ekey, return_index=True, return_counts=True)
    first = first[count == 2]
    uniq = uniq[count == 2]
    quads = np.stack((uniq // Nv, uniq % Nv, opp[first], opp[first + 1]), axis=1).astype(np.int32).reshape(-1, 4)
    # vertex -> (quad, slot): a stable sort of the flattened quads lists 4 q + slot ascending within a vertex
    flat = quads.reshape(-1).astype(np.int64)
    inc = np.argsort(flat, kind='stable').astype(np.int32)
    inc_offsets = np.zeros(Nv + 1, np.int64)
    inc_offsets[1:] = np.cumsum(np.bincount(flat, minlength=Nv))
    return nbr_offsets.astype(np.int32), nbr, np.ascontiguousarray(quads), inc_offsets.astype(np.int32), inc


def _tables(faces, num_vertices):
    """-> MeshTables on faces' device, cached on the index tensor (and for a view on the tensor it is a view of) under its
    identity: data_ptr, shape, strides, version counter and the vertex count."""
    def build():
        host = faces.detach().cpu().numpy()
        if host.ndim == 3:
            if not (host == host[0:1]).all():
                raise ValueError('mesh losses: the faces of all images must be equal (one topology per call)')
            host = host[0]
        return MeshTables(*(torch.from_numpy(a).to(faces.device) for a in build_tables(host, num_vertices)))

    return _util.cached_on_index(faces, _TABLES_ATTR, (int(num_vertices),), build,
                                 'the mesh loss tables of this index tensor are not built yet, and building them reads the '
                                 'indices on the host: call laplacian_loss / flatness_loss once with it before the capture')


# ---------------------------------------------------------------------------------------------------------------------
# checks shared by both implementations

def _check(name, vertices, faces):
    """-> (vertices [B,Nv,3], squeeze): shape / dtype / device checks."""
    if not (torch.is_tensor(vertices) and vertices.is_floating_point() and vertices.dim() in (2, 3) and vertices.shape[-1] == 3
            and vertices.shape[-2] >= 1 and vertices.shape[0] >= 1):
        raise ValueError('%s: vertices must be a float tensor [num of vertices, 3] or [batch size, num of vertices, 3]' % name)
    squeeze = vertices.dim() == 2
    if squeeze:
        vertices = vertices[None]
    B = int(vertices.shape[0])
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dtype != torch.bool and faces.dim() in (2, 3)
            and faces.shape[-1] == 3 and faces.shape[-2] >= 1):
        raise ValueError('%s: faces must be an integer tensor [num of faces, 3] or [batch size, num of faces, 3]' % name)
    if faces.dim() == 3 and faces.shape[0] != B:
        raise ValueError('%s: faces have batch size %d, vertices %d' % (name, faces.shape[0], B))
    if faces.device != vertices.device:
        raise ValueError('%s: vertices and faces must be on one device (%s, %s)' % (name, vertices.device, faces.device))
    return vertices, squeeze


def _prepare(name, vertices, faces, implementation):
    """-> (vertices [B,Nv,3], squeeze, tables, use_hip)"""
    vertices, squeeze = _check(name, vertices, faces)
    B, Nv = int(vertices.shape[0]), int(vertices.shape[1])
    fits = vertices.is_cuda and vertices.dtype == torch.float32 and B <= 65535
    hip = _util.takes_hip(name, implementation, fits, 'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at '
                          'most')
    _util.check_face_indices(faces, Nv, vertices.device)
    return vertices, squeeze, _tables(faces, Nv), hip


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _laplacian_torch(x, t):
    B, Nv = x.shape[:2]
    off = t.nbr_offsets.long()
    deg = off[1:] - off[:-1]
    owner = torch.repeat_interleave(torch.arange(Nv, device=x.device), deg)
    s = torch.zeros_like(x).index_add(1, owner, x[:, t.nbr.long()])
    mean = s / deg.clamp(min=1).to(x.dtype)[None, :, None]
    delta = torch.where((deg > 0)[None, :, None], x - mean, torch.zeros_like(x))
    return (delta * delta).sum((1, 2))


def _flatness_torch(x, t, eps):
    q = t.quads.long()
    x0, x1, x2, x3 = (x[:, q[:, k]] for k in range(4))
    a, b1, b2 = x1 - x0, x2 - x0, x3 - x0
    A = (a * a).sum(2) + eps
    c1 = b1 - ((a * b1).sum(2) / A)[:, :, None] * a
    c2 = b2 - ((a * b2).sum(2) / A)[:, :, None] * a
    l1 = torch.sqrt((c1 * c1).sum(2) + eps)
    l2 = torch.sqrt((c2 * c2).sum(2) + eps)
    cos = (c1 * c2).sum(2) / (l1 * l2 + eps)
    return ((cos + 1) ** 2).sum(1)


def laplacian_loss_torch(vertices, faces):
    """laplacian_loss in plain torch (any device, any float dtype), differentiable by torch's autograd."""
    vertices, squeeze = _check('laplacian_loss_torch', vertices, faces)
    _util.check_face_indices(faces, int(vertices.shape[1]), vertices.device)
    loss = _laplacian_torch(vertices, _tables(faces, int(vertices.shape[1])))
    return loss[0] if squeeze else loss


def flatness_loss_torch(vertices, faces, eps=1e-6):
    """flatness_loss in plain torch (any device, any float dtype), differentiable by torch's autograd."""
    vertices, squeeze = _check('flatness_loss_torch', vertices, faces)
    _util.check_face_indices(faces, int(vertices.shape[1]), vertices.device)
    loss = _flatness_torch(vertices, _tables(faces, int(vertices.shape[1])), float(eps))
    return loss[0] if squeeze else loss


# ---------------------------------------------------------------------------------------------------------------------
# HIP

class _LaplacianLoss(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], tables) -> loss [B]; delta [B,Nv,3] is kept for the backward when one can follow."""

    @staticmethod
    def forward(ctx, vertices, t):
        v = _lib.dense(vertices.detach())
        dev = v.device
        B, Nv = v.shape[:2]
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        delta = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        _lib.launch('nr_laplacian_forward', dev, v.data_ptr(), t.nbr_offsets.data_ptr(), _lib.ptr(t.nbr), _lib.ptr(delta),
                    loss.data_ptr(), B, Nv, int(t.nbr.shape[0]),
                    workspace_bytes=_lib.workspace_bytes('nr_mesh_loss_workspace_bytes', B, Nv))
        if delta is not None:
            ctx.save_for_backward(delta)
        ctx.tables = t
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None
        delta, = ctx.saved_tensors
        t = ctx.tables
        dev = delta.device
        B, Nv = delta.shape[:2]
        g = _lib.dense(grad_loss)
        grad_v = torch.empty_like(delta)
        _lib.launch('nr_laplacian_backward', dev, delta.data_ptr(), t.nbr_offsets.data_ptr(), _lib.ptr(t.nbr), g.data_ptr(),
                    grad_v.data_ptr(), B, Nv, int(t.nbr.shape[0]))
        return grad_v, None


class _FlatnessLoss(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], tables, eps) -> loss [B]"""

    @staticmethod
    def forward(ctx, vertices, t, eps):
        v = _lib.dense(vertices.detach())
        dev = v.device
        B, Nv = v.shape[:2]
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.launch('nr_flatness_forward', dev, v.data_ptr(), _lib.ptr(t.quads) if t.num_quads else None, loss.data_ptr(), B, Nv,
                    t.num_quads, eps, workspace_bytes=_lib.workspace_bytes('nr_mesh_loss_workspace_bytes', B, t.num_quads))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(v)
        ctx.tables, ctx.eps = t, eps
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        v, = ctx.saved_tensors
        t = ctx.tables
        dev = v.device
        B, Nv = v.shape[:2]
        g = _lib.dense(grad_loss)
        grad_v = torch.empty_like(v)
        some = t.num_quads > 0
        _lib.launch('nr_flatness_backward', dev, v.data_ptr(), _lib.ptr(t.quads) if some else None,
                    _lib.ptr(t.inc_offsets) if some else None, _lib.ptr(t.inc) if some else None, g.data_ptr(),
                    grad_v.data_ptr(), B, Nv, t.num_quads, ctx.eps)
        return grad_v, None, None


def laplacian_loss(vertices, faces, implementation=None):
    """sum_v |x_v - centroid of N(v)|^2 per image: [B] from vertices [B,Nv,3], a 0-dim tensor from [Nv,3]; faces [Nf,3], or
    [B,Nf,3] whose images are all equal.  Differentiable (once) in vertices.  `implementation`: None picks the HIP kernels
    when the call fits them (see the module docstring), 'torch' / 'hip' force one ('hip' raises when the call does not fit)."""
    vertices, squeeze, t, hip = _prepare('laplacian_loss', vertices, faces, implementation)
    loss = _LaplacianLoss.apply(vertices, t) if hip else _laplacian_torch(vertices, t)
    return loss[0] if squeeze else loss


def flatness_loss(vertices, faces, eps=1e-6, implementation=None):
    """sum over the interior edges of (cos of the angle between the two faces' in-plane directions + 1)^2 per image: [B]
    from vertices [B,Nv,3], a 0-dim tensor from [Nv,3]; faces as in laplacian_loss.  0 (up to eps) on a flat mesh; exactly 0
    with zero gradients when no edge lies in exactly two faces.  Differentiable (once) in vertices; `implementation` as in
    laplacian_loss."""
    vertices, squeeze, t, hip = _prepare('flatness_loss', vertices, faces, implementation)
    loss = _FlatnessLoss.apply(vertices, t, float(eps)) if hip else _flatness_torch(vertices, t, float(eps))
    return loss[0] if squeeze else loss
