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
run one eager step with the same index tensor first (inside a capture an unknown topology raises).

`edge_length_loss(vertices, faces, target)` and `cotangent_laplacian_loss(vertices, faces, eps)`, the priors of a 3-D fit --
every edge near its rest length; the cotangent-weighted Laplacian, which penalises bending and not an irregular triangulation,
with its weights held constant in the gradient --, and `mesh_edges` / `edge_lengths` are defined in the second half of this
file, with the same shapes, batching, dispatch and discipline (nr_edge_length_* / nr_cot_*)."""
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

@_util.once_differentiable
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


@_util.once_differentiable
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


# ---------------------------------------------------------------------------------------------------------------------
# edge length and cotangent Laplacian (DESIGN "Mesh losses: edge length and cotangent Laplacian")
#
# Edges: the distinct undirected pairs {v0 < v1} that share a face -- exactly the pairs of the neighbour CSR above, so an edge
# in one, two or three faces or in a duplicated face counts once and a repeated index inside a face adds nothing --, ordered by
# (v0, v1); E their number.
#     l_e = sqrt(|x_v1 - x_v0|^2),    edge length loss_b = sum_e (l_e - t_e)^2,    d/dx_v1 = 2 g_b (l_e - t_e) (x_v1 - x_v0) / l_e
# with the gradient exactly 0 where l_e = 0; with the number 0 for a target the square root is skipped: sum_e |e|^2.
# Cotangents: for a face (i, j, k) without a repeated index  cot_k = (a . b) / sqrt(|a x b|^2 + eps),  a = x_i - x_k,
# b = x_j - x_k, likewise at the other two corners (finite for every finite input; a face with a repeated index has three zeros;
# every face counts, a duplicated one twice).  With the corner indices mod 3 inside a face
#     H_v = 1/2 sum_{(f, c) with f_c = v} [cot_{c+2} (x_{c+1} - x_v) + cot_{c+1} (x_{c+2} - x_v)],    loss_b = sum_v |H_{b,v}|^2
# -- the corner opposite an edge weights that edge: the usual 1/2 (cot alpha + cot beta), summed face by face.  THE WEIGHTS ARE
# CONSTANTS OF THE STEP: the gradient does not differentiate cot (the common convention of cotangent smoothing, which keeps the
# backward linear), and the operator being symmetric, d loss / d x_v = 2 g_b L(H)_v: the same gather applied to H.

_EDGE_ATTR = '_nr_mesh_edge_tables'


class EdgeTables(object):
    """The int32 edge tables of one topology, on one device: edges [E,2] ordered by (v0, v1), v0 < v1; nbr_edge [sum deg]: the
    edge number of every entry of mesh.nbr; mesh: the MeshTables they were built from."""

    def __init__(self, edges, nbr_edge, mesh):
        self.edges, self.nbr_edge, self.mesh = edges, nbr_edge, mesh
        self.num_edges = int(edges.shape[0])


def build_edge_tables(nbr_offsets, nbr):
    """Host arrays (edges [E,2], nbr_edge [sum deg]), int32, from the neighbour CSR of build_tables (see EdgeTables)."""
    off = np.asarray(nbr_offsets, dtype=np.int64)
    u = np.asarray(nbr, dtype=np.int64)
    Nv = off.shape[0] - 1
    v = np.repeat(np.arange(Nv, dtype=np.int64), off[1:] - off[:-1])
    # the CSR lists the keys v * Nv + u ascending: its entries with v < u are the edges in (v0, v1) order, and an entry's edge
    # is the rank of its own key with the ends swapped into that order
    edge_keys = (v * Nv + u)[v < u]
    nbr_edge = np.searchsorted(edge_keys, np.minimum(v, u) * Nv + np.maximum(v, u))
    edges = np.stack((edge_keys // max(Nv, 1), edge_keys % max(Nv, 1)), axis=1).reshape(-1, 2)
    return np.ascontiguousarray(edges.astype(np.int32)), nbr_edge.astype(np.int32)


def _edge_tables(faces, num_vertices):
    """-> EdgeTables on faces' device, cached on the index tensor as _tables caches its own."""
    def build():
        t = _tables(faces, num_vertices)
        edges, nbr_edge = build_edge_tables(t.nbr_offsets.cpu().numpy(), t.nbr.cpu().numpy())
        return EdgeTables(torch.from_numpy(edges).to(faces.device), torch.from_numpy(nbr_edge).to(faces.device), t)

    return _util.cached_on_index(faces, _EDGE_ATTR, (int(num_vertices),), build,
                                 'the edge tables of this index tensor are not built yet, and building them reads the indices '
                                 'on the host: call edge_length_loss once with it before the capture')


def _check_index_only(name, faces, num_vertices):
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dtype != torch.bool and faces.dim() in (2, 3)
            and faces.shape[-1] == 3 and faces.shape[-2] >= 1):
        raise ValueError('%s: faces must be an integer tensor [num of faces, 3] or [batch size, num of faces, 3]' % name)
    if isinstance(num_vertices, bool) or not isinstance(num_vertices, int) or num_vertices < 1:
        raise ValueError('%s: num_vertices must be a positive integer, got %r' % (name, num_vertices))
    _util.check_face_indices(faces, num_vertices)


def mesh_edges(faces, num_vertices):
    """The edges of a topology: int64 [E,2] on faces' device, every row v0 < v1, ordered by (v0, v1) -- the order of
    edge_length_loss's target and of edge_lengths.  faces [Nf,3], or [B,Nf,3] whose images are all equal."""
    _check_index_only('mesh_edges', faces, num_vertices)
    return _edge_tables(faces, num_vertices).edges.long()


def _edge_lengths(x, edges):
    d = x[:, edges[:, 1].long()] - x[:, edges[:, 0].long()]
    return torch.sqrt((d * d).sum(2))


def edge_lengths(vertices, faces):
    """The length of every edge in mesh_edges' order: [B,E] from vertices [B,Nv,3], [E] from [Nv,3]; plain torch (any device,
    any float dtype), differentiable by torch's autograd (not at a zero-length edge: use it for targets,
    `edge_lengths(rest_vertices, faces).detach()`)."""
    vertices, squeeze = _check('edge_lengths', vertices, faces)
    _util.check_face_indices(faces, int(vertices.shape[1]), vertices.device)
    out = _edge_lengths(vertices, _edge_tables(faces, int(vertices.shape[1])).edges)
    return out[0] if squeeze else out


def _edge_target(name, target, vertices, num_edges):
    """-> (tensor [E] | [B,E] in vertices' dtype, or None; the number)"""
    if torch.is_tensor(target):
        B = int(vertices.shape[0])
        if not (target.is_floating_point() and tuple(target.shape) in ((num_edges,), (B, num_edges))):
            raise ValueError('%s: a target tensor must be a float tensor [num of edges] or [batch size, num of edges] = [%d] or '
                             '[%d, %d] in the order of mesh_edges, got %s %s'
                             % (name, num_edges, B, num_edges, target.dtype, tuple(target.shape)))
        if target.device != vertices.device:
            raise ValueError('%s: vertices and target must be on one device (%s, %s)' % (name, vertices.device, target.device))
        return target.to(vertices.dtype), 0.0
    value = _util.number(name, 'target', target)
    if not (0.0 <= value < float('inf')):
        raise ValueError('%s: target must be a finite number >= 0 (or a tensor), got %r' % (name, target))
    return None, value


def _edge_length_torch(x, e, target, value):
    q = e.edges.long()
    d = x[:, q[:, 1]] - x[:, q[:, 0]]
    n = (d * d).sum(2)
    if target is None and value == 0.0:
        return n.sum(1)
    pos = n > 0
    l = torch.sqrt(torch.where(pos, n, torch.ones_like(n)))      # (sqrt has no derivative at 0: the gradient is exactly 0 there)
    l = torch.where(pos, l, torch.zeros_like(n))
    r = l - (target if target is not None else value)
    return (r * r).sum(1)


def _cot_weights_torch(x, idx, eps):
    """cot [B,F,3] (not detached) for idx int64 [F,3]"""
    p = x[:, idx]                                                 # [B,F,3 corners,3]
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 0] != idx[:, 2])
    cots = []
    for c in range(3):
        a, b = p[:, :, (c + 1) % 3] - p[:, :, c], p[:, :, (c + 2) % 3] - p[:, :, c]
        n = torch.cross(a, b, dim=2)
        cots.append((a * b).sum(2) / torch.sqrt((n * n).sum(2) + eps))
    cot = torch.stack(cots, dim=2)
    return torch.where(ok[None, :, None], cot, torch.zeros_like(cot))


def _cot_apply_torch(phi, cot, idx):
    """L(phi) [B,Nv,3] with the weights cot [B,F,3]"""
    H = torch.zeros_like(phi)
    p = phi[:, idx]
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        term = cot[:, :, c2, None] * (p[:, :, c1] - p[:, :, c]) + cot[:, :, c1, None] * (p[:, :, c2] - p[:, :, c])
        H = H.index_add(1, idx[:, c], term)
    return 0.5 * H


def _one_topology(name, faces):
    """int64 [F,3] of faces [F,3] or [B,F,3] with equal images (checked on the host by the table builders; here by torch)."""
    if faces.dim() == 3:
        if faces.shape[0] > 1 and not bool((faces == faces[0:1]).all()):
            raise ValueError('%s: the faces of all images must be equal (one topology per call)' % name)
        faces = faces[0]
    return faces.long()


def _cotangent_laplacian_torch(x, idx, eps):
    H = _cot_apply_torch(x, _cot_weights_torch(x, idx, eps).detach(), idx)
    return (H * H).sum((1, 2))


def edge_length_loss_torch(vertices, faces, target=0.0):
    """edge_length_loss in plain torch (any device, any float dtype), differentiable by torch's autograd -- in a target tensor
    too."""
    vertices, squeeze = _check('edge_length_loss_torch', vertices, faces)
    _util.check_face_indices(faces, int(vertices.shape[1]), vertices.device)
    e = _edge_tables(faces, int(vertices.shape[1]))
    loss = _edge_length_torch(vertices, e, *_edge_target('edge_length_loss_torch', target, vertices, e.num_edges))
    return loss[0] if squeeze else loss


def cotangent_laplacian_loss_torch(vertices, faces, eps=1e-12):
    """cotangent_laplacian_loss in plain torch (any device, any float dtype), differentiable by torch's autograd with the
    cotangent weights under detach(): constants of the step."""
    vertices, squeeze = _check('cotangent_laplacian_loss_torch', vertices, faces)
    _util.check_face_indices(faces, int(vertices.shape[1]), vertices.device)
    loss = _cotangent_laplacian_torch(vertices, _one_topology('cotangent_laplacian_loss_torch', faces), float(eps))
    return loss[0] if squeeze else loss


@_util.once_differentiable
class _EdgeLengthLoss(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], edge tables, target tensor or None, target number) -> loss [B]; nothing but the vertices
    is saved: the backward recomputes every edge."""

    @staticmethod
    def forward(ctx, vertices, e, target, value):
        v = _lib.dense(vertices.detach())
        dev = v.device
        B, Nv = v.shape[:2]
        E = e.num_edges
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        per_batch = int(target is not None and target.dim() == 2)
        _lib.launch('nr_edge_length_forward', dev, v.data_ptr(), _lib.ptr(e.edges) if E else None, _lib.ptr(target),
                    loss.data_ptr(), B, Nv, E, per_batch, value,
                    workspace_bytes=_lib.workspace_bytes('nr_mesh_loss_workspace_bytes', B, E))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(v)
        ctx.tables, ctx.target, ctx.value, ctx.per_batch = e, target, value, per_batch
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        v, = ctx.saved_tensors
        e, t = ctx.tables, ctx.tables.mesh
        dev = v.device
        B, Nv = v.shape[:2]
        g = _lib.dense(grad_loss)
        grad_v = torch.empty_like(v)
        some = int(t.nbr.shape[0]) > 0
        _lib.launch('nr_edge_length_backward', dev, v.data_ptr(), t.nbr_offsets.data_ptr(), _lib.ptr(t.nbr) if some else None,
                    _lib.ptr(e.nbr_edge) if some else None, _lib.ptr(ctx.target), g.data_ptr(), grad_v.data_ptr(), B, Nv,
                    int(t.nbr.shape[0]), e.num_edges, ctx.per_batch, ctx.value)
        return grad_v, None, None, None


@_util.once_differentiable
class _CotangentLaplacianLoss(torch.autograd.Function):
    """forward(ctx, vertices [B,Nv,3], adjacency (vertex_colors._adjacency), eps) -> loss [B]; cot [B,F,3] and H [B,Nv,3] are
    kept for the backward when one can follow, and only then."""

    @staticmethod
    def forward(ctx, vertices, adj, eps):
        v = _lib.dense(vertices.detach())
        dev = v.device
        B, Nv = v.shape[:2]
        idx, offsets, entries = adj[:3]
        F = int(idx.shape[1])
        keep = ctx.needs_input_grad[0]
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        cot = torch.empty((B, F, 3), dtype=torch.float32, device=dev)
        H = torch.empty_like(v) if keep else None
        _lib.launch('nr_cot_weights', dev, v.data_ptr(), idx.data_ptr(), cot.data_ptr(), B, Nv, F, eps)
        _lib.launch('nr_cot_apply', dev, v.data_ptr(), cot.data_ptr(), idx.data_ptr(), offsets.data_ptr(), entries.data_ptr(), None,
                    _lib.ptr(H), loss.data_ptr(), B, Nv, F,
                    workspace_bytes=_lib.workspace_bytes('nr_mesh_loss_workspace_bytes', B, Nv))
        if keep:
            ctx.save_for_backward(cot, H)
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        cot, H = ctx.saved_tensors
        idx, offsets, entries = ctx.adj[:3]
        dev = H.device
        B, Nv = H.shape[:2]
        g = _lib.dense(grad_loss)
        grad_v = torch.empty_like(H)
        _lib.launch('nr_cot_apply', dev, H.data_ptr(), cot.data_ptr(), idx.data_ptr(), offsets.data_ptr(), entries.data_ptr(),
                    g.data_ptr(), grad_v.data_ptr(), None, B, Nv, int(idx.shape[1]), workspace_bytes=0)
        return grad_v, None, None


_NEEDS = 'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most'


def edge_length_loss(vertices, faces, target=0.0, implementation=None):
    """sum over the edges of (length - target)^2 per image: [B] from vertices [B,Nv,3], a 0-dim tensor from [Nv,3]; faces
    [Nf,3], or [B,Nf,3] whose images are all equal.  The edges are the distinct vertex pairs that share a face, in
    mesh_edges(faces, Nv)'s order.  `target`: a number >= 0 for every edge -- with 0, the default, the loss is the sum of the
    squared lengths and no square root is taken --, or a float tensor [E] or [B,E] in that order (rest lengths:
    `edge_lengths(rest_vertices, faces).detach()`), read in place and not differentiated by the kernels: a target that
    requires a gradient takes the torch path.  Differentiable (once) in vertices; the gradient of an edge of length 0 is
    exactly 0.  `implementation` as in laplacian_loss."""
    name = 'edge_length_loss'
    vertices, squeeze = _check(name, vertices, faces)
    B, Nv = int(vertices.shape[0]), int(vertices.shape[1])
    _util.check_implementation(name, implementation)
    _util.check_face_indices(faces, Nv, vertices.device)
    e = _edge_tables(faces, Nv)
    tensor, value = _edge_target(name, target, vertices, e.num_edges)
    fits = (vertices.is_cuda and vertices.dtype == torch.float32 and B <= 65535
            and not (tensor is not None and tensor.requires_grad))
    if _util.takes_hip(name, implementation, fits, _NEEDS + ' and a target that requires no gradient'):
        loss = _EdgeLengthLoss.apply(vertices, e, _lib.dense(tensor), value)
    else:
        loss = _edge_length_torch(vertices, e, tensor, value)
    return loss[0] if squeeze else loss


def cotangent_laplacian_loss(vertices, faces, eps=1e-12, implementation=None):
    """sum_v |H_v|^2 per image with the cotangent-weighted Laplacian H_v = 1/2 sum over the faces around v of
    cot_(c+2) (x_(c+1) - x_v) + cot_(c+1) (x_(c+2) - x_v), cot = (a . b) / sqrt(|a x b|^2 + eps) at every corner: [B] from
    vertices [B,Nv,3], a 0-dim tensor from [Nv,3]; faces as in laplacian_loss (one topology; a face with a repeated index adds
    nothing, a duplicated face counts twice).  H approximates the mean-curvature normal: the loss penalises bending, not an
    irregular triangulation.  Differentiable (once) in vertices WITH THE WEIGHTS HELD CONSTANT: the gradient is 2 g L(H), it
    does not differentiate the cotangents.  `implementation` as in laplacian_loss."""
    name = 'cotangent_laplacian_loss'
    vertices, squeeze = _check(name, vertices, faces)
    B, Nv = int(vertices.shape[0]), int(vertices.shape[1])
    eps = _util.number(name, 'eps', eps)
    fits = vertices.is_cuda and vertices.dtype == torch.float32 and B <= 65535
    hip = _util.takes_hip(name, implementation, fits, _NEEDS)
    _util.check_face_indices(faces, Nv, vertices.device)
    if hip:
        from .vertex_colors import _adjacency
        adj = _adjacency(faces, Nv)
        if adj[3]:
            raise ValueError('%s: the faces of all images must be equal (one topology per call)' % name)
        loss = _CotangentLaplacianLoss.apply(vertices, adj, eps)
    else:
        loss = _cotangent_laplacian_torch(vertices, _one_topology(name, faces), eps)
    return loss[0] if squeeze else loss
