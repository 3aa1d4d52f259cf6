"""Mesh subdivision: differentiable Loop and midpoint refinement (not in the reference's library).

`subdivision(faces, num_vertices, levels, scheme)` plans `levels` refinements of ONE topology and returns a `Subdivision`:
its `faces` are the refined indices, and calling it on per-vertex data [Nv,C] or [B,Nv,C] -- positions, `VertexColors`, any
attribute with 1 <= C <= 16 channels -- returns the refined data [..,Nv',C], once-differentiable in the data.
`subdivide(vertices, faces, levels, scheme)` does both at once; `icosphere(level)` is a sphere template;
`Mesh.subdivide` refines a `Mesh` in place.  Two uses: coarse to fine (fit a few hundred vertices, subdivide, continue), and
a subdivision-surface parametrisation (learn a coarse control mesh, render its Loop surface on every step).

Definition of one level, on faces [F,3] over Nv vertices.
  Edges: every unordered pair {p < q} that occurs as a side of a face, E of them, ordered by (p, q).  Edge number e owns the
    new vertex Nv + e; old vertices keep their indices: Nv' = Nv + E.
  Sharp edges: m(e) is the number of (face, side) occurrences of the edge, duplicate faces counted; the edge is SHARP when
    m(e) != 2 -- a boundary edge, or an edge in three or more faces.
  Children: face f = (a, b, c) becomes faces 4 f .. 4 f + 3 = (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca): the
    winding is kept, and `face_parent[k] = k // 4^L` after L levels.
  scheme='midpoint': old vertex v: the row {v: 1}; edge vertex: {p: 1/2, q: 1/2}.
  scheme='loop' (Loop's rules with Warren's weights and the usual boundary and crease rules).  N(v) is the set of distinct
    vertices joined to v by an edge, n = |N(v)|, s(v) the number of sharp edges at v.
      old vertex, n = 0 (no face):      {v: 1}
      old vertex, s = 0:                beta = 3/16 if n = 3 else 3 / (8 n);  {v: 1 - n beta, u: beta for u in N(v)}
      old vertex, s = 2:                {v: 3/4, the two sharp neighbours: 1/8 each}
      old vertex, any other s:          {v: 1}                        (a corner, a non-manifold point)
      edge vertex, sharp edge:          {p: 1/2, q: 1/2}
      edge vertex, edge in two faces:   {p: 3/8, q: 3/8, o1: 1/8, o2: 1/8}, o1 and o2 the opposite vertices
  Weights: computed in float64 with exactly these expressions (1.0 - n * beta), entries of a row with equal column added in
    float64 (o1 = o2: two identical faces), then rounded to float32 once.  Every row sums to 1 (affine invariance).
  Summation order of a row: its entries in ascending column; with x_k the float32 input of the k-th entry,
    acc = w_0 * x_0 (one rounding), then acc = fmaf(w_k, x_k, acc).  A row {v: 1} copies its input bit for bit.
  Backward: every level is the transposed table, built on the host once -- its rows are the input vertices, its entries in
    ascending output vertex -- applied to the incoming gradient by the same kernel.
  L levels are L applications on the successive topologies: one launch per level and direction, the intermediates ordinary
    torch allocations.

On CUDA float32 data with B <= 65535 and C <= 16 every level runs as the HIP kernel of csrc/nr_subdivision.hip
(nr_stencil_apply) in both directions: a gather without atomics in a fixed order, every output element stored, so every
result repeats bit for bit and an image alone gives the bits it has inside a batch.  Everything else -- CPU tensors, other
dtypes, C > 16 -- takes the plain-torch path (`implementation='torch'`), an index_add over the same tables in any order.

The tables are built on the host in vectorised NumPy the first time (index tensor, num_vertices, levels, scheme) is seen
and cached on the index tensor, as mesh_losses._tables caches its tables: the build reads the indices back, so it must
happen BEFORE a graph capture (inside a capture an unknown topology raises).

Out of scope: resampling texture cubes across a subdivision (`Mesh.subdivide` repeats the parent's cube), subdividing a
`UVLayout`, adaptive or partial refinement, creases chosen by the user."""
import numpy as np
import torch

from . import _lib, _util

_PLANS_ATTR = '_nr_subdivision_plans'  # stashed on the index tensor OBJECT (see _util._INDEX_ATTR for why not on data_ptr alone)
_INT32_MAX = 2 ** 31 - 1
MAX_CHANNELS = 16   # nr_stencil_apply's limit
SCHEMES = ('loop', 'midpoint')


# ---------------------------------------------------------------------------------------------------------------------
# host tables

def _csr(rows, cols, w64, num_rows, num_cols):
    """Entries (row, col, float64 weight) -> (offsets int32 [num_rows + 1], cols int32, weights float32), entries with equal
    (row, col) added in float64, ordered by (row, col)."""
    key, inverse = np.unique(rows * np.int64(num_cols) + cols, return_inverse=True)
    if key.size > _INT32_MAX:
        raise ValueError('subdivision: %d table entries do not fit in int32' % key.size)
    w = np.bincount(inverse.reshape(-1), weights=w64, minlength=key.size)
    offsets = np.zeros(num_rows + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(key // num_cols, minlength=num_rows))
    return offsets.astype(np.int32), (key % num_cols).astype(np.int32), w.astype(np.float32)


def _transpose(offsets, cols, weights, num_cols):
    """The CSR table of the transposed operator: rows = the columns, entries in ascending (old) row."""
    num_rows = offsets.shape[0] - 1
    rows = np.repeat(np.arange(num_rows, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    order = np.argsort(cols.astype(np.int64) * num_rows + rows, kind='stable')
    t_off = np.zeros(num_cols + 1, np.int64)
    t_off[1:] = np.cumsum(np.bincount(cols, minlength=num_cols))
    return t_off.astype(np.int32), rows[order].astype(np.int32), np.ascontiguousarray(weights[order])


def build_level(faces_idx, num_vertices, scheme='loop'):
    """One level on the host: -> (child faces int32 [4F,3], Nv', (offsets, cols, weights) of the level's table).  See the
    module docstring for the definition."""
    f = np.asarray(faces_idx, dtype=np.int64).reshape(-1, 3)
    Nv, F = int(num_vertices), int(f.shape[0])
    if f.size and (f.min() < 0 or f.max() >= Nv):
        raise IndexError('a vertex index outside [0, %d)' % Nv)
    bad = np.nonzero((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))[0]
    if bad.size:
        k = int(bad[0])
        raise ValueError('subdivision: face %d (%d, %d, %d) repeats a vertex index' % ((k,) + tuple(int(i) for i in f[k])))
    if 4 * F > _INT32_MAX:
        raise ValueError('subdivision: %d faces do not fit in int32' % (4 * F))
    # the three sides of every face, face-major: side k of face f joins corner k and corner k + 1, opposite corner k + 2
    e0, e1, opp = f[:, (0, 1, 2)].reshape(-1), f[:, (1, 2, 0)].reshape(-1), f[:, (2, 0, 1)].reshape(-1)
    lo, hi = np.minimum(e0, e1), np.maximum(e0, e1)
    uniq, side_edge, m = np.unique(lo * Nv + hi, return_inverse=True, return_counts=True)   # ordered by (p, q)
    side_edge = side_edge.reshape(-1)
    E = int(uniq.shape[0])
    if Nv + E > _INT32_MAX:
        raise ValueError('subdivision: %d vertices do not fit in int32' % (Nv + E))
    p, q = uniq // Nv, uniq % Nv
    mid = (Nv + side_edge).reshape(F, 3)
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    children = np.stack((a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca), axis=1).reshape(4 * F, 3).astype(np.int32)

    old = np.arange(Nv, dtype=np.int64)
    new = Nv + np.arange(E, dtype=np.int64)
    half, ones = np.full(E, 0.5), np.ones(Nv)
    if scheme == 'midpoint':
        rows = np.concatenate((old, new, new))
        cols = np.concatenate((old, p, q))
        w = np.concatenate((ones, half, half))
    else:
        sharp = m != 2
        n = np.bincount(p, minlength=Nv) + np.bincount(q, minlength=Nv)
        s = np.bincount(p[sharp], minlength=Nv) + np.bincount(q[sharp], minlength=Nv)
        smooth_v = (n > 0) & (s == 0)
        crease_v = (n > 0) & (s == 2)
        nf = n.astype(np.float64)
        beta = np.where(n == 3, 3.0 / 16.0, 3.0 / (8.0 * np.maximum(nf, 1.0)))
        centre = np.where(smooth_v, 1.0 - nf * beta, np.where(crease_v, 0.75, 1.0))
        # old vertices: the directed edges (v, u) of the smooth vertices with beta, of the crease vertices' sharp edges with 1/8
        dv, du, dsharp = np.concatenate((p, q)), np.concatenate((q, p)), np.concatenate((sharp, sharp))
        ring = smooth_v[dv]
        crease = crease_v[dv] & dsharp
        # edge vertices: interior edges take their two opposite corners
        inner = ~sharp[side_edge]
        rows = np.concatenate((old, dv[ring], dv[crease], new, new, Nv + side_edge[inner]))
        cols = np.concatenate((old, du[ring], du[crease], p, q, opp[inner]))
        end = np.where(sharp, 0.5, 0.375)
        w = np.concatenate((centre, beta[dv[ring]], np.full(int(crease.sum()), 0.125), end, end, np.full(int(inner.sum()), 0.125)))
    return children, Nv + E, _csr(rows, cols, w, Nv + E, Nv)


class _Table(object):
    """A CSR table on a device: y[r] = sum over e in [offsets[r], offsets[r + 1]) of weights[e] x[cols[e]]."""

    def __init__(self, offsets, cols, weights, num_in, device):
        self.num_in, self.num_out, self.num_entries = int(num_in), int(offsets.shape[0]) - 1, int(cols.shape[0])
        self.offsets, self.cols, self.weights = (torch.from_numpy(t).to(device) for t in (offsets, cols, weights))
        self._rows = None

    def rows(self):
        """The row of every entry, int64 (the torch path's index_add)."""
        if self._rows is None:
            off = self.offsets.long()
            self._rows = torch.repeat_interleave(torch.arange(self.num_out, device=off.device), off[1:] - off[:-1])
        return self._rows


class _Level(object):
    """One level: the table and its transpose."""

    def __init__(self, table, num_in, device):
        offsets, cols, weights = table
        self.forward = _Table(offsets, cols, weights, num_in, device)
        self.backward = _Table(*_transpose(offsets, cols, weights, num_in), num_in=offsets.shape[0] - 1, device=device)


# ---------------------------------------------------------------------------------------------------------------------
# applying a table

def _apply_torch(x, t):
    B, _, C = x.shape
    terms = x[:, t.cols.long()] * t.weights.to(x.dtype)[None, :, None]
    return torch.zeros((B, t.num_out, C), dtype=x.dtype, device=x.device).index_add(1, t.rows(), terms)


def _apply_hip(x, t):
    x = _lib.dense(x)
    B, _, C = x.shape
    y = torch.empty((B, t.num_out, C), dtype=torch.float32, device=x.device)
    _lib.launch('nr_stencil_apply', x.device, x.data_ptr(), t.offsets.data_ptr(), t.cols.data_ptr(), t.weights.data_ptr(),
                y.data_ptr(), B, t.num_in, t.num_out, C, t.num_entries)
    return y


@_util.once_differentiable
class _ApplyLevel(torch.autograd.Function):
    """forward(ctx, x [B,Nin,C], level) -> [B,Nout,C]; the backward applies the transposed table to the gradient."""

    @staticmethod
    def forward(ctx, x, level):
        ctx.level = level
        return _apply_hip(x.detach(), level.forward)

    @staticmethod
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None
        return _apply_hip(grad, ctx.level.backward), None


# ---------------------------------------------------------------------------------------------------------------------
# the plan

class Subdivision(object):
    """`levels` refinements of one topology (see the module docstring).
    faces [4^L F, 3] int32 on the input faces' device; face_parent [4^L F] int64: the input face of every output face;
    num_vertices_in, num_vertices, levels, scheme.  Calling the plan refines per-vertex data."""

    def __init__(self, faces, face_parent, num_vertices_in, num_vertices, levels, scheme, tables):
        self.faces, self.face_parent = faces, face_parent
        self.num_vertices_in, self.num_vertices, self.levels, self.scheme = num_vertices_in, num_vertices, levels, scheme
        self._levels = tables

    def __call__(self, x, implementation=None):
        """x [Nv,C] or [B,Nv,C] float -> [..,Nv',C], differentiable (once) in x.  `implementation`: None picks the HIP
        kernel when the call fits it (float32 CUDA, B <= 65535, C <= 16), 'torch' / 'hip' force one ('hip' raises when the
        call does not fit)."""
        _util.check_implementation('subdivision', implementation)
        if not (torch.is_tensor(x) and x.is_floating_point() and x.dim() in (2, 3) and x.shape[-1] >= 1 and x.shape[0] >= 1):
            raise ValueError('subdivision: the data must be a float tensor [num of vertices, channels] or [batch size, num of '
                             'vertices, channels]')
        if x.shape[-2] != self.num_vertices_in:
            raise ValueError('subdivision: the plan takes %d vertices, the data has %d' % (self.num_vertices_in, x.shape[-2]))
        if x.device != self.faces.device:
            raise ValueError('subdivision: the data and the faces must be on one device (%s, %s)' % (x.device, self.faces.device))
        if not self._levels:   # levels = 0: the input itself
            return x
        squeeze = x.dim() == 2
        if squeeze:
            x = x[None]
        B, C = int(x.shape[0]), int(x.shape[2])
        fits = x.is_cuda and x.dtype == torch.float32 and B <= 65535 and C <= MAX_CHANNELS
        hip = _util.takes_hip('subdivision', implementation, fits, 'the HIP kernel takes float32 CUDA tensors with a batch size '
                              'of 65535 and %d channels at most' % MAX_CHANNELS)
        for level in self._levels:
            x = _ApplyLevel.apply(x, level) if hip else _apply_torch(x, level.forward)
        return x[0] if squeeze else x


def _check_faces(faces):
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dtype != torch.bool and faces.dim() in (2, 3)
            and faces.shape[-1] == 3 and faces.shape[-2] >= 1 and faces.shape[0] >= 1):
        raise ValueError('subdivision: faces must be an integer tensor [num of faces, 3] or [batch size, num of faces, 3]')


def _check_arguments(num_vertices, levels, scheme):
    if scheme not in SCHEMES:
        raise ValueError("subdivision: scheme must be 'loop' or 'midpoint'")
    if int(levels) != levels or levels < 0:
        raise ValueError('subdivision: levels must be an integer >= 0')
    if not 1 <= int(num_vertices) <= _INT32_MAX:
        raise ValueError('subdivision: %d vertices do not fit in int32' % int(num_vertices))


def subdivision(faces, num_vertices, levels=1, scheme='loop'):
    """-> the Subdivision plan of `levels` refinements of faces [F,3] (or [B,F,3] whose images are all equal) over
    `num_vertices` vertices, cached on the index tensor (and for a view on the tensor it is a view of) under its identity:
    data_ptr, shape, strides, version counter, device, and (num_vertices, levels, scheme)."""
    _check_arguments(num_vertices, levels, scheme)
    _check_faces(faces)
    Nv, levels = int(num_vertices), int(levels)
    F = int(faces.shape[-2])
    if F * 4 ** levels > _INT32_MAX:
        raise ValueError('subdivision: %d faces after %d levels do not fit in int32' % (F * 4 ** levels, levels))
    _util.check_face_indices(faces, Nv)   # (the vertex and entry counts of every level: build_level, ahead of any launch)

    def build():
        host = faces.detach().cpu().numpy()
        if host.ndim == 3:
            if not (host == host[0:1]).all():
                raise ValueError('subdivision: the faces of all images must be equal (one topology per call)')
            host = host[0]
        dev = faces.device
        f, nv, tables = host, Nv, []
        for _ in range(levels):
            f, nv_out, table = build_level(f, nv, scheme)
            tables.append(_Level(table, nv, dev))
            nv = nv_out
        out_faces = torch.from_numpy(np.ascontiguousarray(f.astype(np.int32))).to(dev)
        parent = torch.arange(out_faces.shape[0], dtype=torch.int64, device=dev) // (4 ** levels)
        return Subdivision(out_faces, parent, Nv, nv, levels, scheme, tables)

    return _util.cached_on_index(faces, _PLANS_ATTR, (Nv, levels, scheme), build,
                                 'the subdivision plan of this index tensor is not built yet, and building it reads the indices '
                                 'on the host: call subdivision / subdivide once with it before the capture')


def subdivide(vertices, faces, levels=1, scheme='loop', implementation=None):
    """-> (vertices' [..,Nv',C], faces'): `levels` refinements of vertices [Nv,C] or [B,Nv,C] on faces [F,3] or [B,F,3] (all
    images equal), differentiable (once) in the vertices.  faces' has the batch layout of faces: [4^L F, 3], or an expanded
    view [B, 4^L F, 3].  levels = 0 returns the inputs unchanged."""
    _util.check_implementation('subdivision', implementation)
    if not (torch.is_tensor(vertices) and vertices.dim() in (2, 3)):
        raise ValueError('subdivision: the data must be a float tensor [num of vertices, channels] or [batch size, num of '
                         'vertices, channels]')
    _check_faces(faces)
    if faces.dim() == 3 and (vertices.dim() != 3 or faces.shape[0] != vertices.shape[0]):
        raise ValueError('subdivision: faces have batch size %d, vertices %s' % (faces.shape[0], tuple(vertices.shape)))
    if faces.device != vertices.device:
        raise ValueError('subdivision: the data and the faces must be on one device (%s, %s)' % (vertices.device, faces.device))
    plan = subdivision(faces, vertices.shape[-2], levels, scheme)
    out = plan(vertices, implementation)
    if plan.levels == 0:
        return out, faces
    return out, (plan.faces[None].expand(faces.shape[0], -1, -1) if faces.dim() == 3 else plan.faces)


# ---------------------------------------------------------------------------------------------------------------------
# a sphere template

def _icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                  (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], np.int32)
    return v / np.linalg.norm(v, axis=1, keepdims=True), f


def icosphere(level, radius=1.0, device=None):
    """-> (vertices float32 [10 * 4^level + 2, 3] on the sphere of `radius`, faces int32 [20 * 4^level, 3], outward for the
    renderer's convention): the icosahedron refined `level` times by this module's midpoint scheme in float64, every vertex
    put back on the sphere after each level.  Host code, not differentiable."""
    if int(level) != level or level < 0:
        raise ValueError('icosphere: level must be an integer >= 0')
    if 20 * 4 ** int(level) > _INT32_MAX:
        raise ValueError('icosphere: %d faces do not fit in int32' % (20 * 4 ** int(level)))
    v, f = _icosahedron()
    for _ in range(int(level)):
        f, nv, (offsets, cols, weights) = build_level(f, v.shape[0], 'midpoint')
        rows = np.repeat(np.arange(nv), np.diff(offsets))
        out = np.zeros((nv, 3), np.float64)
        np.add.at(out, rows, v[cols] * weights.astype(np.float64)[:, None])
        v = out / np.linalg.norm(out, axis=1, keepdims=True)
    vertices = torch.from_numpy((v * float(radius)).astype(np.float32))
    faces = torch.from_numpy(np.ascontiguousarray(f.astype(np.int32)))
    return (vertices, faces) if device is None else (vertices.to(device), faces.to(device))
