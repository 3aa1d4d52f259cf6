"""Isosurface extraction (not in the reference's library): from a grid of values -- a predicted occupancy, a signed distance
under optimisation, a fused TSDF -- to a triangle mesh, by marching tetrahedra.  It is the way back from `voxelize`,
`signed_distance` and `voxel_centers`, and the extraction step of DMTet / MeshSDF-style fits, whose unknown is the grid.

`extract_isosurface(values, iso=0.0, inside='below')` -> `IsoSurface` (a list of B for values [B,D,H,W]): the topology -- `faces`
[F,3] int32 and `edge_nodes` [Nv,2] int32, the two grid nodes of the edge each vertex lies on -- without a gradient.
`IsoSurface.vertices(values, bounds=(-1, 1), align='centers', positions=None)` -> [Nv,3]: the positions, plain torch on the gathered
nodes, differentiable any number of times in `values` and `positions`.  `marching_tetrahedra(values, ...)` -> (vertices, faces) does
both.

ONE definition (csrc/nr_marching_tets.h, restated in `_extract_torch` and in tests/isosurface_ref.py).
  Grid.  values [D,H,W] with D, H, W >= 2; node (i,j,k) has the linear index n = (i H + j) W + k; axis 0 is x, as in
    `voxel_centers`.  A node is inside iff value < iso (inside='below', the convention of `signed_distance`) or value > iso
    (inside='above', for occupancies: `voxelize` with iso = 0.5).  A node exactly at iso is outside.  A non-finite value raises.
  Tetrahedra.  Cell (i,j,k), i < D-1, j < H-1, k < W-1, is cut into six tetrahedra along its main diagonal (Kuhn): for each
    permutation pi of the axes (0,1,2) in lexicographic order the corners c0 = (i,j,k), c1 = c0 + e_pi0, c2 = c1 + e_pi1,
    c3 = (i+1,j+1,k+1).  Every cell takes the same cut, so the diagonals on the faces of neighbouring cells agree.
  Vertices.  The grid's edges are the 7 kinds (di,dj,dk) in {0,1}^3 \\ 0 from a lower node a to b = a + (di,dj,dk) -- every edge of
    every tetrahedron is one of them.  A vertex lies on every edge with exactly one inside end; vertices are numbered in
    ascending (a, b), which within one a is the order of the code 4 di + 2 dj + dk.  edge_nodes holds (a, b), a < b.  Every
    crossing edge is used by a face: there are no unreferenced vertices.
  Faces, per tetrahedron, with e(p,q) the vertex on the edge of the corners p and q (local numbers 0..3): one inside corner p, the
    others q < r < s: the triangle e(p,q), e(p,r), e(p,s); three inside corners and the outside corner p: the same triple; two
    inside corners p < q and outside r < s: the quad e(p,r), e(p,s), e(q,s), e(q,r) as the triangles (0,1,2), (0,2,3).
  Orientation.  Counter-clockwise seen from the outside: the normal points from the inside corners' centroid to the outside
    corners'.  Where the order as written is the other one, the triangle's last two entries are exchanged.  This is decided
    once per (permutation, case) in a table (`_table`, the same numbers as the header's), never by arithmetic on the values.
  Face order.  Cells ascending by n of c0; within a cell the permutations in their order; within a tetrahedron as above.
  Positions.  t = (iso - s_a) / (s_b - s_a), v = p_a + t (p_b - p_a), always from a to b, so every cell of an edge computes the
    same bits.  With `bounds` (a pair or three pairs) and align='centers' a node sits at its `voxel_centers` position, lo + (i +
    1/2)(hi - lo) / D per axis -- the grid of `voxelize` extracts in place --; with align='corners' at lo + i (hi - lo) / (D - 1);
    both computed in float64 and rounded once.  `positions` [D,H,W,3] instead is a deformable grid.
  Degenerate vertices.  A node exactly at iso pulls the vertices of its crossing edges onto itself (t = 0 or 1): coincident
    vertices and zero-area faces, which are emitted as they are -- every operator of the package accepts collapsed faces; there
    is no weld.
The result is a manifold with consistent orientation for every field: no directed edge twice, every undirected edge in two faces
or, on the grid's boundary, in one.  A constant field gives faces [0,3] and edge_nodes [0,2].

Gradients.  The topology depends on the values through comparisons only and carries none.  The positions are the closed form
above on gathered nodes: there is no torch.autograd.Function here, so a second derivative simply works.  The gradient to the
values goes through torch's indexing backward, which adds the (at most 14) edges of a node in torch's order.

On float32 CUDA values (see `_NEEDS`) the extraction runs as HIP kernels (nr_isosurface_*, csrc/nr_isosurface.hip): a count
with a scan inside each workgroup's run of nodes, a scan of the workgroups' totals, ONE readback of the batch's counts, and an
emit -- no atomics, no workgroup that waits for another, the same bits in every run, for an image alone or inside a batch.  The
images of a batch have different topologies and still share the launches, the readback and the two allocations, of which the
per-image results are views.  Everything else -- CPU, other dtypes -- takes `_extract_torch`, the same definition vectorised
(gathers, the table, cumsum for the numbering), which returns the same integers entry for entry; it is also the kernels' second
yardstick in the tests.

Every new `faces` tensor makes the mesh operators (`laplacian_loss`, `point_mesh_distance`, ...) rebuild their host tables,
which are cached on the index tensor: 3-100 ms per topology.

HIP graphs: the operator reads back by design; inside a stream capture it raises."""
import math
import os

import torch

from . import _lib, _util
from .winding import _bounds

_NEEDS = ('the HIP kernels take float32 CUDA values with a batch size B of 65535 at most and 7 x D x H x W < 2^31')
# nodes per workgroup (1 .. 4096): 0 lets the library decide; the result does not depend on it (tests set it to reach the
# multi-workgroup paths on small grids)
_RUN = int(os.environ.get('NR_ISOSURFACE_RUN', '0') or 0)

_PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
_AXIS_BIT = (4, 2, 1)  # a corner's code 4 di + 2 dj + dk


def _make_table():
    """-> (corners [6][4]: the codes of c0..c3 per permutation, count [16]: triangles per 4-bit inside mask (bit p: corner p),
    table [6][16][6]: per triangle three bytes `owner code << 3 | edge code`, the vertex on the edge from cell corner `owner`
    along `edge`).  The orientation is decided here in integers: on doubled coordinates the midpoints, the normal and the
    centroids' difference times the counts are exact."""
    corners, table = [], []
    count = [bin(m).count('1') for m in range(16)]
    count = [0 if c in (0, 4) else (2 if c == 2 else 1) for c in count]
    for perm in _PERMUTATIONS:
        codes = [0, _AXIS_BIT[perm[0]], _AXIS_BIT[perm[0]] | _AXIS_BIT[perm[1]], 7]
        xyz = [((c >> 2) & 1, (c >> 1) & 1, c & 1) for c in codes]
        corners.append(codes)
        rows = []
        for mask in range(16):
            ins = [p for p in range(4) if (mask >> p) & 1]
            out = [p for p in range(4) if not (mask >> p) & 1]
            if len(ins) == 1 or len(ins) == 3:
                p = ins[0] if len(ins) == 1 else out[0]
                q, r, s = [x for x in range(4) if x != p]
                tris = [[(p, q), (p, r), (p, s)]]
            elif len(ins) == 2:
                (p, q), (r, s) = ins, out
                quad = [(p, r), (p, s), (q, s), (q, r)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            else:
                tris = []
            row = []
            for tri in tris:
                mid = [[xyz[a][c] + xyz[b][c] for c in range(3)] for a, b in tri]  # doubled midpoints
                u = [mid[1][c] - mid[0][c] for c in range(3)]
                v = [mid[2][c] - mid[0][c] for c in range(3)]
                n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
                d = [len(ins) * sum(xyz[p][c] for p in out) - len(out) * sum(xyz[p][c] for p in ins) for c in range(3)]
                side = sum(n[c] * d[c] for c in range(3))
                assert side != 0
                if side < 0:
                    tri = [tri[0], tri[2], tri[1]]
                for a, b in tri:
                    a, b = min(a, b), max(a, b)
                    row.append(codes[a] << 3 | (codes[a] ^ codes[b]))
            rows.append(row + [0] * (6 - len(row)))
        table.append(rows)
    return corners, count, table


_CORNERS, _COUNT, _TABLE = _make_table()


class IsoSurface(object):
    """The topology of an extracted surface: `faces` [F,3] int32, `edge_nodes` [Nv,2] int32 (the nodes a < b of each vertex's
    edge, linear indices into the grid), `grid_shape` (D,H,W), `iso`, `inside`, `num_vertices`, `num_faces`.  No gradient."""

    def __init__(self, faces, edge_nodes, grid_shape, iso, inside):
        self.faces, self.edge_nodes = faces, edge_nodes
        self.grid_shape, self.iso, self.inside = tuple(int(s) for s in grid_shape), float(iso), inside
        self.num_vertices, self.num_faces = int(edge_nodes.shape[0]), int(faces.shape[0])

    def vertices(self, values, bounds=(-1, 1), align='centers', positions=None):
        """-> [Nv,3]: v = p_a + t (p_b - p_a), t = (iso - s_a) / (s_b - s_a), on the nodes of `edge_nodes`; differentiable in
        `values` [D,H,W] and `positions` [D,H,W,3].  May be called again on changed values of the same topology: the caller
        keeps the signs of the values the surface was built from -- on an edge that no longer crosses t leaves [0,1], and
        nothing here checks it."""
        name = 'IsoSurface.vertices'
        if not (torch.is_tensor(values) and values.is_floating_point() and tuple(values.shape) == self.grid_shape):
            raise ValueError('%s: values must be a float tensor of the grid shape %s' % (name, self.grid_shape))
        if values.device != self.edge_nodes.device:
            raise ValueError('%s: values are on %s but the surface on %s' % (name, values.device, self.edge_nodes.device))
        a, b = self.edge_nodes[:, 0].long(), self.edge_nodes[:, 1].long()
        if positions is None:
            pa, pb = _node_positions(name, self.grid_shape, bounds, align, values, (a, b))
        else:
            _check_align(name, align)
            if not (torch.is_tensor(positions) and positions.is_floating_point()
                    and tuple(positions.shape) == self.grid_shape + (3,)):
                raise ValueError('%s: positions must be a float tensor of shape %s' % (name, self.grid_shape + (3,)))
            if positions.dtype != values.dtype or positions.device != values.device:
                raise ValueError('%s: positions and values must share dtype and device (%s %s, %s %s)'
                                 % (name, positions.dtype, positions.device, values.dtype, values.device))
            flat = positions.reshape(-1, 3)
            pa, pb = flat[a], flat[b]
        s = values.reshape(-1)
        sa, sb = s[a], s[b]
        t = (self.iso - sa) / (sb - sa)
        return pa + t[:, None] * (pb - pa)


def _check_align(name, align):
    if align not in ('centers', 'corners'):
        raise ValueError("%s: align must be 'centers' or 'corners', got %r" % (name, align))


def _node_positions(name, shape, bounds, align, like, nodes):
    """p of the nodes `nodes` (linear indices): per axis a table in float64, rounded once to `like`'s dtype"""
    _check_align(name, align)
    axes = []
    for (lo, hi), n in zip(_bounds(name, bounds), shape):
        i = torch.arange(n, dtype=torch.float64)
        axis = lo + (i + 0.5) * ((hi - lo) / n) if align == 'centers' else lo + i * ((hi - lo) / (n - 1))
        axes.append(axis.to(device=like.device, dtype=like.dtype))
    D, H, W = shape
    out = []
    for n in nodes:
        ij = torch.div(n, W, rounding_mode='floor')
        out.append(torch.stack((axes[0][torch.div(ij, H, rounding_mode='floor')], axes[1][ij % H], axes[2][n % W]), -1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# checks

def _inputs(name, values, iso, inside, implementation):
    """-> (values [B,D,H,W], iso, above, squeeze, use_hip)"""
    _util.check_implementation(name, implementation)
    if not (torch.is_tensor(values) and values.is_floating_point() and values.dim() in (3, 4) and values.shape[0] >= 1):
        raise ValueError('%s: values must be a float tensor [D, H, W] or [batch size, D, H, W]' % name)
    if min(values.shape[-3:]) < 2:
        raise ValueError('%s: D, H and W must be 2 at least, got %s' % (name, tuple(values.shape[-3:])))
    iso = _util.number(name, 'iso', iso)
    if not math.isfinite(iso):
        raise ValueError('%s: iso must be finite, got %r' % (name, iso))
    if inside not in ('below', 'above'):
        raise ValueError("%s: inside must be 'below' or 'above', got %r" % (name, inside))
    squeeze = values.dim() == 3
    v = values.detach()[None] if squeeze else values.detach()
    B, N = int(v.shape[0]), int(v.shape[1]) * int(v.shape[2]) * int(v.shape[3])
    fits = v.is_cuda and v.dtype == torch.float32 and B <= 65535 and 7 * N < 2 ** 31
    hip = _util.takes_hip(name, implementation, fits, _NEEDS)
    if v.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('%s reads the counts of vertices and faces back: extract the surface before the capture' % name)
    return v, iso, inside == 'above', squeeze, hip


def _non_finite(name):
    return ValueError('%s: values must be finite' % name)


# ---------------------------------------------------------------------------------------------------------------------
# plain torch: csrc/nr_marching_tets.h vectorised

def _tables(device):
    corners = torch.tensor(_CORNERS, dtype=torch.long, device=device)                   # [6,4]
    count = torch.tensor(_COUNT, dtype=torch.long, device=device)                       # [16]
    table = torch.tensor(_TABLE, dtype=torch.long, device=device).reshape(6, 16, 2, 3)  # [6,16,2,3]
    return corners, count, table


def _extract_torch(name, v, iso, above):
    """-> (edge_nodes [sum Nv,2] int32, faces [sum F,3] int32, Nv per image, F per image) of values [B,D,H,W]; the vertex
    numbers in `faces` count from 0 in every image"""
    B, D, H, W = (int(s) for s in v.shape)
    N, dev = D * H * W, v.device
    if not bool(torch.isfinite(v).all()):
        raise _non_finite(name)
    level = torch.tensor(iso, dtype=v.dtype, device=dev)
    inside = (v > level) if above else (v < level)
    # the crossing edges of every node: [B,D,H,W,7] for the codes 1..7
    cross = torch.zeros((B, D, H, W, 7), dtype=torch.bool, device=dev)
    offsets = []
    for code in range(1, 8):
        di, dj, dk = (code >> 2) & 1, (code >> 1) & 1, code & 1
        offsets.append((di * H + dj) * W + dk)
        cross[:, :D - di, :H - dj, :W - dk, code - 1] = inside[:, :D - di, :H - dj, :W - dk] != inside[:, di:, dj:, dk:]
    offsets = torch.tensor([0] + offsets, dtype=torch.long, device=dev)
    flat = cross.reshape(B, N * 7)
    number = torch.cumsum(flat, 1, dtype=torch.int32) - 1              # the vertex of (node, code) where it crosses
    num_vertices = [int(x) for x in flat.sum(1)]
    where = flat.nonzero()                                             # ascending (image, node, code)
    a = torch.div(where[:, 1], 7, rounding_mode='floor')
    b = a + offsets[where[:, 1] % 7 + 1]
    edge_nodes = torch.stack((a, b), 1).to(torch.int32)
    # the cells that hold faces: the 8-bit inside mask, bit = corner code
    mask = torch.zeros((B, D - 1, H - 1, W - 1), dtype=torch.long, device=dev)
    for code in range(8):
        di, dj, dk = (code >> 2) & 1, (code >> 1) & 1, code & 1
        mask |= inside[:, di:D - 1 + di, dj:H - 1 + dj, dk:W - 1 + dk].long() << code
    active = ((mask != 0) & (mask != 255)).nonzero()                    # ascending (image, i, j, k)
    image = active[:, 0]
    node = (active[:, 1] * H + active[:, 2]) * W + active[:, 3]
    mask = mask[active[:, 0], active[:, 1], active[:, 2], active[:, 3]]  # [A]
    corners, count, table = _tables(dev)
    tet = ((mask[:, None, None] >> corners[None]) & 1)                  # [A,6,4]
    tet = tet[..., 0] | tet[..., 1] << 1 | tet[..., 2] << 2 | tet[..., 3] << 3      # [A,6]
    perm = torch.arange(6, device=dev)[None].expand_as(tet)
    entries = table[perm, tet]                                          # [A,6,2,3]
    valid = torch.arange(2, device=dev)[None, None] < count[tet][..., None]         # [A,6,2]
    owner = node[:, None, None, None] + offsets[entries >> 3]
    slot = owner * 7 + (entries & 7) - 1
    ids = number[image[:, None, None, None].expand_as(slot), slot]      # [A,6,2,3] int32
    faces = ids[valid]                                                  # ascending (cell, permutation, triangle)
    per_cell = valid.sum((1, 2))
    num_faces = [int(x) for x in torch.zeros(B, dtype=torch.long, device=dev).index_add_(0, image, per_cell)]
    return edge_nodes, faces.reshape(-1, 3), num_vertices, num_faces


# ---------------------------------------------------------------------------------------------------------------------
# HIP

def _extract_hip(name, v, iso, above):
    """the same outputs from the kernels: count and scans, ONE readback of [B,3], emit"""
    v = _lib.dense(v)
    B, D, H, W = (int(s) for s in v.shape)
    dev = v.device
    ws_bytes = _lib.workspace_bytes('nr_isosurface_workspace_bytes', B, D, H, W, _RUN)
    ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)  # lives from the count to the emit
    totals = torch.empty((B, 3), dtype=torch.int32, device=dev)
    _lib.launch('nr_isosurface_count', dev, v.data_ptr(), totals.data_ptr(), B, D, H, W, iso, 1 if above else 0, _RUN,
                ws.data_ptr(), ws_bytes)
    counts = totals.cpu().tolist()                                      # the one synchronisation
    if any(row[2] for row in counts):
        raise _non_finite(name)
    num_vertices = [row[0] for row in counts]
    num_faces = [row[1] & 0xffffffff for row in counts]                 # (an unsigned count: up to 12 per cell)
    edge_nodes = torch.empty((sum(num_vertices), 2), dtype=torch.int32, device=dev)
    faces = torch.empty((sum(num_faces), 3), dtype=torch.int32, device=dev)
    if edge_nodes.shape[0]:
        _lib.launch('nr_isosurface_emit', dev, edge_nodes.data_ptr(), faces.data_ptr(), int(edge_nodes.shape[0]),
                    int(faces.shape[0]), B, D, H, W, _RUN, ws.data_ptr(), ws_bytes)
    return edge_nodes, faces, num_vertices, num_faces


# ---------------------------------------------------------------------------------------------------------------------
# public

def extract_isosurface(values, iso=0.0, inside='below', implementation=None):
    """-> IsoSurface (a list of B for values [B,D,H,W]): the marching-tetrahedra surface of the level `iso`, topology only.
    One set of launches and one readback for the batch; the per-image tensors are views of two shared allocations.  See the
    module docstring."""
    return _extract('extract_isosurface', values, iso, inside, implementation)


def _extract(name, values, iso, inside, implementation):
    v, iso, above, squeeze, hip = _inputs(name, values, iso, inside, implementation)
    with torch.no_grad():
        edge_nodes, faces, nv, nf = (_extract_hip if hip else _extract_torch)(name, v, iso, above)
    out, v0, f0 = [], 0, 0
    for b in range(int(v.shape[0])):
        out.append(IsoSurface(faces[f0:f0 + nf[b]], edge_nodes[v0:v0 + nv[b]], v.shape[1:], iso, inside))
        v0, f0 = v0 + nv[b], f0 + nf[b]
    return out[0] if squeeze else out


def marching_tetrahedra(values, iso=0.0, bounds=(-1, 1), inside='below', align='centers', positions=None, implementation=None):
    """-> (vertices [Nv,3], faces [F,3] int32), or a list of B such pairs for values [B,D,H,W] (with `positions` [B,D,H,W,3]):
    `extract_isosurface` and `IsoSurface.vertices` in one call; the vertices are differentiable in `values` and `positions`."""
    name = 'marching_tetrahedra'
    _check_align(name, align)
    if positions is None:
        _bounds(name, bounds)
    elif not (torch.is_tensor(positions) and torch.is_tensor(values) and tuple(positions.shape) == tuple(values.shape) + (3,)):
        raise ValueError('%s: positions must be a float tensor of the shape of values + (3,)' % name)
    surfaces = _extract(name, values, iso, inside, implementation)
    if isinstance(surfaces, IsoSurface):
        return surfaces.vertices(values, bounds, align, positions), surfaces.faces
    return [(s.vertices(values[b], bounds, align, None if positions is None else positions[b]), s.faces)
            for b, s in enumerate(surfaces)]
