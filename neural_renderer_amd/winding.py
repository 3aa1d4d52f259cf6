"""Generalized winding numbers (not in the reference's library): whether a point is inside a mesh, and what follows from it --
occupancy, voxel grids, the sign of the distance -- with exact gradients to points and vertices.

`winding_number(points, vertices, faces)` -> [B,N]: w(p) = (1 / 4 pi) sum_f Omega_f(p), the signed solid angles of the faces
seen from p.  With A = v0 - p, B = v1 - p, C = v2 - p and la, lb, lc their lengths (van Oosterom-Strackee)

    num = A . (B x C),   den = la lb lc + (A . B) lc + (B . C) la + (C . A) lb,   Omega = 2 atan2(num, den).

w is 1 inside a closed mesh with outward faces and 0 outside, -1 inside when the faces are reversed, k inside k nested
shells, and it degrades gracefully on open, self-intersecting or partly collapsed meshes.  It is smooth away from the surface
and once-differentiable in points and vertices; the gradient is the exact derivative of the expression above
(csrc/nr_solid_angle.h).  EXACTLY ON a face the value is not specified: the sign of a zero `num` decides between +1/2 and
-1/2 of that face.  Edge rules: a face with two corners equal as positions contributes exactly 0 to w and to every gradient; a
point on a vertex (num = den = 0) takes Omega = 0 and a zero gradient from that face; a non-finite coordinate of a point makes
its value NaN and a non-finite corner of a face that is not skipped makes the image's values NaN -- nothing is clamped, and no
epsilon appears anywhere: a scene scaled by a power of two has the same w, bit for bit.

`mesh_occupancy(points, vertices, faces, threshold=0.5)` -> bool [B,N], w > threshold.  `voxel_centers(grid_size, bounds)` ->
[G^3,3]: voxel [i,j,k] has its centre at lo + (i + 1/2, j + 1/2, k + 1/2) (hi - lo) / G in x, y, z.  `voxelize(vertices, faces,
grid_size, bounds, hard)` -> [B,G,G,G] float32: w > 0.5 as 0 / 1 (hard), or w itself, differentiable in the vertices; the centres
are one cloud shared by the batch.  (Inside and outside a CLOSED mesh w is 1 and 0 wherever the vertices are, so its gradient
is 0 there: w supervises open, self-intersecting and collapsing meshes; to fit a closed mesh to an occupancy grid take the
soft occupancy from `signed_distance`, as examples/example_voxel_fit.py does.)  `voxel_iou(a, b)` -> [B]: sum ab / (sum (a + b - ab) + eps).  `signed_distance(points,
vertices, faces)` -> [B,N]: -sqrt(dist2) where w > 0.5 and +sqrt(dist2) elsewhere, dist2 from `closest_surface_points`; the
gradient goes through dist2 only (0 where dist2 = 0), the sign carries none.

points [B,N,3], or [N,3] / [1,N,3] shared by the batch and read in place; vertices [B,Nv,3] or [Nv,3]; faces [F,3] integer, one
topology per call.  When no input has a batch axis the outputs have none.

On float32 CUDA tensors (see `_NEEDS`) the sums run as HIP kernels (nr_winding_*, csrc/nr_winding.hip): dense points x faces
sweeps with the streamed side in LDS, split over workgroups for small calls, the sums in double in a fixed two-level order --
no atomics, the same bits in every run, for an image alone or inside a batch, split or not.  Everything else -- CPU, other
dtypes, a shared `points` tensor that requires a gradient -- takes the plain-torch path, a chunked sweep in the same operation
order with the same analytic gradient; it is also the kernels' second yardstick in the tests.

HIP graphs: nothing here was ever captured, and a captured point-loss step once crashed inside torch's capture_end for a
reason that is only supposed (README "Soft silhouettes").  The advice that holds for the soft operators holds here: capture
before any eager backward on the same leaves, or run the eager steps under no_grad; the index tensor's tables must exist
before a capture (call once eagerly)."""
import math
import os

import torch

from . import _lib, _util
from .point_losses import _CHUNK_ELEMENTS
from .point_mesh import _inputs, closest_surface_points
from .vertex_colors import _adjacency

_NEEDS = ('the HIP kernels take float32 CUDA tensors with a batch size B of 65535 at most, B x points <= (2^31 - 1) / 3, B x faces '
          '<= (2^31 - 1) / 18, B x vertices <= (2^31 - 1) / 6, and a shared points tensor only when it requires no gradient')
# the number of parts the streamed side is cut into: 0 lets the library decide, n >= 1 forces n (1: none); the result does not
# depend on it (tests and scripts/winding_timing.py set it)
_SPLIT = int(os.environ.get('NR_WINDING_SPLIT', '0') or 0)
# csrc/nr_winding.hip's NR_WN_T and NR_WN_Q: the tile of the two-level sums and the points per thread (the tests' shapes)
_T, _Q = 256, 2
_FORWARD, _BACKWARD_POINTS, _BACKWARD_VERTICES = 0, 1, 2  # nr_winding_workspace_bytes' `which`
_INV_4PI = 1.0 / (4.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------------------
# plain torch: csrc/nr_solid_angle.h in its operation order

def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _cross(p, q):
    return torch.stack((p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                        p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]), -1)


def _nan_x(t, bad):
    """t [...,3] with x = NaN where `bad` [...]"""
    return torch.cat((torch.where(bad, torch.full_like(t[..., 0], float('nan')), t[..., 0])[..., None], t[..., 1:]), -1)


def _records_torch(vertices, faces):
    """-> (v0, v1, v2 [B,F,3], skip [B,F]): v0's x is NaN on a face with a non-finite corner; skip marks two equal corners"""
    f = faces.long()
    v0, v1, v2 = vertices[:, f[:, 0]], vertices[:, f[:, 1]], vertices[:, f[:, 2]]
    finite = (torch.isfinite(v0) & torch.isfinite(v1) & torch.isfinite(v2)).all(-1)
    skip = (v0 == v1).all(-1) | (v1 == v2).all(-1) | (v2 == v0).all(-1)
    return _nan_x(v0, ~finite), v1, v2, skip


def _points_torch(points):
    return _nan_x(points, ~torch.isfinite(points).all(-1))


def _pair_torch(p, v0, v1, v2):
    """The pair quantities for p [B,n,1,3] against corners [B,1,F,3]"""
    A, B, C = v0 - p, v1 - p, v2 - p
    la, lb, lc = torch.sqrt(_dot(A, A)), torch.sqrt(_dot(B, B)), torch.sqrt(_dot(C, C))
    num = _dot(A, _cross(B, C))
    ab, bc, ca = _dot(A, B), _dot(B, C), _dot(C, A)
    den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb
    return A, B, C, la, lb, lc, ab, bc, ca, num, den


def _inv_length(x):
    pos = x > 0
    return torch.where(pos, 1.0 / torch.where(pos, x, torch.ones_like(x)), torch.zeros_like(x))


def _gradient_torch(pair):
    """dOmega/dv0, dOmega/dv1, dOmega/dv2 [B,n,F,3] of the pairs"""
    A, B, C, la, lb, lc, ab, bc, ca, num, den = pair
    s = num * num + den * den
    zero = s == 0
    s1 = torch.where(zero, torch.ones_like(s), s)
    kn = torch.where(zero, torch.zeros_like(s), (2.0 * den) / s1)[..., None]
    kd = torch.where(zero, torch.zeros_like(s), (2.0 * num) / s1)[..., None]
    ila, ilb, ilc = _inv_length(la)[..., None], _inv_length(lb)[..., None], _inv_length(lc)[..., None]
    la, lb, lc = la[..., None], lb[..., None], lc[..., None]
    ma, mb, mc = lb * lc + bc[..., None], lc * la + ca[..., None], la * lb + ab[..., None]
    dA = ((A * ila) * ma + B * lc) + C * lb
    dB = ((B * ilb) * mb + C * la) + A * lc
    dC = ((C * ilc) * mc + A * lb) + B * la
    keep = ~zero[..., None]
    z = torch.zeros_like(dA)
    return (torch.where(keep, kn * _cross(B, C) - kd * dA, z), torch.where(keep, kn * _cross(C, A) - kd * dB, z),
            torch.where(keep, kn * _cross(A, B) - kd * dC, z))


@_util.once_differentiable
class _WindingTorch(torch.autograd.Function):
    """forward(ctx, points [B or 1,N,3], vertices [B,Nv,3], faces) -> w [B,N], in chunks of points; the sums in double"""

    @staticmethod
    def forward(ctx, points, vertices, faces):
        B, N, F = int(vertices.shape[0]), int(points.shape[1]), int(faces.shape[0])
        v0, v1, v2, skip = _records_torch(vertices, faces)
        p = _points_torch(points)
        step = max(1, _CHUNK_ELEMENTS // (B * F * 12))
        out = []
        for n0 in range(0, N, step):
            pair = _pair_torch(p[:, n0:n0 + step, None, :], v0[:, None], v1[:, None], v2[:, None])
            num, den = pair[-2], pair[-1]
            omega = torch.where((num == 0) & (den == 0), torch.zeros_like(num), 2.0 * torch.atan2(num, den))
            omega = torch.where(skip[:, None, :], torch.zeros_like(omega), omega)
            out.append((omega.double().sum(2) * _INV_4PI).to(vertices.dtype))
        ctx.save_for_backward(points, vertices, faces)
        return torch.cat(out, 1)

    @staticmethod
    def backward(ctx, grad_w):
        points, vertices, faces = ctx.saved_tensors
        B, N, F = int(vertices.shape[0]), int(points.shape[1]), int(faces.shape[0])
        v0, v1, v2, skip = _records_torch(vertices, faces)
        p = _points_torch(points)
        keep = ~skip[:, None, :, None]
        step = max(1, _CHUNK_ELEMENTS // (B * F * 48))
        grad_points, corners = [], torch.zeros((B, F, 3, 3), dtype=torch.float64, device=vertices.device)
        for n0 in range(0, N, step):
            g = _gradient_torch(_pair_torch(p[:, n0:n0 + step, None, :], v0[:, None], v1[:, None], v2[:, None]))
            g = [torch.where(keep, t, torch.zeros_like(t)) for t in g]
            gw = grad_w[:, n0:n0 + step]
            if ctx.needs_input_grad[0]:
                gp = (-((g[0] + g[1]) + g[2])).double().sum(2)
                grad_points.append(gp * (gw.double() * _INV_4PI)[..., None])
            if ctx.needs_input_grad[1]:
                for k in range(3):
                    corners[:, :, k] += (gw[:, :, None, None] * g[k]).double().sum(1)
        gp = gv = None
        if ctx.needs_input_grad[0]:
            gp = torch.cat(grad_points, 1)
            if points.shape[0] != B:
                gp = gp.sum(0, keepdim=True)
            gp = gp.to(points.dtype)
        if ctx.needs_input_grad[1]:
            gv = torch.zeros(vertices.shape, dtype=torch.float64, device=vertices.device)
            gv.index_add_(1, faces.long().reshape(-1), (corners * _INV_4PI).reshape(B, 3 * F, 3))
            gv = gv.to(vertices.dtype)
        return gp, gv, None


# ---------------------------------------------------------------------------------------------------------------------
# HIP

@_util.once_differentiable
class _Winding(torch.autograd.Function):
    """forward(ctx, points [B or 1,N,3], vertices [B,Nv,3], faces, split) -> w [B,N]"""

    @staticmethod
    def forward(ctx, points, vertices, faces, split):
        p, v = _lib.dense(points.detach()), _lib.dense(vertices.detach())
        dev = v.device
        B, Nv, N = int(v.shape[0]), int(v.shape[1]), int(p.shape[1])
        idx, adj_off, adj_ent, _ = _adjacency(faces, Nv)
        F = int(idx.shape[1])
        per_batch = 1 if int(p.shape[0]) == B else 0  # 0: one cloud [1,N,3] read in place by every image
        w = torch.empty((B, N), dtype=torch.float32, device=dev)
        _lib.launch('nr_winding_forward', dev, p.data_ptr(), v.data_ptr(), idx.data_ptr(), w.data_ptr(), B, N, Nv, F, per_batch, split,
                    workspace_bytes=_lib.workspace_bytes('nr_winding_workspace_bytes', B, N, F, _FORWARD, split))
        ctx.save_for_backward(p, v)
        ctx.tables, ctx.per_batch, ctx.split = (idx, adj_off, adj_ent), per_batch, split
        ctx.set_materialize_grads(False)
        return w

    @staticmethod
    def backward(ctx, grad_w):
        if grad_w is None:
            return None, None, None, None
        p, v = ctx.saved_tensors
        idx, adj_off, adj_ent = ctx.tables
        dev = v.device
        B, Nv, N, F = int(v.shape[0]), int(v.shape[1]), int(p.shape[1]), int(idx.shape[1])
        g = _lib.dense(grad_w.to(torch.float32))
        grad_points = grad_vertices = None
        if ctx.needs_input_grad[0]:  # (a shared cloud that requires a gradient never gets here: _NEEDS)
            grad_points = torch.empty_like(p)
            _lib.launch('nr_winding_backward_points', dev, p.data_ptr(), v.data_ptr(), idx.data_ptr(), g.data_ptr(),
                        grad_points.data_ptr(), B, N, Nv, F, ctx.split,
                        workspace_bytes=_lib.workspace_bytes('nr_winding_workspace_bytes', B, N, F, _BACKWARD_POINTS, ctx.split))
        if ctx.needs_input_grad[1]:
            grad_vertices = torch.empty_like(v)
            _lib.launch('nr_winding_backward_vertices', dev, p.data_ptr(), v.data_ptr(), idx.data_ptr(), adj_off.data_ptr(),
                        adj_ent.data_ptr(), g.data_ptr(), grad_vertices.data_ptr(), B, N, Nv, F, ctx.per_batch, ctx.split,
                        workspace_bytes=_lib.workspace_bytes('nr_winding_workspace_bytes', B, N, F, _BACKWARD_VERTICES, ctx.split))
        return grad_points, grad_vertices, None, None


# ---------------------------------------------------------------------------------------------------------------------
# public

def _winding(name, points, vertices, faces, implementation):
    """-> (w [B,N], squeeze)"""
    points, vertices, faces, squeeze, hip = _inputs(name, points, vertices, faces, implementation, _NEEDS)
    if hip:
        return _Winding.apply(points, vertices, faces, _SPLIT), squeeze
    return _WindingTorch.apply(points, vertices, faces), squeeze


def winding_number(points, vertices, faces, implementation=None):
    """-> w [B,N] ([N] when no input has a batch axis): the generalized winding number of the mesh at every point, 1 inside a
    closed outward-oriented mesh and 0 outside; once-differentiable in points and vertices.  On a face the value is not
    specified.  See the module docstring."""
    w, squeeze = _winding('winding_number', points, vertices, faces, implementation)
    return w[0] if squeeze else w


def mesh_occupancy(points, vertices, faces, threshold=0.5, implementation=None):
    """-> bool [B,N] ([N]): winding_number > threshold; no gradient."""
    threshold = _util.number('mesh_occupancy', 'threshold', threshold)
    with torch.no_grad():
        w, squeeze = _winding('mesh_occupancy', points, vertices, faces, implementation)
    w = w > threshold
    return w[0] if squeeze else w


def _bounds(name, bounds):
    """-> ((lo, hi),) * 3 of floats from a pair or three pairs"""
    try:
        pairs = [tuple(float(x) for x in b) for b in bounds] if hasattr(bounds[0], '__len__') else [tuple(float(x) for x in bounds)] * 3
    except (TypeError, ValueError, IndexError):
        pairs = []
    if len(pairs) != 3 or any(len(b) != 2 or not (math.isfinite(b[0]) and math.isfinite(b[1]) and b[0] < b[1]) for b in pairs):
        raise ValueError('%s: bounds must be a pair (lo, hi) with lo < hi, or three such pairs for x, y, z, got %r' % (name, bounds))
    return pairs


def _grid_size(name, grid_size):
    if isinstance(grid_size, bool) or not isinstance(grid_size, int) or grid_size < 1:
        raise ValueError('%s: grid_size must be a positive integer, got %r' % (name, grid_size))
    return grid_size


def voxel_centers(grid_size, bounds=(-1.0, 1.0), device=None, dtype=torch.float32):
    """-> [G^3,3]: the centres of a G x G x G grid over `bounds` (a pair, or three pairs for x, y, z); voxel [i,j,k] is row
    (i G + j) G + k and has its centre at lo + (i + 1/2, j + 1/2, k + 1/2) (hi - lo) / G, computed in float64 and rounded once."""
    G = _grid_size('voxel_centers', grid_size)
    axes = [lo + (torch.arange(G, dtype=torch.float64) + 0.5) * ((hi - lo) / G) for lo, hi in _bounds('voxel_centers', bounds)]
    grid = torch.stack(torch.meshgrid(*axes, indexing='ij'), -1).reshape(G ** 3, 3)
    return grid.to(device=device, dtype=dtype)


def voxelize(vertices, faces, grid_size, bounds=(-1.0, 1.0), hard=True, implementation=None):
    """-> [B,G,G,G] float32 ([G,G,G] for vertices [Nv,3]): the mesh on the grid of `voxel_centers`.  hard: 1 where the winding
    number of the centre is above 0.5, else 0, without a gradient; not hard: the winding number itself, differentiable in the
    vertices.  The centres are one cloud shared by the batch."""
    G = _grid_size('voxelize', grid_size)
    _bounds('voxelize', bounds)
    if not (torch.is_tensor(vertices) and vertices.is_floating_point()):
        raise ValueError('voxelize: vertices must be a float tensor [num of vertices, 3] or [batch size, num of vertices, 3]')
    centers = voxel_centers(G, bounds, vertices.device, vertices.dtype)
    if hard:
        with torch.no_grad():
            w, squeeze = _winding('voxelize', centers, vertices, faces, implementation)
            w = (w > 0.5).to(torch.float32)
    else:
        w, squeeze = _winding('voxelize', centers, vertices, faces, implementation)
        w = w.to(torch.float32)
    w = w.reshape(w.shape[0], G, G, G)
    return w[0] if squeeze else w


def voxel_iou(a, b, eps=1e-6):
    """-> [B] (0-dim for [G,G,G] grids): sum a b / (sum (a + b - a b) + eps) of two grids [B,G,G,G] of occupancies in [0,1]."""
    if not (torch.is_tensor(a) and torch.is_tensor(b) and a.is_floating_point() and b.is_floating_point() and a.shape == b.shape
            and a.dim() in (3, 4)):
        raise ValueError('voxel_iou: a and b must be float tensors of one shape [batch size, G, G, G] or [G, G, G]')
    eps = _util.number('voxel_iou', 'eps', eps)
    first = 0 if a.dim() == 3 else 1
    ab = a * b
    return ab.flatten(first).sum(-1) / ((a + b - ab).flatten(first).sum(-1) + eps)


def signed_distance(points, vertices, faces, implementation=None):
    """-> [B,N] ([N]): the distance of every point to the mesh (`closest_surface_points`), negative where the winding number is
    above 0.5.  The gradient goes through the distance only, and is 0 where the distance is 0."""
    _util.check_implementation('signed_distance', implementation)
    dist2 = closest_surface_points(points, vertices, faces, implementation)[0]
    with torch.no_grad():
        w, squeeze = _winding('signed_distance', points, vertices, faces, implementation)
        inside = w[0] > 0.5 if squeeze else w > 0.5
    zero = dist2 == 0  # (sqrt's own gradient there is infinite)
    d = torch.where(zero, torch.zeros_like(dist2), torch.sqrt(torch.where(zero, torch.ones_like(dist2), dist2)))
    return torch.where(inside, -d, d)
