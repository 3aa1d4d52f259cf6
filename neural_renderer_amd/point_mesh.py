"""Point-to-mesh distance (not in the reference's library): the term of a 3-D fit that compares a scan with the SURFACE of a
mesh, not with samples of it -- for every point the nearest triangle, for every triangle the nearest point.

`closest_surface_points(points, vertices, faces)` -> (dist2 [B,N], face_ids [B,N] int64, barycentric [B,N,3]):
dist2[b,i] = min_f min_{c in triangle f} |p_bi - c|^2, face_ids the LOWEST face among those whose computed dist2 is minimal,
barycentric the weights (w0, w1, w2 >= 0, summing to 1 within 4 ulp) of the closest point c = w0 v0 + w1 v1 + w2 v2 -- sorted
by face they are a `SurfaceSamples`.  `closest_cloud_points(points, vertices, faces)` -> (dist2 [B,F], point_ids [B,F] int64,
barycentric [B,F,3]): for every face the nearest point of the cloud (the lowest index on a tie) and the point of the face nearest
to it.  `point_mesh_distance(points, vertices, faces, direction, reduction)` -> [B]:
loss_b = wp sum_i dist2_points[b,i] + wf sum_f dist2_faces[b,f], wp, wf = 1/N, 1/F ('mean') or 1, 1 ('sum'); direction
'points_to_mesh' / 'mesh_to_points' keeps one term and launches only its kernels.  The sums are taken in double in a fixed
order and rounded once.

points [B,N,3], or [N,3] / [1,N,3] shared by the batch and read in place; vertices [B,Nv,3] or [Nv,3]; faces [F,3] integer, one
topology per call.  When no input has a batch axis the outputs have none.  dist2 and the loss are once-differentiable in
points and vertices; ids and weights carry no gradient.  The gradient is the exact derivative of the definition: by the
envelope theorem the weights need not be differentiated, so for a pair with r = p - sum_k w_k v_k it is d|r|^2/dp = 2 r and
d|r|^2/dv_k = -2 w_k r.

The closest point of a triangle is ONE definition (csrc/nr_point_triangle.h, restated in `_closest_torch`): the smallest of
the three edge segments, t = clamp(e.(p - u) / |e|^2, 0, 1) with t = 0 when |e|^2 = 0, and the projection onto the plane when
it lies inside -- not the textbook region walk, which returns a corner on a face with a repeated vertex.  On a face without
area it is exactly the distance to its segment or point, so a mesh under optimisation may collapse faces.  A pair whose
dist2 is NaN never wins, ids are always in range, and a row all of whose pairs are NaN reports id 0 and a non-finite dist2.

On float32 CUDA tensors (see `_NEEDS`) all of it runs as HIP kernels (nr_point_mesh_*, csrc/nr_point_mesh.hip): brute-force
sweeps with the streamed side in LDS, split over workgroups for small calls, gathers in a fixed order for the gradients --
no atomics, the same bits in every run and for an image alone or inside a batch.  The two orderings the gathers need are
device-side stable sorts; nothing is read back.  Everything else -- CPU, other dtypes, a shared `points` tensor that requires
a gradient -- takes the plain-torch path, a chunked sweep under no_grad and |r|^2 recomputed from the gathered vertices with
detached weights; it is also the kernels' second yardstick in the tests.

HIP graphs: nothing here was ever captured, and a captured point-loss step once crashed inside torch's capture_end for a
reason that is only supposed (README "Soft silhouettes").  The advice that holds for the soft operators holds here:
capture before any eager backward on the same leaves, or run the eager steps under no_grad; the index tensor's tables must
exist before a capture (call once eagerly)."""
import os

import torch

from . import _lib, _util
from .point_losses import _CHUNK_ELEMENTS, _mesh
from .vertex_colors import _adjacency

_NEEDS = ('the HIP kernels take float32 CUDA tensors with a batch size B of 65535 at most, B x points <= (2^31 - 1) / 3, B x faces '
          '<= (2^31 - 1) / 18, B x vertices <= (2^31 - 1) / 6, and a shared points tensor only when it requires no gradient')
# the number of parts the streamed side is cut into: 0 lets the library decide, n >= 1 forces n (1: none); the result does not
# depend on it (tests and scripts/point_mesh_timing.py set it)
_SPLIT = int(os.environ.get('NR_POINT_MESH_SPLIT', '0') or 0)
_DIRECTIONS = ('both', 'points_to_mesh', 'mesh_to_points')


# ---------------------------------------------------------------------------------------------------------------------
# checks

def _inputs(name, points, vertices, faces, implementation, needs=None):
    """-> (points [B or 1,N,3], vertices [B,Nv,3], faces [F,3], squeeze, use_hip); `needs`: the limit sentence of another module
    whose kernels take the same arguments (winding.py)"""
    if not (torch.is_tensor(points) and points.is_floating_point() and points.dim() in (2, 3) and points.shape[-1] == 3
            and points.shape[-2] >= 1 and points.shape[0] >= 1):
        raise ValueError('%s: points must be a float tensor [num of points, 3] or [batch size, num of points, 3] with at least '
                         'one point' % name)
    no_batch = points.dim() == 2 and torch.is_tensor(vertices) and vertices.dim() == 2
    vertices, faces, _ = _mesh(name, vertices, faces)
    if points.dtype != vertices.dtype or points.device != vertices.device:
        raise ValueError('%s: points and vertices must share dtype and device (%s %s, %s %s)'
                         % (name, points.dtype, points.device, vertices.dtype, vertices.device))
    if points.dim() == 2:
        points = points[None]
    Bp, Bv = int(points.shape[0]), int(vertices.shape[0])
    if Bp != Bv and Bp != 1 and Bv != 1:
        raise ValueError('%s: points have batch size %d, vertices %d' % (name, Bp, Bv))
    B = max(Bp, Bv)
    if Bv != B:
        vertices = vertices.expand(B, -1, -1)
    N, Nv, F = int(points.shape[1]), int(vertices.shape[1]), int(faces.shape[0])
    lim = 2 ** 31 - 1
    fits = (points.is_cuda and points.dtype == torch.float32 and B <= 65535 and B * N <= lim // 3 and B * F <= lim // 18
            and B * Nv <= lim // 6 and (Bp == B or not points.requires_grad or not torch.is_grad_enabled()))
    return points, vertices, faces, no_batch, _util.takes_hip(name, implementation, fits, needs or _NEEDS)


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _inv(x):
    pos = x > 0
    return torch.where(pos, 1.0 / torch.where(pos, x, torch.ones_like(x)), torch.zeros_like(x))


def _clamp01(t):
    t = torch.where(t > 0, t, torch.zeros_like(t))  # (0 for a NaN, as fminf(fmaxf(t, 0), 1))
    return torch.where(t < 1, t, torch.ones_like(t))


def _records_torch(v0, v1, v2):
    """The per-face invariants of csrc/nr_point_triangle.h for corners [..., 3], in its operation order."""
    ab, ac, e = v1 - v0, v2 - v0, v2 - v1
    bb = _dot(ab, ac)
    iaa = _inv(_dot(ab, ab))
    g = ac - (bb * iaa)[..., None] * ab
    finite = (torch.isfinite(v0) & torch.isfinite(v1) & torch.isfinite(v2)).all(-1)
    a = torch.where(finite[..., None], v0, torch.full_like(v0, float('nan')))  # a face with a non-finite corner: NaN pairs
    return a, ab, ac, e, g, iaa, _inv(_dot(ac, ac)), _inv(_dot(e, e)), _inv(_dot(g, g)), bb


def _closest_torch(p, rec, weights):
    """dist2 of the points p [..., 3] to the faces of `rec` (broadcast against each other), and with `weights` the barycentric
    weights [..., 3] of the closest points: the four candidates of csrc/nr_point_triangle.h compared with a strict < in the
    order ab, ac, bc, plane."""
    a, ab, ac, e, g, iaa, icc, iee, igg, bb = rec
    ap = p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    t1 = _clamp01(d1 * iaa)
    r = ap - t1[..., None] * ab
    best = _dot(r, r)
    t2 = _clamp01(d2 * icc)
    r = ap - t2[..., None] * ac
    s2 = _dot(r, r)
    bp = ap - ab
    t3 = _clamp01(_dot(e, bp) * iee)
    r = bp - t3[..., None] * e
    s3 = _dot(r, r)
    y = _dot(g, ap) * igg
    x = (d1 - y * bb) * iaa
    r = (ap - x[..., None] * ab) - y[..., None] * ac
    s4 = _dot(r, r)
    inside = (x >= 0) & (y >= 0) & (x + y <= 1)
    take2 = s2 < best
    best = torch.where(take2, s2, best)
    take3 = s3 < best
    best = torch.where(take3, s3, best)
    take4 = inside & (s4 < best)
    best = torch.where(take4, s4, best)
    if not weights:
        return best, None
    zero = torch.zeros_like(best)
    w = torch.stack((1 - t1, t1 + zero, zero), -1)
    w = torch.where(take2[..., None], torch.stack((1 - t2, zero, t2 + zero), -1), w)
    w = torch.where(take3[..., None], torch.stack((zero, 1 - t3, t3 + zero), -1), w)
    w0 = (1 - x) - y
    w = torch.where(take4[..., None], torch.stack((torch.where(w0 > 0, w0, zero), x + zero, y + zero), -1), w)
    return best, w


def _corners(vertices, faces):
    f = faces.long()
    return vertices[:, f[:, 0]], vertices[:, f[:, 1]], vertices[:, f[:, 2]]  # [B,F,3] each


def _argmin(d, dim):
    """the first index of the minimum along `dim`; a NaN never wins"""
    return torch.min(torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d), dim=dim)[1]


def _search_torch(points, vertices, faces, to_points):
    """ids [B,N] (the nearest face of every point) or [B,F] (to_points: the nearest point of every face), in chunks"""
    B, N, F = int(vertices.shape[0]), int(points.shape[1]), int(faces.shape[0])
    out = []
    with torch.no_grad():
        rec = _records_torch(*_corners(vertices.detach(), faces))
        p = points.detach()
        if to_points:
            step = max(1, _CHUNK_ELEMENTS // (B * N * 3))
            for f0 in range(0, F, step):
                part = tuple(t[:, f0:f0 + step, None] for t in rec)
                out.append(_argmin(_closest_torch(p[:, None, :, :], part, False)[0], 2))
        else:
            step = max(1, _CHUNK_ELEMENTS // (B * F * 3))
            whole = tuple(t[:, None] for t in rec)
            for n0 in range(0, N, step):
                out.append(_argmin(_closest_torch(p[:, n0:n0 + step, None, :], whole, False)[0], 2))
    return torch.cat(out, 1)


def _pairs_torch(points, vertices, faces, point_of, face_of):
    """(dist2, weights) of the pairs (points[b, point_of], face face_of) -- None: the row's own number.  The weights come from
    the definition under no_grad, and so does r = ((p - v0) - w1 (v1 - v0)) - w2 (v2 - v0), whose error is relative to the
    triangle's size, not to the coordinates.  dist2 = |r|^2 + 2 r . ((p - [p]) - sum_k w_k (v_k - [v_k])), [.] detached: the
    second term is exactly 0 and hands autograd both gradients of the definition, 2 r and -2 w_k r, with the weights that are
    returned (differentiating the r above instead would give corner 0 the weight 1 - w1 - w2 by cancellation)."""
    B = int(vertices.shape[0])
    rows = torch.arange(B, device=vertices.device)[:, None]
    corners = faces.long() if face_of is None else faces.long()[face_of]  # [F,3] | [B,N,3]
    v0, v1, v2 = (vertices[rows, corners[..., k]] if corners.dim() == 3 else vertices[:, corners[:, k]] for k in range(3))
    p = points if point_of is None else (points[0][point_of] if points.shape[0] == 1 else points[rows, point_of])
    pd, v0d, v1d, v2d = p.detach(), v0.detach(), v1.detach(), v2.detach()
    with torch.no_grad():
        w = _closest_torch(pd, _records_torch(v0d, v1d, v2d), True)[1]
        r = ((pd - v0d) - w[..., 1:2] * (v1d - v0d)) - w[..., 2:3] * (v2d - v0d)
        dist2 = _dot(r, r)
    if torch.is_grad_enabled() and (p.requires_grad or vertices.requires_grad):
        lin = (p - pd) - ((w[..., 0:1] * (v0 - v0d) + w[..., 1:2] * (v1 - v1d)) + w[..., 2:3] * (v2 - v2d))
        dist2 = dist2 + 2 * _dot(r, lin)
    return dist2, w


def _surface_torch(points, vertices, faces):
    ids = _search_torch(points, vertices, faces, False)
    dist2, w = _pairs_torch(points, vertices, faces, None, ids)
    return dist2, ids, w


def _cloud_torch(points, vertices, faces):
    ids = _search_torch(points, vertices, faces, True)
    dist2, w = _pairs_torch(points, vertices, faces, ids, None)
    return dist2, ids, w


# ---------------------------------------------------------------------------------------------------------------------
# HIP

def _sorted_by(ids, count):
    """(order [B,n] int32: the row numbers sorted by id, stable; offsets [B,count+1] int32), on the device"""
    sorted_ids, order = torch.sort(ids, dim=1, stable=True)
    bounds = torch.arange(count + 1, device=ids.device, dtype=ids.dtype)[None].expand(ids.shape[0], -1).contiguous()
    return order.to(torch.int32), torch.searchsorted(sorted_ids.contiguous(), bounds).to(torch.int32)


@_util.once_differentiable
class _PointMesh(torch.autograd.Function):
    """forward(ctx, points [B or 1,N,3], vertices [B,Nv,3], faces, to_faces, to_points, split) -> (dist2_points [B,N],
    face_ids int32, barycentric_points, dist2_faces [B,F], point_ids int32, barycentric_faces); a direction that is not
    asked for gives three None."""

    @staticmethod
    def forward(ctx, points, vertices, faces, to_faces, to_points, split):
        p, v = _lib.dense(points.detach()), _lib.dense(vertices.detach())
        dev = v.device
        B, Nv, N = int(v.shape[0]), int(v.shape[1]), int(p.shape[1])
        idx, adj_off, adj_ent, _ = _adjacency(faces, Nv)
        F = int(idx.shape[1])
        per_batch = 1 if int(p.shape[0]) == B else 0  # 0: one cloud [1,N,3] read in place by every image
        out = []
        for wanted, name, rows, flag in ((to_faces, 'nr_point_mesh_points_to_faces', N, 0),
                                         (to_points, 'nr_point_mesh_faces_to_points', F, 1)):
            if not wanted:
                out += [None, None, None]
                continue
            dist2 = torch.empty((B, rows), dtype=torch.float32, device=dev)
            ids = torch.empty((B, rows), dtype=torch.int32, device=dev)
            bary = torch.empty((B, rows, 3), dtype=torch.float32, device=dev)
            _lib.launch(name, dev, p.data_ptr(), v.data_ptr(), idx.data_ptr(), dist2.data_ptr(), ids.data_ptr(), bary.data_ptr(),
                        B, N, Nv, F, per_batch, split,
                        workspace_bytes=_lib.workspace_bytes('nr_point_mesh_workspace_bytes', B, N, F, flag, split))
            out += [dist2, ids, bary]
        ctx.save_for_backward(p, v, out[1], out[2], out[4], out[5])
        ctx.tables, ctx.per_batch = (idx, adj_off, adj_ent), per_batch
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (out[1], out[2], out[4], out[5]) if t is not None))
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_p, _1, _2, grad_f, _3, _4):
        p, v, face_ids, bary_p, point_ids, bary_f = ctx.saved_tensors
        idx, adj_off, adj_ent = ctx.tables
        dev = v.device
        B, Nv, N, F = int(v.shape[0]), int(v.shape[1]), int(p.shape[1]), int(idx.shape[1])
        grad_p = _lib.dense(grad_p.to(torch.float32)) if grad_p is not None and face_ids is not None else None
        grad_f = _lib.dense(grad_f.to(torch.float32)) if grad_f is not None and point_ids is not None else None
        if grad_p is None:
            face_ids = bary_p = None
        if grad_f is None:
            point_ids = bary_f = None
        grad_points = grad_vertices = None
        if grad_p is None and grad_f is None:
            return None, None, None, None, None, None
        ptr = _lib.ptr
        if ctx.needs_input_grad[0]:
            order_f, off_p = _sorted_by(point_ids, N) if point_ids is not None else (None, None)
            grad_points = torch.empty_like(p)
            _lib.launch('nr_point_mesh_backward_points', dev, p.data_ptr(), v.data_ptr(), idx.data_ptr(), ptr(face_ids), ptr(bary_p),
                        ptr(grad_p), ptr(point_ids), ptr(bary_f), ptr(grad_f), ptr(order_f), ptr(off_p), grad_points.data_ptr(),
                        B, N, Nv, F)
        if ctx.needs_input_grad[1]:
            order_p, off_f = _sorted_by(face_ids, F) if face_ids is not None else (None, None)
            grad_vertices = torch.empty_like(v)
            _lib.launch('nr_point_mesh_backward_vertices', dev, p.data_ptr(), v.data_ptr(), idx.data_ptr(), adj_off.data_ptr(),
                        adj_ent.data_ptr(), ptr(face_ids), ptr(bary_p), ptr(grad_p), ptr(order_p), ptr(off_f), ptr(point_ids),
                        ptr(bary_f), ptr(grad_f), grad_vertices.data_ptr(), B, N, Nv, F, ctx.per_batch)
        return grad_points, grad_vertices, None, None, None, None


@_util.once_differentiable
class _LossSum(torch.autograd.Function):
    """forward(ctx, dist2_points [B,N] or None, dist2_faces [B,F] or None, wp, wf) -> loss [B]"""

    @staticmethod
    def forward(ctx, dist2_points, dist2_faces, wp, wf):
        dp, df = _lib.dense(dist2_points), _lib.dense(dist2_faces)
        some = dp if dp is not None else df
        B = int(some.shape[0])
        N, F = (int(dp.shape[1]) if dp is not None else 1), (int(df.shape[1]) if df is not None else 1)
        loss = torch.empty((B,), dtype=torch.float32, device=some.device)
        _lib.launch('nr_point_mesh_loss', some.device, _lib.ptr(dp), _lib.ptr(df), loss.data_ptr(), B, N, F, wp, wf)
        ctx.sizes = (B, N, F, wp, wf, dp is not None, df is not None)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        B, N, F, wp, wf, has_p, has_f = ctx.sizes
        g_p = (grad_loss * wp)[:, None].expand(B, N) if has_p and ctx.needs_input_grad[0] else None
        g_f = (grad_loss * wf)[:, None].expand(B, F) if has_f and ctx.needs_input_grad[1] else None
        return g_p, g_f, None, None


# ---------------------------------------------------------------------------------------------------------------------
# public

def closest_surface_points(points, vertices, faces, implementation=None):
    """-> (dist2 [B,N], face_ids [B,N] int64, barycentric [B,N,3]): for every point its squared distance to the mesh, the
    nearest face (the lowest on a tie) and the weights of the closest point on it ([N], [N], [N,3] when no input has a batch
    axis).  dist2 is differentiable in points and vertices.  See the module docstring."""
    points, vertices, faces, squeeze, hip = _inputs('closest_surface_points', points, vertices, faces, implementation)
    if hip:
        dist2, ids, w = _PointMesh.apply(points, vertices, faces, True, False, _SPLIT)[:3]
        ids = ids.long()
    else:
        dist2, ids, w = _surface_torch(points, vertices, faces)
    return (dist2[0], ids[0], w[0]) if squeeze else (dist2, ids, w)


def closest_cloud_points(points, vertices, faces, implementation=None):
    """-> (dist2 [B,F], point_ids [B,F] int64, barycentric [B,F,3]): for every face the nearest point of the cloud (the
    lowest index on a tie), its squared distance and the weights of the point of the face nearest to it.  dist2 is
    differentiable in points and vertices.  See the module docstring."""
    points, vertices, faces, squeeze, hip = _inputs('closest_cloud_points', points, vertices, faces, implementation)
    if hip:
        dist2, ids, w = _PointMesh.apply(points, vertices, faces, False, True, _SPLIT)[3:]
        ids = ids.long()
    else:
        dist2, ids, w = _cloud_torch(points, vertices, faces)
    return (dist2[0], ids[0], w[0]) if squeeze else (dist2, ids, w)


def point_mesh_distance(points, vertices, faces, direction='both', reduction='mean', implementation=None):
    """The point-to-mesh distance of a cloud and a mesh: [B], a 0-dim tensor when no input has a batch axis.  direction
    'both' | 'points_to_mesh' | 'mesh_to_points'; reduction 'mean' | 'sum'.  Differentiable in points and vertices.  See the
    module docstring."""
    name = 'point_mesh_distance'
    if direction not in _DIRECTIONS:
        raise ValueError("%s: direction must be 'both', 'points_to_mesh' or 'mesh_to_points'" % name)
    if reduction not in ('mean', 'sum'):
        raise ValueError("%s: reduction must be 'mean' or 'sum'" % name)
    points, vertices, faces, squeeze, hip = _inputs(name, points, vertices, faces, implementation)
    N, F = int(points.shape[1]), int(faces.shape[0])
    wp, wf = (1.0 / N, 1.0 / F) if reduction == 'mean' else (1.0, 1.0)
    to_faces, to_points = direction != 'mesh_to_points', direction != 'points_to_mesh'
    if hip:
        out = _PointMesh.apply(points, vertices, faces, to_faces, to_points, _SPLIT)
        loss = _LossSum.apply(out[0], out[3], wp, wf)
    else:
        loss = None
        if to_faces:
            loss = _surface_torch(points, vertices, faces)[0].double().sum(1) * wp
        if to_points:
            term = _cloud_torch(points, vertices, faces)[0].double().sum(1) * wf
            loss = term if loss is None else loss + term
        loss = loss.to(vertices.dtype)
    return loss[0] if squeeze else loss
