"""Ray casting (not in the reference's library): what a ray hits first on a mesh and how far away -- the third geometric query
next to `closest_surface_points` (where is the nearest surface) and `winding_number` (is a point inside) -- for fitting range
scans along their lines of sight, for visibility, and for shadow and occlusion tests.

`ray_mesh_intersect(origins, directions, vertices, faces, near=0.0, far=inf, cull_backfaces=False)` -> (t [B,R], face_ids [B,R]
int64, barycentric [B,R,3]): the first hit of every ray o + t d on the mesh.  d is NOT normalised, so t counts in lengths of d
(a segment from a to b is o = a, d = b - a, near = 0, far = 1).  A miss reports t = +inf, face_id = -1 and weights 0.
`ray_mesh_occluded(origins, directions, vertices, faces, near=0.0, far=inf)` -> bool [B,R]: whether the ray hits anything.
`vertex_visibility(vertices, faces, eye, eps=1e-4)` -> bool [B,Nv]: whether the segment from each vertex to `eye` ([3] or [B,3]) is
free, d = eye - v and t in [eps, 1).  `camera_rays(renderer, batch_size, like, image_size=None)` -> (origins [B,3], directions
[B,S*S,3]): the rays through the rasterizer's pixel centres, for which t IS the camera depth of `Renderer.render_depth`.

Whether a ray hits a face is ONE definition (csrc/nr_ray_triangle.h, restated in `_pair_torch` and in tests/ray_ref.py).  With
e1 = v1 - v0, e2 = v2 - v0, pvec = d x e2, det = e1 . pvec, tvec = o - v0, qvec = tvec x e1, s = sign(det), D = |det|,
U = s (tvec . pvec), V = s (d . qvec), T = s (e2 . qvec):  a hit iff D > 0, U >= 0, V >= 0, U + V <= D -- on the undivided
numerators --, with `cull_backfaces` det > 0 (the ray arrives against n = e1 x e2, on the side from which v0, v1, v2 run
counter-clockwise), and near <= t < far for t = T / D.  The weights are w1 = U / D, w2 = V / D, w0 = max((1 - w1) - w2, 0).
The first hit is the smallest t under a strict < over ascending face numbers: the lowest face wins a tie.  A NaN never wins, so a NaN ray
misses and a face with a non-finite corner is never hit; a collapsed face, or one parallel to the ray, has D = 0 and is never hit
either.  Shared edges are NOT watertight: the two faces of an edge round U, V and D independently, so a ray through the edge
itself may hit both faces or, rarely, neither.

origins and directions [B,R,3], or [R,3] / [1,R,3] shared by the batch and read in place; an origin [3], or [B,3] next to
directions [B,R,3], is one origin for all rays (of an image).  vertices [B,Nv,3] or [Nv,3]; faces [F,3] integer, one topology per
call.  When no input has a batch axis the outputs have none.

Gradients.  t is differentiable in origins, directions and vertices, any number of times: the search -- R x F pairs -- runs
under no_grad, and t is rebuilt from the R gathered corners of the hit faces in plain torch, t_d = ((v0 - o) . n) / (d . n),
n = e1 x e2, and returned as t_kernel + (t_d - t_d.detach()): the value is the search's, the derivative the plane's.  Miss rows
are computed on substituted harmless inputs and hand exact zeros to every input.  face_ids and the weights carry no
gradient.  There is no torch.autograd.Function here, so a second derivative simply works.  The gradient to the vertices goes
through torch's indexing backward, which adds the rays of a vertex in torch's order.

On float32 CUDA tensors (see `_NEEDS`) the search runs as HIP kernels (nr_ray_mesh_*, csrc/nr_ray_mesh.hip): a brute-force
sweep with the faces streamed through LDS, split over workgroups for small calls -- no atomics, the same bits in every run,
for an image alone or inside a batch, split or not.  Everything else -- CPU, other dtypes -- takes the plain-torch path, a
chunked sweep of the same definition in the same operation order; it is also the kernels' second yardstick in the tests.

HIP graphs: nothing here was ever captured."""
import math
import os

import torch

from . import _lib, _util
from .point_losses import _CHUNK_ELEMENTS, _mesh
from .vertex_colors import _adjacency

_NEEDS = ('the HIP kernels take float32 CUDA tensors with a batch size B of 65535 at most, B x rays <= (2^31 - 1) / 3, B x faces '
          '<= (2^31 - 1) / 18 and B x vertices <= (2^31 - 1) / 6')
# the number of parts the faces are cut into: 0 lets the library decide, n >= 1 forces n (1: none); the result does not
# depend on it (tests and scripts/ray_mesh_timing.py set it)
_SPLIT = int(os.environ.get('NR_RAY_MESH_SPLIT', '0') or 0)


# ---------------------------------------------------------------------------------------------------------------------
# checks

def _rays(name, origins, directions):
    """-> (origins, directions) as [Br,R,3] views broadcast against each other (Br = 1: shared by the batch), and whether
    neither had a batch axis"""
    if not (torch.is_tensor(directions) and directions.is_floating_point() and directions.dim() in (2, 3)
            and directions.shape[-1] == 3 and directions.shape[-2] >= 1 and directions.shape[0] >= 1):
        raise ValueError('%s: directions must be a float tensor [num of rays, 3] or [batch size, num of rays, 3] with at least '
                         'one ray' % name)
    if not (torch.is_tensor(origins) and origins.is_floating_point() and origins.dim() in (1, 2, 3) and origins.shape[-1] == 3
            and origins.numel() >= 3):
        raise ValueError('%s: origins must be a float tensor shaped like directions, or one origin [3] or [batch size, 3]' % name)
    if origins.dtype != directions.dtype or origins.device != directions.device:
        raise ValueError('%s: origins and directions must share dtype and device (%s %s, %s %s)'
                         % (name, origins.dtype, origins.device, directions.dtype, directions.device))
    no_batch = directions.dim() == 2 and origins.dim() <= 2
    d = directions[None] if directions.dim() == 2 else directions
    R = int(d.shape[1])
    if origins.dim() == 1:
        o = origins[None, None]
    elif origins.dim() == 2 and directions.dim() == 3:
        o = origins[:, None]            # [B,3]: one origin per image
    elif origins.dim() == 2:
        o = origins[None]               # [R,3] next to [R,3]
    else:
        o = origins
    if o.shape[1] not in (1, R):
        raise ValueError('%s: origins %s do not match directions %s' % (name, tuple(origins.shape), tuple(directions.shape)))
    Bo, Bd = int(o.shape[0]), int(d.shape[0])
    if Bo != Bd and Bo != 1 and Bd != 1:
        raise ValueError('%s: origins have batch size %d, directions %d' % (name, Bo, Bd))
    Br = max(Bo, Bd)
    return o.expand(Br, R, 3), d.expand(Br, R, 3), no_batch


def _inputs(name, origins, directions, vertices, faces, near, far, implementation):
    """-> (origins, directions [Br,R,3] views, vertices [B,Nv,3], faces [F,3], near, far, squeeze, use_hip)"""
    _util.check_implementation(name, implementation)
    o, d, no_batch = _rays(name, origins, directions)
    no_batch = no_batch and torch.is_tensor(vertices) and vertices.dim() == 2
    vertices, faces, _ = _mesh(name, vertices, faces)
    if d.dtype != vertices.dtype or d.device != vertices.device:
        raise ValueError('%s: rays and vertices must share dtype and device (%s %s, %s %s)'
                         % (name, d.dtype, d.device, vertices.dtype, vertices.device))
    near, far = _util.number(name, 'near', near), _util.number(name, 'far', far)
    Br, Bv = int(d.shape[0]), int(vertices.shape[0])
    if Br != Bv and Br != 1 and Bv != 1:
        raise ValueError('%s: rays have batch size %d, vertices %d' % (name, Br, Bv))
    B = max(Br, Bv)
    if Bv != B:
        vertices = vertices.expand(B, -1, -1)
    R, Nv, F = int(d.shape[1]), int(vertices.shape[1]), int(faces.shape[0])
    lim = 2 ** 31 - 1
    fits = (d.is_cuda and d.dtype == torch.float32 and B <= 65535 and B * R <= lim // 3 and B * F <= lim // 18
            and B * Nv <= lim // 6)
    return o, d, vertices, faces, near, far, no_batch, _util.takes_hip(name, implementation, fits, _NEEDS)


# ---------------------------------------------------------------------------------------------------------------------
# plain torch: csrc/nr_ray_triangle.h in its operation order

def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _cross(p, q):
    return torch.stack((p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                        p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]), -1)


def _records_torch(vertices, faces):
    """-> (v0, e1, e2) [B,F,3]; v0's x is NaN on a face with a non-finite corner"""
    f = faces.long()
    v0, v1, v2 = vertices[:, f[:, 0]], vertices[:, f[:, 1]], vertices[:, f[:, 2]]
    finite = (torch.isfinite(v0) & torch.isfinite(v1) & torch.isfinite(v2)).all(-1)
    x = torch.where(finite, v0[..., 0], torch.full_like(v0[..., 0], float('nan')))
    return torch.cat((x[..., None], v0[..., 1:]), -1), v1 - v0, v2 - v0


def _pair_torch(o, d, v0, e1, e2, near, far, cull, weights=False):
    """t of the pairs (broadcast against each other; +inf where the pair is no hit within [near, far)), and with `weights`
    the barycentric weights (0 on a miss)"""
    pvec = _cross(d, e2)
    det = _dot(e1, pvec)
    tvec = o - v0
    qvec = _cross(tvec, e1)
    neg = det < 0
    D = det.abs()
    u, v, tt = _dot(tvec, pvec), _dot(d, qvec), _dot(e2, qvec)
    U, V, T = torch.where(neg, -u, u), torch.where(neg, -v, v), torch.where(neg, -tt, tt)
    inside = (D > 0) & (U >= 0) & (V >= 0) & (U + V <= D)
    if cull:
        inside = inside & ~neg
    D1 = torch.where(inside, D, torch.ones_like(D))
    t = T / D1
    hit = inside & (t >= near) & (t < far)
    t = torch.where(hit, t, torch.full_like(t, float('inf')))
    if not weights:
        return t, None
    zero = torch.zeros_like(t)
    w1, w2 = torch.where(hit, U / D1, zero), torch.where(hit, V / D1, zero)
    w0 = (1 - w1) - w2
    w0 = torch.where(hit & (w0 > 0), w0, zero)
    return t, torch.stack((w0, w1, w2), -1)


def _search_torch(o, d, vertices, faces, near, far, cull, any_hit):
    """ids [B,R] int64 (-1: a miss) of the first hits, or with any_hit bool [B,R]; a chunked sweep under no_grad"""
    B, R, F = int(vertices.shape[0]), int(d.shape[1]), int(faces.shape[0])
    out = []
    with torch.no_grad():
        v0, e1, e2 = (t[:, None] for t in _records_torch(vertices.detach(), faces))
        o, d = o.detach(), d.detach()
        step = max(1, _CHUNK_ELEMENTS // (B * F * 12))
        for r0 in range(0, R, step):
            t = _pair_torch(o[:, r0:r0 + step, None, :], d[:, r0:r0 + step, None, :], v0, e1, e2, near, far, cull)[0]
            best, ids = torch.min(t, dim=2)  # (the first index of the minimum; a miss is +inf, never NaN)
            hit = best < float('inf')
            out.append(hit if any_hit else torch.where(hit, ids, torch.full_like(ids, -1)))
    return torch.cat(out, 1)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

def _search_hip(o, d, vertices, faces, near, far, cull, any_hit):
    """The kernels' outputs: (t [B,R], ids [B,R] int64, weights [B,R,3]), or with any_hit bool [B,R]"""
    with torch.no_grad():
        o, d, v = _lib.dense(o.detach()), _lib.dense(d.detach()), _lib.dense(vertices.detach())
        dev = v.device
        B, Nv, R = int(v.shape[0]), int(v.shape[1]), int(d.shape[1])
        idx = _adjacency(faces, Nv)[0]
        F = int(idx.shape[1])
        per_batch = 1 if int(d.shape[0]) == B else 0  # 0: one bundle [1,R,3] read in place by every image
        ws = _lib.workspace_bytes('nr_ray_mesh_workspace_bytes', B, R, F, 1 if any_hit else 0, _SPLIT)
        if any_hit:
            occluded = torch.empty((B, R), dtype=torch.bool, device=dev)
            _lib.launch('nr_ray_mesh_any_hit', dev, o.data_ptr(), d.data_ptr(), v.data_ptr(), idx.data_ptr(), occluded.data_ptr(),
                        B, R, Nv, F, per_batch, near, far, 1 if cull else 0, _SPLIT, workspace_bytes=ws)
            return occluded
        t = torch.empty((B, R), dtype=torch.float32, device=dev)
        ids = torch.empty((B, R), dtype=torch.int32, device=dev)
        w = torch.empty((B, R, 3), dtype=torch.float32, device=dev)
        _lib.launch('nr_ray_mesh_first_hit', dev, o.data_ptr(), d.data_ptr(), v.data_ptr(), idx.data_ptr(), t.data_ptr(),
                    ids.data_ptr(), w.data_ptr(), B, R, Nv, F, per_batch, near, far, 1 if cull else 0, _SPLIT, workspace_bytes=ws)
        return t, ids.long(), w


# ---------------------------------------------------------------------------------------------------------------------
# the differentiable tail

_HARMLESS = {}  # (device, dtype) -> [5,3]: the origin, direction and corners a miss row is computed on


def _harmless(like):
    """a unit ray towards a unit triangle: o, d, v0, v1, v2 (made once per device and dtype: no copy from the host per call)"""
    key = (like.device, like.dtype)
    hit = _HARMLESS.get(key)
    if hit is None:
        hit = torch.tensor(((0, 0, 0), (0, 0, 1), (0, 0, 1), (1, 0, 1), (0, 1, 1)), dtype=like.dtype, device=like.device)
        if not torch.is_inference_mode_enabled():  # (a tensor made in inference mode cannot enter a later graph: not kept)
            _HARMLESS[key] = hit
    return hit


def _gather(o, d, vertices, faces, ids):
    """-> (hit [B,R], o, d, v0, v1, v2 [B,R,3]) of the pairs (ray, face ids); miss rows on substituted harmless inputs.  The
    tail is bound by its number of small launches, so the five vectors of a pair travel as one [B,R,5,3] tensor: one gather of
    the corners, one `where`."""
    B, R = int(vertices.shape[0]), int(ids.shape[1])
    hit = ids >= 0
    corners = faces.long()[ids.clamp(min=0)]                                    # [B,R,3]
    rows = torch.arange(B, device=vertices.device)[:, None, None]
    pairs = torch.cat((o.expand(B, R, 3)[:, :, None], d.expand(B, R, 3)[:, :, None], vertices[rows, corners]), 2)
    pairs = torch.where(hit[..., None, None], pairs, _harmless(vertices))
    return (hit,) + pairs.unbind(2)


def _finish(o, d, vertices, faces, ids, t=None, w=None, near=0.0, far=math.inf, cull=False):
    """(t, weights) of the first hits `ids`: the search's own values when given (HIP), else the definition's on the gathered
    pairs; t with the plane's derivative when an input requires a gradient"""
    differentiable = torch.is_grad_enabled() and (o.requires_grad or d.requires_grad or vertices.requires_grad)
    if t is not None and not differentiable:
        return t, w
    hit, og, dg, v0, v1, v2 = _gather(o, d, vertices, faces, ids)
    if t is None:
        with torch.no_grad():
            t, w = _pair_torch(og, dg, v0, v1 - v0, v2 - v0, near, far, cull, True)
            inf = torch.full_like(t, float('inf'))
            t, w = torch.where(hit, t, inf), torch.where(hit[..., None], w, torch.zeros_like(w))
    if differentiable:
        n = torch.linalg.cross(v1 - v0, v2 - v0)   # (the value is the search's; this chain is here for its derivative)
        t_d = ((v0 - og) * n).sum(-1) / (dg * n).sum(-1)
        t_d = torch.where(hit, t_d, torch.zeros_like(t_d))
        t = t + (t_d - t_d.detach())
    return t, w


# ---------------------------------------------------------------------------------------------------------------------
# public

def ray_mesh_intersect(origins, directions, vertices, faces, near=0.0, far=math.inf, cull_backfaces=False, implementation=None):
    """-> (t [B,R], face_ids [B,R] int64, barycentric [B,R,3]): the first hit of every ray o + t d with near <= t < far -- the
    smallest t, the lowest face on a tie --, the face and the weights of the hit point ([R], [R], [R,3] when no input has a batch
    axis); a miss gives +inf, -1 and zeros.  t is differentiable in origins, directions and vertices.  See the module
    docstring."""
    name = 'ray_mesh_intersect'
    o, d, vertices, faces, near, far, squeeze, hip = _inputs(name, origins, directions, vertices, faces, near, far, implementation)
    cull = bool(cull_backfaces)
    if hip:
        t, ids, w = _search_hip(o, d, vertices, faces, near, far, cull, False)
        t, w = _finish(o, d, vertices, faces, ids, t, w)
    else:
        ids = _search_torch(o, d, vertices, faces, near, far, cull, False)
        t, w = _finish(o, d, vertices, faces, ids, None, None, near, far, cull)
    return (t[0], ids[0], w[0]) if squeeze else (t, ids, w)


def ray_mesh_occluded(origins, directions, vertices, faces, near=0.0, far=math.inf, implementation=None):
    """-> bool [B,R] ([R]): whether the ray o + t d hits any face with near <= t < far; no gradient.  On the device a workgroup
    stops as soon as all its rays are occluded.  See the module docstring."""
    name = 'ray_mesh_occluded'
    o, d, vertices, faces, near, far, squeeze, hip = _inputs(name, origins, directions, vertices, faces, near, far, implementation)
    occluded = (_search_hip if hip else _search_torch)(o, d, vertices, faces, near, far, False, True)
    return occluded[0] if squeeze else occluded


def vertex_visibility(vertices, faces, eye, eps=1e-4, implementation=None):
    """-> bool [B,Nv] ([Nv] for vertices [Nv,3] and eye [3]): whether the segment from each vertex to `eye` ([3] or [B,3]) meets no
    face, with d = eye - v and t in [eps, 1): `eps`, a fraction of the segment, keeps the vertex's own faces from hiding it.  No
    gradient."""
    name = 'vertex_visibility'
    eps = _util.number(name, 'eps', eps)
    if not (torch.is_tensor(vertices) and vertices.is_floating_point() and vertices.dim() in (2, 3) and vertices.shape[-1] == 3):
        raise ValueError('%s: vertices must be a float tensor [num of vertices, 3] or [batch size, num of vertices, 3]' % name)
    eye = _util.as_tensor_like(eye, vertices, vertices.dtype)
    if not (eye.dim() in (1, 2) and eye.shape[-1] == 3):
        raise ValueError('%s: eye must be [3] or [batch size, 3]' % name)
    with torch.no_grad():
        v = vertices.detach()
        if eye.dim() == 2 and v.dim() == 2:
            v = v[None].expand(eye.shape[0], -1, -1)
        d = (eye.detach()[:, None] if eye.dim() == 2 else eye.detach()) - v
        return ~ray_mesh_occluded(v, d, v, faces, eps, 1.0, implementation)


def camera_rays(renderer, batch_size, like, image_size=None):
    """-> (origins [B,3], directions [B,S*S,3]) in `like`'s dtype and on its device: the rays of the renderer's camera
    (camera_mode 'look_at' or 'look', with perspective) through the rasterizer's pixel centres, xp = (2 xi + 1 - S) / S, ray
    r = row * S + column in the order of the rendered images (the top row first).  In camera axes a direction is
    (xp tan, yp tan, 1) with `perspective`'s own angle constant, rotated into the world by the inverse of `camera_rotation`:
    `look_at` and `perspective` send o + t d to (xp, yp, t), so the t of `ray_mesh_intersect` IS the camera depth.  S is
    `image_size`, None: the renderer's.  Plain torch: a learnable eye gets its gradient."""
    from .normals import camera_rotation
    from .perspective import _PI_REFERENCE
    if renderer.camera_mode not in ('look_at', 'look'):
        raise ValueError("camera_rays: camera_mode must be 'look_at' or 'look', got %r" % (renderer.camera_mode,))
    if not renderer.perspective:
        raise ValueError('camera_rays: the renderer must have perspective = True (one origin per image)')
    S = renderer.image_size if image_size is None else image_size
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError('camera_rays: image_size must be a positive integer, got %r' % (S,))
    B = int(batch_size)
    if B < 1:
        raise ValueError('camera_rays: batch_size must be a positive integer, got %r' % (batch_size,))
    eye = _util.as_tensor_like(renderer.eye, like, like.dtype)
    given = [('eye', eye)]
    if renderer.camera_mode == 'look':
        given.append(('camera_direction', _util.as_tensor_like(renderer.camera_direction, like, like.dtype)))
    for what, value in given:
        if not (value.dim() in (1, 2) and value.shape[-1] == 3 and (value.dim() == 1 or value.shape[0] in (1, B))):
            raise ValueError('camera_rays: Renderer.%s must be [3] or [batch size, 3] with batch size %d, got %s'
                             % (what, B, tuple(value.shape)))
    rot = camera_rotation(renderer, B, like)                           # [B,3,3], rows x, y, z (orthogonal, not quite unit)
    eye = (eye[None] if eye.dim() == 1 else eye).expand(B, 3)
    angle = renderer.viewing_angle
    if not torch.is_tensor(angle):
        angle = torch.tensor(float(angle), dtype=torch.float32, device=like.device)
    tangent = torch.tan(angle.to(torch.float32) / 180. * _PI_REFERENCE).to(like.dtype).reshape(-1, 1, 1)  # [1 or B,1,1]
    centre = ((2.0 * torch.arange(S, dtype=torch.float64, device=like.device) + 1 - S) / S).to(like.dtype)
    yp, xp = torch.meshgrid(centre.flip(0), centre, indexing='ij')     # the image's top row is the largest y
    cam = torch.stack((xp.reshape(-1), yp.reshape(-1)), -1)[None] * tangent                           # [1 or B,S*S,2]
    cam = torch.cat((cam, torch.ones_like(cam[..., :1])), -1).expand(B, S * S, 3)
    norms = (rot * rot).sum(2)                                         # R R^T = diag(norms): the rows are orthogonal
    return eye, torch.matmul(cam / norms[:, None, :], rot)
