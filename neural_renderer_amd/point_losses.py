"""Point-cloud terms of a 3-D fit (not in the reference's library): points sampled on a mesh's surface, differentiable in
the vertices, and the chamfer distance between two point sets with its nearest-neighbour search exposed.

`nearest_points(x, y)` -> (dist2, idx): dist2[b,i] = min_j |x_bi - y_bj|^2 and the LOWEST minimising j, for x [B,N,3] (or
[N,3]) and y [B,M,3], or [M,3] / [1,M,3] shared by the batch and read in place.  The distance is dx^2 + dy^2 + dz^2 of the
coordinate differences (never the |x|^2 + |y|^2 - 2 x.y expansion, which cancels); a NaN distance never wins, so idx always
lies in [0, M).  dist2 is differentiable in x and y; idx is int64.

`chamfer_distance(x, y, direction, reduction)`: loss_b = wx sum_i dist2(x_i, y) + wy sum_j dist2(y_j, x), wx, wy = 1/N, 1/M
('mean') or 1, 1 ('sum'); direction 'x_to_y' / 'y_to_x' keeps one term and launches only its kernels.

`sample_surface(vertices, faces, num_samples, generator)` draws per image faces in proportion to their area and uniform
barycentric weights, and returns a `SurfaceSamples` (face ids ascending per image, weights, per-face segment offsets);
`samples.points(vertices, faces)` evaluates them, differentiably in the vertices; `sample_surface_points` does both.

Everything here is plain torch, on any device and in any float dtype: the search computes by differences in chunks over N
(its [B,n,M,3] temporary stays near 2^26 elements, never the whole [B,N,M] matrix), and the sums over the points are taken
in float64 and rounded once.  HIP kernels for the search, the loss, its backward and the surface points were written and
measured, but a step of them captured into a HIP graph crashed when the capture ended and the cause was not found, so
they are not part of the package (DESIGN "Point-cloud losses"); `implementation='hip'` therefore raises."""
import torch

from . import _util

_CHUNK_ELEMENTS = 1 << 26  # the torch path's [B, n, M, 3] temporary


# ---------------------------------------------------------------------------------------------------------------------
# checks

def _clouds(name, x, y):
    """-> (x [B,N,3], y [B or 1,M,3], squeeze)"""
    for what, t in (('x', x), ('y', y)):
        if not (torch.is_tensor(t) and t.is_floating_point() and t.dim() in (2, 3) and t.shape[-1] == 3 and t.shape[-2] >= 1
                and t.shape[0] >= 1):
            raise ValueError('%s: %s must be a float tensor [num of points, 3] or [batch size, num of points, 3] with at least '
                             'one point' % (name, what))
    if x.dtype != y.dtype or x.device != y.device:
        raise ValueError('%s: x and y must share dtype and device (%s %s, %s %s)' % (name, x.dtype, x.device, y.dtype, y.device))
    squeeze = x.dim() == 2 and y.dim() == 2
    if x.dim() == 2:
        if y.dim() == 3 and y.shape[0] != 1:
            raise ValueError('%s: x has no batch axis but y has a batch of %d' % (name, y.shape[0]))
        x = x[None]
    if y.dim() == 2:
        y = y[None]
    if y.shape[0] not in (1, x.shape[0]):
        raise ValueError('%s: y has batch size %d, x %d' % (name, y.shape[0], x.shape[0]))
    return x, y, squeeze


def _check_implementation(name, implementation):
    """None and 'torch' are the plain-torch path; 'hip' names kernels that this package does not have."""
    _util.takes_hip(name, implementation, False, 'there are no HIP kernels for the point-cloud losses; use implementation=None')


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _search_torch(x, y):
    """idx [B,N] int64 of the nearest y for every x (lowest j on a tie, NaN never wins), in chunks over N."""
    B, N, M = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    step = max(1, _CHUNK_ELEMENTS // (B * M * 3))
    out = []
    with torch.no_grad():
        for n0 in range(0, N, step):
            diff = x[:, n0:n0 + step, None, :] - y[:, None, :, :]
            d = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
            d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)
            out.append(torch.min(d, dim=2)[1])
    return torch.cat(out, 1)


def _gather(y, idx):
    """y[b, idx[b, i]] -> [B,N,3] for y [B or 1,M,3]"""
    B = idx.shape[0]
    if y.shape[0] == 1:
        return y[0][idx]
    return y[torch.arange(B, device=y.device)[:, None], idx]


def _nearest_torch(x, y):
    idx = _search_torch(x.detach(), y.detach())
    diff = x - _gather(y, idx)
    return diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2], idx


def _chamfer_torch(x, y, direction, wx, wy):
    """The sums over the points in float64 (one rounding to the inputs' dtype at the end, as the kernels do)."""
    total = None
    if direction in ('both', 'x_to_y'):
        total = _nearest_torch(x, y)[0].double().sum(1) * wx
    if direction in ('both', 'y_to_x'):
        yb = y if y.shape[0] == x.shape[0] else y.expand(x.shape[0], -1, -1)
        term = _nearest_torch(yb, x)[0].double().sum(1) * wy
        total = term if total is None else total + term
    return total.to(x.dtype)


def nearest_points(x, y, implementation=None):
    """-> (dist2 [B,N] in x's dtype, idx [B,N] int64): the squared distance of every x to its nearest y and that y's index,
    the lowest on a tie ([N] each when neither input has a batch axis).  See the module docstring."""
    x, y, squeeze = _clouds('nearest_points', x, y)
    _check_implementation('nearest_points', implementation)
    dist2, idx = _nearest_torch(x, y)
    return (dist2[0], idx[0]) if squeeze else (dist2, idx)


def chamfer_distance(x, y, direction='both', reduction='mean', implementation=None):
    """The chamfer distance of x [B,N,3] and y [B,M,3] (or [M,3] / [1,M,3] shared by the batch): [B], a 0-dim tensor when
    neither input has a batch axis.  direction 'both' | 'x_to_y' | 'y_to_x'; reduction 'mean' | 'sum'.  Differentiable
    in x and y.  See the module docstring."""
    x, y, squeeze = _clouds('chamfer_distance', x, y)
    if direction not in ('both', 'x_to_y', 'y_to_x'):
        raise ValueError("chamfer_distance: direction must be 'both', 'x_to_y' or 'y_to_x'")
    if reduction not in ('mean', 'sum'):
        raise ValueError("chamfer_distance: reduction must be 'mean' or 'sum'")
    N, M = int(x.shape[1]), int(y.shape[1])
    wx, wy = (1.0 / N, 1.0 / M) if reduction == 'mean' else (1.0, 1.0)
    _check_implementation('chamfer_distance', implementation)
    loss = _chamfer_torch(x, y, direction, wx, wy)
    return loss[0] if squeeze else loss


# ---------------------------------------------------------------------------------------------------------------------
# surface samples

def _mesh(name, vertices, faces):
    """-> (vertices [B,Nv,3], faces [Nf,3], squeeze)"""
    if not (torch.is_tensor(vertices) and vertices.is_floating_point() and vertices.dim() in (2, 3) and vertices.shape[-1] == 3
            and vertices.shape[-2] >= 1 and vertices.shape[0] >= 1):
        raise ValueError('%s: vertices must be a float tensor [num of vertices, 3] or [batch size, num of vertices, 3]' % name)
    squeeze = vertices.dim() == 2
    if squeeze:
        vertices = vertices[None]
    if not (torch.is_tensor(faces) and not faces.is_floating_point() and faces.dtype != torch.bool and faces.dim() == 2
            and faces.shape[-1] == 3 and faces.shape[0] >= 1):
        raise ValueError('%s: faces must be an integer tensor [num of faces, 3] (one topology per call)' % name)
    if faces.device != vertices.device:
        raise ValueError('%s: vertices and faces must be on one device (%s, %s)' % (name, vertices.device, faces.device))
    _util.check_face_indices(faces, int(vertices.shape[1]), vertices.device)
    return vertices, faces, squeeze


def _segment_offsets(face_ids, num_faces):
    """[B,F+1] int32: offsets[b,f] = the number of samples of image b with a face id below f (ids ascending)."""
    B = face_ids.shape[0]
    bounds = torch.arange(num_faces + 1, device=face_ids.device, dtype=face_ids.dtype)[None].expand(B, -1).contiguous()
    return torch.searchsorted(face_ids.contiguous(), bounds).to(torch.int32)


class SurfaceSamples(object):
    """Points on a mesh given by face and barycentric weights: face_ids [B,N] int32 ascending per image, barycentric
    [B,N,3] (w0, w1, w2 of the face's corners) and segment_offsets [B,F+1] int32 (the samples of face f of image b are
    [segment_offsets[b,f], segment_offsets[b,f+1])).  The constructor checks range and order with one readback (inside a
    graph capture it raises: build the samples before the capture)."""

    def __init__(self, face_ids, barycentric, num_faces, _trusted=False):
        num_faces = int(num_faces)
        if not (torch.is_tensor(face_ids) and not face_ids.is_floating_point() and face_ids.dtype != torch.bool
                and face_ids.dim() == 2 and face_ids.shape[0] >= 1 and face_ids.shape[1] >= 1):
            raise ValueError('SurfaceSamples: face_ids must be an integer tensor [batch size, num of samples]')
        if not (torch.is_tensor(barycentric) and barycentric.is_floating_point()
                and tuple(barycentric.shape) == tuple(face_ids.shape) + (3,)):
            raise ValueError('SurfaceSamples: barycentric must be a float tensor [batch size, num of samples, 3]')
        if barycentric.device != face_ids.device:
            raise ValueError('SurfaceSamples: face_ids and barycentric must be on one device')
        if num_faces < 1:
            raise ValueError('SurfaceSamples: num_faces must be positive')
        if not _trusted:
            if face_ids.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('SurfaceSamples cannot be checked while a HIP graph is being captured (the check reads two '
                                   'flags back): build the samples before the capture')
            in_range = ((face_ids >= 0) & (face_ids < num_faces)).all()
            ascending = (face_ids[:, 1:] >= face_ids[:, :-1]).all()
            in_range, ascending = torch.stack((in_range, ascending)).tolist()
            if not in_range:
                raise IndexError('SurfaceSamples: a face id outside [0, %d)' % num_faces)
            if not ascending:
                raise ValueError('SurfaceSamples: the face ids of an image must be ascending')
        self.face_ids = face_ids.to(torch.int32).contiguous()
        self.barycentric = barycentric.detach().contiguous()
        self.num_faces = num_faces
        self.segment_offsets = _segment_offsets(self.face_ids, num_faces)

    @property
    def device(self):
        return self.face_ids.device

    @property
    def num_samples(self):
        return int(self.face_ids.shape[1])

    def points(self, vertices, faces, implementation=None):
        """[B,N,3] ([N,3] for vertices [Nv,3]): w0 v0 + w1 v1 + w2 v2 of every sample's face, differentiable in the
        vertices."""
        vertices, faces, squeeze = _mesh('SurfaceSamples.points', vertices, faces)
        B, Nv = int(vertices.shape[0]), int(vertices.shape[1])
        if int(faces.shape[0]) != self.num_faces:
            raise ValueError('SurfaceSamples.points: the samples were made for %d faces, the mesh has %d' % (self.num_faces, faces.shape[0]))
        if self.face_ids.shape[0] != B or self.device != vertices.device:
            raise ValueError('SurfaceSamples.points: the samples are for %d images on %s, the vertices for %d on %s'
                             % (self.face_ids.shape[0], self.device, B, vertices.device))
        _check_implementation('SurfaceSamples.points', implementation)
        points = _points_torch(vertices, faces, self.face_ids, self.barycentric.to(vertices.dtype))
        return points[0] if squeeze else points


def _points_torch(vertices, faces, face_ids, barycentric):
    corners = faces.long()[face_ids.long()]  # [B,N,3] vertex indices
    rows = torch.arange(vertices.shape[0], device=vertices.device)[:, None]
    v0, v1, v2 = (vertices[rows, corners[..., k]] for k in range(3))
    w = barycentric
    return w[..., 0:1] * v0 + w[..., 1:2] * v1 + w[..., 2:3] * v2


def sample_surface(vertices, faces, num_samples, generator=None):
    """Draw, per image, `num_samples` faces with probability proportional to their area (from the detached vertices; a
    zero-area face is never drawn, an image without area raises) and barycentric weights uniform on the triangle,
    w = (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2).  Both draws are torch's, on the vertices' device, from `generator`.
    The samples of an image are sorted by face id (they are independent, so nothing is lost).  -> SurfaceSamples"""
    vertices, faces, _ = _mesh('sample_surface', vertices, faces)
    num_samples = int(num_samples)
    if num_samples < 1:
        raise ValueError('sample_surface: num_samples must be positive')
    if vertices.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('sample_surface reads the total area back: draw the samples before the capture')
    B, dev = int(vertices.shape[0]), vertices.device
    with torch.no_grad():
        v = vertices.detach().float()
        f = faces.long()
        v0, v1, v2 = v[:, f[:, 0]], v[:, f[:, 1]], v[:, f[:, 2]]
        area = torch.linalg.cross(v1 - v0, v2 - v0, dim=2).norm(dim=2)  # (twice the area: only the proportions matter)
        total = area.sum(1)
        if not bool((torch.isfinite(total) & (total > 0)).all()):
            raise ValueError('sample_surface: an image whose faces have no area (or a non-finite one) cannot be sampled')
        face_ids = torch.multinomial(area, num_samples, replacement=True, generator=generator)
        face_ids = torch.sort(face_ids, dim=1)[0]
        r = torch.rand((B, num_samples, 2), generator=generator, device=dev, dtype=torch.float32)
        s = torch.sqrt(r[..., 0])
        barycentric = torch.stack((1.0 - s, s * (1.0 - r[..., 1]), s * r[..., 1]), dim=2)
    return SurfaceSamples(face_ids, barycentric, int(faces.shape[0]), _trusted=True)


def sample_surface_points(vertices, faces, num_samples, generator=None):
    """sample_surface, then the samples' points: -> (points [B,N,3] or [N,3], samples)"""
    samples = sample_surface(vertices, faces, num_samples, generator)
    return samples.points(vertices, faces), samples
