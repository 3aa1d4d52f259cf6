"""Point-to-mesh distance without a GPU (neural_renderer_amd/point_mesh.py): the public names, the C ABI's argument checks, and
the plain-torch path -- the kernels' second yardstick -- entry by entry against the float64 restatement of
tests/point_mesh_ref.py within its derived bounds, in float32 and float64: distances, assignments, weights, loss and both
gradients, the exact lattice case in both directions, collapsed faces, gradcheck, validation and the Mesh method."""
import re

import numpy as np
import pytest
import torch

import neural_renderer
import neural_renderer_amd as nr
from neural_renderer_amd import _build, _lib, point_mesh

import point_mesh_ref as R

NAMES = ('closest_surface_points', 'closest_cloud_points', 'point_mesh_distance')
DIRECTIONS = ('both', 'points_to_mesh', 'mesh_to_points')
REDUCTIONS = ('mean', 'sum')
# (B, N, F, points shared by the batch): one pair, a wave, a tile and a split each crossed with a remainder
SHAPES = ((1, 1, 1, False), (2, 63, 255, False), (3, 257, 65, False), (2, 1027, 515, True), (3, 1, 515, False),
          (1, 70, 5000, False))
SYMBOLS = ('nr_point_mesh_workspace_bytes', 'nr_point_mesh_points_to_faces', 'nr_point_mesh_faces_to_points',
           'nr_point_mesh_loss', 'nr_point_mesh_backward_points', 'nr_point_mesh_backward_vertices')


def case(k):
    """-> (points, vertices [B,Nv,3], faces) float32 / int32 NumPy arrays of SHAPES[k]"""
    B, N, F, shared = SHAPES[k]
    vertices, faces = R.grid_mesh(200 + k, B, F)
    return R.cloud_near(300 + k, vertices, faces, N, shared), vertices, faces


def tensors(points, vertices, faces, dtype=torch.float32, device='cpu', grad=False):
    p = torch.tensor(points, dtype=dtype, device=device)
    v = torch.tensor(vertices, dtype=dtype, device=device)
    if grad:
        p.requires_grad_(True)
        v.requires_grad_(True)
    return p, v, torch.tensor(faces, device=device)


def host(t):
    return t.detach().cpu().numpy()


def check_case(points, vertices, faces, dtype=torch.float32, device='cpu', implementation=None, what='', upstream_seed=1):
    """closest_surface_points, closest_cloud_points and their gradients for per-pair upstream gradients that differ per image,
    against the restatement.  Shared points take no gradient.  -> the worst ratios"""
    u = R.U if dtype == torch.float32 else R.U64
    shared = points.ndim == 2
    as64 = (lambda a: np.asarray(a, np.float64)) if dtype == torch.float64 else (lambda a: a)
    p, v, f = tensors(points, vertices, faces, dtype, device, grad=True)
    if shared:
        p = p.detach()
    B, Nv = vertices.shape[:2]
    rng = np.random.default_rng(upstream_seed)
    ds, fid, ws = nr.closest_surface_points(p, v, f, implementation)
    dc, pid, wc = nr.closest_cloud_points(p, v, f, implementation)
    assert fid.dtype == torch.int64 and pid.dtype == torch.int64 and ds.dtype == dtype and ws.dtype == dtype
    assert not fid.requires_grad and not ws.requires_grad and not wc.requires_grad
    ratios = list(R.check_closest(host(ds), host(fid), host(ws), as64(points), as64(vertices), faces, u, what + ' surface'))
    ratios += R.check_closest(host(dc), host(pid), host(wc), as64(points), as64(vertices), faces, u, what + ' cloud', True)
    gs = rng.uniform(-1, 1, ds.shape).astype(np.float32)
    gc = rng.uniform(-1, 1, dc.shape).astype(np.float32)
    total = (ds * torch.tensor(gs, dtype=dtype, device=device)).sum() + (dc * torch.tensor(gc, dtype=dtype, device=device)).sum()
    grads = torch.autograd.grad(total, [v] if shared else [p, v])
    pb = np.broadcast_to(points, (B,) + points.shape[-2:])
    (gp, mp, kp), (gv, mv, kv) = R.gradients(as64(pb), as64(vertices), faces, (host(fid), host(ws), gs),
                                             (host(pid), host(wc), gc), Nv)
    r_v = R.gradient_ratio(host(grads[-1]), gv, mv, kv, u)
    r_p = 0.0 if shared else R.gradient_ratio(host(grads[0]), gp, mp, kp, u)
    print('%s grad_points ratio %.4f grad_vertices ratio %.4f' % (what, r_p, r_v))
    assert r_p <= 1.0 and r_v <= 1.0, (what, r_p, r_v)
    assert np.isfinite(host(grads[-1])).all()
    return ratios + [r_p, r_v]


def check_loss(points, vertices, faces, direction, reduction, dtype=torch.float32, device='cpu', implementation=None, what=''):
    """point_mesh_distance and its gradients (through the pairs of the closest_* calls, which share the kernels) against the
    restatement, with an upstream gradient per image"""
    u = R.U if dtype == torch.float32 else R.U64
    shared = points.ndim == 2
    as64 = (lambda a: np.asarray(a, np.float64)) if dtype == torch.float64 else (lambda a: a)
    p, v, f = tensors(points, vertices, faces, dtype, device, grad=True)
    if shared:
        p = p.detach()
    B, Nv = vertices.shape[:2]
    N, F = points.shape[-2], faces.shape[0]
    loss = nr.point_mesh_distance(p, v, f, direction, reduction, implementation)
    assert tuple(loss.shape) == (B,) and loss.dtype == dtype
    want, bnd = R.loss(as64(points), as64(vertices), faces, direction, reduction, B, u)
    r_l = R._ratio(np.abs(host(loss).astype(np.float64) - want), bnd)
    gl = np.random.default_rng(4).uniform(0.5, 1.5, B).astype(np.float32)
    grads = torch.autograd.grad((loss * torch.tensor(gl, dtype=dtype, device=device)).sum(), [v] if shared else [p, v])
    wp, wf = R.weights(N, F, reduction)
    surface = cloud = None
    with torch.no_grad():
        if direction != 'mesh_to_points':
            _, fid, ws = nr.closest_surface_points(p, v, f, implementation)
            surface = (host(fid), host(ws), np.repeat((gl * wp)[:, None], N, 1))
        if direction != 'points_to_mesh':
            _, pid, wc = nr.closest_cloud_points(p, v, f, implementation)
            cloud = (host(pid), host(wc), np.repeat((gl * wf)[:, None], F, 1))
    pb = np.broadcast_to(points, (B,) + points.shape[-2:])
    (gp, mp, kp), (gv, mv, kv) = R.gradients(as64(pb), as64(vertices), faces, surface, cloud, Nv)
    r_v = R.gradient_ratio(host(grads[-1]), gv, mv, kv, u)
    r_p = 0.0 if shared else R.gradient_ratio(host(grads[0]), gp, mp, kp, u)
    print('%s %s %s loss ratio %.4f grad_points %.4f grad_vertices %.4f' % (what, direction, reduction, r_l, r_p, r_v))
    assert r_l <= 1.0 and r_p <= 1.0 and r_v <= 1.0, (what, r_l, r_p, r_v)
    return r_l, r_p, r_v


# ---------------------------------------------------------------------------------------------------------------------

def test_public_names():
    for name in NAMES:
        assert name in nr.__all__
        assert getattr(neural_renderer, name) is getattr(nr, name) is getattr(point_mesh, name)
    assert callable(nr.Mesh.point_mesh_distance)


def test_abi_declares_binds_and_exports_the_entry_points():
    import ctypes
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nr_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(n for n in re.findall(r'\b(nr_[a-z_0-9]+)\s*\(', header) if n.startswith('nr_point_mesh_'))
    assert declared == set(SYMBOLS)
    assert set(n for n in _lib.SIGNATURES if n.startswith('nr_point_mesh_')) == set(SYMBOLS)
    lib = ctypes.CDLL(_build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.load().nr_version() == 600


def test_argument_errors_do_not_need_a_device():
    _build.build()
    lib = _lib.load()
    NULL, SIZE, MODE, WS = -1, -2, -4, -3
    for fn in (lib.nr_point_mesh_points_to_faces, lib.nr_point_mesh_faces_to_points):
        assert fn(None, 1, 1, 1, 1, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
        assert fn(1, None, 1, 1, 1, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
        assert fn(1, 1, 1, 1, None, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
        assert fn(1, 1, 1, 1, 1, 1, 0, 4, 3, 1, 1, 0, None, 0, None) == SIZE
        assert fn(1, 1, 1, 1, 1, 1, 65536, 4, 3, 1, 1, 0, None, 0, None) == SIZE
        assert fn(1, 1, 1, 1, 1, 1, 1, 0, 3, 1, 1, 0, None, 0, None) == SIZE
        assert fn(1, 1, 1, 1, 1, 1, 1, 4, 3, 0, 1, 0, None, 0, None) == SIZE
        assert fn(1, 1, 1, 1, 1, 1, 1, 4, 3, 1, 1, -1, None, 0, None) == SIZE
        assert fn(1, 1, 1, 1, 1, 1, 40000, 40000, 3, 1, 1, 0, None, 0, None) == SIZE   # B N 3 above int32
        assert fn(1, 1, 1, 1, 1, 1, 1, 5000, 3, 5000, 1, 3, None, 0, None) == WS         # a split call without its workspace
        # a forced split on a very large cloud: more than 2^31 - 1 workgroups along x is a size error, before the workspace
        assert fn(1, 1, 1, 1, 1, 1, 1, 600000000, 3, 100000000, 1, 7000, None, 0, None) == SIZE
        assert fn(1, 1, 1, 1, 1, 1, 1, 600000000, 3, 100000000, 1, 1000, None, 0, None) == WS  # (fewer: the workspace is asked for)
    for faces_to_points in (0, 1):
        assert lib.nr_point_mesh_workspace_bytes(1, 600000000, 100000000, faces_to_points, 7000) == 0
    assert lib.nr_point_mesh_workspace_bytes(1, 5000, 5000, 0, 1) == 0
    assert lib.nr_point_mesh_workspace_bytes(1, 5000, 5000, 0, 3) == 3 * 5000 * 8
    assert lib.nr_point_mesh_workspace_bytes(1, 70, 5000, 1, 0) == 0     # one tile of points: nothing to split
    assert lib.nr_point_mesh_workspace_bytes(0, 70, 5000, 0, 0) == 0
    assert lib.nr_point_mesh_workspace_bytes(64, 8192, 2464, 0, 0) == 0  # 1 024 workgroups: the grid fills the machine
    assert lib.nr_point_mesh_loss(1, 1, None, 1, 4, 4, 1.0, 1.0, None) == NULL
    assert lib.nr_point_mesh_loss(None, None, 1, 1, 4, 4, 1.0, 1.0, None) == MODE
    assert lib.nr_point_mesh_loss(1, None, 1, 0, 4, 4, 1.0, 1.0, None) == SIZE
    bp, bv = lib.nr_point_mesh_backward_points, lib.nr_point_mesh_backward_vertices
    assert bp(1, 1, 1, 1, 1, 1, None, None, None, None, None, None, 1, 4, 3, 1, None) == NULL
    assert bp(1, 1, 1, 1, None, 1, None, None, None, None, None, 1, 1, 4, 3, 1, None) == NULL
    assert bp(1, 1, 1, None, None, None, 1, 1, 1, None, 1, 1, 1, 4, 3, 1, None) == NULL   # the list without its order
    assert bp(1, 1, 1, None, None, None, None, None, None, None, None, 1, 1, 4, 3, 1, None) == MODE
    assert bp(1, 1, 1, 1, 1, 1, None, None, None, None, None, 1, 0, 4, 3, 1, None) == SIZE
    assert bv(1, 1, 1, None, 1, 1, 1, 1, 1, 1, None, None, None, 1, 1, 4, 3, 1, 1, None) == NULL  # no adjacency table
    assert bv(1, 1, 1, 1, 1, 1, 1, 1, None, 1, None, None, None, 1, 1, 4, 3, 1, 1, None) == NULL
    assert bv(1, 1, 1, 1, 1, None, None, None, None, None, None, None, None, 1, 1, 4, 3, 1, 1, None) == MODE
    assert bv(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, None, None, None, 1, 1, 4, 0, 1, 1, None) == SIZE


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_torch_path_against_the_float64_restatement(k, dtype):
    points, vertices, faces = case(k)
    check_case(points, vertices, faces, dtype, what='torch %s %s' % (SHAPES[k], dtype))


@pytest.mark.parametrize('direction', DIRECTIONS)
@pytest.mark.parametrize('reduction', REDUCTIONS)
def test_torch_loss_against_the_float64_restatement(direction, reduction):
    for k in (1, 3):
        points, vertices, faces = case(k)
        check_loss(points, vertices, faces, direction, reduction, what='torch %s' % (SHAPES[k],))


def test_random_triangles_at_three_distances():
    """400 random triangles, 1 500 points at 1, 0.05 and 1e-3 from them: the float32 torch path inside the bound"""
    vertices, faces = R.triangle_soup(11, 400)
    points = R.cloud_near(12, vertices, faces, 1500)
    check_case(points, vertices, faces, what='soup')


def check_lattice(device='cpu', implementation=None):
    points, vertices, faces = R.lattice()
    assert vertices.shape == (26, 3) and faces.shape == (48, 3)
    v0, v1, v2 = R.corners(vertices, faces, 0)
    m = R.pair_matrix(points, v0, v1, v2)
    assert R.tied_rows(m) == 230 and int((m.min(1) == 0).sum()) == 58 and R.tied_rows(m.T) == 33
    p, v, f = tensors(points, vertices, faces, device=device)
    d, i, w = nr.closest_surface_points(p, v, f, implementation)
    assert tuple(d.shape) == (300,) and np.array_equal(host(d).astype(np.float64), m.min(1))
    assert np.array_equal(host(i), m.argmin(1))
    d, i, w = nr.closest_cloud_points(p, v, f, implementation)
    assert tuple(d.shape) == (48,) and np.array_equal(host(d).astype(np.float64), m.min(0))
    assert np.array_equal(host(i), m.argmin(0))


def test_lattice_is_exact_in_both_directions():
    check_lattice()


def check_collapsed(device='cpu', implementation=None):
    for what, (vertices, faces) in (('collapsed alone', R.collapsed_faces()),
                                    ('collapsed mixed', R.with_collapsed(*R.grid_mesh(31, 2, 199)))):
        points = np.random.default_rng(8).uniform(-1.2, 1.2, (vertices.shape[0], 97, 3)).astype(np.float32)
        ratios = check_case(points, vertices, faces, device=device, implementation=implementation, what=what)
        assert np.isfinite(ratios).all()
        p, v, f = tensors(points, vertices, faces, device=device, grad=True)
        loss = nr.point_mesh_distance(p, v, f, implementation=implementation)
        loss.sum().backward()
        assert np.isfinite(host(loss)).all() and np.isfinite(host(p.grad)).all() and np.isfinite(host(v.grad)).all()


def test_collapsed_faces():
    check_collapsed()


def test_surface_samples_evaluate_to_the_closest_points():
    points, vertices, faces = case(2)
    p, v, f = tensors(points, vertices, faces)
    dist2, ids, w = nr.closest_surface_points(p, v, f)
    order = torch.sort(ids, dim=1, stable=True)[1]
    rows = torch.arange(ids.shape[0])[:, None]
    samples = nr.SurfaceSamples(ids[rows, order], w[rows, order], faces.shape[0])
    c = samples.points(v, f)
    d = ((p[rows, order] - c) ** 2).sum(2)
    # the samples' points are w0 v0 + w1 v1 + w2 v2 in float32: 3 u x the coordinates' magnitude per component
    tol = 2 * np.sqrt(host(dist2[rows, order])) * 3 * R.U * 3 * np.abs(vertices).max() * np.sqrt(3) + 1e-12
    assert (np.abs(host(d) - host(dist2[rows, order])) <= tol).all()


def test_gradcheck_away_from_ties():
    vertices, faces = R.grid_mesh(41, 2, 7)
    points = R.cloud_near(42, vertices, faces, 5)
    p, v, f = tensors(points, vertices, faces, torch.float64, grad=True)
    for direction in DIRECTIONS:
        assert torch.autograd.gradcheck(lambda a, b: nr.point_mesh_distance(a, b, f, direction, 'sum'), (p, v), eps=1e-7,
                                        atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a, b: nr.closest_surface_points(a, b, f)[0], (p, v), eps=1e-7, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a, b: nr.closest_cloud_points(a, b, f)[0], (p, v), eps=1e-7, atol=1e-6, rtol=1e-5)


def test_shapes_and_batching():
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces)
    assert nr.point_mesh_distance(p[0], v[0], f).dim() == 0
    d, i, w = nr.closest_surface_points(p[0], v[0], f)
    assert tuple(d.shape) == (63,) and tuple(i.shape) == (63,) and tuple(w.shape) == (63, 3)
    d, i, w = nr.closest_cloud_points(p[0], v[0], f)
    assert tuple(d.shape) == (255,) and tuple(w.shape) == (255, 3)
    # points shared by the batch, as [N,3] and as [1,N,3]; vertices shared by the batch
    whole = nr.point_mesh_distance(p[0], v, f)
    assert tuple(whole.shape) == (2,) and torch.equal(whole, nr.point_mesh_distance(p[0:1], v, f))
    assert torch.equal(whole[1], nr.point_mesh_distance(p[0], v[1], f))
    assert torch.equal(nr.point_mesh_distance(p, v[0], f)[1], nr.point_mesh_distance(p[1], v[0], f))
    # a single direction is its own term; both is their sum in double
    both = nr.point_mesh_distance(p, v, f, 'both', 'sum').double()
    parts = nr.point_mesh_distance(p, v, f, 'points_to_mesh', 'sum').double() + \
        nr.point_mesh_distance(p, v, f, 'mesh_to_points', 'sum').double()
    assert torch.allclose(both, parts, rtol=1e-6, atol=0)


def test_non_finite_input_never_wins():
    points, vertices, faces = case(1)
    bad = vertices.copy()
    bad[:, 5] = np.nan
    moved = vertices.copy()
    moved[:, 5] = 1000.0
    p, v, f = tensors(points, bad, faces)
    d, i, w = nr.closest_surface_points(p, v, f)
    touched = torch.tensor((faces == 5).any(1))
    assert not touched[i].any() and torch.isfinite(d).all()
    d2, i2, w2 = nr.closest_surface_points(p, torch.tensor(moved), f)
    other = ~touched[i2]  # (the moved vertex stretches its faces across the cloud: rows that choose one of them differ)
    assert int(other.sum()) > other.numel() // 2
    assert torch.equal(d[other], d2[other]) and torch.equal(i[other], i2[other]) and torch.equal(w[other], w2[other])
    dc, ic, wc = nr.closest_cloud_points(p, v, f)
    dc2, ic2, wc2 = nr.closest_cloud_points(p, torch.tensor(moved), f)
    keep = ~touched
    assert torch.equal(dc[:, keep], dc2[:, keep]) and torch.equal(ic[:, keep], ic2[:, keep])
    assert (ic[:, touched] == 0).all() and not torch.isfinite(dc[:, touched]).any()
    # a row all of whose pairs are NaN
    pn = p.clone()
    pn[0, 3] = float('nan')
    d, i, w = nr.closest_surface_points(pn, torch.tensor(vertices), f)
    assert int(i[0, 3]) == 0 and not torch.isfinite(d[0, 3]) and int(i.min()) >= 0 and int(i.max()) < faces.shape[0]


def test_validation():
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces)
    with pytest.raises(ValueError, match='points must be a float tensor'):
        nr.point_mesh_distance(p[..., :2], v, f)
    with pytest.raises(ValueError, match='points must be a float tensor'):
        nr.closest_surface_points(p.long(), v, f)
    with pytest.raises(ValueError, match='vertices must be a float tensor'):
        nr.closest_cloud_points(p, v[..., :2], f)
    with pytest.raises(ValueError, match='faces must be an integer tensor'):
        nr.point_mesh_distance(p, v, f[None])
    with pytest.raises(ValueError, match='share dtype and device'):
        nr.point_mesh_distance(p.double(), v, f)
    with pytest.raises(ValueError, match='points have batch size 3, vertices 2'):
        nr.point_mesh_distance(torch.cat((p, p[:1])), v, f)
    with pytest.raises(IndexError):
        nr.point_mesh_distance(p, v, f + 1000)
    with pytest.raises(ValueError, match='direction must be'):
        nr.point_mesh_distance(p, v, f, 'x_to_y')
    with pytest.raises(ValueError, match='reduction must be'):
        nr.point_mesh_distance(p, v, f, 'both', 'max')
    with pytest.raises(ValueError, match='implementation must be'):
        nr.point_mesh_distance(p, v, f, implementation='cuda')


def test_hip_on_cpu_tensors_raises_the_limit_sentence():
    points, vertices, faces = case(0)
    p, v, f = tensors(points, vertices, faces)
    for fn in (nr.closest_surface_points, nr.closest_cloud_points, nr.point_mesh_distance):
        with pytest.raises(ValueError) as err:
            fn(p, v, f, implementation='hip')
        assert point_mesh._NEEDS in str(err.value)
        fn(p, v, f, implementation='torch')


def test_mesh_method(tmp_path):
    import point_loss_ref
    v, f = point_loss_ref.octahedron()
    path = str(tmp_path / 'octa.obj')
    with open(path, 'w') as fh:
        fh.write(''.join('v %g %g %g\n' % tuple(p) for p in v) + ''.join('f %d %d %d\n' % tuple(t + 1) for t in f))
    mesh = nr.Mesh(path, normalization=False)
    points = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (40, 3)), dtype=torch.float32)
    loss = mesh.point_mesh_distance(points, direction='points_to_mesh', reduction='sum')
    assert loss.dim() == 0 and torch.equal(loss, nr.point_mesh_distance(points, mesh.vertices, mesh.faces, 'points_to_mesh', 'sum'))
    loss.backward()
    assert mesh.vertices.grad is not None and float(mesh.vertices.grad.abs().sum()) > 0
