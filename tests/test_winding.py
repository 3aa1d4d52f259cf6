"""Winding numbers without a GPU (neural_renderer_amd/winding.py): the public names, the C ABI's argument checks, and the
plain-torch path -- the kernels' second yardstick -- entry by entry against the float64 restatement of tests/winding_ref.py
within its derived bounds, in float32 and float64: w and both gradients, the analytic pins, every edge rule, gradcheck, the
voxel grid, the voxel IoU, the signed distance, validation and the Mesh methods."""
import os
import re

import numpy as np
import pytest
import torch

import neural_renderer
import neural_renderer_amd as nr
from neural_renderer_amd import _build, _lib, winding

import winding_ref as R

NAMES = ('winding_number', 'mesh_occupancy', 'voxel_centers', 'voxelize', 'voxel_iou', 'signed_distance')
SYMBOLS = ('nr_winding_workspace_bytes', 'nr_winding_forward', 'nr_winding_backward_points', 'nr_winding_backward_vertices')
T, Q = winding._T, winding._Q
# (B, N, F, points shared by the batch): F in {1, T - 1, T, T + 1, 2 T + 3} and N in {1, 63, 64, 65, 256 Q + 1}, every value at least
# once, with one image and three, with a cloud per image and a shared one
SHAPES = ((1, 1, 1, False), (3, 63, T - 1, False), (3, 64, T, True), (1, 65, T + 1, False), (3, 256 * Q + 1, 2 * T + 3, False),
          (3, 256 * Q + 1, 1, True), (1, 256 * Q + 1, 2 * T + 3, False), (3, 1, T + 1, True))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SPHERE = {}


def sphere(level=3):
    if level not in _SPHERE:
        _SPHERE[level] = R.icosphere(level)
    return _SPHERE[level]


def case(k):
    """-> (points, vertices [B,Nv,3], faces) float32 / int32 NumPy arrays of SHAPES[k]: the first F faces of icosphere(3), the
    vertices jittered per image, the points off the sphere"""
    B, N, F, shared = SHAPES[k]
    v, f = sphere()
    return R.shell_points(300 + k, N, 1.0, None if shared else B), R.batch_of(v, B, 200 + k), f[:F].copy()


def tensors(points, vertices, faces, dtype=torch.float32, device='cpu', grad=False):
    p = torch.tensor(points, dtype=dtype, device=device)
    v = torch.tensor(vertices, dtype=dtype, device=device)
    if grad:
        p.requires_grad_(True)
        v.requires_grad_(True)
    return p, v, torch.tensor(faces, device=device)


def host(t):
    return t.detach().cpu().numpy()


def check_case(points, vertices, faces, dtype=torch.float32, device='cpu', implementation=None, what='', upstream_seed=1,
               scale=1.0):
    """winding_number and both gradients for per-entry upstream gradients that differ per image, against the restatement; the
    bound of w is itself at most MAX_BOUND on every entry.  Shared points take no gradient.  `scale`: the bounds times it (the
    sum of two paths' bounds).  -> (w, grad_points or None, grad_vertices) and the worst ratios"""
    u = R.U if dtype == torch.float32 else R.U64
    shared = points.ndim == 2
    p, v, f = tensors(points, vertices, faces, dtype, device, grad=True)
    if shared:
        p = p.detach()
    B, Nv = vertices.shape[:2]
    w = nr.winding_number(p, v, f, implementation)
    assert w.dtype == dtype and tuple(w.shape) == (B, points.shape[-2])
    want, bnd = R.winding(points, vertices, faces, u)
    assert np.isfinite(bnd).all() and bnd.max() <= R.MAX_BOUND * (u / R.U), (what, bnd.max())
    r_w = R.ratio(host(w), want, scale * bnd)
    g = np.random.default_rng(upstream_seed).uniform(-1, 1, (B, points.shape[-2])).astype(np.float32)
    grads = torch.autograd.grad((w * torch.tensor(g, dtype=dtype, device=device)).sum(), [v] if shared else [p, v])
    pb = np.broadcast_to(points, (B,) + points.shape[-2:])
    (gp, bp), (gv, bv) = R.gradients(pb, vertices, faces, g, Nv, u)
    r_v = R.ratio(host(grads[-1]), gv, scale * bv)
    r_p = 0.0 if shared else R.ratio(host(grads[0]), gp, scale * bp)
    print('%s w ratio %.4f grad_points ratio %.4f grad_vertices ratio %.4f (w bound at most %.2e)' % (what, r_w, r_p, r_v, bnd.max()))
    assert r_w <= 1.0 and r_p <= 1.0 and r_v <= 1.0, (what, r_w, r_p, r_v)
    return (w, None if shared else grads[0], grads[-1]), (r_w, r_p, r_v)


# ---------------------------------------------------------------------------------------------------------------------

def test_public_names():
    for name in NAMES:
        assert name in nr.__all__
        assert getattr(neural_renderer, name) is getattr(nr, name) is getattr(winding, name)
    for name in ('winding_number', 'voxelize', 'signed_distance'):
        assert callable(getattr(nr.Mesh, name))
    assert 'float32 CUDA tensors' in winding._NEEDS and 'requires no gradient' in winding._NEEDS
    assert 'capture' in winding.__doc__ and 'Soft silhouettes' in winding.__doc__


def test_tile_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, 'neural_renderer_amd', 'csrc', 'nr_winding.hip')).read()
    assert int(re.search(r'#define NR_WN_T (\d+)', src).group(1)) == T
    assert int(re.search(r'#define NR_WN_Q (\d+)', src).group(1)) == Q


def test_abi_declares_binds_and_exports_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, 'include', 'nr_hip.h')).read()
    assert all(name in header[:header.index('#define NR_E_')] for name in SYMBOLS)   # the 0.6.0 list of the version comment
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(n for n in re.findall(r'\b(nr_[a-z_0-9]+)\s*\(', header) if n.startswith('nr_winding_'))
    assert declared == set(SYMBOLS)
    assert set(n for n in _lib.SIGNATURES if n.startswith('nr_winding_')) == set(SYMBOLS)
    lib = ctypes.CDLL(_build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.load().nr_version() == 600
    assert os.path.join(_build.HERE, 'csrc', 'nr_winding.hip') in _build.SOURCES


def test_argument_errors_do_not_need_a_device():
    _build.build()
    lib = _lib.load()
    NULL, SIZE, WS, MODE = -1, -2, -3, -4
    fw, bp, bv = lib.nr_winding_forward, lib.nr_winding_backward_points, lib.nr_winding_backward_vertices
    assert fw(None, 1, 1, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
    assert fw(1, None, 1, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
    assert fw(1, 1, None, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
    assert fw(1, 1, 1, None, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
    assert fw(None, 1, 1, 1, 0, 4, 3, 1, 1, 0, None, 0, None) == NULL                  # NULL before sizes
    assert fw(1, 1, 1, 1, 0, 4, 3, 1, 1, 0, None, 0, None) == SIZE
    assert fw(1, 1, 1, 1, 65536, 4, 3, 1, 1, 0, None, 0, None) == SIZE
    assert fw(1, 1, 1, 1, 1, 0, 3, 1, 1, 0, None, 0, None) == SIZE
    assert fw(1, 1, 1, 1, 1, 4, 0, 1, 1, 0, None, 0, None) == SIZE
    assert fw(1, 1, 1, 1, 1, 4, 3, 0, 1, 0, None, 0, None) == SIZE
    assert fw(1, 1, 1, 1, 1, 4, 3, 1, 1, -1, None, 0, None) == SIZE
    assert fw(1, 1, 1, 1, 40000, 40000, 3, 1, 1, 0, None, 0, None) == SIZE                # B N 3 above int32
    assert fw(1, 1, 1, 1, 1, 4, 3, 1, 2, 0, None, 0, None) == MODE                        # points_per_batch is 0 or 1
    assert fw(1, 1, 1, 1, 1, 5000, 3, 5000, 1, 3, None, 0, None) == WS                    # a split call without its workspace
    assert fw(1, 1, 1, 1, 1, 5000, 3, 5000, 1, 3, 1, 8, None) == WS
    assert bp(1, 1, 1, None, 1, 1, 4, 3, 1, 0, None, 0, None) == NULL
    assert bp(1, 1, 1, 1, None, 1, 4, 3, 1, 0, None, 0, None) == NULL
    assert bp(1, 1, 1, 1, 1, 1, 4, 3, 0, 0, None, 0, None) == SIZE
    assert bp(1, 1, 1, 1, 1, 1, 5000, 3, 5000, 2, None, 0, None) == WS
    assert bv(1, 1, 1, None, 1, 1, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL           # no adjacency table
    assert bv(1, 1, 1, 1, 1, None, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
    assert bv(1, 1, 1, 1, 1, 1, None, 1, 4, 3, 1, 1, 0, None, 0, None) == NULL
    assert bv(1, 1, 1, 1, 1, 1, 1, 1, 4, 0, 1, 1, 0, None, 0, None) == SIZE
    assert bv(1, 1, 1, 1, 1, 1, 1, 1, 4, 3, 1, 7, 0, None, 0, None) == MODE
    assert bv(1, 1, 1, 1, 1, 1, 1, 1, 4, 3, 1, 1, 0, None, 0, None) == WS                 # the corner gradients need a workspace
    # a forced split on a very large cloud: more than 2^31 - 1 workgroups along x is a size error, before the workspace
    assert fw(1, 1, 1, 1, 1, 600000000, 3, 2000000, 1, 7000, None, 0, None) == SIZE
    assert bp(1, 1, 1, 1, 1, 1, 600000000, 3, 2000000, 7000, None, 0, None) == SIZE
    assert bv(1, 1, 1, 1, 1, 1, 1, 1, 600000000, 3, 100000000, 1, 7000, None, 0, None) == SIZE
    assert all(lib.nr_winding_workspace_bytes(1, 600000000, 2000000, which, 7000) == 0 for which in (0, 1))
    assert lib.nr_winding_workspace_bytes(1, 600000000, 100000000, 2, 7000) == 0
    size = lib.nr_winding_workspace_bytes
    assert size(1, 5000, 5000, 0, 1) == 0
    tiles = (5000 + T - 1) // T
    assert size(1, 5000, 5000, 0, 3) == tiles * 5000 * 8                                  # a double per point and tile
    assert size(1, 5000, 5000, 1, 3) == 3 * tiles * 5000 * 8
    corners = (5000 * 9 * 4 + 15) // 16 * 16
    assert size(1, 5000, 5000, 2, 1) == corners
    assert size(1, 5000, 5000, 2, 3) == corners + 9 * tiles * 5000 * 8
    assert size(1, 70, 200, 0, 0) == 0                                                    # one tile of faces: nothing to split
    assert size(1, 70, 5000, 0, 0) > 0                                                    # a small call splits by itself
    assert size(64, 8192, 2464, 0, 0) == 0                                                # 1 024 workgroups: the grid fills the machine
    assert size(0, 70, 5000, 0, 0) == 0 and size(1, 70, 5000, 3, 0) == 0 and size(1, 70, 5000, 0, -1) == 0
    assert size(64, 40000, 40000, 0, 7) == 0                                              # tile sums above 256 MiB: not split


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_torch_path_against_the_float64_restatement(k, dtype):
    points, vertices, faces = case(k)
    check_case(points, vertices, faces, dtype, what='torch %s %s' % (SHAPES[k], dtype))


def test_the_restatement_s_gradients_are_its_value_s_differences():
    points, vertices, faces = case(1)
    points, vertices, faces = points[:1, :5], vertices[:1], faces[:40]
    g = np.random.default_rng(0).uniform(-1, 1, (1, 5))
    (gp, _), (gv, _) = R.gradients(points, vertices, faces, g, vertices.shape[1])
    p64, v64, h = points.astype(np.float64), vertices.astype(np.float64), 1e-6
    for idx in ((0, 2, 1), (0, 4, 0)):
        up, down = p64.copy(), p64.copy()
        up[idx] += h
        down[idx] -= h
        fd = ((R.winding(up, v64, faces)[0] - R.winding(down, v64, faces)[0]) * g).sum() / (2 * h)
        assert abs(fd - gp[idx]) <= 1e-7 * max(1.0, abs(fd))
    for idx in ((0, int(faces[3, 1]), 2), (0, int(faces[17, 0]), 0)):
        up, down = v64.copy(), v64.copy()
        up[idx] += h
        down[idx] -= h
        fd = ((R.winding(p64, up, faces)[0] - R.winding(p64, down, faces)[0]) * g).sum() / (2 * h)
        assert abs(fd - gv[idx]) <= 1e-7 * max(1.0, abs(fd))


def test_gradcheck_off_the_surface():
    v, f = sphere(1)
    vertices = R.batch_of(v, 2, 5)
    points = R.shell_points(6, 6, 1.0, 2)
    p, v, f = tensors(points, vertices, f, torch.float64, grad=True)
    assert torch.autograd.gradcheck(lambda a, b: nr.winding_number(a, b, f), (p, v), eps=1e-6, atol=1e-7, rtol=1e-5)
    shared = p[0].detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: nr.winding_number(a, b, f), (shared, v), eps=1e-6, atol=1e-7, rtol=1e-5)
    soft = nr.voxelize(v, f, 3, (-1.3, 1.3), hard=False)      # float32 out: the same gradient as the winding number's
    assert soft.dtype == torch.float32 and tuple(soft.shape) == (2, 3, 3, 3)
    upstream = torch.rand((2, 27), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = torch.autograd.grad((soft.reshape(2, 27) * upstream).sum(), v)[0]
    centers = nr.voxel_centers(3, (-1.3, 1.3), dtype=torch.float64)
    want = torch.autograd.grad((nr.winding_number(centers, v, f) * upstream).sum(), v)[0]
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-9)


def check_pins(device='cpu', implementation=None):
    """the analytic values, within the restatement's bound of them (float32)"""
    def w_of(points, vertices, faces):
        p, v, f = tensors(np.asarray(points, np.float32), np.asarray(vertices, np.float32), np.asarray(faces, np.int32), device=device)
        got = host(nr.winding_number(p, v, f, implementation)).astype(np.float64)
        bnd = R.winding(np.asarray(points, np.float32), np.asarray(vertices, np.float32), np.asarray(faces, np.int32))[1]
        assert bnd.max() <= R.MAX_BOUND
        return got, bnd.reshape(got.shape)

    got, bnd = w_of([[0, 0, 0]], [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 2]])
    assert tuple(got.shape) == (1,) and abs(got[0] - 0.125) <= bnd[0]
    rng = np.random.default_rng(3)
    cv, cf = R.cube(4.0)
    pts = rng.uniform(-8, 8, (2000, 3)).astype(np.float32)
    pts = pts[np.abs(np.abs(pts).max(1) - 4.0) > 0.25]
    inside = (np.abs(pts).max(1) < 4.0).astype(np.float64)
    assert 100 < inside.sum() < len(pts) - 100
    got, bnd = w_of(pts, cv, cf)
    assert (np.abs(got - inside) <= bnd).all()
    got, bnd = w_of(pts, cv, cf[:, ::-1].copy())
    assert (np.abs(got + inside) <= bnd).all()
    for level in range(4):
        sv, sf = sphere(level)
        pts = R.shell_points(40 + level, 300, 1.0, gap=0.3)
        inside = (np.linalg.norm(pts.astype(np.float64), axis=1) < 0.75).astype(np.float64)
        got, bnd = w_of(pts, sv, sf)
        assert (np.abs(got - inside) <= bnd).all(), level
    sv, sf = sphere(2)
    nested_v, nested_f = np.concatenate((sv, 2 * sv)), np.concatenate((sf, sf + len(sv)))
    d = rng.normal(size=(300, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * np.array([0.6, 1.5, 3.0])[np.arange(300) % 3][:, None]).astype(np.float32)
    radius = np.linalg.norm(pts.astype(np.float64), axis=1)
    want = (radius < 1).astype(np.float64) + (radius < 2)
    assert set(want) == {0.0, 1.0, 2.0}
    got, bnd = w_of(pts, nested_v, nested_f)
    assert (np.abs(got - want) <= bnd).all()


def test_analytic_pins():
    check_pins()


def test_cube_in_float64_is_one_or_zero_to_1e_13():
    cv, cf = R.cube(4.0)
    pts = np.random.default_rng(4).uniform(-8, 8, (500, 3))
    pts = pts[np.abs(np.abs(pts).max(1) - 4.0) > 0.25]
    w = nr.winding_number(torch.tensor(pts), torch.tensor(cv, dtype=torch.float64), torch.tensor(cf))
    assert np.abs(host(w) - (np.abs(pts).max(1) < 4.0)).max() <= 1e-13


def hemisphere():
    v, f = sphere()
    return v, f[v[f].mean(1)[:, 2] > 0].copy()


def test_hemisphere_against_the_restatement():
    v, f = hemisphere()
    assert 600 < len(f) < 680
    (w, _, _), _ = check_case(R.shell_points(7, 200, 1.0, 2), R.batch_of(v, 2, 8), f, what='hemisphere')
    assert float(((w > 0.05) & (w < 0.95)).float().mean()) > 0.25   # an open mesh: fractional values


def with_collapsed(vertices, faces):
    """the mesh with faces (a,a,a), (a,b,a), (a,a,b), (a,b,b) by index spliced in, and one collapsed by POSITION only (a, b, a'
    with a' a copy of vertex a appended)"""
    a, b = int(faces[0, 0]), int(faces[0, 1])
    n = vertices.shape[-2]
    v = np.concatenate((vertices, vertices[..., a:a + 1, :]), -2)
    new = np.array([(a, a, a), (a, b, a), (a, a, b), (a, b, b), (a, b, n)], np.int32)
    return v, np.insert(faces, [0, 3, 3, 9, len(faces)], new, axis=0)


def check_collapsed(device='cpu', implementation=None):
    """collapsed faces contribute exactly nothing: the same bits with and without them, also when they hold a point"""
    points, vertices, faces = case(1)
    vc, fc = with_collapsed(vertices, faces)
    points = points.copy()
    points[0, 0] = vertices[0, int(faces[0, 0])]      # a point ON the collapsed faces' vertex: num = den = 0, la = 0
    g = torch.tensor(np.random.default_rng(2).uniform(-1, 1, points.shape[:2]).astype(np.float32), device=device)
    out = []
    for v_np, f_np in ((vertices, faces), (vc, fc)):
        p, v, f = tensors(points, v_np, f_np, device=device, grad=True)
        w = nr.winding_number(p, v, f, implementation)
        gp, gv = torch.autograd.grad((w * g).sum(), [p, v])
        out.append((w, gp, gv))
    (w0, gp0, gv0), (w1, gp1, gv1) = out
    assert torch.isfinite(w0).all() and torch.isfinite(gp0).all() and torch.isfinite(gv0).all()
    assert torch.equal(w0, w1) and torch.equal(gp0, gp1) and torch.equal(gv0, gv1[:, :-1])
    assert float(gv1[:, -1].abs().max()) == 0.0     # the appended vertex belongs to a collapsed face only
    # a mesh of collapsed faces alone is exactly 0 everywhere
    p, v, f = tensors(points, vc, fc[[0, 4]], device=device, grad=True)
    w = nr.winding_number(p, v, f, implementation)
    gp, gv = torch.autograd.grad((w * g).sum(), [p, v])
    assert float(w.detach().abs().max()) == 0.0 and float(gp.abs().max()) == 0.0 and float(gv.abs().max()) == 0.0


def test_collapsed_faces_contribute_exactly_nothing():
    check_collapsed()


def check_point_on_a_vertex(device='cpu', implementation=None):
    """num = den = 0 for the faces around the vertex: Omega = 0 and no gradient from them; the rest as the restatement has it"""
    v, f = sphere(1)
    points = np.stack((v[5], 0.5 * v[5])).astype(np.float32)[None]
    p, vt, ft = tensors(points, v[None], f, device=device, grad=True)
    w = nr.winding_number(p, vt, ft, implementation)
    gp, gv = torch.autograd.grad(w.sum(), [p, vt])
    assert torch.isfinite(w).all() and torch.isfinite(gp).all() and torch.isfinite(gv).all()
    want = R.winding(points, v[None], f)[0]
    touching = (f == 5).any(1)
    rest = R.winding(points, v[None], f[~touching])[0]
    assert abs(want[0, 0] - rest[0, 0]) <= 1e-14          # (the restatement follows the rule)
    assert abs(float(w.detach()[0, 0]) - want[0, 0]) <= 1e-5 and abs(float(w.detach()[0, 1]) - 1.0) <= 1e-5
    (gpr, _), (gvr, _) = R.gradients(points, v[None], f, np.ones((1, 2)), len(v))
    assert np.abs(host(gp) - gpr).max() <= 1e-4 * max(1.0, np.abs(gpr).max())
    assert np.abs(host(gv) - gvr).max() <= 1e-4 * max(1.0, np.abs(gvr).max())


def test_a_point_on_a_vertex():
    check_point_on_a_vertex()


def check_non_finite(device='cpu', implementation=None):
    points, vertices, faces = case(4)
    for bad_value in (float('nan'), float('inf'), -float('inf')):
        p, v, f = tensors(points, vertices, faces, device=device)
        clean = nr.winding_number(p, v, f, implementation)
        v[1, int(faces[7, 2]), 1] = bad_value
        w = nr.winding_number(p, v, f, implementation)
        assert torch.isnan(w[1]).all() and torch.equal(w[0], clean[0]) and torch.equal(w[2], clean[2])
        p2 = p.clone()
        p2[2, 9, 2] = bad_value
        w = nr.winding_number(p2, torch.tensor(vertices, device=device), f, implementation)
        assert torch.isnan(w[2, 9])
        w[2, 9] = clean[2, 9]
        assert torch.equal(w, clean)
        w = nr.winding_number(p2.requires_grad_(True), v.requires_grad_(True), f, implementation)
        w.sum().backward()       # non-finite values flow through without leaving the buffers
        used = torch.tensor(np.unique(faces), device=device).long()
        assert torch.isnan(v.grad[2][used]).all() and torch.isfinite(v.grad[0]).all()


def test_non_finite_coordinates_give_nan():
    check_non_finite()


def check_power_of_two_scaling(device='cpu', implementation=None):
    for k in (1, 4, 6):
        points, vertices, faces = case(k)
        p, v, f = tensors(points, vertices, faces, device=device)
        w = nr.winding_number(p, v, f, implementation)
        for s in (2.0 ** 8, 2.0 ** -8):
            assert torch.equal(w, nr.winding_number(p * s, v * s, f, implementation)), (k, s)


def test_a_scene_scaled_by_a_power_of_two_has_the_same_bits():
    check_power_of_two_scaling()


def test_voxel_centers():
    c = nr.voxel_centers(4)
    assert tuple(c.shape) == (64, 3) and c.dtype == torch.float32
    assert torch.equal(c[(1 * 4 + 2) * 4 + 3], torch.tensor([-0.25, 0.25, 0.75]))
    c = nr.voxel_centers(2, ((0, 1), (10, 14), (-3, -1)), dtype=torch.float64)
    assert torch.equal(c[0], torch.tensor([0.25, 11.0, -2.5], dtype=torch.float64))
    assert torch.equal(c[7], torch.tensor([0.75, 13.0, -1.5], dtype=torch.float64))
    for bad in ((1.0, 1.0), (1.0,), ((0, 1), (0, 1)), 'ab', (0.0, float('inf'))):
        with pytest.raises(ValueError, match='bounds must be'):
            nr.voxel_centers(4, bad)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match='grid_size must be'):
            nr.voxel_centers(bad)


def check_lattice_cube(device='cpu', implementation=None):
    """the cube [-4,4]^3 on the 8^3 grid over [-8,8]^3: the centres are the odd integers, the inner 4^3 block is inside"""
    cv, cf = R.cube(4.0)
    exact = torch.zeros((8, 8, 8))
    exact[2:6, 2:6, 2:6] = 1.0
    v, f = torch.tensor(cv, device=device), torch.tensor(cf, device=device)
    grid = nr.voxelize(v, f, 8, (-8.0, 8.0), implementation=implementation)
    assert tuple(grid.shape) == (8, 8, 8) and grid.dtype == torch.float32 and not grid.requires_grad
    assert torch.equal(grid.cpu(), exact)
    batch = torch.stack((v, 0.5 * v, v + 2.0))
    grids = nr.voxelize(batch, f, 8, ((-8, 8), (-8, 8), (-8, 8)), implementation=implementation).cpu()
    assert tuple(grids.shape) == (3, 8, 8, 8) and torch.equal(grids[0], exact)
    assert float(grids[1].sum()) == 8.0 and torch.equal(grids[2][3:7, 3:7, 3:7], torch.ones((4, 4, 4))) and float(grids[2].sum()) == 64.0
    soft = nr.voxelize(batch.requires_grad_(True), f, 8, (-8.0, 8.0), hard=False, implementation=implementation)
    assert soft.requires_grad and float((soft.detach().cpu()[0] - exact).abs().max()) <= 1e-5
    assert torch.equal(nr.mesh_occupancy(nr.voxel_centers(8, (-8.0, 8.0), device=device), v, f,
                                         implementation=implementation).reshape(8, 8, 8).cpu(), exact.bool())
    iou = nr.voxel_iou(grids.to(device), torch.stack((exact, exact, exact)).to(device)).cpu()
    assert torch.allclose(iou, torch.tensor([1.0, 8.0 / 64.0, 27.0 / 101.0]), rtol=1e-6, atol=0)


def test_voxelize_of_the_lattice_cube_is_the_exact_grid():
    check_lattice_cube()


def test_voxel_iou():
    x = (torch.rand((2, 4, 4, 4), generator=torch.Generator().manual_seed(0)) > 0.5).float()
    assert torch.allclose(nr.voxel_iou(x, x), torch.ones(2), rtol=1e-6, atol=0)
    a = torch.zeros((2, 2, 2))
    b = torch.zeros((2, 2, 2))
    a[0, 0, 0], a[0, 0, 1], b[0, 0, 1], b[1, 1, 1] = 1.0, 0.5, 1.0, 1.0
    # sum ab = 0.5; sum (a + b - ab) = 1 + 1 + 1 = 3
    assert nr.voxel_iou(a, b).dim() == 0 and abs(float(nr.voxel_iou(a, b, eps=0.5)) - 0.5 / 3.5) <= 1e-7
    assert float(nr.voxel_iou(torch.zeros((1, 2, 2, 2)), torch.zeros((1, 2, 2, 2)))) == 0.0
    a.requires_grad_(True)
    nr.voxel_iou(a, b).backward()
    assert float(a.grad.abs().sum()) > 0
    with pytest.raises(ValueError, match='voxel_iou'):
        nr.voxel_iou(a, b[None])


def ball_fraction_left_out(G=16, bounds=(-1.5, 1.5)):
    """voxels of the G^3 grid whose centre is within one voxel diagonal of the unit sphere: (mask of the others, fraction)"""
    c = nr.voxel_centers(G, bounds, dtype=torch.float64).numpy()
    diagonal = np.sqrt(3.0) * (bounds[1] - bounds[0]) / G
    keep = np.abs(np.linalg.norm(c, axis=1) - 1.0) > diagonal
    return keep.reshape(G, G, G), c, 1.0 - keep.mean()


def check_ball(device='cpu', implementation=None):
    keep, c, left_out = ball_fraction_left_out()
    assert left_out <= 0.4, left_out
    v, f = sphere()
    grid = nr.voxelize(torch.tensor(v, device=device), torch.tensor(f, device=device), 16, (-1.5, 1.5), implementation=implementation)
    want = (np.linalg.norm(c, axis=1) < 1.0).reshape(16, 16, 16)
    assert want[keep].sum() > 100 and (~want[keep]).sum() > 100
    assert np.array_equal(host(grid)[keep] == 1.0, want[keep]) and set(np.unique(host(grid))) <= {0.0, 1.0}


def test_voxelize_of_a_sphere_is_the_ball_off_its_surface():
    check_ball()


def check_signed_distance(device='cpu', implementation=None):
    v, f = sphere()
    v64 = v.astype(np.float64)
    n = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    r_in = ((n / np.linalg.norm(n, axis=1, keepdims=True)) * v64[f[:, 0]]).sum(1).min()   # the mesh lies between r_in and 1
    assert 0.99 < r_in < 1.0
    points = R.shell_points(9, 400, 1.0, gap=0.05)
    p, vt, ft = tensors(points, v, f, device=device, grad=True)
    sd = nr.signed_distance(p, vt, ft, implementation)
    radius = np.linalg.norm(points.astype(np.float64), axis=1)
    got = host(sd).astype(np.float64)
    assert tuple(sd.shape) == (400,) and (got < 0).sum() == 200
    assert (got >= radius - 1.0 - 1e-6).all() and (got <= radius - r_in + 1e-6).all()
    gp, gv = torch.autograd.grad(sd.sum(), [p, vt])
    # the gradient is the distance's: a unit vector at every point, pointing away from the surface outside and towards it inside
    assert np.abs(np.linalg.norm(host(gp), axis=1) - 1.0).max() <= 1e-4
    assert ((host(gp) * points).sum(1) > 0).all() and float(gv.abs().sum()) > 0
    # a point on the mesh: distance 0, gradient 0
    on = torch.tensor(v[f[0, 0]][None], device=device).requires_grad_(True)   # (corner 0 of a face: p - v0 = 0 exactly)
    sd = nr.signed_distance(on, vt, ft, implementation)
    g = torch.autograd.grad(sd.sum(), [on, vt])
    assert float(sd.detach()) == 0.0 and float(g[0].abs().sum()) == 0.0 and float(g[1].abs().sum()) == 0.0
    sd = nr.signed_distance(p.detach()[None, :5], torch.stack((vt, 0.5 * vt)), ft, implementation)
    assert tuple(sd.shape) == (2, 5)


def test_signed_distance_of_a_sphere():
    check_signed_distance()


def test_shapes_and_batching():
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces)
    assert tuple(nr.winding_number(p[0], v[0], f).shape) == (63,)
    whole = nr.winding_number(p[0], v, f)
    assert tuple(whole.shape) == (3, 63) and torch.equal(whole, nr.winding_number(p[0:1], v, f))
    assert torch.equal(whole[1], nr.winding_number(p[0], v[1], f))
    assert torch.equal(nr.winding_number(p, v[0], f)[2], nr.winding_number(p[2], v[0], f))
    occ = nr.mesh_occupancy(p, v.requires_grad_(True), f, threshold=0.2)
    assert occ.dtype == torch.bool and not occ.requires_grad and torch.equal(occ, nr.winding_number(p, v, f) > 0.2)
    assert tuple(nr.mesh_occupancy(p[0], v[0], f).shape) == (63,)


def test_validation():
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces)
    with pytest.raises(ValueError, match='points must be a float tensor'):
        nr.winding_number(p[..., :2], v, f)
    with pytest.raises(ValueError, match='vertices must be a float tensor'):
        nr.winding_number(p, v[..., :2], f)
    with pytest.raises(ValueError, match='vertices must be a float tensor'):
        nr.voxelize(v.long(), f, 4)
    with pytest.raises(ValueError, match='faces must be an integer tensor'):
        nr.signed_distance(p, v, f[None])
    with pytest.raises(ValueError, match='share dtype and device'):
        nr.winding_number(p.double(), v, f)
    with pytest.raises(ValueError, match='points have batch size 2, vertices 3'):
        nr.mesh_occupancy(p[:2], v, f)
    with pytest.raises(IndexError):
        nr.winding_number(p, v, f + 1000)
    with pytest.raises(ValueError, match='threshold must be a number'):
        nr.mesh_occupancy(p, v, f, threshold='half')
    with pytest.raises(ValueError, match='grid_size must be'):
        nr.voxelize(v, f, 0)
    for fn in (nr.winding_number, nr.mesh_occupancy, nr.signed_distance):
        with pytest.raises(ValueError, match='implementation must be'):
            fn(p, v, f, implementation='cuda')
    with pytest.raises(ValueError, match='implementation must be'):
        nr.voxelize(v, f, 4, implementation='cuda')


def test_hip_on_cpu_tensors_raises_the_limit_sentence():
    points, vertices, faces = case(0)
    p, v, f = tensors(points, vertices, faces)
    for fn in (nr.winding_number, nr.mesh_occupancy):
        with pytest.raises(ValueError) as err:
            fn(p, v, f, implementation='hip')
        assert winding._NEEDS in str(err.value)
        fn(p, v, f, implementation='torch')
    with pytest.raises(ValueError) as err:
        nr.voxelize(v, f, 2, implementation='hip')
    assert winding._NEEDS in str(err.value)


def test_mesh_methods(tmp_path):
    cv, cf = R.cube(0.5)
    path = str(tmp_path / 'cube.obj')
    with open(path, 'w') as fh:
        fh.write(''.join('v %g %g %g\n' % tuple(p) for p in cv) + ''.join('f %d %d %d\n' % tuple(t + 1) for t in cf))
    mesh = nr.Mesh(path, normalization=False)
    points = torch.tensor([[0.1, 0.2, -0.3], [0.9, 0.0, 0.0]])
    w = mesh.winding_number(points).detach()
    assert torch.equal(w, nr.winding_number(points, mesh.vertices, mesh.faces)) and abs(float(w[0]) - 1) < 1e-5 and abs(float(w[1])) < 1e-5
    grid = mesh.voxelize(4, bounds=(-1.0, 1.0))
    assert tuple(grid.shape) == (4, 4, 4) and float(grid.sum()) == 8.0
    soft = mesh.voxelize(4, hard=False)
    soft.sum().backward()
    assert mesh.vertices.grad is not None and torch.isfinite(mesh.vertices.grad).all()
    sd = mesh.signed_distance(points).detach()
    assert abs(float(sd[0]) + 0.2) < 1e-6 and abs(float(sd[1]) - 0.4) < 1e-6
