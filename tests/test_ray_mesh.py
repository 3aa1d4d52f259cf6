"""Ray casting without a GPU (neural_renderer_amd/ray_mesh.py): the public names, the C ABI's argument checks, and the plain-torch
path -- the kernels' second yardstick -- against the float64 restatement of tests/ray_ref.py within its derived bounds, in
float32 and float64: t, ids, weights and the three gradients, miss rows, the exact lattice, collapsed faces, non-finite input,
near and far, any-hit against first-hit, gradcheck, the camera's rays, vertex visibility, the rasterizer cross-check's cap
established in float64 against the oracle's rasterizer, validation and the Mesh methods."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import neural_renderer
import neural_renderer_amd as nr
from neural_renderer_amd import _build, _lib, ray_mesh

import point_mesh_ref as PM
import ray_ref as R

NAMES = ('ray_mesh_intersect', 'ray_mesh_occluded', 'vertex_visibility', 'camera_rays')
# (B, R, F, rays shared by the batch): those of tests/test_point_mesh.py -- one pair, a wave, a tile and a split each crossed
# with a remainder
SHAPES = ((1, 1, 1, False), (2, 63, 255, False), (3, 257, 65, False), (2, 1027, 515, True), (3, 1, 515, False),
          (1, 70, 5000, False))
SYMBOLS = ('nr_ray_mesh_workspace_bytes', 'nr_ray_mesh_first_hit', 'nr_ray_mesh_any_hit')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def case(k):
    """-> (origins, directions, vertices [B,Nv,3], faces) float32 / int32 NumPy arrays of SHAPES[k] (shared, not to be changed)"""
    B, N, F, shared = SHAPES[k]
    vertices, faces = PM.grid_mesh(200 + k, B, F)
    origins, directions = R.rays(400 + k, vertices, faces, N, shared)
    return origins, directions, vertices, faces


@functools.lru_cache(maxsize=None)
def analysis(k, dtype=torch.float32):
    """the restatement's (ids, ambiguous) of case k, computed once"""
    o, d, v, f = case(k)
    return R.analyse(o, d, v, f, u=R.U if dtype == torch.float32 else R.U64, B=SHAPES[k][0])


def tensors(origins, directions, vertices, faces, dtype=torch.float32, device='cpu', grad=False):
    o, d, v = (torch.tensor(t, dtype=dtype, device=device) for t in (origins, directions, vertices))
    if grad:
        for t in (o, d, v):
            t.requires_grad_(True)
    return o, d, v, torch.tensor(faces, device=device)


def host(t):
    return t.detach().cpu().numpy()


def upstream(shape, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def check_gradients(grads, ids, g, origins, directions, vertices, faces, u, what=''):
    """grads = (grad_origins, grad_directions, grad_vertices) of sum g t against the restatement; rays shared by the batch sum
    over it.  -> the three worst ratios"""
    (go, bo), (gd, bd), (gv, bv) = R.gradients(origins, directions, vertices, faces, ids, g, u)
    if np.asarray(origins).ndim == 2:
        (go, bo), (gd, bd) = R.shared_sum(go, bo, 0, u), R.shared_sum(gd, bd, 0, u)
        go, bo, gd, bd = go[0], bo[0], gd[0], bd[0]
    ratios = [PM._ratio(np.abs(host(got).astype(np.float64) - want), bnd)
              for got, want, bnd in zip(grads, (go, gd, gv), (bo, bd, bv))]
    print('%s gradient ratios: origins %.4f directions %.4f vertices %.4f' % ((what,) + tuple(ratios)))
    assert all(np.isfinite(host(t)).all() for t in grads), what
    assert max(ratios) <= 1.0, (what, ratios)
    return ratios


def check_case(k, dtype=torch.float32, device='cpu', implementation=None, what=''):
    """ray_mesh_intersect and its three gradients on case k, for per-ray upstream gradients that differ per image, against
    the restatement -> (t, ids, w) as NumPy arrays"""
    origins, directions, vertices, faces = case(k)
    u = R.U if dtype == torch.float32 else R.U64
    o, d, v, f = tensors(origins, directions, vertices, faces, dtype, device, grad=True)
    t, ids, w = nr.ray_mesh_intersect(o, d, v, f, implementation=implementation)
    assert ids.dtype == torch.int64 and t.dtype == dtype and w.dtype == dtype
    assert not ids.requires_grad and not w.requires_grad and t.requires_grad
    R.check_hits(host(t), host(ids), host(w), origins, directions, vertices, faces, u=u, what=what, analysis=analysis(k, dtype))
    g = upstream(tuple(t.shape))
    grads = torch.autograd.grad(t, [o, d, v], torch.tensor(g, dtype=dtype, device=device))
    check_gradients(grads, host(ids), g, origins, directions, vertices, faces, u, what)
    return host(t), host(ids), host(w)


# ---------------------------------------------------------------------------------------------------------------------

def test_public_names():
    for name in NAMES:
        assert name in nr.__all__
        assert getattr(neural_renderer, name) is getattr(nr, name) is getattr(ray_mesh, name)
    assert callable(nr.Mesh.cast_rays) and callable(nr.Mesh.visible_vertices)


def test_abi_declares_binds_and_exports_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, 'include', 'nr_hip.h')).read()
    assert all(name in header.split('argument errors')[0] for name in SYMBOLS)   # the header's list of entry points
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(n for n in re.findall(r'\b(nr_[a-z_0-9]+)\s*\(', header) if n.startswith('nr_ray_mesh_'))
    assert declared == set(SYMBOLS)
    assert set(n for n in _lib.SIGNATURES if n.startswith('nr_ray_mesh_')) == set(SYMBOLS)
    lib = ctypes.CDLL(_build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.load().nr_version() == 600 == _lib.NR_VERSION


def test_argument_errors_do_not_need_a_device():
    _build.build()
    lib = _lib.load()
    NULL, SIZE, MODE, WS = -1, -2, -4, -3
    inf = math.inf

    def first(*a):   # (origins, directions, vertices, faces, t, ids, bary, B, R, Nv, F, per_batch, near, far, cull, split)
        return lib.nr_ray_mesh_first_hit(*a, None, 0, None)

    def any_hit(*a):
        return lib.nr_ray_mesh_any_hit(*a, None, 0, None)

    ok = (1, 4, 3, 1, 1, 0.0, inf, 0, 0)
    for k in range(7):
        ptrs = [1] * 7
        ptrs[k] = None
        assert first(*ptrs, *ok) == NULL, k
    for k in range(5):
        ptrs = [1] * 5
        ptrs[k] = None
        assert any_hit(*ptrs, *ok) == NULL, k
    for fn, n in ((first, 7), (any_hit, 5)):
        p = [1] * n
        assert fn(*p, 0, 4, 3, 1, 1, 0.0, inf, 0, 0) == SIZE
        assert fn(*p, 65536, 4, 3, 1, 1, 0.0, inf, 0, 0) == SIZE
        assert fn(*p, 1, 0, 3, 1, 1, 0.0, inf, 0, 0) == SIZE
        assert fn(*p, 1, 4, 0, 1, 1, 0.0, inf, 0, 0) == SIZE
        assert fn(*p, 1, 4, 3, 0, 1, 0.0, inf, 0, 0) == SIZE
        assert fn(*p, 1, 4, 3, 1, 1, 0.0, inf, 0, -1) == SIZE
        assert fn(*p, 40000, 40000, 3, 1, 1, 0.0, inf, 0, 0) == SIZE     # B R 3 above int32
        assert fn(*p, 1, 4, 3, 1, 2, 0.0, inf, 0, 0) == MODE            # rays_per_batch
        assert fn(*p, 1, 4, 3, 1, 1, 0.0, inf, 2, 0) == MODE            # cull
        assert fn(*p, 1, 4, 3, 1, 1, math.nan, inf, 0, 0) == MODE
        assert fn(*p, 1, 4, 3, 1, 1, 0.0, math.nan, 0, 0) == MODE
        assert fn(*p, 1, 5000, 3, 5000, 1, 0.0, inf, 0, 3) == WS        # a split call without its workspace
    # a forced split on a very large bundle: more than 2^31 - 1 workgroups along x is a size error, before the workspace
    big = (1, 600000000, 3, 2000000, 1, 0.0, inf, 0, 7000)
    assert first(*[1] * 7, *big) == SIZE and any_hit(*[1] * 5, *big) == SIZE
    assert lib.nr_ray_mesh_workspace_bytes(1, 600000000, 2000000, 0, 7000) == 0
    assert first(*[1] * 7, 1, 600000000, 3, 2000000, 1, 0.0, inf, 0, 1000) == WS    # (1.2e9 workgroups: the workspace is asked for)
    wb = lib.nr_ray_mesh_workspace_bytes
    assert wb(1, 5000, 5000, 0, 1) == 0 and wb(1, 5000, 5000, 1, 1) == 0
    assert wb(1, 5000, 5000, 0, 3) == 3 * 5000 * 8 and wb(1, 5000, 5000, 1, 3) == 3 * 5000 * 4
    assert wb(1, 70, 5000, 0, 0) > 0          # (1, 70, 5000) splits its faces by itself
    assert wb(1, 70, 200, 0, 0) == 0          # one tile of faces: nothing to split
    assert wb(0, 70, 5000, 0, 0) == 0
    assert wb(64, 8192, 2464, 0, 0) == 0      # 1 024 workgroups: the grid fills the machine


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_torch_path_against_the_float64_restatement(k, dtype):
    check_case(k, dtype, what='torch %s %s' % (SHAPES[k], dtype))


def test_about_two_thirds_of_the_rays_hit_and_few_are_ambiguous():
    for k in (1, 2, 3, 5):
        ids, amb = analysis(k)
        assert 0.55 <= float((ids >= 0).mean()) <= 0.8 and float(amb.mean()) <= R.CAP, (k, (ids >= 0).mean(), amb.mean())


def check_miss_rows(device='cpu', implementation=None):
    origins, directions, vertices, faces = case(2)
    o, d, v, f = tensors(origins, directions, vertices, faces, device=device, grad=True)
    t, ids, w = nr.ray_mesh_intersect(o, d, v, f, implementation=implementation)
    miss = ids < 0
    assert int(miss.sum()) > 10 and torch.isposinf(t[miss]).all() and (w[miss] == 0).all()
    go, gd, gv = torch.autograd.grad(t, [o, d, v], torch.ones_like(t))   # (the upstream reaches the miss rows as well)
    assert (go[miss] == 0).all() and (gd[miss] == 0).all()
    assert all(torch.isfinite(x).all() for x in (go, gd, gv))
    # an image none of whose rays hits: its vertices get exact zeros
    away = o.detach().clone()
    away[0, :, 2] = 5.0
    away_d = d.detach().clone()
    away_d[0] = torch.tensor((0.0, 0.0, 1.0))
    t, ids, w = nr.ray_mesh_intersect(away, away_d, v, f, implementation=implementation)
    assert (ids[0] < 0).all() and (ids[1] >= 0).any()
    gv = torch.autograd.grad(torch.where(ids >= 0, t, torch.zeros_like(t)).sum(), v)[0]
    assert (gv[0] == 0).all() and float(gv[1].abs().sum()) > 0 and torch.isfinite(gv).all()


def test_miss_rows_give_exact_zeros():
    check_miss_rows()


# ---------------------------------------------------------------------------------------------------------------------
# the lattice

def lattice_rays():
    """Integer origins in [-6,6]^3 and axis or diagonal directions with entries in {0, +-1, +-2}: 400 rays"""
    rng = np.random.default_rng(7)
    origins = rng.integers(-6, 7, (400, 3)).astype(np.float32)
    directions = rng.integers(-1, 2, (400, 3)).astype(np.float32)
    directions[(directions == 0).all(1)] = (0.0, 0.0, 1.0)
    directions *= rng.choice((1.0, 2.0), (400, 1)).astype(np.float32)
    # rays through vertices and edges of the cube, on purpose
    origins[:6] = ((0, 0, -6), (4, 4, -6), (0, 4, -6), (-6, 0, 0), (2, 2, -6), (-6, -6, -6))
    directions[:6] = ((0, 0, 1), (0, 0, 1), (0, 0, 2), (1, 0, 0), (0, 0, 1), (1, 1, 1))
    return origins, directions


def lattice_expectation(origins, directions, vertices, faces, near, far, cull):
    """The definition evaluated in float64 -- exact on the lattice -- without margins: (t, ids, hits [R,F])"""
    v0, v1, v2 = PM.corners(vertices, faces, 0)
    tm = R.pair_terms(origins[:, None].astype(np.float64), directions[:, None].astype(np.float64), v0[None], v1[None], v2[None])
    s = np.where(tm['det'] < 0, -1.0, 1.0)
    D, Uq, Vq, Tq = np.abs(tm['det']), s * tm['u'], s * tm['v'], s * tm['T']
    inside = (D > 0) & (Uq >= 0) & (Vq >= 0) & (Uq + Vq <= D)
    if cull:
        inside &= tm['det'] > 0
    t = Tq / np.where(D > 0, D, 1.0)
    hits = inside & (t >= near) & (t < far)
    t = np.where(hits, t, np.inf)
    # every determinant is 0 or a power of two times +-1, so every quotient is exact in float32 as well
    assert set(np.unique(D)) <= {0.0, 16.0, 32.0, 64.0}
    return t.min(1), np.where(np.isfinite(t.min(1)), t.argmin(1), -1), hits


def check_lattice(device='cpu', implementation=None):
    _, vertices, faces = PM.lattice()
    origins, directions = lattice_rays()
    o, d, v, f = tensors(origins, directions, vertices, faces, device=device)
    t_want, id_want, hits = lattice_expectation(origins, directions, vertices, faces, 0.0, np.inf, False)
    # rays through shared edges and vertices: more than one face at the first t; ray 0 meets the middle vertex of a side
    t_all = np.where(hits, lattice_t(origins, directions, vertices, faces), np.inf)
    tied = ((t_all == t_want[:, None]) & hits).sum(1)
    assert int((tied > 1).sum()) >= 40 and tied[0] == 6 and id_want[0] == np.flatnonzero(hits[0])[0]
    t, ids, w = nr.ray_mesh_intersect(o, d, v, f, implementation=implementation)
    assert tuple(t.shape) == (400,) and np.array_equal(host(t).astype(np.float64), t_want)
    assert np.array_equal(host(ids), id_want)
    assert 150 <= int((id_want >= 0).sum()) < 400
    # cull_backfaces, by hand: the lattice builds both sides across an axis with the same winding, n = e1 x e2 = +16 along that
    # axis for all 16 of them, and det = -d . n.  A direction with m non-zero entries has 16 m candidate faces (D > 0), and
    # det > 0 on the 16 of every axis along which it runs backwards; a direction and its reverse halve the candidates between
    # them.  A ray that runs backwards along no axis hits nothing when culled.
    v0, v1, v2 = PM.corners(vertices, faces, 0)
    det = R.pair_terms(origins[:, None].astype(np.float64), directions[:, None].astype(np.float64), v0[None], v1[None], v2[None])['det']
    assert np.array_equal((det != 0).sum(1), 16 * (directions != 0).sum(1))
    assert np.array_equal((det > 0).sum(1), 16 * (directions < 0).sum(1))
    tc_want, idc_want, hits_c = lattice_expectation(origins, directions, vertices, faces, 0.0, np.inf, True)
    assert np.array_equal(hits_c, hits & (det > 0)) and 0 < hits_c.sum() < hits.sum()
    tc, idc, wc = nr.ray_mesh_intersect(o, d, v, f, cull_backfaces=True, implementation=implementation)
    assert np.array_equal(host(tc).astype(np.float64), tc_want) and np.array_equal(host(idc), idc_want)
    forwards = (directions >= 0).all(1)
    assert int(forwards.sum()) > 20 and (idc_want[forwards] == -1).all() and (id_want[forwards] >= 0).any()
    # the reversed rays, culled, over all t: together with the culled rays they see every face the unculled rays see
    hits_all = lattice_expectation(origins, directions, vertices, faces, -np.inf, np.inf, False)[2]
    hits_fwd = lattice_expectation(origins, directions, vertices, faces, -np.inf, np.inf, True)[2]
    hits_rev = lattice_expectation(origins, -directions, vertices, faces, -np.inf, np.inf, True)[2]
    assert np.array_equal(hits_all, hits_fwd | hits_rev) and not (hits_fwd & hits_rev).any()
    # near and far: a hit at exactly near counts, a hit at exactly far does not
    k = int(np.argmax(np.isfinite(t_want) & (t_want > 0)))
    tk = float(t_want[k])
    one = (o[k:k + 1], d[k:k + 1], v, f)
    above = float(np.nextafter(np.float32(tk), np.float32(np.inf)))
    assert float(nr.ray_mesh_intersect(*one, near=tk, implementation=implementation)[0]) == tk
    assert float(nr.ray_mesh_intersect(*one, far=tk, implementation=implementation)[0]) == math.inf
    assert float(nr.ray_mesh_intersect(*one, near=above, implementation=implementation)[0]) > tk
    assert float(nr.ray_mesh_intersect(*one, far=above, implementation=implementation)[0]) == tk
    for near, far in ((0.5, 2.0), (1.0, 1.5), (-3.0, 0.0)):
        tw, iw, _ = lattice_expectation(origins, directions, vertices, faces, near, far, False)
        t2, i2, _ = nr.ray_mesh_intersect(o, d, v, f, near=near, far=far, implementation=implementation)
        assert np.array_equal(host(t2).astype(np.float64), tw) and np.array_equal(host(i2), iw)
        occ = nr.ray_mesh_occluded(o, d, v, f, near=near, far=far, implementation=implementation)
        assert np.array_equal(host(occ), iw >= 0)


def lattice_t(origins, directions, vertices, faces):
    v0, v1, v2 = PM.corners(vertices, faces, 0)
    tm = R.pair_terms(origins[:, None].astype(np.float64), directions[:, None].astype(np.float64), v0[None], v1[None], v2[None])
    return np.where(tm['det'] < 0, -1.0, 1.0) * tm['T'] / np.where(tm['det'] != 0, np.abs(tm['det']), 1.0)


def test_lattice_is_exact():
    check_lattice()


# ---------------------------------------------------------------------------------------------------------------------

def check_collapsed(device='cpu', implementation=None):
    """collapsed faces are never hit, and the others' results are unchanged to the bit"""
    vertices, faces = PM.collapsed_faces()
    rng = np.random.default_rng(8)
    origins = rng.uniform(-1.2, 1.2, (1, 97, 3)).astype(np.float32)
    directions = rng.normal(size=(1, 97, 3)).astype(np.float32)
    t, ids, w = nr.ray_mesh_intersect(*tensors(origins, directions, vertices, faces, device=device), implementation=implementation)
    assert (ids == -1).all() and torch.isposinf(t).all() and (w == 0).all()
    base_v, base_f = PM.grid_mesh(31, 2, 199)
    mixed_v, mixed_f = PM.with_collapsed(base_v, base_f)
    origins, directions = R.rays(32, base_v, base_f, 300)
    t0, i0, w0 = nr.ray_mesh_intersect(*tensors(origins, directions, base_v, base_f, device=device), implementation=implementation)
    t1, i1, w1 = nr.ray_mesh_intersect(*tensors(origins, directions, mixed_v, mixed_f, device=device), implementation=implementation)
    spliced = np.array([not any((row == base).all() for base in base_f) for row in mixed_f])
    assert int(spliced.sum()) == 6
    old_number = np.cumsum(~spliced) - 1          # the number a face of the mixed mesh had before
    assert not spliced[host(i1)[host(i1) >= 0]].any()
    assert torch.equal(t0, t1) and torch.equal(w0, w1)
    assert np.array_equal(host(i0), np.where(host(i1) >= 0, old_number[np.maximum(host(i1), 0)], -1))
    assert int((i0 >= 0).sum()) > 150


def test_collapsed_faces_are_never_hit():
    check_collapsed()


def check_non_finite(device='cpu', implementation=None):
    origins, directions, vertices, faces = case(1)
    F = faces.shape[0]
    bad = vertices.copy()
    bad[:, 5] = np.nan
    touched = (faces == 5).any(1)
    keep = np.flatnonzero(~touched)
    o, d, v, f = tensors(origins, directions, bad, faces, device=device)
    t, ids, w = nr.ray_mesh_intersect(o, d, v, f, implementation=implementation)
    assert int(ids.min()) >= -1 and int(ids.max()) < F and not torch.isnan(t).any() and not torch.isnan(w).any()
    assert not touched[host(ids)[host(ids) >= 0]].any()
    # a NaN vertex removes its faces only: the same as the mesh without them, to the bit
    t2, i2, w2 = nr.ray_mesh_intersect(o, d, torch.tensor(vertices, device=device), torch.tensor(faces[keep], device=device),
                                       implementation=implementation)
    assert torch.equal(t, t2) and torch.equal(w, w2)
    assert np.array_equal(host(ids), np.where(host(i2) >= 0, keep[np.maximum(host(i2), 0)], -1))
    for value in (np.inf, -np.inf):
        bad[:, 5] = value
        ti, ii, wi = nr.ray_mesh_intersect(o, d, torch.tensor(bad, device=device), f, implementation=implementation)
        assert torch.equal(ti, t) and torch.equal(ii, ids) and torch.equal(wi, w)
    # a NaN ray is a miss
    on = o.clone()
    dn = d.clone()
    on[0, 3, 1] = float('nan')
    dn[1, 7, 2] = float('nan')
    dn[1, 8] = float('inf')
    v = torch.tensor(vertices, device=device)
    t, ids, w = nr.ray_mesh_intersect(on, dn, v, f, implementation=implementation)
    assert int(ids[0, 3]) == -1 and int(ids[1, 7]) == -1 and int(ids[1, 8]) == -1 and torch.isposinf(t[0, 3]) and (w[1, 7] == 0).all()
    assert int(ids.min()) >= -1 and int(ids.max()) < F and not torch.isnan(t).any()
    occ = nr.ray_mesh_occluded(on, dn, v, f, implementation=implementation)
    assert not bool(occ[0, 3]) and not bool(occ[1, 7]) and not bool(occ[1, 8])
    on.requires_grad_(True)
    v.requires_grad_(True)
    t = nr.ray_mesh_intersect(on, dn, v, f, implementation=implementation)[0]
    torch.where(torch.isfinite(t), t, torch.zeros_like(t)).sum().backward()
    assert torch.isfinite(v.grad).all() and (on.grad[0, 3] == 0).all()


def test_non_finite_input():
    check_non_finite()


def check_any_hit(device='cpu', implementation=None):
    for k in (1, 2, 3, 5):
        origins, directions, vertices, faces = case(k)
        o, d, v, f = tensors(origins, directions, vertices, faces, device=device)
        ids = nr.ray_mesh_intersect(o, d, v, f, implementation=implementation)[1]
        occ = nr.ray_mesh_occluded(o, d, v, f, implementation=implementation)
        assert occ.dtype == torch.bool and occ.shape == ids.shape
        keep = ~analysis(k)[1]
        assert np.array_equal(host(occ)[keep], (host(ids) >= 0)[keep]) and keep.mean() >= 1 - R.CAP
        assert np.array_equal(host(occ)[keep], (analysis(k)[0] >= 0)[keep])


def test_any_hit_equals_first_hit():
    check_any_hit()


def test_gradcheck_away_from_edges():
    vertices, faces = PM.grid_mesh(41, 2, 7)
    origins, directions = R.rays(42, vertices, faces, 6)
    ids, amb = R.analyse(origins, directions, vertices, faces, u=1e-3 / R.KN)   # a margin of 1e-3 relative to the magnitudes
    assert not amb.any() and (ids >= 0).sum() >= 6
    o, d, v, f = tensors(origins, directions, vertices, faces, torch.float64, grad=True)

    def t_of(a, b, c):
        t = nr.ray_mesh_intersect(a, b, c, f)[0]
        return torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    assert torch.autograd.gradcheck(t_of, (o, d, v), eps=1e-7, atol=1e-6, rtol=1e-5)
    # a second derivative simply works: plain torch
    t = t_of(o, d, v)
    first = torch.autograd.grad(t.sum(), v, create_graph=True)[0]
    second = torch.autograd.grad((first ** 2).sum(), d)[0]
    assert torch.isfinite(second).all() and float(second.abs().sum()) > 0
    assert torch.autograd.gradgradcheck(t_of, (o, d, v), eps=1e-7, atol=1e-5, rtol=1e-4)


def test_shapes_and_batching():
    origins, directions, vertices, faces = case(1)
    o, d, v, f = tensors(origins, directions, vertices, faces)
    t, ids, w = nr.ray_mesh_intersect(o[0], d[0], v[0], f)
    assert tuple(t.shape) == (63,) and tuple(ids.shape) == (63,) and tuple(w.shape) == (63, 3)
    assert tuple(nr.ray_mesh_occluded(o[0], d[0], v[0], f).shape) == (63,)
    whole = nr.ray_mesh_intersect(o, d, v, f)
    assert torch.equal(whole[0][0], t) and torch.equal(whole[1][0], ids) and torch.equal(whole[2][0], w)
    # rays shared by the batch as [R,3] and [1,R,3]; vertices shared by the batch
    shared = nr.ray_mesh_intersect(o[0], d[0], v, f)
    assert tuple(shared[0].shape) == (2, 63) and torch.equal(shared[0][0], t)
    assert all(torch.equal(a, b) for a, b in zip(shared, nr.ray_mesh_intersect(o[0:1], d[0:1], v, f)))
    assert torch.equal(nr.ray_mesh_intersect(o, d, v[0], f)[0][0], t)
    # one origin [3] for all rays, and one per image [B,3]
    eye = torch.tensor((0.1, -0.2, 1.5))
    single = nr.ray_mesh_intersect(eye, d, v, f)
    assert all(torch.equal(a, b) for a, b in zip(single, nr.ray_mesh_intersect(eye.expand(2, 63, 3), d, v, f)))
    eyes = torch.tensor(((0.1, -0.2, 1.5), (0.3, 0.2, -1.1)))
    per_image = nr.ray_mesh_intersect(eyes, d, v, f)
    assert all(torch.equal(a, b) for a, b in zip(per_image, nr.ray_mesh_intersect(eyes[:, None].expand(2, 63, 3), d, v, f)))
    # a learnable single origin and learnable shared rays collect their gradients
    eye.requires_grad_(True)
    shared_d = d[0].clone().requires_grad_(True)
    t = nr.ray_mesh_intersect(eye, shared_d, v, f)[0]
    torch.where(torch.isfinite(t), t, torch.zeros_like(t)).sum().backward()
    assert tuple(eye.grad.shape) == (3,) and float(eye.grad.abs().sum()) > 0 and tuple(shared_d.grad.shape) == (63, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the camera's rays

def make_renderer(mode, S=8):
    renderer = nr.Renderer()
    renderer.camera_mode, renderer.image_size = mode, S
    renderer.eye = [1.2, 0.7, -2.3]
    renderer.camera_direction = [-0.4, -0.2, 0.9]
    renderer.viewing_angle = 25
    return renderer


@pytest.mark.parametrize('mode', ('look_at', 'look'))
def test_camera_rays_land_on_the_pixel_centres(mode):
    S, B = 8, 2
    renderer = make_renderer(mode, S)
    like = torch.zeros(1)
    origins, directions = nr.camera_rays(renderer, B, like)
    assert tuple(origins.shape) == (B, 3) and tuple(directions.shape) == (B, S * S, 3) and directions.dtype == torch.float32
    t = torch.tensor(np.random.default_rng(3).uniform(1.0, 5.0, (B, S * S)), dtype=torch.float32)
    points = origins[:, None] + t[..., None] * directions
    cam = nr.look_at(points, renderer.eye) if mode == 'look_at' else nr.look(points, renderer.eye, renderer.camera_direction)
    ndc = nr.perspective(cam, renderer.viewing_angle)
    centre = (2.0 * np.arange(S) + 1 - S) / S
    rows, cols = np.divmod(np.arange(S * S), S)
    want_x, want_y = centre[cols], centre[S - 1 - rows]      # the top row of an image is the largest y
    # float rounding: the world coordinates |o| + t |d| carry ~u each through ~16 operations; x and y are divided by z tan
    tan = math.tan(25 / 180. * 3.1416)
    size = float(origins.abs().sum(1).max()) + host(t) * host(directions.abs().sum(2))
    tol = 16 * R.U * size
    assert (np.abs(host(ndc[..., 2]) - host(t)) <= tol).all()
    assert (np.abs(host(ndc[..., 0]) - want_x[None]) <= tol / (host(t) * tan) + 4 * R.U).all()
    assert (np.abs(host(ndc[..., 1]) - want_y[None]) <= tol / (host(t) * tan) + 4 * R.U).all()
    # another raster through image_size; float64 through `like`; the other modes raise
    o2, d2 = nr.camera_rays(renderer, 1, torch.zeros(1, dtype=torch.float64), image_size=3)
    assert tuple(d2.shape) == (1, 9, 3) and d2.dtype == torch.float64 and o2.dtype == torch.float64
    renderer.camera_mode = 'projection'
    with pytest.raises(ValueError, match="camera_mode must be 'look_at' or 'look'"):
        nr.camera_rays(renderer, 1, like)
    renderer.camera_mode = mode
    renderer.perspective = False
    with pytest.raises(ValueError, match='perspective'):
        nr.camera_rays(renderer, 1, like)
    # a batched eye (or direction) must match batch_size
    renderer.perspective = True
    renderer.eye = torch.tensor(((1.2, 0.7, -2.3), (0.0, 0.5, -2.0), (1.0, 1.0, 1.0)))
    assert tuple(nr.camera_rays(renderer, 3, like)[0].shape) == (3, 3)
    with pytest.raises(ValueError, match=r'Renderer.eye must be \[3\] or \[batch size, 3\] with batch size 2'):
        nr.camera_rays(renderer, 2, like)
    if mode == 'look':
        renderer.eye = [1.2, 0.7, -2.3]
        renderer.camera_direction = torch.tensor(((0.0, 0.0, 1.0),) * 3)
        with pytest.raises(ValueError, match='Renderer.camera_direction must be'):
            nr.camera_rays(renderer, 2, like)


def cross_check_scenes():
    """-> [(name, vertices [Nv,3] float32, faces [F,3] int32)]: icosphere(2) and the teapot of tests/golden"""
    v, f = nr.icosphere(2, 0.5)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_fixtures.npz'))
    tv = g['teapot_vertices_raw'].astype(np.float32).copy()
    tv -= tv.min(0)[None, :]
    tv /= np.abs(tv).max()
    tv *= 2
    tv -= tv.max(0)[None, :] / 2
    return [('icosphere', host(v).astype(np.float32), host(f).astype(np.int32)), ('teapot', tv, g['teapot_faces'].astype(np.int32))]


CROSS_EYES = [nr.get_points_from_angles(2.732, 30.0, az) for az in (0.0, 100.0, 215.0)]


def cross_check_renderer(S=32):
    renderer = nr.Renderer()
    renderer.image_size, renderer.anti_aliasing, renderer.fill_back = S, False, True
    renderer.eye = torch.tensor(CROSS_EYES, dtype=torch.float32)
    return renderer


def test_float64_rays_agree_with_the_oracle_rasterizer_within_the_cap():
    """What tests/test_ray_mesh_gpu.py relies on, established without the product's kernels: the oracle's float32 rasterizer
    against the restatement's float64 first hits along float64 camera rays, on the scenes and eyes of the GPU test."""
    from oracle import oracle as O
    S, B = 32, len(CROSS_EYES)
    renderer = cross_check_renderer(S)
    like = torch.zeros(1, dtype=torch.float64)
    origins, directions = (host(t) for t in nr.camera_rays(renderer, B, like))
    rot = host(nr.camera_rotation(renderer, B, like))
    tangent = math.tan(np.float32(30.0) / np.float32(180.0) * np.float32(3.1416))
    for name, v, f in cross_check_scenes():
        vertices = np.repeat(v[None], B, 0)
        ref = O.Renderer()
        ref.image_size, ref.anti_aliasing, ref.eye = S, False, np.array(CROSS_EYES, np.float32)
        depth = ref.render_depth(vertices, np.repeat(f[None], B, 0))
        ids, amb = R.analyse(origins[:, None], directions, vertices, f, near=renderer.near, far=renderer.far, u=R.U64, B=B)
        t64, _, b_t, _ = R.pair_values(origins[:, None], directions, vertices, f, ids, R.U64)
        t64 = np.where(ids >= 0, t64, np.inf)
        share, worst = R.check_depth_maps(depth, t64, ids, b_t, origins[:, None], directions, vertices, f, CROSS_EYES, rot, tangent, S,
                                          renderer.far, what='oracle rasterizer against float64 rays, %s' % name)
        assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------

def check_visibility(device='cpu', implementation=None):
    v, f = nr.icosphere(3, 0.7, device=device)
    # (eyes off the sphere's symmetry axes: from an axis whole families of segments pass exactly through far edges, which are
    # not watertight)
    eyes = torch.tensor(((0.3, -0.2, -3.0), (2.0, 1.0, 1.5)), device=device)
    vis = nr.vertex_visibility(v, f, eyes, implementation=implementation)
    assert vis.dtype == torch.bool and tuple(vis.shape) == (2, v.shape[0])
    assert torch.equal(nr.vertex_visibility(v, f, eyes[0], implementation=implementation), vis[0])
    # A vertex of a convex polyhedron is seen from the eye iff the segment does not enter the cone of the faces around it:
    # iff n . (eye - v) > 0 for the outward normal n of at least ONE of those faces (with the sphere's own normal at v in place
    # of the faces' the horizon would be a band as wide as an edge, 9 % of this sphere).  Vertices whose largest cosine is
    # within the margin of 0 are left out.
    vn, fn, en = host(v).astype(np.float64), host(f), host(eyes).astype(np.float64)
    n = np.cross(vn[fn[:, 1]] - vn[fn[:, 0]], vn[fn[:, 2]] - vn[fn[:, 0]])
    n *= np.sign((n * vn[fn].mean(1)).sum(1))[:, None] / np.linalg.norm(n, axis=1)[:, None]
    to_eye = en[:, None] - vn[None]
    to_eye /= np.linalg.norm(to_eye, axis=2, keepdims=True)
    cosine = np.full((2, vn.shape[0]), -np.inf)
    for k in range(3):
        np.maximum.at(cosine, (slice(None), fn[:, k]), (to_eye[:, fn[:, k]] * n[None]).sum(2))
    keep = np.abs(cosine) > 1e-3
    print('vertex visibility: left out %.4f, seen %.3f' % (float((~keep).mean()), float(host(vis).mean())))
    assert float((~keep).mean()) <= R.CAP and np.array_equal(host(vis)[keep], (cosine > 0)[keep])
    assert 0.3 < float(host(vis).mean()) < 0.5
    return vis


def test_vertex_visibility_on_a_sphere():
    check_visibility()


def test_validation():
    origins, directions, vertices, faces = case(1)
    o, d, v, f = tensors(origins, directions, vertices, faces)
    with pytest.raises(ValueError, match='directions must be a float tensor'):
        nr.ray_mesh_intersect(o, d[..., :2], v, f)
    with pytest.raises(ValueError, match='origins must be a float tensor'):
        nr.ray_mesh_intersect(o.long(), d, v, f)
    with pytest.raises(ValueError, match='do not match directions'):
        nr.ray_mesh_intersect(o[:, :5], d, v, f)
    with pytest.raises(ValueError, match='origins have batch size 3, directions 2'):
        nr.ray_mesh_intersect(torch.cat((o, o[:1])), d, v, f)
    with pytest.raises(ValueError, match='rays have batch size 3, vertices 2'):
        nr.ray_mesh_occluded(torch.cat((o, o[:1])), torch.cat((d, d[:1])), v, f)
    with pytest.raises(ValueError, match='vertices must be a float tensor'):
        nr.ray_mesh_intersect(o, d, v[..., :2], f)
    with pytest.raises(ValueError, match='faces must be an integer tensor'):
        nr.ray_mesh_intersect(o, d, v, f[None])
    with pytest.raises(ValueError, match='share dtype and device'):
        nr.ray_mesh_intersect(o.double(), d, v, f)
    with pytest.raises(ValueError, match='share dtype and device'):
        nr.ray_mesh_intersect(o.double(), d.double(), v, f)
    with pytest.raises(IndexError):
        nr.ray_mesh_intersect(o, d, v, f + 1000)
    with pytest.raises(ValueError, match='near must be a number'):
        nr.ray_mesh_intersect(o, d, v, f, near=float('nan'))
    with pytest.raises(ValueError, match='far must be a number'):
        nr.ray_mesh_occluded(o, d, v, f, far='1')
    with pytest.raises(ValueError, match='implementation must be'):
        nr.ray_mesh_intersect(o, d, v, f, implementation='cuda')
    with pytest.raises(ValueError, match='eye must be'):
        nr.vertex_visibility(v, f, torch.zeros(4))


def test_hip_on_cpu_tensors_raises_the_limit_sentence():
    o, d, v, f = tensors(*case(0))
    for fn in (nr.ray_mesh_intersect, nr.ray_mesh_occluded):
        with pytest.raises(ValueError) as err:
            fn(o, d, v, f, implementation='hip')
        assert ray_mesh._NEEDS in str(err.value)
        fn(o, d, v, f, implementation='torch')
    with pytest.raises(ValueError) as err:
        nr.vertex_visibility(v, f, torch.zeros(3), implementation='hip')
    assert ray_mesh._NEEDS in str(err.value)


def test_the_sweep_is_chunked(monkeypatch):
    """never the whole [B,R,F] matrix at once"""
    origins, directions, vertices, faces = case(3)
    o, d, v, f = tensors(origins, directions, vertices, faces)
    whole = nr.ray_mesh_intersect(o, d, v, f)
    sizes = []
    pair = ray_mesh._pair_torch
    monkeypatch.setattr(ray_mesh, '_pair_torch', lambda *a, **k: (sizes.append(a[0].shape[1]), pair(*a, **k))[1])
    monkeypatch.setattr(ray_mesh, '_CHUNK_ELEMENTS', 2 * 515 * 12 * 100)
    chunked = nr.ray_mesh_intersect(o, d, v, f)
    assert sizes[:-1] == [100] * 10 + [27] and all(torch.equal(a, b) for a, b in zip(whole, chunked))


def test_mesh_methods(tmp_path):
    import point_loss_ref
    v, f = point_loss_ref.octahedron()
    path = str(tmp_path / 'octa.obj')
    with open(path, 'w') as fh:
        fh.write(''.join('v %g %g %g\n' % tuple(p) for p in v) + ''.join('f %d %d %d\n' % tuple(t + 1) for t in f))
    mesh = nr.Mesh(path, normalization=False)
    origins = torch.tensor(((0.1, 0.2, -3.0), (0.1, 0.2, 3.0), (5.0, 5.0, -3.0)))
    directions = torch.tensor(((0.0, 0.0, 1.0), (0.0, 0.0, -2.0), (0.0, 0.0, 1.0)))
    t, ids, w = mesh.cast_rays(origins, directions)
    want = nr.ray_mesh_intersect(origins, directions, mesh.vertices, mesh.faces)
    assert tuple(t.shape) == (3,) and torch.equal(t, want[0]) and torch.equal(ids, want[1]) and int(ids[2]) == -1
    t[:2].sum().backward()
    assert mesh.vertices.grad is not None and float(mesh.vertices.grad.abs().sum()) > 0
    vis = mesh.visible_vertices(torch.tensor((0.0, 0.0, -5.0)))
    assert vis.dtype == torch.bool and tuple(vis.shape) == (6,)
    assert torch.equal(vis, nr.vertex_visibility(mesh.vertices, mesh.faces, torch.tensor((0.0, 0.0, -5.0))))
    assert torch.equal(mesh.cast_rays(origins, directions, far=1.0)[1], torch.tensor((-1, -1, -1)))
