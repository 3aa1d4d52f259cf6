"""Vertex colours and smooth shading without a GPU: the entry points' argument checks (include/nr_hip.h
nr_forward_rasterize_corner, nr_backward_corner_colors, nr_vertex_shade_forward / _backward), the input checks of VertexColors,
CornerColors, vertex_shade and Renderer.shading, and the plain-torch vertex_shade against the NumPy restatements in float64."""
import numpy as np
import pytest

import helpers as H
import vertex_ref as R

from neural_renderer_amd import _build, _lib


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    E_NULL, E_SIZE, E_WS, E_MODE = -1, -2, -3, -4

    def fwd(cc=1, faces=1, fim=1, rgb=1, bg=1, B=2, F=8, S=16, ws=None, wsb=0):
        return lib.nr_forward_rasterize_corner(cc, faces, fim, None, None, rgb, None, None, bg, 0, B, F, S, 0.1, 100.0, 0,
                                               ws, wsb, None)
    assert fwd(cc=None) == E_NULL
    assert fwd(rgb=None) == E_NULL
    assert fwd(bg=None) == E_NULL
    assert fwd(faces=None) == E_NULL
    assert fwd(fim=None) == E_NULL
    assert fwd(B=0) == E_SIZE
    assert fwd(F=0) == E_SIZE
    assert fwd(S=0) == E_SIZE
    assert fwd() == E_WS                                             # everything right but the workspace
    assert fwd(ws=1, wsb=lib.nr_forward_workspace_bytes(2, 8, 16) - 1) == E_WS

    def bwd(faces=1, fim=1, wm=1, dm=1, g=1, gc=1, B=2, F=8, S=16, ws=None, wsb=0):
        return lib.nr_backward_corner_colors(faces, fim, wm, dm, g, None, gc, B, F, S, ws, wsb, None)
    for name in ('faces', 'fim', 'wm', 'dm', 'g', 'gc'):
        assert bwd(**{name: None}) == E_NULL, name
    assert bwd(B=0) == E_SIZE
    assert bwd(S=0) == E_SIZE
    need = lib.nr_backward_corner_colors_workspace_bytes(2, 8)
    assert need >= 2 * 8 * (9 * 8 + 1)
    assert lib.nr_backward_corner_colors_workspace_bytes(0, 8) == 0
    assert lib.nr_backward_corner_colors_workspace_bytes(2, 0) == 0
    assert bwd() == E_WS
    assert bwd(ws=1, wsb=need - 1) == E_WS

    light = _lib.Light()

    def vs(v=1, idx=1, col=1, off=1, ent=1, out=1, B=2, Nv=5, Nf=4, Bc=1, smooth=0, light=light, ws=None, wsb=0):
        return lib.nr_vertex_shade_forward(v, idx, col, off, ent, out, B, Nv, Nf, Bc, 0, 1, smooth, light, ws, wsb, None)
    for name in ('v', 'idx', 'col', 'out', 'light'):
        assert vs(**{name: None}) == E_NULL, name
    assert vs(smooth=1, off=None) == E_NULL                          # the table is required in smooth mode ...
    assert vs(smooth=1, ent=None) == E_NULL
    assert vs(smooth=2) == E_MODE
    assert vs(Bc=3) == E_SIZE                                        # colour batch neither 1 nor B
    assert vs(Bc=0) == E_SIZE
    assert vs(B=0) == E_SIZE
    assert vs(Nv=0) == E_SIZE
    assert vs(Nf=0) == E_SIZE
    need = lib.nr_vertex_shade_workspace_bytes(2, 5)
    assert need >= 2 * 5 * 6 * 4
    assert lib.nr_vertex_shade_workspace_bytes(0, 5) == 0
    assert lib.nr_vertex_shade_workspace_bytes(2, 0) == 0
    assert vs(smooth=1) == E_WS
    assert vs(smooth=1, ws=1, wsb=need - 1) == E_WS

    def vb(v=1, idx=1, col=1, off=1, ent=1, g=1, gc=1, gv=1, B=2, Nv=5, Nf=4, Bc=2, smooth=0, light=light, ws=None, wsb=0):
        return lib.nr_vertex_shade_backward(v, idx, col, off, ent, g, gc, gv, B, Nv, Nf, Bc, 0, 1, smooth, light, ws, wsb, None)
    for name in ('v', 'idx', 'col', 'off', 'ent', 'g', 'light'):     # ... and by every backward
        assert vb(**{name: None}) == E_NULL, name
    assert vb(gc=None, gv=None) == E_MODE                            # no gradient asked for
    assert vb(smooth=3) == E_MODE
    assert vb(Bc=3) == E_SIZE
    assert vb(Nv=0) == E_SIZE
    assert vb(smooth=1) == E_WS                                      # grad_vertices in smooth mode needs the scratch
    assert vb(smooth=1, ws=1, wsb=need - 1) == E_WS


def test_vertex_and_corner_colors_reject_bad_tensors():
    import torch
    import neural_renderer_amd as nr
    assert nr.VertexColors(torch.zeros(5, 3)).color_batch == 1
    assert nr.VertexColors(torch.zeros(2, 5, 3)).color_batch == 2
    for bad in (np.zeros((5, 3), np.float32), torch.zeros(5, 3).double(), torch.zeros(5, 4), torch.zeros(5), torch.zeros(1, 2, 5, 3),
                torch.zeros(0, 3)):
        with pytest.raises(ValueError):
            nr.VertexColors(bad)
    assert nr.CornerColors(torch.zeros(2, 8, 3, 3)).colors.shape[1] == 8
    for bad in (np.zeros((2, 8, 3, 3), np.float32), torch.zeros(2, 8, 3, 3).double(), torch.zeros(2, 8, 3), torch.zeros(2, 8, 3, 4),
                torch.zeros(2, 0, 3, 3)):
        with pytest.raises(ValueError):
            nr.CornerColors(bad)
    fn = nr.Rasterize(16, 0.1, 100, 1e-3, (0, 0, 0), return_rgb=True)
    cc = nr.CornerColors(torch.zeros(1, 4, 3, 3))
    with pytest.raises(NotImplementedError):
        fn.forward_gpu((torch.zeros(1, 4, 3, 3), cc))
    with pytest.raises(NotImplementedError):
        fn.backward_gpu((torch.zeros(1, 4, 3, 3), cc), (None,))


def test_vertex_shade_and_renderer_checks():
    import torch
    import neural_renderer_amd as nr
    v, f, c = torch.zeros(2, 5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]]), torch.zeros(5, 3)
    assert tuple(nr.vertex_shade(v, f, c).colors.shape) == (2, 4, 3, 3)
    assert tuple(nr.vertex_shade(v, f[None].expand(2, -1, -1), nr.VertexColors(c), fill_back=False).colors.shape) == (2, 2, 3, 3)
    for args in ((v[0], f, c), (v, f.float(), c), (v, f[None].expand(3, -1, -1), c), (v, f, torch.zeros(4, 3)),
                 (v, f, torch.zeros(3, 5, 3)), (v, f, c.double()), (v.double(), f, c.double())):
        with pytest.raises(ValueError):
            nr.vertex_shade(*args)
    with pytest.raises(ValueError):
        nr.vertex_shade(v, f, c, implementation='hip')               # CPU tensors do not fit the kernels
    with pytest.raises(ValueError):
        nr.vertex_shade(v, f, c, implementation='cuda')
    r = nr.Renderer()
    assert r.shading == 'flat'
    r.shading = 'gouraud'
    with pytest.raises(ValueError, match='shading'):
        r.render(v, f[None].expand(2, -1, -1), nr.VertexColors(c))
    r.shading = 'smooth'
    with pytest.raises(ValueError, match='VertexColors'):
        r.render(v, f[None].expand(2, -1, -1), torch.zeros(2, 2, 2, 2, 2, 3))   # smooth light on cubes: the follow-up
    r.shading = 'flat'
    for bad in (nr.VertexColors(torch.zeros(4, 3)), nr.VertexColors(torch.zeros(3, 5, 3))):
        with pytest.raises(ValueError, match='VertexColors'):
            r.render(v, f[None].expand(2, -1, -1), bad)


def test_adjacency_table():
    from neural_renderer_amd.vertex_colors import build_adjacency
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 9, (2, 30, 3))
    idx[idx == 4] = 5                                                 # vertex 4 has no face
    off, ent = build_adjacency(idx, 10)
    for t in range(2):
        assert off[t, 0] == 0 and off[t, -1] == 90
        for v in range(10):
            e = ent[t, off[t, v]:off[t, v + 1]]
            assert (np.diff(e) > 0).all()
            assert (idx[t].reshape(-1)[e] == v).all()
            assert len(e) == (idx[t] == v).sum()
        assert off[t, 4] == off[t, 5] and off[t, 9] == off[t, 10]
    with pytest.raises(IndexError):
        build_adjacency(idx, 8)


def _mesh(seed, B=2):
    rng = np.random.default_rng(seed)
    v, f = R.icosphere(1)
    v = v[None] + rng.normal(scale=0.05, size=(B,) + v.shape)
    v = np.concatenate((v, rng.normal(size=(B, 1, 3))), axis=1)     # one vertex without a face
    col = rng.uniform(0.1, 1, (B if seed % 2 else 1, v.shape[1], 3))
    r32 = lambda x: np.asarray(x, np.float32).astype(np.float64)    # (the torch path takes the light's vectors as float32)
    L = R.Light(0.3, 0.8, r32((1.0, 0.9, 0.8)), r32((0.7, 1.0, 0.6)), r32(rng.normal(size=3) / 1.7))
    return rng, v, f, col, L


@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('fill_back', [False, True])
@pytest.mark.parametrize('seed', range(2))
def test_torch_vertex_shade_equals_restatement_in_float64(seed, fill_back, smooth):
    """vertex_shade_torch in float64 against shade64, and its autograd gradients against shade_adjoint64.  Both evaluate the
    same formulas in double with other groupings; every output is a product of a colour and a light built from at most
    3 (cross) + 5 (norm) + 5 (dot) + 3 (light) + 1 operations plus the normal sum over the faces of a vertex (6 here):
    gamma_32 in double, relative to the term magnitudes (the light is a sum of positive terms, so its own size).
    Measured: forward 2.8e-16; gradients within 0.09 of the bound."""
    import torch
    from neural_renderer_amd.vertex_colors import vertex_shade_torch
    rng, v, f, col, L = _mesh(seed)
    want = R.shade64(v, f, col, L, fill_back, smooth)
    vt = torch.tensor(v, requires_grad=True)
    ct = torch.tensor(col if col.shape[0] > 1 else col[0], requires_grad=True)
    got = vertex_shade_torch(vt, torch.tensor(f), ct, fill_back=fill_back, smooth=smooth, **L.kwargs())
    bound = H.gamma(32, H.UD)
    err = np.abs(got.detach().numpy() - want)
    print('torch vs restatement, float64: forward max diff %.3e' % err.max())
    assert (err <= bound * np.abs(want).max()).all()
    assert (got.detach().numpy()[:, :, :, :] >= 0).all()
    g = rng.normal(size=want.shape)
    got.backward(torch.tensor(g))
    gc, gc_mag, gv, gv_mag = R.shade_adjoint64(v, f, col if col.shape[0] > 1 else col[0], L, fill_back, smooth, g)
    worst_c = (np.abs(ct.grad.numpy() - gc) / (bound * gc_mag + 1e-300)).max()
    worst_v = (np.abs(vt.grad.numpy() - gv) / (bound * gv_mag + 1e-300)).max()
    print('torch vs restatement, float64: grad_colors %.3f, grad_vertices %.3f of the bound' % (worst_c, worst_v))
    assert worst_c <= 1 and worst_v <= 1
    # the vertex without a face: ambient light only would show in a face, which it has none of; its gradients are zero
    assert not vt.grad.numpy()[:, -1].any() and not ct.grad.numpy()[..., -1, :].any()


def test_finite_differences_of_the_restatement():
    """shade_adjoint64's grad_vertices against central differences of shade64 (float64 against float64): the step and the
    tolerance that tests/test_vertex_colors_gpu.py uses for the kernels come from here.  h = 1e-6 on unit-size geometry:
    truncation ~ h^2 |f'''| ~ 1e-12, rounding ~ u_d |loss| / h ~ 1e-9.  Measured: max |fd - analytic| = 1.3e-10 of the largest
    gradient entry; FD_TOL = 1e-7 leaves room for other meshes."""
    for smooth in (False, True):
        rng, v, f, col, L = _mesh(3)
        g = rng.normal(size=(v.shape[0], 2 * len(f), 3, 3))
        _, _, gv, _ = R.shade_adjoint64(v, f, col, L, True, smooth, g)
        fd = fd_vertices(v, f, col, L, True, smooth, g, [(0, 0), (1, 5), (1, 17), (0, 30)])
        for (b, i), d in fd.items():
            err = np.abs(d - gv[b, i]).max() / np.abs(gv).max()
            print('finite differences (smooth=%s) vertex %s: %.3e' % (smooth, (b, i), err))
            assert err <= FD_TOL


FD_STEP, FD_TOL = 1e-6, 1e-7


def fd_vertices(v, f, col, L, fill_back, smooth, g, which):
    out = {}
    for b, i in which:
        d = np.zeros(3)
        for c in range(3):
            vp, vm = v.copy(), v.copy()
            vp[b, i, c] += FD_STEP
            vm[b, i, c] -= FD_STEP
            d[c] = ((R.shade64(vp, f, col, L, fill_back, smooth) - R.shade64(vm, f, col, L, fill_back, smooth)) * g).sum() \
                / (2 * FD_STEP)
        out[(b, i)] = d
    return out


def test_smooth_restatement_on_a_sphere_is_lambert():
    """On a unit icosphere the area-weighted vertex normal is the vertex itself up to the discretisation: the smooth light at a
    vertex is the Lambert term of its position (the formula, not the arithmetic, is checked here)."""
    v, f = R.icosphere(3)
    assert len(f) == 1280
    n = np.cross(v[f[:, 0]] - v[f[:, 1]], v[f[:, 2]] - v[f[:, 1]])
    sign = np.sign((n * v[f].mean(1)).sum(1))
    assert (sign == sign[0]).all()                                    # consistently oriented
    L = R.Light(0.0, 1.0, (1, 1, 1), (1, 1, 1), (0.0, 0.6, 0.8))
    out = R.shade64(v[None], f, np.ones((len(v), 3)), L, True, True)
    vis = out[0, :1280] if sign[0] > 0 else out[0, 1280:][:, ::-1]    # the copy whose normal points outwards
    want = np.maximum(v[f] @ L.dir, 0)
    # the faces around a vertex tilt by about an edge length h = 0.16 from its direction; the symmetric part cancels in the
    # sum, what is left is second order, h^2 / 2 = 0.013 (measured 0.0118)
    assert np.abs(vis[:, :, 0] - want).max() < 2e-2
