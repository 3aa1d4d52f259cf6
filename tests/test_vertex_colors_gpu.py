"""Vertex colours and smooth shading on the GPU (include/nr_hip.h nr_forward_rasterize_corner / nr_backward_corner_colors,
nr_vertex_shade_forward / _backward; VertexColors, CornerColors, Renderer.shading): the rasterizer's corner mode bit for bit
against the NumPy restatement and against the cube path where they must coincide, its adjoint, vertex shading in both
directions against the restatements, the renderer's paths, what smooth shading is for (a sphere), a fit and graph capture."""
import numpy as np
import pytest

import helpers as H
import vertex_ref as R

pytestmark = pytest.mark.gpu

EPS = 1e-3
BG = (0.1, 0.2, 0.3)


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device='cuda', requires_grad=grad)


# ---------------------------------------------------------------------------------------------------------------------
# the rasterizer's corner mode

def _scene(seed):
    """A fuzz scene as tests/test_uv_pixel_gpu.py's: random triangles, fill_back on or off, B = 1..3, odd and
    non-power-of-two rasters; nine random numbers per face (the reversed copies carry their own)."""
    rng = np.random.default_rng(700 + seed)
    B = int(rng.integers(1, 4))
    Nf = int(rng.integers(20, 120))
    fill_back = bool(seed % 2)
    S = int(rng.choice([37, 50, 64, 96]))
    faces = H.random_scene(rng, B, Nf, size=0.4)
    if fill_back:
        faces = np.ascontiguousarray(np.concatenate((faces, faces[:, :, ::-1]), axis=1))
    F = faces.shape[1]
    corner = rng.uniform(0, 1.2, (B, F, 3, 3)).astype(np.float32)
    return dict(rng=rng, B=B, S=S, F=F, faces=faces, corner=corner)


def _run(sc, exact=False, g_rgb=None, alpha=True, depth=True):
    import neural_renderer_amd as nr
    fn = nr.Rasterize(sc['S'], 0.1, 100, EPS, BG, return_rgb=True, return_alpha=alpha, return_depth=depth)
    fn.exact_gradient = exact
    faces = _cuda(sc['faces'], True)
    corner = _cuda(sc['corner'], True)
    rgb, a, d = fn(faces, nr.CornerColors(corner))
    if g_rgb is not None:
        rgb.backward(_cuda(g_rgb))
    return fn, rgb, a, d, faces, corner


def _maps(fn):
    return tuple(m.detach().cpu().numpy() for m in (fn.face_index_map, fn.weight_map, fn.depth_map))


@pytest.mark.parametrize('seed', range(8))
def test_forward_equals_restatement_and_cube_geometry(seed):
    import neural_renderer_amd as nr
    sc = _scene(seed)
    fn, rgb, alpha, depth, _, _ = _run(sc)
    fi, wm, dm = _maps(fn)
    assert (fi >= 0).any()
    want = R.corner_render(sc['faces'], fi, wm, dm, sc['corner'], BG)
    assert np.array_equal(rgb.detach().cpu().numpy(), want)
    # alpha, depth and the face index map are the cube path's on the same faces
    tex = _cuda(sc['rng'].uniform(0, 1, (sc['B'], sc['F'], 2, 2, 2, 3)).astype(np.float32))
    fc = nr.Rasterize(sc['S'], 0.1, 100, EPS, BG, return_rgb=True, return_alpha=True, return_depth=True)
    _, a2, d2 = fc(_cuda(sc['faces']), tex)
    assert np.array_equal(fc.face_index_map.cpu().numpy(), fi)
    assert np.array_equal(a2.cpu().numpy(), alpha.detach().cpu().numpy())
    assert np.array_equal(d2.cpu().numpy(), depth.detach().cpu().numpy())


def _adjoint_check(sc, fn, corner, g):
    fi, wm, dm = _maps(fn)
    want, mag = R.corner_adjoint(sc['faces'], fi, wm, dm, g, sc['F'])
    got = corner.grad.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= 1e-6 * mag).all()
    # faces that own no pixel: exact zeros
    owned = np.zeros((sc['B'], sc['F']), bool)
    b, y, x = np.nonzero(fi >= 0)
    owned[b, fi[b, y, x]] = True
    assert (~owned).any() and not got[~owned].any()
    return fi


@pytest.mark.parametrize('seed', range(8))
def test_adjoint(seed):
    sc = _scene(seed)
    g = sc['rng'].normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    fn, _, _, _, _, corner = _run(sc, g_rgb=g)
    _adjoint_check(sc, fn, corner, g)


def test_adjoint_two_large_faces():
    """Two faces that own more than 5 000 pixels each (and small ones, some hidden behind them): thousands of terms per sum."""
    rng = np.random.default_rng(4)
    S = 128
    faces = H.random_scene(rng, 1, 30, size=0.2, zmin=2.0, zmax=3.0)
    faces[0, 0] = [[-0.95, -0.9, 1.2], [0.9, -0.95, 1.5], [-0.9, 0.95, 1.1]]
    faces[0, 1] = [[0.95, 0.9, 1.3], [-0.85, 0.97, 1.6], [0.93, -0.9, 1.2]]
    for f in (0, 1):  # (either orientation may be the visible one: keep the one the rasterizer draws)
        p = faces[0, f]
        if (p[2, 1] - p[0, 1]) * (p[1, 0] - p[0, 0]) < (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0]):
            faces[0, f] = p[::-1].copy()
    sc = dict(rng=rng, B=1, S=S, F=30, faces=np.ascontiguousarray(faces), corner=rng.uniform(0, 1, (1, 30, 3, 3)).astype(np.float32))
    g = rng.normal(size=(1, S, S, 3)).astype(np.float32)
    fn, _, _, _, _, corner = _run(sc, g_rgb=g)
    fi = _adjoint_check(sc, fn, corner, g)
    assert int((fi == 0).sum()) > 5000 and int((fi == 1).sum()) > 5000


@pytest.mark.parametrize('exact', [False, True])
def test_grad_faces_is_the_rasterizers_own(exact):
    """grad_faces bit for bit what nr_backward_rasterize_lit(NULL, ..., grad_textures = NULL) gives on the same rgb_map."""
    import torch
    from neural_renderer_amd import _lib
    for seed in (1, 2):
        sc = _scene(seed)
        B, S, F = sc['B'], sc['S'], sc['F']
        g = sc['rng'].normal(size=(B, S, S, 3)).astype(np.float32)
        fn, rgb, _, _, faces, _ = _run(sc, exact=exact, g_rgb=g, alpha=False, depth=False)
        lib = _lib.load()
        gf = torch.empty_like(faces)
        wsb = lib.nr_backward_workspace_bytes(B, F, S, 1, 0)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device='cuda')
        gd = _cuda(g)
        _lib.check(lib.nr_backward_rasterize_lit(
            None, fn.faces.data_ptr(), None, fn.face_index_map.data_ptr(), fn.weight_map.data_ptr(), fn.depth_map.data_ptr(),
            rgb.detach().contiguous().data_ptr(), None, gd.data_ptr(), None, None, gf.data_ptr(), None, B, F, S, 2, EPS,
            _lib.NR_FLAG_EXACT_GRADIENT if exact else 0, None, ws.data_ptr(), wsb,
            torch.cuda.current_stream().cuda_stream), 'nr_backward_rasterize_lit')
        torch.cuda.synchronize()
        assert torch.equal(faces.grad, gf)


def test_reproducible():
    """Faces of up to 1 024 candidate pixels are gathered in a fixed order (the same bits by construction); larger ones are
    summed with double atomics (wave-level pre-reduction, then a rounding pass), the scheme of nr_backward_uv_images: those
    double additions arrive in no fixed order, the sums rounded to float gave the same bits in every run measured -- the
    statement tests/test_uv_pixel_gpu.py::test_reproducible makes, checked the same way.  The scene has faces of both kinds."""
    sc = _scene(3)
    g = sc['rng'].normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    runs = []
    for _ in range(2):
        fn, rgb, _, _, faces, corner = _run(sc, g_rgb=g)
        runs.append([rgb.detach(), faces.grad, corner.grad])
    for a, b in zip(*runs):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# coincidence with the cube path

def _teapot(B, size, anti_aliasing=True):
    import torch
    import neural_renderer_amd as nr
    v, f = H.teapot()
    vertices = torch.tensor(v, device='cuda')[None].expand(B, -1, -1).contiguous()
    faces = torch.tensor(f, device='cuda')[None].expand(B, -1, -1).contiguous()
    r = nr.Renderer()
    r.image_size = size
    r.anti_aliasing = anti_aliasing
    r.eye = torch.tensor(np.stack([nr.get_points_from_angles(2.732, 30.0, 360.0 * i / B) for i in range(B)]),
                         dtype=torch.float32, device='cuda')
    return r, vertices, faces


def test_flat_constant_colour_is_the_cube_path():
    """All vertex colours = c, flat shading: Renderer.render against the cube path on textures = c with face_light.  Same
    geometry kernels, so the maps are bit-equal.  rgb: the cube path forms sum_taps w_t c (the trilinear weights sum to 1
    within their own roundings) times light; this mode forms ((c light) d0 + (c light) d1) + (c light) d2 with d_k carrying
    the roundings of zp / z_k, the product and the clamp.  From the operation count: gamma_16 |c light| per pixel.
    Measured on the MI355X: max |diff| 2.98e-7, the worst pixel at 0.43 of its bound."""
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import frontend
    B, S = 8, 128
    r, vertices, faces = _teapot(B, S, anti_aliasing=False)
    c = torch.tensor([0.7, 0.4, 0.9], device='cuda')
    colors = c[None].expand(vertices.shape[1], 3).contiguous()
    tex = c.expand(B, faces.shape[1], 2, 2, 2, 3).contiguous()
    r.face_light = True
    cube = r.render(vertices, faces, tex)
    vc = r.render(vertices, faces, nr.VertexColors(colors))
    assert r.last_frontend == 'fused'
    covered = r.render_silhouettes(vertices, faces) > 0
    assert int(covered.sum()) > 10000
    err = (vc - cube).abs()
    bound = float(H.gamma(16)) * cube.abs()
    worst = float((err / bound.clamp_min(1e-30))[covered[:, None].expand_as(err)].max())
    print('flat vertex colours vs cube path: max |diff| = %.3e, worst diff / (gamma_16 |c light|) = %.3f'
          % (float(err.max()), worst))
    assert torch.equal(vc[~covered[:, None].expand_as(vc)], cube[~covered[:, None].expand_as(vc)])
    assert worst <= 1.0
    # coverage, alpha and depth: the rasterizer on the same projected faces
    pf, light = frontend.project_and_light_colors(r, vertices, faces)
    corner = nr.vertex_shade(vertices, faces, colors, fill_back=True, smooth=False)
    a = nr.rasterize_rgbad(pf, corner, S, False, r.near, r.far, r.rasterizer_eps, r.background_color)
    b = nr.rasterize_rgbad(pf, tex, S, False, r.near, r.far, r.rasterizer_eps, r.background_color, face_light=light)
    assert torch.equal(a['alpha'], b['alpha']) and torch.equal(a['depth'], b['depth'])
    assert torch.equal(a['rgb'], vc)


# ---------------------------------------------------------------------------------------------------------------------
# vertex shading

def _mesh(seed, B=3, shared_colors=False, per_image_topology=False):
    """A jittered icosphere (320 faces) plus a vertex without a face and a face whose three vertices coincide (zero normal)."""
    rng = np.random.default_rng(900 + seed)
    v, f = R.icosphere(2)
    n0 = len(v)
    v = v[None] + rng.normal(scale=0.03, size=(B,) + v.shape)
    extra = rng.normal(size=(B, 4, 3))
    extra[:, 2] = extra[:, 1]
    extra[:, 3] = extra[:, 1]
    v = np.concatenate((v, extra), axis=1).astype(np.float32)      # n0: no face; n0 + 1 .. n0 + 3: one point
    f = np.concatenate((f, [[n0 + 1, n0 + 2, n0 + 3]]), axis=0).astype(np.int32)
    if per_image_topology:
        f = np.stack([f[rng.permutation(len(f))][:, rng.permutation(3)] for _ in range(B)])
    col = rng.uniform(0.1, 1, (1 if shared_colors else B, v.shape[1], 3)).astype(np.float32)
    r32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    L = R.Light(0.3, 0.8, r32((1.0, 0.9, 0.8)), r32((0.7, 1.0, 0.6)), r32(rng.normal(size=3) / 1.7))
    return rng, v, f, col, L, n0


def _shade(v, f, col, L, fill_back, smooth, implementation='hip', grad=False):
    import neural_renderer_amd as nr
    vt, ct = _cuda(v, grad), _cuda(col[0] if col.shape[0] == 1 else col, grad)
    out = nr.vertex_shade(vt, _cuda(f), ct, fill_back=fill_back, smooth=smooth, implementation=implementation, **L.kwargs())
    return out.colors, vt, ct


@pytest.mark.parametrize('fill_back', [False, True])
@pytest.mark.parametrize('seed', range(3))
def test_flat_forward_is_bit_equal(seed, fill_back):
    """Flat: the restatement bit for bit, and colors[v] * light with the light colours of nr_frontend_forward_light."""
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import frontend
    rng, v, f, col, L, n0 = _mesh(seed, shared_colors=bool(seed % 2))
    got, vt, ct = _shade(v, f, col, L, fill_back, False)
    assert np.array_equal(got.cpu().numpy(), R.shade32(v, f, col, L, fill_back, False))
    r = nr.Renderer()
    r.fill_back = fill_back
    r.light_intensity_ambient, r.light_intensity_directional = L.ia, L.id
    r.light_color_ambient, r.light_color_directional, r.light_direction = L.ca.tolist(), L.cd.tolist(), L.dir.tolist()
    idx = _cuda(f)[None].expand(v.shape[0], -1, -1).contiguous()
    _, light = frontend.project_and_light_colors(r, vt, idx)
    Nf = len(f)
    cf = (ct if ct.dim() == 3 else ct[None].expand(v.shape[0], -1, -1))[torch.arange(v.shape[0], device='cuda')[:, None, None],
                                                                         idx.long()]
    want = cf * light[:, :Nf, None, :]
    if fill_back:
        want = torch.cat((want, torch.flip(cf * light[:, Nf:, None, :], dims=[2])), dim=1)
    assert torch.equal(got, want)


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('seed', range(3))
def test_smooth_forward_against_restatement(seed, per_image):
    """Smooth: the restatement sums the face normals in the kernels' ascending (face, corner) order, every other operation is
    the flat path's, so the bits should agree; the bound, should they not, is gamma_(n + 16) of the light for n faces around
    a vertex.  `per_image`: an index tensor [B,Nf,3] with another face order and corner rotation per image gets one table per
    image.  Also: a zero normal sum gives the ambient light only, and two runs give the same bits."""
    rng, v, f, col, L, n0 = _mesh(seed, shared_colors=bool(seed % 2), per_image_topology=per_image)
    got, _, _ = _shade(v, f, col, L, True, True)
    again, _, _ = _shade(v, f, col, L, True, True)
    want = R.shade32(v, f, col, L, True, True)
    got = got.cpu().numpy()
    diff = np.abs(got.astype(np.float64) - want)
    print('smooth forward vs restatement: bit-equal %s, max diff %.3e' % (np.array_equal(got, want), diff.max()))
    assert (diff <= H.gamma(7 + 16) * np.abs(want)).all()
    assert np.array_equal(got, want)   # measured on the MI355X: the same bits
    assert np.array_equal(got, again.cpu().numpy())
    # the degenerate face (last; its vertices n0 + 1 .. n0 + 3 have a zero normal sum): colour * ambient, front and back
    B, Nf = v.shape[0], f.shape[-2]
    fl = f if f.ndim == 3 else np.broadcast_to(f, (B,) + f.shape)
    amb = (np.float32(L.ia) * L.ca.astype(np.float32))
    for b in range(B):
        k = int(np.nonzero((fl[b] > n0).all(1))[0][0])
        c = np.broadcast_to(col, (B,) + col.shape[1:])[b][fl[b, k]]
        assert np.array_equal(got[b, k], c * amb) and np.array_equal(got[b, Nf + k], (c * amb)[::-1])


# grad_colors: a double sum of float products of a gradient and a light colour that carries <= 16 float roundings (the
# normal sum of <= 7 faces included), rounded once: gamma_24 of the term magnitudes.  grad_vertices: a float32 chain of
# cross product (3), norm (6), dot (5), the light's backward (8), normalize's backward (9) and two cross products (6) per
# term, summed over <= 7 faces around a vertex, in smooth mode twice (the normal sum's gradient is gathered from three
# vertices: + 3): 37 + 7 + 10 <= 64 roundings, against magnitudes that propagate absolute values: gamma_64.
GAMMA_COLORS, GAMMA_VERTICES = 24, 64


@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('seed', range(4))
def test_backward_against_adjoint_and_finite_differences(seed, smooth):
    """Both gradients entry by entry against the float64 adjoint's term magnitudes; grad_vertices also against central
    differences of the float64 restatement (step and tolerance from tests/test_vertex_colors.py, where they are measured
    float64 against float64) at vertices whose n . direction is away from the relu's kink; a vertex without a face gets zeros;
    colours shared by the batch get the sum over the batch."""
    from test_vertex_colors import FD_TOL, fd_vertices
    fill_back = seed % 2 == 0
    rng, v, f, col, L, n0 = _mesh(seed, shared_colors=seed >= 2, per_image_topology=seed == 3)
    F = (2 if fill_back else 1) * f.shape[-2]
    g = rng.normal(size=(v.shape[0], F, 3, 3)).astype(np.float32)
    out, vt, ct = _shade(v, f, col, L, fill_back, smooth, grad=True)
    out.backward(_cuda(g))
    gc, gc_mag, gv, gv_mag = R.shade_adjoint64(v, f, col[0] if col.shape[0] == 1 else col, L, fill_back, smooth, g)
    got_c, got_v = ct.grad.cpu().numpy().astype(np.float64), vt.grad.cpu().numpy().astype(np.float64)
    wc = (np.abs(got_c - gc) / (H.gamma(GAMMA_COLORS) * gc_mag + 1e-300)).max()
    wv = (np.abs(got_v - gv) / (H.gamma(GAMMA_VERTICES) * gv_mag + 1e-300)).max()
    # measured on the MI355X: grad_colors <= 0.102 and grad_vertices <= 0.020 of their bounds
    print('vertex shading backward (smooth=%s, seed %d): grad_colors %.3f, grad_vertices %.3f of their bounds' % (smooth, seed, wc, wv))
    assert wc <= 1 and wv <= 1
    assert (gv != 0).any() and (gc != 0).any()
    # the vertex without a face
    assert not got_v[:, n0].any() and not got_c[..., n0, :].any()
    # shared colours: the sum over the batch of what per-image colours receive
    if col.shape[0] == 1:
        colB = np.broadcast_to(col, (v.shape[0],) + col.shape[1:]).copy()
        outB, _, ctB = _shade(v, f, colB, L, fill_back, smooth, grad=True)
        outB.backward(_cuda(g))
        per = ctB.grad.cpu().numpy().astype(np.float64)
        assert (np.abs(got_c - per.sum(0)) <= H.gamma(GAMMA_COLORS) * gc_mag + np.spacing(np.abs(per).sum(0).astype(np.float32))).all()
    # finite differences of the float64 restatement, away from the kink
    if f.ndim == 2:
        fv = np.stack([v[b][f] for b in range(v.shape[0])]).astype(np.float64)
        nrm = np.cross(fv[:, :, 0] - fv[:, :, 1], fv[:, :, 2] - fv[:, :, 1])
        nrm /= np.linalg.norm(nrm, axis=2, keepdims=True) + 1e-12
        away = np.ones(v.shape[:2], bool)                            # vertices all of whose faces are away from the kink
        for k in range(3):
            np.logical_and.at(away, (np.arange(v.shape[0])[:, None], f[None, :, k]), np.abs(nrm @ L.dir) > 0.05)
        away[:, n0:] = False
        pick = [tuple(p) for p in np.argwhere(away)[:: max(1, int(away.sum()) // 5)][:5]]
        assert len(pick) >= 3
        col64 = (col[0] if col.shape[0] == 1 else col).astype(np.float64)
        fd = fd_vertices(v.astype(np.float64), f, col64, L, fill_back, smooth, g.astype(np.float64), pick)
        for (b, i), d in fd.items():
            tol = FD_TOL * np.abs(gv).max() + H.gamma(GAMMA_VERTICES) * gv_mag[b, i]
            assert (np.abs(got_v[b, i] - d) <= tol).all(), (b, i)


def test_fused_and_torch_paths_agree_through_the_renderer():
    """Renderer.render with vertex colours, both shadings, look_at and projection cameras: the fused path (HIP vertex shading
    and front-end) against the torch path (a tensor light direction keeps both off the kernels).  The torch front-end projects
    with other roundings, so edge pixels may see another face: the upstream gradient is zeroed where the two renders differ
    by more than 1e-5, as in tests/test_uv_pixel_gpu.py.  Gradients reach vertices and colours on both paths."""
    import torch
    import neural_renderer_amd as nr
    B, S = 2, 64
    v, f = R.icosphere(2)
    rng = np.random.default_rng(21)
    v = (v * np.array([1.0, 0.7, 0.8]) + rng.normal(scale=0.02, size=v.shape)).astype(np.float32)
    vertices = _cuda(np.stack([v, v * 0.9]), True)
    faces = _cuda(f)[None].expand(B, -1, -1).contiguous()
    colors = _cuda(rng.uniform(0.2, 1, (len(v), 3)).astype(np.float32), True)
    eyes = np.stack([nr.get_points_from_angles(2.5, 15, -90), nr.get_points_from_angles(2.7, 30, 40)]).astype(np.float32)
    e = torch.tensor(eyes)
    zax = torch.nn.functional.normalize(-e, dim=1)
    xax = torch.nn.functional.normalize(torch.cross(torch.tensor([[0., 1., 0.]]).expand(B, 3), zax, dim=1), dim=1)
    yax = torch.nn.functional.normalize(torch.cross(zax, xax, dim=1), dim=1)
    R0 = torch.stack((xax, -yax, zax), dim=1)
    t0 = -torch.matmul(R0, e[:, :, None])[:, :, 0]
    fl = S / (2 * np.tan(np.radians(30)))
    K0 = torch.tensor([[fl, 0, S / 2], [0, fl, S / 2], [0, 0, 1]], dtype=torch.float32)

    def renderer(mode, shading, torch_front):
        r = nr.Renderer()
        r.image_size = S
        r.shading = shading
        r.light_direction = [0.3, 0.8, -0.5]
        if mode == 'look_at':
            r.eye = torch.tensor(eyes, device='cuda')
        else:
            r.camera_mode = 'projection'
            r.K, r.R, r.t = (x.cuda() for x in (K0, R0, t0))
            r.orig_size = S
        if torch_front:
            r.light_direction = torch.tensor(r.light_direction, device='cuda')
        return r

    for mode in ('look_at', 'projection'):
        for shading in ('flat', 'smooth'):
            imgs = {}
            for torch_front in (False, True):
                r = renderer(mode, shading, torch_front)
                imgs[torch_front] = r.render(vertices, faces, nr.VertexColors(colors))
                assert r.last_frontend == ('torch' if torch_front else 'fused')
            same = ((imgs[False] - imgs[True]).abs() <= 1e-5).all(1, keepdim=True).detach()
            assert float(same.float().mean()) > 0.99, (mode, shading)
            w = torch.tensor(rng.normal(size=imgs[False].shape).astype(np.float32), device='cuda') * same
            grads = {}
            for torch_front in (False, True):
                grads[torch_front] = torch.autograd.grad((imgs[torch_front] * w).sum(), [colors, vertices])
                for t in grads[torch_front]:
                    assert torch.isfinite(t).all() and (t != 0).any(), (mode, shading, torch_front)
            errs = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(grads[True], grads[False])]
            print('vertex colours %s %s: torch vs fused, max diff / max: colours %.3e, vertices %.3e'
                  % (mode, shading, errs[0], errs[1]))
            assert errs[0] <= BOUND_PATHS[0] and errs[1] <= BOUND_PATHS[1], (mode, shading, errs)


# (colours, vertices): max diff / max between the torch and the fused path's gradients.  The torch front-end's projected
# vertices differ from the fused one's in the last bits, so the pixels' weights d_k do, and K6 reads the projected faces.
# Measured on the MI355X: colours 8.1e-6 / 7.5e-6 (look_at flat / smooth) and 1.8e-6 / 2.5e-6 (projection), vertices
# 7.6e-5 / 5.1e-5 and 5.4e-5 / 4.6e-5; the bounds leave the factor ~5 that tests/test_uv_pixel_gpu.py leaves for the same
# comparison.
BOUND_PATHS = (4e-5, 4e-4)


def _erode(mask, n):
    import torch
    m = mask[:, None].float()
    return (-torch.nn.functional.max_pool2d(-m, 2 * n + 1, 1, n))[:, 0] > 0.5


def test_smooth_shading_on_a_sphere_approaches_lambert():
    """A unit icosphere of 1 280 faces, white, directional light only: at pixels more than two pixels inside the silhouette
    the smooth render is close to the analytic Lambert sphere max(n . dir, 0) and the flat render clearly farther.  The
    pixel's sphere normal comes from a second render whose vertex colours are the vertex positions under ambient light (the
    interpolated position, normalised)."""
    import torch
    import neural_renderer_amd as nr
    v, f = R.icosphere(3)
    assert len(f) == 1280
    vertices = _cuda(v.astype(np.float32))[None]
    faces = _cuda(f)[None]
    direction = np.array([0.3, 0.8, -0.52])
    direction /= np.linalg.norm(direction)
    r = nr.Renderer()
    r.image_size = 256
    r.anti_aliasing = False
    r.eye = nr.get_points_from_angles(2.732, 20, 30)
    r.light_intensity_ambient, r.light_intensity_directional = 1.0, 0.0
    with torch.no_grad():
        pos = r.render(vertices, faces, nr.VertexColors(_cuda((v * 0.5 + 0.5).astype(np.float32)))) * 2 - 1
        normal = pos / pos.norm(dim=1, keepdim=True).clamp_min(1e-6)
        want = (normal * _cuda(direction.astype(np.float32))[None, :, None, None]).sum(1).clamp_min(0)
        inside = _erode(r.render_silhouettes(vertices, faces) > 0, 3)
        assert int(inside.sum()) > 10000
        r.light_intensity_ambient, r.light_intensity_directional = 0.0, 1.0
        r.light_direction = direction.tolist()
        white = nr.VertexColors(torch.ones(len(v), 3, device='cuda'))
        err = {}
        for shading in ('flat', 'smooth'):
            r.shading = shading
            img = r.render(vertices, faces, white)
            e = (img[:, 0] - want).abs()[inside]
            err[shading] = (float(e.mean()), float(e.max()))
    print('sphere: mean / max |render - Lambert|: flat %.3e / %.3e, smooth %.3e / %.3e, mean ratio %.1f'
          % (err['flat'] + err['smooth'] + (err['flat'][0] / err['smooth'][0],)))
    assert err['smooth'][0] <= SPHERE_SMOOTH_MEAN * 1.5
    assert err['flat'][0] >= 2 * err['smooth'][0]


# measured on the MI355X, mean (max) |render - Lambert| over the 21 000 pixels more than two pixels inside the silhouette:
# smooth 2.864e-3 (1.58e-2), flat 1.618e-2 (7.63e-2): flat is 5.7 times farther
SPHERE_SMOOTH_MEAN = 2.864e-3


def _fit(shading, steps=150):
    import torch
    import neural_renderer_amd as nr
    B = 8
    r, vertices, faces = _teapot(B, 128)
    r.shading = shading
    v = vertices[0]
    truth = (0.5 + 0.4 * v @ torch.tensor([[0.9, -0.3, 0.2], [0.1, 0.8, -0.5], [-0.4, 0.3, 0.7]], device='cuda')).clamp(0, 1)
    colors = torch.full_like(truth, 0.5).requires_grad_(True)
    with torch.no_grad():
        target = r.render(vertices, faces, nr.VertexColors(truth))
    opt = torch.optim.Adam([colors], lr=0.03)
    losses, seen = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss = ((r.render(vertices, faces, nr.VertexColors(colors)) - target) ** 2).mean()
        loss.backward()
        if seen is None:
            seen = colors.grad.abs().sum(1) > 0
            err0 = float((colors.detach() - truth).abs()[seen].mean())
        losses.append(float(loss))
        opt.step()
    err = float((colors.detach() - truth).abs()[seen].mean())
    return losses[0], losses[-1], err0, err, int(seen.sum())


@pytest.mark.parametrize('shading', ['flat', 'smooth'])
def test_fit_vertex_colours_to_views(shading):
    """A teapot's vertex colours from 0.5 towards a linear colour field, 8 views at 128^2, Adam as tests/test_uv_pixel_gpu.py's
    _fit, with its two conditions."""
    l0, l1, e0, e1, n = _fit(shading)
    # measured on the MI355X: flat loss 9.876e-4 -> 9.9e-11, error on the 1 120 (of 1 292) vertices with a gradient
    # 0.1099 -> 0.0009; smooth 9.844e-4 -> 1.0e-10, 0.1099 -> 0.0009
    print('fit vertex colours (%s): loss %.3e -> %.3e, error on the vertices with a gradient %.4f -> %.4f (%d of 1292 vertices)'
          % (shading, l0, l1, e0, e1, n))
    assert l1 < 0.05 * l0
    assert e1 < 0.5 * e0


def test_graph_capture_equals_eager():
    """A whole step -- Renderer.render with vertex colours, smooth shading, and the gradients of vertices and colours --
    captured with neural_renderer_amd.graph.capture replays equal to eager.  The vertex adjacency table is built on the host:
    one eager call with the same index tensor comes first (graph.capture's warm-up does it too)."""
    import torch
    import neural_renderer_amd as nr
    B, S = 2, 64
    v, f = H.teapot()
    vertices = torch.tensor(v, device='cuda')[None].expand(B, -1, -1).contiguous().requires_grad_(True)
    faces = torch.tensor(f, device='cuda')[None].expand(B, -1, -1).contiguous()
    colors = torch.zeros(len(v), 3, device='cuda', requires_grad=True)
    rng = np.random.default_rng(12)
    r = nr.Renderer()
    r.image_size = S
    r.shading = 'smooth'
    r.eye = nr.get_points_from_angles(2.732, 15, -90)
    w = torch.zeros((B, 3, S, S), device='cuda')
    out = torch.zeros((B, 3, S, S), device='cuda')

    def step():
        img = r.render(vertices, faces, nr.VertexColors(colors))
        out.copy_(img)
        return torch.autograd.grad((img * w).sum(), [vertices, colors])
    with torch.no_grad():
        r.render(vertices, faces, nr.VertexColors(colors))   # builds the adjacency table (and checks the indices) eagerly
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        colors.copy_(torch.tensor(rng.uniform(0, 1, colors.shape).astype(np.float32)))
        w.copy_(torch.tensor(rng.normal(size=w.shape).astype(np.float32)))
    replay()
    torch.cuda.synchronize()
    got_img, got = out.clone(), [g.clone() for g in grads[0]]
    eager = step()
    assert torch.equal(got_img, out)
    for a, b in zip(got, eager):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
