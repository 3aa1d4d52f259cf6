"""Smooth light on per-pixel UV images on the GPU (include/nr_hip.h nr_forward_rasterize_uv_smooth /
nr_backward_uv_images_smooth; Renderer.shading = 'smooth' with a UVImages): the forward bit for bit against the NumPy
restatement, the flat call's geometry, the adjoint, grad_faces against the rasterizer's own backward, reproducibility, the
renderer's paths, the Lambert sphere, a fit and graph capture."""
import numpy as np
import pytest

import helpers as H
import uv_smooth_ref as R
import vertex_ref as V

pytestmark = pytest.mark.gpu

EPS = 1e-3
BG = (0.1, 0.2, 0.3)


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device='cuda', requires_grad=grad)


def _run(sc, exact=False, g_rgb=None, alpha=True, depth=True, light=None):
    """Rasterize (no epilogue) with the scene's light -- [B,F,3,3], or `light` -- returns (fn, layout, rgb, alpha, depth,
    faces tensor, light tensor, image tensors)."""
    import neural_renderer_amd as nr
    layout = nr.UVLayout(sc['uv'], sc['face_image'], sc['base'], sc['sizes'])
    fn = nr.Rasterize(sc['S'], 0.1, 100, EPS, BG, return_rgb=True, return_alpha=alpha, return_depth=depth)
    fn.exact_gradient = exact
    faces = _cuda(sc['faces'], True)
    lt = _cuda(sc['light'] if light is None else light, True)
    x = [_cuda(im[0] if sc['shared'] or im.shape[0] == 1 else im, True) for im in sc['images']]
    rgb, a, d = fn(faces, nr.UVImages(layout, x), lt)
    if g_rgb is not None:
        rgb.backward(_cuda(g_rgb))
    return fn, layout, rgb, a, d, faces, lt, x


def _maps(fn):
    return tuple(m.detach().cpu().numpy() for m in (fn.face_index_map, fn.weight_map, fn.depth_map))


@pytest.mark.parametrize('seed', range(8))
def test_forward_equals_restatement_and_flat_geometry(seed):
    sc = R.scene(seed)
    fn, layout, rgb, alpha, depth, _, _, _ = _run(sc)
    fi, wm, dm = _maps(fn)
    assert (fi >= 0).any()
    want = R.render(sc['faces'], fi, wm, dm, sc['light'], layout, R.np_images(sc), EPS, BG)
    assert np.array_equal(rgb.detach().cpu().numpy(), want)
    # alpha, depth and the face index map are the flat UV call's on the same faces
    f2, _, _, a2, d2, _, _, _ = _run(sc, light=np.ascontiguousarray(sc['light'][:, :, 0, :]))
    assert np.array_equal(f2.face_index_map.cpu().numpy(), fi)
    assert np.array_equal(a2.detach().cpu().numpy(), alpha.detach().cpu().numpy())
    assert np.array_equal(d2.detach().cpu().numpy(), depth.detach().cpu().numpy())
    assert np.array_equal(f2.weight_map.cpu().numpy(), wm)


def _adjoint_check(sc, fn, layout, light, x, g, label):
    """grad_light [B,F,3,3] and every image gradient within 1e-6 of their sums of |terms| (the header's bound)."""
    fi, wm, dm = _maps(fn)
    assert (fi >= 0).any()
    gi, gi_mag, gl, gl_mag = R.adjoint(sc['faces'], fi, wm, dm, sc['light'], layout, R.np_images(sc), EPS, g)
    assert tuple(light.grad.shape) == sc['light'].shape and light.grad.dim() == 4
    got_l = light.grad.cpu().numpy().astype(np.float64)
    worst = [float((np.abs(got_l - gl) / (1e-6 * gl_mag + 1e-300)).max())]
    assert not got_l[gl_mag == 0].any()                         # every element stored: zeros where no pixel feeds
    for m, xm in enumerate(x):
        got = xm.grad.cpu().numpy().astype(np.float64).reshape(gi[m].shape)
        worst.append(float((np.abs(got - gi[m]) / (1e-6 * gi_mag[m] + 1e-300)).max()))
        assert not got[gi_mag[m] == 0].any()
    # measured on the MI355X: at most 0.057 of the bound over the 8 seeds, 0.035 on the magnified scene
    print('uv smooth adjoint %s: worst share of 1e-6 x sum|terms|: light %.3f, images %s'
          % (label, worst[0], ', '.join('%.3f' % w for w in worst[1:])))
    assert max(worst) <= 1
    return gi_mag, gl_mag


@pytest.mark.parametrize('seed', range(8))
def test_adjoint(seed):
    sc = R.scene(seed)
    g = sc['rng'].normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    fn, layout, _, _, _, _, light, x = _run(sc, g_rgb=g)
    _adjoint_check(sc, fn, layout, light, x, g, 'seed %d' % seed)


def test_adjoint_one_pixel_images_heavily_magnified():
    """Thousands of pixels feed the same image pixel and the nine light sums of one face."""
    sc = R.magnified_scene()
    g = sc['rng'].normal(size=(2, 128, 128, 3)).astype(np.float32)
    fn, layout, _, _, _, _, light, x = _run(sc, g_rgb=g)
    gi_mag, gl_mag = _adjoint_check(sc, fn, layout, light, x, g, 'magnified')
    fi = fn.face_index_map.cpu().numpy()
    assert int((fi >= 0).sum()) > 5000
    key = np.arange(fi.shape[0])[:, None, None] * sc['faces'].shape[1] + fi
    assert np.bincount(key[fi >= 0]).max() > 1000                 # one face of one view owns more than a thousand pixels
    assert gi_mag[0].max() > 100 * np.abs(g).mean()               # the 1x1 image collected thousands of terms


@pytest.mark.parametrize('exact', [False, True])
def test_grad_faces_is_the_rasterizers_own(exact):
    """grad_faces bit for bit what nr_backward_rasterize_lit(NULL, ..., grad_textures = NULL) gives on the same rgb_map."""
    import torch
    from neural_renderer_amd import _lib
    for seed in (1, 2):
        sc = R.scene(seed)
        B, S, F = sc['B'], sc['S'], sc['faces'].shape[1]
        g = sc['rng'].normal(size=(B, S, S, 3)).astype(np.float32)
        fn, _, rgb, _, _, faces, _, _ = _run(sc, exact=exact, g_rgb=g, alpha=False, depth=False)
        assert (fn.face_index_map >= 0).any()
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
        assert (faces.grad != 0).any()
        assert torch.equal(faces.grad, gf)


def test_reproducible():
    """Two calls: the images and grad_faces repeat bit for bit (the forward has no atomics; K6 + K8 promise the same bits
    since ABI 0.6.0).  The image and light sums are double atomics in arrival order (the runs of a wave are summed in a fixed
    order first): the kernel guarantees each call the header's 1e-6 x sum|terms|, not the same last bit -- that bound is what
    is asserted for both calls, and the difference observed between them is printed."""
    import torch
    sc = R.scene(3)
    g = sc['rng'].normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    runs = []
    for k in range(2):
        fn, layout, rgb, _, _, faces, light, x = _run(sc, g_rgb=g)
        _adjoint_check(sc, fn, layout, light, x, g, 'call %d' % k)
        runs.append([rgb.detach(), faces.grad, light.grad] + [xi.grad for xi in x])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # measured on the MI355X: 0 for every gradient (the rounding to float hid the order of the double additions)
    diff = [float((a - b).abs().max()) for a, b in zip(runs[0][2:], runs[1][2:])]
    print('uv smooth: max |difference| between two calls: grad_light %.3e, grad_images %s'
          % (diff[0], ', '.join('%.3e' % d for d in diff[1:])))


# ---------------------------------------------------------------------------------------------------------------------
# through the Renderer

def _sphere(level=3, B=1, image=None, grad=False):
    """vertex_ref.icosphere with lat/long uvs and one image (default: a white 1x1 one)."""
    import torch
    import neural_renderer_amd as nr
    v, f = V.icosphere(level)
    layout = R.image_layout(R.latlong_uv(v, f), (1, 1) if image is None else image.shape[:2])
    vertices = _cuda(np.broadcast_to(v.astype(np.float32), (B,) + v.shape), grad)
    faces = _cuda(f)[None].expand(B, -1, -1).contiguous()
    img = torch.ones(1, 1, 3, device='cuda') if image is None else _cuda(image, grad)
    return v, f, layout, vertices, faces, img


def test_white_image_smooth_is_the_vertex_colour_render():
    """Renderer.render(UVImages(white 1x1), shading = 'smooth') against render(VertexColors(ones)), smooth, pixel by pixel.
    n, the roundings by which the two orders differ: a 1x1 image has W - 1 = H - 1 = 0, so pos_x = pos_y = 0 and the four
    read weights are exactly 1, 0, 0, 0; with the pixel 1 the sample is c = ((0 + 1 * 1) + 1 * 0) + ... = 1 exactly.  The
    corner light is vertex_shade's colour of a white vertex, 1 * light = light exactly, which is also the corner colour C_k of
    the VertexColors render.  Both then evaluate (C_0 e_0 + C_1 e_1) + C_2 e_2 with the same e_k = d_k from the same maps (the
    geometry goes through the same front-end call), the UV path multiplies by c = 1 (exact) and both apply * 1 + 0 * bg and
    the same epilogue: n = 0, gamma_0 = 0, the renders are equal bit for bit."""
    import torch
    import neural_renderer_amd as nr
    v, f, layout, vertices, faces, img = _sphere(3)
    r = nr.Renderer()
    r.image_size = 128
    r.eye = nr.get_points_from_angles(2.732, 20, 30)
    r.light_direction = [0.3, 0.8, -0.52]
    r.shading = 'smooth'
    with torch.no_grad():
        a = r.render(vertices, faces, nr.UVImages(layout, [img]))
        assert r.last_frontend == 'fused'
        b = r.render(vertices, faces, nr.VertexColors(torch.ones(len(v), 3, device='cuda')))
        r.shading = 'flat'
        flat = r.render(vertices, faces, nr.UVImages(layout, [img]))
    assert float((a > 0).float().mean()) > 0.2
    # (gamma_0 |value| = 0 leaves no share of a bound to print: the largest difference is printed instead)
    print('uv smooth, white 1x1 image vs vertex colours: max |difference| %.3e (n = 0: bit for bit)'
          % float((a - b).abs().max()))
    assert torch.equal(a, b)
    assert not torch.equal(a, flat)


def _erode(mask, n):
    import torch
    m = mask[:, None].float()
    return (-torch.nn.functional.max_pool2d(-m, 2 * n + 1, 1, n))[:, 0] > 0.5


def test_smooth_light_on_a_textured_sphere_approaches_lambert():
    """tests/test_vertex_colors_gpu.py's sphere statement for a textured white sphere (1 280 faces, lat/long uvs, a white 1x1
    image): more than two pixels inside the silhouette the smooth render is close to max(n . dir, 0) and the flat render at
    least twice as far.  The pixel's sphere normal comes from a vertex-colour render of the positions under ambient light."""
    import torch
    import neural_renderer_amd as nr
    v, f, layout, vertices, faces, img = _sphere(3)
    assert len(f) == 1280
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
        err = {}
        for shading in ('flat', 'smooth'):
            r.shading = shading
            e = (r.render(vertices, faces, nr.UVImages(layout, [img]))[:, 0] - want).abs()[inside]
            err[shading] = (float(e.mean()), float(e.max()))
    # measured on the MI355X: flat 1.618e-2 (max 7.63e-2), smooth 2.864e-3 (max 1.58e-2) over the 21 000 pixels: flat is 5.7
    # times farther -- the vertex-colour sphere's figures, as the white-image test above says they must be
    print('textured sphere: mean / max |render - Lambert|: flat %.3e / %.3e, smooth %.3e / %.3e, mean ratio %.1f'
          % (err['flat'] + err['smooth'] + (err['flat'][0] / err['smooth'][0],)))
    assert err['flat'][0] >= 2 * err['smooth'][0]


def _smooth_image(h, w):
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    return np.stack((0.5 + 0.4 * np.sin(2 * np.pi * x) * np.cos(np.pi * y), 0.5 + 0.3 * np.cos(2 * np.pi * (x + y)),
                     0.3 + 0.4 * y * x), axis=2).astype(np.float32)


def test_fused_and_torch_paths_agree_and_gradients_reach_everything():
    """Renderer.render(UVImages), shading = 'smooth': the fused path (HIP vertex light and front-end) against the torch path
    (a tensor light direction keeps both off the kernels).  The torch front-end projects with other roundings, so edge pixels
    may see another face: the upstream gradient is zeroed where the two renders differ by more than 1e-5, as in
    tests/test_uv_pixel_gpu.py.  Gradients reach the image, the vertices and a learnable eye on both paths."""
    import torch
    import neural_renderer_amd as nr
    B, S = 2, 64
    rng = np.random.default_rng(31)
    v, f = V.icosphere(2)
    layout = R.image_layout(R.latlong_uv(v, f), (24, 48))
    v = (v * np.array([1.0, 0.7, 0.8]) + rng.normal(scale=0.02, size=v.shape)).astype(np.float32)
    vertices = _cuda(np.stack([v, v * 0.9]), True)
    faces = _cuda(f)[None].expand(B, -1, -1).contiguous()
    image = _cuda(_smooth_image(24, 48), True)
    eyes = np.stack([nr.get_points_from_angles(2.5, 15, -90), nr.get_points_from_angles(2.7, 30, 40)]).astype(np.float32)

    def renderer(torch_front):
        r = nr.Renderer()
        r.image_size = S
        r.shading = 'smooth'
        r.eye = torch.tensor(eyes, device='cuda', requires_grad=True)
        r.light_direction = [0.3, 0.8, -0.5]
        if torch_front:
            r.light_direction = torch.tensor(r.light_direction, device='cuda')
        return r
    rs, imgs = {}, {}
    for torch_front in (False, True):
        rs[torch_front] = r = renderer(torch_front)
        calls = dict(r.frontend_calls)
        imgs[torch_front] = r.render(vertices, faces, nr.UVImages(layout, [image]))
        name = 'torch' if torch_front else 'fused'
        assert r.last_frontend == name
        assert r.frontend_calls[name] == calls[name] + 1 and sum(r.frontend_calls.values()) == sum(calls.values()) + 1
    same = ((imgs[False] - imgs[True]).abs() <= 1e-5).all(1, keepdim=True).detach()
    assert float(same.float().mean()) > 0.99
    w = torch.tensor(rng.normal(size=imgs[False].shape).astype(np.float32), device='cuda') * same
    grads = {}
    for torch_front in (False, True):
        grads[torch_front] = torch.autograd.grad((imgs[torch_front] * w).sum(), [image, vertices, rs[torch_front].eye])
        for t in grads[torch_front]:
            assert torch.isfinite(t).all() and (t != 0).any(), torch_front
    errs = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(grads[True], grads[False])]
    print('uv smooth: torch vs fused, max diff / max: image %.3e, vertices %.3e, eye %.3e' % tuple(errs))
    assert errs[0] <= BOUND_PATHS[0] and errs[1] <= BOUND_PATHS[1] and errs[2] <= BOUND_PATHS[2], errs


# (image, vertices, eye): max diff / max between the torch and the fused path's gradients.  The torch front-end's projected
# vertices differ from the fused one's in the last bits, so the pixels' weights do: a pixel's image reads move with them (an
# ulp of a weight moves a read by about an ulp times the image width), and K6 reads the projected faces.
# Measured on the MI355X: image 2.38e-5, vertices 4.25e-5, eye 2.10e-5; the bounds leave the factor ~5 that
# tests/test_vertex_colors_gpu.py documents for the same comparison.
BOUND_PATHS = (1.2e-4, 2e-4, 1e-4)


# Restated from tests/test_vertex_colors.py (FD_STEP, FD_TOL: h = 1e-6 on unit-size geometry, truncation ~1e-12, rounding
# ~1e-9; measured there float64 against float64 at 1.3e-10 of the largest entry) and tests/test_vertex_colors_gpu.py
# (GAMMA_VERTICES: the float32 chain of the vertex-shading backward has at most 64 roundings per term, against magnitudes
# that propagate absolute values).
FD_STEP, FD_TOL, GAMMA_VERTICES = 1e-6, 1e-7, 64


def test_vertex_gradient_through_the_light_against_finite_differences():
    """The light's share of the vertex gradient: vertex_light (HIP) feeds the rasterizer's per-corner light while the
    projected faces are detached, so vertices.grad is nr_vertex_shade_backward applied to the kernel's grad_light.  It is
    compared with the float64 adjoint (vertex_ref.shade_adjoint64 on the restatement's grad_light) within that test's own term
    magnitudes, and at a handful of vertices with central differences of a float64 torch restatement (vertex_shade_torch in
    double on the CPU), with the step and tolerance of tests/test_vertex_colors_gpu.py:
    test_backward_against_adjoint_and_finite_differences -- FD_TOL of the largest entry plus gamma_64 of the entry's term
    magnitudes -- plus the 1e-6 x sum|terms| the header allows grad_light, pushed through the same adjoint."""
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd.vertex_colors import vertex_shade_torch
    B, S = 2, 64
    rng = np.random.default_rng(41)
    v, f = V.icosphere(2)
    layout = R.image_layout(R.latlong_uv(v, f), (24, 48))
    v = np.stack([v + rng.normal(scale=0.02, size=v.shape), 0.9 * v + rng.normal(scale=0.02, size=v.shape)]).astype(np.float32)
    r32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    L = V.Light(0.3, 0.8, r32((1.0, 0.9, 0.8)), r32((0.7, 1.0, 0.6)), r32((0.3, 0.8, -0.5)))
    vertices = _cuda(v, True)
    faces = _cuda(f)[None].expand(B, -1, -1).contiguous()
    image_np = _smooth_image(24, 48)
    image = _cuda(image_np)
    eye = torch.tensor(np.stack([nr.get_points_from_angles(2.5, 15, -90), nr.get_points_from_angles(2.7, 30, 40)]),
                       dtype=torch.float32, device='cuda')
    with torch.no_grad():
        pf = nr.vertices_to_faces(nr.perspective(nr.look_at(vertices, eye), angle=30), faces)
        pf = torch.cat((pf, torch.flip(pf, dims=[2])), dim=1).contiguous()
    light = nr.vertex_light(vertices, faces, fill_back=True, smooth=True, implementation='hip', **L.kwargs())
    assert tuple(light.shape) == (B, 2 * len(f), 3, 3)
    fn = nr.Rasterize(S, 0.1, 100, EPS, BG, return_rgb=True)
    rgb, _, _ = fn(pf, nr.UVImages(layout, [image]), light)
    g = rng.normal(size=(B, S, S, 3)).astype(np.float32)
    rgb.backward(_cuda(g))
    fi, wm, dm = _maps(fn)
    assert (fi >= 0).sum() > 1000
    light_np = light.detach().cpu().numpy()
    _, _, gl, gl_mag = R.adjoint(pf.cpu().numpy(), fi, wm, dm, light_np, layout, [image_np[None]], EPS, g)
    ones = np.ones((v.shape[1], 3))
    _, _, gv, gv_mag = V.shade_adjoint64(v, f, ones, L, True, True, gl)
    _, _, _, gv_up = V.shade_adjoint64(v, f, ones, L, True, True, gl_mag)
    got = vertices.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and (got != 0).any()
    tol = H.gamma(GAMMA_VERTICES) * gv_mag + 1e-6 * gv_up
    # measured on the MI355X: 0.011 of the bound
    print('uv smooth: vertex gradient through the light, worst share of its bound: %.3f'
          % float((np.abs(got - gv) / (tol + 1e-300)).max()))
    assert (np.abs(got - gv) <= tol).all()
    # central differences in float64, at vertices away from the relu's kink that receive a gradient
    vhat = v / np.linalg.norm(v, axis=2, keepdims=True)
    away = (np.abs(vhat @ L.dir) > 0.1) & (np.abs(gv).max(2) > 0.01 * np.abs(gv).max())
    pick = [tuple(p) for p in np.argwhere(away)[:: max(1, int(away.sum()) // 5)][:5]]
    assert len(pick) >= 3
    ft, g64 = torch.tensor(f), torch.tensor(gl)

    def loss(vv):
        return float((vertex_shade_torch(torch.tensor(vv), ft, torch.ones(v.shape[1], 3, dtype=torch.float64),
                                         fill_back=True, smooth=True, **L.kwargs()) * g64).sum())
    v64 = v.astype(np.float64)
    for b, i in pick:
        for c in range(3):
            vp, vm = v64.copy(), v64.copy()
            vp[b, i, c] += FD_STEP
            vm[b, i, c] -= FD_STEP
            d = (loss(vp) - loss(vm)) / (2 * FD_STEP)
            assert abs(got[b, i, c] - d) <= FD_TOL * np.abs(gv).max() + tol[b, i, c], (b, i, c, got[b, i, c], d)


def _fit(steps=150):
    import torch
    import neural_renderer_amd as nr
    v, f, uv = R.latlong_sphere()
    board = R.checkerboard()
    layout = R.image_layout(uv, board.shape[:2])
    B = 8
    vertices = _cuda(v)[None].expand(B, -1, -1).contiguous()
    faces = _cuda(f)[None].expand(B, -1, -1).contiguous()
    r = nr.Renderer()
    r.image_size = 64
    r.shading = 'smooth'
    r.eye = torch.tensor(np.stack([nr.get_points_from_angles(2.5, 20.0 * (i % 2), 45.0 * i) for i in range(B)]),
                         dtype=torch.float32, device='cuda')
    truth = _cuda(board)
    image = torch.full_like(truth, 0.5).requires_grad_(True)
    with torch.no_grad():
        target = r.render(vertices, faces, nr.UVImages(layout, [truth]))
    opt = torch.optim.Adam([image], lr=0.03)
    losses, seen = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss = ((r.render(vertices, faces, nr.UVImages(layout, [image])) - target) ** 2).mean()
        loss.backward()
        if seen is None:
            seen = image.grad.abs().sum(2) > 0
            err0 = float((image.detach() - truth).abs()[seen].mean())
        losses.append(float(loss))
        opt.step()
    assert r.last_frontend == 'fused'
    err = float((image.detach() - truth).abs()[seen].mean())
    return losses[0], losses[-1], err0, err, int(seen.sum())


def test_fit_grey_image_to_checkerboard_views_under_smooth_light():
    """tests/test_uv_pixel_gpu.py's fit (a lat/long sphere, a 64 x 128 checkerboard, 8 views at 64^2, Adam, 150 steps) with
    shading = 'smooth', and its two conditions."""
    l0, l1, e0, e1, n = _fit()
    # measured on the MI355X: loss 1.171e-2 -> 1.9e-9, seen-pixel error 0.2333 -> 0.0112 (6 316 seen pixels)
    print('fit under smooth light: loss %.3e -> %.3e, seen-pixel error %.4f -> %.4f (%d seen pixels)' % (l0, l1, e0, e1, n))
    assert l1 < 0.05 * l0
    assert e1 < 0.5 * e0


def test_graph_capture_equals_eager():
    """A whole step -- Renderer.render with a UVImages under smooth light and the gradients of the vertices and the image --
    captured with neural_renderer_amd.graph.capture replays equal to eager.  The vertex adjacency table is built on the host:
    one eager call with the same index tensor comes first.  It runs under no_grad, as in tests/test_vertex_colors_gpu.py: a
    differentiable eager step on the default stream would leave the leaves' AccumulateGrad nodes tied to that stream, and the
    captured backward would then wait on the default stream, which a capture does not allow (torch warns, and the capture
    takes the process down -- with shading 'flat' just the same)."""
    import torch
    import neural_renderer_amd as nr
    B, S = 2, 64
    v, f, uv = R.latlong_sphere(8, 16)
    layout = R.image_layout(uv, (16, 32))
    vertices = _cuda(v)[None].expand(B, -1, -1).contiguous().requires_grad_(True)
    faces = _cuda(f)[None].expand(B, -1, -1).contiguous()
    x = torch.zeros((B, 16, 32, 3), device='cuda', requires_grad=True)
    rng = np.random.default_rng(12)
    r = nr.Renderer()
    r.image_size = S
    r.shading = 'smooth'
    r.eye = nr.get_points_from_angles(2.5, 15, -90)
    w = torch.zeros((B, 3, S, S), device='cuda')
    out = torch.zeros((B, 3, S, S), device='cuda')

    def step():
        img = r.render(vertices, faces, nr.UVImages(layout, [x]))
        out.copy_(img)
        return torch.autograd.grad((img * w).sum(), [vertices, x])
    with torch.no_grad():                                    # eager warm-up: the adjacency table exists before the capture
        r.render(vertices, faces, nr.UVImages(layout, [x]))
    torch.cuda.synchronize()
    from neural_renderer_amd.vertex_colors import _ADJ_ATTR
    assert getattr(faces, _ADJ_ATTR, None) or getattr(faces._base, _ADJ_ATTR, None)
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        x.copy_(torch.tensor(rng.uniform(0, 1, x.shape).astype(np.float32)))
        w.copy_(torch.tensor(rng.normal(size=w.shape).astype(np.float32)))
    replay()
    torch.cuda.synchronize()
    got_img, got = out.clone(), [g.clone() for g in grads[0]]
    eager = step()
    assert (got_img > 0).any() and (eager[0] != 0).any() and (eager[1] != 0).any()
    assert torch.equal(got_img, out)
    for a, b in zip(got, eager):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_calls_that_used_to_raise_now_run_and_cubes_still_raise():
    import torch
    import neural_renderer_amd as nr
    v, f, layout, vertices, faces, img = _sphere(1, B=2)
    r = nr.Renderer()
    r.image_size = 32
    r.shading = 'smooth'
    out = r.render(vertices, faces, nr.UVImages(layout, [img]))
    assert tuple(out.shape) == (2, 3, 32, 32) and (out > 0).any()
    light = nr.vertex_light(vertices, faces)
    assert tuple(light.shape) == (2, 2 * len(f), 3, 3) and light.is_cuda
    pf = nr.vertices_to_faces(nr.perspective(nr.look_at(vertices, r.eye)), faces)
    pf = torch.cat((pf, torch.flip(pf, dims=[2])), dim=1).contiguous()
    rgb = nr.rasterize(pf, nr.UVImages(layout, [img]), 32, face_light=light)
    assert tuple(rgb.shape) == (2, 3, 32, 32) and (rgb > 0).any()
    cubes = torch.ones(2, len(f), 2, 2, 2, 3, device='cuda')
    with pytest.raises(ValueError, match='UVImages or VertexColors'):
        r.render(vertices, faces, cubes)
    with pytest.raises(ValueError, match='per corner'):
        nr.rasterize(pf, torch.cat((cubes, cubes), dim=1), 32, face_light=light)
    with pytest.raises(ValueError, match='per corner'):
        nr.rasterize(pf, nr.UVImages(layout, [img]), 32, face_light=light[:, :, :2])
