"""Per-pixel UV images on the GPU (include/nr_hip.h nr_forward_rasterize_uv / nr_backward_uv_images; UVImages): the forward
bit for bit against the NumPy restatement, the cube path where the two must agree, grad_faces against the rasterizer's own
backward, the adjoint, reproducibility, the renderer's paths, convergence of the bake towards it, a fit and graph capture."""
import numpy as np
import pytest

import helpers as H
import uv_pixel_ref as R
import uv_ref as U

pytestmark = pytest.mark.gpu

EPS = 1e-3


def _scene(seed):
    """A fuzz scene: random triangles, a random layout (1x1 images, degenerate uv triangles, faces without an image), fill_back
    on or off, shared or per-view images, B = 1..3, odd and non-power-of-two rasters."""
    rng = np.random.default_rng(500 + seed)
    B = int(rng.integers(1, 4))
    Nf = int(rng.integers(20, 120))
    fill_back = bool(seed % 2)
    S = int(rng.choice([37, 50, 64, 96]))
    sizes = [(1, 1) if rng.uniform() < 0.3 else (int(rng.integers(1, 40)), int(rng.integers(1, 60)))
             for _ in range(int(rng.integers(1, 4)))]
    ts = int(rng.choice([2, 3, 4]))
    uv, face_image, base = U.random_layout(rng, Nf, ts, sizes)
    faces = H.random_scene(rng, B, Nf, size=0.4)
    if fill_back:
        faces = np.ascontiguousarray(np.concatenate((faces, faces[:, :, ::-1]), axis=1))
    F = faces.shape[1]
    light = rng.uniform(0.2, 1.2, (B, F, 3)).astype(np.float32)
    Bi = 1 if (seed // 2) % 2 == 0 else B
    images = [rng.uniform(0, 1, (Bi, h, w, 3)).astype(np.float32) for h, w in sizes]
    return dict(rng=rng, B=B, S=S, sizes=sizes, ts=ts, uv=uv, face_image=face_image, base=base, faces=faces, light=light,
                images=images, shared=Bi == 1 and B > 1)


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device='cuda', requires_grad=grad)


def _uv_images(layout, images, shared):
    import neural_renderer_amd as nr
    x = [_cuda(im[0] if shared or im.shape[0] == 1 else im, True) for im in images]
    return x, nr.UVImages(layout, x)


def _run(sc, exact=False, g_rgb=None, alpha=True, depth=True):
    """Rasterize (no epilogue) in per-pixel mode; returns (fn, rgb, faces tensor, light tensor, image tensors)."""
    import neural_renderer_amd as nr
    layout = nr.UVLayout(sc['uv'], sc['face_image'], sc['base'], sc['sizes'])
    fn = nr.Rasterize(sc['S'], 0.1, 100, EPS, (0.1, 0.2, 0.3), return_rgb=True, return_alpha=alpha, return_depth=depth)
    fn.exact_gradient = exact
    faces = _cuda(sc['faces'], True)
    light = _cuda(sc['light'], True)
    x, uvi = _uv_images(layout, sc['images'], sc['shared'])
    rgb, a, d = fn(faces, uvi, light)
    if g_rgb is not None:
        rgb.backward(_cuda(g_rgb))
    return fn, layout, rgb, a, d, faces, light, x


def _maps(fn):
    return tuple(m.detach().cpu().numpy() for m in (fn.face_index_map, fn.weight_map, fn.depth_map))


def _np_images(sc):
    return [im[:1] if sc['shared'] else im for im in sc['images']]


@pytest.mark.parametrize('seed', range(8))
def test_forward_equals_restatement_and_cube_geometry(seed):
    import neural_renderer_amd as nr
    sc = _scene(seed)
    fn, layout, rgb, alpha, depth, _, _, _ = _run(sc)
    fi, wm, dm = _maps(fn)
    assert (fi >= 0).any()
    want = R.render(sc['faces'], fi, wm, dm, sc['light'], layout, _np_images(sc), EPS, (0.1, 0.2, 0.3))
    assert np.array_equal(rgb.detach().cpu().numpy(), want)
    # alpha, depth and the face index map are the cube path's (the bake of the same images, per-face light colours)
    tex = nr.bake_uv_textures([_cuda(im[0] if sc['shared'] else im) for im in sc['images']], layout)
    tex = tex.expand(sc['B'], -1, -1, -1, -1, -1).contiguous()
    fc = nr.Rasterize(sc['S'], 0.1, 100, EPS, (0.1, 0.2, 0.3), return_rgb=True, return_alpha=True, return_depth=True)
    _, a2, d2 = fc(_cuda(sc['faces']), tex, _cuda(sc['light']))
    assert np.array_equal(fc.face_index_map.cpu().numpy(), fi)
    assert np.array_equal(a2.cpu().numpy(), alpha.detach().cpu().numpy())
    assert np.array_equal(d2.cpu().numpy(), depth.detach().cpu().numpy())


def test_faces_without_images_render_as_the_cube_path():
    """face_image = -1 everywhere (one unused image): the per-pixel render is the face_light cube render of the bake (= base)
    bit for bit, with the pixel's own batch element's depths (fix_batch_z) as this mode always takes them."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(7)
    Nf, ts, B, S = 80, 4, 2, 64
    uv, _, base = U.random_layout(rng, Nf, ts, [(3, 5)])
    base = rng.uniform(0, 1, base.shape).astype(np.float32)   # texels that differ within a face
    layout = nr.UVLayout(uv, np.full(Nf, -1, np.int32), base, [(3, 5)])
    faces = H.random_scene(rng, B, Nf, size=0.4)
    faces = np.ascontiguousarray(np.concatenate((faces, faces[:, :, ::-1]), axis=1))
    light = rng.uniform(0.2, 1.2, (B, 2 * Nf, 3)).astype(np.float32)
    image = _cuda(rng.uniform(0, 1, (3, 5, 3)).astype(np.float32))
    fn = nr.Rasterize(S, 0.1, 100, EPS, (0, 0, 0), return_rgb=True)
    rgb, _, _ = fn(_cuda(faces), nr.UVImages(layout, [image]), _cuda(light))
    fc = nr.Rasterize(S, 0.1, 100, EPS, (0, 0, 0), return_rgb=True)
    fc.fix_batch_z = True
    tex = nr.bake_uv_textures([image], layout).expand(B, -1, -1, -1, -1, -1).contiguous()
    rgb2, _, _ = fc(_cuda(faces), tex, _cuda(light))
    assert (fn.face_index_map >= 0).sum() > 500
    assert np.array_equal(rgb.cpu().numpy(), rgb2.cpu().numpy())


@pytest.mark.parametrize('exact', [False, True])
def test_grad_faces_is_the_rasterizers_own(exact):
    """grad_faces bit for bit what nr_backward_rasterize_lit(NULL, ..., grad_textures = NULL) gives on the same rgb_map."""
    import torch
    from neural_renderer_amd import _lib
    for seed in (1, 2):
        sc = _scene(seed)
        B, S, F = sc['B'], sc['S'], sc['faces'].shape[1]
        g = sc['rng'].normal(size=(B, S, S, 3)).astype(np.float32)
        fn, _, rgb, _, _, faces, _, _ = _run(sc, exact=exact, g_rgb=g, alpha=False, depth=False)
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


def _adjoint_check(sc, fn, layout, light, x, g):
    fi, wm, dm = _maps(fn)
    gi, gi_mag, gl, gl_mag = R.adjoint(sc['faces'], fi, wm, dm, sc['light'], layout, _np_images(sc), EPS, g)
    got_l = light.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got_l - gl) <= 1e-6 * gl_mag).all()
    for m, xm in enumerate(x):
        got = xm.grad.cpu().numpy().astype(np.float64).reshape(gi[m].shape)
        assert (np.abs(got - gi[m]) <= 1e-6 * gi_mag[m]).all(), m
    return gi_mag


@pytest.mark.parametrize('seed', range(8))
def test_adjoint(seed):
    sc = _scene(seed)
    g = sc['rng'].normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    fn, layout, _, _, _, _, light, x = _run(sc, g_rgb=g)
    _adjoint_check(sc, fn, layout, light, x, g)


def test_adjoint_one_pixel_images_heavily_magnified():
    """Thousands of pixels read the same image pixel: a 1x1 image and a 2x2 one on large faces."""
    rng = np.random.default_rng(3)
    sc = _scene(0)
    Nf = 40
    uv, face_image, base = U.random_layout(rng, Nf, 2, [(1, 1), (2, 2)])
    face_image = (np.arange(Nf) % 2).astype(np.int32)
    faces = H.random_scene(rng, 2, Nf, spread=0.3, size=0.9)
    sc.update(B=2, S=128, sizes=[(1, 1), (2, 2)], uv=uv, face_image=face_image, base=base, faces=faces, shared=True,
              light=rng.uniform(0.2, 1.2, (2, Nf, 3)).astype(np.float32),
              images=[rng.uniform(0, 1, (1, 1, 1, 3)).astype(np.float32), rng.uniform(0, 1, (1, 2, 2, 3)).astype(np.float32)])
    g = rng.normal(size=(2, 128, 128, 3)).astype(np.float32)
    fn, layout, _, _, _, _, light, x = _run(sc, g_rgb=g)
    mag = _adjoint_check(sc, fn, layout, light, x, g)
    assert int((fn.face_index_map >= 0).sum()) > 5000
    assert mag[0].max() > 100 * np.abs(g).mean()   # the 1x1 image collected thousands of terms


def test_reproducible():
    sc = _scene(3)
    g = sc['rng'].normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    runs = []
    for _ in range(2):
        fn, _, rgb, _, _, faces, light, x = _run(sc, g_rgb=g)
        runs.append([rgb.detach(), faces.grad, light.grad] + [xi.grad for xi in x])
    for a, b in zip(*runs):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _display(tmp):
    import torch
    import neural_renderer_amd as nr
    path = H.write_display_model(str(tmp))
    layout = nr.UVLayout.from_obj(path, texture_size=4)
    v, f = nr.load_obj(path)[:2]
    return layout, torch.tensor(v, device='cuda')[None], torch.tensor(f, device='cuda')[None]


def test_renderer_paths_agree_and_gradients_reach_everything(tmp_path):
    """Fused look_at and fused projection against the torch front-end (tensor light direction) with the same camera.  The torch
    front-end projects with other roundings, so edge pixels may see another face: the upstream gradient is zeroed where the two
    renders differ by more than 1e-5, as in test_uv_textures_gpu.py."""
    import torch
    import neural_renderer_amd as nr
    layout, vertices, faces = _display(tmp_path)
    tex = nr.UVTextures(layout).cuda()
    B = 2
    vertices = vertices.expand(B, -1, -1).contiguous().requires_grad_(True)
    faces = faces.expand(B, -1, -1).contiguous()
    rng = np.random.default_rng(5)

    eyes = np.stack([nr.get_points_from_angles(2, 15, -90), nr.get_points_from_angles(2.2, 30, 40)]).astype(np.float32)
    # the same views as a projection camera (tests/test_projection_gpu.py: test_projection_equals_look_at_camera)
    e = torch.tensor(eyes)
    zax = torch.nn.functional.normalize(-e, dim=1)
    xax = torch.nn.functional.normalize(torch.cross(torch.tensor([[0., 1., 0.]]).expand(B, 3), zax, dim=1), dim=1)
    yax = torch.nn.functional.normalize(torch.cross(zax, xax, dim=1), dim=1)
    R0 = torch.stack((xax, -yax, zax), dim=1)
    t0 = -torch.matmul(R0, e[:, :, None])[:, :, 0]
    fl = 64 / (2 * np.tan(np.radians(30)))
    K0 = torch.tensor([[fl, 0, 32], [0, fl, 32], [0, 0, 1]], dtype=torch.float32)

    def renderer(mode, torch_front):
        r = nr.Renderer()
        r.image_size = 64
        if mode == 'look_at':
            r.eye = torch.tensor(eyes, device='cuda', requires_grad=True)
        else:
            r.camera_mode = 'projection'
            r.K, r.R, r.t = (x.cuda().requires_grad_(True) for x in (K0, R0, t0))
            r.orig_size = 64
        if torch_front:
            r.light_direction = torch.tensor([0.0, 1.0, 0.0], device='cuda')
        return r

    for mode in ('look_at', 'projection'):
        outs = {}
        for torch_front in (False, True):
            r = renderer(mode, torch_front)
            img = r.render(vertices, faces, tex.uv_images())
            assert r.last_frontend == ('torch' if torch_front else 'fused'), mode
            outs[torch_front] = (r, img)
        same = (((outs[False][1] - outs[True][1]).abs() <= 1e-5).all(1, keepdim=True)).detach()
        assert float(same.float().mean()) > 0.99, mode
        w = torch.tensor(rng.normal(size=outs[False][1].shape).astype(np.float32), device='cuda') * same
        grads = {}
        for torch_front in (False, True):
            r = renderer(mode, torch_front)
            for p in list(tex.images) + [vertices]:
                p.grad = None
            (r.render(vertices, faces, tex.uv_images()) * w).sum().backward()
            cams = [r.eye] if mode == 'look_at' else [r.K, r.R, r.t]
            grads[torch_front] = [p.grad.clone() for p in list(tex.images) + [vertices]]
            for t in grads[torch_front][:-1] + [c.grad for c in cams]:
                assert t is not None and torch.isfinite(t).all() and (t != 0).any(), (mode, torch_front)
            # (the torch front-end's lighting normalises the normals of the display model's degenerate faces: 0 / 0 in its
            # backward, NaN at their vertices -- as in the reference; the fused front-end's vertex gradient is finite)
            gv = grads[torch_front][-1]
            assert (gv != 0).any() and (torch_front or torch.isfinite(gv).all()), (mode, torch_front)
        # The torch front-end's projected vertices differ from the fused one's in the last bits.  Unlike the bake, whose
        # texels sit at fixed uv points, a pixel's image reads move with its barycentric weights: an ulp of a weight moves a
        # read by about an ulp times the image width, so the image gradients differ more than the bake path's 1e-4 allows.
        # Measured on the MI355X (max diff / max): images 4.3e-4 (look_at) and 0 (projection), vertices 8.3e-3 / 8.5e-3
        # (the light -> normal -> vertex backward sums in another order, near-degenerate faces amplify it).
        errs = []
        for k, (a, b) in enumerate(zip(grads[True], grads[False])):
            ok = torch.isfinite(a)
            errs.append(float((a - b)[ok].abs().max()) / float(b.abs().max()))
            print('uv per-pixel %s: torch vs fused front-end, %s gradient max diff / max = %.3e'
                  % (mode, 'vertex' if k == len(grads[True]) - 1 else 'image', errs[-1]))
        assert max(errs[:-1]) <= 2e-3 and errs[-1] <= 2e-2, (mode, errs)


def _smooth_image(h, w):
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    return np.stack((0.5 + 0.4 * np.sin(2 * np.pi * x) * np.cos(np.pi * y), 0.5 + 0.3 * np.cos(2 * np.pi * (x + y)),
                     0.3 + 0.4 * y * x), axis=2).astype(np.float32)


def test_bake_converges_to_per_pixel_sampling(tmp_path):
    """The bake path's render approaches the per-pixel render as texture_size grows: catches a flip or orientation mistake
    that the restatement, written by the same hand, would share."""
    import torch
    import neural_renderer_amd as nr
    from test_uv_textures_gpu import _write_sphere
    path, _ = _write_sphere(str(tmp_path))
    v, f = nr.load_obj(path)[:2]
    vertices, faces = torch.tensor(v, device='cuda')[None], torch.tensor(f, device='cuda')[None]
    image = _cuda(_smooth_image(64, 128))
    errs = []
    with torch.no_grad():
        for ts in (2, 4, 8, 16):
            layout = nr.UVLayout.from_obj(path, texture_size=ts)
            r = nr.Renderer()
            r.image_size = 128
            r.eye = nr.get_points_from_angles(2.5, 20, 30)
            r.face_light = True
            per_pixel = r.render(vertices, faces, nr.UVImages(layout, [image]))
            baked = r.render(vertices, faces, nr.bake_uv_textures([image], layout))
            mask = nr.Renderer.render_silhouettes(r, vertices, faces) > 0
            errs.append(float((per_pixel - baked).abs().mean(1)[mask].mean()))
    print('uv per-pixel: mean |bake - per-pixel| over textured pixels at ts = 2, 4, 8, 16: %s'
          % ', '.join('%.3e' % e for e in errs))
    assert all(a > b for a, b in zip(errs, errs[1:]))
    assert errs[-1] <= 2 * ERR_TS16


# measured on the MI355X: 7.56e-4, 3.93e-4, 6.23e-5, 1.33e-5 at ts = 2, 4, 8, 16
ERR_TS16 = 1.33e-5


def _fit(path, per_pixel, steps=150):
    import torch
    import neural_renderer_amd as nr
    layout = nr.UVLayout.from_obj(path, texture_size=4)
    v, f = nr.load_obj(path)[:2]
    B = 8
    vertices = torch.tensor(v, device='cuda')[None].expand(B, -1, -1).contiguous()
    faces = torch.tensor(f, device='cuda')[None].expand(B, -1, -1).contiguous()
    r = nr.Renderer()
    r.image_size = 64
    r.eye = torch.tensor(np.stack([nr.get_points_from_angles(2.5, 20.0 * (i % 2), 45.0 * i) for i in range(B)]),
                         dtype=torch.float32, device='cuda')
    tex = nr.UVTextures(layout).cuda()
    board = tex.images[0].detach().clone()

    def textures():
        return tex.uv_images() if per_pixel else tex(B)
    with torch.no_grad():
        target = r.render(vertices, faces, textures())
        tex.images[0].fill_(0.5)
    opt = torch.optim.Adam(tex.parameters(), lr=0.03)
    losses, seen = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss = ((r.render(vertices, faces, textures()) - target) ** 2).mean()
        loss.backward()
        if seen is None:
            seen = tex.images[0].grad.abs().sum(2) > 0
            err0 = float((tex.images[0].detach() - board).abs()[seen].mean())
        losses.append(float(loss))
        opt.step()
    err = float((tex.images[0].detach() - board).abs()[seen].mean())
    return losses[0], losses[-1], err0, err, int(seen.sum())


def test_fit_grey_image_to_checkerboard_views_per_pixel(tmp_path):
    from test_uv_textures_gpu import _write_sphere
    path, _ = _write_sphere(str(tmp_path))
    l0, l1, e0, e1, n = _fit(path, True)
    b = _fit(path, False)
    # measured on the MI355X: per pixel loss 1.2e-2 -> 1.8e-9, seen-texel error 0.234 -> 0.011 (6 316 seen pixels); baked
    # (the existing fit's scene and target) 7.2e-3 -> 4.0e-7, 0.234 -> 0.057
    print('fit per pixel: loss %.3e -> %.3e, seen-texel error %.4f -> %.4f (%d seen pixels)' % (l0, l1, e0, e1, n))
    print('fit baked:     loss %.3e -> %.3e, seen-texel error %.4f -> %.4f (%d seen pixels)' % b)
    assert l1 < 0.05 * l0
    assert e1 < 0.5 * e0


def test_graph_capture_equals_eager(tmp_path):
    import torch
    import neural_renderer_amd as nr
    layout, vertices, faces = _display(tmp_path)
    B = 2
    vertices = vertices.expand(B, -1, -1).contiguous().requires_grad_(True)
    faces = faces.expand(B, -1, -1).contiguous()
    rng = np.random.default_rng(12)
    x = [torch.zeros((B,) + tuple(s) + (3,), device='cuda', requires_grad=True) for s in layout.image_sizes]
    r = nr.Renderer()
    r.image_size = 64
    r.eye = nr.get_points_from_angles(2, 15, -90)
    w = torch.zeros((B, 3, 64, 64), device='cuda')
    out = torch.zeros((B, 3, 64, 64), device='cuda')

    def step():
        img = r.render(vertices, faces, nr.UVImages(layout, x))
        out.copy_(img)
        return torch.autograd.grad((img * w).sum(), [vertices] + x)
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        for xi in x:
            xi.copy_(torch.tensor(rng.uniform(0, 1, xi.shape).astype(np.float32)))
        w.copy_(torch.tensor(rng.normal(size=w.shape).astype(np.float32)))
    replay()
    torch.cuda.synchronize()
    got_img, got = out.clone(), [g.clone() for g in grads[0]]
    eager = step()
    assert torch.equal(got_img, out)
    for a, b in zip(got, eager):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
