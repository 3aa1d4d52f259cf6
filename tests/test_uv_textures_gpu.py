"""Learnable UV texture images on the GPU (include/nr_hip.h nr_bake_uv_textures[_backward], nr_uv_texture_map;
neural_renderer_amd/uv_textures.py): parity with load_obj's bake, the adjoint, reproducibility, the renderer's three texture
paths, an end-to-end fit, the save / load round trip and graph capture."""
import os

import numpy as np
import pytest

import helpers as H
import uv_ref as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def display_obj(tmp_path_factory):
    return H.write_display_model(str(tmp_path_factory.mktemp('display_uv_gpu')))


def _cuda(images):
    import torch
    return [torch.tensor(np.ascontiguousarray(im), device='cuda') for im in images]


def _off_origin(t):
    return t.reshape(t.shape[0], -1, 3)[:, 1:]


@pytest.mark.parametrize('ts', [2, 4, 6])
def test_bake_equals_load_obj(display_obj, ts):
    import neural_renderer_amd as nr
    _, _, t0 = nr.load_obj(display_obj, load_texture=True, texture_size=ts)
    layout = nr.UVLayout.from_obj(display_obj, texture_size=ts)
    got = nr.bake_uv_textures(_cuda(layout.images), layout)[0].cpu().numpy()
    assert got.shape == t0.shape
    textured = layout.face_image >= 0
    assert np.array_equal(got[~textured], t0[~textured])
    assert np.array_equal(_off_origin(got[textured]), _off_origin(t0[textured]))
    assert np.isfinite(got).all()
    want = U.bake(layout.images, layout.faces_uv, layout.face_image, layout.base, ts)
    assert np.array_equal(got[:, 0, 0, 0], want[:, 0, 0, 0])


def _fuzz_case(rng):
    M = int(rng.integers(1, 4))
    sizes = []
    for _ in range(M):
        kind = rng.uniform()
        sizes.append((1, 1) if kind < 0.2 else (int(rng.integers(1, 40)), int(rng.integers(1, 70))))
    ts = int(rng.choice([2, 3, 4, 5]))
    F = int(rng.integers(1, 300))
    uv, face_image, base = U.random_layout(rng, F, ts, sizes)
    return sizes, ts, uv, face_image, base


@pytest.mark.parametrize('seed', range(6))
def test_fuzz_forward_and_adjoint(seed):
    import torch
    import neural_renderer_amd as nr
    rng = np.random.default_rng(100 + seed)
    for _ in range(4):
        sizes, ts, uv, face_image, base = _fuzz_case(rng)
        layout = nr.UVLayout(uv, face_image, base, sizes)
        Bi = int(rng.integers(1, 3))
        images = [rng.uniform(0, 1, (Bi, h, w, 3)).astype(np.float32) for h, w in sizes]
        x = [torch.tensor(im, device='cuda', requires_grad=True) for im in images]
        out = nr.bake_uv_textures(x, layout)
        g = rng.normal(size=out.shape).astype(np.float32)
        out.backward(torch.tensor(g, device='cuda'))
        got = out.detach().cpu().numpy()
        for b in range(Bi):
            want = U.bake([im[b] for im in images], uv, face_image, base, ts)
            assert np.array_equal(got[b], want)
            ref, mag = U.bake_adjoint(g[b], uv, face_image, sizes, ts)
            for m in range(len(sizes)):
                gm = x[m].grad[b].cpu().numpy().astype(np.float64)
                assert (np.abs(gm - ref[m]) <= 1e-6 * mag[m]).all()


def test_backward_reproducible_and_batch_equals_singles(display_obj):
    import torch
    import neural_renderer_amd as nr
    layout = nr.UVLayout.from_obj(display_obj, texture_size=4)
    rng = np.random.default_rng(3)
    images = [rng.uniform(0, 1, (4,) + tuple(s) + (3,)).astype(np.float32) for s in layout.image_sizes]
    g = torch.tensor(rng.normal(size=(4, layout.num_faces, 4, 4, 4, 3)).astype(np.float32), device='cuda')

    def run(imgs, grad):
        x = [torch.tensor(im, device='cuda', requires_grad=True) for im in imgs]
        out = nr.bake_uv_textures(x, layout)
        out.backward(grad)
        return out.detach(), [xi.grad for xi in x]
    out, grads = run(images, g)
    out2, grads2 = run(images, g)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    for b in range(4):
        ob, gb = run([im[b:b + 1] for im in images], g[b:b + 1])
        assert torch.equal(ob[0], out[b])
        assert all(torch.equal(x[0], y[b]) for x, y in zip(gb, grads))


def _renderer(mode):
    import torch
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.image_size = 64
    r.eye = nr.get_points_from_angles(2, 15, -90)
    if mode == 'face_light':
        r.face_light = True
    elif mode == 'lit':
        r.face_light = False
    else:   # a tensor light direction sends the call through the module-by-module front-end (fill_back on)
        r.face_light = False
        r.light_direction = torch.tensor([0.0, 1.0, 0.0], device='cuda')
    return r


def test_gradients_reach_images_on_every_renderer_path(display_obj):
    """The fused front-end with face_light, the lit-texture path and the torch front-end with fill_back, all fed by
    UVTextures.  The lit path differs from face_light only in the rounding order of the light product.  The torch
    front-end projects the vertices with other roundings, so a few edge pixels of the 64 x 64 image see another face
    (measured: 3 of 12 288 values differ, by up to 0.08): the upstream gradient is zeroed on the pixels where the three
    renders differ by more than 1e-5, and the image gradients are compared on what remains."""
    import torch
    import neural_renderer_amd as nr
    layout = nr.UVLayout.from_obj(display_obj, texture_size=4)
    v, f = nr.load_obj(display_obj)[:2]
    vertices = torch.tensor(v, device='cuda')[None]
    faces = torch.tensor(f, device='cuda')[None]
    tex = nr.UVTextures(layout).cuda()
    modes = ('face_light', 'lit', 'torch')
    with torch.no_grad():
        images = {m: _renderer(m).render(vertices, faces, tex(1)) for m in modes}
    same = torch.ones_like(images['lit'][:, :1], dtype=torch.bool)
    for m in modes[1:]:
        same &= ((images[m] - images['face_light']).abs() <= 1e-5).all(1, keepdim=True)
    assert float(same.float().mean()) > 0.99
    w = torch.tensor(np.random.default_rng(5).normal(size=images['lit'].shape).astype(np.float32), device='cuda') * same
    grads = {}
    for m in modes:
        r = _renderer(m)
        for p in tex.images:
            p.grad = None
        (r.render(vertices, faces, tex(1)) * w).sum().backward()
        assert r.last_frontend == ('torch' if m == 'torch' else 'fused')
        grads[m] = [p.grad.clone() for p in tex.images]
        assert all(torch.isfinite(g).all() and (g != 0).any() for g in grads[m]), m
    # Measured on the MI355X: lit 0 (bit-equal), torch 5.3e-6 of the largest entry.  lit: 1e-5 allows for the light
    # product's rounding order (3e-7 of the images, tests/test_face_light_gpu.py) summed over a pixel's texels.  torch: the
    # projected vertices differ in the last bits, which moves a pixel's barycentric weights by more than an ulp near the
    # edges of small faces, so 1e-4 (19x the measured value).
    for m, tol in (('lit', 1e-5), ('torch', 1e-4)):
        for a, b in zip(grads[m], grads['face_light']):
            err = float((a - b).abs().max()) / float(b.abs().max())
            print('renderer paths: %s vs face_light, image gradient max diff / max = %.3e' % (m, err))
            assert err <= tol, m


def _write_sphere(dirpath, n_lat=16, n_lon=32, checker=(64, 128)):
    """A UV sphere as OBJ + MTL + PNG with a checkerboard; returns the path and the checkerboard [H,W,3] in [0,1]."""
    from PIL import Image
    h, w = checker
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    board = (((rows // 8) + (cols // 8)) % 2).astype(np.float32)
    image = np.stack((0.1 + 0.8 * board, 0.2 + 0.6 * (1 - board), np.full_like(board, 0.5)), axis=2)
    q = np.floor(image * 255 + 0.5).astype(np.uint8)
    Image.fromarray(q).save(os.path.join(dirpath, 'checker.png'))
    with open(os.path.join(dirpath, 'sphere.mtl'), 'w') as fh:
        fh.write('newmtl skin\nKd 1 1 1\nmap_Kd checker.png\n')
    lines = ['mtllib sphere.mtl\n']
    for i in range(n_lat + 1):
        th = np.pi * i / n_lat
        for j in range(n_lon + 1):
            ph = 2 * np.pi * j / n_lon
            lines.append('v %.6f %.6f %.6f\n' % (np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
            lines.append('vt %.6f %.6f\n' % (j / n_lon, 1 - i / n_lat))
    lines.append('usemtl skin\n')
    for i in range(n_lat):
        for j in range(n_lon):
            a = i * (n_lon + 1) + j + 1
            b, c, d = a + 1, a + n_lon + 1, a + n_lon + 2
            lines.append('f %d/%d %d/%d %d/%d\n' % (a, a, c, c, b, b))
            lines.append('f %d/%d %d/%d %d/%d\n' % (b, b, c, c, d, d))
    path = os.path.join(dirpath, 'sphere.obj')
    with open(path, 'w') as fh:
        fh.writelines(lines)
    return path, q.astype(np.float32) / np.float32(255)


def test_fit_grey_image_to_checkerboard_views(tmp_path):
    import torch
    import neural_renderer_amd as nr
    path, board = _write_sphere(str(tmp_path))
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
    with torch.no_grad():
        target = r.render(vertices, faces, tex(B))
        tex.images[0].fill_(0.5)
    opt = torch.optim.Adam(tex.parameters(), lr=0.03)
    board_d = torch.tensor(board, device='cuda')
    losses, seen = [], None
    for step in range(150):
        opt.zero_grad()
        loss = ((r.render(vertices, faces, tex(B)) - target) ** 2).mean()
        loss.backward()
        if seen is None:
            seen = tex.images[0].grad.abs().sum(2) > 0
            err0 = float((tex.images[0].detach() - board_d).abs()[seen].mean())
        losses.append(float(loss))
        opt.step()
    err = float((tex.images[0].detach() - board_d).abs()[seen].mean())
    print('fit: loss %.3e -> %.3e, seen-texel error %.4f -> %.4f (%d seen pixels)'
          % (losses[0], losses[-1], err0, err, int(seen.sum())))
    # measured on the MI355X: loss 7.2e-3 -> 4.0e-7, seen-texel error 0.234 -> 0.057 (6 624 seen pixels)
    assert losses[-1] < 0.05 * losses[0]
    assert err < 0.5 * err0


def test_save_obj_round_trip(display_obj, tmp_path):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd.uv_textures import quantize
    ts = 4
    layout = nr.UVLayout.from_obj(display_obj, texture_size=ts)
    tex = nr.UVTextures(layout).cuda()
    rng = np.random.default_rng(9)
    with torch.no_grad():
        for p in tex.images:
            p.copy_(torch.tensor(rng.uniform(-0.2, 1.2, p.shape).astype(np.float32)))
    v, f = nr.load_obj(display_obj, normalization=False)[:2]
    out = str(tmp_path / 'learned.obj')
    tex.save_obj(out, v, f)
    v2, f2, t2 = nr.load_obj(out, normalization=False, load_texture=True, texture_size=ts)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    q = [quantize(p.detach().cpu().numpy()).astype(np.float32) / np.float32(255) for p in tex.images]
    want = nr.bake_uv_textures(_cuda(q), layout)[0].cpu().numpy()
    textured = layout.face_image >= 0
    assert np.array_equal(t2[~textured], want[~textured])
    assert np.array_equal(_off_origin(t2[textured]), _off_origin(want[textured]))
    layout2 = nr.UVLayout.from_obj(out, texture_size=ts)
    assert np.array_equal(layout2.faces_uv, layout.faces_uv)


def test_graph_capture_equals_eager(display_obj):
    import torch
    import neural_renderer_amd as nr
    layout = nr.UVLayout.from_obj(display_obj, texture_size=4)
    rng = np.random.default_rng(11)
    shapes = [(2,) + tuple(s) + (3,) for s in layout.image_sizes]
    x = [torch.zeros(s, device='cuda', requires_grad=True) for s in shapes]
    gout = torch.zeros((2, layout.num_faces, 4, 4, 4, 3), device='cuda')

    def step():
        out = nr.bake_uv_textures(x, layout)
        return (out,) + torch.autograd.grad(out, x, gout)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()          # warm-up: uploads the layout and builds the inverse map
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    new_x = [rng.uniform(0, 1, s).astype(np.float32) for s in shapes]
    new_g = rng.normal(size=gout.shape).astype(np.float32)
    with torch.no_grad():
        for xi, n in zip(x, new_x):
            xi.copy_(torch.tensor(n))
        gout.copy_(torch.tensor(new_g))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert all(torch.equal(a, b) for a, b in zip(static, eager))
