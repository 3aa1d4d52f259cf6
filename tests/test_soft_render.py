"""CPU checks of soft colour rendering (neural_renderer_amd/soft_render.py, Renderer.render_soft): soft_render_torch in
float64 against the restatement of tests/soft_render_ref.py, the restatement's analytic gradient against central differences
of itself, the sensitivity of its float32 bounds, the masked-pixel and doubt caps of every case the GPU file runs, argument
errors of the Python function and of the three ABI entries, the renderer on CPU tensors, and the semantics."""
import numpy as np
import pytest
import torch

import soft_render_ref as R

BG = (0.2, 0.3, 0.4)


def _colors(B, F, seed=1):
    return np.random.default_rng(seed).uniform(0, 1, (B, F, 3)).astype(np.float32)


def _torch64(faces, colors, S, sigma, gamma, g, **kw):
    import neural_renderer_amd as nr
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(colors, dtype=torch.float64, requires_grad=True)
    out = nr.soft_render_torch(ft, ct, S, sigma, gamma, 0.1, 100.0, kw.get('eps', 1e-3), kw.get('background', BG))
    out.backward(torch.tensor(g))
    return out.detach().numpy(), ft.grad.numpy(), ct.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. torch in float64 against the restatement

@pytest.mark.parametrize('S,sigma,gamma', [(16, 1e-3, 1e-1), (20, 1e-3, 1e-4), (16, 1.0, 1e-1), (16, 1e-6, 1e-4)])
def test_torch_float64_equals_the_restatement(S, sigma, gamma):
    """Values to 1e-12, autograd gradients to 1e-9 of the restatement's term magnitudes (analytic)."""
    faces = R.sphere_faces(1, 2)
    colors = _colors(2, faces.shape[1])
    g = np.random.default_rng(2).normal(size=(2, 4, S, S))
    ref = R.restate(faces, colors, S, sigma, gamma, background=BG, g=g)
    out, gf, gc = _torch64(faces, colors, S, sigma, gamma, ref.g)
    assert np.abs(out - ref.rgba).max() <= 1e-12
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_colors).max() > 0
    assert R.worst_ratio(gf, ref.grad_faces, 1e-9 * ref.grad_faces_mag) <= 1
    assert R.worst_ratio(gc, ref.grad_colors, 1e-9 * ref.grad_colors_mag) <= 1


def test_shared_colors_in_torch():
    import neural_renderer_amd as nr
    faces = torch.tensor(R.sphere_faces(1, 3), dtype=torch.float64)
    colors = torch.tensor(_colors(1, 80), dtype=torch.float64, requires_grad=True)
    g = torch.tensor(np.random.default_rng(3).normal(size=(3, 4, 16, 16)))
    nr.soft_render_torch(faces, colors, 16, 1e-3, 1e-2).backward(g)
    wide = colors.detach().expand(3, 80, 3).clone().requires_grad_(True)
    nr.soft_render_torch(faces, wide, 16, 1e-3, 1e-2).backward(g)
    assert tuple(colors.grad.shape) == (1, 80, 3)
    assert torch.allclose(colors.grad[0], wide.grad.sum(0), rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# 2. central differences of the restatement itself

ONE = np.array([[[[-0.55, -0.45, 1.2], [0.62, -0.33, 1.9], [0.08, 0.71, 2.6]]]])
TWO = np.concatenate((ONE, np.array([[[[-0.3, -0.6, 2.2], [0.7, 0.1, 1.4], [-0.45, 0.52, 1.7]]]])), 1)


@pytest.mark.parametrize('faces,sigma,gamma', [(ONE, 3e-2, 5e-2), (TWO, 3e-2, 5e-2), (TWO, 1e-1, 1e-2)],
                         ids=['one', 'two', 'two-sharp'])
def test_analytic_gradient_against_central_differences(faces, sigma, gamma):
    """S = 8, away from doubt: every face entry (z included) and every colour entry; the case has outside pixels with a free
    t, inside pixels and pixels with a clamped t."""
    S, F = 8, faces.shape[1]
    colors = _colors(1, F, 4).astype(np.float64)
    g = np.random.default_rng(5).normal(size=(1, 4, S, S))
    ref = R.restate(faces, colors, S, sigma, gamma, background=BG, g=g)
    assert ref.masked == [0] and ref.doubt == [0]
    loss = lambda f, c: float((R.restate(f, c, S, sigma, gamma, background=BG).rgba * g).sum())
    hstep = 1e-6
    for idx in np.ndindex(faces.shape):
        up, dn = faces.copy(), faces.copy()
        up[idx] += hstep
        dn[idx] -= hstep
        fd = (loss(up, colors) - loss(dn, colors)) / (2 * hstep)
        assert abs(fd - ref.grad_faces[idx]) <= 1e-6 * max(1.0, ref.grad_faces_mag[idx]), (idx, fd, ref.grad_faces[idx])
    for idx in np.ndindex(colors.shape):
        up, dn = colors.copy(), colors.copy()
        up[idx] += hstep
        dn[idx] -= hstep
        fd = (loss(faces, up) - loss(faces, dn)) / (2 * hstep)
        assert abs(fd - ref.grad_colors[idx]) <= 1e-6 * max(1.0, ref.grad_colors_mag[idx]), (idx, fd)
    assert np.abs(ref.grad_faces[..., 2]).min() > 0


def test_the_difference_case_has_every_kind_of_pair():
    import neural_renderer_amd as nr
    ft = torch.tensor(TWO, requires_grad=True)
    # a free t moves the depth: with the colours' and alpha's gradients off, x and y still get something through zn
    out = nr.soft_render_torch(ft, torch.tensor(_colors(1, 2, 4), dtype=torch.float64), 8, 3e-2, 5e-2)
    out[:, :3].sum().backward()
    assert ft.grad[..., 2].abs().min() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the bounds can tell wrong from right

@pytest.mark.parametrize('variant,what', [('no_z', 'grad_faces'), ('no_background', 'rgba'), ('no_1mD', 'grad_faces')])
def test_bounds_are_not_vacuous(variant, what):
    """The first sphere case of the GPU file: the restatement with one defect misses its own bounds."""
    import test_soft_render_gpu as G
    mesh, B, S, sigma, gamma = G.CASES[0]
    faces, colors, ref = G.reference(mesh, B, S, sigma, gamma)
    with np.errstate(all='ignore'):   # (without the background a pixel without a pair divides by 0)
        bad = R.restate(faces, colors, S, sigma, gamma, background=G.BG, g=ref.g, variant=variant)
    if what == 'rgba':
        ratio = R.masked_ratio(bad.rgba, ref.rgba, ref.rgba_bound, ref.mask)
    else:
        ratio = R.worst_ratio(bad.grad_faces, ref.grad_faces, ref.grad_faces_bound)
    assert ratio > 1, ratio


def test_caps_of_every_gpu_case():
    """Conditions, not measurements: masked pixels <= 1 % of the pixels with a taken pair, pairs in doubt <= 2 % of the
    taken pairs, in every case and image of the GPU file."""
    import test_soft_render_gpu as G
    for case in G.CASES:
        _, _, ref = G.reference(*case)
        assert ref.masked_share <= 0.01, (case, ref.masked, ref.with_pair)
        assert ref.doubt_share <= 0.02, (case, ref.doubt, ref.pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument errors

def test_argument_errors_of_the_python_function():
    import neural_renderer_amd as nr
    f, c = torch.rand(2, 5, 3, 3) + 1, torch.rand(2, 5, 3)
    ok = dict(image_size=8, sigma=1e-3, gamma=1e-2)
    assert nr.soft_render(f, c, **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render(f, c[:1], **ok).shape == (2, 4, 8, 8)
    bad = [((f[0], c), {}), ((f, c[:, :4]), {}), ((f, c[..., :2]), {}), ((f, torch.rand(3, 5, 3)), {}), ((f.long(), c), {}),
           ((f, c), dict(image_size=0)), ((f, c), dict(image_size=8.0)), ((f, c), dict(sigma=0)), ((f, c), dict(sigma=float('nan'))),
           ((f, c), dict(gamma=0)), ((f, c), dict(gamma=float('inf'))), ((f, c), dict(gamma='1')), ((f, c), dict(near=1, far=1)),
           ((f, c), dict(far=float('inf'))), ((f, c), dict(eps=float('nan'))), ((f, c), dict(background_color=(0, 0))),
           ((f, c), dict(background_color=(0, 0, float('inf')))), ((f, c), dict(background_color=1.0)),
           ((f, c), dict(implementation='cuda')), ((f, c), dict(implementation='hip')),
           ((f.double(), c.double()), dict(implementation='hip'))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            nr.soft_render(*args, **dict(ok, **kw))


def test_argument_errors_of_the_abi_need_no_gpu():
    """NR_E_* before any launch (the pattern of tests/test_abi.py's host-only tests): fake non-NULL pointers never reach a
    kernel."""
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert lib.nr_soft_render_workspace_bytes(3, 80, 32) >= 3 * 80 * 80
    assert lib.nr_soft_render_workspace_bytes(0, 80, 32) == 0 and lib.nr_soft_render_workspace_bytes(1, 80, 20000) == 0
    assert lib.nr_soft_render_workspace_bytes(1, 2 ** 24 + 1, 8) == 0
    num = dict(sigma=1e-3, gamma=1e-2, near=0.1, far=100.0, eps=1e-3, r=0.0, g=0.0, b=0.0)

    def fwd(ptrs=(1, 1, 1, 1, 1), sizes=(1, 4, 8, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_render_forward(*ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'], n['g'],
                                          n['b'], ws[0], ws[1], None)

    def bwd(ptrs=(1,) * 8, sizes=(1, 4, 8, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_render_backward(*ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'], n['g'],
                                           n['b'], ws[0], ws[1], None)
    nan, inf = float('nan'), float('inf')
    for call, count in ((fwd, 5), (bwd, 8)):
        for i in range(count):
            assert call(ptrs=tuple(None if j == i else 1 for j in range(count))) == -1, i
        for sizes in ((0, 4, 8, 1), (1, 0, 8, 1), (1, 4, 0, 1), (70000, 4, 8, 1), (1, 4, 20000, 1), (1, 2 ** 24 + 1, 8, 1)):
            assert call(sizes=sizes) == -2, sizes
        for kw in (dict(sigma=0.0), dict(sigma=1e31), dict(sigma=nan), dict(gamma=0.0), dict(gamma=1e-31), dict(gamma=nan),
                   dict(near=1.0, far=1.0), dict(near=2.0, far=1.0), dict(near=nan), dict(far=inf), dict(eps=nan), dict(eps=inf),
                   dict(r=nan), dict(g=inf), dict(b=-inf)):
            assert call(**kw) == -4, kw
        assert call(sizes=(1, 4, 8, 2)) == -4
        assert call(ws=(None, 1 << 20)) == -3 and call(ws=(1, 16)) == -3


# ---------------------------------------------------------------------------------------------------------------------
# 5. the renderer on CPU tensors

def _scene(B=2):
    import neural_renderer_amd as nr
    v, f = nr.icosphere(1, 0.8)
    return v[None].repeat(B, 1, 1), f[None].repeat(B, 1, 1)


def _renderer(S=16):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.image_size = S
    r.eye = nr.get_points_from_angles(2.732, 20, 30)
    r.soft_sigma, r.soft_gamma = 1e-3, 1e-2
    r.background_color = [0.1, 0.6, 0.3]
    return r


def test_render_soft_shapes_sources_and_background():
    import neural_renderer_amd as nr
    v, f = _scene()
    r = _renderer()
    assert r.soft_gamma == 1e-2 and nr.Renderer().soft_gamma == 1e-4 and nr.Renderer().soft_eps == 1e-3
    F = f.shape[1]
    face_colors = torch.rand(2, F, 3)
    img = r.render_soft(v, f, face_colors)
    assert img.shape == (2, 4, 16, 16) and torch.isfinite(img).all()
    assert torch.equal(r.render_soft(v, f, face_colors[0]), r.render_soft(v, f, face_colors[:1]))   # [F,3] is [1,F,3]
    # far from everything: the background, alpha 0
    corner = img[:, :, 0, 0]
    assert torch.allclose(corner[:, :3], torch.tensor(r.background_color).expand(2, 3), atol=1e-6) and corner[:, 3].abs().max() < 1e-6
    assert img[:, 3].max() > 0.99
    # constant vertex colours == a face-colour tensor of that colour; a constant cube likewise
    colour = torch.tensor([0.9, 0.5, 0.2])
    by_face = r.render_soft(v, f, colour.expand(1, F, 3))
    vc = nr.VertexColors(colour.expand(v.shape[1], 3).clone())
    assert torch.allclose(r.render_soft(v, f, vc), by_face, atol=1e-6)
    cubes = colour.expand(1, F, 2, 2, 2, 3).clone()
    assert torch.allclose(r.render_soft(v, f, cubes), by_face, atol=1e-6)
    # the light of the front copy enters: no light, no colour
    dark = _renderer()
    dark.light_intensity_ambient, dark.light_intensity_directional = 0.0, 0.0
    centre = dark.render_soft(v, f, face_colors)[:, :3, 8, 8]
    assert centre.abs().max() < 1e-6
    # sigma and gamma arguments, ignored attributes
    assert not torch.equal(r.render_soft(v, f, face_colors, sigma=1e-2), img)
    assert not torch.equal(r.render_soft(v, f, face_colors, gamma=1.0), img)
    r.anti_aliasing, r.shading = False, 'smooth'
    assert torch.equal(r.render_soft(v, f, face_colors), img)
    with pytest.raises(ValueError):
        r.render_soft(v, f, torch.rand(2, F, 4))


def test_render_soft_gradients_reach_vertices_colours_and_cubes():
    import neural_renderer_amd as nr
    v, f = _scene(1)
    v.requires_grad_(True)
    r = _renderer()
    vcol = torch.rand(v.shape[1], 3, requires_grad=True)
    w = torch.tensor(np.random.default_rng(7).normal(size=(1, 4, 16, 16)), dtype=torch.float32)
    (r.render_soft(v, f, nr.VertexColors(vcol)) * w).sum().backward()
    assert torch.isfinite(v.grad).all() and v.grad[..., 2].abs().sum() > 0 and vcol.grad.abs().sum() > 0
    cubes = torch.rand(1, f.shape[1], 2, 2, 2, 3, requires_grad=True)
    (r.render_soft(v, f, cubes) * w).sum().backward()
    assert cubes.grad.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. semantics: two parallel triangles, one behind the other

FRONT = [[-0.6, -0.5, 1.0], [0.6, -0.5, 1.0], [0.0, 0.6, 1.0]]
BACK = [[-0.6, -0.5, 2.0], [0.6, -0.5, 2.0], [0.0, 0.6, 2.0]]
RED, BLUE = [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]


def _pair(front_first=True, gamma=1e-4, sigma=1e-4, S=16):
    import neural_renderer_amd as nr
    faces = torch.tensor([[FRONT, BACK] if front_first else [BACK, FRONT]], dtype=torch.float64)
    colors = torch.tensor([[RED, BLUE]], dtype=torch.float64)
    return nr.soft_render_torch(faces, colors, S, sigma, gamma, 0.1, 100.0, 1e-3, BG), faces


def test_depth_order_and_background():
    img, _ = _pair(True)
    centre, corner = img[0, :, 8, 8], img[0, :, 0, 0]
    assert torch.allclose(centre[:3], torch.tensor(RED, dtype=torch.float64), atol=1e-6) and centre[3] > 0.999   # face 0 is in front
    swapped, _ = _pair(False)
    assert torch.allclose(swapped[0, :3, 8, 8], torch.tensor(BLUE, dtype=torch.float64), atol=1e-6)   # now face 1's colour
    assert torch.allclose(corner[:3], torch.tensor(BG, dtype=torch.float64), atol=1e-12) and corner[3] == 0
    # a large gamma mixes the two
    mixed, _ = _pair(True, gamma=10.0)
    assert 0.2 < mixed[0, 0, 8, 8] < 0.8 and 0.2 < mixed[0, 2, 8, 8] < 0.8


def test_a_hidden_face_gets_a_gradient_that_pulls_it_forward():
    """The target is the hidden face's colour: descent on z moves the hidden face towards the camera and the occluder away."""
    import neural_renderer_amd as nr
    faces = torch.tensor([[FRONT, BACK]], dtype=torch.float64, requires_grad=True)
    colors = torch.tensor([[RED, BLUE]], dtype=torch.float64)
    img = nr.soft_render_torch(faces, colors, 16, 1e-4, 0.05, 0.1, 100.0, 1e-3, BG)
    target = torch.tensor(BLUE, dtype=torch.float64)[None, :, None, None]
    ((img[:, :3] - target) ** 2).sum().backward()
    gz = faces.grad[0, :, :, 2]
    assert (gz[1] > 0).all() and (gz[0] < 0).all()   # z - lr * grad: the back face comes nearer, the front one recedes


@pytest.mark.parametrize('sigma', [1e-4, 1e-2, 1.0])
def test_alpha_agrees_with_the_soft_silhouette(sigma):
    """No zero-area faces: alpha differs from soft_silhouettes_torch by the pairs beyond the cutoff alone, D < 2^-24 each."""
    import neural_renderer_amd as nr
    faces = torch.tensor(R.sphere_faces(1, 2), dtype=torch.float64)
    F = faces.shape[1]
    img = nr.soft_render_torch(faces, torch.rand(2, F, 3, dtype=torch.float64), 20, sigma, 1e-2)
    sil = nr.soft_silhouettes_torch(faces, 20, sigma)
    assert (img[:, 3] - sil).abs().max() <= F * 2.0 ** -24
    assert (img[:, 3] <= sil + 1e-15).all()
