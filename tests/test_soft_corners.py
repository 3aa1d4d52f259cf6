"""CPU checks of soft colour rendering with corner colours (soft_render with colors [B|1,F,3,3],
Renderer.render_soft(per_pixel=True)): soft_render_torch in float64 against the restatement of tests/soft_render_ref.py, the
restatement's analytic gradient against central differences of itself, equal corners against the flat definition, shared
colours, the sensitivity of the float32 bounds, the masked-pixel and doubt caps of every case the GPU file runs, argument
errors of the Python function and of the three ABI entries, and the renderer on CPU tensors."""
import numpy as np
import pytest
import torch

import soft_render_ref as R
from test_soft_render import TWO

BG = (0.2, 0.3, 0.4)


def _colors(B, F, seed=1):
    return np.random.default_rng(seed).uniform(0, 1, (B, F, 3, 3)).astype(np.float32)


def _torch64(faces, colors, S, sigma, gamma, g):
    import neural_renderer_amd as nr
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(colors, dtype=torch.float64, requires_grad=True)
    out = nr.soft_render_torch(ft, ct, S, sigma, gamma, 0.1, 100.0, 1e-3, BG)
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
    assert tuple(gc.shape) == (2, faces.shape[1], 3, 3)
    assert np.abs(out - ref.rgba).max() <= 1e-12
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_colors).max() > 0
    assert R.worst_ratio(gf, ref.grad_faces, 1e-9 * ref.grad_faces_mag) <= 1
    assert R.worst_ratio(gc, ref.grad_colors, 1e-9 * ref.grad_colors_mag) <= 1


def test_shared_colors_in_torch():
    import neural_renderer_amd as nr
    faces = torch.tensor(R.sphere_faces(1, 3), dtype=torch.float64)
    colors = torch.tensor(_colors(1, 80), dtype=torch.float64, requires_grad=True)
    g = torch.tensor(np.random.default_rng(3).normal(size=(3, 4, 16, 16)))
    shared = nr.soft_render_torch(faces, colors, 16, 1e-3, 1e-2)
    shared.backward(g)
    wide = colors.detach().expand(3, 80, 3, 3).clone().requires_grad_(True)
    out = nr.soft_render_torch(faces, wide, 16, 1e-3, 1e-2)
    out.backward(g)
    assert torch.equal(shared, out)
    assert tuple(colors.grad.shape) == (1, 80, 3, 3)
    assert torch.allclose(colors.grad[0], wide.grad.sum(0), rtol=1e-12, atol=1e-14)
    # the restatement with [1,F,3,3]
    ref = R.restate(faces.numpy(), colors.detach().numpy(), 16, 1e-3, 1e-2, g=g.numpy())
    total, _ = R.shared_colors(ref)
    assert tuple(total.shape) == (1, 80, 3, 3) and np.abs(total).max() > 0
    again = torch.tensor(colors.detach().numpy(), requires_grad=True)
    nr.soft_render_torch(faces, again, 16, 1e-3, 1e-2).backward(torch.tensor(ref.g))
    assert R.worst_ratio(again.grad.numpy(), total, 1e-9 * ref.grad_colors_mag.sum(0, keepdims=True)) <= 1


def test_three_equal_corners_are_the_flat_render():
    """Float64: the image, the face gradients and the colour gradients (added over a face's corners) to 1e-12."""
    import neural_renderer_amd as nr
    faces = R.sphere_faces(1, 2)
    F = faces.shape[1]
    flat = np.random.default_rng(6).uniform(0, 1, (2, F, 3))
    g = np.random.default_rng(7).normal(size=(2, 4, 16, 16))
    outs = []
    for col in (flat, np.repeat(flat[:, :, None, :], 3, 2)):
        ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
        ct = torch.tensor(col, requires_grad=True)
        out = nr.soft_render_torch(ft, ct, 16, 1e-3, 1e-1, 0.1, 100.0, 1e-3, BG)
        out.backward(torch.tensor(g))
        outs.append((out.detach(), ft.grad, ct.grad))
    (a, af, ac), (b, bf, bc) = outs
    assert (a - b).abs().max() <= 1e-12
    assert (af - bf).abs().max() <= 1e-12 * max(1.0, float(af.abs().max()))
    assert (ac - bc.sum(2)).abs().max() <= 1e-12 * max(1.0, float(ac.abs().max()))
    ref_c = R.restate(faces, np.repeat(flat[:, :, None, :], 3, 2), 16, 1e-3, 1e-1, background=BG, g=g)
    ref_f = R.restate(faces, flat, 16, 1e-3, 1e-1, background=BG, g=g)
    assert np.abs(ref_c.rgba - ref_f.rgba).max() <= 1e-12
    assert np.abs(ref_c.grad_faces - ref_f.grad_faces).max() <= 1e-12 * max(1.0, np.abs(ref_f.grad_faces).max())
    assert np.abs(ref_c.grad_colors.sum(2) - ref_f.grad_colors).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 2. central differences of the restatement itself

@pytest.mark.parametrize('sigma,gamma', [(3e-2, 5e-2), (1e-1, 1e-2)], ids=['two', 'two-sharp'])
def test_analytic_gradient_against_central_differences(sigma, gamma):
    """S = 8 on the two-triangle case of test_soft_render.py (an inside pair, a free-t pair and a clamped-t pair), away from
    doubt: every face entry (z included) and every corner-colour entry."""
    faces, S = TWO, 8
    colors = _colors(1, 2, 4).astype(np.float64)
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
    assert np.abs(ref.grad_faces).min() > 0 and np.abs(ref.grad_colors).min() > 0


def test_the_colour_path_reaches_the_geometry():
    """The colour's own way into x, y and z: with it cut ('no_colour_path') the analytic gradient of the difference case is
    another one, in every face entry."""
    colors = _colors(1, 2, 4).astype(np.float64)
    g = np.random.default_rng(5).normal(size=(1, 4, 8, 8))
    ref = R.restate(TWO, colors, 8, 3e-2, 5e-2, background=BG, g=g)
    cut = R.restate(TWO, colors, 8, 3e-2, 5e-2, background=BG, g=g, variant='no_colour_path')
    assert (np.abs(ref.grad_faces - cut.grad_faces) > 1e-6 * ref.grad_faces_mag).all()
    assert np.array_equal(ref.grad_colors, cut.grad_colors) and np.array_equal(ref.rgba, cut.rgba)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the bounds can tell wrong from right

@pytest.mark.parametrize('variant,what', [('affine', 'rgba'), ('rotated', 'rgba'), ('no_colour_path', 'grad_faces')])
def test_bounds_are_not_vacuous(variant, what):
    """The first sphere case of the GPU file: the restatement with one defect misses its own bounds."""
    import test_soft_corners_gpu as G
    mesh, B, S, sigma, gamma = G.CASES[0]
    faces, colors, ref = G.reference(mesh, B, S, sigma, gamma)
    bad = R.restate(faces, colors, S, sigma, gamma, background=G.BG, g=ref.g, variant=variant)
    if what == 'rgba':
        ratio = R.masked_ratio(bad.rgba, ref.rgba, ref.rgba_bound, ref.mask)
    else:
        ratio = R.worst_ratio(bad.grad_faces, ref.grad_faces, ref.grad_faces_bound)
    assert ratio > 1, ratio


def test_caps_of_every_gpu_case():
    """Conditions, not measurements: masked pixels <= 1 % of the pixels with a taken pair, pairs in doubt <= 2 % of the
    taken pairs, in every case and image of the GPU file (both depend on the geometry and sigma alone)."""
    import test_soft_corners_gpu as G
    import test_soft_render_gpu as G0
    assert [c[:5] for c in G.CASES] == [c[:5] for c in G0.CASES]
    seen = {}
    for mesh, B, S, sigma, gamma in G.CASES:
        key = (mesh, B, S, sigma)
        if key not in seen:   # (no gradient asked: the forward half of the restatement is enough)
            faces = G._faces(mesh, B)
            seen[key] = R.restate(faces, np.zeros((1, faces.shape[1], 3, 3)), S, sigma, gamma)
        ref = seen[key]
        assert ref.masked_share <= 0.01, (key, ref.masked, ref.with_pair)
        assert ref.doubt_share <= 0.02, (key, ref.doubt, ref.pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument errors

def test_argument_errors_of_the_python_function_with_corner_colors():
    import neural_renderer_amd as nr
    f, c = torch.rand(2, 5, 3, 3) + 1, torch.rand(2, 5, 3, 3)
    ok = dict(image_size=8, sigma=1e-3, gamma=1e-2)
    assert nr.soft_render(f, c, **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render(f, c[:1], **ok).shape == (2, 4, 8, 8)
    bad = [((f[0], c), {}), ((f, c[:, :4]), {}), ((f, c[..., :2]), {}), ((f, c[:, :, :2]), {}), ((f, torch.rand(3, 5, 3, 3)), {}),
           ((f, c[0]), {}), ((f, c[:, :, :, :, None]), {}), ((f, c.long()), {}), ((f.long(), c), {}),
           ((f, c), dict(image_size=0)), ((f, c), dict(sigma=0)), ((f, c), dict(gamma=float('inf'))),
           ((f, c), dict(near=1, far=1)), ((f, c), dict(eps=float('nan'))), ((f, c), dict(background_color=(0, 0))),
           ((f, c), dict(implementation='cuda')), ((f, c), dict(implementation='hip')),
           ((f.double(), c.double()), dict(implementation='hip'))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            nr.soft_render(*args, **dict(ok, **kw))


def test_argument_errors_of_the_abi_need_no_gpu():
    """NR_E_* before any launch (the pattern of tests/test_soft_render.py): fake non-NULL pointers never reach a kernel."""
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    # a 96-byte record per face, then the per-image colour gradients of a call with shared colours
    assert lib.nr_soft_corners_workspace_bytes(3, 80, 32) >= 3 * 80 * (96 + 36)
    assert lib.nr_soft_corners_workspace_bytes(3, 80, 32) > lib.nr_soft_render_workspace_bytes(3, 80, 32)
    assert lib.nr_soft_corners_workspace_bytes(0, 80, 32) == 0 and lib.nr_soft_corners_workspace_bytes(1, 80, 20000) == 0
    assert lib.nr_soft_corners_workspace_bytes(1, 2 ** 24 + 1, 8) == 0
    assert lib.nr_version() == 600
    num = dict(sigma=1e-3, gamma=1e-2, near=0.1, far=100.0, eps=1e-3, r=0.0, g=0.0, b=0.0)

    def fwd(ptrs=(1, 1, 1, 1, 1), sizes=(1, 4, 8, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_corners_forward(*ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'], n['g'],
                                           n['b'], ws[0], ws[1], None)

    def bwd(ptrs=(1,) * 8, sizes=(1, 4, 8, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_corners_backward(*ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'], n['g'],
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
        # the flat entry's workspace is too small for the corner records
        assert call(ws=(1, lib.nr_soft_render_workspace_bytes(1, 4, 8))) == -3


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


def test_render_soft_per_pixel_shapes_and_sources():
    import neural_renderer_amd as nr
    v, f = _scene()
    r = _renderer()
    F, Nv = f.shape[1], v.shape[1]
    vc = nr.VertexColors(torch.rand(Nv, 3))
    img = r.render_soft(v, f, vc, per_pixel=True)
    assert img.shape == (2, 4, 16, 16) and torch.isfinite(img).all()
    assert not torch.equal(img, r.render_soft(v, f, vc))                  # the facet mean is another image
    # batched vertex colours
    assert r.render_soft(v, f, nr.VertexColors(torch.rand(2, Nv, 3)), per_pixel=True).shape == (2, 4, 16, 16)
    # a VertexColors is the corner tensor of its gather
    corner = vc.colors[f[0].long()][None]                                 # [1,F,3,3]
    by_tensor = r.render_soft(v, f, corner, per_pixel=True)
    assert torch.allclose(by_tensor, img, atol=1e-6)
    assert torch.equal(r.render_soft(v, f, corner[0], per_pixel=True), by_tensor)                 # [F,3,3] is [1,F,3,3]
    assert torch.equal(r.render_soft(v, f, corner.expand(2, F, 3, 3), per_pixel=True), by_tensor)
    # face colours at all three corners: the flat render
    face = torch.rand(2, F, 3)
    flat = r.render_soft(v, f, face)
    assert torch.allclose(r.render_soft(v, f, face, per_pixel=True), flat, atol=1e-6)
    assert torch.equal(r.render_soft(v, f, face[0], per_pixel=True), r.render_soft(v, f, face[:1], per_pixel=True))
    # constant vertex colours equal the flat render of that colour
    colour = torch.tensor([0.9, 0.5, 0.2])
    const = nr.VertexColors(colour.expand(Nv, 3).clone())
    assert torch.allclose(r.render_soft(v, f, const, per_pixel=True), r.render_soft(v, f, colour.expand(1, F, 3)), atol=1e-6)
    # per_pixel=False is the call without the keyword
    assert torch.equal(r.render_soft(v, f, vc, per_pixel=False), r.render_soft(v, f, vc))
    assert torch.equal(r.render_soft(v, f, face, per_pixel=False), flat)
    # cubes are not sampled per pixel; wrong shapes
    with pytest.raises(ValueError):
        r.render_soft(v, f, torch.rand(1, F, 2, 2, 2, 3), per_pixel=True)
    for wrong in (torch.rand(2, F, 4), torch.rand(2, F, 3, 2), torch.rand(2, F + 1, 3, 3), torch.rand(F, 4)):
        with pytest.raises(ValueError):
            r.render_soft(v, f, wrong, per_pixel=True)
    with pytest.raises(ValueError):
        r.render_soft(v, f, nr.VertexColors(torch.rand(Nv + 1, 3)), per_pixel=True)


def test_render_soft_per_pixel_honours_shading_and_lights():
    import neural_renderer_amd as nr
    v, f = _scene()
    r = _renderer()
    F, Nv = f.shape[1], v.shape[1]
    vc = nr.VertexColors(torch.rand(Nv, 3))
    corner, face = torch.rand(1, F, 3, 3), torch.rand(1, F, 3)
    flat = [r.render_soft(v, f, c, per_pixel=True) for c in (vc, corner, face)]
    r.shading = 'smooth'
    smooth = [r.render_soft(v, f, c, per_pixel=True) for c in (vc, corner, face)]
    for a, b in zip(flat, smooth):
        assert b.shape == a.shape and torch.isfinite(b).all() and (a - b).abs().max() > 1e-3
    assert torch.equal(r.render_soft(v, f, face), _renderer().render_soft(v, f, face))   # per_pixel=False ignores shading
    # the lit corner colours are render()'s own
    proj, cc, _ = r._render_vertex_colors(v, f, vc)
    want = nr.soft_render(proj[:, :F], cc.colors[:, :F], 16, 1e-3, 1e-2, r.near, r.far, r.soft_eps, r.background_color)
    assert torch.equal(smooth[0], want)
    # no light, no colour
    dark = _renderer()
    dark.light_intensity_ambient, dark.light_intensity_directional = 0.0, 0.0
    assert dark.render_soft(v, f, vc, per_pixel=True)[:, :3, 8, 8].abs().max() < 1e-6
    # a Lights, flat and smooth
    for shading in ('flat', 'smooth'):
        lit = _renderer()
        lit.shading, lit.lights = shading, nr.Lights()
        for c in (vc, corner, face):
            out = lit.render_soft(v, f, c, per_pixel=True)
            assert out.shape == (2, 4, 16, 16) and torch.isfinite(out).all()
    r.shading = 'phong'
    with pytest.raises(ValueError):
        r.render_soft(v, f, vc, per_pixel=True)


def test_render_soft_per_pixel_gradients_reach_vertices_and_colours():
    import neural_renderer_amd as nr
    v, f = _scene(1)
    v.requires_grad_(True)
    r = _renderer()
    r.shading = 'smooth'
    vcol = torch.rand(v.shape[1], 3, requires_grad=True)
    w = torch.tensor(np.random.default_rng(7).normal(size=(1, 4, 16, 16)), dtype=torch.float32)
    (r.render_soft(v, f, nr.VertexColors(vcol), per_pixel=True) * w).sum().backward()
    assert torch.isfinite(v.grad).all() and v.grad[..., 2].abs().sum() > 0 and vcol.grad.abs().sum() > 0
    corner = torch.rand(1, f.shape[1], 3, 3, requires_grad=True)
    (r.render_soft(v, f, corner, per_pixel=True) * w).sum().backward()
    assert corner.grad.abs().sum() > 0 and tuple(corner.grad.shape) == (1, f.shape[1], 3, 3)
