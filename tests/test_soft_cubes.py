"""CPU checks of soft colour rendering with texture cubes sampled at the pixel (soft_render_cubes, soft_render_cubes_torch,
TextureCubes, Renderer.render_soft(per_pixel=True) with a TextureCubes): the three gradient identities of the definition --
soft_render_cubes_torch's autograd in float64 against the analytic gradient of tests/soft_cubes_ref.py --, the restatement
against central differences of itself, an affine cube against the corner-colour definition, a constant cube against the flat
one, the caps of every case the GPU file runs (the tap-doubt share against its derived size), the sensitivity of the float32
bounds, argument errors of the Python function and of the three ABI entries, and the renderer."""
import numpy as np
import pytest
import torch

import soft_cubes_ref as R
import soft_render_ref as R0
import test_soft_cubes_gpu as G
from test_soft_render import TWO

BG = (0.2, 0.3, 0.4)


def _torch64(faces, textures, light, S, sigma, gamma, g, texture_eps=1e-3):
    import neural_renderer_amd as nr
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(textures, dtype=torch.float64, requires_grad=True)
    lt = torch.tensor(light, dtype=torch.float64, requires_grad=True)
    out = nr.soft_render_cubes_torch(ft, tt, lt, S, sigma, gamma, 0.1, 100.0, 1e-3, BG, texture_eps)
    out.backward(torch.tensor(g))
    return out.detach().numpy(), ft.grad.numpy(), tt.grad.numpy(), lt.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gradient identities: autograd in float64 against the analytic restatement

@pytest.mark.parametrize('S,sigma,gamma,ts', [(16, 1e-3, 1e-1, 2), (20, 1e-3, 1e-4, 4), (16, 1.0, 1e-1, 5), (16, 1e-6, 1e-4, 3)])
def test_torch_float64_equals_the_restatement(S, sigma, gamma, ts):
    """dL/dtex += W g L w_pn, dL/dL += W g T, and E_k = W zp (G_k - sum mu_j G_j) in the corner colours' place: values to
    1e-12, autograd gradients to 1e-9 of the restatement's term magnitudes."""
    faces = R.sphere_faces(1, 2)
    F = faces.shape[1]
    rng = np.random.default_rng(2 + ts)
    textures = rng.uniform(0, 1, (2, F, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.5, 1.5, (2, F, 3)).astype(np.float32)
    g = rng.normal(size=(2, 4, S, S))
    ref = R.restate(faces, textures, light, S, sigma, gamma, background=BG, g=g)
    out, gf, gt, gl = _torch64(faces, textures, light, S, sigma, gamma, ref.g)
    assert np.abs(out - ref.rgba).max() <= 1e-12
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_light).max() > 0 and np.abs(ref.grad_textures).max() > 0
    assert R.worst_ratio(gf, ref.grad_faces, 1e-9 * ref.grad_faces_mag) <= 1
    assert R.worst_ratio(gt, ref.grad_textures, 1e-9 * ref.grad_textures_mag) <= 1
    assert R.worst_ratio(gl, ref.grad_light, 1e-9 * ref.grad_light_mag) <= 1


def test_shared_cubes_and_light_in_torch_and_the_public_function():
    """Cubes [1,F,...] and light [1,F,3] beside B = 3: the expanded call's image, its gradients summed; soft_render_cubes on
    CPU tensors is soft_render_cubes_torch, a TextureCubes is its tensor, light=None is a light of ones."""
    import neural_renderer_amd as nr
    faces = R.sphere_faces(1, 3)
    F = faces.shape[1]
    rng = np.random.default_rng(4)
    textures = rng.uniform(0, 1, (1, F, 3, 3, 3, 3))
    light = rng.uniform(0.5, 1.5, (1, F, 3))
    g = rng.normal(size=(3, 4, 16, 16))
    ref = R.restate(faces, textures, light, 16, 1e-3, 1e-2, background=BG, g=g)
    out, gf, gt, gl = _torch64(faces, textures, light, 16, 1e-3, 1e-2, ref.g)
    assert gt.shape == textures.shape and gl.shape == (1, F, 3)
    for name, got in (('grad_textures', gt), ('grad_light', gl)):
        total, mag, _ = R.shared(ref, name)
        assert np.abs(total).max() > 0 and R.worst_ratio(got, total, 1e-9 * mag) <= 1
    ft = torch.tensor(faces, dtype=torch.float64)
    tt, lt = torch.tensor(textures), torch.tensor(light)
    pub = nr.soft_render_cubes(ft, tt, lt, 16, 1e-3, 1e-2, background_color=BG)
    assert np.abs(pub.numpy() - out).max() <= 1e-12
    assert torch.equal(pub, nr.soft_render_cubes(ft, nr.TextureCubes(tt), lt, 16, 1e-3, 1e-2, background_color=BG))
    a = nr.soft_render_cubes(ft, tt, None, 16, 1e-3, 1e-2)
    assert torch.equal(a, nr.soft_render_cubes(ft, tt, torch.ones(1, F, 3, dtype=torch.float64), 16, 1e-3, 1e-2))


# ---------------------------------------------------------------------------------------------------------------------
# 2. central differences of the restatement itself

@pytest.mark.parametrize('sigma,gamma', [(3e-2, 5e-2), (1e-1, 1e-2)], ids=['two', 'two-sharp'])
def test_analytic_gradient_against_central_differences(sigma, gamma):
    """S = 8 on the two-triangle case of test_soft_render.py (an inside pair, a free-t pair and a clamped-t pair), away from
    doubt: every face entry (z included), every texel and every light entry, 1e-6 of the magnitudes."""
    faces, S, ts = TWO, 8, 3
    rng = np.random.default_rng(4)
    textures, light = rng.uniform(0, 1, (1, 2, ts, ts, ts, 3)), rng.uniform(0.5, 1.5, (1, 2, 3))
    g = np.random.default_rng(5).normal(size=(1, 4, S, S))
    ref = R.restate(faces, textures, light, S, sigma, gamma, background=BG, g=g)
    assert ref.masked == [0] and ref.doubt == [0] and ref.tap_doubt == [0]
    loss = lambda f, t, l: float((R.restate(f, t, l, S, sigma, gamma, background=BG).rgba * g).sum())
    hstep = 1e-6
    inputs = [faces.astype(np.float64), textures, light]
    for i, (name, x) in enumerate(zip(('grad_faces', 'grad_textures', 'grad_light'), inputs)):
        got, mag = getattr(ref, name), getattr(ref, name + '_mag')
        for idx in np.ndindex(x.shape):
            up, dn = x.copy(), x.copy()
            up[idx] += hstep
            dn[idx] -= hstep
            fd = (loss(*(inputs[:i] + [up] + inputs[i + 1:])) - loss(*(inputs[:i] + [dn] + inputs[i + 1:]))) / (2 * hstep)
            assert abs(fd - got[idx]) <= 1e-6 * max(1.0, mag[idx]), (name, idx, fd, got[idx])
    assert np.abs(ref.grad_faces).min() > 0 and np.abs(ref.grad_light).min() > 0 and np.abs(ref.grad_textures).max() > 0


def test_the_texture_path_reaches_the_geometry():
    """With E_k cut ('no_texture_geometry') the analytic gradient of the difference case is another one, in every face entry."""
    rng = np.random.default_rng(4)
    textures, light = rng.uniform(0, 1, (1, 2, 3, 3, 3, 3)), rng.uniform(0.5, 1.5, (1, 2, 3))
    g = np.random.default_rng(5).normal(size=(1, 4, 8, 8))
    ref = R.restate(TWO, textures, light, 8, 3e-2, 5e-2, background=BG, g=g)
    cut = R.restate(TWO, textures, light, 8, 3e-2, 5e-2, background=BG, g=g, variant='no_texture_geometry')
    assert (np.abs(ref.grad_faces - cut.grad_faces) > 1e-6 * ref.grad_faces_mag).all()
    assert np.array_equal(ref.grad_textures, cut.grad_textures) and np.array_equal(ref.rgba, cut.rgba)


# ---------------------------------------------------------------------------------------------------------------------
# 3. an affine cube is the corner-colour definition, a constant cube the flat one

@pytest.mark.parametrize('ts', [2, 5])
def test_an_affine_cube_is_the_corner_colour_render(ts):
    """tex[i,j,k] = a + b . (i, j, k), texture_eps = 0: rgba, grad_faces and grad_light (the corner gradient contracted with
    the unlit corner colours a + (ts - 1) b_k) of soft_render_torch with corner colours, to 1e-12, in float64."""
    import neural_renderer_amd as nr
    faces = R.sphere_faces(1, 2)
    F, S = faces.shape[1], 16
    rng = np.random.default_rng(8)
    cube, unlit = G.affine_cube(rng, F, ts)
    textures = cube[None]
    light = rng.uniform(0.5, 1.5, (2, F, 3))
    g = rng.normal(size=(2, 4, S, S))
    out, gf, _, gl = _torch64(faces, textures, light, S, 1e-3, 1e-1, g, texture_eps=0.0)
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(light[:, :, None, :] * unlit[None], requires_grad=True)
    want = nr.soft_render_torch(ft, ct, S, 1e-3, 1e-1, 0.1, 100.0, 1e-3, BG)
    want.backward(torch.tensor(g))
    assert np.abs(out - want.detach().numpy()).max() <= 1e-12
    assert np.abs(gf - ft.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(gf).max())
    wl = (ct.grad.numpy() * unlit[None]).sum(2)
    assert np.abs(gl - wl).max() <= 1e-12 * max(1.0, np.abs(wl).max())
    # ... and the two restatements
    ref_t = R.restate(faces, textures, light, S, 1e-3, 1e-1, background=BG, texture_eps=0.0, g=g)
    ref_c = R0.restate(faces, light[:, :, None, :] * unlit[None], S, 1e-3, 1e-1, background=BG, g=g)
    assert np.abs(ref_t.rgba - ref_c.rgba).max() <= 1e-12
    assert np.abs(ref_t.grad_faces - ref_c.grad_faces).max() <= 1e-12 * max(1.0, np.abs(ref_c.grad_faces).max())


def test_a_constant_cube_is_the_flat_render():
    """Every texel of a face the same colour: soft_render_torch with the colours L_f c_f, to 1e-12 in float64; the cube's
    gradient summed over its texels is the flat colour gradient times the light."""
    import neural_renderer_amd as nr
    faces = R.sphere_faces(1, 2)
    F, S, ts = faces.shape[1], 16, 4
    rng = np.random.default_rng(9)
    col, light = rng.uniform(0, 1, (2, F, 3)), rng.uniform(0.5, 1.5, (2, F, 3))
    textures = np.ascontiguousarray(np.broadcast_to(col[:, :, None, None, None, :], (2, F, ts, ts, ts, 3)))
    g = rng.normal(size=(2, 4, S, S))
    out, gf, gt, gl = _torch64(faces, textures, light, S, 1e-3, 1e-1, g)
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(light * col, requires_grad=True)
    want = nr.soft_render_torch(ft, ct, S, 1e-3, 1e-1, 0.1, 100.0, 1e-3, BG)
    want.backward(torch.tensor(g))
    assert np.abs(out - want.detach().numpy()).max() <= 1e-12
    assert np.abs(gf - ft.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(gf).max())
    assert np.abs(gl - ct.grad.numpy() * col).max() <= 1e-12 * max(1.0, np.abs(gl).max())
    assert np.abs(gt.sum((2, 3, 4)) - ct.grad.numpy() * light).max() <= 1e-12 * max(1.0, np.abs(gt).max())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the caps, 5. the bounds can tell wrong from right

def test_caps_of_every_gpu_case():
    """Conditions, not measurements: masked pixels <= 1 % of the pixels with a taken pair, segment doubt <= 2 % and tap doubt
    <= 1 % of the taken pairs, in every case and image of the GPU file.  The tap-doubt share is derived: 3 (ts - 2) interior
    integers, each with a band of twice a bound of a few u (ts - 1) around it, on positions spread over [0, ts - 1]: about
    6 (ts - 2) times that bound, of the order of 1e-4.  Found: no pair or one pair per image with ts <= 5 (at most 1 of 10 298, 1e-4),
    and 1.5e-4 (3 pairs of 20 480 in an image) at ts = 8, sigma = 1, where every face reaches every pixel and the bound of v
    is largest -- so the order of magnitude is what is asserted beside the cap: 1e-3."""
    import test_soft_render_gpu as G0
    assert all(c[:5] in G0.CASES for c in G.CASES)
    assert {c[5] for c in G.CASES} == {2, 4, 5, 8} and sum(c[5] == 8 for c in G.CASES) == 1
    assert {c[:5] for c in G.CASES if c[0] == 'mix'} == {c for c in G0.CASES if c[0] == 'mix' and c[1] == 2}
    for case in G.CASES:
        ref = G.reference(*case)[3]
        assert ref.masked_share <= 0.01, (case, ref.masked, ref.with_pair)
        assert ref.doubt_share <= 0.02, (case, ref.doubt, ref.pairs)
        assert ref.tap_doubt_share <= 0.01, (case, ref.tap_doubt, ref.pairs)
        assert ref.tap_doubt_share <= 1e-3, (case, ref.tap_doubt, ref.pairs)
        assert sum(ref.pairs) > 0
        if case[5] == 2:   # no interior integer
            assert ref.tap_doubt == [0] * case[1]


@pytest.mark.parametrize('variant,what', [('affine', ('rgba', 'grad_textures')), ('no_texture_geometry', ('grad_faces',)),
                                          ('transposed', ('rgba', 'grad_textures')), ('unweighted_light', ('grad_light',))])
def test_bounds_are_not_vacuous(variant, what):
    """The first sphere case of the GPU file: the restatement with one defect misses its own bounds."""
    case = [c for c in G.CASES if c[0] == 'ico1'][0]
    faces, textures, light, ref = G.reference(*case)
    S, sigma, gamma = case[2:5]
    bad = R.restate(faces, textures, light, S, sigma, gamma, background=G.BG, g=ref.g, variant=variant)
    for name in what:
        if name == 'rgba':
            ratio = R.masked_ratio(bad.rgba, ref.rgba, ref.rgba_bound, ref.mask)
        else:
            ratio = R.worst_ratio(getattr(bad, name), getattr(ref, name), getattr(ref, name + '_bound'))
        assert ratio > 1, (name, ratio)
    with pytest.raises(ValueError):
        R.restate(faces, textures, light, S, sigma, gamma, variant='no_mirror')


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument errors

def test_argument_errors_of_the_python_function():
    import neural_renderer_amd as nr
    F = 5
    f, t, l = torch.rand(2, F, 3, 3) + 1, torch.rand(2, F, 2, 2, 2, 3), torch.rand(2, F, 3)
    ok = dict(image_size=8, sigma=1e-3, gamma=1e-2)
    assert nr.soft_render_cubes(f, t, l, **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render_cubes(f, t[:1], l[:1], **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render_cubes(f, t, **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render_cubes(f, torch.rand(2, F, 9, 9, 9, 3), l, **ok).shape == (2, 4, 8, 8)      # beyond the HIP range: torch
    assert nr.soft_render_cubes(f, t, l, texture_eps=0, **ok).shape == (2, 4, 8, 8)
    bad = [((f[0], t, l), {}), ((f, None, l), {}), ((f, t[0], l), {}),
           ((f, torch.rand(2, F, 1, 1, 1, 3), l), {}),                                                # ts = 1
           ((f, torch.rand(2, F, 2, 2, 3, 3), l), {}), ((f, torch.rand(2, F, 2, 2, 2, 4), l), {}),
           ((f, torch.rand(2, F + 1, 2, 2, 2, 3), l), {}), ((f, torch.rand(2, 2 * F, 2, 2, 2, 3), l), {}),   # a wrong F (fill_back copies)
           ((f, torch.rand(3, F, 2, 2, 2, 3), l), {}), ((f, t.long(), l), {}),
           ((f, t, l[:, :4]), {}), ((f, t, l[..., :2]), {}), ((f, t, torch.rand(3, F, 3)), {}), ((f, t, l[0]), {}),
           ((f, t, l.long()), {}), ((f.long(), t, l), {}),
           ((f, t, l), dict(texture_eps=1.0)), ((f, t, l), dict(texture_eps=-1e-9)), ((f, t, l), dict(texture_eps=float('nan'))),
           ((f, t, l), dict(texture_eps=float('inf'))), ((f, t, l), dict(texture_eps='1e-3')),
           ((f, t, l), dict(image_size=0)), ((f, t, l), dict(sigma=0)), ((f, t, l), dict(gamma=float('inf'))),
           ((f, t, l), dict(near=1, far=1)), ((f, t, l), dict(eps=float('nan'))), ((f, t, l), dict(background_color=(0, 0))),
           ((f, t, l), dict(implementation='cuda')), ((f, t, l), dict(implementation='hip'))]
    for a, kw in bad:
        with pytest.raises(ValueError):
            nr.soft_render_cubes(*a, **dict(ok, **kw))
    for x in (torch.rand(F, 2, 2, 2, 3), torch.rand(1, F, 1, 1, 1, 3), torch.rand(1, F, 2, 2, 2, 3).long(), None, [1.0]):
        with pytest.raises(ValueError):
            nr.TextureCubes(x)
    assert nr.TextureCubes(t).texture_size == 2 and nr.TextureCubes(t).textures is t


def test_argument_errors_of_the_abi_need_no_gpu():
    """NR_E_* before any launch (the pattern of tests/test_soft_corners.py): fake non-NULL pointers never reach a kernel."""
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    # an 80-byte record and twelve bytes of light gradient per (image, face); shared cubes: a cube gradient per image
    assert lib.nr_soft_cubes_workspace_bytes(3, 80, 32, 4, 1) >= 3 * 80 * (80 + 12)
    assert lib.nr_soft_cubes_workspace_bytes(3, 80, 32, 4, 0) >= 3 * 80 * (80 + 12 + 64 * 12)
    assert lib.nr_soft_cubes_workspace_bytes(3, 80, 32, 4, 1) < lib.nr_soft_corners_workspace_bytes(3, 80, 32)
    for args in ((0, 80, 32, 4, 1), (1, 80, 20000, 4, 1), (1, 2 ** 24 + 1, 8, 4, 1), (1, 80, 32, 1, 1), (1, 80, 32, 9, 1),
                 (1, 80, 32, 4, 2), (1, 2 ** 22, 8, 8, 1)):
        assert lib.nr_soft_cubes_workspace_bytes(*args) == 0, args
    num = dict(sigma=1e-3, gamma=1e-2, near=0.1, far=100.0, eps=1e-3, r=0.0, g=0.0, b=0.0, teps=1e-3)

    def fwd(ptrs=(1,) * 6, sizes=(1, 4, 8, 2, 1, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_cubes_forward(*ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'], n['g'],
                                         n['b'], n['teps'], ws[0], ws[1], None)

    def bwd(ptrs=(1,) * 10, sizes=(1, 4, 8, 2, 1, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_cubes_backward(*ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'], n['g'],
                                          n['b'], n['teps'], ws[0], ws[1], None)
    nan, inf = float('nan'), float('inf')
    for call, count in ((fwd, 6), (bwd, 10)):
        for i in range(count):
            if call is bwd and i == 9:   # grad_textures may be NULL: not computed
                continue
            assert call(ptrs=tuple(None if j == i else 1 for j in range(count))) == -1, i
        for sizes in ((0, 4, 8, 2, 1, 1), (1, 0, 8, 2, 1, 1), (1, 4, 0, 2, 1, 1), (70000, 4, 8, 2, 1, 1), (1, 4, 20000, 2, 1, 1),
                      (1, 2 ** 24 + 1, 8, 2, 1, 1), (1, 4, 8, 1, 1, 1), (1, 4, 8, 0, 1, 1), (1, 4, 8, 9, 1, 1), (1, 4, 8, -3, 1, 1)):
            assert call(sizes=sizes) == -2, sizes
        for kw in (dict(sigma=0.0), dict(sigma=1e31), dict(sigma=nan), dict(gamma=0.0), dict(gamma=1e-31), dict(gamma=nan),
                   dict(near=1.0, far=1.0), dict(near=2.0, far=1.0), dict(near=nan), dict(far=inf), dict(eps=nan), dict(eps=inf),
                   dict(r=nan), dict(g=inf), dict(b=-inf), dict(teps=1.0), dict(teps=-1e-9), dict(teps=nan), dict(teps=inf)):
            assert call(**kw) == -4, kw
        assert call(teps=0.0, ws=(1, 16)) == -3                                    # texture_eps = 0 is in range
        assert call(sizes=(1, 4, 8, 2, 2, 1)) == -4 and call(sizes=(1, 4, 8, 2, 1, 2)) == -4
        # the order: a size before a number, a number before the workspace
        assert call(sizes=(1, 4, 8, 9, 1, 1), teps=2.0, ws=(None, 0)) == -2 and call(teps=2.0, ws=(None, 0)) == -4
        assert call(ws=(None, 1 << 20)) == -3 and call(ws=(1, 16)) == -3
        assert call(ws=(1, lib.nr_soft_cubes_workspace_bytes(1, 4, 8, 2, 1) - 1)) == -3
        assert call(sizes=(3, 4, 8, 2, 0, 1), ws=(1, lib.nr_soft_cubes_workspace_bytes(3, 4, 8, 2, 1))) == -3   # shared cubes need more


# ---------------------------------------------------------------------------------------------------------------------
# 7. the renderer

def test_render_soft_with_texture_cubes_on_cpu_tensors_and_its_errors():
    """render_soft with a TextureCubes equals soft_render_cubes_torch of the composition: the front copies of the front-end's
    faces, the per-face light of the front copies, texture_eps = rasterizer_eps; with and without `lights`; its errors; a
    bare tensor of cubes keeps both of its behaviours."""
    import neural_renderer_amd as nr
    v, f = nr.icosphere(1, 0.8)
    v, f = v[None].repeat(2, 1, 1), f[None].repeat(2, 1, 1)
    F = f.shape[1]
    cubes = torch.rand(1, F, 3, 3, 3, 3)
    r = nr.Renderer()
    r.image_size, r.eye = 16, nr.get_points_from_angles(2.732, 20, 30)
    r.soft_sigma, r.soft_gamma, r.rasterizer_eps = 1e-3, 1e-2, 2e-3
    img = r.render_soft(v, f, nr.TextureCubes(cubes), per_pixel=True)
    assert img.shape == (2, 4, 16, 16) and torch.isfinite(img).all() and img[:, :3].abs().sum() > 0
    proj, light = r._frontend(v, f, light_colors=True)
    want = nr.soft_render_cubes_torch(proj[:, :F], cubes, light[:, :F], 16, 1e-3, 1e-2, r.near, r.far, r.soft_eps,
                                      r.background_color, 2e-3)
    assert torch.equal(img, want)
    assert not torch.equal(img, nr.soft_render_cubes_torch(proj[:, :F], cubes, light[:, :F], 16, 1e-3, 1e-2, r.near, r.far,
                                                           r.soft_eps, r.background_color, 0.5))
    lit = nr.Renderer()
    lit.image_size, lit.eye, lit.soft_sigma, lit.soft_gamma, lit.lights = 16, r.eye, 1e-3, 1e-2, nr.Lights()
    img2 = lit.render_soft(v, f, nr.TextureCubes(cubes), per_pixel=True)
    light2 = nr.light_colors(v, f, lit.lights, fill_back=lit.fill_back, smooth=False)
    want2 = nr.soft_render_cubes_torch(lit._frontend(v, f)[0][:, :F], cubes, light2[:, :F], 16, 1e-3, 1e-2, lit.near, lit.far,
                                       lit.soft_eps, lit.background_color, lit.rasterizer_eps)
    assert torch.equal(img2, want2)
    # gradients reach the vertices and the cubes
    vg, cg = v.clone().requires_grad_(True), cubes.clone().requires_grad_(True)
    r.render_soft(vg, f, nr.TextureCubes(cg), per_pixel=True).sum().backward()
    assert vg.grad.abs().sum() > 0 and cg.grad.abs().sum() > 0
    with pytest.raises(ValueError, match='per_pixel=True'):
        r.render_soft(v, f, nr.TextureCubes(cubes))
    with pytest.raises(ValueError, match='per_pixel=True'):
        r.render_soft(v, f, nr.TextureCubes(cubes), per_pixel=False)
    with pytest.raises(ValueError):                                       # fill_back copies are not taken
        r.render_soft(v, f, nr.TextureCubes(torch.rand(1, 2 * F, 3, 3, 3, 3)), per_pixel=True)
    r.shading = 'smooth'
    with pytest.raises(ValueError, match='light per corner is not done for texture cubes in the soft renderer'):
        r.render_soft(v, f, nr.TextureCubes(cubes), per_pixel=True)
    r.shading = 'phong'
    with pytest.raises(ValueError):
        r.render_soft(v, f, nr.TextureCubes(cubes), per_pixel=True)
    r.shading = 'flat'
    with pytest.raises(ValueError):                                       # a bare tensor: not sampled per pixel
        r.render_soft(v, f, cubes, per_pixel=True)
    assert r.render_soft(v, f, cubes).shape == (2, 4, 16, 16)             # ... and the mean of each cube without it
