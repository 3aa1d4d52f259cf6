"""CPU checks of soft colour rendering with UV texture images (soft_render_uv, soft_render_uv_torch,
Renderer.render_soft(per_pixel=True) with a UVImages): soft_render_uv_torch in float64 against the restatement of
tests/soft_uv_ref.py, the restatement's analytic gradient against central differences of itself, a ramp image against the
corner-colour definition, the caps of every case the GPU file runs, the sensitivity of the float32 bounds, argument errors of
the Python function and of the three ABI entries, and the renderer's new errors."""
import ctypes

import numpy as np
import pytest
import torch

import soft_render_ref as R0
import soft_uv_ref as R
import test_soft_uv_gpu as G
from test_soft_render import TWO

BG = (0.2, 0.3, 0.4)


def _torch64(faces, lay, packed, light, S, sigma, gamma, g):
    import neural_renderer_amd as nr
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(packed, dtype=torch.float64, requires_grad=True)
    lt = torch.tensor(light, dtype=torch.float64, requires_grad=True)
    out = nr.soft_render_uv_torch(ft, lay.faces_uv, lay.face_image, lay.base_mean, lay.table, pt, lt, S, sigma, gamma, 0.1,
                                  100.0, 1e-3, BG)
    out.backward(torch.tensor(g))
    return out.detach().numpy(), ft.grad.numpy(), pt.grad.numpy(), lt.grad.numpy()


def _cpu_uv(args, images):
    """A UVImages of CPU tensors (its constructor takes CUDA tensors only): what soft_render_uv's torch path needs."""
    import neural_renderer_amd as nr
    uv = nr.UVImages.__new__(nr.UVImages)
    uv.layout, uv.images = nr.UVLayout(*args), list(images)
    uv.batch = next((int(im.shape[0]) for im in images if im.dim() == 4), None)
    return uv


# ---------------------------------------------------------------------------------------------------------------------
# 1. torch in float64 against the restatement

@pytest.mark.parametrize('S,sigma,gamma', [(16, 1e-3, 1e-1), (20, 1e-3, 1e-4), (16, 1.0, 1e-1), (16, 1e-6, 1e-4)])
def test_torch_float64_equals_the_restatement(S, sigma, gamma):
    """Values to 1e-12, autograd gradients to 1e-9 of the restatement's term magnitudes (analytic)."""
    faces = R.sphere_faces(1, 2)
    F = faces.shape[1]
    rng = np.random.default_rng(2)
    _, lay = G.make_layout(F, 9)
    _, packed = G.make_images(rng, 2)
    light = rng.uniform(0.5, 1.5, (2, F, 3)).astype(np.float32)
    g = rng.normal(size=(2, 4, S, S))
    ref = R.restate(faces, lay, packed, light, S, sigma, gamma, background=BG, g=g)
    out, gf, gp, gl = _torch64(faces, lay, packed, light, S, sigma, gamma, ref.g)
    assert np.abs(out - ref.rgba).max() <= 1e-12
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_light).max() > 0 and np.abs(ref.grad_images).max() > 0
    assert R.worst_ratio(gf, ref.grad_faces, 1e-9 * ref.grad_faces_mag) <= 1
    assert R.worst_ratio(gp, ref.grad_images, 1e-9 * ref.grad_images_mag) <= 1
    assert R.worst_ratio(gl, ref.grad_light, 1e-9 * ref.grad_light_mag) <= 1


def test_shared_images_and_light_in_torch_and_the_public_function():
    """packed [1,P,3] and light [1,F,3] beside B = 3: the expanded call's image, its gradients summed; soft_render_uv on CPU
    tensors is soft_render_uv_torch of the layout's tensors, and its gradients reach every image tensor."""
    import neural_renderer_amd as nr
    faces = R.sphere_faces(1, 3)
    F = faces.shape[1]
    rng = np.random.default_rng(4)
    args, lay = G.make_layout(F, 9)
    images, packed = G.make_images(rng, None)
    light = rng.uniform(0.5, 1.5, (1, F, 3))
    g = rng.normal(size=(3, 4, 16, 16))
    ref = R.restate(faces, lay, packed, light, 16, 1e-3, 1e-2, background=BG, g=g)
    out, gf, gp, gl = _torch64(faces, lay, packed, light, 16, 1e-3, 1e-2, ref.g)
    assert gp.shape == (1, lay.num_pixels, 3) and gl.shape == (1, F, 3)
    for name, got in (('grad_images', gp), ('grad_light', gl)):
        total, mag, _ = R.shared(ref, name)
        assert np.abs(total).max() > 0 and R.worst_ratio(got, total, 1e-9 * mag) <= 1
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    xs = [torch.tensor(im, dtype=torch.float64, requires_grad=True) for im in images]
    lt = torch.tensor(light, requires_grad=True)
    pub = nr.soft_render_uv(ft, _cpu_uv(args, xs), lt, 16, 1e-3, 1e-2, background_color=BG)
    assert np.abs(pub.detach().numpy() - out).max() <= 1e-12
    pub.backward(torch.tensor(ref.g))
    assert [tuple(x.grad.shape) for x in xs] == [im.shape for im in images]
    assert np.abs(G.pack([x.grad.numpy() for x in xs]) - gp).max() <= 1e-12 * max(1.0, np.abs(gp).max())
    assert np.abs(ft.grad.numpy() - gf).max() <= 1e-12 * max(1.0, np.abs(gf).max())
    # light=None is a light of ones
    a = nr.soft_render_uv(ft.detach(), _cpu_uv(args, xs), None, 16, 1e-3, 1e-2)
    b = nr.soft_render_uv(ft.detach(), _cpu_uv(args, xs), torch.ones(1, F, 3, dtype=torch.float64), 16, 1e-3, 1e-2)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 2. central differences of the restatement itself

def _two_case():
    rng = np.random.default_rng(4)
    faces_uv = rng.uniform(0.05, 0.95, (2, 3, 2))
    sizes = [(7, 5), (4, 9)]
    lay = R.Layout(faces_uv, np.array([0, 1]), np.zeros((2, 1, 3)), sizes)
    packed = rng.uniform(0, 1, (1, 35 + 36, 3))
    light = rng.uniform(0.5, 1.5, (1, 2, 3))
    return lay, packed, light


@pytest.mark.parametrize('sigma,gamma', [(3e-2, 5e-2), (1e-1, 1e-2)], ids=['two', 'two-sharp'])
def test_analytic_gradient_against_central_differences(sigma, gamma):
    """S = 8 on the two-triangle case of test_soft_render.py (an inside pair, a free-t pair and a clamped-t pair), away from
    doubt: every face entry (z included), every image entry and every light entry, 1e-6 of the magnitudes."""
    faces, S = TWO, 8
    lay, packed, light = _two_case()
    g = np.random.default_rng(5).normal(size=(1, 4, S, S))
    ref = R.restate(faces, lay, packed, light, S, sigma, gamma, background=BG, g=g)
    assert ref.masked == [0] and ref.doubt == [0] and ref.texel_doubt == [0]
    loss = lambda f, p, l: float((R.restate(f, lay, p, l, S, sigma, gamma, background=BG).rgba * g).sum())
    hstep = 1e-6
    inputs = [faces.astype(np.float64), packed, light]
    for i, (name, x) in enumerate(zip(('grad_faces', 'grad_images', 'grad_light'), inputs)):
        got, mag = getattr(ref, name), getattr(ref, name + '_mag')
        for idx in np.ndindex(x.shape):
            up, dn = x.copy(), x.copy()
            up[idx] += hstep
            dn[idx] -= hstep
            fd = (loss(*(inputs[:i] + [up] + inputs[i + 1:])) - loss(*(inputs[:i] + [dn] + inputs[i + 1:]))) / (2 * hstep)
            assert abs(fd - got[idx]) <= 1e-6 * max(1.0, mag[idx]), (name, idx, fd, got[idx])
    assert np.abs(ref.grad_faces).min() > 0 and np.abs(ref.grad_light).min() > 0 and np.abs(ref.grad_images).max() > 0


def test_the_texture_path_reaches_the_geometry():
    """With E_k cut ('no_uv_geometry') the analytic gradient of the difference case is another one, in every face entry."""
    lay, packed, light = _two_case()
    g = np.random.default_rng(5).normal(size=(1, 4, 8, 8))
    ref = R.restate(TWO, lay, packed, light, 8, 3e-2, 5e-2, background=BG, g=g)
    cut = R.restate(TWO, lay, packed, light, 8, 3e-2, 5e-2, background=BG, g=g, variant='no_uv_geometry')
    assert (np.abs(ref.grad_faces - cut.grad_faces) > 1e-6 * ref.grad_faces_mag).all()
    assert np.array_equal(ref.grad_images, cut.grad_images) and np.array_equal(ref.rgba, cut.rgba)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a ramp image is the corner-colour definition

def test_a_ramp_image_is_the_corner_colour_render():
    """I = a + b col + c row_from_bottom with uv strictly inside (0, 1): rgba, grad_faces and grad_light (the corner gradient
    contracted with ramp(uv_fk)) of soft_render_torch with corner colours L_f ramp(uv_fk), to 1e-12, in float64."""
    import neural_renderer_amd as nr
    faces = R.sphere_faces(1, 2)
    F, S = faces.shape[1], 16
    rng = np.random.default_rng(8)
    sizes = G.SIZES
    face_image = rng.integers(0, len(sizes), F)
    faces_uv = rng.uniform(0.05, 0.95, (F, 3, 2))
    lay = R.Layout(faces_uv, face_image, np.zeros((F, 1, 3)), sizes)
    coef = rng.uniform(0.1, 0.5, (len(sizes), 3, 3))
    images = []
    for (h, w), k in zip(sizes, coef):
        col, row = np.arange(w)[None, :, None], (h - 1 - np.arange(h))[:, None, None]
        images.append(k[None, None, :, 0] + k[None, None, :, 1] * col + k[None, None, :, 2] * row)
    packed = G.pack(images)
    light = rng.uniform(0.5, 1.5, (2, F, 3))
    hw = np.array(sizes, np.float64)[face_image]
    k = coef[face_image]
    ramp = (k[:, None, :, 0] + k[:, None, :, 1] * (faces_uv[:, :, None, 0] * (hw[:, None, None, 1] - 1))
            + k[:, None, :, 2] * (faces_uv[:, :, None, 1] * (hw[:, None, None, 0] - 1)))
    g = rng.normal(size=(2, 4, S, S))
    out, gf, _, gl = _torch64(faces, lay, packed, light, S, 1e-3, 1e-1, g)
    ft = torch.tensor(faces, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(light[:, :, None, :] * ramp[None], requires_grad=True)
    want = nr.soft_render_torch(ft, ct, S, 1e-3, 1e-1, 0.1, 100.0, 1e-3, BG)
    want.backward(torch.tensor(g))
    assert np.abs(out - want.detach().numpy()).max() <= 1e-12
    assert np.abs(gf - ft.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(gf).max())
    wl = (ct.grad.numpy() * ramp[None]).sum(2)
    assert np.abs(gl - wl).max() <= 1e-12 * max(1.0, np.abs(wl).max())
    # ... and the two restatements
    ref_u = R.restate(faces, lay, packed, light, S, 1e-3, 1e-1, background=BG, g=g)
    ref_c = R0.restate(faces, light[:, :, None, :] * ramp[None], S, 1e-3, 1e-1, background=BG, g=g)
    assert np.abs(ref_u.rgba - ref_c.rgba).max() <= 1e-12
    assert np.abs(ref_u.grad_faces - ref_c.grad_faces).max() <= 1e-12 * max(1.0, np.abs(ref_c.grad_faces).max())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the caps, 5. the bounds can tell wrong from right

def test_caps_of_every_gpu_case():
    """Conditions, not measurements: masked pixels <= 1 % of the pixels with a taken pair, segment doubt <= 2 % and texel
    doubt <= 1 % of the taken pairs, in every case and image of the GPU file."""
    import test_soft_render_gpu as G0
    assert all(c in G0.CASES for c in G.CASES)
    assert sum(c[0] == 'mix' for c in G.CASES) == sum(c[0] == 'mix' for c in G0.CASES)
    assert {c[3] for c in G.CASES if c[0] == 'ico1'} == {c[3] for c in G0.CASES if c[0] == 'ico1'}
    for case in G.CASES:
        ref = G.reference(*case)[4]
        assert ref.masked_share <= 0.01, (case, ref.masked, ref.with_pair)
        assert ref.doubt_share <= 0.02, (case, ref.doubt, ref.pairs)
        assert ref.texel_doubt_share <= 0.01, (case, ref.texel_doubt, ref.pairs)
        assert sum(ref.pairs) > 0


@pytest.mark.parametrize('variant,what', [('no_uv_geometry', ('grad_faces',)), ('no_mirror', ('rgba', 'grad_images')),
                                          ('unweighted_light', ('grad_light',))])
def test_bounds_are_not_vacuous(variant, what):
    """The first sphere case of the GPU file: the restatement with one defect misses its own bounds."""
    case = [c for c in G.CASES if c[0] == 'ico1'][0]
    faces, args, images, light, ref = G.reference(*case)
    S, sigma, gamma = case[2:]
    bad = R.restate(faces, R.Layout(*args), G.pack(images), light, S, sigma, gamma, background=G.BG, g=ref.g, variant=variant)
    for name in what:
        if name == 'rgba':
            ratio = R.masked_ratio(bad.rgba, ref.rgba, ref.rgba_bound, ref.mask)
        else:
            ratio = R.worst_ratio(getattr(bad, name), getattr(ref, name), getattr(ref, name + '_bound'))
        assert ratio > 1, (name, ratio)
    with pytest.raises(ValueError):
        R.restate(faces, R.Layout(*args), G.pack(images), light, S, sigma, gamma, variant='affine')


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument errors

def test_argument_errors_of_the_python_function():
    import neural_renderer_amd as nr
    F = 5
    args, _ = G.make_layout(F, 1)
    images = [torch.rand(h, w, 3) for h, w in G.SIZES]
    uv = _cpu_uv(args, images)
    f, l = torch.rand(2, F, 3, 3) + 1, torch.rand(2, F, 3)
    ok = dict(image_size=8, sigma=1e-3, gamma=1e-2)
    assert nr.soft_render_uv(f, uv, l, **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render_uv(f, uv, l[:1], **ok).shape == (2, 4, 8, 8)
    assert nr.soft_render_uv(f, uv, **ok).shape == (2, 4, 8, 8)
    batched = _cpu_uv(args, [torch.rand(3, h, w, 3) for h, w in G.SIZES])
    bad = [((f[0], uv, l), {}), ((f, images, l), {}), ((f, None, l), {}),
           ((torch.rand(2, F + 1, 3, 3) + 1, uv, None), {}),                                  # the layout's face count
           ((f, batched, l), {}),                                                              # the image batch
           ((f, uv, l[:, :4]), {}), ((f, uv, l[..., :2]), {}), ((f, uv, torch.rand(3, F, 3)), {}), ((f, uv, l[0]), {}),
           ((f, uv, torch.rand(2, F, 3, 3)), {}), ((f, uv, l.long()), {}), ((f.long(), uv, l), {}),
           ((f, uv, l), dict(image_size=0)), ((f, uv, l), dict(sigma=0)), ((f, uv, l), dict(gamma=float('inf'))),
           ((f, uv, l), dict(near=1, far=1)), ((f, uv, l), dict(eps=float('nan'))), ((f, uv, l), dict(background_color=(0, 0))),
           ((f, uv, l), dict(implementation='cuda')), ((f, uv, l), dict(implementation='hip'))]
    for a, kw in bad:
        with pytest.raises(ValueError):
            nr.soft_render_uv(*a, **dict(ok, **kw))
    assert nr.soft_render_uv(torch.rand(3, F, 3, 3) + 1, batched, **ok).shape == (3, 4, 8, 8)


def test_argument_errors_of_the_abi_need_no_gpu():
    """NR_E_* before any launch (the pattern of tests/test_soft_corners.py): fake non-NULL pointers never reach a kernel."""
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    P = 78

    def uvs(ptrs=(1, 1, 1, 1, 1), ts=2, M=4, pixels=P, batch=1):
        return _lib.UVImagesStruct(*ptrs, ts, M, pixels, batch)
    # a 112-byte record and twelve bytes of light gradient per (image, face), then 24 bytes per image pixel
    assert lib.nr_soft_uv_workspace_bytes(uvs(), 3, 80, 32) >= 3 * 80 * (112 + 12) + P * 24
    assert lib.nr_soft_uv_workspace_bytes(uvs(batch=3), 3, 80, 32) >= 3 * 80 * (112 + 12) + 3 * P * 24
    assert lib.nr_soft_uv_workspace_bytes(uvs(), 3, 80, 32) > lib.nr_soft_corners_workspace_bytes(3, 80, 32)
    assert lib.nr_soft_uv_workspace_bytes(None, 3, 80, 32) == 0 and lib.nr_soft_uv_workspace_bytes(uvs(batch=2), 3, 80, 32) == 0
    assert lib.nr_soft_uv_workspace_bytes(uvs(), 0, 80, 32) == 0 and lib.nr_soft_uv_workspace_bytes(uvs(), 1, 80, 20000) == 0
    assert lib.nr_soft_uv_workspace_bytes(uvs(), 1, 2 ** 24 + 1, 8) == 0 and lib.nr_soft_uv_workspace_bytes(uvs(pixels=0), 1, 8, 8) == 0
    num = dict(sigma=1e-3, gamma=1e-2, near=0.1, far=100.0, eps=1e-3, r=0.0, g=0.0, b=0.0)

    def fwd(uv=None, ptrs=(1, 1, 1, 1, 1), sizes=(1, 4, 8, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_uv_forward(uv or uvs(), *ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'],
                                      n['g'], n['b'], ws[0], ws[1], None)

    def bwd(uv=None, ptrs=(1,) * 9, sizes=(1, 4, 8, 1), ws=(1, 1 << 20), **kw):
        n = dict(num, **kw)
        return lib.nr_soft_uv_backward(uv or uvs(), *ptrs, *sizes, n['sigma'], n['gamma'], n['near'], n['far'], n['eps'], n['r'],
                                       n['g'], n['b'], ws[0], ws[1], None)
    nan, inf = float('nan'), float('inf')
    for call, count in ((fwd, 5), (bwd, 9)):
        for i in range(count):
            if call is bwd and i == 8:   # grad_images may be NULL: not computed
                continue
            assert call(ptrs=tuple(None if j == i else 1 for j in range(count))) == -1, i
        assert lib.nr_soft_uv_forward(None, 1, 1, 1, 1, 1, 1, 4, 8, 1, 1e-3, 1e-2, 0.1, 100.0, 1e-3, 0.0, 0.0, 0.0, 1, 1 << 20, None) == -1
        for i in range(5):
            assert call(uv=uvs(ptrs=tuple(None if j == i else 1 for j in range(5)))) == -1, i
        for sizes in ((0, 4, 8, 1), (1, 0, 8, 1), (1, 4, 0, 1), (70000, 4, 8, 1), (1, 4, 20000, 1), (1, 2 ** 24 + 1, 8, 1)):
            assert call(sizes=sizes) == -2, sizes
        for uv in (uvs(ts=1), uvs(ts=1025), uvs(M=0), uvs(pixels=0), uvs(batch=2), uvs(batch=0)):
            assert call(uv=uv) == -2
        for kw in (dict(sigma=0.0), dict(sigma=1e31), dict(sigma=nan), dict(gamma=0.0), dict(gamma=1e-31), dict(gamma=nan),
                   dict(near=1.0, far=1.0), dict(near=2.0, far=1.0), dict(near=nan), dict(far=inf), dict(eps=nan), dict(eps=inf),
                   dict(r=nan), dict(g=inf), dict(b=-inf)):
            assert call(**kw) == -4, kw
        assert call(sizes=(1, 4, 8, 2)) == -4
        assert call(ws=(None, 1 << 20)) == -3 and call(ws=(1, 16)) == -3
        # the corner entry's workspace is too small, and so is one byte less than asked
        assert call(ws=(1, lib.nr_soft_corners_workspace_bytes(1, 4, 8))) == -3
        assert call(ws=(1, lib.nr_soft_uv_workspace_bytes(uvs(), 1, 4, 8) - 1)) == -3
    assert isinstance(ctypes.sizeof(_lib.UVImagesStruct), int)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the renderer

def test_render_soft_with_uv_images_on_cpu_tensors_and_its_errors():
    import neural_renderer_amd as nr
    v, f = nr.icosphere(1, 0.8)
    v, f = v[None].repeat(2, 1, 1), f[None].repeat(2, 1, 1)
    F = f.shape[1]
    args, _ = G.make_layout(F, 3)
    uv = _cpu_uv(args, [torch.rand(h, w, 3) for h, w in G.SIZES])
    r = nr.Renderer()
    r.image_size, r.eye = 16, nr.get_points_from_angles(2.732, 20, 30)
    r.soft_sigma, r.soft_gamma = 1e-3, 1e-2
    img = r.render_soft(v, f, uv, per_pixel=True)
    assert img.shape == (2, 4, 16, 16) and torch.isfinite(img).all() and img[:, :3].abs().sum() > 0
    lit = nr.Renderer()
    lit.image_size, lit.eye, lit.soft_sigma, lit.soft_gamma, lit.lights = 16, r.eye, 1e-3, 1e-2, nr.Lights()
    assert lit.render_soft(v, f, uv, per_pixel=True).shape == (2, 4, 16, 16)
    with pytest.raises(ValueError, match='per_pixel=True'):
        r.render_soft(v, f, uv)
    with pytest.raises(ValueError, match='per_pixel=True'):
        r.render_soft(v, f, uv, per_pixel=False)
    r.shading = 'smooth'
    with pytest.raises(ValueError, match='light per corner is not done for UV images in the soft renderer'):
        r.render_soft(v, f, uv, per_pixel=True)
    r.shading = 'phong'
    with pytest.raises(ValueError):
        r.render_soft(v, f, uv, per_pixel=True)
    r.shading = 'flat'
    with pytest.raises(ValueError):                                       # cubes are still not sampled per pixel
        r.render_soft(v, f, torch.rand(1, F, 2, 2, 2, 3), per_pixel=True)
    with pytest.raises(ValueError):                                       # a layout of another mesh
        r.render_soft(v[:, :, :], f[:, :F - 1], uv, per_pixel=True)
