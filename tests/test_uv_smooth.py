"""Smooth light on per-pixel UV images without a GPU: vertex_light against vertex_shade_torch, the NumPy restatement
(uv_smooth_ref) against finite differences and against the flat restatement, the entry points' argument checks
(include/nr_hip.h nr_forward_rasterize_uv_smooth / nr_backward_uv_images_smooth) and the Python-side shape checks.  The maps
the restatement starts from come from the CPU oracle's rasterizer."""
import types

import numpy as np
import pytest

import helpers as H
import uv_pixel_ref as P
import uv_smooth_ref as R
import vertex_ref as V

from neural_renderer_amd import _build, _lib

EPS = 1e-3
BG = (0.1, 0.2, 0.3)


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def _oracle_maps(sc):
    from oracle import oracle as O
    O.build()
    fn = O.Rasterize(sc['S'], 0.1, 100, EPS, BG, return_alpha=True, return_depth=True)
    fn(sc['faces'])
    return fn.face_index_map, fn.weight_map, fn.depth_map


def _layout(sc):
    import neural_renderer_amd as nr
    return nr.UVLayout(sc['uv'], sc['face_image'], sc['base'], sc['sizes'])


@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('fill_back', [False, True])
def test_vertex_light_is_vertex_shade_of_a_white_mesh(fill_back, smooth):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd.vertex_colors import vertex_shade_torch
    rng = np.random.default_rng(11)
    v, f = V.icosphere(1)
    v = torch.tensor((v[None] + rng.normal(scale=0.05, size=(2,) + v.shape)).astype(np.float32), requires_grad=True)
    f = torch.tensor(f)
    kw = dict(intensity_ambient=0.3, intensity_directional=0.8, color_ambient=(1.0, 0.9, 0.8),
              color_directional=(0.7, 1.0, 0.6), direction=(0.3, 0.8, -0.5), fill_back=fill_back, smooth=smooth)
    got = nr.vertex_light(v, f, implementation='torch', **kw)
    want = vertex_shade_torch(v, f, torch.ones(v.shape[1], 3), **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, (2 if fill_back else 1) * f.shape[0], 3, 3)
    assert torch.equal(got, want)
    assert nr.vertex_light is __import__('neural_renderer').vertex_light
    g = torch.tensor(rng.normal(size=tuple(got.shape)).astype(np.float32))
    gv, = torch.autograd.grad((got * g).sum(), v)
    gw, = torch.autograd.grad((want * g).sum(), v)
    assert torch.equal(gv, gw) and (gv != 0).any()
    with pytest.raises(ValueError):
        nr.vertex_light(v[0], f)
    with pytest.raises(ValueError):
        nr.vertex_light(v, f, implementation='hip')    # CPU tensors do not fit the kernels


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_adjoint_matches_central_differences(seed):
    """The restatement's adjoint against central differences of render64, float64 against float64.  The render is affine in
    every single entry of the light and of the images, so a central difference has no truncation error and h = 0.25 keeps its
    rounding error near 1e-15 of the loss.  The adjoint multiplies the forward's FLOAT32 c and L (as the kernel does) where
    render64 has their float64 values.  With uv triangles inside [0, 1]^2 (clipped here) every read weight is >= 0, so c is a
    sum of non-negative terms with 4 products and 4 additions (the first to 0) and L one with 3 products and 2 additions:
    |c32 - c| <= gamma_8 c and |L32 - L| <= gamma_5 L in float32, hence every term of an entry, and so the entry, lies within
    gamma_8 of its sum of |terms|."""
    sc = R.scene(seed)
    sc['uv'] = np.clip(sc['uv'], 0, 1)
    fi, wm, dm = _oracle_maps(sc)
    assert (fi >= 0).sum() > 50
    layout = _layout(sc)
    images = R.np_images(sc)
    rng = sc['rng']
    g = rng.normal(size=(sc['B'], sc['S'], sc['S'], 3)).astype(np.float32)
    gi, gi_mag, gl, gl_mag = R.adjoint(sc['faces'], fi, wm, dm, sc['light'], layout, images, EPS, g)
    assert gl.shape == sc['light'].shape and (gl_mag > 0).any()

    def loss(light, imgs):
        (b, y, x), rgb = R.render64(sc['faces'], fi, wm, dm, light, layout, imgs, EPS)
        return float((rgb * g[b, y, x].astype(np.float64)).sum())
    light64 = sc['light'].astype(np.float64)
    images64 = [im.astype(np.float64) for im in images]
    h, bound, worst, checked = 0.25, H.gamma(8), 0.0, 0
    fed = np.argwhere(gl_mag > 0)
    for idx in fed[rng.permutation(len(fed))[:12]]:
        idx = tuple(idx)
        lp, lm = light64.copy(), light64.copy()
        lp[idx] += h
        lm[idx] -= h
        fd = (loss(lp, images64) - loss(lm, images64)) / (2 * h)
        worst = max(worst, abs(fd - gl[idx]) / (bound * gl_mag[idx]))
        checked += 1
    for m in range(len(images)):
        fed = np.argwhere(gi_mag[m] > 0)
        for idx in fed[rng.permutation(len(fed))[:6]]:
            idx = tuple(idx)
            ip, im_ = [a.copy() for a in images64], [a.copy() for a in images64]
            ip[m][idx] += h
            im_[m][idx] -= h
            fd = (loss(light64, ip) - loss(light64, im_)) / (2 * h)
            worst = max(worst, abs(fd - gi[m][idx]) / (bound * gi_mag[m][idx]))
            checked += 1
    print('uv smooth restatement: adjoint vs central differences, worst share of gamma_8 x sum|terms| = %.3f (%d entries)'
          % (worst, checked))
    assert checked >= 12 and worst <= 1


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_equal_corner_lights_give_the_flat_render(seed):
    """light[b,f,k] = l for the three corners: the smooth restatement against uv_pixel_ref.render with light l.  The forward
    made w_k in [0, 1] and zp = 1 / ((w_0 / z_0 + w_1 / z_1) + w_2 / z_2) with z_k > 0, so with T_k = w_k / z_k the stored
    zp times sum T_k is 1 up to 4 roundings a term (its division, two additions, the reciprocal).  e_k = w_k * (zp / z_k) adds
    2, the clamp to 1 at most 1 (it only cuts what rounding put above 1), l * e_k 1 and the two additions 2: L = l (1 +
    theta_10), every term non-negative.  The two renders then round c * L and c * l once each: they differ by at most
    gamma_12 |value|."""
    sc = R.scene(seed)
    fi, wm, dm = _oracle_maps(sc)
    assert (fi >= 0).sum() > 50
    layout = _layout(sc)
    images = R.np_images(sc)
    flat = sc['light'][:, :, 0, :].copy()
    light = np.repeat(flat[:, :, None, :], 3, axis=2)
    got = R.render(sc['faces'], fi, wm, dm, light, layout, images, EPS, BG)
    want = P.render(sc['faces'], fi, wm, dm, flat, layout, images, EPS, BG)
    cov = fi >= 0
    assert np.array_equal(got[~cov], want[~cov])
    err = np.abs(got.astype(np.float64) - want)[cov]
    bound = H.gamma(12) * np.abs(want.astype(np.float64))[cov]
    print('uv smooth restatement, equal corner lights: worst share of gamma_12 |value| = %.3f'
          % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()
    # and a light that differs between the corners changes the picture
    assert not np.array_equal(R.render(sc['faces'], fi, wm, dm, sc['light'], layout, images, EPS, BG)[cov], want[cov])


def _uv(images=1, table=1, faces_uv=1, face_image=1, base=1, ts=4, M=1, P_=16, Bi=1):
    return _lib.UVImagesStruct(images, table, faces_uv, face_image, base, ts, M, P_, Bi)


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    E_NULL, E_SIZE, E_WS, E_MODE = -1, -2, -3, -4
    lit = _lib.CornerLight(1, 4, None)          # Nf = 4, F = 8 (fill_back)

    def fwd(lit=lit, uv=None, faces=1, fim=1, rgb=1, bg=1, B=2, F=8, S=16, ws=None):
        uv = _uv() if uv is None else uv
        return lib.nr_forward_rasterize_uv_smooth(lit, uv, faces, fim, None, None, rgb, None, None, bg, 0, B, F, S, 0.1,
                                                  100.0, 1e-3, 0, ws, 0, None)
    assert fwd(lit=None) == E_NULL
    assert fwd(lit=_lib.CornerLight(None, 4, None)) == E_NULL
    assert fwd(uv=_uv(images=None)) == E_NULL
    assert fwd(uv=_uv(base=None)) == E_NULL
    assert fwd(rgb=None) == E_NULL
    assert fwd(bg=None) == E_NULL
    assert fwd(faces=None) == E_NULL
    assert fwd(fim=None) == E_NULL
    assert fwd(lit=_lib.CornerLight(1, 3, None)) == E_SIZE          # texture_faces neither F nor F / 2
    assert fwd(F=4) == E_WS                                          # F == Nf (no fill_back) is valid too
    assert fwd(uv=_uv(Bi=3)) == E_SIZE                               # image_batch neither 1 nor B
    assert fwd(uv=_uv(ts=1)) == E_SIZE
    assert fwd(S=0) == E_SIZE
    assert fwd() == E_WS                                             # everything right but the workspace

    def bwd(lit=_lib.CornerLight(1, 4, 1), uv=None, wm=1, g=1, gi=1, B=2, F=8, S=16, ws=None, wsb=0):
        uv = _uv() if uv is None else uv
        return lib.nr_backward_uv_images_smooth(lit, uv, 1, 1, wm, 1, g, gi, B, F, S, 1e-3, ws, wsb, None)
    assert bwd(lit=None) == E_NULL
    assert bwd(lit=_lib.CornerLight(None, 4, 1)) == E_NULL
    assert bwd(uv=_uv(face_image=None)) == E_NULL
    assert bwd(wm=None) == E_NULL
    assert bwd(g=None) == E_NULL
    assert bwd(lit=_lib.CornerLight(1, 5, 1)) == E_SIZE
    assert bwd(uv=_uv(Bi=3)) == E_SIZE
    assert bwd(B=0) == E_SIZE
    assert bwd(lit=_lib.CornerLight(1, 4, None), gi=None) == E_MODE   # no gradient asked for
    need = lib.nr_backward_uv_images_smooth_workspace_bytes(2, 8, 16, 1)
    assert need >= 8 * (16 * 3 + 2 * 8 * 9)                          # nine sums per face
    assert need > lib.nr_backward_uv_images_workspace_bytes(2, 8, 16, 1)
    assert lib.nr_backward_uv_images_smooth_workspace_bytes(2, 8, 16, 2) >= 8 * (2 * 16 * 3 + 2 * 8 * 9)
    assert lib.nr_backward_uv_images_smooth_workspace_bytes(2, 8, 16, 3) == 0
    assert lib.nr_backward_uv_images_smooth_workspace_bytes(2, 8, 0, 1) == 0
    assert bwd() == E_WS
    assert bwd(ws=1, wsb=need - 1) == E_WS


def test_shapes_refused_before_any_device_work():
    """The shading sources' own checks (they run before anything is allocated or launched), on CPU tensors."""
    import torch
    import neural_renderer_amd as nr
    import sys
    rz = sys.modules[nr.rasterize.__module__]  # (the package attribute `rasterize` is the function)
    B, Nf = 2, 6
    layout = _layout(dict(uv=np.zeros((Nf, 3, 2), np.float32), face_image=np.zeros(Nf, np.int32),
                          base=np.zeros((Nf, 2, 2, 2, 3), np.float32), sizes=[(2, 2)]))
    cfg = types.SimpleNamespace(return_rgb=True)
    faces = torch.zeros(B, Nf, 3, 3)
    src = rz._UVSource(types.SimpleNamespace(layout=layout, image_batch=1, device=faces.device))
    for F, shape in ((Nf, (B, Nf)), (Nf, (B, Nf, 4)), (Nf, (B, Nf, 3, 2)), (Nf, (B, Nf, 2, 3)), (Nf, (B, Nf + 1, 3, 3)),
                     (Nf, (1, Nf, 3, 3)), (2 * Nf, (B, Nf, 3, 3)), (Nf, (B, Nf, 3, 3, 1))):
        with pytest.raises(ValueError, match=r'3\] \(a colour per face\) or .*3, 3\] \(a colour per corner\)'):
            src.check(cfg, faces, B, F, (torch.zeros(shape),))
    with pytest.raises(ValueError, match='per corner'):
        src.check(cfg, faces, B, Nf, (torch.zeros(B, Nf, 3, 3, dtype=torch.float64),))
    with pytest.raises(ValueError, match='on the GPU'):
        src.check(cfg, faces, B, Nf, (torch.zeros(B, Nf, 3, 3),))      # the right shape, but not on the GPU
    # cubes take one colour per face: a light per corner is refused with a message that says so
    cubes = torch.zeros(B, Nf, 2, 2, 2, 3)
    with pytest.raises(ValueError, match='per corner.*UVImages'):
        rz._CUBES.check(cfg, faces, B, Nf, (cubes, torch.zeros(B, Nf, 3, 3)))
    with pytest.raises(ValueError, match='face_light must be float32'):
        rz._CUBES.check(cfg, faces, B, Nf, (cubes, torch.zeros(B, Nf, 3, 2)))
    with pytest.raises(ValueError, match='per corner'):
        rz._source_of(nr.UVImages.__new__(nr.UVImages), None)          # UVImages without face_light: both shapes named
    # Renderer: cubes stay flat, and the message points to what takes smooth light
    r = nr.Renderer()
    r.shading = 'smooth'
    with pytest.raises(ValueError, match='UVImages or VertexColors'):
        r.render(torch.zeros(B, 5, 3), torch.zeros(B, Nf, 3, dtype=torch.int32), cubes)
