"""`-m gpu`: the soft colour kernels with texture cubes sampled at the pixel (csrc/nr_soft_render.hip, the nr_soft_cubes_*
entries), soft_render_cubes and Renderer.render_soft(per_pixel=True) with a TextureCubes.

rgba, grad_faces, grad_textures and grad_light against the float64 restatement of tests/soft_cubes_ref.py under its derived
bounds, on the geometry and (S, sigma, gamma) of tests/test_soft_render_gpu.py's cases with ts = 2 (fewer texels than lanes), 4
(exactly a wave), 5 (a partial tail) and 8; reproducibility; shared cubes and light; texture_eps = 0 and cubes that must not
be read; the tensor boundary and a side stream; an affine and a constant cube against the corner and the flat kernels; the
renderer end to end, against soft_render_cubes of the composition and against the hard rasterizer; the example.  "Bit for
bit" is torch.equal, for all four outputs: the cube gradient is summed in a fixed order without atomics.  The cases and
their references are also read by tests/test_soft_cubes.py (CPU: the caps and the sensitivity of the bounds).

No stream-capture test: two capture sequences on this project have ended in a host segmentation fault inside torch (DESIGN
"Soft silhouettes", Stream capture); capture before any eager backward on the same leaves.

Worst ratios measured on the MI355X: see DESIGN "Soft colour rendering", Texture cubes (every case prints its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import soft_cubes_ref as R
import soft_render_ref as R0
from test_soft_render_gpu import BG, _cuda, _faces, _host

pytestmark = pytest.mark.gpu

# (mesh, B, S, sigma, gamma, ts): B = 3 runs with cubes shared by the batch, B = 2 with cubes per image; the spheres at the
# three (S, sigma, gamma) of the issue, both 'mix' geometries (330 faces: a chunk and a tail, dropped and zero-area faces);
# ts = 8 once, on the smallest case
_BASE = [('ico1', 3, 20, 1e-6, 1e-1), ('ico1', 3, 32, 1e-3, 1e-4), ('ico1', 3, 16, 1.0, 1e-1),
         ('mix', 2, 32, 1e-3, 1e-4), ('mix', 2, 20, 1e-3, 1e-1)]
CASES = [c + (ts,) for c in _BASE for ts in (2, 4, 5)] + [('ico1', 3, 16, 1.0, 1e-1, 8)]
IDS = ['%s-B%d-S%d-sigma%g-gamma%g-ts%d' % c for c in CASES]
U = 2.0 ** -24

_cache = {}


def reference(mesh, B, S, sigma, gamma, ts, adds=None):
    """(faces, textures, light, the restatement's Result -- with .g, the upstream gradient, 0 on the masked pixels): once per
    case.  B = 3: cubes shared by the batch; otherwise one set per image."""
    key = (mesh, B, S, sigma, gamma, ts, adds)
    if key not in _cache:
        faces = _faces(mesh, B)
        F = faces.shape[1]
        rng = np.random.default_rng(B * 1000 + S + 17 * ts)
        textures = rng.uniform(0, 1, (1 if B == 3 else B, F, ts, ts, ts, 3)).astype(np.float32)
        light = rng.uniform(0.5, 1.5, (B, F, 3)).astype(np.float32)
        g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
        ref = R.restate(faces, textures, light, S, sigma, gamma, background=BG, g=g, adds=adds)
        _cache[key] = (faces, textures, light, ref)
    return _cache[key]


def _run(faces, textures, light, g, S, sigma, gamma, texture_eps=1e-3, implementation='hip', texture_grad=True):
    """-> rgba, grad_faces, grad_textures (None without texture_grad), grad_light."""
    import neural_renderer_amd as nr
    ft, tt, lt = _cuda(faces, True), _cuda(textures, texture_grad), _cuda(light, True)
    rgba = nr.soft_render_cubes(ft, tt, lt, S, sigma, gamma, background_color=BG, texture_eps=texture_eps,
                                implementation=implementation)
    rgba.backward(_cuda(np.asarray(g, np.float32)))
    return rgba.detach(), ft.grad, tt.grad, lt.grad


def _off(faces):
    """[B,F]: the faces that do not contribute."""
    f64 = faces.astype(np.float64)
    with np.errstate(all='ignore'):
        area = (f64[:, :, 1, 0] - f64[:, :, 0, 0]) * (f64[:, :, 2, 1] - f64[:, :, 0, 1]) \
            - (f64[:, :, 2, 0] - f64[:, :, 0, 0]) * (f64[:, :, 1, 1] - f64[:, :, 0, 1])
        return ~(np.isfinite(f64).all((2, 3)) & (f64[..., 2] >= 0.1).all(2) & (f64[..., 2] <= 100).all(2) & (area != 0))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement's bounds

@pytest.mark.parametrize('mesh,B,S,sigma,gamma,ts', CASES, ids=IDS)
def test_forward_and_gradients_within_the_derived_bounds(mesh, B, S, sigma, gamma, ts):
    """rgba (outside the masked pixels), grad_faces, grad_textures and grad_light from random upstream gradients (0 on the
    masked pixels) within the per-entry bounds of soft_cubes_ref (its docstring); the caps."""
    faces, textures, light, ref = reference(mesh, B, S, sigma, gamma, ts)
    rgba, gf, gt, gl = _run(faces, textures, light, ref.g, S, sigma, gamma)
    assert tuple(rgba.shape) == (B, 4, S, S) and tuple(gf.shape) == faces.shape and tuple(gl.shape) == light.shape
    assert tuple(gt.shape) == textures.shape
    rr = R.masked_ratio(_host(rgba), ref.rgba, ref.rgba_bound, ref.mask)
    rf = R.worst_ratio(_host(gf), ref.grad_faces, ref.grad_faces_bound)
    rl = R.worst_ratio(_host(gl), ref.grad_light, ref.grad_light_bound)
    if B == 3:
        total, _, bound = R.shared(ref, 'grad_textures')
    else:
        total, bound = ref.grad_textures, ref.grad_textures_bound
    rt = R.worst_ratio(_host(gt), total, bound)
    print('%s B=%d S=%d sigma=%g gamma=%g ts=%d: rgba %.3f, grad_faces %.3f, grad_textures %.3f, grad_light %.3f of the bound; '
          'masked %.2f %% of the pixels with a pair, segment doubt %.2f %%, tap doubt %.4f %% of %d pairs'
          % (mesh, B, S, sigma, gamma, ts, rr, rf, rt, rl, 100 * ref.masked_share, 100 * ref.doubt_share,
             100 * ref.tap_doubt_share, sum(ref.pairs)))
    assert ref.masked_share <= 0.01 and ref.doubt_share <= 0.02 and ref.tap_doubt_share <= 0.01
    assert rr <= 1 and rf <= 1 and rt <= 1 and rl <= 1, (rr, rf, rt, rl)
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_light).max() > 0 and np.abs(total).max() > 0
    assert all(torch.isfinite(x).all() for x in (rgba, gf, gt, gl))
    assert gf[..., 2].abs().max() > 0 and gt.abs().max() > 0 and gl.abs().max() > 0
    off = _off(faces)
    if off.any():   # a dropped face's entries are exact zeros
        assert (_host(gf)[off] == 0).all() and (_host(gl)[off] == 0).all()
        assert (_host(gt)[off if B != 3 else off[:1]] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. reproducibility

@pytest.mark.parametrize('case', [('mix', 2, 32, 1e-3, 1e-4, 5), ('ico1', 3, 32, 1e-3, 1e-4, 4)])
def test_two_runs_and_an_image_alone(case):
    """All four outputs: the same bits in two runs, and for an image alone (with its own cubes) as inside the batch."""
    mesh, B, S, sigma, gamma, ts = case
    faces, textures, light, ref = reference(*case)
    wide = np.ascontiguousarray(np.broadcast_to(textures, (B,) + textures.shape[1:]))    # cubes per image
    a0 = _run(faces, wide, light, ref.g, S, sigma, gamma)
    a1 = _run(faces, wide, light, ref.g, S, sigma, gamma)
    assert all(torch.equal(x, y) for x, y in zip(a0, a1)) and all(x.abs().sum() > 0 for x in a0)
    for b in range(B):
        one = _run(faces[b:b + 1], wide[b:b + 1], light[b:b + 1], ref.g[b:b + 1], S, sigma, gamma)
        assert all(torch.equal(x[0], y[b]) for x, y in zip(one, a0)), b


# ---------------------------------------------------------------------------------------------------------------------
# 3. shared cubes and shared light

def test_shared_cubes_and_shared_light():
    """Cubes [1,F,...] and light [1,F,3] beside B = 3: rgba and grad_faces have the bits of the expanded call; the shared
    gradients agree with the float64 sum over the batch within its bound."""
    S, sigma, gamma, ts = 20, 1e-3, 1e-1, 4
    faces = _faces('ico1', 3)
    F = faces.shape[1]
    rng = np.random.default_rng(19)
    textures = rng.uniform(0, 1, (1, F, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.5, 1.5, (1, F, 3)).astype(np.float32)
    g = rng.normal(size=(3, 4, S, S)).astype(np.float32)
    ref = R.restate(faces, textures, light, S, sigma, gamma, background=BG, g=g)
    assert ref.masked_share <= 0.01
    rgba, gf, gt, gl = _run(faces, textures, light, ref.g, S, sigma, gamma)
    rgba_w, gf_w, gt_w, gl_w = _run(faces, np.repeat(textures, 3, 0), np.repeat(light, 3, 0), ref.g, S, sigma, gamma)
    assert tuple(gl.shape) == (1, F, 3) and tuple(gl_w.shape) == (3, F, 3)
    assert tuple(gt.shape) == textures.shape and tuple(gt_w.shape) == (3,) + textures.shape[1:]
    assert torch.equal(rgba, rgba_w) and torch.equal(gf, gf_w)
    tt, _, bt = R.shared(ref, 'grad_textures')
    tl, _, bl = R.shared(ref, 'grad_light')
    rt, rl = R.worst_ratio(_host(gt), tt, bt), R.worst_ratio(_host(gl), tl, bl)
    rw = R.worst_ratio(_host(gt_w), ref.grad_textures, ref.grad_textures_bound)
    print('shared cubes and light: grad_textures %.3f (per image %.3f), grad_light %.3f of the bound' % (rt, rw, rl))
    assert rt <= 1 and rl <= 1 and rw <= 1 and np.abs(tt).max() > 0 and np.abs(tl).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. texture_eps = 0, and cubes that must not be read

def test_texture_eps_zero_and_cubes_that_must_not_be_read():
    """texture_eps = 0 on the mixed case plus one face of constant depth 2 (outside, at its vertices, mu is exactly (1, 0, 0):
    v = ts - 1, the upper taps leave the cube) with the dropped and zero-area faces' cubes filled with NaN: everything is
    finite, rgba has the bits of the call without those faces, their grad_textures are exact zeros."""
    S, sigma, gamma, ts, B = 20, 1e-3, 1e-1, 4, 2
    flat_face = np.array([[-0.6, -0.5, 2.0], [-0.1, -0.55, 2.0], [-0.3, -0.1, 2.0]], np.float32)
    faces = _faces('mix', B)
    faces = np.ascontiguousarray(np.concatenate((faces, np.broadcast_to(flat_face, (B, 1, 3, 3))), 1))
    F = faces.shape[1]
    off = _off(faces)
    assert (off.sum(1) == 6).all() and np.array_equal(off[0], off[1])
    rng = np.random.default_rng(23)
    textures = rng.uniform(0, 1, (B, F, ts, ts, ts, 3)).astype(np.float32)
    textures[off] = np.nan
    light = rng.uniform(0.5, 1.5, (B, F, 3)).astype(np.float32)
    g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
    rgba, gf, gt, gl = _run(faces, textures, light, g, S, sigma, gamma, texture_eps=0.0)
    assert all(torch.isfinite(x).all() for x in (rgba, gf, gt, gl))
    assert (_host(gt)[off] == 0).all() and (_host(gf)[off] == 0).all() and (_host(gl)[off] == 0).all()
    assert gt[:, -1].abs().sum() > 0 and gf[:, -1].abs().sum() > 0
    keep = ~off[0]
    rgba2, gf2, gt2, gl2 = _run(faces[:, keep], textures[:, keep], light[:, keep], g, S, sigma, gamma, texture_eps=0.0)
    assert torch.equal(rgba, rgba2) and torch.equal(gf[:, keep], gf2) and torch.equal(gt[:, keep], gt2) and torch.equal(gl[:, keep], gl2)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the tensor boundary

def test_layouts_alignment_and_a_side_stream():
    """faces, cubes, light and the upstream gradient as a strided view, as views 4 / 8 / 12 bytes off the 16-byte grid and
    permuted, and one call on a side stream: the bits of the dense call.  Cubes without requires_grad (grad_textures = NULL):
    the same grad_faces and grad_light bits."""
    import neural_renderer_amd as nr
    from test_layout_invariance_gpu import FLOAT_LAYOUTS, grad_as, lay
    case = ('ico1', 3, 32, 1e-3, 1e-4, 4)
    S, sigma, gamma = case[2:5]
    faces, textures, light, ref = reference(*case)
    gt = _cuda(np.asarray(ref.g, np.float32))
    ref_a, ref_f, ref_t, ref_l = _run(faces, textures, light, ref.g, S, sigma, gamma)
    assert all(x.abs().sum() > 0 for x in (ref_a, ref_f, ref_t, ref_l))
    for fl in FLOAT_LAYOUTS:
        for gl in ('plain', fl):
            lf, lt, ll = [lay(_cuda(x), fl).requires_grad_(True) for x in (faces, textures, light)]
            out = nr.soft_render_cubes(lf, lt, ll, S, sigma, gamma, background_color=BG, implementation='hip')
            assert torch.equal(out.detach(), ref_a), fl
            grad_as(out, gl).backward(gt)
            assert torch.equal(lf.grad, ref_f) and torch.equal(lt.grad, ref_t) and torch.equal(ll.grad, ref_l), (fl, gl)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    lf, lt, ll = _cuda(faces, True), _cuda(textures, True), _cuda(light, True)
    with torch.cuda.stream(side):
        out = nr.soft_render_cubes(lf, lt, ll, S, sigma, gamma, background_color=BG, implementation='hip')
        out.backward(gt)
    side.synchronize()
    assert torch.equal(out.detach(), ref_a) and torch.equal(lf.grad, ref_f) and torch.equal(lt.grad, ref_t) and torch.equal(ll.grad, ref_l)
    rgba, gf, none, gl = _run(faces, textures, light, ref.g, S, sigma, gamma, texture_grad=False)
    assert none is None and torch.equal(rgba, ref_a) and torch.equal(gf, ref_f) and torch.equal(gl, ref_l)


# ---------------------------------------------------------------------------------------------------------------------
# 6. an affine and a constant cube: the corner and the flat kernels

def affine_cube(rng, F, ts):
    """Cubes whose texels are a + b . (i, j, k) per face and channel, every number a short dyadic fraction -> (cubes
    [F,ts,ts,ts,3], the corner colours [F,3 corners,3] they interpolate: corner k is the texel at (ts - 1) e_k)."""
    a = rng.integers(1, 8, (F, 1, 1, 1, 3)) / 16.0
    b = rng.integers(-3, 4, (F, 3, 3)) / 32.0                                  # [F, axis, rgb]
    i, j, k = np.meshgrid(np.arange(ts), np.arange(ts), np.arange(ts), indexing='ij')
    cube = a + i[None, ..., None] * b[:, None, None, None, 0] + j[None, ..., None] * b[:, None, None, None, 1] \
        + k[None, ..., None] * b[:, None, None, None, 2]
    corner = a.reshape(F, 1, 3) + (ts - 1) * b
    return cube, corner


@pytest.mark.parametrize('case', [('mix', 2, 20, 1e-3, 1e-1, 5), ('ico1', 3, 32, 1e-3, 1e-4, 4)])
def test_an_affine_cube_against_the_corner_kernels(case):
    """tex[i,j,k] = a + b . (i, j, k): the trilinear read of an affine cube is affine in v, v = mu (ts - 1) and sum mu_k = 1, so
    the definition equals soft_render with the corner colours L_f (a + (ts - 1) b_k) once texture_eps = 0 takes the upper
    clamp away (at v_k = ts - 1 the taps that leave the cube carry weight 0; what their absence does to D_k is multiplied by
    an exact 0, soft_render_cubes' docstring).  rgba, grad_faces and grad_light (against the corner gradient contracted with
    the unlit corners) within the sum of the two restatements' bounds."""
    import neural_renderer_amd as nr
    mesh, B, S, sigma, gamma, ts = case
    faces = _faces(mesh, B)
    F = faces.shape[1]
    rng = np.random.default_rng(F + S)
    cube, unlit = affine_cube(rng, F, ts)
    textures = cube[None].astype(np.float32)
    light = (rng.integers(2, 6, (B, F, 3)) / 4.0).astype(np.float32)
    corner = (light[:, :, None, :] * unlit[None]).astype(np.float32)
    assert np.array_equal(textures.astype(np.float64), cube[None])
    assert np.array_equal(corner.astype(np.float64), light[:, :, None, :].astype(np.float64) * unlit[None])   # exact
    g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
    ref_t = R.restate(faces, textures, light, S, sigma, gamma, background=BG, texture_eps=0.0, g=g)
    ref_c = R0.restate(faces, corner, S, sigma, gamma, background=BG, g=ref_t.g)
    assert np.array_equal(ref_c.mask, ref_t.mask) and np.array_equal(ref_c.g, ref_t.g)
    a, af, _, al = _run(faces, textures, light, ref_t.g, S, sigma, gamma, texture_eps=0.0)
    ft, ct = _cuda(faces, True), _cuda(corner, True)
    b = nr.soft_render(ft, ct, S, sigma, gamma, background_color=BG, implementation='hip')
    b.backward(_cuda(np.asarray(ref_t.g, np.float32)))
    keep = ~np.broadcast_to(ref_t.mask[:, None], ref_t.rgba.shape)
    rr = R.worst_ratio(_host(a)[keep], _host(b).astype(np.float64)[keep], (ref_t.rgba_bound + ref_c.rgba_bound)[keep])
    rf = R.worst_ratio(_host(af), _host(ft.grad).astype(np.float64), ref_t.grad_faces_bound + ref_c.grad_faces_bound)
    bl = (_host(ct.grad).astype(np.float64) * unlit[None]).sum(2)   # dL/dL_fc = sum_k dL/dC_fkc unlit_fkc
    rl = R.worst_ratio(_host(al), bl, ref_t.grad_light_bound + (ref_c.grad_colors_bound * np.abs(unlit[None])).sum(2))
    print('%s affine cube against corner colours: rgba %.3f, grad_faces %.3f, grad_light %.3f of the two bounds' % (mesh, rr, rf, rl))
    assert rr <= 1 and rf <= 1 and rl <= 1, (rr, rf, rl)
    assert af.abs().sum() > 0 and al.abs().sum() > 0


def test_a_constant_cube_against_the_flat_kernels():
    """Every texel of a face's cube the same colour: the sample is that colour (the weights sum to 1 within their roundings)
    and E_k is a rounding.  rgba, grad_faces and grad_light (against the flat colour gradient times the colour) within the sum
    of the two restatements' bounds."""
    import neural_renderer_amd as nr
    mesh, B, S, sigma, gamma, ts = 'mix', 2, 20, 1e-3, 1e-1, 4
    faces = _faces(mesh, B)
    F = faces.shape[1]
    rng = np.random.default_rng(29)
    col = rng.integers(1, 16, (B, F, 3)) / 16.0
    textures = np.ascontiguousarray(np.broadcast_to(col[:, :, None, None, None, :], (B, F, ts, ts, ts, 3))).astype(np.float32)
    light = (rng.integers(2, 6, (B, F, 3)) / 4.0).astype(np.float32)
    flat = (light * col).astype(np.float32)
    assert np.array_equal(flat.astype(np.float64), light.astype(np.float64) * col)
    g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
    ref_t = R.restate(faces, textures, light, S, sigma, gamma, background=BG, g=g)
    ref_c = R0.restate(faces, flat, S, sigma, gamma, background=BG, g=ref_t.g)
    a, af, _, al = _run(faces, textures, light, ref_t.g, S, sigma, gamma)
    ft, ct = _cuda(faces, True), _cuda(flat, True)
    b = nr.soft_render(ft, ct, S, sigma, gamma, background_color=BG, implementation='hip')
    b.backward(_cuda(np.asarray(ref_t.g, np.float32)))
    keep = ~np.broadcast_to(ref_t.mask[:, None], ref_t.rgba.shape)
    rr = R.worst_ratio(_host(a)[keep], _host(b).astype(np.float64)[keep], (ref_t.rgba_bound + ref_c.rgba_bound)[keep])
    rf = R.worst_ratio(_host(af), _host(ft.grad).astype(np.float64), ref_t.grad_faces_bound + ref_c.grad_faces_bound)
    rl = R.worst_ratio(_host(al), _host(ct.grad).astype(np.float64) * col, ref_t.grad_light_bound + ref_c.grad_colors_bound * col)
    print('constant cube against the flat kernels: rgba %.3f, grad_faces %.3f, grad_light %.3f of the two bounds' % (rr, rf, rl))
    assert rr <= 1 and rf <= 1 and rl <= 1, (rr, rf, rl)


# ---------------------------------------------------------------------------------------------------------------------
# 7. through the renderer

def _sphere_scene(B=2):
    import neural_renderer_amd as nr
    v, f = nr.icosphere(2, 0.8)
    return v[None].repeat(B, 1, 1).cuda(), f[None].repeat(B, 1, 1).cuda()


@pytest.mark.parametrize('lights', [False, True])
def test_render_soft_per_pixel_is_the_composition(lights):
    """Bit-equal to soft_render_cubes(the front copies of the front-end's faces, the cubes, the per-face light of the front
    copies that render() hands its rasterizer, texture_eps = rasterizer_eps); `lights` are honoured."""
    import neural_renderer_amd as nr
    vertices, faces = _sphere_scene()
    F = faces.shape[1]
    cubes = torch.rand(1, F, 4, 4, 4, 3, device='cuda')
    r = nr.Renderer()
    r.image_size, r.eye = 32, nr.get_points_from_angles(2.732, 25, 40)
    r.soft_gamma, r.background_color = 1e-2, list(BG)
    if lights:
        r.lights = nr.Lights(sh=0.1 * torch.randn(9, 3)).cuda()
    img = r.render_soft(vertices, faces, nr.TextureCubes(cubes), per_pixel=True)
    proj, same, kw = r._shade(vertices, faces, cubes)          # (cubes shared by a batch: render() lights them per face)
    assert proj.shape[1] == 2 * F and same is cubes and tuple(kw['face_light'].shape) == (2, 2 * F, 3)
    want = nr.soft_render_cubes(proj[:, :F], cubes, kw['face_light'][:, :F], 32, r.soft_sigma, 1e-2, r.near, r.far, r.soft_eps,
                                BG, r.rasterizer_eps)
    assert img.shape == (2, 4, 32, 32) and torch.equal(img, want) and img[:, :3].abs().sum() > 0
    if lights:
        plain = nr.Renderer()
        plain.image_size, plain.eye, plain.soft_gamma, plain.background_color = 32, r.eye, 1e-2, list(BG)
        assert not torch.equal(img, plain.render_soft(vertices, faces, nr.TextureCubes(cubes), per_pixel=True))


def test_render_soft_per_pixel_gradients_on_the_gpu():
    """Gradients reach the vertices (z included), the cubes and a learnable eye."""
    import neural_renderer_amd as nr
    vertices, faces = _sphere_scene(1)
    vertices.requires_grad_(True)
    cubes = torch.rand(1, faces.shape[1], 4, 4, 4, 3, device='cuda', requires_grad=True)
    r = nr.Renderer()
    r.image_size = 32
    r.eye = torch.tensor(nr.get_points_from_angles(2.732, 25, 40), dtype=torch.float32, device='cuda', requires_grad=True)
    r.soft_sigma, r.soft_gamma = 1e-3, 1e-2
    w = torch.randn(1, 4, 32, 32, device='cuda')
    (r.render_soft(vertices, faces, nr.TextureCubes(cubes), per_pixel=True) * w).sum().backward()
    assert torch.isfinite(vertices.grad).all() and vertices.grad[..., 2].abs().sum() > 0
    assert torch.isfinite(cubes.grad).all() and cubes.grad.abs().sum() > 0
    assert torch.isfinite(r.eye.grad).all() and r.eye.grad.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. the hard rasterizer

def test_render_soft_per_pixel_against_the_hard_rasterizer():
    """The strongly tilted quad of test_soft_corners_gpu.py with random cubes of ts = 4, ambient light only: render() without
    anti-aliasing and render_soft(per_pixel=True) with sigma = 1e-8, gamma = 1e-4 on the pixels farther than sqrt(30 sigma) from
    every edge.  In float64 the two definitions differ by 0 there (asserted to 1e-12).  The float32 images may differ by a few
    ulp of v times the cube's slope -- the two kernels form the weights as w_k (zp / z_k) and as (lambda_k / z_k) zp --: the
    ceiling 64 u (ts - 1) sum_dims max |delta texel| + 16 u is asserted (the UV test measured 8 ulp of its position: a factor
    near 8 is left); an affine interpolation would be off by 0.05.  Measured on the MI355X: see DESIGN."""
    import neural_renderer_amd as nr
    S, sigma, gamma, ts = 32, 1e-8, 1e-4, 4
    vertices = torch.tensor([[[-0.93, -0.71, -0.83], [0.91, -0.69, -0.79], [0.89, 0.73, 0.91], [-0.87, 0.67, 0.88]]], device='cuda')
    faces = torch.tensor([[[0, 1, 2], [0, 2, 3]]], dtype=torch.int32, device='cuda')
    rng = np.random.default_rng(37)
    cubes_h = rng.uniform(0, 1, (1, 2, ts, ts, ts, 3)).astype(np.float32)
    cubes = _cuda(cubes_h)
    r = nr.Renderer()
    r.image_size, r.anti_aliasing, r.background_color = S, False, list(BG)
    r.light_intensity_ambient, r.light_intensity_directional = 1.0, 0.0
    hard = r.render(vertices, faces, cubes)
    soft = r.render_soft(vertices, faces, nr.TextureCubes(cubes), sigma=sigma, gamma=gamma, per_pixel=True)
    assert hard.shape == (1, 3, S, S) and soft.shape == (1, 4, S, S)
    proj = r._shade(vertices, faces, cubes)[0]
    pf, pl = _host(proj[:, :2]).astype(np.float64), np.ones((1, 2, 3))
    ref = R.restate(pf, cubes_h, pl, S, sigma, gamma, r.near, r.far, r.soft_eps, BG, r.rasterizer_eps)
    hard64 = R.hard_image(pf, cubes_h, pl, S, BG, r.rasterizer_eps)
    compared = np.broadcast_to((ref.edge_d2 > 30 * sigma)[:, None], hard64.shape)
    covered = compared & np.broadcast_to((ref.rgba[:, 3:] > 0.5), hard64.shape)
    assert covered.sum() >= 3 * 100 and (compared & ~covered).sum() >= 3 * 100          # the quad and the background
    assert np.abs(ref.rgba[:, :3] - hard64)[compared].max() <= 1e-12
    c64 = cubes_h.astype(np.float64)
    slope = sum(np.abs(np.diff(c64, axis=ax)).max() for ax in (2, 3, 4))
    ceiling = 64 * U * (ts - 1) * slope + 16 * U
    got = np.abs(_host(soft[:, :3]).astype(np.float64) - _host(hard).astype(np.float64))[compared].max()
    print('render_soft(per_pixel, TextureCubes) against render: worst difference %.3e on %d compared values, ceiling %.3e'
          % (got, compared.sum(), ceiling))
    assert ceiling < 1e-4
    assert got <= ceiling
    # ... and each against its own float64 definition
    assert np.abs(_host(soft[:, :3]) - ref.rgba[:, :3])[compared].max() <= 1e-3
    assert np.abs(_host(hard) - hard64)[compared].max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 9. the example

def test_example_soft_cubes_runs():
    """examples/example_soft_cubes.py as a child process with 30 steps: it exits 0 and its last printed loss is below its
    first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_soft_cubes.py'), '30'], cwd=root, env=env,
                         capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('soft cubes step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
