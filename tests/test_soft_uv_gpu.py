"""`-m gpu`: the soft colour kernels with UV texture images (csrc/nr_soft_render.hip, the nr_soft_uv_* entries), soft_render_uv
and Renderer.render_soft(per_pixel=True) with a UVImages.

rgba, grad_faces, grad_images and grad_light against the float64 restatement of tests/soft_uv_ref.py under its derived bounds,
on the geometry and (S, sigma, gamma) of tests/test_soft_render_gpu.py's cases; a ramp image against the corner-colour
kernels; shared images and light; reproducibility; the tensor boundary and a side stream; dropped, zero-area and image-less
faces; the renderer end to end, against soft_render_uv of the composition and against the hard rasterizer; the example.
"Bit for bit" is torch.equal; grad_images is a double sum rounded once whose additions arrive in no fixed order, and is
compared within one float32 ulp where the others are compared bit for bit.  The cases and their references are also read by
tests/test_soft_uv.py (CPU: the caps and the sensitivity of the bounds).

No stream-capture test: two capture sequences on this project have ended in a host segmentation fault inside torch (DESIGN
"Soft silhouettes", Stream capture); capture before any eager backward on the same leaves.

Worst ratios measured on the MI355X: see DESIGN "Soft colour rendering", UV images (every case prints its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import soft_render_ref as R0
import soft_uv_ref as R
import test_soft_render_gpu as G0
from test_soft_render_gpu import BG, _cuda, _faces, _host

pytestmark = pytest.mark.gpu

# both 'mix' geometries at B = 2 and the one at B = 1 (F = 330: a chunk and a tail; dropped and zero-area faces; S = 20 a
# clipped tile), and one sphere per sigma; B = 3 runs with images shared by the batch, B = 2 with images per render
_ICO = [('ico1', 3, 20, 1e-6, 1e-1), ('ico1', 3, 32, 1e-3, 1e-4), ('ico1', 3, 16, 1.0, 1e-1), ('ico1', 3, 20, 1e-3, 1e-1)]
CASES = [c for c in G0.CASES if c[0] == 'mix' or c in _ICO]
IDS = ['%s-B%d-S%d-sigma%g-gamma%g' % c for c in CASES]
SIZES = [(7, 5), (4, 9), (1, 1), (1, 6)]   # (H, W) of the four images
TS = 2
# the float32 allowance of the comparison with the hard rasterizer: the worst difference MEASURED on the MI355X beyond the
# float64 difference of the two definitions (the test prints it; DESIGN "Soft colour rendering", UV images); 4 times it is
# asserted.  The two kernels form the weights as w_k (zp / z_k) and as (lambda_k / z_k) zp: a few ulp of pos times the
# image's slope (an 8 x 9 image: pos up to 8, texels in [0, 1]).  Measured: 1.699e-6
HARD_ALLOWANCE = 1.699e-6

_cache = {}


def make_layout(F, seed, every_face=False):
    """(nr-side arguments, the restatement's Layout): four images of SIZES; a tenth of the faces without an image and a
    non-constant base; uv uniform in (0.05, 0.95), a few faces in [-0.3, 1.4] (the index clamp).  every_face: all faces
    with an image."""
    rng = np.random.default_rng(seed)
    face_image = rng.integers(0, len(SIZES), F).astype(np.int32)
    faces_uv = rng.uniform(0.05, 0.95, (F, 3, 2)).astype(np.float32)
    base = rng.uniform(0, 1, (F, TS, TS, TS, 3)).astype(np.float32)
    if not every_face:
        order = rng.permutation(F)
        face_image[order[:max(1, F // 10)]] = -1
        wild = order[-4:]
        faces_uv[wild] = rng.uniform(-0.3, 1.4, (len(wild), 3, 2)).astype(np.float32)
        face_image[wild] = np.arange(len(wild)) % 2                          # (on the two larger images)
    return (faces_uv, face_image, base, SIZES), R.Layout(faces_uv, face_image, base, SIZES)


def make_images(rng, batch):
    """The four images, [H,W,3] (batch None) or [batch,H,W,3], uniform in [0, 1] -> (list, packed [Bi,Pn,3])."""
    lead = () if batch is None else (batch,)
    images = [rng.uniform(0, 1, lead + (h, w, 3)).astype(np.float32) for h, w in SIZES]
    return images, pack(images)


def pack(images):
    Bi = images[0].shape[0] if images[0].ndim == 4 else 1
    return np.concatenate([im.reshape(Bi, -1, 3) for im in images], 1)


def reference(mesh, B, S, sigma, gamma, adds=None):
    """(faces, nr-side layout arguments, images, light, the restatement's Result -- with .g, the upstream gradient, 0 on the
    masked pixels): once per case.  B = 3: images shared by the batch; otherwise one set per render."""
    key = (mesh, B, S, sigma, gamma, adds)
    if key not in _cache:
        faces = _faces(mesh, B)
        F = faces.shape[1]
        rng = np.random.default_rng(B * 1000 + S + 13)
        args, lay = make_layout(F, F + S)
        images, packed = make_images(rng, None if B == 3 else B)
        light = rng.uniform(0.5, 1.5, (B, F, 3)).astype(np.float32)
        g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
        ref = R.restate(faces, lay, packed, light, S, sigma, gamma, background=BG, g=g, adds=adds)
        _cache[key] = (faces, args, images, light, ref)
    return _cache[key]


def _uv(args, images, grad=True):
    import neural_renderer_amd as nr
    key = ('layout', id(args))
    if key not in _cache:
        _cache[key] = (args, nr.UVLayout(*args))                             # (args kept alive: its id is the key)
    xs = [_cuda(im, grad) for im in images]
    return xs, nr.UVImages(_cache[key][1], xs)


def _run(faces, args, images, light, g, S, sigma, gamma, implementation='hip'):
    """-> rgba, grad_faces, grad_light, [grad of every image]."""
    import neural_renderer_amd as nr
    ft, lt = _cuda(faces, True), _cuda(light, True)
    xs, uv = _uv(args, images)
    rgba = nr.soft_render_uv(ft, uv, lt, S, sigma, gamma, background_color=BG, implementation=implementation)
    rgba.backward(_cuda(np.asarray(g, np.float32)))
    return rgba.detach(), ft.grad, lt.grad, [x.grad for x in xs]


def _packed_grad(grads):
    return pack([_host(x) for x in grads])


def _within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement's bounds

@pytest.mark.parametrize('mesh,B,S,sigma,gamma', CASES, ids=IDS)
def test_forward_and_gradients_within_the_derived_bounds(mesh, B, S, sigma, gamma):
    """rgba (outside the masked pixels), grad_faces, grad_images and grad_light from random upstream gradients (0 on the
    masked pixels) within the per-entry bounds of soft_uv_ref (its docstring); the caps."""
    faces, args, images, light, ref = reference(mesh, B, S, sigma, gamma)
    rgba, gf, gl, gi = _run(faces, args, images, light, ref.g, S, sigma, gamma)
    assert tuple(rgba.shape) == (B, 4, S, S) and tuple(gf.shape) == faces.shape and tuple(gl.shape) == light.shape
    assert [tuple(x.shape) for x in gi] == [im.shape for im in images]
    rr = R.masked_ratio(_host(rgba), ref.rgba, ref.rgba_bound, ref.mask)
    rf = R.worst_ratio(_host(gf), ref.grad_faces, ref.grad_faces_bound)
    rl = R.worst_ratio(_host(gl), ref.grad_light, ref.grad_light_bound)
    if B == 3:
        total, _, bound = R.shared(ref, 'grad_images')
    else:
        total, bound = ref.grad_images, ref.grad_images_bound
    ri = R.worst_ratio(_packed_grad(gi), total, bound)
    print('%s B=%d S=%d sigma=%g gamma=%g: rgba %.3f, grad_faces %.3f, grad_images %.3f, grad_light %.3f of the bound; masked '
          '%.2f %% of the pixels with a pair, segment doubt %.2f %%, texel doubt %.2f %% of %d pairs'
          % (mesh, B, S, sigma, gamma, rr, rf, ri, rl, 100 * ref.masked_share, 100 * ref.doubt_share,
             100 * ref.texel_doubt_share, sum(ref.pairs)))
    assert ref.masked_share <= 0.01 and ref.doubt_share <= 0.02 and ref.texel_doubt_share <= 0.01
    assert rr <= 1 and rf <= 1 and ri <= 1 and rl <= 1, (rr, rf, ri, rl)
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_light).max() > 0
    off, h, w = R.Layout(*args).table[2]
    assert (h, w) == (1, 1) and np.abs(total[:, off]).max() > 0 and gi[2].abs().max() > 0       # the 1 x 1 image
    assert all(torch.isfinite(x).all() for x in [rgba, gf, gl] + gi)
    assert gf[..., 2].abs().max() > 0 and all(x.abs().max() > 0 for x in gi)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a ramp image: the corner-colour kernels

@pytest.mark.parametrize('case', [('mix', 2, 20, 1e-3, 1e-1), ('ico1', 3, 32, 1e-3, 1e-4)])
def test_a_ramp_image_against_the_corner_kernels(case):
    """I = a + b col + c row_from_bottom, uv strictly inside (0, 1): a bilinear read of an affine image is affine in uv and
    sum mu_k = 1, so the definition equals soft_render with corner colours L_f ramp(uv_fk).  Every number is a short dyadic
    fraction, so the corner colours are exact in float32.  rgba, grad_faces and grad_light (against the corner gradient
    contracted with ramp(uv_fk)) within the sum of the two restatements' bounds."""
    import neural_renderer_amd as nr
    mesh, B, S, sigma, gamma = case
    faces = _faces(mesh, B)
    F = faces.shape[1]
    rng = np.random.default_rng(F + S)
    face_image = rng.integers(0, len(SIZES), F).astype(np.int32)
    faces_uv = ((2 * rng.integers(2, 30, (F, 3, 2)) + 1) / 64.0).astype(np.float32)          # odd k / 64: no pos on the lattice
    base = np.zeros((F, TS, TS, TS, 3), np.float32)
    args, lay = (faces_uv, face_image, base, SIZES), R.Layout(faces_uv, face_image, base, SIZES)
    coef = rng.integers(1, 8, (len(SIZES), 3, 3)) / 16.0                                      # (image, channel, (a, b, c))
    images = []
    for (h, w), k in zip(SIZES, coef):
        col, row = np.arange(w)[None, :, None], (h - 1 - np.arange(h))[:, None, None]         # stored top row first
        images.append((k[None, None, :, 0] + k[None, None, :, 1] * col + k[None, None, :, 2] * row).astype(np.float32))
    light = (rng.integers(2, 6, (B, F, 3)) / 4.0).astype(np.float32)
    hw = np.array(SIZES, np.float64)[face_image]                                              # [F,2]: H, W
    k = coef[face_image]                                                                      # [F,3,3]
    ramp = (k[:, None, :, 0] + k[:, None, :, 1] * (faces_uv[:, :, None, 0] * (hw[:, None, None, 1] - 1))
            + k[:, None, :, 2] * (faces_uv[:, :, None, 1] * (hw[:, None, None, 0] - 1)))      # [F,corner,rgb]
    corner = (light[:, :, None, :] * ramp[None]).astype(np.float32)
    assert np.array_equal(corner.astype(np.float64), light[:, :, None, :].astype(np.float64) * ramp[None])   # exact
    g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
    ref_u = R.restate(faces, lay, pack(images), light, S, sigma, gamma, background=BG, g=g)
    ref_c = R0.restate(faces, corner, S, sigma, gamma, background=BG, g=ref_u.g)
    assert np.array_equal(ref_c.mask, ref_u.mask) and np.array_equal(ref_c.g, ref_u.g)
    a, af, al, _ = _run(faces, args, images, light, ref_u.g, S, sigma, gamma)
    ft, ct = _cuda(faces, True), _cuda(corner, True)
    b = nr.soft_render(ft, ct, S, sigma, gamma, background_color=BG, implementation='hip')
    b.backward(_cuda(np.asarray(ref_u.g, np.float32)))
    keep = ~np.broadcast_to(ref_u.mask[:, None], ref_u.rgba.shape)
    rr = R.worst_ratio(_host(a)[keep], _host(b).astype(np.float64)[keep], (ref_u.rgba_bound + ref_c.rgba_bound)[keep])
    rf = R.worst_ratio(_host(af), _host(ft.grad).astype(np.float64), ref_u.grad_faces_bound + ref_c.grad_faces_bound)
    # dL/dL_fc = sum_k dL/dC_fkc ramp_fkc
    bl = (_host(ct.grad).astype(np.float64) * ramp[None]).sum(2)
    rl = R.worst_ratio(_host(al), bl, ref_u.grad_light_bound + (ref_c.grad_colors_bound * np.abs(ramp[None])).sum(2))
    print('%s ramp image against corner colours: rgba %.3f, grad_faces %.3f, grad_light %.3f of the two bounds' % (mesh, rr, rf, rl))
    assert rr <= 1 and rf <= 1 and rl <= 1, (rr, rf, rl)
    assert af.abs().sum() > 0 and al.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. shared images and shared light

def test_shared_images_and_shared_light():
    """Images [H,W,3] and light [1,F,3] beside B = 3: rgba and grad_faces have the bits of the expanded call; the shared
    gradients agree with the float64 sum over the batch within its bound."""
    S, sigma, gamma = 20, 1e-3, 1e-1
    faces = _faces('ico1', 3)
    F = faces.shape[1]
    rng = np.random.default_rng(17)
    args, lay = make_layout(F, 5)
    images, packed = make_images(rng, None)
    light = rng.uniform(0.5, 1.5, (1, F, 3)).astype(np.float32)
    g = rng.normal(size=(3, 4, S, S)).astype(np.float32)
    ref = R.restate(faces, lay, packed, light, S, sigma, gamma, background=BG, g=g)
    assert ref.masked_share <= 0.01
    rgba, gf, gl, gi = _run(faces, args, images, light, ref.g, S, sigma, gamma)
    wide = [np.ascontiguousarray(np.repeat(im[None], 3, 0)) for im in images]
    rgba_w, gf_w, gl_w, gi_w = _run(faces, args, wide, np.repeat(light, 3, 0), ref.g, S, sigma, gamma)
    assert tuple(gl.shape) == (1, F, 3) and tuple(gl_w.shape) == (3, F, 3)
    assert [tuple(x.shape) for x in gi] == [im.shape for im in images] and [tuple(x.shape) for x in gi_w] == [im.shape for im in wide]
    assert torch.equal(rgba, rgba_w) and torch.equal(gf, gf_w)
    ti, _, bi = R.shared(ref, 'grad_images')
    tl, _, bl = R.shared(ref, 'grad_light')
    ri, rl = R.worst_ratio(_packed_grad(gi), ti, bi), R.worst_ratio(_host(gl), tl, bl)
    rw = R.worst_ratio(_packed_grad(gi_w), ref.grad_images, ref.grad_images_bound)
    print('shared images and light: grad_images %.3f (per render %.3f), grad_light %.3f of the bound' % (ri, rw, rl))
    assert ri <= 1 and rl <= 1 and rw <= 1 and np.abs(ti).max() > 0 and np.abs(tl).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. reproducibility

@pytest.mark.parametrize('case', [('mix', 2, 32, 1e-3, 1e-4), ('ico1', 3, 20, 1e-3, 1e-1)])
def test_two_runs_and_an_image_alone(case):
    """rgba, grad_faces and grad_light: the same bits in two runs and for an image alone; grad_images of two runs within
    one float32 ulp (the double sums differ by less than a float rounding)."""
    mesh, B, S, sigma, gamma = case
    faces, args, images, light, ref = reference(*case)
    a0 = _run(faces, args, images, light, ref.g, S, sigma, gamma)
    a1 = _run(faces, args, images, light, ref.g, S, sigma, gamma)
    assert all(torch.equal(x, y) for x, y in zip(a0[:3], a1[:3])) and a0[1].abs().sum() > 0 and a0[2].abs().sum() > 0
    assert all(_within_one_ulp(_host(x), _host(y)) for x, y in zip(a0[3], a1[3])) and all(x.abs().sum() > 0 for x in a0[3])
    for b in range(B):
        own = [im if im.ndim == 3 else im[b:b + 1] for im in images]
        one = _run(faces[b:b + 1], args, own, light[b:b + 1], ref.g[b:b + 1], S, sigma, gamma)
        assert all(torch.equal(x[0], y[b]) for x, y in zip(one[:3], a0[:3])), b


# ---------------------------------------------------------------------------------------------------------------------
# 5. the tensor boundary

def test_layouts_alignment_and_a_side_stream():
    """faces, light, the images and the upstream gradient as a strided view, as views 4 / 8 / 12 bytes off the 16-byte grid
    and permuted, and one call on a side stream: the fixed-order outputs have the bits of the dense call, grad_images
    agrees within one ulp."""
    import neural_renderer_amd as nr
    from test_layout_invariance_gpu import FLOAT_LAYOUTS, grad_as, lay
    case = ('ico1', 3, 20, 1e-3, 1e-1)
    S, sigma, gamma = case[2:]
    faces, args, images, light, ref = reference(*case)
    gt = _cuda(np.asarray(ref.g, np.float32))
    ref_a, ref_f, ref_l, ref_i = _run(faces, args, images, light, ref.g, S, sigma, gamma)
    assert ref_a.abs().sum() > 0 and ref_f.abs().sum() > 0 and ref_l.abs().sum() > 0
    layout = _uv(args, images)[1].layout
    for fl in FLOAT_LAYOUTS:
        for gl in ('plain', fl):
            lf, ll = lay(_cuda(faces), fl).requires_grad_(True), lay(_cuda(light), fl).requires_grad_(True)
            xs = [lay(_cuda(im), fl).requires_grad_(True) for im in images]
            out = nr.soft_render_uv(lf, nr.UVImages(layout, xs), ll, S, sigma, gamma, background_color=BG, implementation='hip')
            assert torch.equal(out.detach(), ref_a), fl
            grad_as(out, gl).backward(gt)
            assert torch.equal(lf.grad, ref_f) and torch.equal(ll.grad, ref_l), (fl, gl)
            assert all(_within_one_ulp(_host(x.grad), _host(y)) for x, y in zip(xs, ref_i)), (fl, gl)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    lf, ll = _cuda(faces, True), _cuda(light, True)
    xs, uv = _uv(args, images)
    with torch.cuda.stream(side):
        out = nr.soft_render_uv(lf, uv, ll, S, sigma, gamma, background_color=BG, implementation='hip')
        out.backward(gt)
    side.synchronize()
    assert torch.equal(out.detach(), ref_a) and torch.equal(lf.grad, ref_f) and torch.equal(ll.grad, ref_l)
    assert all(_within_one_ulp(_host(x.grad), _host(y)) for x, y in zip(xs, ref_i))


# ---------------------------------------------------------------------------------------------------------------------
# 6. dropped, zero-area and image-less faces

def test_dropped_and_zero_area_faces():
    """The mixed case: the four dropped and the two zero-area faces get exactly 0 in grad_faces and grad_light and add
    nothing to grad_images -- the call without them gives the same rgba bits and the same image gradient (one ulp)."""
    case = ('mix', 2, 20, 1e-3, 1e-1)
    mesh, B, S, sigma, gamma = case
    faces, args, images, light, ref = reference(*case)
    f64 = faces.astype(np.float64)
    with np.errstate(all='ignore'):
        area = (f64[:, :, 1, 0] - f64[:, :, 0, 0]) * (f64[:, :, 2, 1] - f64[:, :, 0, 1]) \
            - (f64[:, :, 2, 0] - f64[:, :, 0, 0]) * (f64[:, :, 1, 1] - f64[:, :, 0, 1])
        off = ~(np.isfinite(f64).all((2, 3)) & (f64[..., 2] >= 0.1).all(2) & (f64[..., 2] <= 100).all(2) & (area != 0))
    assert (off.sum(1) == 6).all() and np.array_equal(off[0], off[1])
    rgba, gf, gl, gi = _run(faces, args, images, light, ref.g, S, sigma, gamma)
    assert (_host(gf)[off] == 0).all() and (_host(gl)[off] == 0).all()
    keep = ~off[0]
    faces_uv, face_image, base, sizes = args
    less = (faces_uv[keep], face_image[keep], base[keep], sizes)
    rgba2, gf2, gl2, gi2 = _run(faces[:, keep], less, images, light[:, keep], ref.g, S, sigma, gamma)
    assert torch.equal(rgba, rgba2) and torch.equal(gf[:, keep], gf2) and torch.equal(gl[:, keep], gl2)
    assert all(_within_one_ulp(_host(x), _host(y)) for x, y in zip(gi, gi2))


def test_a_face_without_an_image_shows_the_mean_of_its_base():
    """One large face in front, no image, a hard depth order: the covered centre shows L * mean(base), within the roundings
    of L T, w C and the division (4 u)."""
    import neural_renderer_amd as nr
    S = 16
    faces = np.array([[[[-0.9, -0.8, 1.0], [0.9, -0.7, 1.2], [0.1, 0.9, 1.1]]]], np.float32)
    rng = np.random.default_rng(3)
    base = rng.uniform(0, 1, (1, TS, TS, TS, 3)).astype(np.float32)
    args = (rng.uniform(0.1, 0.9, (1, 3, 2)).astype(np.float32), np.array([-1], np.int32), base, [(3, 4)])
    image = _cuda(rng.uniform(0, 1, (3, 4, 3)).astype(np.float32), True)
    light = np.array([[[0.7, 1.1, 0.4]]], np.float32)
    lt = _cuda(light, True)
    out = nr.soft_render_uv(_cuda(faces), nr.UVImages(nr.UVLayout(*args), [image]), lt, S, 1e-6, 1e-4,
                            background_color=BG, implementation='hip')
    want = light[0, 0].astype(np.float64) * base.reshape(-1, 3).astype(np.float64).mean(0).astype(np.float32)
    got = _host(out)[0, :3, 8, 8].astype(np.float64)
    assert _host(out)[0, 3, 8, 8] > 0.99 and (np.abs(got - want) <= 4 * 2.0 ** -24 * np.abs(want)).all(), (got, want)
    out.sum().backward()
    assert image.grad.abs().max() == 0 and lt.grad.abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. through the renderer

def _sphere_scene(B=2):
    import neural_renderer_amd as nr
    v, f = nr.icosphere(2, 0.8)
    return v[None].repeat(B, 1, 1).cuda(), f[None].repeat(B, 1, 1).cuda()


@pytest.mark.parametrize('lights', [False, True])
def test_render_soft_per_pixel_is_the_composition(lights):
    """Bit-equal to soft_render_uv(the front copies of the front-end's faces, the UVImages, the per-face light of the front
    copies that render() hands its rasterizer); `lights` are honoured."""
    import neural_renderer_amd as nr
    vertices, faces = _sphere_scene()
    F = faces.shape[1]
    args, _ = make_layout(F, 21)
    images, _ = make_images(np.random.default_rng(22), None)
    _, uv = _uv(args, images, grad=False)
    r = nr.Renderer()
    r.image_size, r.eye = 32, nr.get_points_from_angles(2.732, 25, 40)
    r.soft_gamma, r.background_color = 1e-2, list(BG)
    if lights:
        r.lights = nr.Lights(sh=0.1 * torch.randn(9, 3)).cuda()
    img = r.render_soft(vertices, faces, uv, per_pixel=True)
    proj, same, kw = r._shade(vertices, faces, uv)
    assert proj.shape[1] == 2 * F and same is uv and tuple(kw['face_light'].shape) == (2, 2 * F, 3)
    want = nr.soft_render_uv(proj[:, :F], uv, kw['face_light'][:, :F], 32, r.soft_sigma, 1e-2, r.near, r.far, r.soft_eps, BG)
    assert img.shape == (2, 4, 32, 32) and torch.equal(img, want) and img[:, :3].abs().sum() > 0
    if lights:
        plain = nr.Renderer()
        plain.image_size, plain.eye, plain.soft_gamma, plain.background_color = 32, r.eye, 1e-2, list(BG)
        assert not torch.equal(img, plain.render_soft(vertices, faces, uv, per_pixel=True))


def test_render_soft_per_pixel_gradients_on_the_gpu():
    """Gradients reach the vertices (z included), every image and a learnable eye."""
    import neural_renderer_amd as nr
    vertices, faces = _sphere_scene(1)
    vertices.requires_grad_(True)
    F = faces.shape[1]
    args, _ = make_layout(F, 23, every_face=True)
    images, _ = make_images(np.random.default_rng(24), None)
    xs, uv = _uv(args, images)
    r = nr.Renderer()
    r.image_size = 32
    r.eye = torch.tensor(nr.get_points_from_angles(2.732, 25, 40), dtype=torch.float32, device='cuda', requires_grad=True)
    r.soft_sigma, r.soft_gamma = 1e-3, 1e-2
    w = torch.randn(1, 4, 32, 32, device='cuda')
    (r.render_soft(vertices, faces, uv, per_pixel=True) * w).sum().backward()
    assert torch.isfinite(vertices.grad).all() and vertices.grad[..., 2].abs().sum() > 0
    assert all(torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0 for x in xs)
    assert torch.isfinite(r.eye.grad).all() and r.eye.grad.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. the hard rasterizer

def test_render_soft_per_pixel_against_the_hard_rasterizer():
    """The strongly tilted quad of test_soft_corners_gpu.py with one 8 x 9 image, ambient light only: render() without
    anti-aliasing and render_soft(per_pixel=True) with sigma = 1e-8, gamma = 1e-4 on the pixels farther than sqrt(30 sigma) from
    every edge, for the same UVImages.  Tolerance per pixel: the float64 difference of the two definitions there (computed
    here from the projected faces) plus 4 x the float32 allowance measured on the MI355X, never above 1e-3."""
    import neural_renderer_amd as nr
    S, sigma, gamma = 32, 1e-8, 1e-4
    vertices = torch.tensor([[[-0.93, -0.71, -0.83], [0.91, -0.69, -0.79], [0.89, 0.73, 0.91], [-0.87, 0.67, 0.88]]], device='cuda')
    faces = torch.tensor([[[0, 1, 2], [0, 2, 3]]], dtype=torch.int32, device='cuda')
    rng = np.random.default_rng(31)
    faces_uv = np.array([[[0.07, 0.11], [0.93, 0.09], [0.91, 0.94]], [[0.07, 0.11], [0.91, 0.94], [0.06, 0.89]]], np.float32)
    args = (faces_uv, np.zeros(2, np.int32), np.zeros((2, TS, TS, TS, 3), np.float32), [(8, 9)])
    image = rng.uniform(0, 1, (8, 9, 3)).astype(np.float32)
    lay = R.Layout(*args)
    uv = nr.UVImages(nr.UVLayout(*args), [_cuda(image)])
    r = nr.Renderer()
    r.image_size, r.anti_aliasing, r.background_color = S, False, list(BG)
    r.light_intensity_ambient, r.light_intensity_directional = 1.0, 0.0
    hard = r.render(vertices, faces, uv)
    soft = r.render_soft(vertices, faces, uv, sigma=sigma, gamma=gamma, per_pixel=True)
    assert hard.shape == (1, 3, S, S) and soft.shape == (1, 4, S, S)
    proj, _, kw = r._shade(vertices, faces, uv)
    pf, pl = _host(proj[:, :2]).astype(np.float64), _host(kw['face_light'][:, :2]).astype(np.float64)
    ref = R.restate(pf, lay, pack([image]), pl, S, sigma, gamma, r.near, r.far, r.soft_eps, BG)
    hard64 = R.hard_image(pf, lay, pack([image]), pl, S, BG)
    compared = np.broadcast_to((ref.edge_d2 > 30 * sigma)[:, None], hard64.shape)
    covered = compared & np.broadcast_to((ref.rgba[:, 3:] > 0.5), hard64.shape)
    assert covered.sum() >= 3 * 100 and (compared & ~covered).sum() >= 3 * 100          # the quad and the background
    definitions = np.abs(ref.rgba[:, :3] - hard64)
    got = np.abs(_host(soft[:, :3]).astype(np.float64) - _host(hard).astype(np.float64))
    beyond = (got - definitions)[compared].max()
    print('render_soft(per_pixel, UVImages) against render: worst difference %.3e, of the two definitions in float64 %.3e, '
          'beyond it %.3e on %d compared values' % (got[compared].max(), definitions[compared].max(), beyond, compared.sum()))
    assert 4 * HARD_ALLOWANCE <= 1e-3
    assert beyond <= 4 * HARD_ALLOWANCE
    # ... and each against its own float64 definition
    assert np.abs(_host(soft[:, :3]) - ref.rgba[:, :3])[compared].max() <= 1e-3
    assert np.abs(_host(hard) - hard64)[compared].max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 9. the example

def test_example_soft_uv_runs():
    """examples/example_soft_uv.py as a child process with 30 steps: it exits 0 and its last printed loss is below its
    first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_soft_uv.py'), '30'], cwd=root, env=env,
                         capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('soft uv step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
