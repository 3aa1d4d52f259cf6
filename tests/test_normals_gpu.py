"""`-m gpu`: the normal kernels (csrc/nr_normals.hip) and Renderer.render_normals.

The normals are pinned bit for bit against the kernels that already hold them (vertex_light with a unit light along an
axis), against the float64 restatement of tests/normals_ref.py under its derived bounds, on degenerate input, for
reproducibility, across tensor layouts, through the renderer, inside a captured graph and in the example.  "Bit for bit"
is torch.equal / np.array_equal: the two zeros compare equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import normals_ref as R
import vertex_ref as VR

pytestmark = pytest.mark.gpu

NAMES = sorted(R.meshes())
# (mesh, batch size, an index tensor [B,Nf,3] with another topology per image)
CASES = [(n, B, False) for n in NAMES for B in (1, 3)] + [(n, 3, True) for n in ('grid3', 'fan12', 'icosphere1', 'degenerate')]
IDS = ['%s-B%d%s' % (n, B, '-per_image' if p else '') for n, B, p in CASES]


def _cuda(a, grad=False):
    a = np.ascontiguousarray(a)
    return torch.tensor(a, device='cuda', requires_grad=bool(grad) and a.dtype.kind == 'f')


def _host(t):
    return t.detach().cpu().numpy()


def _ops(smooth_fill=((False, False), (False, True), (True, False), (True, True))):
    """name -> f(vertices, faces) for the three operators (corner normals in every mode), HIP path."""
    import neural_renderer_amd as nr
    ops = {'vertex': lambda v, f: nr.vertex_normals(v, f, implementation='hip'),
           'face': lambda v, f: nr.face_normals(v, f, implementation='hip')}
    for smooth, fill_back in smooth_fill:
        ops['corner-%s-%s' % ('smooth' if smooth else 'flat', 'fill_back' if fill_back else 'front')] = \
            (lambda v, f, s=smooth, fb=fill_back: nr.corner_normals(v, f, smooth=s, fill_back=fb, implementation='hip').colors)
    return ops


def _mode(name):
    """op name -> (what, smooth, fill_back) of normals_ref."""
    p = name.split('-')
    return (p[0], False, False) if len(p) == 1 else ('corner', p[1] == 'smooth', p[2] == 'fill_back')


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels that already hold these normals

def _light_normals(vt, ft, smooth):
    """[B,Nf,3(corner),3(xyz)] from vertex_light: with no ambient light, a white directional light of intensity 1 along +-e_c
    and white colours the light at a corner is max(+-n[c], 0), so light(+e_c) - light(-e_c) = n[c] exactly."""
    import neural_renderer_amd as nr
    kw = dict(intensity_ambient=0, intensity_directional=1, color_ambient=(1, 1, 1), color_directional=(1, 1, 1),
              fill_back=False, smooth=smooth, implementation='hip')
    out = []
    for c in range(3):
        e = [0.0, 0.0, 0.0]
        e[c] = 1.0
        plus = nr.vertex_light(vt, ft, direction=list(e), **kw)
        e[c] = -1.0
        minus = nr.vertex_light(vt, ft, direction=list(e), **kw)
        assert torch.equal(plus[..., 0], plus[..., 1]) and torch.equal(plus[..., 0], plus[..., 2])
        out.append(plus[..., 0] - minus[..., 0])
    return torch.stack(out, dim=-1)


@pytest.mark.parametrize('name,B,per_image', CASES, ids=IDS)
def test_bit_equal_to_the_normals_inside_vertex_light(name, B, per_image):
    import neural_renderer_amd as nr
    v, f = R.batch(name, B, per_image_topology=per_image)
    vt, ft = _cuda(v), _cuda(f)
    flat, smooth = _light_normals(vt, ft, False), _light_normals(vt, ft, True)
    assert flat.abs().sum() > 0 and smooth.abs().sum() > 0
    assert torch.equal(nr.corner_normals(vt, ft, smooth=False, fill_back=False, implementation='hip').colors, flat)
    assert torch.equal(nr.corner_normals(vt, ft, smooth=True, fill_back=False, implementation='hip').colors, smooth)
    assert torch.equal(nr.face_normals(vt, ft, implementation='hip'), flat[:, :, 0])
    idx = (ft if ft.dim() == 3 else ft[None].expand(B, -1, -1)).long()
    want = torch.zeros_like(vt)    # a vertex without a face: 0
    want[torch.arange(B, device='cuda')[:, None, None], idx] = smooth   # (every corner at a vertex holds the same bits)
    assert torch.equal(want[torch.arange(B, device='cuda')[:, None, None], idx], smooth)
    assert torch.equal(nr.vertex_normals(vt, ft, implementation='hip'), want)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the restatement's bounds

@pytest.mark.parametrize('name,B,per_image', CASES, ids=IDS)
def test_forward_and_backward_within_the_derived_bounds(name, B, per_image):
    """Forward against the float64 restatement under gamma_k * magnitude, backward from random gradients against the float64
    adjoint under gamma_(24 + 3 deg) * magnitude (normals_ref's docstring; equality where a magnitude is 0).
    Measured on the MI355X: see the figures printed here and DESIGN "Normal maps"."""
    v, f = R.batch(name, B, per_image_topology=per_image)
    Nv = v.shape[1]
    rng = np.random.default_rng(31)
    fm, vm = R.forward_mag(v, f)
    kb = R.backward_k(f, Nv, B)
    worst_f, worst_b = 0.0, 0.0
    for op_name, op in _ops().items():
        what, smooth, fill_back = _mode(op_name)
        vt, ft = _cuda(v, True), _cuda(f)
        out = op(vt, ft)
        if what == 'vertex':
            ref, bound = R.vertex_normals(v, f), R.gamma(R.forward_k(f, Nv, 'vertex', B)) * vm
        elif what == 'face':
            ref, bound = R.face_normals(v, f), R.gamma(R.forward_k(f, Nv, 'face')) * fm
        else:
            ref = R.corner_normals(v, f, smooth, fill_back)
            bound = R.gamma(R.corner_k(f, Nv, smooth, fill_back, B)) * R.corner_mag(v, f, smooth, fill_back)
        assert tuple(out.shape) == ref.shape
        rf = R.worst_ratio(_host(out), ref, bound)
        g = rng.normal(size=ref.shape).astype(np.float32)
        out.backward(_cuda(g))
        gv, gv_mag = R.adjoint64(v, f, g, what, smooth, fill_back)
        rb = R.worst_ratio(_host(vt.grad), gv, R.gamma(kb) * gv_mag)
        print('%s %s: forward %.3f, backward %.3f of the bound' % (name, op_name, rf, rb))
        assert rf <= 1 and rb <= 1, (op_name, rf, rb)
        assert name == 'degenerate' or np.abs(gv).max() > 0
        worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
    print('%s B=%d per_image=%s: worst forward %.3f, worst backward %.3f of the bounds' % (name, B, per_image, worst_f, worst_b))


# ---------------------------------------------------------------------------------------------------------------------
# 3. degenerate input

def test_degenerate_pins():
    """The zero-area face (last) and the vertex without a face (9): exact zeros forward, finite gradients, and exactly 0
    for the isolated vertex."""
    v, f = R.batch('degenerate', 3)
    rng = np.random.default_rng(8)
    for op_name, op in _ops().items():
        what, smooth, fill_back = _mode(op_name)
        vt, ft = _cuda(v, True), _cuda(f)
        out = op(vt, ft)
        Nf = len(f)
        if what == 'vertex':
            assert not out[:, 9].any() and out[:, :9].abs().sum() > 0
        elif what == 'face':
            assert not out[:, -1].any()
        elif not smooth:
            assert not out[:, Nf - 1].any() and (not fill_back or not out[:, 2 * Nf - 1].any())
        out.backward(_cuda(rng.normal(size=tuple(out.shape)).astype(np.float32)))
        assert torch.isfinite(vt.grad).all() and vt.grad.abs().sum() > 0
        assert not vt.grad[:, 9].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. reproducibility

@pytest.mark.parametrize('name,per_image', [('icosphere3', False), ('fan12', True), ('degenerate', True)])
def test_two_runs_and_an_image_alone_give_the_same_bits(name, per_image):
    B = 3
    v, f = R.batch(name, B, per_image_topology=per_image)
    rng = np.random.default_rng(2)
    for op_name, op in _ops().items():
        runs = []
        for _ in range(2):
            vt = _cuda(v, True)
            out = op(vt, _cuda(f))
            g = rng.normal(size=tuple(out.shape)).astype(np.float32) if not runs else g
            out.backward(_cuda(g))
            runs.append((out.detach(), vt.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), op_name
        for b in range(B):
            vt = _cuda(v[b:b + 1], True)
            out = op(vt, _cuda(f[b:b + 1] if per_image else f))
            out.backward(_cuda(g[b:b + 1]))
            assert torch.equal(out.detach()[0], runs[0][0][b]) and torch.equal(vt.grad[0], runs[0][1][b]), (op_name, b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. fill_back

@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('name', ['icosphere1', 'fan12', 'degenerate'])
def test_fill_back_relation_and_gradient(name, smooth):
    import neural_renderer_amd as nr
    v, f = R.batch(name, 3)
    Nf = len(f)
    rng = np.random.default_rng(6)
    vt, ft = _cuda(v, True), _cuda(f)
    c = nr.corner_normals(vt, ft, smooth=smooth, fill_back=True, implementation='hip').colors
    assert c.shape == (3, 2 * Nf, 3, 3)
    assert torch.equal(c[:, Nf:], -c[:, :Nf].flip(2))
    g = _cuda(rng.normal(size=tuple(c.shape)).astype(np.float32))
    c.backward(g)
    v2 = _cuda(v, True)
    c2 = nr.corner_normals(v2, ft, smooth=smooth, fill_back=False, implementation='hip').colors
    assert torch.equal(c2, c[:, :Nf])
    c2.backward(g[:, :Nf] - g[:, Nf:].flip(2))
    assert vt.grad.abs().sum() > 0 and torch.equal(vt.grad, v2.grad)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tensor boundary

@pytest.mark.parametrize('per_image', [False, True])
def test_layouts_alignment_and_a_side_stream(per_image):
    """The contract of tests/test_layout_invariance_gpu.py for the three operators: vertices as offset-4/8/12, strided,
    permuted and expanded views, faces as int64 and as a non-contiguous view, upstream gradients in those layouts and the
    stride-0 gradient of sum(): the bits of the dense call.  One call on a side stream."""
    from test_layout_invariance_gpu import FLOAT_LAYOUTS, grad_as, lay
    B = 3
    v, f = R.batch('icosphere1', B, per_image_topology=per_image)
    v[:] = v[0:1]   # (all images equal: `expanded` applies)
    rng = np.random.default_rng(12)
    for op_name, op in _ops(((False, True), (True, True))).items():
        base = _cuda(v, True)
        out = op(base, _cuda(f))
        g = _cuda(rng.normal(size=tuple(out.shape)).astype(np.float32))
        out.backward(g)
        ref_out, ref_grad = out.detach(), base.grad
        assert ref_out.abs().sum() > 0 and ref_grad.abs().sum() > 0
        base1 = _cuda(v, True)
        op(base1, _cuda(f)).sum().backward()
        ref_ones = base1.grad
        for vl in FLOAT_LAYOUTS + ('expanded',):
            for fl in ('plain', 'int64', 'strided'):
                for gl in ((vl, 'stride0') if fl == 'plain' else (vl,)):
                    leaf = lay(_cuda(v), vl).requires_grad_(True)   # (a leaf in that layout: its .grad is per image)
                    o = op(leaf, lay(_cuda(f), fl))
                    assert torch.equal(o.detach(), ref_out), (op_name, vl, fl)
                    if gl == 'stride0':
                        grad_as(o, gl).sum().backward()
                        assert torch.equal(leaf.grad, ref_ones), (op_name, vl, fl, gl)
                    else:
                        grad_as(o, gl).backward(g)
                        assert torch.equal(leaf.grad, ref_grad), (op_name, vl, fl, gl)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        leaf = _cuda(v, True)
        ft = _cuda(f)
        with torch.cuda.stream(side):
            o = op(leaf, ft)
            o.backward(g)
        side.synchronize()
        assert torch.equal(o.detach(), ref_out) and torch.equal(leaf.grad, ref_grad), (op_name, 'side stream')


# ---------------------------------------------------------------------------------------------------------------------
# 7. / 8. through the renderer

S = 32
CAMERAS = ('look_at', 'look', 'projection')


def _renderer(camera, shading, anti_aliasing=True):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.image_size = S
    r.anti_aliasing = anti_aliasing
    r.shading = shading
    r.camera_mode = camera
    r.eye = nr.get_points_from_angles(2.732, 25, 40)
    if camera == 'look':
        r.eye = [0.3, 0.2, -2.732]
        r.camera_direction = [-0.1, -0.05, 1.0]
    if camera == 'projection':
        a = 0.3
        r.K = [[30.0, 0.0, 16.0], [0.0, 30.0, 16.0], [0.0, 0.0, 1.0]]
        r.R = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        r.t = [0.05, -0.1, 3.0]
        r.orig_size = float(S)
    return r


def _sphere(B=2):
    v, f = R.batch('icosphere1', B, seed=3)
    return v, np.ascontiguousarray(np.broadcast_to(f, (B,) + f.shape))


def _compose(r, vt, ft, corner, **kw):
    import neural_renderer_amd as nr
    proj, _ = r._frontend(vt, ft)
    return nr.rasterize_rgbad(proj, nr.CornerColors(corner), r.image_size, r.anti_aliasing, r.near, r.far, r.rasterizer_eps,
                              [0, 0, 0], **kw)


@pytest.mark.parametrize('shading', ['flat', 'smooth'])
@pytest.mark.parametrize('camera', CAMERAS)
def test_render_normals_is_the_composition(camera, shading):
    """Bit-equal to rasterize_rgbad(projected faces, corner_normals, background 0) composed by hand; alpha and depth of
    return_dict bit-equal to render_rgbad's; background_color ignored; the light attributes ignored."""
    import neural_renderer_amd as nr
    v, f = _sphere()
    vt, ft = _cuda(v), _cuda(f)
    r = _renderer(camera, shading)
    img = r.render_normals(vt, ft)
    assert img.shape == (2, 3, S, S)
    corner = nr.corner_normals(vt, ft, smooth=shading == 'smooth', fill_back=True).colors
    want = _compose(r, vt, ft, corner)
    assert torch.equal(img, want['rgb'])
    assert (img != 0).any() and (img < 0).any() and (want['alpha'] == 0).any()
    d = r.render_normals(vt, ft, return_dict=True)
    assert sorted(d) == ['alpha', 'depth', 'normals'] and torch.equal(d['normals'], img)
    ad = r.render_rgbad(vt, ft, None, return_rgb=False)
    assert torch.equal(d['alpha'], ad['alpha']) and torch.equal(d['depth'], ad['depth'])
    assert not img.permute(0, 2, 3, 1)[d['alpha'] == 0].any()
    r.background_color = [0.3, 0.4, 0.5]
    r.light_intensity_directional, r.light_direction = 0.9, [1, 0, 0]
    assert torch.equal(r.render_normals(vt, ft), img)
    r.fill_back = False
    front = nr.corner_normals(vt, ft, smooth=shading == 'smooth', fill_back=False).colors
    assert torch.equal(r.render_normals(vt, ft), _compose(r, vt, ft, front)['rgb'])


@pytest.mark.parametrize('shading', ['flat', 'smooth'])
@pytest.mark.parametrize('camera', CAMERAS)
def test_render_normals_against_the_float64_corner_normals(camera, shading):
    """The rasterizer's maps, then (C0 d0 + C1 d1) + C2 d2 with the float64 corner normals of the restatement and the
    forward's float32 weights d_k (vertex_ref.corner_render's formula in float64).  Bound per pixel entry: the corner normals'
    own, gamma_k * magnitude, interpolated with the same weights, plus gamma_3 of sum_k d_k |C_k| for the two products and
    the two additions along the interpolation's longest chain.  Without anti-aliasing the image is the map, flipped."""
    import neural_renderer_amd as nr
    v, f = _sphere()
    vt, ft = _cuda(v), _cuda(f)
    smooth = shading == 'smooth'
    r = _renderer(camera, shading, anti_aliasing=False)
    img = r.render_normals(vt, ft)
    proj, _ = r._frontend(vt, ft)
    corner = nr.corner_normals(vt, ft, smooth=smooth, fill_back=True).colors
    fn = nr.Rasterize(S, r.near, r.far, r.rasterizer_eps, [0, 0, 0], return_rgb=True, return_alpha=True, return_depth=True)
    rgb, _, _ = fn(proj, nr.CornerColors(corner))
    assert torch.equal(rgb.permute(0, 3, 1, 2).flip(2), img)
    fi, wm, dm = (_host(m) for m in (fn.face_index_map, fn.weight_map, fn.depth_map))
    faces = _host(proj)
    assert np.array_equal(_host(rgb), VR.corner_render(faces, fi, wm, dm, _host(corner), (0, 0, 0)))
    (b, y, x), face, d = VR._weights(faces, fi, wm, dm)
    assert len(b) > 50
    d = d.astype(np.float64)[:, :, None]
    c64 = R.corner_normals(v, f, smooth, True)[b, face]
    cbound = (R.gamma(R.corner_k(f, v.shape[1], smooth, True, 2)) * R.corner_mag(v, f, smooth, True))[b, face]
    ref = (c64 * d).sum(1)
    bound = (cbound * d).sum(1) + R.gamma(3) * (np.abs(c64) * d).sum(1)
    ratio = R.worst_ratio(_host(rgb)[b, y, x], ref, bound)
    print('render_normals %s %s: %.3f of the bound' % (camera, shading, ratio))
    assert ratio <= 1


@pytest.mark.parametrize('shading', ['flat', 'smooth'])
@pytest.mark.parametrize('camera', CAMERAS)
def test_camera_space_is_the_rotated_world_space(camera, shading):
    """space = 'camera' against the world-space image rotated per pixel, anti-aliasing off (pixels map one to one).  The
    bound: three products and two additions, gamma_5, on |R| |n|, |n| the image of the absolute corner normals."""
    import neural_renderer_amd as nr
    v, f = _sphere()
    vt, ft = _cuda(v), _cuda(f)
    r = _renderer(camera, shading, anti_aliasing=False)
    world, cam = r.render_normals(vt, ft), r.render_normals(vt, ft, space='camera')
    rot = nr.camera_rotation(r, 2, vt)
    corner = nr.corner_normals(vt, ft, smooth=shading == 'smooth', fill_back=True).colors
    mag = _compose(r, vt, ft, corner.abs())['rgb']
    want = torch.einsum('bij,bjyx->biyx', rot.double(), world.double())
    bound = H.gamma(5) * torch.einsum('bij,bjyx->biyx', rot.abs().double(), mag.double())
    ratio = R.worst_ratio(_host(cam), _host(want), _host(bound))
    print('camera space %s %s: %.3f of the bound' % (camera, shading, ratio))
    assert (cam != world).any() and ratio <= 1


@pytest.mark.parametrize('shading', ['flat', 'smooth'])
def test_normalize_gives_unit_length(shading):
    """normalize = True: n / (|n| + 1e-5) per pixel.  Where alpha is 1 the length is |n| / (|n| + 1e-5) up to the roundings
    of three squares, two additions, the root, the addition of eps, the division and the root of the check itself: within
    gamma_10 of it, |n| taken in float64 from the image without normalize."""
    v, f = _sphere()
    vt, ft = _cuda(v), _cuda(f)
    r = _renderer('look_at', shading)
    d = r.render_normals(vt, ft, return_dict=True)
    unit = r.render_normals(vt, ft, normalize=True)
    inside = _host(d['alpha']) == 1
    assert inside.sum() > 50
    n = np.sqrt((_host(d['normals']).astype(np.float64) ** 2).sum(1))[inside]
    got = np.sqrt((_host(unit).astype(np.float64) ** 2).sum(1))[inside]
    assert n.min() > 0.5
    assert (np.abs(got - n / (n + 1e-5)) <= H.gamma(10)).all()
    assert (np.abs(got - 1) <= 1e-5 / n + H.gamma(10)).all()


def test_gradient_chain_through_the_renderer():
    """render_normals(...).backward reaches the vertices and, with space = 'camera', a learnable eye.  The vertex gradient of
    a smooth world-space render = the adjoint of the corner normals applied to the rasterizer's own grad_corner (float64
    restatement, gamma_(24 + 3 deg) of its magnitudes) + the front-end's part, both taken from the existing operators by
    rendering the detached corner normals.  The front-end scatters its part with float atomics in arrival order: two runs
    of it differ, and the suite's criterion for that gradient is GRAD_TOL of its largest entry (test_face_light_gpu.py)."""
    import neural_renderer_amd as nr
    from test_face_light_gpu import GRAD_TOL
    v, f = _sphere()
    ft = _cuda(f)
    r = _renderer('look_at', 'smooth')
    rng = np.random.default_rng(21)
    G = _cuda(rng.normal(size=(2, 3, S, S)).astype(np.float32))
    v1 = _cuda(v, True)
    r.render_normals(v1, ft).backward(G)
    v2 = _cuda(v, True)
    leaf = nr.corner_normals(v2, ft, smooth=True, fill_back=True).colors.detach().requires_grad_(True)
    _compose(r, v2, ft, leaf)['rgb'].backward(G)
    g_corner, g_front = _host(leaf.grad), _host(v2.grad).astype(np.float64)
    assert np.abs(g_corner).sum() > 0 and np.abs(g_front).sum() > 0
    gv, gv_mag = R.adjoint64(v, f, g_corner, 'corner', True, True)
    got = _host(v1.grad).astype(np.float64)
    bound = R.gamma(R.backward_k(f, v.shape[1], 2)) * gv_mag + H.U * np.abs(got) + GRAD_TOL * np.abs(g_front).max()
    ratio = R.worst_ratio(got, gv + g_front, bound)
    print('gradient chain: %.3f of the bound; normals part %.3e, front-end part %.3e'
          % (ratio, np.abs(gv).max(), np.abs(g_front).max()))
    assert ratio <= 1
    assert np.abs(gv).max() > 100 * GRAD_TOL * np.abs(g_front).max()   # (the normals' part is what the bound is about)
    # camera space: a learnable eye
    r.eye = torch.tensor(nr.get_points_from_angles(2.732, 25, 40), dtype=torch.float32, device='cuda', requires_grad=True)
    v3 = _cuda(v, True)
    (r.render_normals(v3, ft, space='camera') * G).sum().backward()
    assert torch.isfinite(r.eye.grad).all() and r.eye.grad.abs().sum() > 0
    assert torch.isfinite(v3.grad).all() and v3.grad.abs().sum() > 0
    eye_cam = r.eye.grad.clone()
    r.eye.grad = None
    (r.render_normals(_cuda(v), ft, space='world') * G).sum().backward()
    assert not torch.equal(eye_cam, r.eye.grad)   # (the rotation's share is in the camera-space gradient)


# ---------------------------------------------------------------------------------------------------------------------
# 9. a captured graph

def test_graph_capture_equals_eager():
    """A whole step -- Renderer.render_normals, smooth, and the gradient of the vertices -- captured with
    neural_renderer_amd.graph.capture replays equal to eager.  The vertex adjacency table is built on the host: one eager
    call with the same index tensor comes first (graph.capture's warm-up does it too)."""
    import neural_renderer_amd as nr
    B, S = 2, 64
    v, f = H.teapot()
    vertices = torch.tensor(v, device='cuda')[None].expand(B, -1, -1).contiguous().requires_grad_(True)
    faces = torch.tensor(f, device='cuda')[None].expand(B, -1, -1).contiguous()
    rng = np.random.default_rng(12)
    r = nr.Renderer()
    r.image_size = S
    r.shading = 'smooth'
    r.eye = nr.get_points_from_angles(2.732, 15, -90)
    w = torch.zeros((B, 3, S, S), device='cuda')
    out = torch.zeros((B, 3, S, S), device='cuda')

    def step():
        img = r.render_normals(vertices, faces)
        out.copy_(img)
        return torch.autograd.grad((img * w).sum(), [vertices])
    with torch.no_grad():
        r.render_normals(vertices, faces)   # builds the adjacency table (and checks the indices) eagerly
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        w.copy_(torch.tensor(rng.normal(size=w.shape).astype(np.float32)))
    replay()
    torch.cuda.synchronize()
    got_img, got = out.clone(), [g.clone() for g in grads[0]]
    eager = step()
    assert torch.equal(got_img, out) and (out != 0).any()
    for a, b in zip(got, eager):
        assert b.abs().sum() > 0
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 10. the example

def test_example_normals_runs():
    """examples/example_normals.py as a child process with 20 steps: it exits 0 and its last printed loss is below its first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_normals.py'), '20'], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
