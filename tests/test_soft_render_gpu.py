"""`-m gpu`: the soft colour kernels (csrc/nr_soft_render.hip), soft_render and Renderer.render_soft.

rgba, grad_faces and grad_colors against the float64 restatement of tests/soft_render_ref.py under its derived bounds, on cases
built for the kernel's seams; shared colours; reproducibility; the tensor boundary and a side stream; the renderer end to
end; the dispatch and the plain-torch implementation in float32.  "Bit for bit" is torch.equal.  The cases and their
references are also read by tests/test_soft_render.py (CPU: the caps and the sensitivity of the bounds).

Worst ratios measured on the MI355X: see DESIGN "Soft colour rendering" (every case prints its own)."""
import numpy as np
import pytest
import torch

import soft_render_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 256   # csrc/nr_soft_pair.h: SOFT_CHUNK, the face records per LDS chunk
BG = (0.2, 0.3, 0.4)
NAN = float('nan')
# (the contributing ones at coordinates that are no pixel centres and put no edge through one: the masked-pixel cap)
EXTRA = [[[-3.013, -2.507, 1.5], [3.217, -2.011, 2.0], [0.309, 4.003, 6.0]],   # larger than the screen, behind most of the sphere
         [[1.503, 0.207, 1.0], [2.511, 0.103, 1.0], [2.009, 0.907, 1.0]],      # wholly off screen
         [[0.2, 0.1, 1.0], [0.2, 0.1, 1.0], [-0.4, 0.3, 1.2]],                 # zero area: a repeated vertex
         [[-0.1, 0.3, 2.0], [0.4, -0.2, 2.5], [0.4, -0.2, 2.5]],               # zero area: a repeated vertex
         [[0.0, 0.1, 1.0], [NAN, 0.4, 1.0], [0.3, 0.2, 1.0]],                  # dropped: a NaN
         [[0.0, 0.1, 1.0], [0.5, float('inf'), 1.0], [0.3, 0.2, 1.0]],         # dropped: an inf
         [[0.0, 0.1, 0.05], [0.5, 0.4, 1.0], [0.3, 0.2, 1.0]],                 # dropped: z in front of near
         [[0.0, 0.1, 1.0], [0.5, 0.4, 1.0], [0.3, 0.2, 200.0]],                # dropped: z behind far
         [[-0.503, -0.307, 1.2], [0.509, -0.253, 1.8], [0.053, 0.447, 1.5]],   # two faces that cross in depth inside a tile:
         [[-0.457, -0.353, 1.8], [0.551, -0.207, 1.2], [0.003, 0.501, 1.5]]]   # their order changes from pixel to pixel


def _cuda(a, grad=False):
    a = np.ascontiguousarray(a)
    return torch.tensor(a, device='cuda', requires_grad=bool(grad) and a.dtype.kind == 'f')


def _host(t):
    return t.detach().cpu().numpy()


def _faces(mesh, B):
    if mesh == 'ico1':
        return R.sphere_faces(1, B)
    sphere, extra = R.sphere_faces(2, B), np.asarray(EXTRA, np.float32)
    at = np.linspace(0, sphere.shape[1], len(extra)).astype(int)   # in front of, inside and behind every image's mesh
    out = []
    for b in range(B):
        rows = list(sphere[b])
        for i in reversed(range(len(extra))):
            rows.insert(at[i], extra[i])
        out.append(np.stack(rows))
    return np.stack(out).astype(np.float32)


# (mesh, B, S, sigma, gamma): S 16 one tile, 20 a partial tile, 32 several tiles; 80 faces below a chunk, 330 a chunk and a
# tail; sigma 1e-6 boxes that miss most pixel centres, 1 every face reaches every pixel; gamma 1e-4 a hard depth order, 1e-1 a mix
CASES = [('ico1', 3, S, sg, gm) for S in (16, 20, 32) for sg in (1e-6, 1e-3, 1.0) for gm in (1e-4, 1e-1)] + \
        [('mix', 2, 32, 1e-3, 1e-4), ('mix', 2, 20, 1e-3, 1e-1), ('mix', 1, 20, 1.0, 1e-2)]
IDS = ['%s-B%d-S%d-sigma%g-gamma%g' % c for c in CASES]

_cache = {}


def reference(mesh, B, S, sigma, gamma, adds=None):
    """(faces, colors, the restatement's Result -- with .g, the upstream gradient, 0 on the masked pixels): once per case."""
    key = (mesh, B, S, sigma, gamma, adds)
    if key not in _cache:
        faces = _faces(mesh, B)
        rng = np.random.default_rng(B * 1000 + S)
        colors = rng.uniform(0, 1, (B, faces.shape[1], 3)).astype(np.float32)
        g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
        _cache[key] = (faces, colors, R.restate(faces, colors, S, sigma, gamma, background=BG, g=g, adds=adds))
    return _cache[key]


def _run(faces, colors, g, S, sigma, gamma, implementation='hip'):
    import neural_renderer_amd as nr
    ft, ct = _cuda(faces, True), _cuda(colors, True)
    rgba = nr.soft_render(ft, ct, S, sigma, gamma, background_color=BG, implementation=implementation)
    rgba.backward(_cuda(np.asarray(g, np.float32)))
    return rgba.detach(), ft.grad, ct.grad


def _ratios(ref, rgba, gf, gc):
    return (R.masked_ratio(_host(rgba), ref.rgba, ref.rgba_bound, ref.mask),
            R.worst_ratio(_host(gf), ref.grad_faces, ref.grad_faces_bound),
            R.worst_ratio(_host(gc), ref.grad_colors, ref.grad_colors_bound))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement's bounds

def test_the_cases_reach_the_seams():
    F = _faces('mix', 1).shape[1]
    assert F == 330 > CHUNK > 80 and F % CHUNK != 0


@pytest.mark.parametrize('mesh,B,S,sigma,gamma', CASES, ids=IDS)
def test_forward_and_gradients_within_the_derived_bounds(mesh, B, S, sigma, gamma):
    """rgba (outside the masked pixels), grad_faces and grad_colors from random upstream gradients (0 on the masked pixels)
    within the per-entry bounds of soft_render_ref (its docstring); the caps on masked pixels and pairs in doubt."""
    faces, colors, ref = reference(mesh, B, S, sigma, gamma)
    rgba, gf, gc = _run(faces, colors, ref.g, S, sigma, gamma)
    assert tuple(rgba.shape) == (B, 4, S, S) and tuple(gf.shape) == faces.shape and tuple(gc.shape) == colors.shape
    rr, rf, rc = _ratios(ref, rgba, gf, gc)
    print('%s B=%d S=%d sigma=%g gamma=%g: rgba %.3f, grad_faces %.3f, grad_colors %.3f of the bound; masked %.2f %% of the '
          'pixels with a pair, in doubt %.2f %% of %d pairs' % (mesh, B, S, sigma, gamma, rr, rf, rc, 100 * ref.masked_share,
                                                                 100 * ref.doubt_share, sum(ref.pairs)))
    assert ref.masked_share <= 0.01, 'masked pixels: %.2f %% of the pixels with a taken pair' % (100 * ref.masked_share)
    assert ref.doubt_share <= 0.02
    assert rr <= 1 and rf <= 1 and rc <= 1, (rr, rf, rc)
    assert np.abs(ref.grad_faces[..., 2]).max() > 0 and np.abs(ref.grad_colors).max() > 0


def test_dropped_and_zero_area_faces():
    """The mixed case: the four dropped and the two zero-area faces get exactly 0 everywhere and leave the image as it is
    without them."""
    import neural_renderer_amd as nr
    faces, colors, ref = reference('mix', 2, 20, 1e-3, 1e-1)
    rgba, gf, gc = _run(faces, colors, ref.g, 20, 1e-3, 1e-1)
    F = faces.shape[1]
    at = np.linspace(0, F - len(EXTRA), len(EXTRA)).astype(int) + np.arange(len(EXTRA))
    assert all(np.array_equal(faces[0, at[i]], np.asarray(EXTRA[i], np.float32), equal_nan=True) for i in range(len(EXTRA)))
    assert torch.isfinite(gf).all() and torch.isfinite(gc).all() and torch.isfinite(rgba).all()
    assert not gf[:, at[2:8]].any() and not gc[:, at[2:8]].any()
    assert gf[:, at[8:]].abs().sum() > 0 and gf[:, at[0]].abs().sum() > 0
    keep = np.delete(np.arange(F), at[2:8])
    alone = nr.soft_render(_cuda(faces[:, keep]), _cuda(colors[:, keep]), 20, 1e-3, 1e-1, background_color=BG, implementation='hip')
    assert torch.equal(alone, rgba)


# ---------------------------------------------------------------------------------------------------------------------
# 2. shared colours

def test_shared_colors():
    """colors [1,F,3] beside B = 3: the rgba bits of the expanded tensor; grad_colors [1,F,3] within the bound of the float64
    sum over the images."""
    S, sigma, gamma = 20, 1e-3, 1e-1
    faces = _faces('ico1', 3)
    rng = np.random.default_rng(11)
    colors = rng.uniform(0, 1, (1, faces.shape[1], 3)).astype(np.float32)
    g = rng.normal(size=(3, 4, S, S)).astype(np.float32)
    ref = R.restate(faces, colors, S, sigma, gamma, background=BG, g=g)
    assert ref.masked_share <= 0.01
    rgba, gf, gc = _run(faces, colors, ref.g, S, sigma, gamma)
    wide, gfw, gcw = _run(faces, np.repeat(colors, 3, 0), ref.g, S, sigma, gamma)
    assert tuple(gc.shape) == (1, faces.shape[1], 3) and tuple(gcw.shape) == (3, faces.shape[1], 3)
    assert torch.equal(rgba, wide) and torch.equal(gf, gfw)
    total, bound = R.shared_colors(ref)
    rc = R.worst_ratio(_host(gc), total, bound)
    print('shared colours: grad_colors %.3f of the bound' % rc)
    assert rc <= 1 and np.abs(total).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. reproducibility

@pytest.mark.parametrize('case', [('mix', 2, 32, 1e-3, 1e-4), ('ico1', 3, 20, 1.0, 1e-1)])
def test_two_runs_and_an_image_alone_give_the_same_bits(case):
    mesh, B, S, sigma, gamma = case
    faces, colors, ref = reference(*case)
    a0 = _run(faces, colors, ref.g, S, sigma, gamma)
    a1 = _run(faces, colors, ref.g, S, sigma, gamma)
    assert all(torch.equal(x, y) for x, y in zip(a0, a1)) and a0[1].abs().sum() > 0 and a0[2].abs().sum() > 0
    for b in range(B):
        one = _run(faces[b:b + 1], colors[b:b + 1], ref.g[b:b + 1], S, sigma, gamma)
        assert all(torch.equal(x[0], y[b]) for x, y in zip(one, a0)), b


# ---------------------------------------------------------------------------------------------------------------------
# 4. the tensor boundary

def test_layouts_alignment_and_a_side_stream():
    """faces, colors and the upstream gradient as a strided view, as views 4 / 8 / 12 bytes off the 16-byte grid and
    permuted, and one call on a side stream: the bits of the dense call."""
    import neural_renderer_amd as nr
    from test_layout_invariance_gpu import FLOAT_LAYOUTS, grad_as, lay
    case = ('ico1', 3, 20, 1e-3, 1e-1)
    S, sigma, gamma = case[2:]
    faces, colors, ref = reference(*case)
    gt = _cuda(np.asarray(ref.g, np.float32))
    ref_a, ref_f, ref_c = _run(faces, colors, ref.g, S, sigma, gamma)
    assert ref_a.abs().sum() > 0 and ref_f.abs().sum() > 0 and ref_c.abs().sum() > 0
    for fl in FLOAT_LAYOUTS:
        for gl in ('plain', fl):
            lf, lc = lay(_cuda(faces), fl).requires_grad_(True), lay(_cuda(colors), fl).requires_grad_(True)
            out = nr.soft_render(lf, lc, S, sigma, gamma, background_color=BG, implementation='hip')
            assert torch.equal(out.detach(), ref_a), fl
            grad_as(out, gl).backward(gt)
            assert torch.equal(lf.grad, ref_f) and torch.equal(lc.grad, ref_c), (fl, gl)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    lf, lc = _cuda(faces, True), _cuda(colors, True)
    with torch.cuda.stream(side):
        out = nr.soft_render(lf, lc, S, sigma, gamma, background_color=BG, implementation='hip')
        out.backward(gt)
    side.synchronize()
    assert torch.equal(out.detach(), ref_a) and torch.equal(lf.grad, ref_f) and torch.equal(lc.grad, ref_c)


# ---------------------------------------------------------------------------------------------------------------------
# 5. through the renderer

def _two_spheres():
    """A sphere of radius 0.7 at the origin and one of radius 0.3 behind it, seen from (0, 0, -2.732): wholly hidden."""
    import neural_renderer_amd as nr
    v0, f0 = nr.icosphere(1, 0.7)
    v1, f1 = nr.icosphere(1, 0.3)
    v1 = v1 + torch.tensor([0.0, 0.0, 1.2])
    vertices = torch.cat((v0, v1))[None].cuda()
    faces = torch.cat((f0, f1 + v0.shape[0]))[None].cuda()
    return vertices, faces, v0.shape[0], f0.shape[0]


def test_render_soft_moves_a_hidden_sphere_where_render_cannot():
    import neural_renderer_amd as nr
    S = 32
    vertices, faces, nv, nf = _two_spheres()
    r = nr.Renderer()
    r.image_size, r.eye = S, [0.0, 0.0, -2.732]
    r.soft_sigma, r.soft_gamma = 1e-3, 1e-2
    F = faces.shape[1]
    face_colors = torch.zeros(1, F, 3, device='cuda')
    face_colors[:, :nf, 0] = 1.0   # the front sphere red
    face_colors[:, nf:, 2] = 1.0   # the hidden one blue
    cubes = face_colors[:, :, None, None, None, :].expand(1, F, 2, 2, 2, 3).contiguous()
    with torch.no_grad():   # the target: the small sphere in front
        moved = vertices.clone()
        moved[:, nv:, 2] -= 2.2
        target = r.render_soft(moved, faces, face_colors)[:, :3]
    # the rasterizer: nothing for the hidden sphere
    v = vertices.clone().requires_grad_(True)
    nr.squared_error_loss(r.render(v, faces, cubes), target).sum().backward()
    assert v.grad[:, :nv].abs().sum() > 0 and not v.grad[:, nv:].any()
    # the soft image: a gradient, z included, and a step along it lowers the loss
    v = vertices.clone().requires_grad_(True)
    loss = nr.squared_error_loss(r.render_soft(v, faces, face_colors)[:, :3], target).sum()
    loss.backward()
    assert r.last_frontend == 'fused'
    hidden = v.grad[:, nv:]
    assert torch.isfinite(v.grad).all() and hidden.abs().sum() > 0 and hidden[..., 2].abs().sum() > 0
    assert float(hidden[..., 2].sum()) > 0   # descent brings it nearer to the camera at -z
    with torch.no_grad():
        stepped = v - (1e-3 / float(v.grad.abs().max())) * v.grad
        after = nr.squared_error_loss(r.render_soft(stepped, faces, face_colors)[:, :3], target).sum()
    print('loss %.6f -> %.6f' % (float(loss.detach()), float(after)))
    assert float(after) < float(loss.detach())


def test_render_soft_is_the_composition():
    """Bit-equal to soft_render(the front-end's faces without the fill_back copies, colours times the front copies' light)."""
    import neural_renderer_amd as nr
    vertices, faces, nv, nf = _two_spheres()
    vertices, faces = vertices.repeat(2, 1, 1), faces.repeat(2, 1, 1)
    r = nr.Renderer()
    r.image_size, r.eye = 32, nr.get_points_from_angles(2.732, 25, 40)
    r.soft_gamma, r.background_color = 1e-2, list(BG)
    F = faces.shape[1]
    colors = torch.rand(1, F, 3, device='cuda')
    img = r.render_soft(vertices, faces, colors)
    proj, light = r._frontend(vertices, faces, light_colors=True)
    assert proj.shape[1] == 2 * F
    want = nr.soft_render(proj[:, :F], colors * light[:, :F], 32, r.soft_sigma, 1e-2, r.near, r.far, r.soft_eps, BG)
    assert img.shape == (2, 4, 32, 32) and torch.equal(img, want)
    vc = nr.VertexColors(torch.rand(vertices.shape[1], 3, device='cuda'))
    mean = vc.colors[faces[0].long()].mean(1)[None]
    assert torch.equal(r.render_soft(vertices, faces, vc), r.render_soft(vertices, faces, mean))


# ---------------------------------------------------------------------------------------------------------------------
# 6. dispatch, and the other implementation

def test_dispatch():
    import neural_renderer_amd as nr
    f, c = torch.rand(1, 4, 3, 3) + 1, torch.rand(1, 4, 3)
    for ft, ct in ((f, c), (f.cuda().double(), c.cuda().double())):
        with pytest.raises(ValueError):
            nr.soft_render(ft, ct, 8, implementation='hip')
        assert nr.soft_render(ft, ct, 8).shape == (1, 4, 8, 8)   # ... and None takes torch
    with pytest.raises(ValueError):
        nr.soft_render(f.cuda(), c, 8)


@pytest.mark.parametrize('case', [('ico1', 3, 20, 1e-3, 1e-1), ('ico1', 3, 16, 1.0, 1e-4)])
def test_torch_in_float32_within_the_bounds(case):
    """soft_render_torch in float32 on the GPU against the restatement, with S^2 additions for torch's pixel sum in an order
    of its own."""
    mesh, B, S, sigma, gamma = case
    faces, colors, ref = reference(*case, adds=S * S)
    rr, rf, rc = _ratios(ref, *_run(faces, colors, ref.g, S, sigma, gamma, 'torch'))
    print('%s torch: rgba %.3f, grad_faces %.3f, grad_colors %.3f of the bound' % (mesh, rr, rf, rc))
    assert rr <= 1 and rf <= 1 and rc <= 1, (rr, rf, rc)
