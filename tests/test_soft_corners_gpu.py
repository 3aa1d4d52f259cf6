"""`-m gpu`: the soft colour kernels with corner colours (csrc/nr_soft_render.hip, the nr_soft_corners_* entries), soft_render
with colors [B|1,F,3,3] and Renderer.render_soft(per_pixel=True).

rgba, grad_faces and grad_colors against the float64 restatement of tests/soft_render_ref.py under its derived bounds, on the
geometry and (S, sigma, gamma) of tests/test_soft_render_gpu.py's cases; shared colours; reproducibility; the tensor boundary
and a side stream; equal corners against the flat kernels; the renderer end to end, against soft_render of the composition
and against the hard rasterizer; the example.  "Bit for bit" is torch.equal.  The cases and their references are also read
by tests/test_soft_corners.py (CPU: the caps and the sensitivity of the bounds).

Worst ratios measured on the MI355X: see DESIGN "Soft colour rendering", Corner colours (every case prints its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import soft_render_ref as R
import test_soft_render_gpu as G0
from test_soft_render_gpu import BG, _cuda, _faces, _host, _ratios, _run

pytestmark = pytest.mark.gpu

CASES = list(G0.CASES)
IDS = list(G0.IDS)
# the float32 allowance of the comparison with the hard rasterizer: the worst difference MEASURED on the MI355X beyond the
# float64 difference of the two definitions was 3.576e-7, six ulp of a colour near 1 (the test prints it; DESIGN); 4 times it
# is asserted
HARD_ALLOWANCE = 3.576e-7

_cache = {}


def reference(mesh, B, S, sigma, gamma, adds=None):
    """(faces, corner colours uniform in [0, 1], the restatement's Result -- with .g, the upstream gradient, 0 on the masked
    pixels): once per case."""
    key = (mesh, B, S, sigma, gamma, adds)
    if key not in _cache:
        faces = _faces(mesh, B)
        rng = np.random.default_rng(B * 1000 + S + 7)
        colors = rng.uniform(0, 1, (B, faces.shape[1], 3, 3)).astype(np.float32)
        g = rng.normal(size=(B, 4, S, S)).astype(np.float32)
        _cache[key] = (faces, colors, R.restate(faces, colors, S, sigma, gamma, background=BG, g=g, adds=adds))
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement's bounds

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
    assert torch.isfinite(gf).all() and torch.isfinite(gc).all() and torch.isfinite(rgba).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. shared colours

def test_shared_colors():
    """colors [1,F,3,3] beside B = 3: the rgba bits of the expanded tensor; grad_colors [1,F,3,3] within the bound of the
    float64 sum over the images."""
    S, sigma, gamma = 20, 1e-3, 1e-1
    faces = _faces('ico1', 3)
    rng = np.random.default_rng(11)
    colors = rng.uniform(0, 1, (1, faces.shape[1], 3, 3)).astype(np.float32)
    g = rng.normal(size=(3, 4, S, S)).astype(np.float32)
    ref = R.restate(faces, colors, S, sigma, gamma, background=BG, g=g)
    assert ref.masked_share <= 0.01
    rgba, gf, gc = _run(faces, colors, ref.g, S, sigma, gamma)
    wide, gfw, gcw = _run(faces, np.repeat(colors, 3, 0), ref.g, S, sigma, gamma)
    assert tuple(gc.shape) == (1, faces.shape[1], 3, 3) and tuple(gcw.shape) == (3, faces.shape[1], 3, 3)
    assert torch.equal(rgba, wide) and torch.equal(gf, gfw)
    total, bound = R.shared_colors(ref)
    rc = R.worst_ratio(_host(gc), total, bound)
    print('shared corner colours: grad_colors %.3f of the bound' % rc)
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
# 5. three equal corners: the flat kernels

@pytest.mark.parametrize('case', [('mix', 2, 20, 1e-3, 1e-1), ('ico1', 3, 32, 1e-3, 1e-4)])
def test_equal_corners_against_the_flat_kernels(case):
    """The same face colour at the three corners: rgba and grad_faces of the corner kernels against the flat kernels' within
    the sum of the two restatements' bounds; the colour gradient of a face, added over its corners in float64, likewise."""
    mesh, B, S, sigma, gamma = case
    faces, flat, ref_f = G0.reference(*case)
    wide = np.ascontiguousarray(np.repeat(flat[:, :, None, :], 3, 2))
    ref_c = R.restate(faces, wide, S, sigma, gamma, background=BG, g=ref_f.g)
    assert np.array_equal(ref_c.mask, ref_f.mask) and np.array_equal(ref_c.g, ref_f.g)
    a, af, ac = G0._run(faces, flat, ref_f.g, S, sigma, gamma)
    b, bf, bc = _run(faces, wide, ref_f.g, S, sigma, gamma)
    keep = ~np.broadcast_to(ref_f.mask[:, None], ref_f.rgba.shape)
    rr = R.worst_ratio(_host(b)[keep], _host(a).astype(np.float64)[keep], (ref_c.rgba_bound + ref_f.rgba_bound)[keep])
    rf = R.worst_ratio(_host(bf), _host(af).astype(np.float64), ref_c.grad_faces_bound + ref_f.grad_faces_bound)
    rc = R.worst_ratio(_host(bc).astype(np.float64).sum(2), _host(ac).astype(np.float64),
                       ref_c.grad_colors_bound.sum(2) + ref_f.grad_colors_bound)
    print('%s equal corners against flat: rgba %.3f, grad_faces %.3f, grad_colors %.3f of the two bounds' % (mesh, rr, rf, rc))
    assert rr <= 1 and rf <= 1 and rc <= 1, (rr, rf, rc)
    assert af.abs().sum() > 0 and ac.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. through the renderer

def _sphere_scene(B=2):
    import neural_renderer_amd as nr
    v, f = nr.icosphere(2, 0.8)
    return v[None].repeat(B, 1, 1).cuda(), f[None].repeat(B, 1, 1).cuda()


@pytest.mark.parametrize('shading', ['flat', 'smooth'])
@pytest.mark.parametrize('lights', [False, True])
def test_render_soft_per_pixel_is_the_composition(shading, lights):
    """Bit-equal to soft_render(the front copies of the front-end's faces, the front copies of the lit corner colours that
    render() rasterizes)."""
    import neural_renderer_amd as nr
    vertices, faces = _sphere_scene()
    r = nr.Renderer()
    r.image_size, r.eye, r.shading = 32, nr.get_points_from_angles(2.732, 25, 40), shading
    r.soft_gamma, r.background_color = 1e-2, list(BG)
    if lights:
        r.lights = nr.Lights(sh=0.1 * torch.randn(9, 3)).cuda()
    F = faces.shape[1]
    vc = nr.VertexColors(torch.rand(vertices.shape[1], 3, device='cuda'))
    img = r.render_soft(vertices, faces, vc, per_pixel=True)
    proj, corner, kw = r._shade(vertices, faces, vc)
    assert proj.shape[1] == 2 * F and isinstance(corner, nr.CornerColors) and not kw
    want = nr.soft_render(proj[:, :F], corner.colors[:, :F], 32, r.soft_sigma, 1e-2, r.near, r.far, r.soft_eps, BG)
    assert img.shape == (2, 4, 32, 32) and torch.equal(img, want)
    assert not torch.equal(img, r.render_soft(vertices, faces, vc))
    # tensors: the corner colours of the gather times the light give the VertexColors image
    gathered = vc.colors[faces[0].long()][None]
    by_tensor = r.render_soft(vertices, faces, gathered, per_pixel=True)
    assert float((by_tensor - img).abs().max()) <= 1e-5
    assert torch.equal(r.render_soft(vertices, faces, vc, per_pixel=False), r.render_soft(vertices, faces, vc))


def test_render_soft_per_pixel_gradients_on_the_gpu():
    import neural_renderer_amd as nr
    vertices, faces = _sphere_scene(1)
    vertices.requires_grad_(True)
    r = nr.Renderer()
    r.image_size, r.eye, r.shading = 32, nr.get_points_from_angles(2.732, 25, 40), 'smooth'
    r.soft_sigma, r.soft_gamma = 1e-3, 1e-2
    vcol = torch.rand(vertices.shape[1], 3, device='cuda', requires_grad=True)
    w = torch.randn(1, 4, 32, 32, device='cuda')
    (r.render_soft(vertices, faces, nr.VertexColors(vcol), per_pixel=True) * w).sum().backward()
    assert r.last_frontend == 'fused'
    assert torch.isfinite(vertices.grad).all() and vertices.grad[..., 2].abs().sum() > 0
    assert torch.isfinite(vcol.grad).all() and vcol.grad.abs().sum() > 0


def test_render_soft_per_pixel_against_the_hard_rasterizer():
    """A strongly tilted quad of two large faces with four different vertex colours, ambient light only: render() without
    anti-aliasing and render_soft(per_pixel=True) with sigma = 1e-8, gamma = 1e-4 on the pixels farther than sqrt(30 sigma) from
    every edge.  Tolerance per pixel: the float64 difference of the two definitions there (computed here from the projected
    faces) plus 4 x the float32 allowance measured on the MI355X, never above 1e-3.  The scene tells perspective-correct from
    screen-space interpolation: the 'affine' restatement is >= 0.05 off at a compared pixel."""
    import neural_renderer_amd as nr
    S, sigma, gamma = 32, 1e-8, 1e-4
    vertices = torch.tensor([[[-0.93, -0.71, -0.83], [0.91, -0.69, -0.79], [0.89, 0.73, 0.91], [-0.87, 0.67, 0.88]]], device='cuda')
    faces = torch.tensor([[[0, 1, 2], [0, 2, 3]]], dtype=torch.int32, device='cuda')
    vc = nr.VertexColors(torch.tensor([[1.0, 0.1, 0.0], [0.0, 0.9, 0.2], [0.1, 0.0, 1.0], [0.9, 0.8, 0.1]], device='cuda'))
    r = nr.Renderer()
    r.image_size, r.anti_aliasing, r.background_color = S, False, list(BG)
    r.light_intensity_ambient, r.light_intensity_directional = 1.0, 0.0
    hard = r.render(vertices, faces, vc)
    soft = r.render_soft(vertices, faces, vc, sigma=sigma, gamma=gamma, per_pixel=True)
    assert hard.shape == (1, 3, S, S) and soft.shape == (1, 4, S, S)
    # the two definitions in float64, from the very faces and corner colours the kernels got
    proj, corner, _ = r._shade(vertices, faces, vc)
    pf, pc = _host(proj[:, :2]).astype(np.float64), _host(corner.colors[:, :2]).astype(np.float64)
    ref = R.restate(pf, pc, S, sigma, gamma, r.near, r.far, r.soft_eps, BG)
    hard64 = R.hard_image(pf, pc, S, BG)
    compared = np.broadcast_to((ref.edge_d2 > 30 * sigma)[:, None], hard64.shape)
    covered = compared & np.broadcast_to((ref.rgba[:, 3:] > 0.5), hard64.shape)
    assert covered.sum() >= 3 * 100 and (compared & ~covered).sum() >= 3 * 100          # the quad and the background
    definitions = np.abs(ref.rgba[:, :3] - hard64)
    affine = R.restate(pf, pc, S, sigma, gamma, r.near, r.far, r.soft_eps, BG, variant='affine')
    assert np.abs(affine.rgba[:, :3] - ref.rgba[:, :3])[compared].max() >= 0.05
    got = np.abs(_host(soft[:, :3]).astype(np.float64) - _host(hard).astype(np.float64))
    beyond = (got - definitions)[compared].max()
    print('render_soft(per_pixel) against render: worst difference %.3e, of the two definitions in float64 %.3e, beyond it '
          '%.3e on %d compared values' % (got[compared].max(), definitions[compared].max(), beyond, compared.sum()))
    assert 4 * HARD_ALLOWANCE <= 1e-3
    assert beyond <= 4 * HARD_ALLOWANCE
    # ... and each against its own float64 definition
    assert np.abs(_host(soft[:, :3]) - ref.rgba[:, :3])[compared].max() <= 1e-3
    assert np.abs(_host(hard) - hard64)[compared].max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 7. the example

def test_example_soft_vertex_colors_runs():
    """examples/example_soft_vertex_colors.py as a child process with 30 steps: it exits 0 and its last printed loss is below
    its first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_soft_vertex_colors.py'), '30'], cwd=root, env=env,
                         capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('soft step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
