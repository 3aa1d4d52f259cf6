"""`-m gpu`: the soft-silhouette kernels (csrc/nr_soft_silhouette.hip), soft_silhouettes and Renderer.render_soft_silhouettes.

Forward and gradient against the float64 restatement of tests/soft_ref.py under its derived bounds, on cases built for the
kernel's seams; the pixel centres and the row flip against the shipped rasterizer; reproducibility; the plain-torch
implementation and the tensor boundary; the renderer; a captured graph; the example.  "Bit for bit" is torch.equal.

Worst ratios measured on the MI355X: see DESIGN "Soft silhouettes" (every case prints its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import soft_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 256   # csrc/nr_soft_pair.h: SOFT_CHUNK, the face records per LDS chunk


def _cuda(a, grad=False):
    a = np.ascontiguousarray(a)
    return torch.tensor(a, device='cuda', requires_grad=bool(grad) and a.dtype.kind == 'f')


def _host(t):
    return t.detach().cpu().numpy()


def _with(faces, extra):
    """faces [B,F,3,3] with the faces `extra` [n,3,3] put in front of, into the middle of and behind every image's mesh."""
    B, F = faces.shape[:2]
    extra = np.asarray(extra, np.float32)
    at = np.linspace(0, F, len(extra)).astype(int)
    out = []
    for b in range(B):
        rows = list(faces[b])
        for i in reversed(range(len(extra))):
            rows.insert(at[i], extra[i])
        out.append(np.stack(rows))
    return np.stack(out).astype(np.float32)


TRI = np.array([[[-0.5, -0.4, 1.0], [0.6, -0.3, 1.5], [0.1, 0.7, 2.0]]], np.float32)
BIG = [[[-3.0, -2.5, 1.0], [3.2, -2.0, 1.0], [0.3, 4.0, 1.0]]]           # larger than the screen
OFF = [[[1.5, 0.2, 1.0], [2.5, 0.1, 1.0], [2.0, 0.9, 1.0]]]              # wholly off screen
NAN, INF = float('nan'), float('inf')
ODD = [[[-0.3, -0.2, 1.0], [0.1, 0.2, 1.0], [0.5, 0.6, 1.0]],            # zero area: three points on a line
       [[0.2, 0.1, 1.0], [0.2, 0.1, 1.0], [-0.4, 0.3, 1.0]],             # zero area: a repeated vertex
       [[0.0, 0.1, 1.0], [NAN, 0.4, 1.0], [0.3, 0.2, 1.0]],              # dropped: a NaN
       [[0.0, 0.1, 1.0], [0.5, INF, 1.0], [0.3, 0.2, 1.0]],              # dropped: an inf
       [[0.0, 0.1, 0.05], [0.5, 0.4, 1.0], [0.3, 0.2, 1.0]],             # dropped: z in front of near
       [[0.0, 0.1, 1.0], [0.5, 0.4, 1.0], [0.3, 0.2, 200.0]]]            # dropped: z behind far


def _faces(mesh, B):
    if mesh == 'tri':
        return np.repeat(TRI[None], B, 0) + np.float32(0.01) * np.arange(B, dtype=np.float32)[:, None, None, None]
    if mesh in ('big', 'off', 'odd'):
        level = 2 if mesh == 'odd' else 0   # (326 faces: the two zero-area faces stay a small share of the pairs)
        return _with(R.sphere_faces(level, B), {'big': BIG, 'off': OFF, 'odd': ODD}[mesh])
    return R.sphere_faces({'ico0': 0, 'ico1': 1, 'ico2': 2}[mesh], B)


# (mesh, B, S, sigma): S 16 a whole tile, 20 partial tiles, 32 several workgroups; F 1 / 20 / 80 below a chunk, 320 a chunk and
# a partial tail; sigma 1e-6 boxes that miss every pixel centre, 1 every face reaches every pixel and nothing is left out
CASES = [('ico1', 3, S, sg) for S in (16, 20, 32) for sg in (1e-6, 1e-3, 1.0)] + \
        [('tri', 1, 20, 1e-3), ('tri', 3, 16, 1.0), ('ico0', 1, 20, 1e-3), ('ico0', 3, 32, 1e-6), ('ico1', 1, 20, 1e-3),
         ('ico2', 1, 20, 1e-3), ('ico2', 3, 32, 1e-3), ('ico2', 1, 16, 1.0), ('ico2', 1, 32, 1e-6),
         ('big', 3, 20, 1e-3), ('big', 1, 32, 1.0), ('off', 3, 20, 1e-3), ('off', 1, 16, 1.0),
         ('odd', 3, 20, 1e-3), ('odd', 1, 32, 1e-6), ('odd', 1, 16, 1.0)]
IDS = ['%s-B%d-S%d-sigma%g' % c for c in CASES]

_cache = {}


def _reference(mesh, B, S, sigma, adds=None):
    """(faces, g, the restatement's Result): computed once per case and shared."""
    key = (mesh, B, S, sigma, adds)
    if key not in _cache:
        faces = _faces(mesh, B)
        g = np.random.default_rng(B * 1000 + S).normal(size=(B, S, S)).astype(np.float32)
        _cache[key] = (faces, g, R.restate(faces, S, sigma, g=g, adds=adds))
    return _cache[key]


def _run(faces, g, S, sigma, implementation='hip'):
    import neural_renderer_amd as nr
    ft = _cuda(faces, True)
    alpha = nr.soft_silhouettes(ft, S, sigma, implementation=implementation)
    alpha.backward(_cuda(g))
    return alpha.detach(), ft.grad


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement's bounds

def test_the_cases_reach_the_seams():
    assert R.sphere_faces(2).shape[1] == 320 > CHUNK > 80 and 320 % CHUNK != 0


@pytest.mark.parametrize('mesh,B,S,sigma', CASES, ids=IDS)
def test_forward_and_gradient_within_the_derived_bounds(mesh, B, S, sigma):
    """alpha (and with it Q) and grad_faces from random upstream gradients within the per-entry bounds of soft_ref (its
    docstring); equality where a bound is 0 (every z, every dropped face).  Pairs in doubt: at most 2 % of the pairs."""
    faces, g, ref = _reference(mesh, B, S, sigma)
    alpha, grad = _run(faces, g, S, sigma)
    assert tuple(alpha.shape) == (B, S, S) and tuple(grad.shape) == faces.shape
    ra = R.worst_ratio(_host(alpha), ref.alpha, ref.alpha_bound)
    rg = R.worst_ratio(_host(grad), ref.grad, ref.grad_bound)
    print('%s B=%d S=%d sigma=%g: alpha %.3f, grad_faces %.3f of the bound; in doubt %.2f %% of %d pairs'
          % (mesh, B, S, sigma, ra, rg, 100 * ref.doubt_share, sum(ref.pairs)))
    assert ref.doubt_share <= 0.02
    assert ra <= 1 and rg <= 1, (ra, rg)
    assert not _host(grad)[..., 2].any()
    assert np.abs(ref.grad).max() > 0 or sigma == 1e-6


def test_dropped_and_degenerate_faces():
    """The mixed case: the four dropped faces get exactly 0 and leave the image as it is without them; the zero-area faces
    get finite gradients."""
    import neural_renderer_amd as nr
    faces, g, _ = _reference('odd', 3, 20, 1e-3)
    alpha, grad = _run(faces, g, 20, 1e-3)
    F = faces.shape[1]
    at = np.linspace(0, F - len(ODD), len(ODD)).astype(int) + np.arange(len(ODD))
    assert all(np.array_equal(faces[0, at[i]], np.asarray(ODD[i], np.float32), equal_nan=True) for i in range(len(ODD)))
    assert torch.isfinite(grad).all() and torch.isfinite(alpha).all()
    assert not grad[:, at[2:]].any() and grad[:, at[:2]].abs().sum() > 0
    keep = np.delete(np.arange(F), at[2:])
    assert torch.equal(nr.soft_silhouettes(_cuda(faces[:, keep]), 20, 1e-3, implementation='hip'), alpha)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the product's own rasterizer

def test_agrees_with_the_rasterizer_on_pixel_centres_and_rows():
    """icosphere(1), S = 32, sigma = 1e-8: soft > 0.5 is the hard silhouette on every pixel farther than sqrt(30 sigma) from
    every edge (float64 distance of the restatement); at most 2 % of the image is nearer."""
    import neural_renderer_amd as nr
    S, sigma = 32, 1e-8
    faces = R.sphere_faces(1, 2)
    ft = _cuda(faces)
    soft = nr.soft_silhouettes(ft, S, sigma, implementation='hip') > 0.5
    hard = nr.rasterize_silhouettes(torch.cat((ft, ft.flip(2)), dim=1), S, anti_aliasing=False) > 0
    ref = R.restate(faces, S, sigma)
    far = torch.tensor(np.ascontiguousarray(ref.d2_min > 30 * sigma), device='cuda')
    print('pixels left out: %.2f %%' % (100 * (1 - float(far.float().mean()))))
    assert float(far.float().mean()) >= 0.98
    assert hard.any() and not hard.all() and not torch.equal(hard, hard.flip(1))
    assert torch.equal(soft[far], hard[far])


# ---------------------------------------------------------------------------------------------------------------------
# 3. reproducibility

@pytest.mark.parametrize('mesh,S,sigma', [('ico2', 32, 1e-3), ('odd', 20, 1.0)])
def test_two_runs_and_an_image_alone_give_the_same_bits(mesh, S, sigma):
    faces, g, _ = _reference(mesh, 3, S, sigma) if (mesh, 3, S, sigma) in CASES else (_faces(mesh, 3), None, None)
    if g is None:
        g = np.random.default_rng(5).normal(size=(3, S, S)).astype(np.float32)
    a0, g0 = _run(faces, g, S, sigma)
    a1, g1 = _run(faces, g, S, sigma)
    assert torch.equal(a0, a1) and torch.equal(g0, g1) and g0.abs().sum() > 0
    for b in range(3):
        ab, gb = _run(faces[b:b + 1], g[b:b + 1], S, sigma)
        assert torch.equal(ab[0], a0[b]) and torch.equal(gb[0], g0[b]), b


# ---------------------------------------------------------------------------------------------------------------------
# 4. the other implementation, the tensor boundary

@pytest.mark.parametrize('mesh,B,S,sigma', [('ico1', 3, 20, 1e-3), ('odd', 1, 16, 1.0)])
def test_hip_and_torch_within_their_bounds(mesh, B, S, sigma):
    """soft_silhouettes_torch in float32 on the GPU against the restatement, with S^2 additions for torch's pixel sum in an
    order of its own; the HIP result against the same restatement with the kernel's count."""
    faces, g, ref = _reference(mesh, B, S, sigma)
    _, _, ref_t = _reference(mesh, B, S, sigma, adds=S * S)
    for name, r, (alpha, grad) in (('hip', ref, _run(faces, g, S, sigma)), ('torch', ref_t, _run(faces, g, S, sigma, 'torch'))):
        ra = R.worst_ratio(_host(alpha), r.alpha, r.alpha_bound)
        rg = R.worst_ratio(_host(grad), r.grad, r.grad_bound)
        print('%s %s: alpha %.3f, grad_faces %.3f of the bound' % (mesh, name, ra, rg))
        assert ra <= 1 and rg <= 1, (name, ra, rg)


def test_layouts_alignment_and_a_side_stream():
    """Faces as a strided view, as views 4 / 8 / 12 bytes off the 16-byte grid and permuted, the upstream gradient in those
    layouts, and one call on a side stream: the bits of the dense call."""
    import neural_renderer_amd as nr
    from test_layout_invariance_gpu import FLOAT_LAYOUTS, grad_as, lay
    S, sigma = 20, 1e-3
    faces, g, _ = _reference('ico1', 3, S, sigma)
    gt = _cuda(g)
    ref_a, ref_g = _run(faces, g, S, sigma)
    assert ref_a.abs().sum() > 0 and ref_g.abs().sum() > 0
    for fl in FLOAT_LAYOUTS:
        for gl in ('plain', fl):
            leaf = lay(_cuda(faces), fl).requires_grad_(True)
            out = nr.soft_silhouettes(leaf, S, sigma, implementation='hip')
            assert torch.equal(out.detach(), ref_a), fl
            grad_as(out, gl).backward(gt)
            assert torch.equal(leaf.grad, ref_g), (fl, gl)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    leaf = _cuda(faces, True)
    with torch.cuda.stream(side):
        out = nr.soft_silhouettes(leaf, S, sigma, implementation='hip')
        out.backward(gt)
    side.synchronize()
    assert torch.equal(out.detach(), ref_a) and torch.equal(leaf.grad, ref_g)


# ---------------------------------------------------------------------------------------------------------------------
# 5. through the renderer

CAMERAS = ('look_at', 'look', 'projection')


def _renderer(camera, S=32):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.image_size = S
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


def _sphere(B=2, level=1, radius=0.8, shift=0.0):
    import neural_renderer_amd as nr
    v, f = nr.icosphere(level, radius)
    v = v[None].repeat(B, 1, 1).clone()
    v[:, :, :2] += shift   # (sideways and upwards alike)
    return v.cuda(), f[None].repeat(B, 1, 1).cuda()


@pytest.mark.parametrize('fill_back', [True, False])
@pytest.mark.parametrize('camera', CAMERAS)
def test_render_soft_silhouettes_is_the_composition(camera, fill_back):
    """Bit-equal to soft_silhouettes(the front-end's faces without the fill_back copies, image_size, soft_sigma, near, far);
    the fused front-end serves it; anti_aliasing and the light are ignored."""
    import neural_renderer_amd as nr
    vt, ft = _sphere()
    r = _renderer(camera)
    r.fill_back = fill_back
    r.soft_sigma = 3e-3
    img = r.render_soft_silhouettes(vt, ft)
    assert r.last_frontend == 'fused'
    assert img.shape == (2, 32, 32) and (img > 0.9).any() and (img < 0.1).any()
    proj, _ = r._frontend(vt, ft)
    assert proj.shape[1] == ft.shape[1] * (2 if fill_back else 1)
    assert torch.equal(img, nr.soft_silhouettes(proj[:, :ft.shape[1]], 32, 3e-3, r.near, r.far))
    assert torch.equal(r.render_soft_silhouettes(vt, ft, sigma=1e-2), nr.soft_silhouettes(proj[:, :ft.shape[1]], 32, 1e-2, r.near, r.far))
    r.anti_aliasing, r.light_intensity_directional, r.shading = False, 0.9, 'smooth'
    assert torch.equal(r.render_soft_silhouettes(vt, ft), img)
    r.near = 2.5   # the front of the sphere is nearer: those faces drop out
    assert not torch.equal(r.render_soft_silhouettes(vt, ft), img)


def test_gradient_reaches_vertices_and_a_learnable_eye():
    import neural_renderer_amd as nr
    vt, ft = _sphere()
    vt.requires_grad_(True)
    r = _renderer('look_at')
    r.eye = torch.tensor(nr.get_points_from_angles(2.732, 25, 40), dtype=torch.float32, device='cuda', requires_grad=True)
    w = torch.tensor(np.random.default_rng(3).normal(size=(2, 32, 32)).astype(np.float32), device='cuda')
    (r.render_soft_silhouettes(vt, ft) * w).sum().backward()
    assert torch.isfinite(vt.grad).all() and vt.grad.abs().sum() > 0
    assert torch.isfinite(r.eye.grad).all() and r.eye.grad.abs().sum() > 0


def test_a_gradient_where_the_hard_silhouette_has_none():
    """A sphere whose silhouette does not overlap its target: silhouette_iou_loss through render_soft_silhouettes gives the
    vertices a gradient, the same step through render_silhouettes exactly zero.  The target lies diagonally away: the
    rasterizer's gradient sweeps an edge along its pixel row and its pixel column, as far as they go, so a target straight to
    the side would still pull; with no row and no column in common there is nothing."""
    import neural_renderer_amd as nr
    S = 64
    r = _renderer('look_at', S)
    r.eye = [0.0, 0.0, -2.732]
    r.soft_sigma = 1e-2
    with torch.no_grad():
        tv, tf = _sphere(1, 1, 0.3, shift=0.5)
        target = r.render_silhouettes(tv, tf)
    vt, ft = _sphere(1, 1, 0.3, shift=-0.5)
    vt.requires_grad_(True)
    hard = r.render_silhouettes(vt, ft)
    assert target.sum() > 10 and hard.sum() > 10
    assert not (hard.detach().amax(1) * target.amax(1)).any() and not (hard.detach().amax(2) * target.amax(2)).any()
    nr.silhouette_iou_loss(hard, target).sum().backward()
    assert not vt.grad.any()
    vt.grad = None
    nr.silhouette_iou_loss(r.render_soft_silhouettes(vt, ft), target).sum().backward()
    assert torch.isfinite(vt.grad).all() and vt.grad.abs().sum() > 0
    assert float(vt.grad[0, :, 0].sum()) < 0 and float(vt.grad[0, :, 1].sum()) < 0   # descent moves it right and up, to the target


# ---------------------------------------------------------------------------------------------------------------------
# 6. a captured graph

def test_graph_capture_equals_eager():
    """A step -- render_soft_silhouettes, silhouette_iou_loss and the gradient of the vertices -- captured with
    neural_renderer_amd.graph.capture replays equal to eager.  The eager call that comes first runs without autograd, as in
    tests/test_normals_gpu.py: an eager BACKWARD before the capture would create the leaf's gradient accumulator on the
    default stream, and inside the capture autograd then makes the default stream wait for the capturing one -- torch warns
    that this breaks a capture, and it took this test's process down in capture_end when its eager step was a whole step.
    (The soft silhouette has no atomics; the front-end's backward scatters with float atomics: the criterion of
    tests/test_normals_gpu.py for the vertex gradient.)"""
    import neural_renderer_amd as nr
    B, S = 2, 64
    vertices, faces = _sphere(B, 2)
    vertices.requires_grad_(True)
    r = _renderer('look_at', S)
    r.soft_sigma = 1e-3
    target = torch.zeros((B, S, S), device='cuda')
    out = torch.zeros((B, S, S), device='cuda')

    def step():
        img = r.render_soft_silhouettes(vertices, faces)
        out.copy_(img)
        return torch.autograd.grad(nr.silhouette_iou_loss(img, target).sum(), [vertices])
    with torch.no_grad():
        r.render_soft_silhouettes(vertices, faces)
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        target[:, 20:50, 10:40] = 1
    replay()
    torch.cuda.synchronize()
    got_img, got = out.clone(), [g.clone() for g in grads[0]]
    eager = step()
    assert torch.equal(got_img, out) and (out > 0.5).any()
    for a, b in zip(got, eager):
        assert b.abs().sum() > 0
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 7. the example

def test_example_soft_silhouette_runs():
    """examples/example_soft_silhouette.py as a child process with 30 steps: it exits 0, its last printed loss is below its
    first, and it reports the hard silhouette's zero gradient."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_soft_silhouette.py'), '30'], cwd=root, env=env,
                         capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('soft step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
    assert 'hard silhouette: vertex gradient exactly zero at step 0: True' in run.stdout
