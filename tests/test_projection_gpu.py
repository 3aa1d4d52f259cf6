"""camera_mode = 'projection' on the GPU: the fused HIP front-end (nr_frontend_{forward,backward}_projection) against the
torch module path, a known answer that also pins the image orientation, the look_at camera restated as a projection, the
face_light path, sharding, routing, and a pose-fitting loop.

Tolerances are those of tests/test_frontend_gpu.py: projected faces rtol 1e-5 / atol 2e-6, lit textures rtol 1e-6 /
atol 1e-7, gradients H.rel_err <= 1e-4 (float atomics in the face -> vertex scatter, per-image sums in another order).
Distortion needs no wider forward bound: the kernel (built with -ffp-contract=off and correctly rounded division) and
projection.py evaluate x'' and y'' with the same IEEE float32 operations in the same order, so those terms add no
difference of their own.  They only carry the difference in c = R w + t (matmul order) through their Jacobian, which
stays within 1 +- 0.3 on the cameras of projection_ref.camera.  Measured on an MI355X, as a fraction of the bound, over
the 16 cases of test_fused_projection_matches_torch: faces 0.054 without distortion and 0.060 with it; lit textures
0.37; gradients 0.35 to 0.70.  The closest case is per-image, fill_back, textured, at 0.70.
"""
import math

import numpy as np
import pytest
import torch

import helpers as H
import projection_ref as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4
LIGHT_ORDER = 1e-6  # tests/test_face_light_gpu.py
GRAD_TOL = 1e-5


def _renderer(cam, S=256, fill_back=True):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.camera_mode = 'projection'
    r.K, r.R, r.t, r.dist_coeffs = cam
    r.orig_size = S
    r.fill_back = fill_back
    r.light_direction = [0.3, 0.8, -0.5]
    r.light_color_ambient = [1.0, 0.9, 0.8]
    r.light_color_directional = [0.7, 1.0, 0.6]
    r.light_intensity_ambient = 0.4
    r.light_intensity_directional = 0.6
    return r


def _scene(B, ts, seed):
    rng = np.random.default_rng(seed)
    v, f = H.teapot()
    vb = (v[None] + rng.normal(scale=0.01, size=(B,) + v.shape)).astype(np.float32)
    fb = np.repeat(f[None], B, axis=0)
    tex = rng.uniform(0, 1, (B, f.shape[0], ts, ts, ts, 3)).astype(np.float32)
    return vb, fb, tex


def _cuda(x, grad=False):
    return None if x is None else torch.tensor(x, device='cuda', requires_grad=grad)


def test_known_answer_and_orientation():
    """A small triangle at camera depth 2 whose centroid projects to (u, v) = (10.5, 3.5): the centre of column 10 and of
    row 3 counted from the top.  Fails without the projection mode (the raw vertices would be drawn)."""
    import neural_renderer_amd as nr
    S, f, c = 32, 32.0, 16.0
    K = [[f, 0, c], [0, f, c], [0, 0, 1]]
    z = 2.0
    xc, yc, h = (10.5 - c) / f * z, (3.5 - c) / f * z, 1.5 / f * z  # h: 1.5 pixels
    tri = np.array([[[xc - h, yc - h, z], [xc + h, yc - h, z], [xc, yc + 2 * h, z]]], np.float32)  # centroid (xc, yc)
    v = torch.tensor(tri, device='cuda')
    fi = torch.tensor([[[0, 1, 2]]], dtype=torch.int32, device='cuda')
    r = nr.Renderer()
    r.camera_mode = 'projection'
    r.K, r.R, r.t, r.orig_size = K, np.eye(3), [0, 0, 0], S
    r.image_size, r.anti_aliasing = S, False
    sil = r.render_silhouettes(v, fi)[0].cpu().numpy()
    assert r.last_frontend == 'fused'
    assert sil[3, 10] == 1 and sil[28, 10] == 0 and sil[3, 21] == 0  # not flipped vertically or horizontally
    assert 3 <= sil.sum() <= 20 and sil[:, :6].sum() == 0 and sil[12:].sum() == 0
    depth = r.render_depth(v, fi)[0].cpu().numpy()
    assert abs(float(depth[3, 10]) - 2.0) <= 1e-6


def test_projection_equals_look_at_camera():
    """R = diag(1,-1,1) R_lookat(eye), t = -R eye, f = orig_size / (2 tan(30 deg)), c = orig_size / 2: the look_at +
    perspective faces of the teapot batch."""
    import neural_renderer_amd as nr
    from neural_renderer_amd import frontend
    from neural_renderer_amd._util import normalize
    B, S = 4, 256
    vb, fb, _ = _scene(B, 2, seed=21)
    eyes = np.array([O.get_points_from_angles(2.732, 20.0 + 5 * i, 70.0 * i) for i in range(B)], np.float32)
    e = torch.tensor(eyes)
    zax = normalize(-e)
    xax = normalize(torch.cross(torch.tensor([[0., 1., 0.]]).expand(B, 3), zax, dim=1))
    yax = normalize(torch.cross(zax, xax, dim=1))
    R = torch.stack((xax, -yax, zax), dim=1)
    t = -torch.matmul(R, e[:, :, None])[:, :, 0]
    tan = np.tan(np.float32(30) / np.float32(180) * np.float32(3.1416), dtype=np.float32)
    fl = np.float32(S) / (np.float32(2) * tan)
    K = np.array([[fl, 0, S / 2], [0, fl, S / 2], [0, 0, 1]], np.float32)
    v, f = torch.tensor(vb, device='cuda'), torch.tensor(fb, device='cuda')

    r0 = nr.Renderer()
    r0.eye = torch.tensor(eyes, device='cuda')
    r1 = _renderer((K, R.cuda(), t.cuda(), None), S)
    assert frontend.fusable(r0, v, f, None) and frontend.fusable(r1, v, f, None)
    faces0, _ = frontend.project_and_light(r0, v, f)
    faces1, _ = frontend.project_and_light(r1, v, f)
    np.testing.assert_allclose(faces1.cpu().numpy(), faces0.cpu().numpy(), rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize('textured', [True, False])
@pytest.mark.parametrize('fill_back', [True, False])
@pytest.mark.parametrize('distortion', [True, False])
@pytest.mark.parametrize('per_image', [True, False])
def test_fused_projection_matches_torch(per_image, distortion, fill_back, textured):
    from neural_renderer_amd import frontend
    B = 3
    vb, fb, tex = _scene(B, 2, seed=31)
    cam = P.camera(B, seed=32, per_image=per_image, distortion=distortion)
    rng = np.random.default_rng(33)

    def run(fused):
        v = _cuda(vb, True)
        t = _cuda(tex, True) if textured else None
        K, R, tt = (_cuda(x, True) for x in cam[:3])
        r = _renderer((K, R, tt, cam[3]), fill_back=fill_back)
        f = torch.tensor(fb, device='cuda')
        assert frontend.fusable(r, v, f, t)
        faces, lit = frontend.project_and_light(r, v, f, t) if fused else r._frontend_torch(v, f, t)
        return (v, t, K, R, tt), faces, lit

    p1, faces1, lit1 = run(True)
    p0, faces0, lit0 = run(False)
    assert faces1.shape == faces0.shape
    np.testing.assert_allclose(faces1.detach().cpu().numpy(), faces0.detach().cpu().numpy(), rtol=1e-5, atol=2e-6)
    outs1, outs0 = [faces1], [faces0]
    grads = [torch.tensor(rng.normal(size=tuple(faces0.shape)).astype(np.float32), device='cuda')]
    if textured:
        np.testing.assert_allclose(lit1.detach().cpu().numpy(), lit0.detach().cpu().numpy(), rtol=1e-6, atol=1e-7)
        outs1.append(lit1)
        outs0.append(lit0)
        grads.append(torch.tensor(rng.normal(size=tuple(lit0.shape)).astype(np.float32), device='cuda'))
    else:
        assert lit1 is None and lit0 is None
    torch.autograd.backward(outs1, grads)
    torch.autograd.backward(outs0, grads)
    for name, a, b in zip(('vertices', 'textures', 'K', 'R', 't'), p1, p0):
        if a is None:
            continue
        assert a.grad.shape == b.grad.shape, name
        err = H.rel_err(a.grad.cpu().numpy(), b.grad.cpu().numpy())
        assert err <= RTOL, (name, err)
    assert float(p1[2].grad[..., 2, :].abs().max()) == 0  # row 2 of K is not used


@pytest.mark.parametrize('per_image', [True, False])
def test_face_light_path(per_image):
    """At texture size 3 render() takes the face_light front-end (nr_frontend_forward_projection with light_out); it
    matches face_light = False within the tolerances of tests/test_face_light_gpu.py."""
    import neural_renderer_amd as nr
    B, S, ts = 3, 128, 3
    vb, fb, tex = _scene(B, ts, seed=41)
    cam = P.camera(B, seed=42, per_image=per_image, orig_size=S)
    rng = np.random.default_rng(43)
    up = torch.tensor(rng.normal(size=(B, 3, S, S)).astype(np.float32), device='cuda')
    res = []
    for flag in (None, False):
        v, t = _cuda(vb, True), _cuda(tex, True)
        K, R, tt = (_cuda(x, True) for x in cam[:3])
        r = _renderer((K, R, tt, cam[3]), S)
        r.image_size = S
        r.face_light = flag
        if flag is None:
            assert r._use_face_light(v, torch.tensor(fb, device='cuda'), t)
        img = r.render(v, torch.tensor(fb, device='cuda'), t)
        assert r.last_frontend == 'fused'
        (img * up).sum().backward()
        res.append((img, v.grad, t.grad, K.grad, R.grad, tt.grad))
    assert float(res[1][0].detach().abs().max()) > 0.1

    def close(a, b, tol, what):
        a = a.detach().cpu().numpy().astype(np.float64)
        b = b.detach().cpu().numpy().astype(np.float64)
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
        assert err <= tol, '%s: %.3g > %.3g' % (what, err, tol)

    close(res[0][0], res[1][0], LIGHT_ORDER, 'images')
    close(res[0][1], res[1][1], 1e-4, 'grad_vertices')
    close(res[0][2], res[1][2], GRAD_TOL, 'grad_textures')
    for k, name in ((3, 'grad_K'), (4, 'grad_R'), (5, 'grad_t')):
        close(res[0][k], res[1][k], 1e-4, name)


def test_sharding_is_bit_exact():
    """Per-image K, R, t, dist_coeffs: a batch of 4 and its two halves give the same faces bit for bit."""
    from neural_renderer_amd import frontend
    B = 4
    vb, fb, _ = _scene(B, 2, seed=51)
    K, R, t, d = P.camera(B, seed=52)

    def faces(sl):
        r = _renderer((_cuda(K[sl]), _cuda(R[sl]), _cuda(t[sl]), _cuda(d[sl])))
        v, f = _cuda(vb[sl]), torch.tensor(fb[sl], device='cuda')
        assert frontend.fusable(r, v, f, None)
        return frontend.project_and_light(r, v, f)[0]

    full = faces(slice(0, 4))
    assert torch.equal(full, torch.cat((faces(slice(0, 2)), faces(slice(2, 4))), dim=0))


def test_routing():
    from neural_renderer_amd import frontend
    B, S = 2, 64
    vb, fb, tex = _scene(B, 2, seed=61)
    K, R, t, d = P.camera(B, seed=62, orig_size=S)
    v, f, tx = _cuda(vb, True), torch.tensor(fb, device='cuda'), _cuda(tex)
    r = _renderer((_cuda(K), _cuda(R), _cuda(t[:, None, :]), _cuda(d)), S)
    r.image_size, r.eye = S, None  # the projection mode does not look at eye
    assert frontend.fusable(r, v, f, tx)
    r.K, r.R, r.t, r.dist_coeffs = K.tolist(), R, t[0].tolist(), d[0]  # array-likes
    assert frontend.fusable(r, v, f, tx)
    for bad in (dict(K=_cuda(K).double()), dict(R=torch.tensor(R)), dict(t=np.zeros((B + 1, 3))), dict(orig_size=0),
                dict(orig_size=None), dict(K=None)):
        r2 = _renderer((r.K, r.R, r.t, r.dist_coeffs), S)
        for k, val in bad.items():
            setattr(r2, k, val)
        assert not frontend.fusable(r2, v, f, tx), bad
    dist = _cuda(d, True)
    r.dist_coeffs = dist
    assert not frontend.fusable(r, v, f, tx)
    img = r.render(v, f, tx)
    assert r.last_frontend == 'torch'
    img.square().sum().backward()
    assert dist.grad is not None and torch.isfinite(dist.grad).all() and float(dist.grad.abs().max()) > 0


def _rodrigues(a):
    th = torch.sqrt((a * a).sum())
    k = a / th
    z = torch.zeros((), device=a.device)
    Kx = torch.stack((torch.stack((z, -k[2], k[1])), torch.stack((k[2], z, -k[0])), torch.stack((-k[1], k[0], z))))
    return torch.eye(3, device=a.device) + torch.sin(th) * Kx + (1 - torch.cos(th)) * (Kx @ Kx)


POSE_STEPS = 150
POSE_FACTOR = 50.0


def test_pose_fitting_loop():
    """Fit R (axis-angle) and t to a teapot silhouette from a perturbed start with torch.optim.Adam on the silhouette MSE;
    the pose error |da| + |dt| falls by POSE_FACTOR within POSE_STEPS steps.  Measured on an MI355X: 0.4448 -> 0.00195
    after 150 steps, a factor of 228; POSE_FACTOR = 50 leaves a margin of 4.5."""
    import neural_renderer_amd as nr
    S = 128
    v, fc = H.teapot()
    v, fc = _cuda(v[None]), torch.tensor(fc[None], device='cuda')
    K = _cuda(np.array([[S, 0, S / 2], [0, S, S / 2], [0, 0, 1]], np.float32))
    a_true = torch.tensor([0.4, 0.6, 0.1], device='cuda')
    t_true = torch.tensor([0.0, 0.05, 2.7], device='cuda')
    r = nr.Renderer()
    r.camera_mode, r.K, r.orig_size, r.image_size = 'projection', K, S, S
    r.R, r.t = _rodrigues(a_true), t_true
    target = r.render_silhouettes(v, fc).detach()
    assert float(target.sum()) > 500

    a = (a_true + torch.tensor([0.12, -0.1, 0.08], device='cuda')).requires_grad_(True)
    t = (t_true + torch.tensor([0.08, -0.06, 0.25], device='cuda')).requires_grad_(True)
    opt = torch.optim.Adam([a, t], lr=0.01)

    def err():
        return float((a - a_true).norm() + (t - t_true).norm())

    e0 = err()
    for _ in range(POSE_STEPS):
        opt.zero_grad()
        r.R, r.t = _rodrigues(a), t
        loss = ((r.render_silhouettes(v, fc) - target) ** 2).mean()
        loss.backward()
        opt.step()
        assert r.last_frontend == 'fused'
    e1 = err()
    print('pose error %.5f -> %.5f (factor %.1f) after %d steps' % (e0, e1, e0 / e1, POSE_STEPS))
    assert e1 * POSE_FACTOR <= e0, (e0, e1)
