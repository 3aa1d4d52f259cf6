"""Texture cubes shared by the batch: `textures [1,Nf,ts,ts,ts,3]` beside `faces [B,F,3,3]`, B > 1 (include/nr_hip.h:
NR_FLAG_SHARED_TEXTURES, nr_backward_textures_shared).

The yardstick is the batched path on the same inputs -- the same cubes expanded to [B,Nf,...], as a leaf of its own so that
every image's gradient slice can be read -- which itself is held against the oracle (test_hip_parity.py,
test_face_light_gpu.py):

  * rgb, alpha and depth bit-identical: the forward does the same arithmetic from another base address;
  * grad_textures [1,Nf,...] against the batched slices summed in float64: |shared - sum_b batched_b| <= GRAD_TOL *
    max(sum_b |batched_b|).  GRAD_TOL = 1e-5 is the suite's tolerance for reduction-order-dependent gradients
    (test_hip_parity.SAME_TERMS, test_face_light_gpu.GRAD_TOL); it applies to the sum of magnitudes because each batched slice
    carries that error on its own;
  * grad_light and grad_faces within GRAD_TOL of the batched call's largest component.
"""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-5
LIGHT_ORDER = 1e-6  # test_face_light_gpu.LIGHT_ORDER: lit textures round light * texel per texel, face_light the sample


def _faces_scene(B, Nf, seed, ground=False):
    """Random small triangles in NDC (+ optionally one screen-filling triangle per image: more than BIG_PX candidates)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.8, 0.8, (B, Nf, 1, 2))
    xy = c + rng.uniform(-0.25, 0.25, (B, Nf, 3, 2))
    z = rng.uniform(1.0, 3.0, (B, Nf, 3, 1))
    f = np.concatenate((xy, z), axis=3).astype(np.float32)
    if ground:
        f[:, 0] = np.array([[-0.95, -0.9, 4.0], [0.95, -0.85, 4.5], [0.0, 0.95, 5.0]], np.float32)
    return f


def _upstream(rng, B, S):
    return {k: torch.tensor(rng.normal(size=s).astype(np.float32), device='cuda')
            for k, s in (('rgb', (B, 3, S, S)), ('alpha', (B, S, S)), ('depth', (B, S, S)))}


def _run(faces_np, tex_np, light_np, fill_back, shared, S, up, graph_replay=None):
    """tex_np [1,Nf,...].  -> (images, grad_faces, grad_textures, grad_light); grad_textures is [1,Nf,...] from the shared
    call and [B,Nf,...] -- a slice per image -- from the batched one."""
    import neural_renderer_amd as nr
    B = faces_np.shape[0]
    f0 = torch.tensor(faces_np, device='cuda', requires_grad=True)
    t0 = torch.tensor(tex_np, device='cuda')
    if not shared:
        t0 = t0.expand(B, *t0.shape[1:]).clone()
    t0.requires_grad_(True)
    l0 = torch.tensor(light_np, device='cuda', requires_grad=True) if light_np is not None else None
    faces = torch.cat((f0, f0.flip(2)), dim=1) if fill_back else f0
    out = nr.rasterize_rgbad(faces, t0, S, False, face_light=l0, graph_replay=graph_replay)
    loss = (out['rgb'] * up['rgb']).sum() + (out['alpha'] * up['alpha']).sum() + (out['depth'] * up['depth']).sum()
    loss.backward()
    return out, f0.grad, t0.grad, (l0.grad if l0 is not None else None)


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _close(a, b, tol, what):
    a, b = _f64(a), _f64(b)
    assert a.shape == b.shape, what
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    print('%s: %.3g (tolerance %.3g)' % (what, err, tol))
    assert err <= tol, '%s: %.3g > %.3g' % (what, err, tol)


def _texture_gradient_close(shared, batched, what='grad_textures'):
    """|shared - sum_b batched_b| <= GRAD_TOL * max(sum_b |batched_b|), the sums in float64."""
    s, b = _f64(shared), _f64(batched)
    assert s.shape == (1,) + b.shape[1:], (what, s.shape, b.shape)
    err = np.abs(s[0] - b.sum(axis=0)).max() / max(np.abs(b).sum(axis=0).max(), 1e-30)
    print('%s: %.3g (tolerance %.3g)' % (what, err, GRAD_TOL))
    assert np.isfinite(s).all() and err <= GRAD_TOL, '%s: %.3g > %.3g' % (what, err, GRAD_TOL)


def _compare(faces, tex, light, fill_back, S, seed):
    up = _upstream(np.random.default_rng(seed), faces.shape[0], S)
    o1, gf1, gt1, gl1 = _run(faces, tex, light, fill_back, True, S, up)
    o0, gf0, gt0, gl0 = _run(faces, tex, light, fill_back, False, S, up)
    for k in ('rgb', 'alpha', 'depth'):
        assert torch.equal(o1[k], o0[k]), k
    assert float(o0['alpha'].sum()) > 50  # the scene draws something
    _texture_gradient_close(gt1, gt0)
    _close(gf1, gf0, GRAD_TOL, 'grad_faces')
    assert float(gt0.abs().sum()) > 0 and float(gf0.abs().sum()) > 0
    if light is not None:
        _close(gl1, gl0, GRAD_TOL, 'grad_light')
        assert float(gl0.abs().sum()) > 0


CASES = [(2, True, False, 64), (2, True, True, 96), (2, False, False, 64), (4, True, True, 96), (3, False, True, 96),
         (6, True, False, 48), (9, True, False, 48), (13, False, False, 32)]


# every case with face_light; those without fill_back also without it (reversed copies share a cube only through face_light)
@pytest.mark.parametrize('ts,fill_back,ground,S,lit', [c + (True,) for c in CASES] + [c + (False,) for c in CASES if not c[1]])
def test_shared_cubes_equal_the_expanded_call(ts, fill_back, ground, S, lit):
    B, Nf = 3, 60
    rng = np.random.default_rng(300 + ts)
    faces = _faces_scene(B, Nf, 7 + ts, ground)
    tex = rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.2, 1.5, (B, 2 * Nf if fill_back else Nf, 3)).astype(np.float32) if lit else None
    _compare(faces, tex, light, fill_back, S, 301 + ts)


def test_many_images_few_faces():
    """More images than a wave has lanes, fewer faces than a workgroup has groups."""
    B, Nf, ts, S = 70, 8, 2, 32
    rng = np.random.default_rng(41)
    faces = _faces_scene(B, Nf, 42)
    tex = rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.2, 1.5, (B, 2 * Nf, 3)).astype(np.float32)
    _compare(faces, tex, light, True, S, 43)


def _shared_backward(faces, tex, light, S, up, before_backward=None):
    """One shared call with face_light and fill_back; -> (grad_textures, grad_light, grad_faces)."""
    import neural_renderer_amd as nr
    f0 = torch.tensor(faces, device='cuda', requires_grad=True)
    t0 = torch.tensor(tex, device='cuda', requires_grad=True)
    l0 = torch.tensor(light, device='cuda', requires_grad=True)
    out = nr.rasterize_rgbad(torch.cat((f0, f0.flip(2)), dim=1), t0, S, False, face_light=l0)
    loss = (out['rgb'] * up['rgb']).sum() + (out['alpha'] * up['alpha']).sum() + (out['depth'] * up['depth']).sum()
    if before_backward is not None:
        before_backward()
    loss.backward()
    return t0.grad, l0.grad, f0.grad


def test_cubes_that_own_no_pixel_store_zeros():
    """The gradient's memory holds NaN when the backward receives it: every element must be stored, exact zeros for the cubes
    whose faces are off screen in every image."""
    B, Nf, ts, S = 3, 60, 4, 64
    rng = np.random.default_rng(51)
    faces = _faces_scene(B, Nf, 52)
    gone = np.arange(20, 30)
    faces[:, gone, :, 0] += 10.0
    tex = rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.2, 1.5, (B, 2 * Nf, 3)).astype(np.float32)

    def poison():  # blocks of the gradient's and the scratch's sizes, handed back to the caching allocator full of NaN
        blocks = [torch.full((n,), float('nan'), device='cuda') for n in (Nf * ts ** 3 * 3, 2 * Nf * ts ** 3 * 3, B * 2 * Nf * 3)]
        torch.cuda.synchronize()
        del blocks

    gt, gl, gf = _shared_backward(faces, tex, light, S, _upstream(rng, B, S), poison)
    assert gt.shape == (1, Nf, ts, ts, ts, 3)
    assert bool(torch.isfinite(gt).all()) and bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gf).all())
    assert float(gt[0, gone].abs().max()) == 0.0
    assert float(gl[:, gone].abs().max()) == 0.0 and float(gl[:, Nf + gone].abs().max()) == 0.0
    assert float(gt.abs().sum()) > 0


def test_two_backward_calls_agree():
    """The double sums of the images arrive in no fixed order: rounded to float, two calls may differ by one ulp of the
    largest component (2^-22 of it allows for a component just below a power of two)."""
    B, Nf, ts, S = 3, 60, 4, 96
    rng = np.random.default_rng(61)
    faces = _faces_scene(B, Nf, 62, ground=True)
    tex = rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.2, 1.5, (B, 2 * Nf, 3)).astype(np.float32)
    up = _upstream(rng, B, S)
    a = _shared_backward(faces, tex, light, S, up)
    b = _shared_backward(faces, tex, light, S, up)
    for x, y, what in zip(a, b, ('grad_textures', 'grad_light', 'grad_faces')):
        diff = float((x - y).abs().max()) / float(y.abs().max())
        print('%s: two calls differ by %.3g of the largest component' % (what, diff))
        assert diff <= 2.0 ** -22, (what, diff)


def test_backward_memory_does_not_grow_with_the_batch():
    """Nothing the shared backward allocates has B * Nf * ts^3 elements: its peak lies below the batched backward's by at
    least half the batched gradient (gradient + double scratch are 3/8 of it at B = 8)."""
    import neural_renderer_amd as nr
    B, Nf, ts, S = 8, 600, 8, 64
    rng = np.random.default_rng(71)
    c = rng.uniform(-0.9, 0.9, (B, Nf, 1, 2))
    faces = np.concatenate((c + rng.uniform(-0.06, 0.06, (B, Nf, 3, 2)), rng.uniform(1.0, 3.0, (B, Nf, 3, 1))),
                           axis=3).astype(np.float32)
    tex = rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.2, 1.5, (B, Nf, 3)).astype(np.float32)
    up = torch.tensor(rng.normal(size=(B, 3, S, S)).astype(np.float32), device='cuda')
    peak, rise = {}, {}
    for shared in (True, False):
        f0 = torch.tensor(faces, device='cuda', requires_grad=True)
        t0 = torch.tensor(tex, device='cuda')
        if not shared:
            t0 = t0.expand(B, *t0.shape[1:]).clone()
        t0.requires_grad_(True)
        l0 = torch.tensor(light, device='cuda', requires_grad=True)
        loss = (nr.rasterize(f0, t0, S, False, face_light=l0) * up).sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        peak[shared] = torch.cuda.max_memory_allocated()
        rise[shared] = peak[shared] - held
        assert t0.grad.shape[0] == (1 if shared else B) and float(t0.grad.abs().sum()) > 0
        del f0, t0, l0, loss
    half = B * Nf * ts ** 3 * 3 * 4 // 2
    print('backward peak: shared %d, batched %d bytes; above what the forward holds: %d, %d; required difference %d'
          % (peak[True], peak[False], rise[True], rise[False], half))
    assert peak[False] - peak[True] >= half
    assert rise[False] - rise[True] >= half  # (the same without the inputs, which are B-fold in the batched call too)


def _teapot_views(B, ts, seed):
    rng = np.random.default_rng(seed)
    v, f = H.teapot()
    vb = (v[None] + rng.normal(scale=0.01, size=(B,) + v.shape)).astype(np.float32)
    tex = rng.uniform(0, 1, (1, f.shape[0], ts, ts, ts, 3)).astype(np.float32)
    eyes = np.array([O.get_points_from_angles(2.732, 20.0 + 5 * i, 70.0 * i) for i in range(B)], np.float32)
    return vb, np.repeat(f[None], B, axis=0), tex, eyes


@pytest.mark.parametrize('per_image_light', [False, True])
def test_renderer_shares_the_cubes(per_image_light):
    """Renderer.render with textures[0:1] against textures.expand(3, ...) with face_light = True.  With a light colour per image
    (a tensor) neither call fits the fused front-end: the shared call takes its colours from lighting() behind the
    module-by-module front-end, the expanded one falls back onto lit textures, whose light product is rounded per texel
    (LIGHT_ORDER, as in test_face_light_gpu.py) -- there the images agree to that order instead of bit for bit."""
    import neural_renderer_amd as nr
    B, ts = 3, 4
    vb, fb, tex, eyes = _teapot_views(B, ts, 81)
    rng = np.random.default_rng(82)
    up = torch.tensor(rng.normal(size=(B, 3, 32, 32)).astype(np.float32), device='cuda')
    res = []
    for shared in (True, False):
        r = nr.Renderer()
        r.image_size = 32
        r.eye = torch.tensor(eyes, device='cuda')
        r.light_direction = [0.3, 0.8, -0.5]
        r.light_intensity_ambient, r.light_intensity_directional = 0.4, 0.6
        if per_image_light:
            r.light_color_ambient = torch.tensor([[1.0, 0.9, 0.8], [0.8, 1.0, 0.9], [0.9, 0.8, 1.0]], device='cuda')
        r.face_light = True
        v = torch.tensor(vb, device='cuda', requires_grad=True)
        t = torch.tensor(tex, device='cuda')
        if not shared:
            t = t.expand(B, *t.shape[1:]).clone()
        t.requires_grad_(True)
        img = r.render(v, torch.tensor(fb, device='cuda'), t)
        assert r.last_frontend == ('torch' if per_image_light else 'fused')
        (img * up).sum().backward()
        res.append((img, v.grad, t.grad))
    assert float(res[1][0].abs().sum()) > 0
    if per_image_light:
        _close(res[0][0], res[1][0], LIGHT_ORDER, 'images')
    else:
        assert torch.equal(res[0][0], res[1][0])
    _texture_gradient_close(res[0][2], res[1][2])
    _close(res[0][1], res[1][1], GRAD_TOL, 'grad_vertices')


def test_shape_errors():
    import neural_renderer_amd as nr
    B, Nf = 3, 8
    f = torch.tensor(_faces_scene(B, Nf, 1), device='cuda')
    ff = torch.cat((f, f.flip(2)), dim=1)
    cubes = lambda b, n: torch.rand((b, n, 2, 2, 2, 3), device='cuda')
    with pytest.raises(ValueError):  # a batch of neither 1 nor B
        nr.rasterize(f, cubes(2, Nf), 32, False)
    with pytest.raises(ValueError):
        nr.rasterize(ff, cubes(2, Nf), 32, False, face_light=torch.ones((B, 2 * Nf, 3), device='cuda'))
    with pytest.raises(ValueError):  # [1,Nf,...] cubes, light colours of neither Nf nor 2 Nf faces
        nr.rasterize(torch.cat((f, f, f), dim=1), cubes(1, Nf), 32, False, face_light=torch.ones((B, 3 * Nf, 3), device='cuda'))
    with pytest.raises(ValueError):  # [1, 2 Nf, ...] cubes without light
        nr.rasterize(f, cubes(1, 2 * Nf), 32, False)


def test_graph_replay_runs_a_shared_call_eagerly():
    B, Nf, ts, S = 3, 40, 2, 32
    rng = np.random.default_rng(91)
    faces = _faces_scene(B, Nf, 92)
    tex = rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32)
    up = _upstream(rng, B, S)
    o1, gf1, gt1, _ = _run(faces, tex, None, False, True, S, up, graph_replay=True)
    o0, gf0, gt0, _ = _run(faces, tex, None, False, True, S, up, graph_replay=False)
    for k in ('rgb', 'alpha', 'depth'):
        assert torch.equal(o1[k], o0[k]), k
    assert gt1.shape == (1, Nf, ts, ts, ts, 3)
    _close(gt1, gt0, 2.0 ** -22, 'grad_textures')
    assert torch.equal(gf1, gf0)


def test_protocol_and_sampling_maps():
    """forward_gpu / backward_gpu return grad_textures [1,...]; the sampling maps of a shared call read as None."""
    import neural_renderer_amd as nr
    B, Nf, ts, S = 3, 40, 3, 32
    rng = np.random.default_rng(95)
    f = torch.tensor(_faces_scene(B, Nf, 96), device='cuda')
    t = torch.tensor(rng.uniform(0, 1, (1, Nf, ts, ts, ts, 3)).astype(np.float32), device='cuda')
    g = torch.tensor(rng.normal(size=(B, S, S, 3)).astype(np.float32), device='cuda')
    res = []
    for tex in (t, t.expand(B, *t.shape[1:]).contiguous()):
        fn = nr.Rasterize(S, 0.1, 100, 1e-3, (0, 0, 0), return_rgb=True)
        rgb, _, _ = fn.forward_gpu((f, tex))
        gf, gt = fn.backward_gpu((f, tex), (g, None, None))
        res.append((rgb, gf, gt, fn.sampling_index_map))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][3] is None and res[1][3] is not None
    _texture_gradient_close(res[0][2], res[1][2])
