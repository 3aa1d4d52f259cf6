"""Renderer.render_rgbad on the GPU (neural_renderer_amd/renderer.py): rgb, alpha and depth of one rasterization against
render, render_silhouettes and render_depth on every shading path, what a return_* = False skips, one forward entry point per
call, the gradient of a joint loss against two separate passes, and graph replay on the lit-texture path."""
import sys

import numpy as np
import pytest

import vertex_ref

pytestmark = pytest.mark.gpu

S, TS, B = 64, 4, 2
FORWARD_ENTRY_POINTS = ('nr_forward_rasterize', 'nr_forward_rasterize_lit', 'nr_forward_rasterize_uv',
                        'nr_forward_rasterize_uv_smooth', 'nr_forward_rasterize_corner', 'nr_forward_face_index_map')


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device='cuda', requires_grad=grad)


def _scene():
    """a level-2 icosphere (320 faces), two views, every shading source"""
    import neural_renderer_amd as nr
    rng = np.random.RandomState(23)
    v, f = vertex_ref.icosphere(2)
    v = np.stack((v, v * 0.85)).astype(np.float32) + rng.uniform(-0.02, 0.02, (B,) + v.shape).astype(np.float32)
    Nf, Nv = f.shape[0], v.shape[1]
    layout = nr.UVLayout(rng.uniform(0, 1, (Nf, 3, 2)).astype(np.float32), np.zeros(Nf, np.int32),
                         np.full((Nf, 2, 2, 2, 3), 0.5, np.float32), [(16, 24)])
    return dict(vertices=_cuda(v), faces=_cuda(f.astype(np.int32))[None].expand(B, -1, -1).contiguous(),
                cubes=_cuda(rng.uniform(0.1, 1, (B, Nf, TS, TS, TS, 3)).astype(np.float32)),
                uv=nr.UVImages(layout, [_cuda(rng.uniform(0.1, 1, (16, 24, 3)).astype(np.float32))]),
                vc=nr.VertexColors(_cuda(rng.uniform(0.2, 1, (Nv, 3)).astype(np.float32))))


def _renderer(**attrs):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.image_size = S
    r.light_direction = [0.3, 0.8, -0.45]
    r.light_color_directional = [1.0, 0.7, 0.85]
    r.eye = _cuda(np.stack([nr.get_points_from_angles(2.732, 20, -60), nr.get_points_from_angles(2.5, -10, 100)]).astype(np.float32))
    for k, val in attrs.items():
        setattr(r, k, val)
    return r


# name -> (renderer attributes, the scene's textures, lights?)
PATHS = {
    'cubes': (dict(face_light=False), 'cubes', False),
    'cubes_face_light': (dict(face_light=True), 'cubes', False),
    'shared_cubes': (dict(), 'shared', False),
    'uv_flat': (dict(shading='flat'), 'uv', False),
    'uv_smooth': (dict(shading='smooth'), 'uv', False),
    'vertex_colors_flat': (dict(shading='flat'), 'vc', False),
    'vertex_colors_smooth': (dict(shading='smooth'), 'vc', False),
    'lights': (dict(), 'cubes', True),
    'lights_uv_smooth': (dict(shading='smooth'), 'uv', True),
}


def _path(name, sc):
    import torch
    import neural_renderer_amd as nr
    attrs, tex, lights = PATHS[name]
    r = _renderer(**attrs)
    if lights:
        r.lights = nr.Lights(0.4, 0.6, direction=(0.3, 0.8, -0.45), sh=torch.full((9, 3), 0.05)).cuda()
    return r, (sc['cubes'][:1] if tex == 'shared' else sc[tex])


class _Counter(object):
    """counts the calls of the library's forward entry points and records the flags of every Rasterize call"""

    def __init__(self, monkeypatch):
        from neural_renderer_amd import _lib
        self.calls, self.flags = [], []
        lib = _lib.load()
        for n in FORWARD_ENTRY_POINTS:
            monkeypatch.setattr(lib, n, self._counting(n, getattr(lib, n)), raising=True)
        module = sys.modules['neural_renderer_amd.rasterize']   # (the package attribute `rasterize` is the function)
        real = module.Rasterize.__call__
        counter = self

        def call(fn, faces, textures=None, face_light=None):
            counter.flags.append((bool(fn.return_rgb), bool(fn.return_alpha), bool(fn.return_depth), textures is not None))
            return real(fn, faces, textures, face_light)
        monkeypatch.setattr(module.Rasterize, '__call__', call)

    def _counting(self, n, real):
        def call(*args):
            self.calls.append(n)
            return real(*args)
        return call

    def reset(self):
        del self.calls[:], self.flags[:]


@pytest.mark.parametrize('name', sorted(PATHS))
def test_forward_equals_the_three_renders(name, monkeypatch):
    """'rgb' is render()'s image, 'alpha' render_silhouettes' and 'depth' render_depth's (default near / far), bit for bit,
    from ONE call of a forward entry point; an output that is not asked for is None and the rasterizer is not asked for it."""
    import torch
    sc = _scene()
    r, textures = _path(name, sc)
    v, f = sc['vertices'], sc['faces']
    with torch.no_grad():
        want = r.render(v, f, textures), r.render_silhouettes(v, f), r.render_depth(v, f)
        assert bool((want[0].flatten(1).max(1).values > 0.2).all()) and bool((want[1].flatten(1).max(1).values == 1).all())
        count = _Counter(monkeypatch)
        out = r.render_rgbad(v, f, textures)
        assert len(count.calls) == 1 and count.flags == [(True, True, True, True)], (count.calls, count.flags)
        assert sorted(out) == ['alpha', 'depth', 'rgb']
        assert out['rgb'].shape == (B, 3, S, S) and out['alpha'].shape == (B, S, S) and out['depth'].shape == (B, S, S)
        assert torch.equal(out['rgb'], want[0]) and torch.equal(out['alpha'], want[1]) and torch.equal(out['depth'], want[2])
        for flags in ((True, True, False), (True, False, False), (False, True, True), (False, True, False), (False, False, True)):
            count.reset()
            calls_before = dict(r.frontend_calls)
            got = r.render_rgbad(v, f, textures, *flags)
            assert len(count.calls) == 1, (flags, count.calls)
            # the rasterizer's own flags: what is not asked for is not drawn; without rgb no shading source reaches it
            assert count.flags == [flags + (flags[0],)], (flags, count.flags)
            assert sum(r.frontend_calls.values()) == sum(calls_before.values()) + 1
            for key, flag, ref in zip(('rgb', 'alpha', 'depth'), flags, want):
                assert (got[key] is None) if not flag else torch.equal(got[key], ref), (flags, key)
        with pytest.raises(Exception):
            r.render_rgbad(v, f, textures, False, False, False)     # nothing to draw


def test_alpha_and_depth_take_the_renderers_near_far_and_eps(monkeypatch):
    """render_rgbad forwards near, far and rasterizer_eps, which render_silhouettes / render_depth do not (quirk Q2): the
    Rasterize behind it is built with them."""
    import torch
    sc = _scene()
    r, textures = _path('cubes', sc)
    r.near, r.far, r.rasterizer_eps = 2.0, 3.0, 2e-3
    module = sys.modules['neural_renderer_amd.rasterize']
    seen = []
    real = module.Rasterize.__init__

    def init(fn, image_size, near, far, eps, *args, **kw):
        seen.append((near, far, eps))
        return real(fn, image_size, near, far, eps, *args, **kw)
    monkeypatch.setattr(module.Rasterize, '__init__', init)
    with torch.no_grad():
        out = r.render_rgbad(sc['vertices'], sc['faces'], textures)
        r.render_silhouettes(sc['vertices'], sc['faces'])
    assert seen[0] == (2.0, 3.0, 2e-3) and seen[1][2] == 1e-4 and seen[1][:2] == (0.1, 100)
    assert bool((out['alpha'] > 0).any())


def test_graph_replay_on_the_lit_texture_path():
    """graph_replay = True (the lit-texture path: face_light off) gives the eager bits, forward and backward."""
    import torch
    import neural_renderer_amd as nr
    sc = _scene()
    results = []
    try:
        for replay in (False, True):
            r, textures = _path('cubes', sc)
            r.graph_replay = replay
            x = sc['vertices'].clone().requires_grad_(True)
            t = textures.clone().requires_grad_(True)
            out = r.render_rgbad(x, sc['faces'], t)
            (out['rgb'].sum() + 2 * out['alpha'].sum() + 0.5 * out['depth'].clamp(max=10).sum()).backward()
            results.append((out['rgb'].detach().clone(), out['alpha'].detach().clone(), out['depth'].detach().clone(),
                            x.grad.clone(), t.grad.clone()))
            assert r.last_frontend == 'fused'
    finally:
        sys.modules['neural_renderer_amd.rasterize'].clear_graph_replay_cache()
    for k in range(3):
        assert torch.equal(results[0][k], results[1][k]), k
    # the rasterizer's backward is the same kernels on the same maps; the front-end scatters the face gradients into the
    # vertices with float atomics in both modes, whose order differs from run to run: (n - 1) u of the sum of |terms| for
    # the n <= 16 corner terms of a vertex, which 64 u of the largest entry covers (as in
    # test_mesh_losses_gpu.test_regularisers_next_to_a_silhouette_loss)
    for k in (3, 4):   # (the texture gather may use float atomics too)
        assert float((results[0][k] - results[1][k]).abs().max()) <= 2.0 ** -18 * float(results[0][k].abs().max())
        assert bool(results[0][k].abs().sum() > 0)


@pytest.mark.parametrize('name', ['cubes', 'vertex_colors_smooth'])
def test_one_backward_equals_two_separate_passes(name):
    """One backward of rgb-loss + alpha-loss through render_rgbad against the sum of the gradients of two passes: render() with
    the rgb-loss, and rasterize_silhouettes(projected faces, eps = rasterizer_eps) with the alpha-loss (not
    render_silhouettes, whose backward runs with eps 1e-4: quirk Q2).

    The two losses are brightness and coverage, sum(w rgb) and sum(w' alpha) with positive per-pixel weights, on the default
    black background.  The rasterizer's approximate gradient takes a pixel pair's contribution only when the pair's COMBINED
    difference, sum over the channels of (colour difference) x (gradient), is positive (reference rasterize.py:647), so a
    joint pass is the sum of two passes exactly when the rgb and the alpha part of every pair agree in sign wherever the
    alpha part is not 0 -- which these losses guarantee: alpha differs only between a covered and an uncovered pixel, and
    there every colour channel differs the same way, the object being brighter than the background.  (A squared error to
    a target image has no such guarantee, and additivity is not a property of the operator for it.)

    The bound, as in test_mesh_losses_gpu.test_regularisers_next_to_a_silhouette_loss: the sum of two gradients is one
    float addition against autograd's accumulation in its own order, 2 u of the sum of the magnitudes on either side, 4 u =
    2^-22 of |part 1| + |part 2|; the front-end scatters its face gradients into the vertices with float atomics, whose
    order differs from run to run: up to (n - 1) u of the sum of |terms| for the n <= 16 corner terms of a vertex, which
    64 u = 2^-18 of the largest gradient entry covers with room for cancellation.  The rasterizer's K6 adds, per face, the
    pixel pairs' terms in float in one fixed order; the joint pass rounds each term once where the two passes round its
    two parts, n u of sum |terms| again, inside the same 2^-18 term."""
    import torch
    import neural_renderer_amd as nr
    sc = _scene()
    faces = sc['faces']
    rng = np.random.RandomState(5)
    w_rgb = _cuda(rng.uniform(0.5, 1.5, (B, 3, S, S)).astype(np.float32))
    w_alpha = _cuda(rng.uniform(0.5, 1.5, (B, S, S)).astype(np.float32))

    def leaf():
        return sc['vertices'].clone().requires_grad_(True)
    r, textures = _path(name, sc)
    x = leaf()
    out = r.render_rgbad(x, faces, textures, return_depth=False)
    ((out['rgb'] * w_rgb).sum() + (out['alpha'] * w_alpha).sum()).backward()
    x1 = leaf()
    (r.render(x1, faces, textures) * w_rgb).sum().backward()
    x2 = leaf()
    projected, _ = r._frontend(x2, faces)
    (nr.rasterize_silhouettes(projected, r.image_size, r.anti_aliasing, eps=r.rasterizer_eps) * w_alpha).sum().backward()
    parts = (x1.grad, x2.grad)
    assert all(bool(p.abs().sum() > 0) for p in parts)
    want, mags = parts[0] + parts[1], parts[0].abs() + parts[1].abs()
    err = (x.grad - want).abs()
    bound = 2.0 ** -22 * mags + 2.0 ** -18 * max(float(parts[0].abs().max()), float(parts[1].abs().max()))
    print('%s: joint backward against two passes: worst error %.3g, at %.3f of its bound; largest entries %.3g / %.3g'
          % (name, float(err.max()), float((err / bound).max()), float(parts[0].abs().max()), float(parts[1].abs().max())))
    assert bool((err <= bound).all())
