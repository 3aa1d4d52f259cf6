"""Learnable lights on the GPU (include/nr_hip.h: nr_light_colors_forward / _backward; nr.Lights, nr.light_colors,
Renderer.lights): the kernels against the float64 restatement within the constants of tests/test_lights.py, bit equality
with today's host light, reproducibility, what ctx.needs_input_grad saves, the renderer's paths, graph capture and the
example's first steps."""
import functools

import numpy as np
import pytest

import lights_ref as R
import vertex_ref
from test_lights import CONSTANTS, run_torch_like, to_lights

pytestmark = pytest.mark.gpu


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device='cuda', requires_grad=grad)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(light, its M, the adjoint with its M) in float64: computed once per case, read only."""
    name, per_batch, layout, with_sh, fill_back, smooth = case
    v, faces, P, g = R.case_inputs(*case)
    return R.light(v, faces, P, fill_back, smooth) + (R.adjoint(v, faces, P, fill_back, smooth, g),)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels against the restatement

@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('name', R.MESHES)
def test_kernels_against_the_restatement(name, smooth):
    """Forward and every gradient within C u M of the float64 restatement, over every variant of the mesh: fill_back on and
    off, faces [Nf,3] and [B,Nf,3], the three parameter layouts, sh given and None; upstream weights that differ per image."""
    import neural_renderer_amd as nr
    import torch
    worst = {n: 0.0 for n in CONSTANTS}
    for case in R.all_cases():
        if case[0] != name or case[5] != smooth:
            continue
        _, per_batch, layout, with_sh, fill_back, _ = case
        v, faces, P, g = R.case_inputs(*case)
        out, grads = run_torch_like(nr.light_colors, v, faces, P, fill_back, smooth, g, torch.float32, 'cuda', implementation='hip')
        ref, mag, adj = _reference(case)
        assert out.shape == ref.shape and out.dtype == np.float32
        ratios = {'light': R.worst_ratio(out, ref, mag)}
        for n, got in grads.items():
            assert got.shape == adj[n][0].shape, (case, n)
            ratios[n] = R.worst_ratio(got, adj[n][0], adj[n][1])
        for n, r in ratios.items():
            worst[n] = max(worst[n], r)
            assert r <= CONSTANTS[n], (case, n, r)
    print('lights %s %s: worst ratios %s' % (name, 'smooth' if smooth else 'flat',
                                             ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------------------------------------------------
# bit equality with the host light

@pytest.mark.parametrize('ia,idir', [(0.45, 0.6), (0.0, 0.6), (0.45, 0.0)])
@pytest.mark.parametrize('smooth', [False, True])
def test_equals_the_host_light(smooth, ia, idir):
    """sh = None and tensor parameters that hold a host light's values: light_colors is vertex_light(..., smooth) -- flat: its
    three equal corners -- and grad_vertices is _VertexShade's for white colours, bit for bit with non-zero intensities
    (the same operations in the same order); with an intensity of 0 the host path skips a term that this one evaluates,
    and the results are equal by value (0 against -0).  The flat upstream sits on corner 0 of every face, so that the host
    path's sum over the corners adds zeros."""
    import neural_renderer_amd as nr
    import torch
    host = dict(intensity_ambient=ia, intensity_directional=idir, color_ambient=[0.9, 0.8, 1.0],
                color_directional=[1.0, 0.7, 0.85], direction=[0.3, 0.8, -0.45])
    for name in ('ico1', 'odd', 'ico3'):
        v, f = R.mesh(name, R.MESH_SEED[name])
        for per_batch in (False, True):
            faces = _cuda(R.faces_per_image(f) if per_batch else f)
            for fill_back in (True, False):
                F = (2 if fill_back else 1) * f.shape[0]
                x1, x2 = _cuda(v, True), _cuda(v, True)
                lights = nr.Lights(**host).cuda()
                mine = nr.light_colors(x1, faces, lights, fill_back=fill_back, smooth=smooth, implementation='hip')
                theirs = nr.vertex_light(x2, faces, fill_back=fill_back, smooth=smooth, implementation='hip', **host)
                want = theirs if smooth else theirs[:, :, 0]
                if not smooth:
                    assert torch.equal(theirs[:, :, 1], want) and torch.equal(theirs[:, :, 2], want)
                w = _cuda(R.upstream((R.B, F, 3, 3) if smooth else (R.B, F, 3), seed=3))
                wc = w if smooth else torch.cat((w[:, :, None], torch.zeros((R.B, F, 2, 3), device='cuda')), dim=2)
                g1, = torch.autograd.grad((mine * w).sum(), x1)
                g2, = torch.autograd.grad((theirs * wc).sum(), x2)
                key = (name, per_batch, fill_back)
                if ia != 0 and idir != 0:
                    assert mine.detach().cpu().numpy().tobytes() == want.detach().cpu().numpy().tobytes(), key
                    assert torch.equal(g1, g2), key
                    assert bool((g1 != 0).any())
                else:
                    assert torch.equal(mine, want) and torch.equal(g1, g2), key


# ---------------------------------------------------------------------------------------------------------------------
# the same bits

def _all_outputs(v, faces, P, fill_back, smooth, g):
    import neural_renderer_amd as nr
    import torch
    out, grads = run_torch_like(nr.light_colors, v, faces, P, fill_back, smooth, g, torch.float32, 'cuda', implementation='hip')
    return dict(grads, light=out)


@pytest.mark.parametrize('smooth', [False, True])
def test_two_runs_and_an_image_alone_give_the_same_bits(smooth):
    """No atomics: two runs agree in every bit of every output, and image b alone gives the bits it has inside the batch --
    its light, its grad_vertices and its parameter gradients (every parameter one per image)."""
    for name in ('ico3', 'odd'):
        case = (name, True, 'per_image', True, True, smooth)
        v, faces, P, g = R.case_inputs(*case)
        first, second = _all_outputs(v, faces, P, True, smooth, g), _all_outputs(v, faces, P, True, smooth, g)
        assert sorted(first) == sorted(('light', 'vertices') + R.NAMES)
        for n in first:
            assert first[n].tobytes() == second[n].tobytes(), (name, n)
        for b in range(R.B):
            alone = _all_outputs(v[b:b + 1], faces[b:b + 1], {n: p[b:b + 1] for n, p in P.items()}, True, smooth, g[b:b + 1])
            for n in first:
                assert alone[n].tobytes() == first[n][b:b + 1].tobytes(), (name, b, n)


# ---------------------------------------------------------------------------------------------------------------------
# needs_input_grad

def test_backward_work_follows_needs_input_grad():
    """With only sh learnable the backward call carries no grad_vertices (the vertex kernels are not launched) and asks for
    the SH sums alone; with nothing learnable no backward call happens at all."""
    import neural_renderer_amd as nr
    import torch
    from neural_renderer_amd import _lib
    lib = _lib.load()
    real = lib.nr_light_colors_backward
    calls = []

    def counting(*args):
        grads = args[7]
        calls.append((args[6] is not None, tuple(n for n in R.NAMES if getattr(grads, n))))
        return real(*args)
    v, f = R.mesh('ico1')
    faces = _cuda(f)
    P = R.params('mixed', True)
    try:
        lib.nr_light_colors_backward = counting
        for smooth in (False, True):
            del calls[:]
            scale = torch.ones(3, device='cuda', requires_grad=True)
            light = nr.light_colors(_cuda(v), faces, to_lights(P, device='cuda'), smooth=smooth, implementation='hip')
            assert not light.requires_grad
            (light * scale).sum().backward()
            assert calls == [] and bool(torch.isfinite(scale.grad).all())
            lights = to_lights(P, device='cuda', learnable=('sh',))
            nr.light_colors(_cuda(v), faces, lights, smooth=smooth, implementation='hip').sum().backward()
            assert calls == [(False, ('sh',))] and bool((lights.sh.grad != 0).any())
            x = _cuda(v, True)
            nr.light_colors(x, faces, lights, smooth=smooth, implementation='hip').sum().backward()
            assert calls[1:] == [(True, ('sh',))] and bool((x.grad != 0).any())
    finally:
        lib.nr_light_colors_backward = real


# ---------------------------------------------------------------------------------------------------------------------
# through the renderer

S, TS = 32, 4


def _scene():
    import neural_renderer_amd as nr
    rng = np.random.RandomState(11)
    v, f = vertex_ref.icosphere(1)
    v = np.stack((v, v * 0.9)).astype(np.float32) + rng.uniform(-0.02, 0.02, (2,) + v.shape).astype(np.float32)
    Nf, Nv = f.shape[0], v.shape[1]
    layout = nr.UVLayout(rng.uniform(0, 1, (Nf, 3, 2)).astype(np.float32), np.zeros(Nf, np.int32),
                         np.full((Nf, 2, 2, 2, 3), 0.5, np.float32), [(16, 24)])
    return dict(vertices=_cuda(v), faces=_cuda(f)[None].expand(2, -1, -1).contiguous(),
                cubes=_cuda(rng.uniform(0.1, 1, (2, Nf, TS, TS, TS, 3)).astype(np.float32)),
                uv=nr.UVImages(layout, [_cuda(rng.uniform(0, 1, (16, 24, 3)).astype(np.float32))]),
                vc=nr.VertexColors(_cuda(rng.uniform(0.2, 1, (Nv, 3)).astype(np.float32))), rng=rng)


def _renderer(shading='flat'):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.image_size = S
    r.shading = shading
    r.light_direction = [0.3, 0.8, -0.45]
    r.light_color_directional = [1.0, 0.7, 0.85]
    r.eye = _cuda(np.stack([nr.get_points_from_angles(2.732, 20, -60), nr.get_points_from_angles(2.5, -10, 100)]).astype(np.float32))
    return r


def test_renderer_with_lights_from_its_own_attributes():
    """lights = Lights.from_renderer(r) against the same renderer with lights = None: cubes (per image and shared by the
    batch; the reference renderer with face_light = True) and UVImages, flat and smooth, bit for bit; VertexColors within
    1 ulp of the largest colour (the product colours * light is torch's here, the kernel's there)."""
    import neural_renderer_amd as nr
    import torch
    sc = _scene()

    def pair(textures, shading, **attrs):
        ref, new = _renderer(shading), _renderer(shading)
        for k, val in attrs.items():
            setattr(ref, k, val)
        new.lights = nr.Lights.from_renderer(new).cuda()
        with torch.no_grad():
            a, b = ref.render(sc['vertices'], sc['faces'], textures), new.render(sc['vertices'], sc['faces'], textures)
        assert ref.last_frontend == 'fused' and new.last_frontend == 'fused'
        assert bool((a.flatten(1).max(1).values > 0.2).all())  # something is drawn in every image
        return a, b
    for textures in (sc['cubes'], sc['cubes'][:1]):
        a, b = pair(textures, 'flat', face_light=True)
        assert torch.equal(a, b)
    for shading in ('flat', 'smooth'):
        a, b = pair(sc['uv'], shading)
        assert torch.equal(a, b), shading
        a, b = pair(sc['vc'], shading)
        ulp = float(np.spacing(np.float32(a.max().item())))
        assert float((a - b).abs().max()) <= ulp, (shading, float((a - b).abs().max()), ulp)
    r = _renderer('smooth')
    r.lights = nr.Lights().cuda()
    with pytest.raises(ValueError):
        r.render(sc['vertices'], sc['faces'], sc['cubes'])
    # render_silhouettes and render_depth ignore the attribute
    plain = _renderer()
    assert torch.equal(r.render_silhouettes(sc['vertices'], sc['faces']), plain.render_silhouettes(sc['vertices'], sc['faces']))
    assert torch.equal(r.render_depth(sc['vertices'], sc['faces']), plain.render_depth(sc['vertices'], sc['faces']))


@pytest.mark.parametrize('source', ['vertex_colors_smooth', 'cubes_flat'])
def test_image_is_linear_in_sh(source):
    """For fixed geometry the image is linear in sh, so the autograd gradient of sum(w * image) with respect to sh[b, k, c]
    is sum(w * (render(sh = e_kc, every other term 0) - render(all 0))) over image b.  Within C u sum|terms| (C the sh
    constant), the terms being the pixels' w * difference."""
    import neural_renderer_amd as nr
    import torch
    sc = _scene()
    textures, shading = (sc['vc'], 'smooth') if source == 'vertex_colors_smooth' else (sc['cubes'], 'flat')
    r = _renderer(shading)
    w = _cuda(sc['rng'].uniform(-1, 1, (2, 3, S, S)).astype(np.float32))

    def render(sh, **kw):
        r.lights = nr.Lights(sh=sh, **kw).cuda()
        return r.render(sc['vertices'], sc['faces'], textures)
    sh = torch.tensor(sc['rng'].uniform(-0.3, 0.3, (2, 9, 3)).astype(np.float32))
    r.lights = nr.Lights(0.4, 0.6, direction=(0.3, 0.8, -0.45), sh=sh, learnable=('sh',)).cuda()
    (r.render(sc['vertices'], sc['faces'], textures) * w).sum().backward()
    got = r.lights.sh.grad.cpu().numpy().astype(np.float64)
    dark = dict(intensity_ambient=0.0, intensity_directional=0.0)
    with torch.no_grad():
        zero = render(torch.zeros(2, 9, 3), **dark).double()
        want, mag = np.zeros((2, 9, 3)), np.zeros((2, 9, 3))
        for k in range(9):
            for c in range(3):
                e = torch.zeros(2, 9, 3)
                e[:, k, c] = 1.0
                terms = w.double() * (render(e, **dark).double() - zero)
                want[:, k, c] = terms.flatten(1).sum(1).cpu().numpy()
                mag[:, k, c] = terms.abs().flatten(1).sum(1).cpu().numpy()
    ratio = R.worst_ratio(got, want, mag)
    print('linearity in sh, %s: worst ratio %.3f' % (source, ratio))
    assert (mag > 0).all() and ratio <= CONSTANTS['sh']


def test_graph_capture_equals_eager():
    """One captured step -- a smooth vertex-colour render under learnable lights and the gradients of the light -- replays
    equal to eager after the parameters were changed in place.  The eager render that comes first builds the adjacency
    table.  (The rasterizer sums the corner gradients of large faces with double atomics in no fixed order: the gradients
    agree to 1e-6 of their largest entry where they are not equal.)"""
    import neural_renderer_amd as nr
    import torch
    sc = _scene()
    r = _renderer('smooth')
    r.lights = nr.Lights(0.3, 0.6, direction=(0.3, 0.8, -0.45), sh=torch.zeros(2, 9, 3), learnable=('sh', 'direction',
                                                                                                   'intensity_ambient')).cuda()
    params = list(r.lights.parameters())
    w = torch.zeros((2, 3, S, S), device='cuda')
    out = torch.zeros((2, 3, S, S), device='cuda')

    def step():
        img = r.render(sc['vertices'], sc['faces'], sc['vc'])
        out.copy_(img)
        return torch.autograd.grad((img * w).sum(), params)
    with torch.no_grad():
        r.render(sc['vertices'], sc['faces'], sc['vc'])
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        r.lights.sh.copy_(_cuda(sc['rng'].uniform(-0.3, 0.3, (2, 9, 3)).astype(np.float32)))
        r.lights.direction.copy_(_cuda(np.array([0.5, 0.6, -0.3], np.float32)))
        w.copy_(_cuda(sc['rng'].normal(size=tuple(w.shape)).astype(np.float32)))
    replay()
    torch.cuda.synchronize()
    got_img, got = out.clone(), [g.clone() for g in grads[0]]
    eager = step()
    assert torch.equal(got_img, out) and bool((out != 0).any())
    for a, b in zip(got, eager):
        assert bool((b != 0).any())
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_example_lights_first_steps():
    """examples/example_lights.py: a few Adam steps on the SH coefficients and the lamp's direction stay finite and lower
    the loss."""
    import os
    import sys
    import torch
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import example_lights
    scene = example_lights.Scene(torch.device('cuda'), views=2, level=1, image_size=32)
    losses = example_lights.fit(scene, 8)
    print('example_lights: loss %.3e -> %.3e' % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert all(bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()) for p in scene.lights.parameters())
