"""The front-end kernels (csrc/nr_frontend.hip: nr_frontend_forward / _backward, their _light and _projection variants) and
nr_vertices_to_faces[_backward] on the GPU, entry by entry against the float64 restatement of tests/frontend_ref.py:

    |got - ref64| <= C u M + gamma(n - 1) M

with u = 2^-24, M the entry's own magnitude, n the number of addends that reach it (valence for grad_vertices, B for a camera
parameter the batch shares, 1 for everything that is stored) and C the constants of tests/test_frontend_ref.py, measured
there on the CPU from the restatement's own float32 error.  Any order of the float atomics stays inside the second term
(Higham), so the fan's vertex of valence 65 needs nothing special.  Entries with M = 0 -- the isolated vertex, row 2 of
grad_K -- must be equal.  No entry is masked.

Worst |got - ref64| as a fraction of the bound, measured on an MI355X over F.all_cases(), the partial requests and the calls
with one topology for the batch (every test prints its own per mesh and camera mode):
    faces_out 0.204   textures_out 0.207   light_out 0.172   grad_vertices 0.150   grad_textures 0.200
    grad_eye 0.194    grad_K 0.217         grad_R 0.214      grad_t 0.162
The constants are 4 x the restatement's own float32 error, so 0.25 is that error: the kernels round no worse than a NumPy
float32 evaluation of the header's formulas, in every case, and nothing had to be fixed in csrc/nr_frontend.hip.  The
largest fractions come from the single face (`one`); on the 1 280-face sphere the camera gradients, sums over 3 840 corners
that the kernels carry in double, stay below 0.01.
"""
import numpy as np
import pytest

import frontend_ref as F
import lights_ref
from test_frontend_ref import CONSTANTS, reference, run_module

pytestmark = pytest.mark.gpu

MODES = ('look_at', 'look', 'projection')


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device='cuda', requires_grad=grad)


def _fused(r, v, f, t, colors):
    from neural_renderer_amd import frontend
    assert frontend.fusable(r, v, f, t) and (not colors or frontend.light_fusable(r))
    return frontend.project_and_light_colors(r, v, f) if colors else frontend.project_and_light(r, v, f, t)


def _check(ratios, worst, case):
    for key, r in ratios.items():
        worst[key] = max(worst.get(key, 0.0), r)
        assert r <= 1, (case, key, r)


def _ratios(outs, grads, fw, adj, case):
    ratios = {}
    for key, got in outs.items():
        ref, M = fw[key]
        assert got.shape == ref.shape and got.dtype == np.float32, (case, key)
        ratios[key + '_out'] = F.worst_ratio(got, ref, M, 1, CONSTANTS[key + '_out'])
    for key, got in grads.items():
        ref, M, n = adj[key]
        assert got is not None and got.shape == ref.shape, (case, key)
        ratios[key] = F.worst_ratio(got, ref, M, n, CONSTANTS[key])
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# the main matrix

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', F.MESHES)
def test_kernels_against_the_restatement(name, mode):
    """frontend.project_and_light and project_and_light_colors over every case of the mesh under the cameras of the mode:
    both outputs and every gradient, entry by entry."""
    import torch
    worst = {}
    count = 0
    for case in F.all_cases():
        if case[0] != name or F.camera(case[1])['mode'] != mode:
            continue
        inp = F.case_inputs(case)
        fw, adj = reference(case)
        outs, grads = run_module(inp, _fused, torch.float32, 'cuda')
        assert sorted(grads) == sorted(adj), case
        _check(_ratios(outs, grads, fw, adj, case), worst, case)
        count += 1
    assert count >= 6
    print('front-end %s %s (%d cases): worst fraction of the bound %s'
          % (name, mode, count, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


def test_zero_normals_and_the_lone_vertex():
    """The odd mesh: a face whose normal is exactly zero gets the ambient colour Ia Ca in both copies, bit for bit, and sends
    the light's gradient nowhere; the vertex that no face names has a gradient of exactly 0."""
    import torch
    v, f = F.mesh('odd')
    w = v[:, f]
    flat = (np.cross(w[:, :, 0] - w[:, :, 1], w[:, :, 2] - w[:, :, 1]) == 0).all(-1)[0]
    lone = np.setdiff1d(np.arange(v.shape[1]), f)
    assert flat.sum() == 2 and lone.size == 1
    for cname in ('look_at_30', 'projection_mixed_dist'):
        inp = F.case_inputs(('odd', cname, 'colors', 0, True, False, 'host'))
        outs, grads = run_module(inp, _fused, torch.float32, 'cuda')
        L = inp['light']
        amb = np.float32(L['ia']) * np.asarray(L['ca'], np.float32)
        both = np.concatenate((flat, flat))
        assert outs['light'][:, both].tobytes() == np.broadcast_to(amb, (F.B, 4, 3)).astype(np.float32).tobytes(), cname
        assert (grads['vertices'][:, lone] == 0).all(), cname
        # a loss on the colours alone: the zero-normal faces' corners that no other face names get exactly 0
        outs, grads = run_module(dict(inp, g_faces=None), _fused, torch.float32, 'cuda', want=['vertices'])
        only_flat = np.setdiff1d(f[flat], f[~flat])
        assert only_flat.size >= 1 and (grads['vertices'][:, only_flat] == 0).all(), cname
        assert bool((grads['vertices'] != 0).any())


# ---------------------------------------------------------------------------------------------------------------------
# partial requests

def _recording(lib, fname, slots):
    """Replace lib.<fname> by a wrapper that records which of the result pointers `slots` = {name: position} were given."""
    real = getattr(lib, fname)
    calls = []

    def wrapper(*args):
        calls.append(tuple(sorted(n for n, i in slots.items() if args[i] is not None)))
        return real(*args)
    setattr(lib, fname, wrapper)
    return real, calls


PARTIAL = [
    # (camera, variant, the inputs that take a gradient, cotangents dropped, the results the backward call may carry)
    ('look_at_30', 'textures', ['eye'], (), ('eye', 'vertices')),           # (the camera sums come out of the vertex pass)
    ('look_at_ortho_shared', 'geometry', ['eye'], (), ('eye', 'vertices')),
    ('look', 'colors', ['eye'], (), ('eye', 'vertices')),
    ('look_at_30', 'textures', ['textures'], (), ('textures',)),
    ('projection_mixed_dist', 'textures', ['textures'], (), ('textures',)),
    ('look_at_30', 'textures', ['vertices'], ('g_faces',), ('vertices',)),  # a loss on the lit textures alone
    ('look_at_30', 'colors', ['vertices'], ('g_faces',), ('vertices',)),
    ('projection_mixed_dist', 'textures', ['vertices'], ('g_faces',), ('vertices',)),
    ('look_at_30', 'textures', ['vertices'], ('g_textures_out',), ('vertices',)),  # a loss on the faces alone
    ('look', 'colors', ['vertices'], ('g_light',), ('vertices',)),
    ('projection_per_image_dist', 'textures', ['vertices'], ('g_textures_out',), ('vertices',)),
    ('projection_mixed_dist', 'textures', ['K'], (), ('K', 'vertices')),
    ('projection_mixed_dist', 'colors', ['R'], (), ('R', 'vertices')),
    ('projection_shared', 'geometry', ['t'], (), ('t', 'vertices')),
    ('projection_t_b13_dist', 'textures', ['t', 'textures'], (), ('t', 'textures', 'vertices')),
]


@pytest.mark.parametrize('name', ['odd', 'fan'])
def test_partial_requests(name):
    """Only some inputs learnable, or a loss that reads one output alone: every gradient that comes back is held to its
    bound, and the backward call asks the kernels for nothing else."""
    import torch
    from neural_renderer_amd import _lib
    lib = _lib.load()
    worst = {}
    for cname, variant, want, dropped, allowed in PARTIAL:
        ts = 3 if variant == 'textures' else 0
        inp = F.case_inputs((name, cname, variant, ts, True, name == 'odd', 'host'))
        inp.update({k: None for k in dropped})
        proj = inp['cam']['mode'] == 'projection'
        fname = 'nr_frontend_backward_projection' if proj else \
            ('nr_frontend_backward_light' if variant == 'colors' else 'nr_frontend_backward')
        slots = {'vertices': 6, 'textures': 7, 'K': 8, 'R': 9, 't': 10} if proj else \
            ({'vertices': 5, 'eye': 6} if variant == 'colors' else {'vertices': 6, 'textures': 7, 'eye': 8})
        real, calls = _recording(lib, fname, slots)
        try:
            outs, grads = run_module(inp, _fused, torch.float32, 'cuda', want=want)
        finally:
            setattr(lib, fname, real)
        assert calls == [tuple(sorted(allowed))], (cname, variant, want, calls)
        adj = F.adjoint(inp['vertices'], inp['faces'], inp['textures'], inp['cam'], inp['light'], True, inp['g_faces'],
                        inp['g_textures_out'], inp['g_light'])
        assert sorted(grads) == sorted(want)
        fw = reference((name, cname, variant, ts, True, name == 'odd', 'host'))[0]
        _check(_ratios(outs, grads, fw, adj, (name, cname, variant, want, dropped)), worst, (name, cname, variant, want, dropped))
    print('front-end partial requests %s: worst fraction of the bound %s'
          % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI with one topology for the batch

def _c_call(inp, shared_topology):
    """Forward and backward of a case through the C entry points; the topology [Nf,3] with idx_per_batch = 0, or repeated
    to [B,Nf,3] with idx_per_batch = 1.  -> dict of numpy results with the restatement's names."""
    import torch
    from neural_renderer_amd import _lib
    lib = _lib.load()
    cam, L = inp['cam'], inp['light']
    f = np.asarray(inp['faces'], np.int32)
    assert f.ndim == 2
    B, Nv, Nf = F.B, inp['vertices'].shape[1], f.shape[0]
    fill_back = int(inp['fill_back'])
    Fo = Nf * (2 if fill_back else 1)
    idx = _cuda(f if shared_topology else np.repeat(f[None], B, axis=0))
    per = 0 if shared_topology else 1
    v = _cuda(inp['vertices'])
    tex = None if inp['textures'] is None else _cuda(inp['textures'])
    ts = 0 if tex is None else tex.shape[2]
    empty = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    faces_out = empty(B, Fo, 3, 3)
    tex_out = None if tex is None else empty(B, Fo, ts, ts, ts, 3)
    light_out = empty(B, Fo, 3) if inp['colors'] else None
    g_faces = _cuda(inp['g_faces'])
    g_tex = None if tex is None else _cuda(inp['g_textures_out'])
    g_light = _cuda(inp['g_light']) if inp['colors'] else None
    grad_v = empty(B, Nv, 3)
    grad_tex = None if tex is None else empty(*tex.shape)
    light = None
    if L is not None:
        light = _lib.Light(intensity_ambient=L['ia'], intensity_directional=L['id'])
        for n, k in (('color_ambient', 'ca'), ('color_directional', 'cd'), ('direction', 'dir')):
            for i in range(3):
                getattr(light, n)[i] = L[k][i]
    p = _lib.ptr
    res = {}
    keep = [idx, v]
    if cam['mode'] == 'projection':
        K, R = _cuda(cam['K']), _cuda(cam['R'])
        t = _cuda(np.asarray(cam['t']).reshape(-1, 3) if np.asarray(cam['t']).ndim == 3 else cam['t'])
        d = None if cam['dist'] is None else _cuda(cam['dist'])
        proj = _lib.Projection(K=K.data_ptr(), R=R.data_ptr(), t=t.data_ptr(), dist_coeffs=p(d), K_per_batch=int(K.dim() == 3),
                               R_per_batch=int(R.dim() == 3), t_per_batch=int(t.dim() == 2),
                               dist_per_batch=int(d is not None and d.dim() == 2), orig_size=cam['orig_size'])
        gK, gR, gt = (empty(*x.shape) for x in (K, R, t))
        nbytes = lib.nr_frontend_projection_workspace_bytes(B)
        assert nbytes == B * 18 * 8
        ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
        assert lib.nr_frontend_forward_projection(v.data_ptr(), idx.data_ptr(), p(tex), faces_out.data_ptr(), p(tex_out),
                                                  p(light_out), B, Nv, Nf, ts, per, fill_back, proj, light, None) == 0
        assert lib.nr_frontend_backward_projection(v.data_ptr(), idx.data_ptr(), p(tex), g_faces.data_ptr(), p(g_tex), p(g_light),
                                                   grad_v.data_ptr(), p(grad_tex), gK.data_ptr(), gR.data_ptr(), gt.data_ptr(),
                                                   B, Nv, Nf, ts, per, fill_back, proj, light, ws.data_ptr(), nbytes, None) == 0
        res.update(K=gK, R=gR, t=gt.reshape(np.shape(cam['t'])))
        keep += [K, R, t, d, ws]
    else:
        camera = _lib.Camera(mode=_lib.NR_CAMERA_LOOK_AT if cam['mode'] == 'look_at' else _lib.NR_CAMERA_LOOK,
                             perspective=int(cam['perspective']),
                             width=float(F.tan_width(cam['angle'])) if cam['perspective'] else 0.0)
        for i in range(3):
            camera.up[i] = F.UP[i]
            camera.target[i] = float(cam['direction'][i]) if cam['mode'] == 'look' else 0.0
        eye = _cuda(cam['eye'])
        eye_per = int(eye.dim() == 2)
        ge = empty(*eye.shape)
        nbytes = lib.nr_frontend_workspace_bytes(B)
        assert nbytes == B * 12 * 8
        ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
        if inp['colors']:
            assert lib.nr_frontend_forward_light(v.data_ptr(), idx.data_ptr(), eye.data_ptr(), faces_out.data_ptr(),
                                                 light_out.data_ptr(), B, Nv, Nf, per, eye_per, fill_back, camera, light, None) == 0
            assert lib.nr_frontend_backward_light(v.data_ptr(), idx.data_ptr(), eye.data_ptr(), g_faces.data_ptr(),
                                                  g_light.data_ptr(), grad_v.data_ptr(), ge.data_ptr(), B, Nv, Nf, per, eye_per,
                                                  fill_back, camera, light, ws.data_ptr(), nbytes, None) == 0
        else:
            assert lib.nr_frontend_forward(v.data_ptr(), idx.data_ptr(), p(tex), eye.data_ptr(), faces_out.data_ptr(), p(tex_out),
                                           B, Nv, Nf, ts, per, eye_per, fill_back, camera, light, None) == 0
            assert lib.nr_frontend_backward(v.data_ptr(), idx.data_ptr(), p(tex), eye.data_ptr(), g_faces.data_ptr(), p(g_tex),
                                            grad_v.data_ptr(), p(grad_tex), ge.data_ptr(), B, Nv, Nf, ts, per, eye_per,
                                            fill_back, camera, light, ws.data_ptr(), nbytes, None) == 0
        res['eye'] = ge
        keep += [eye, ws]
    torch.cuda.synchronize()
    res.update(faces_out=faces_out, vertices=grad_v)
    if tex is not None:
        res.update(textures_out=tex_out, textures=grad_tex)
    if inp['colors']:
        res['light_out'] = light_out
    del keep
    return {k: x.cpu().numpy() for k, x in res.items()}


@pytest.mark.parametrize('name', ['one', 'fan', 'odd'])
def test_one_topology_for_the_batch_through_the_c_abi(name):
    """idx_per_batch = 0, which the Python binding never passes: the six nr_frontend_* entry points and the two
    nr_vertices_to_faces* with a [Nf,3] topology.  What is stored -- faces_out, textures_out, light_out, grad_textures -- has
    the bits of the idx_per_batch = 1 call on the repeated topology; grad_vertices and the camera gradients are within their
    bounds of the restatement."""
    import torch
    from neural_renderer_amd import _lib
    lib = _lib.load()
    worst = {}
    for cname, variant, ts, fill_back in (('look_at_30', 'textures', 5, True), ('look_shared', 'geometry', 0, False),
                                          ('look_at_pole', 'colors', 0, True), ('projection_mixed_dist', 'textures', 1, True),
                                          ('projection_per_image', 'colors', 0, False), ('projection_shared_dist', 'geometry', 0, True)):
        case = (name, cname, variant, ts, fill_back, False, 'host')
        inp = F.case_inputs(case)
        one, rep = _c_call(inp, True), _c_call(inp, False)
        fw, adj = reference(case)
        for key in ('faces_out', 'textures_out', 'light_out', 'textures'):
            if key in one:
                assert np.isfinite(one[key]).all(), (case, key)  # every element stored
                assert one[key].tobytes() == rep[key].tobytes(), (case, key)
        outs = {k[:-4]: one[k] for k in ('faces_out', 'textures_out', 'light_out') if k in one}
        grads = {k: one[k] for k in adj}
        _check(_ratios(outs, grads, fw, adj, case), worst, case)
    # nr_vertices_to_faces / _backward
    v, f = F.mesh(name)
    B, Nv, Nf = F.B, v.shape[1], f.shape[0]
    g = lights_ref.upstream((B, Nf, 3, 3), seed=4)
    dv, dg = _cuda(v), _cuda(g)
    res = []
    for idx, per in ((_cuda(f), 0), (_cuda(np.repeat(f[None], B, axis=0)), 1)):
        out = torch.full((B, Nf, 3, 3), float('nan'), device='cuda')
        gv = torch.full((B, Nv, 3), float('nan'), device='cuda')
        assert lib.nr_vertices_to_faces(dv.data_ptr(), idx.data_ptr(), out.data_ptr(), B, Nv, Nf, per, None) == 0
        assert lib.nr_vertices_to_faces_backward(dg.data_ptr(), idx.data_ptr(), gv.data_ptr(), B, Nv, Nf, per, None) == 0
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), gv.cpu().numpy()))
    assert res[0][0].tobytes() == v[:, f].tobytes() and res[1][0].tobytes() == v[:, f].tobytes()
    ref, mag, n = _scatter_reference(g, np.repeat(f[None], B, axis=0), Nv)
    for out, gv in res:
        assert F.worst_ratio(gv, ref, mag, n, 0.0) <= 1
    print('front-end %s, one topology for the batch: worst fraction of the bound %s'
          % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------------------------------------------------
# properties of the bits

def _bit_cases(name):
    ts = F.TS[name][-1]
    return [(name, 'look_at_30', 'textures', ts, True, True, 'host'), (name, 'look', 'colors', 0, True, True, 'host'),
            (name, 'projection_per_image_dist', 'textures', ts, True, True, 'host'),
            (name, 'projection_t_b13_dist', 'colors', 0, True, True, 'host')]


@pytest.mark.parametrize('name', F.MESHES)
def test_bits(name):
    """No tolerance: the back copy of faces_out is the front copy with its corners reversed; two runs give the same forward
    bits; image b alone gives the forward outputs and the grad_textures it has inside the batch (every camera parameter one
    per image)."""
    import torch
    for case in _bit_cases(name):
        inp = F.case_inputs(case)
        want = ['textures'] if inp['textures'] is not None else ['vertices']
        outs, grads = run_module(inp, _fused, torch.float32, 'cuda', want=want)
        again, _ = run_module(inp, _fused, torch.float32, 'cuda', want=want)
        for key in outs:
            assert outs[key].tobytes() == again[key].tobytes(), (case, key)
        Nf = outs['faces'].shape[1] // 2
        assert outs['faces'][:, Nf:].tobytes() == np.ascontiguousarray(outs['faces'][:, :Nf, ::-1]).tobytes(), case
        for b in range(F.B):
            cam = {k: (x[b:b + 1] if k in ('eye', 'K', 'R', 't', 'dist') and x is not None else x) for k, x in inp['cam'].items()}
            alone = dict(inp, cam=cam, **{k: (None if inp[k] is None else inp[k][b:b + 1])
                                         for k in ('vertices', 'faces', 'textures', 'g_faces', 'g_textures_out', 'g_light')})
            o1, g1 = run_module(alone, _fused, torch.float32, 'cuda', want=want)
            for key in outs:
                assert o1[key].tobytes() == outs[key][b:b + 1].tobytes(), (case, b, key)
            if 'textures' in grads:
                assert g1['textures'].tobytes() == grads['textures'][b:b + 1].tobytes(), (case, b)


# ---------------------------------------------------------------------------------------------------------------------
# vertices_to_faces

def _scatter_reference(g, idx, Nv):
    """grad_vertices of the gather in float64, its sum of |g| and the number of addends per entry."""
    B = g.shape[0]
    ref, mag, n = np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3))
    where = (np.arange(B)[:, None, None], idx)
    np.add.at(ref, where, g.astype(np.float64))
    np.add.at(mag, where, np.abs(g.astype(np.float64)))
    np.add.at(n, where, 1.0)
    return ref, mag, n


@pytest.mark.parametrize('name', F.MESHES)
def test_vertices_to_faces_gather_and_scatter_entrywise(name):
    """nr.vertices_to_faces on the same meshes: the gather is bit-exact; every entry of the scatter is within
    gamma(n - 1) sum |g| of the float64 sum -- n its number of addends, 65 at the fan's centre --, and exact where n <= 1."""
    import neural_renderer_amd as nr
    v, f = F.mesh(name)
    idx = lights_ref.faces_per_image(f)
    x = _cuda(v, True)
    out = nr.vertices_to_faces(x, _cuda(idx))
    want = np.stack([v[b][idx[b]] for b in range(F.B)])
    assert out.detach().cpu().numpy().tobytes() == want.tobytes()
    g = lights_ref.upstream(want.shape, seed=5)
    out.backward(_cuda(g))
    ref, mag, n = _scatter_reference(g, idx, v.shape[1])
    got = x.grad.cpu().numpy()
    r = F.worst_ratio(got, ref, mag, n, 0.0)
    assert r <= 1, r
    single = n <= 1
    assert (got[single] == ref[single].astype(np.float32)).all()
    if name == 'fan':
        assert n[:, 0].max() == 65
    if name == 'odd':
        assert (n == 0).any()
