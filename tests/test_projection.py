"""camera_mode = 'projection' on the CPU: the torch module against its float64 restatement (tests/projection_ref.py), its
gradients, the Renderer's argument checks, the unchanged behaviour of the other camera modes, and the argument checks of
the C entry points (host only, no launch)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import projection_ref as P


def _teapot_batch(B, seed):
    rng = np.random.default_rng(seed)
    v, f = H.teapot()
    vb = (v[None] + rng.normal(scale=0.01, size=(B,) + v.shape)).astype(np.float32)
    return vb, np.repeat(f[None], B, axis=0)


@pytest.mark.parametrize('per_image', [True, False])
@pytest.mark.parametrize('distortion', [True, False])
def test_projection_matches_float64_restatement(per_image, distortion):
    """float32 torch against float64 NumPy: atol covers NDC coordinates near 0, where 2u - orig_size cancels."""
    import neural_renderer_amd as nr
    B, S = 3, 256.0
    vb, _ = _teapot_batch(B, 1)
    K, R, t, d = P.camera(B, seed=2, per_image=per_image, distortion=distortion, orig_size=S)
    got = nr.projection(torch.tensor(vb), torch.tensor(K), R, t.tolist(), d, orig_size=S).numpy()
    want = P.projection(vb, K, R, t, d, S)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6)
    assert np.abs(want[..., :2]).max() < 1.5  # the mesh is in view: the test covers the whole NDC range it uses
    if distortion:  # the distortion terms moved the points
        assert np.abs(want - P.projection(vb, K, R, t, None, S)).max() > 1e-3


def test_projection_t_layouts_and_names():
    import neural_renderer as nr_alias
    import neural_renderer_amd as nr
    assert nr_alias.projection is nr.projection and 'projection' in nr.__all__
    B = 2
    vb, _ = _teapot_batch(B, 3)
    K, R, t, _ = P.camera(B, seed=4)
    v = torch.tensor(vb)
    a = nr.projection(v, K, R, t, orig_size=64)
    b = nr.projection(v, K, R, t[:, None, :], orig_size=64)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        nr.projection(v, K, R, t)  # no orig_size
    with pytest.raises(ValueError):
        nr.projection(v, K[:, :2], R, t, orig_size=64)


def test_projection_gradcheck():
    import neural_renderer_amd as nr
    rng = np.random.default_rng(5)
    B, Nv = 2, 4
    K, R, t, d = P.camera(B, seed=6, orig_size=32.0)
    v = torch.tensor(rng.uniform(-0.5, 0.5, (B, Nv, 3)), dtype=torch.float64, requires_grad=True)
    args = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (K, R, t, d)]
    assert torch.autograd.gradcheck(lambda *a: nr.projection(*a, orig_size=32.0), (v, *args), eps=1e-6, atol=1e-5, rtol=1e-4)
    # shared parameters, no distortion
    args = [torch.tensor(x[0], dtype=torch.float64, requires_grad=True) for x in (K, R, t)]
    assert torch.autograd.gradcheck(lambda *a: nr.projection(*a, orig_size=32.0), (v, *args), eps=1e-6, atol=1e-5, rtol=1e-4)


def _renderer(mode):
    import neural_renderer_amd as nr
    r = nr.Renderer()
    r.camera_mode = mode
    return r


@pytest.mark.parametrize('missing', ['K', 'R', 't', 'orig_size'])
def test_renderer_projection_needs_its_parameters(missing):
    B = 2
    vb, fb = _teapot_batch(B, 7)
    K, R, t, _ = P.camera(B, seed=8)
    r = _renderer('projection')
    r.K, r.R, r.t, r.orig_size = K, R, t, 256
    setattr(r, missing, None)
    v, f = torch.tensor(vb), torch.tensor(fb)
    with pytest.raises(ValueError, match=missing):
        r._frontend_torch(v, f)
    with pytest.raises(ValueError):
        r._frontend(v, f)  # (CPU tensors: the torch path)


def test_renderer_projection_torch_path():
    """The projection mode of the torch front-end: projection() + fill_back + gather; perspective and viewing_angle unused."""
    import neural_renderer_amd as nr
    B = 2
    vb, fb = _teapot_batch(B, 9)
    K, R, t, d = P.camera(B, seed=10)
    r = _renderer('projection')
    r.K, r.R, r.t, r.dist_coeffs, r.orig_size = K, R, t, d, 256
    r.viewing_angle = 50
    faces, _ = r._frontend_torch(torch.tensor(vb), torch.tensor(fb))
    pv = P.projection(vb, K, R, t, d, 256)
    f_all = np.concatenate((fb, fb[:, :, ::-1]), axis=1)
    want = np.stack([pv[b][f_all[b]] for b in range(B)])
    np.testing.assert_allclose(faces.numpy(), want, rtol=2e-6, atol=1e-6)
    assert r.last_frontend is None  # (_frontend_torch is the module path itself)
    r.perspective = False
    faces2, _ = r._frontend_torch(torch.tensor(vb), torch.tensor(fb))
    assert torch.equal(faces, faces2)


@pytest.mark.parametrize('mode', ['look_at', 'none', 'something_else'])
def test_other_camera_modes_unchanged(mode):
    """look_at: look_at + perspective; any other string but 'look' / 'projection': perspective of the raw vertices."""
    import neural_renderer_amd as nr
    B = 2
    vb, fb = _teapot_batch(B, 11)
    r = _renderer(mode)
    r.K, r.R, r.t, r.orig_size = P.camera(B, seed=12)[:3] + (256,)  # set, but not used by these modes
    v, f = torch.tensor(vb), torch.tensor(fb)
    faces, _ = r._frontend_torch(v, f)
    vv = nr.look_at(v, r.eye) if mode == 'look_at' else v
    want = nr.vertices_to_faces(nr.perspective(vv, angle=30), torch.cat((f, f.flip(2)), dim=1))
    assert torch.equal(faces, want)


def test_projection_entry_point_argument_errors():
    """Host-side checks of the six nr_frontend_* entry points: they return before any launch.  Every case is rejected; where
    several arguments are wrong, the code that wins is pinned too (the entry points do not all check in the same order)."""
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert lib.nr_frontend_projection_workspace_bytes(4) == 4 * 18 * 8
    assert lib.nr_frontend_projection_workspace_bytes(0) == 0
    assert lib.nr_frontend_workspace_bytes(4) == 4 * 12 * 8
    assert lib.nr_frontend_workspace_bytes(0) == 0
    X = 4096  # stand-in device addresses: never dereferenced on the host
    proj = _lib.Projection(K=X, R=X, t=X, dist_coeffs=None, orig_size=64.0)
    light = _lib.Light()
    E_NULL, E_SIZE, E_WORKSPACE, E_MODE = -1, -2, -3, -4
    overflow = dict(B=65535, Nf=0x7fffffff // 18 // 65535 + 1)  # B * Nf above the kernels' int32 indexing

    def fwd(p=proj, textures=None, textures_out=None, light_out=None, lt=None, B=2, Nf=5, ts=2):
        return lib.nr_frontend_forward_projection(X, X, textures, X, textures_out, light_out, B, 10, Nf, ts, 1, 1,
                                                  p, lt, None)

    assert fwd(p=None) == -1
    assert fwd(p=_lib.Projection(K=X, R=X, t=None, orig_size=64.0)) == -1
    assert fwd(p=_lib.Projection(K=X, R=X, t=X, orig_size=0.0)) == -2
    assert fwd(p=_lib.Projection(K=X, R=X, t=X, orig_size=float('inf'))) == -2
    assert fwd(textures=X) == -4                                          # textures without textures_out
    assert fwd(textures=X, textures_out=X, light_out=X, lt=light) == -4   # two colour outputs
    assert fwd(light_out=X) == -1                                         # colours without a light
    assert fwd(textures=X, textures_out=X, lt=light, ts=0) == E_SIZE
    assert fwd(light_out=X, lt=light, **overflow) == E_SIZE
    assert fwd(textures=X, textures_out=X, light_out=X, lt=light, B=0) == E_MODE  # output checks before sizes
    assert fwd(p=None, B=0) == E_SIZE                                     # sizes before the camera
    assert fwd(p=_lib.Projection(K=X, R=X, t=X, orig_size=0.0), light_out=X) == E_SIZE  # the camera before the light

    def bwd(grad_vertices=X, grad_K=None, ws=X, ws_bytes=1 << 20, textures=None, g_light=None, lt=None, p=proj, B=2,
            grad_textures=None, g_tex_out=None):
        return lib.nr_frontend_backward_projection(X, X, textures, X, g_tex_out, g_light, grad_vertices, grad_textures, grad_K,
                                                   None, None, B, 10, 5, 2, 1, 1, p, lt, ws, ws_bytes, None)

    assert bwd(grad_vertices=None) == -4                  # nothing requested
    assert bwd(grad_vertices=None, grad_K=X) == -4        # camera sums need the vertex pass
    assert bwd(grad_K=X, ws_bytes=8) == -3                # workspace too small
    assert bwd(grad_K=X, ws=None) == -3
    assert bwd(textures=X, g_light=X, lt=light) == -4     # textures and colours are exclusive
    assert bwd(g_light=X) == -1                           # colours without a light
    assert bwd(grad_textures=X, textures=X, lt=light) == E_MODE  # grad_textures without grad_textures_out
    assert bwd(g_tex_out=X) == E_MODE                     # grad_textures_out without textures
    assert bwd(textures=X, g_light=X) == E_MODE           # exclusive outputs before the missing light
    assert bwd(g_light=X, grad_vertices=None) == E_MODE   # nothing requested before the missing light
    assert bwd(g_light=X, B=0) == E_NULL                  # the missing light before sizes
    assert bwd(textures=X, B=65536) == E_SIZE
    assert bwd(p=None, grad_K=X, ws=None) == E_NULL       # the camera before the workspace
    assert bwd(grad_K=X, ws=None, textures=X) == E_NULL   # the light before the workspace

    # look_at / look: the camera struct's mode is checked after sizes; these entry points do not take the projection mode
    cam = _lib.Camera(mode=_lib.NR_CAMERA_PROJECTION)
    assert lib.nr_frontend_forward(X, X, None, X, X, None, 2, 10, 5, 2, 1, 0, 1, cam, None, None) == -4
    look = _lib.Camera(mode=_lib.NR_CAMERA_LOOK_AT, perspective=1, width=0.5)

    def fwd_look(camera=look, textures=None, eye=X, faces_out=X, textures_out=None, lt=None, B=2, Nv=10, Nf=5, ts=2):
        return lib.nr_frontend_forward(X, X, textures, eye, faces_out, textures_out, B, Nv, Nf, ts, 1, 0, 1, camera, lt, None)

    assert fwd_look(camera=None) == E_NULL
    assert fwd_look(eye=None) == E_NULL
    assert fwd_look(faces_out=None, textures=X) == E_NULL
    assert fwd_look(textures_out=X) == E_MODE
    assert fwd_look(textures=X, textures_out=X) == E_NULL              # textures without a light
    assert fwd_look(camera=_lib.Camera(mode=7)) == E_MODE
    for bad in (dict(B=0), dict(B=65536), dict(Nv=0), dict(Nf=0), overflow):
        assert fwd_look(**bad) == E_SIZE
    assert fwd_look(textures=X, textures_out=X, lt=light, ts=0) == E_SIZE
    assert fwd_look(camera=cam, B=0) == E_SIZE                         # sizes before the camera's mode
    assert fwd_look(textures=X, Nv=0) == E_MODE                        # the output pair before sizes
    assert fwd_look(camera=cam, textures=X, textures_out=X) == E_MODE  # the camera's mode before the light

    def fwd_light(camera=look, eye=X, light_out=X, lt=light, B=2):
        return lib.nr_frontend_forward_light(X, X, eye, X, light_out, B, 10, 5, 1, 0, 1, camera, lt, None)

    assert fwd_light(light_out=None) == E_NULL
    assert fwd_light(light_out=None, B=0) == E_NULL
    assert fwd_light(lt=None) == E_NULL
    assert fwd_light(camera=cam, lt=None) == E_MODE
    assert fwd_light(camera=None, B=0) == E_SIZE
    assert fwd_light(B=65536) == E_SIZE

    def bwd_look(camera=look, textures=None, eye=X, g_tex_out=None, grad_vertices=X, grad_textures=None, grad_eye=None,
                 lt=None, ws=X, ws_bytes=1 << 20, B=2, ts=2):
        return lib.nr_frontend_backward(X, X, textures, eye, X, g_tex_out, grad_vertices, grad_textures, grad_eye, B, 10, 5, ts,
                                        1, 0, 1, camera, lt, ws, ws_bytes, None)

    assert bwd_look(eye=None) == E_NULL
    assert bwd_look(grad_vertices=None) == E_MODE                           # nothing requested
    assert bwd_look(grad_vertices=None, grad_eye=X) == E_MODE               # camera sums need the vertex pass
    assert bwd_look(grad_textures=X, textures=X, lt=light) == E_MODE        # grad_textures without grad_textures_out
    assert bwd_look(g_tex_out=X) == E_MODE                                  # grad_textures_out without textures
    assert bwd_look(textures=X) == E_NULL                                   # textures without a light
    assert bwd_look(camera=cam) == E_MODE
    assert bwd_look(grad_eye=X, ws=None) == E_WORKSPACE
    assert bwd_look(grad_eye=X, ws_bytes=4 * 12 * 8 - 1, B=4) == E_WORKSPACE
    assert bwd_look(textures=X, lt=light, ts=0) == E_SIZE
    assert bwd_look(grad_vertices=None, B=0) == E_MODE                      # argument checks before sizes
    assert bwd_look(grad_eye=X, ws=None, B=0) == E_SIZE                     # sizes before the workspace
    assert bwd_look(grad_eye=X, ws=None, camera=cam) == E_MODE              # the camera before the workspace
    assert bwd_look(grad_eye=X, ws=None, textures=X) == E_NULL              # the light before the workspace

    def bwd_light(camera=look, g_light=X, grad_vertices=X, grad_eye=None, lt=light, ws=X, ws_bytes=1 << 20, B=2):
        return lib.nr_frontend_backward_light(X, X, X, X, g_light, grad_vertices, grad_eye, B, 10, 5, 1, 0, 1, camera, lt, ws,
                                              ws_bytes, None)

    assert bwd_light(lt=None) == E_NULL
    assert bwd_light(lt=None, grad_vertices=None) == E_NULL  # here the missing light wins over every other check
    assert bwd_light(lt=None, B=0) == E_NULL
    assert bwd_light(grad_vertices=None) == E_MODE
    assert bwd_light(g_light=None, lt=None, grad_vertices=None) == E_MODE
    assert bwd_light(camera=cam) == E_MODE
    assert bwd_light(camera=None, B=65536) == E_SIZE
    assert bwd_light(grad_eye=X, ws_bytes=8) == E_WORKSPACE
