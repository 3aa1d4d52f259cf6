"""CPU checks of neural_renderer_amd/normals.py: the plain-torch implementation against the NumPy restatement
(tests/normals_ref.py) under its derived bounds, the restatement's adjoint against central differences of the restatement,
camera_rotation against look_at / look / projection, the fill_back relation and the argument errors."""
import numpy as np
import pytest
import torch

import normals_ref as R

MESHES = sorted(R.meshes())


def _t(a, grad=False, dtype=None):
    t = torch.tensor(np.ascontiguousarray(a), dtype=dtype)
    return t.requires_grad_(True) if grad else t


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('name', MESHES)
def test_torch_forward_against_restatement(name, per_image):
    """float32 torch against the float64 restatement under gamma_k of normals_ref (the CPU's scatter_add runs in the kernels'
    ascending order, its dot products and cross products in orders of torch's own: the bound covers any order); the float64
    torch path against the float64 restatement to 1e-12."""
    import neural_renderer_amd as nr
    v, f = R.batch(name, 3, per_image_topology=per_image)
    Nv = v.shape[1]
    fm, vm = R.forward_mag(v, f)
    vt, ft = _t(v), _t(f)
    got = nr.vertex_normals(vt, ft).numpy()
    assert R.worst_ratio(got, R.vertex_normals(v, f), R.gamma(R.forward_k(f, Nv, 'vertex', 3)) * vm) <= 1
    got = nr.face_normals(vt, ft).numpy()
    assert R.worst_ratio(got, R.face_normals(v, f), R.gamma(R.forward_k(f, Nv, 'face')) * fm) <= 1
    for smooth in (False, True):
        for fill_back in (False, True):
            got = nr.corner_normals(vt, ft, smooth=smooth, fill_back=fill_back).colors.numpy()
            ref = R.corner_normals(v, f, smooth, fill_back)
            assert got.shape == ref.shape
            bound = R.gamma(R.corner_k(f, Nv, smooth, fill_back, 3)) * R.corner_mag(v, f, smooth, fill_back)
            assert R.worst_ratio(got, ref, bound) <= 1
            got64 = nr.normals.corner_normals_torch(vt.double(), ft, smooth, fill_back).numpy()
            assert np.abs(got64 - ref).max() <= 1e-12


def test_restatement_float32_is_close_to_float64():
    v, f = R.batch('icosphere1', 2)
    fm, vm = R.forward_mag(v, f)
    assert R.worst_ratio(R.vertex_normals(v, f, np.float32), R.vertex_normals(v, f), R.gamma(R.forward_k(f, 42, 'vertex', 2)) * vm) <= 1
    assert R.worst_ratio(R.face_normals(v, f, np.float32), R.face_normals(v, f), R.gamma(11) * fm) <= 1


def test_degenerate_entries_are_zero_with_finite_gradients():
    import neural_renderer_amd as nr
    v, f = R.batch('degenerate', 2)
    vt, ft = _t(v, True), _t(f)
    nv, nf = nr.vertex_normals(vt, ft), nr.face_normals(vt, ft)
    assert not nv[:, 9].any() and not nf[:, -1].any()
    rng = np.random.default_rng(5)
    (nv * _t(rng.normal(size=nv.shape), dtype=torch.float32)).sum().backward()
    assert torch.isfinite(vt.grad).all() and not vt.grad[:, 9].any() and vt.grad.abs().sum() > 0
    vt.grad = None
    g = _t(rng.normal(size=nf.shape), dtype=torch.float32)
    (nf * g).sum().backward()
    assert torch.isfinite(vt.grad).all()
    # the r = 0 case of normalize's backward is g / eps: the zero-area face (4, 4, 8) hands terms of that size to its
    # corners 0 and 1, where they cancel (both are vertex 4): the magnitudes carry them, the bound is the adjoint's own
    gv, gv_mag = R.adjoint64(v, f, g.numpy(), 'face')
    assert gv_mag.max() > 1e3 * np.abs(gv).max()
    assert R.worst_ratio(vt.grad.numpy(), gv, R.gamma(R.backward_k(f, v.shape[1])) * gv_mag) <= 1


def _fd(v, f, g, what, smooth, fill_back, picks, h=1e-6):
    fn = {'vertex': lambda x: R.vertex_normals(x, f), 'face': lambda x: R.face_normals(x, f),
          'corner': lambda x: R.corner_normals(x, f, smooth, fill_back)}[what]
    out = {}
    for (b, i) in picks:
        d = np.zeros(3)
        for c in range(3):
            vp, vm = v.copy(), v.copy()
            vp[b, i, c] += h
            vm[b, i, c] -= h
            d[c] = ((fn(vp) - fn(vm)) * g).sum() / (2 * h)
        out[(b, i)] = d
    return out


@pytest.mark.parametrize('what,smooth,fill_back', [('vertex', False, False), ('face', False, False), ('corner', False, True),
                                                   ('corner', True, True), ('corner', True, False)])
@pytest.mark.parametrize('name', ['grid3', 'fan12', 'icosphere1', 'twin_faces'])
def test_adjoint_against_central_differences_and_torch(name, what, smooth, fill_back):
    """The float64 adjoint of the restatement against central differences of the float64 restatement (step 1e-6: truncation
    h^2 f''' / 6 ~ 1e-12 times third derivatives of order 1e2 on these meshes, rounding 1e-16 / 1e-6: 1e-7 relative to the
    largest gradient entry covers both), and the float64 torch path's autograd against the adjoint to 1e-10."""
    import neural_renderer_amd as nr
    from neural_renderer_amd import normals as N
    v32, f = R.batch(name, 2)
    v = v32.astype(np.float64)
    rng = np.random.default_rng(77)
    ref = {'vertex': lambda: R.vertex_normals(v, f), 'face': lambda: R.face_normals(v, f),
           'corner': lambda: R.corner_normals(v, f, smooth, fill_back)}[what]()
    g = rng.normal(size=ref.shape)
    gv, gv_mag = R.adjoint64(v, f, g, what, smooth, fill_back)
    assert (np.abs(gv) <= gv_mag * (1 + 1e-12) + 1e-300).all()
    picks = [(b, i) for b in range(2) for i in sorted(set((0, v.shape[1] // 2, v.shape[1] - 1)))]
    for (b, i), d in _fd(v, f, g, what, smooth, fill_back, picks).items():
        assert np.abs(gv[b, i] - d).max() <= 1e-7 * np.abs(gv).max(), (b, i)
    vt = _t(v, True)
    out = {'vertex': lambda: N.vertex_normals_torch(vt, _t(f)), 'face': lambda: N.face_normals_torch(vt, _t(f)),
           'corner': lambda: N.corner_normals_torch(vt, _t(f), smooth, fill_back)}[what]()
    (out * _t(g)).sum().backward()
    assert np.abs(vt.grad.numpy() - gv).max() <= 1e-10 * np.abs(gv).max()


@pytest.mark.parametrize('smooth', [False, True])
def test_fill_back_relation(smooth):
    import neural_renderer_amd as nr
    v, f = R.batch('icosphere1', 2)
    c = nr.corner_normals(_t(v), _t(f), smooth=smooth, fill_back=True).colors
    Nf = len(f)
    assert c.shape == (2, 2 * Nf, 3, 3)
    assert torch.equal(c[:, Nf:], -c[:, :Nf].flip(2))
    assert torch.equal(c[:, :Nf], nr.corner_normals(_t(v), _t(f), smooth=smooth, fill_back=False).colors)


def test_unbatched_and_exports():
    import neural_renderer as alias
    import neural_renderer_amd as nr
    v, f = R.batch('grid3', 1)
    a = nr.vertex_normals(_t(v[0]), _t(f))
    assert a.shape == (9, 3) and torch.equal(a, nr.vertex_normals(_t(v), _t(f))[0])
    assert nr.face_normals(_t(v[0]), _t(f)).shape == (8, 3)
    for n in ('vertex_normals', 'face_normals', 'corner_normals', 'camera_rotation'):
        assert n in nr.__all__ and getattr(alias, n) is getattr(nr, n)
    assert hasattr(nr.Renderer, 'render_normals')


def test_mesh_vertex_normals(tmp_path):
    import neural_renderer_amd as nr
    v, f = R.meshes()['icosphere1']
    path = tmp_path / 'ico.obj'
    with open(str(path), 'w') as fh:
        for p in v:
            fh.write('v %r %r %r\n' % tuple(float(c) for c in p))
        for t in f:
            fh.write('f %d %d %d\n' % tuple(int(i) + 1 for i in t))
    mesh = nr.Mesh(str(path), normalization=False)
    n = mesh.vertex_normals()
    assert n.shape == (42, 3) and n.requires_grad
    assert torch.equal(n.detach(), nr.vertex_normals(mesh.vertices.detach(), mesh.faces))
    # lighting()'s sign, cross(v0 - v1, v2 - v1): on this sphere the radial direction negated, up to the facets' bias
    assert (n.detach() + mesh.vertices.detach()).abs().max() < 1e-2
    n.sum().backward()
    assert mesh.vertices.grad is not None and torch.isfinite(mesh.vertices.grad).all()


def test_camera_rotation_against_the_camera_modules():
    """look_at(v, eye) = (v - eye) @ R^T, likewise look; projection's camera point is v @ R^T + t.  float32 (look_at and
    look take the eye as float32): R comes from the same three lines, so the two sides differ by the order of a three-term
    dot product at most, gamma_3 of |v - eye| |R|^T."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(3)
    B = 3
    v = _t(rng.normal(size=(B, 7, 3)), dtype=torch.float32)
    r = nr.Renderer()

    def close(rot, eye_b, want):
        d = v - eye_b[:, None, :]
        bound = R.gamma(3) * torch.matmul(d.abs().double(), rot.abs().double().transpose(1, 2))
        return bool(((torch.matmul(d, rot.transpose(1, 2)) - want).abs().double() <= bound).all())

    for eye in (nr.get_points_from_angles(2.732, 30, 40), rng.normal(size=(B, 3)) * 2):
        r.eye = _t(np.asarray(eye, np.float32)) if np.ndim(eye) == 2 else eye
        eye_t = _t(np.asarray(eye, np.float32))
        eye_b = eye_t[None].expand(B, 3) if eye_t.dim() == 1 else eye_t
        r.camera_mode = 'look_at'
        rot = nr.camera_rotation(r, B, v)
        assert rot.shape == (B, 3, 3) and rot.dtype == v.dtype
        want = nr.look_at(v, r.eye)
        assert close(rot, eye_b, want)
        r.camera_mode = 'look'
        r.camera_direction = [0.2, -0.3, 0.9]
        rot = nr.camera_rotation(r, B, v)
        want = nr.look(v, r.eye, r.camera_direction)
        assert close(rot, eye_b, want)
    # orthonormal up to normalize's eps
    assert (torch.matmul(rot, rot.transpose(1, 2)) - torch.eye(3)).abs().max() <= 1e-4
    r.camera_mode = 'projection'
    q, _ = np.linalg.qr(rng.normal(size=(B, 3, 3)))
    r.R, r.t, r.K, r.orig_size = _t(q.astype(np.float32)), _t((rng.normal(size=(B, 3)) + [0, 0, 5]).astype(np.float32)), np.eye(3), 2.0
    rot = nr.camera_rotation(r, B, v)
    assert torch.equal(rot, r.R)
    cam = torch.matmul(v, rot.transpose(1, 2)) + r.t[:, None, :]
    assert torch.equal(nr.projection(v, r.K, r.R, r.t, None, r.orig_size)[..., 2], cam[..., 2])
    r.R = q[0]
    assert nr.camera_rotation(r, B, v).shape == (B, 3, 3)
    # a learnable eye receives a gradient
    r.camera_mode = 'look_at'
    r.eye = _t(np.array([0.5, 1.0, -2.0], np.float32), True)
    nr.camera_rotation(r, B, v)[:, 0, 2].sum().backward()
    assert r.eye.grad is not None and r.eye.grad.abs().sum() > 0
    r.camera_mode = 'orbit'
    with pytest.raises(ValueError):
        nr.camera_rotation(r, B, v)


def test_argument_errors():
    import neural_renderer_amd as nr
    v, f = R.batch('grid3', 2)
    vt, ft = _t(v), _t(f)
    for fn in (nr.vertex_normals, nr.face_normals, nr.corner_normals):
        with pytest.raises(ValueError):
            fn(vt, ft, implementation='hip')        # a CPU tensor
        with pytest.raises(ValueError):
            fn(vt, ft, implementation='cuda')
        with pytest.raises(ValueError):
            fn(vt, ft.float())
        with pytest.raises(ValueError):
            fn(vt[..., :2], ft)
        with pytest.raises(ValueError):
            fn(vt.long(), ft)
        with pytest.raises(ValueError):
            fn(vt, ft[None].expand(3, -1, -1))      # batch sizes differ
        with pytest.raises(ValueError):
            fn(v, ft)
    with pytest.raises(ValueError):
        nr.corner_normals(vt[0], ft)
    with pytest.raises(ValueError):
        nr.corner_normals(vt.double(), ft)          # (corner_normals_torch takes other float types)
    r = nr.Renderer()
    with pytest.raises(ValueError):
        r.render_normals(vt, ft[None].expand(2, -1, -1), space='screen')
    r.shading = 'phong'
    with pytest.raises(ValueError):
        r.render_normals(vt, ft[None].expand(2, -1, -1))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from neural_renderer_amd import _lib
    lib = _lib.load()
    assert lib.nr_normals_workspace_bytes(2, 10, 30) == 2 * 30 * 3 * 4
    assert lib.nr_normals_workspace_bytes(2, 50, 30) == 2 * 50 * 3 * 4
    assert lib.nr_normals_workspace_bytes(0, 10, 30) == 0 and lib.nr_normals_workspace_bytes(70000, 10, 30) == 0
    assert lib.nr_vertex_normals_forward(None, 1, 1, 1, 1, 1, 3, 1, 0, None) == -1
    assert lib.nr_vertex_normals_forward(1, 1, None, 1, 1, 1, 3, 1, 0, None) == -1
    assert lib.nr_vertex_normals_forward(1, 1, 1, 1, 1, 0, 3, 1, 0, None) == -2
    assert lib.nr_vertex_normals_backward(1, 1, 1, 1, None, 1, 1, 3, 1, 0, 1, 1 << 20, None) == -1
    assert lib.nr_vertex_normals_backward(1, 1, 1, 1, 1, 1, 1, 3, 1, 0, None, 0, None) == -3
    assert lib.nr_face_normals_forward(1, None, 1, 1, 3, 1, 0, None) == -1
    assert lib.nr_face_normals_forward(1, 1, 1, 70000, 3, 1, 0, None) == -2
    assert lib.nr_face_normals_backward(1, 1, 1, None, 1, 1, 1, 3, 1, 0, 1, 1 << 20, None) == -1
    assert lib.nr_face_normals_backward(1, 1, 1, 1, 1, 1, 1, 3, 1, 0, 1, 8, None) == -3
    assert lib.nr_corner_normals_forward(1, 1, None, None, None, 1, 3, 1, 0, 1, 0, None, 0, None) == -1
    assert lib.nr_corner_normals_forward(1, 1, None, None, 1, 1, 3, 1, 0, 1, 2, None, 0, None) == -4
    assert lib.nr_corner_normals_forward(1, 1, None, None, 1, 1, 3, 1, 0, 1, 1, None, 0, None) == -1   # smooth needs the table
    assert lib.nr_corner_normals_forward(1, 1, 1, 1, 1, 1, 3, 1, 0, 1, 1, None, 0, None) == -3
    assert lib.nr_corner_normals_backward(1, 1, 1, 1, 1, None, 1, 3, 1, 0, 1, 0, 1, 1 << 20, None) == -1
    assert lib.nr_corner_normals_backward(1, 1, 1, 1, 1, 1, 1, 3, 0, 0, 1, 0, 1, 1 << 20, None) == -2
    assert lib.nr_corner_normals_backward(1, 1, 1, 1, 1, 1, 1, 3, 1, 0, 1, 0, None, 0, None) == -3
