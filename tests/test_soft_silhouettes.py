"""CPU checks of the soft silhouette (neural_renderer_amd/soft_silhouette.py, include/nr_hip.h: nr_soft_silhouette_*):
soft_silhouettes_torch against the float64 restatement of tests/soft_ref.py and against gradcheck, the pins of the
definition, its invariances, argument errors, exports and the host-only part of the entry points.  The kernels themselves:
tests/test_soft_silhouettes_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import soft_ref as R


def _soft(faces, S, sigma, **kw):
    import neural_renderer_amd as nr
    return nr.soft_silhouettes(faces, S, sigma, **kw)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


TRI = [[[-0.5, -0.4, 1.0], [0.6, -0.3, 1.5], [0.1, 0.7, 2.0]]]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, gradcheck

@pytest.mark.parametrize('sigma', [1e-3, 1e-1])
def test_torch_float64_matches_the_restatement(sigma):
    """icosphere(1) in the checked view, S = 16: alpha within 1e-12, the gradient within 1e-12 of its term magnitudes."""
    S = 16
    faces = R.sphere_faces(1, 1)
    g = np.random.default_rng(3).normal(size=(1, S, S))
    ref = R.restate(faces, S, sigma, g=g)
    assert ref.doubt_share <= 0.02
    ft = _t(faces, True)
    alpha = _soft(ft, S, sigma)
    alpha.backward(_t(g))
    assert alpha.dtype == torch.float64 and tuple(alpha.shape) == (1, S, S)
    assert np.abs(alpha.detach().numpy() - ref.alpha).max() <= 1e-12
    assert np.abs(ref.grad).max() > 0
    assert R.worst_ratio(ft.grad.numpy(), ref.grad, 1e-12 * ref.grad_mag + 1e-300) <= 1
    assert not ft.grad.numpy()[..., 2].any()


def test_gradcheck():
    """4 random faces at S = 8, sigma = 0.05, the vertices nudged until no pair is in doubt."""
    S, sigma = 8, 0.05
    for seed in range(50):
        rng = np.random.default_rng(100 + seed)
        faces = np.concatenate((rng.uniform(-0.8, 0.8, size=(1, 4, 3, 2)), np.ones((1, 4, 3, 1))), -1).astype(np.float32)
        if R.restate(faces, S, sigma).doubt[0] == 0:
            break
    else:
        raise AssertionError('no case without a pair in doubt')
    ft = _t(faces, True)
    assert torch.autograd.gradcheck(lambda f: _soft(f, S, sigma), (ft,), eps=1e-7, atol=1e-7, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# pins

def test_a_pixel_centre_on_an_edge_gives_one_half():
    S = 8
    c = (2 * 5 + 1 - S) / S   # the centre of column 5: the edge v0v1 runs along it
    faces = _t([[[[c, -0.9, 1.0], [c, 0.9, 1.0], [0.9, 0.0, 1.0]]]])
    alpha = _soft(faces, S, 1e-2)
    assert (alpha[0, :, 5] == 0.5).all()
    assert (alpha[0, :, 6] > 0.5).any() and (alpha[0, :, 4] < 0.5).all()


@pytest.mark.parametrize('face', [[[-0.3, -0.2, 1.0], [0.1, 0.2, 1.0], [0.5, 0.6, 1.0]],
                                  [[0.2, 0.1, 1.0], [0.2, 0.1, 1.0], [-0.4, 0.3, 1.0]],
                                  [[0.2, 0.1, 1.0], [0.2, 0.1, 1.0], [0.2, 0.1, 1.0]]])
def test_a_zero_area_face_has_no_inside(face):
    ft = _t([[face]], True)
    alpha = _soft(ft, 16, 1e-2)
    assert (alpha <= 0.5).all() and (alpha > 0).any()
    alpha.sum().backward()
    assert torch.isfinite(ft.grad).all()


@pytest.mark.parametrize('bad', [[[0.0, 0.1, 1.0], [float('nan'), 0.4, 1.0], [0.3, 0.2, 1.0]],
                                 [[0.0, 0.1, 1.0], [0.5, float('inf'), 1.0], [0.3, 0.2, 1.0]],
                                 [[0.0, 0.1, 0.05], [0.5, 0.4, 1.0], [0.3, 0.2, 1.0]],
                                 [[0.0, 0.1, 1.0], [0.5, 0.4, 1.0], [0.3, 0.2, 200.0]]])
def test_a_dropped_face_changes_nothing_and_gets_no_gradient(bad):
    ft = _t([[TRI[0], bad]], True)
    alpha = _soft(ft, 16, 1e-2)
    assert torch.equal(alpha.detach(), _soft(_t([TRI]), 16, 1e-2))
    alpha.sum().backward()
    assert not ft.grad[0, 1].any() and ft.grad[0, 0].abs().sum() > 0 and torch.isfinite(ft.grad).all()
    # near and far are the operator's arguments: widened, the two faces dropped for their z come back
    widened = _soft(_t([[TRI[0], bad]]), 16, 1e-2, near=0.01, far=1000.0)
    assert torch.equal(widened, alpha.detach()) == (not np.isfinite(bad).all())


def test_two_identical_faces_square_the_transmittance():
    one = _soft(_t([TRI]), 16, 1e-2)
    two = _soft(_t([[TRI[0], TRI[0]]]), 16, 1e-2)
    assert torch.allclose(two, 1 - (1 - one) ** 2, rtol=0, atol=1e-15) and (two > one).any()


def test_far_outside_is_below_2_to_the_minus_24_without_a_nan():
    ft = _t([[[[5.0, 5.0, 1.0], [5.2, 5.0, 1.0], [5.1, 5.3, 1.0]]]], True)
    alpha = _soft(ft, 8, 1e-4)
    assert (alpha < 2.0 ** -24).all() and (alpha >= 0).all()
    alpha.sum().backward()
    assert torch.isfinite(ft.grad).all()


# ---------------------------------------------------------------------------------------------------------------------
# invariances

def test_vertex_order_and_row_order():
    S, sigma = 16, 1e-2
    faces = R.sphere_faces(0, 1).astype(np.float64)
    g = _t(np.random.default_rng(4).normal(size=(1, S, S)))
    a = _t(faces, True)
    b = _t(faces[:, :, ::-1].copy(), True)   # every face with its vertex order flipped
    out_a, out_b = _soft(a, S, sigma), _soft(b, S, sigma)
    assert torch.allclose(out_a, out_b, rtol=0, atol=1e-14)
    out_a.backward(g)
    out_b.backward(g)
    assert torch.allclose(a.grad, b.grad.flip(2), rtol=1e-9, atol=1e-14) and a.grad.abs().sum() > 0
    # row 0 is the top: a face in the upper half of NDC (y up) lights the first rows
    top = _soft(_t([[[[-0.5, 0.3, 1.0], [0.5, 0.3, 1.0], [0.0, 0.9, 1.0]]]]), S, 1e-3)
    assert top[0, :S // 2].max() > 0.9 and top[0, S // 2:].max() < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# arguments, exports, ABI

def test_argument_errors():
    f = _t([TRI])
    for sigma in (0, -1.0, float('nan'), float('inf'), None, 'x'):
        with pytest.raises(ValueError, match='sigma'):
            _soft(f, 8, sigma)
    for bad in (f[0], f[:, :, :2], f[..., :2], torch.zeros((0, 1, 3, 3)), torch.zeros((1, 0, 3, 3)), [TRI]):
        with pytest.raises(ValueError, match='faces must be'):
            _soft(bad, 8, 1e-2)
    with pytest.raises(ValueError, match='faces must be'):
        _soft(torch.zeros((1, 1, 3, 3), dtype=torch.int32), 8, 1e-2)
    for size in (0, -4, 2.5, None):
        with pytest.raises(ValueError, match='image_size'):
            _soft(f, size, 1e-2)
    with pytest.raises(ValueError, match='implementation'):
        _soft(f, 8, 1e-2, implementation='cuda')
    with pytest.raises(ValueError, match='HIP kernels take float32 CUDA tensors'):
        _soft(f, 8, 1e-2, implementation='hip')
    with pytest.raises(ValueError, match='HIP kernels take float32 CUDA tensors'):
        _soft(f.float(), 8, 1e-2, implementation='hip')
    assert _soft(f.float(), 8, 1e-2, implementation='torch').dtype == torch.float32


def test_exports():
    import neural_renderer
    import neural_renderer_amd as nr
    for name in ('soft_silhouettes', 'soft_silhouettes_torch'):
        assert name in nr.__all__ and getattr(neural_renderer, name) is getattr(nr, name)
    r = nr.Renderer()
    assert r.soft_sigma == 1e-4 and callable(r.render_soft_silhouettes)


def test_renderer_on_the_cpu():
    """render_soft_silhouettes on CPU tensors: the module-by-module front-end and the plain-torch operator."""
    import neural_renderer_amd as nr
    v, f = nr.icosphere(1, 0.8)
    v = v[None].clone().requires_grad_(True)
    r = nr.Renderer()
    r.image_size, r.soft_sigma = 16, 1e-2
    for fill_back in (True, False):
        r.fill_back = fill_back
        img = r.render_soft_silhouettes(v, f[None])
        assert r.last_frontend == 'torch' and img.shape == (1, 16, 16) and img.max() > 0.9 and img.min() < 0.1
        assert torch.equal(img, nr.soft_silhouettes(r._project(v, f[None]), 16, 1e-2, r.near, r.far))
    img.sum().backward()
    assert v.grad.abs().sum() > 0


def test_symbols_and_host_only_entry_points():
    from neural_renderer_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    names = ('nr_soft_silhouette_workspace_bytes', 'nr_soft_silhouette_forward', 'nr_soft_silhouette_backward')
    assert all(hasattr(raw, n) and n in _lib.SIGNATURES for n in names)
    lib = _lib.load()
    wsb = lib.nr_soft_silhouette_workspace_bytes
    assert wsb(2, 10, 16) >= 2 * 10 * 40 and wsb(64, 2464, 256) == wsb(64, 2464, 64)
    for B, F, S in ((0, 1, 8), (65536, 1, 8), (1, 0, 8), (1, 2 ** 24 + 1, 8), (1, 1, 0), (1, 1, 16385), (65535, 2 ** 24, 8)):
        assert wsb(B, F, S) == 0, (B, F, S)
    fwd, bwd = lib.nr_soft_silhouette_forward, lib.nr_soft_silhouette_backward
    assert fwd(None, 1, 1, 1, 1, 8, 1e-4, 0.1, 100.0, 1, 64, None) == -1
    assert fwd(1, None, 1, 1, 1, 8, 1e-4, 0.1, 100.0, 1, 64, None) == -1
    assert fwd(1, 1, None, 1, 1, 8, 1e-4, 0.1, 100.0, 1, 64, None) == -1
    assert bwd(1, 1, None, 1, 1, 1, 8, 1e-4, 0.1, 100.0, 1, 64, None) == -1
    assert bwd(1, 1, 1, None, 1, 1, 8, 1e-4, 0.1, 100.0, 1, 64, None) == -1
    assert fwd(1, 1, 1, 1, 1, 8, 1e-4, 0.1, 100.0, None, 0, None) == -3
    assert fwd(1, 1, 1, 1, 1, 8, 1e-4, 0.1, 100.0, 1, 47, None) == -3
    assert bwd(1, 1, 1, 1, 1, 1, 8, 1e-4, 0.1, 100.0, None, 0, None) == -3
    assert fwd(1, 1, 1, 0, 1, 8, 1e-4, 0.1, 100.0, 1, 64, None) == -2
    assert bwd(1, 1, 1, 1, 1, 1, 20000, 1e-4, 0.1, 100.0, 1, 64, None) == -2
    assert fwd(1, 1, 1, 1, 1, 8, 0.0, 0.1, 100.0, 1, 64, None) == -4
    assert bwd(1, 1, 1, 1, 1, 1, 8, -1.0, 0.1, 100.0, 1, 64, None) == -4
