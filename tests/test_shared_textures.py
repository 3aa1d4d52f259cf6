"""Texture cubes shared by the batch, the parts that need no GPU: Mesh.forward(batch_size, shared_textures=True), the
host-only workspace query of nr_backward_textures_shared, and the entry points that refuse NR_FLAG_SHARED_TEXTURES."""
import pytest
import torch

from neural_renderer_amd import _build, _lib


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def test_mesh_forward_shared_textures(tmp_path):
    import neural_renderer_amd as nr
    path = str(tmp_path / 't.obj')
    with open(path, 'w') as f:
        f.write('v 1 0 0\nv 0 1 0\nv 0 0 1\nv 0 0 0\nf 2 4 3\nf 4 2 1\nf 3 1 2\nf 1 3 4\n')
    mesh = nr.Mesh(path, texture_size=3)
    v, f, t = mesh.forward(4, shared_textures=True)
    assert v.shape == (4, 4, 3) and f.shape == (4, 4, 3) and t.shape == (1, 4, 3, 3, 3, 3)
    assert torch.equal(t[0], torch.sigmoid(mesh.textures))
    t.sum().backward()  # the gradient reaches the parameter without a batch to sum over
    assert mesh.textures.grad.shape == mesh.textures.shape
    # the default is get_batch as it was
    v0, f0, t0 = mesh.forward(4)
    v1, f1, t1 = mesh.get_batch(4)
    assert t0.shape == (4, 4, 3, 3, 3, 3) and torch.equal(t0, t1) and torch.equal(v0, v1) and torch.equal(f0, f1)
    assert torch.equal(t0[2], t[0])
    assert [x.shape for x in mesh(4, shared_textures=True)] == [v.shape, f.shape, t.shape]


def test_workspace_query_is_host_only_and_ignores_the_batch(lib):
    q = lib.nr_backward_textures_shared_workspace_bytes
    for Nf, ts in ((2464, 4), (600, 8), (8, 2), (60, 13)):
        n = q(2, Nf, ts)
        assert n == q(64, Nf, ts) == q(65535, Nf, ts)
        assert Nf * ts ** 3 * 3 * 8 <= n < Nf * ts ** 3 * 3 * 8 + 256  # a double per gradient element, nothing else
    assert q(0, 60, 4) == 0 and q(70000, 60, 4) == 0 and q(2, 0, 4) == 0 and q(2, 60, 1) == 0 and q(2, 60, 14) == 0


def test_argument_errors_do_not_need_a_gpu(lib):
    SHARED = _lib.NR_FLAG_SHARED_TEXTURES
    assert SHARED == 131072 and SHARED & 0xff00 == 0  # (bits 8..15 of a forward's flags carry the z-buffer epoch)
    # the entry points that stride the cubes by the batch refuse the flag before any launch
    assert lib.nr_forward_texture_sampling(1, None, 1, 1, 1, 1, 1, None, None, 1, 0, None, 2, 4, 8, 2, 1e-3, SHARED, None) == -4
    assert lib.nr_backward_textures(1, None, None, 1, None, 1, 1, 1, 1, 2, 4, 8, 2, 1e-3, SHARED, None) == -4
    assert lib.nr_backward_rasterize(1, None, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 4, 8, 2, 1e-3, SHARED, None, 1, 1 << 30, None) == -4
    # nr_backward_textures_shared: NULL pointers, sizes, light descriptors and the workspace are checked first
    call = lib.nr_backward_textures_shared
    assert call(None, None, None, 1, 1, 1, 1, None, 1, 2, 4, 8, 2, 1e-3, 0, 1, 1 << 20, None) == -1
    assert call(None, 1, None, 1, 1, 1, 1, None, 1, 2, 4, 8, 14, 1e-3, 0, 1, 1 << 20, None) == -2
    assert call(None, 1, None, 1, 1, 1, 1, None, 1, 2, 4, 8, 2, 1e-3, 0, None, 0, None) == -3
    assert call(None, 1, None, 1, 1, 1, 1, None, 1, 2, 4, 8, 2, 1e-3, 0, 1, 4 * 24 * 8 - 1, None) == -3
    assert call(_lib.FaceLight(1, 3, None, None), 1, None, 1, 1, 1, 1, None, 1, 2, 4, 8, 2, 1e-3, 0, 1, 1 << 20, None) == -2
    assert call(_lib.FaceLight(1, 2, None, 1), 1, None, 1, 1, 1, 1, None, 1, 2, 4, 8, 2, 1e-3, 0, 1, 1 << 20, None) == -1
