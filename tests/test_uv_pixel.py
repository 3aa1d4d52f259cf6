"""Per-pixel UV images without a GPU: the entry points' argument checks (include/nr_hip.h nr_forward_rasterize_uv,
nr_backward_uv_images), UVImages' input checks, and the NumPy restatement against uv_ref's bake."""
import numpy as np
import pytest

import uv_pixel_ref as R
import uv_ref as U

from neural_renderer_amd import _build, _lib


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def _uv(images=1, table=1, faces_uv=1, face_image=1, base=1, ts=4, M=1, P=16, Bi=1):
    return _lib.UVImagesStruct(images, table, faces_uv, face_image, base, ts, M, P, Bi)


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    E_NULL, E_SIZE, E_WS, E_MODE = -1, -2, -3, -4
    lit = _lib.FaceLight(1, 4, None, None)          # Nf = 4, F = 8 (fill_back)

    def fwd(lit=lit, uv=None, faces=1, fim=1, rgb=1, bg=1, B=2, F=8, S=16, ws=None):
        uv = _uv() if uv is None else uv
        return lib.nr_forward_rasterize_uv(lit, uv, faces, fim, None, None, rgb, None, None, bg, 0, B, F, S, 0.1, 100.0,
                                           1e-3, 0, ws, 0, None)
    assert fwd(lit=None) == E_NULL
    assert fwd(lit=_lib.FaceLight(None, 4, None, None)) == E_NULL
    assert fwd(uv=_uv(images=None)) == E_NULL
    assert fwd(uv=_uv(table=None)) == E_NULL
    assert fwd(uv=_uv(base=None)) == E_NULL
    assert fwd(rgb=None) == E_NULL
    assert fwd(bg=None) == E_NULL
    assert fwd(faces=None) == E_NULL
    assert fwd(fim=None) == E_NULL
    assert fwd(lit=_lib.FaceLight(1, 3, None, None)) == E_SIZE      # texture_faces neither F nor F / 2
    assert fwd(F=4, lit=_lib.FaceLight(1, 4, None, None)) == E_WS   # F == Nf (no fill_back) is valid too
    assert fwd(uv=_uv(Bi=3)) == E_SIZE                               # image_batch neither 1 nor B
    assert fwd(uv=_uv(Bi=0)) == E_SIZE
    assert fwd(uv=_uv(ts=1)) == E_SIZE
    assert fwd(uv=_uv(M=0)) == E_SIZE
    assert fwd(uv=_uv(P=0)) == E_SIZE
    assert fwd(S=0) == E_SIZE
    assert fwd() == E_WS                                             # everything right but the workspace

    def bwd(lit=_lib.FaceLight(1, 4, None, 1), uv=None, wm=1, g=1, gi=1, B=2, F=8, S=16, ws=None, wsb=0):
        uv = _uv() if uv is None else uv
        return lib.nr_backward_uv_images(lit, uv, 1, 1, wm, 1, g, gi, B, F, S, 1e-3, ws, wsb, None)
    assert bwd(lit=None) == E_NULL
    assert bwd(lit=_lib.FaceLight(None, 4, None, 1)) == E_NULL
    assert bwd(uv=_uv(face_image=None)) == E_NULL
    assert bwd(wm=None) == E_NULL
    assert bwd(g=None) == E_NULL
    assert bwd(lit=_lib.FaceLight(1, 5, None, 1)) == E_SIZE
    assert bwd(uv=_uv(Bi=3)) == E_SIZE
    assert bwd(B=0) == E_SIZE
    assert bwd(lit=_lib.FaceLight(1, 4, None, None), gi=None) == E_MODE   # no gradient asked for
    need = lib.nr_backward_uv_images_workspace_bytes(2, 8, 16, 1)
    assert need >= 8 * (16 * 3 + 2 * 8 * 3)
    assert lib.nr_backward_uv_images_workspace_bytes(2, 8, 16, 2) >= 8 * (2 * 16 * 3 + 2 * 8 * 3)
    assert lib.nr_backward_uv_images_workspace_bytes(2, 8, 16, 3) == 0
    assert lib.nr_backward_uv_images_workspace_bytes(2, 8, 0, 1) == 0
    assert bwd() == E_WS
    assert bwd(ws=1, wsb=need - 1) == E_WS


def _layout(rng, sizes=((5, 7), (1, 1)), F=6, ts=3):
    import neural_renderer_amd as nr
    uv, face_image, base = U.random_layout(rng, F, ts, list(sizes))
    return nr.UVLayout(uv, face_image, base, list(sizes))


def test_uv_images_rejects_bad_images():
    import torch
    import neural_renderer_amd as nr
    layout = _layout(np.random.default_rng(0))
    ok = [torch.zeros(5, 7, 3), torch.zeros(1, 1, 3)]
    with pytest.raises(ValueError):
        nr.UVImages(ok, layout)                                          # arguments swapped: not a layout
    with pytest.raises(ValueError):
        nr.UVImages(layout, ok)                                          # CPU tensors
    with pytest.raises(ValueError):
        nr.UVImages(layout, [ok[0].double(), ok[1].double()])            # wrong dtype (and CPU)
    with pytest.raises(ValueError):
        nr.UVImages(layout, ok[:1])                                      # one image short
    with pytest.raises(ValueError):
        nr.UVImages(layout, ok + ok[1:])                                 # one too many
    with pytest.raises(ValueError):
        nr.UVImages(layout, [torch.zeros(7, 5, 3), ok[1]])               # H and W exchanged
    with pytest.raises(ValueError):
        nr.UVImages(layout, [torch.zeros(5, 7, 4), ok[1]])               # four channels
    with pytest.raises(ValueError):
        nr.UVImages(layout, [torch.zeros(2, 5, 7, 3), torch.zeros(3, 1, 1, 3)])   # batches 2 and 3
    with pytest.raises(ValueError):
        nr.UVImages(layout, [np.zeros((5, 7, 3), np.float32), ok[1]])    # not a tensor


@pytest.mark.parametrize('seed', range(4))
def test_pixel_lookup_at_texel_points_is_the_bake(seed):
    """The restatement's per-pixel lookup, evaluated at every texel's barycentric point, is uv_ref.bake bit for bit: the two
    restatements share one convention (rows mirrored, read order, clamping)."""
    rng = np.random.default_rng(40 + seed)
    sizes = [(1, 1), (int(rng.integers(1, 30)), int(rng.integers(1, 50))), (8, 3)]
    ts = int(rng.choice([2, 3, 4, 6]))
    F = 50
    uv, face_image, base = U.random_layout(rng, F, ts, sizes)
    images = [rng.uniform(0, 1, (h, w, 3)).astype(np.float32) for h, w in sizes]
    want = U.bake(images, uv, face_image, base, ts).reshape(F, -1, 3)
    d = U.texel_points(ts)
    T = ts ** 3
    for m, (h, w) in enumerate(sizes):
        faces = np.nonzero(face_image == m)[0]
        if len(faces) == 0:
            continue
        tri = np.repeat(uv[faces], T, axis=0)
        idx, wt = R.reads(tri, np.tile(d, (len(faces), 1)), h, w)
        flat = images[m].reshape(-1, 3)
        c = np.zeros((len(tri), 3), np.float32)
        for r in range(4):
            c = c + flat[idx[:, r]] * wt[:, r, None]
        assert np.array_equal(c.reshape(len(faces), T, 3), want[faces])
