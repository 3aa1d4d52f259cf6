"""Learnable UV texture images, host side (include/nr_hip.h nr_bake_uv_textures, neural_renderer_amd/uv_textures.py).

The test-side restatement of the bake (tests/uv_ref.py) against the oracle's restatement of the reference's load_obj bake,
its adjoint by the dot-product test, UVLayout.from_obj on the textured display model without a GPU, and the argument
checks of the new entry points."""
import numpy as np
import pytest

import helpers as H
import uv_ref as U
from oracle import oracle as O


@pytest.fixture(scope='module')
def display_obj(tmp_path_factory):
    return H.write_display_model(str(tmp_path_factory.mktemp('display_uv')))


def _oracle_bake(image, faces_uv, ts):
    t = np.zeros((faces_uv.shape[0], ts, ts, ts, 3), np.float32)
    O.bake_texture_image(np.ascontiguousarray(image[::-1]), faces_uv, np.ones(faces_uv.shape[0], np.int32), t)
    return t


def _off_origin(t):
    """Every texel but (0,0,0): [F, ts^3 - 1, 3]."""
    f = t.shape[0]
    return t.reshape(f, -1, 3)[:, 1:]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_equals_oracle_bake(seed):
    rng = np.random.default_rng(seed)
    for h, w, ts in ((1, 1, 2), (7, 13, 3), (30, 5, 4), (64, 64, 6)):
        image = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
        uv, _, base = U.random_layout(rng, 40, ts, [(h, w)])
        got = U.bake([image], uv, np.zeros(40, np.int32), base, ts)
        want = _oracle_bake(image, uv, ts)
        assert np.array_equal(_off_origin(got), _off_origin(want))
        assert np.isnan(want[:, 0, 0, 0]).all() and np.isfinite(got[:, 0, 0, 0]).all()


def test_centroid_texel_is_the_lookup_at_the_centroid():
    """Texel (0,0,0) on an image linear in (column, row): the value at the uv centroid."""
    h, w = 37, 53
    cols, rows = np.meshgrid(np.arange(w), np.arange(h))
    image = np.stack((cols / (w - 1.), rows / (h - 1.), np.full((h, w), 0.25)), axis=2).astype(np.float32)
    uv = np.array([[[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]]], np.float32)
    t = U.bake([image], uv, np.zeros(1, np.int32), np.zeros((1, 3, 3, 3, 3), np.float32), 3)
    c = uv[0].mean(0)
    np.testing.assert_allclose(t[0, 0, 0, 0], [c[0], 1 - c[1], 0.25], atol=2e-5)


def test_adjoint_dot_product():
    rng = np.random.default_rng(7)
    sizes = [(9, 14), (1, 1), (20, 3)]
    ts = 4
    uv, face_image, _ = U.random_layout(rng, 60, ts, sizes)
    x = [rng.normal(size=(h, w, 3)) for h, w in sizes]
    y = rng.normal(size=(60, ts, ts, ts, 3))
    y[face_image < 0] = 0.0       # the base texels are constants: not part of the linear map
    ax = U.bake_f64(x, uv, face_image, ts)
    aty, _ = U.bake_adjoint(y, uv, face_image, sizes, ts)
    lhs = float((ax * y).sum())
    rhs = float(sum((a * b).sum() for a, b in zip(x, aty)))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_layout_from_obj_matches_oracle(display_obj):
    import neural_renderer_amd as nr
    ts = 4
    layout = nr.UVLayout.from_obj(display_obj, texture_size=ts)
    g = H.display_model()
    assert layout.num_faces == 3644 and layout.num_images == 2
    assert sorted(layout.image_sizes) == [(100, 545), (225, 225)]
    _, _, t0 = O.load_obj(display_obj, load_texture=True, texture_size=ts)
    textured = np.array([bool(m) for m in g['map_kd']])[g['face_material']]
    assert np.array_equal(layout.face_image >= 0, textured)
    assert np.array_equal(layout.base[~textured], t0[~textured])
    baked = U.bake(layout.images, layout.faces_uv, layout.face_image, layout.base, ts)
    assert np.array_equal(baked[~textured], t0[~textured])
    assert np.array_equal(_off_origin(baked[textured]), _off_origin(t0[textured]))
    assert np.isfinite(baked).all()


def test_load_textures_keeps_its_output_host_half(display_obj):
    """The parsing split out of load_textures gives the oracle's faces_uv and the Kd / 0.5 fill."""
    from neural_renderer_amd.load_obj import parse_textures
    import os
    mtl = os.path.join(os.path.dirname(display_obj), 'model.mtl')
    faces_uv, materials, colors, files, base = parse_textures(display_obj, mtl, 3)
    uv0, names0 = O.parse_obj_texture_faces(display_obj)[:2]
    assert np.array_equal(faces_uv, uv0) and list(materials) == list(names0)
    assert len(files) == 2 and base.shape == (3644, 3, 3, 3, 3)


def test_entry_points_check_arguments_without_a_gpu():
    from neural_renderer_amd import _lib
    lib = _lib.load()
    p = 256   # any non-NULL address: the checks come before any launch
    assert lib.nr_bake_uv_textures(None, p, p, p, p, p, 1, 10, 4, 1, 100, None) == -1
    assert lib.nr_bake_uv_textures(p, p, p, p, p, None, 1, 10, 4, 1, 100, None) == -1
    assert lib.nr_bake_uv_textures(p, p, p, p, p, p, 0, 10, 4, 1, 100, None) == -2
    assert lib.nr_bake_uv_textures(p, p, p, p, p, p, 1, 10, 1, 1, 100, None) == -2
    assert lib.nr_bake_uv_textures(p, p, p, p, p, p, 1, 10, 4, 0, 100, None) == -2
    assert lib.nr_uv_texture_map(p, p, None, p, p, p, 10, 4, 1, 100, p, 1 << 20, None) == -1
    assert lib.nr_uv_texture_map(p, p, p, p, p, p, 0, 4, 1, 100, p, 1 << 20, None) == -2
    assert lib.nr_uv_texture_map(p, p, p, p, p, p, 1 << 24, 16, 1, 100, p, 1 << 20, None) == -2   # entry numbers overflow
    assert lib.nr_uv_texture_map_workspace_bytes(0, 4, 1, 100) == 0
    assert lib.nr_bake_uv_textures_backward(p, None, p, p, p, 1, 10, 4, 100, None) == -1
    assert lib.nr_bake_uv_textures_backward(p, p, p, p, p, 1, 10, 4, 0, None) == -2


def test_bake_refuses_bad_inputs_before_any_launch(display_obj):
    import torch
    import neural_renderer_amd as nr
    layout = nr.UVLayout.from_obj(display_obj, texture_size=2)
    cpu = [torch.from_numpy(im) for im in layout.images]
    with pytest.raises(ValueError):
        nr.bake_uv_textures(cpu, layout)                     # CPU tensors
    with pytest.raises(ValueError):
        nr.bake_uv_textures(cpu[:1], layout)                 # one image short
    with pytest.raises(ValueError):
        nr.bake_uv_textures([im.double() for im in cpu], layout)
    with pytest.raises(ValueError):
        nr.UVLayout(np.zeros((2, 3, 2)), np.array([0, 1]), np.zeros((2, 2, 2, 2, 3)), [(4, 4)])   # image 1 of 1
