"""CPU checks of the one `implementation=None|'torch'|'hip'` dispatch (neural_renderer_amd/_util.py: takes_hip) and of the
operators' messages that go through it."""
import pytest
import torch

NEEDS = 'the HIP kernels take float32 CUDA tensors with a batch size of at most 65535'


@pytest.mark.parametrize('implementation, fits, want', [
    (None, True, True), (None, False, False),
    ('torch', True, False), ('torch', False, False),
    ('hip', True, True),
])
def test_accepted_values(implementation, fits, want):
    from neural_renderer_amd import _util
    got = _util.takes_hip('op', implementation, fits, NEEDS)
    assert got is want


def test_hip_that_does_not_fit_raises_the_operators_sentence():
    from neural_renderer_amd import _util
    with pytest.raises(ValueError) as e:
        _util.takes_hip('op', 'hip', False, NEEDS)
    assert str(e.value) == 'op: ' + NEEDS


@pytest.mark.parametrize('implementation', ['HIP', 'cuda', '', 0, False, ('hip',)])
@pytest.mark.parametrize('fits', [True, False])
def test_unknown_value(implementation, fits):
    from neural_renderer_amd import _util
    for call in (lambda: _util.takes_hip('op', implementation, fits, NEEDS),
                 lambda: _util.check_implementation('op', implementation)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "op: implementation must be None, 'torch' or 'hip'"


def test_operator_messages_are_unchanged():
    """The texts that the operators raised before the dispatch had one definition, on CPU tensors (which never fit)."""
    import neural_renderer_amd as nr
    v = torch.tensor([[[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]])
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32)
    faces = v[:, f.long()] + torch.tensor([0., 0., 2.])
    colors = torch.ones((1, 4, 3))
    image = torch.rand((1, 8, 8))
    cases = [
        (lambda i: nr.face_normals(v, f, implementation=i), 'face_normals',
         'the HIP kernels take float32 CUDA tensors with a batch size of at most 65535'),
        (lambda i: nr.laplacian_loss(v, f, implementation=i), 'laplacian_loss',
         'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most'),
        (lambda i: nr.silhouette_iou_loss(image, image, implementation=i), 'silhouette_iou_loss',
         'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most'),
        (lambda i: nr.light_colors(v, f, nr.Lights(), implementation=i), 'light_colors',
         'the HIP kernels take float32 CUDA tensors and at most 65535 images'),
        (lambda i: nr.subdivide(v, f, 1, implementation=i), 'subdivision',
         'the HIP kernel takes float32 CUDA tensors with a batch size of 65535 and 16 channels at most'),
        (lambda i: nr.vertex_shade(v, f, v[0], implementation=i), 'vertex_shade',
         'the HIP kernels take float32 CUDA tensors and host light parameters'),
        (lambda i: nr.chamfer_distance(v, v, implementation=i), 'chamfer_distance',
         'there are no HIP kernels for the point-cloud losses; use implementation=None'),
        (lambda i: nr.soft_silhouettes(faces, 8, implementation=i), 'soft_silhouettes',
         'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most, at most 2^24 faces '
         '(batch size * faces * 9 < 2^31), an image_size of 16384 at most and 1e-30 <= sigma <= 1e30'),
        (lambda i: nr.soft_render(faces, colors, 8, implementation=i), 'soft_render',
         'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at most, at most 2^24 faces '
         '(batch size * faces * 9 < 2^31), an image_size of 16384 at most and sigma, gamma in [1e-30, 1e30]'),
    ]
    for call, name, needs in cases:
        with pytest.raises(ValueError) as e:
            call('hip')
        assert str(e.value) == '%s: %s' % (name, needs), name
        with pytest.raises(ValueError) as e:
            call('fast')
        assert str(e.value) == "%s: implementation must be None, 'torch' or 'hip'" % name, name
        call('torch')
        call(None)
