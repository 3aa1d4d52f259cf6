"""Winding numbers on the GPU (csrc/nr_winding.hip through neural_renderer_amd/winding.py): every shape that crosses a wave, a
tile and the points of a workgroup with a remainder against the float64 restatement of tests/winding_ref.py within its derived
bounds and against the float32 torch path within the sum of both bounds -- w and both gradients, upstream gradients that differ
per image --, the analytic pins and every edge rule on the device, the bit-level properties (two runs, an image alone or in
a batch, split or not, a scene scaled by a power of two, layouts and streams), the voxel grid of a sphere, the cancellation
inside a closed mesh, dispatch and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

import winding_ref as R
from test_winding import (SHAPES, T, case, check_ball, check_case, check_collapsed, check_lattice_cube, check_non_finite, check_pins,
                          check_point_on_a_vertex, check_power_of_two_scaling, check_signed_distance, host, sphere, tensors)

pytestmark = pytest.mark.gpu


def run_all(p, v, f, seed=9, implementation='hip', first=0):
    """w and both gradients for fixed per-entry upstream gradients (those of the images first, first + 1, ... of a batch of
    four): a tuple of tensors"""
    import torch
    import neural_renderer_amd as nr
    p = p.detach().requires_grad_(p.dim() == 3 and p.shape[0] == v.shape[0])
    v = v.detach().requires_grad_(True)
    w = nr.winding_number(p, v, f, implementation)
    g = torch.rand((4, w.shape[-1]), generator=torch.Generator().manual_seed(seed))[first:first + v.shape[0]].to(w.device) - 0.5
    grads = torch.autograd.grad((w * g).sum(), [p, v] if p.requires_grad else [v])
    return (w,) + tuple(grads)


def same_bits(a, b):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), k


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_kernels_against_the_float64_restatement(k):
    points, vertices, faces = case(k)
    check_case(points, vertices, faces, device='cuda', implementation='hip', what='hip %s' % (SHAPES[k],))


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_kernels_against_the_torch_path(k):
    """|hip - torch| within the sum of the two paths' bounds, entry by entry (both are float32 chains of the same count)"""
    import torch
    points, vertices, faces = case(k)
    B, Nv = vertices.shape[:2]
    out = {}
    for implementation in ('hip', 'torch'):
        p, v, f = tensors(points, vertices, faces, device='cuda')
        out[implementation] = run_all(p, v, f, implementation=implementation)
    w_bound = R.winding(points, vertices, faces)[1]
    g = host(torch.rand((4, points.shape[-2]), generator=torch.Generator().manual_seed(9))[:B] - 0.5)
    (_, bp), (_, bv) = R.gradients(np.broadcast_to(points, (B,) + points.shape[-2:]), vertices, faces, g, Nv)
    bounds = (w_bound,) + ((bp, bv) if len(out['hip']) == 3 else (bv,))
    ratios = [R.ratio(host(x), host(y).astype(np.float64), 2 * b) for x, y, b in zip(out['hip'], out['torch'], bounds)]
    print('hip against torch %s: ratios %s' % (SHAPES[k], ratios))
    assert max(ratios) <= 1.0, ratios


def test_analytic_pins_on_the_device():
    check_pins('cuda', 'hip')


def test_collapsed_faces_on_the_device():
    check_collapsed('cuda', 'hip')


def test_a_point_on_a_vertex_on_the_device():
    check_point_on_a_vertex('cuda', 'hip')


def test_non_finite_coordinates_on_the_device():
    check_non_finite('cuda', 'hip')


def test_power_of_two_scaling_on_the_device():
    check_power_of_two_scaling('cuda', 'hip')


def test_two_runs_and_an_image_alone_have_the_same_bits():
    for k in (1, 2, 4):
        points, vertices, faces = case(k)
        p, v, f = tensors(points, vertices, faces, device='cuda')
        first = run_all(p, v, f)
        same_bits(first, run_all(p, v, f))
        b = vertices.shape[0] - 1
        alone = run_all(p if p.dim() == 2 else p[b:b + 1], v[b:b + 1], f, first=b)
        same_bits(tuple(x[b:b + 1] for x in first), alone)


def split_cases():
    """SHAPES 4 and 2 (three tiles of faces and of points at the most), and seven tiles of each: seven parts are seven parts"""
    yield case(4)
    yield case(2)
    v, f = sphere(4)
    yield R.shell_points(70, 6 * T + 5, 1.0, 1), v[None], f[:6 * T + 9].copy()


def test_split_and_unsplit_agree_to_the_bit(monkeypatch):
    from neural_renderer_amd import _lib, winding
    lib = _lib.load()
    for points, vertices, faces in split_cases():
        B, N, F = vertices.shape[0], points.shape[-2], faces.shape[0]
        p, v, f = tensors(points, vertices, faces, device='cuda')
        monkeypatch.setattr(winding, '_SPLIT', 1)
        assert lib.nr_winding_workspace_bytes(B, N, F, 0, 1) == 0 and lib.nr_winding_workspace_bytes(B, N, F, 1, 1) == 0
        unsplit = run_all(p, v, f)
        for split in (0, 2, 3, 7):
            monkeypatch.setattr(winding, '_SPLIT', split)
            same_bits(unsplit, run_all(p, v, f))
    assert lib.nr_winding_workspace_bytes(1, 6 * T + 5, 6 * T + 9, 0, 7) == 7 * (6 * T + 5) * 8      # seven tiles of faces
    assert lib.nr_winding_workspace_bytes(1, 6 * T + 5, 6 * T + 9, 2, 7) > 9 * 7 * (6 * T + 9) * 8   # seven tiles of points
    assert lib.nr_winding_workspace_bytes(1, 6 * T + 5, 6 * T + 9, 0, 0) > 0                         # and split by itself


def test_layouts_and_a_side_stream_have_the_dense_call_s_bits():
    import torch
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces, device='cuda')
    dense = run_all(p, v, f)
    assert all(float(t.detach().abs().sum()) > 0 for t in dense)

    def offset(x, k):
        flat = torch.zeros(x.numel() + k, dtype=x.dtype, device=x.device)
        flat[k:] = x.reshape(-1)
        return flat[k:].view(x.shape)

    def strided(x):
        wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=x.dtype, device=x.device)
        wide[..., ::2] = x
        return wide[..., ::2]

    def permuted(x):
        return x.permute(*reversed(range(x.dim()))).contiguous().permute(*reversed(range(x.dim())))

    for name, change in (('offset4', lambda x: offset(x, 1)), ('offset8', lambda x: offset(x, 2)),
                         ('offset12', lambda x: offset(x, 3)), ('strided', strided), ('permuted', permuted)):
        assert not (change(p).is_contiguous() and change(p).data_ptr() % 16 == 0), name
        same_bits(dense, run_all(change(p), change(v), change(f)))
    same_bits(dense, run_all(p, v, f.long()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run_all(p, v, f)
        on_side_offset = run_all(offset(p, 1), strided(v), f)
    torch.cuda.current_stream().wait_stream(side)
    same_bits(dense, on_side)
    same_bits(dense, on_side_offset)


def test_grad_output_as_an_expanded_scalar():
    import torch
    import neural_renderer_amd as nr
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces, device='cuda', grad=True)
    nr.winding_number(p, v, f, 'hip').sum().backward()   # (the gradient of .sum() has stride 0)
    got = (p.grad.clone(), v.grad.clone())
    p.grad = v.grad = None
    w = nr.winding_number(p, v, f, 'hip')
    w.backward(torch.ones_like(w))
    same_bits(got, (p.grad, v.grad))


def test_voxelize_of_the_lattice_cube_on_the_device():
    check_lattice_cube('cuda', 'hip')


def test_voxelize_of_a_sphere_is_the_ball_off_its_surface():
    check_ball('cuda', 'hip')


def test_signed_distance_on_the_device():
    check_signed_distance('cuda', 'hip')


def test_inside_a_closed_mesh_the_gradients_cancel():
    """w = 1 wherever the vertices are: both gradients are 0 in exact arithmetic, and within their magnitude-based bounds of it"""
    v, f = sphere()
    points = R.shell_points(80, 200, 1.0, 2, gap=0.2)[:, 0::2]      # the inner ones
    vertices = R.batch_of(v, 2, 81)
    g = np.random.default_rng(1).uniform(-1, 1, (2, 100)).astype(np.float32)   # check_case's own upstream
    (gp, bp), (gv, bv) = R.gradients(points, vertices, f, g, len(v))
    assert np.abs(gp).max() <= 1e-12 and np.abs(gv).max() <= 1e-12 and bp.min() > 1e-9 and bv[:, np.unique(f)].min() > 1e-9
    (w, grad_p, grad_v), _ = check_case(points, vertices, f, device='cuda', implementation='hip', what='hip closed')
    assert float((w - 1).abs().max()) <= 1e-5
    assert (np.abs(host(grad_p)) <= bp + 1e-12).all() and (np.abs(host(grad_v)) <= bv + 1e-12).all()


def test_dispatch(monkeypatch):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import _lib, winding
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces, device='cuda')
    with pytest.raises(ValueError) as err:
        nr.winding_number(p.double(), v.double(), f, implementation='hip')
    assert winding._NEEDS in str(err.value)
    with pytest.raises(ValueError):   # a shared cloud that requires a gradient
        nr.winding_number(p[0].clone().requires_grad_(True), v, f, implementation='hip')

    def no_launch(*a, **k):
        raise AssertionError('a kernel was launched')

    calls = []
    launch = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: (calls.append(name), launch(name, *a, **k))[1])
    w = nr.winding_number(p, v.requires_grad_(True), f)
    assert calls == ['nr_winding_forward']
    w.sum().backward()                 # points without a gradient: their kernel is not launched
    assert calls == ['nr_winding_forward', 'nr_winding_backward_vertices']
    del calls[:]
    nr.winding_number(p.requires_grad_(True), v.detach(), f).sum().backward()
    assert calls == ['nr_winding_forward', 'nr_winding_backward_points']
    del calls[:]
    assert nr.mesh_occupancy(p, v, f).dtype == torch.bool and nr.voxelize(v, f, 4).dtype == torch.float32
    assert calls == ['nr_winding_forward', 'nr_winding_forward']
    monkeypatch.setattr(_lib, 'launch', no_launch)
    assert nr.winding_number(p.double(), v.double(), f).dtype == torch.float64            # float64 on the device: plain torch
    assert nr.winding_number(p[0].detach().clone().requires_grad_(True), v, f).requires_grad  # a shared learnable cloud too


def test_example_voxel_fit_runs():
    """examples/example_voxel_fit.py as a child process at its small size: it exits 0 and its voxel IoU after is above before."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_voxel_fit.py'), '25', '-s', '12'], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    line = [x for x in run.stdout.splitlines() if x.startswith('voxel IoU')][-1].split()
    before, after = float(line[2]), float(line[4])
    assert after > before, (before, after)
