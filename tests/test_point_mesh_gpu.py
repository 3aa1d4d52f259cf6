"""Point-to-mesh distance on the GPU (csrc/nr_point_mesh.hip through neural_renderer_amd/point_mesh.py): every shape that
crosses a wave, a tile and a split with a remainder against the float64 restatement of tests/point_mesh_ref.py within its
derived bounds -- distances, assignments, weights, loss, both gradients, upstream gradients that differ per image --, the exact
lattice and the collapsed faces on the device, the bit-level properties (two runs, an image alone or in a batch, split or
not), non-finite input, layouts and streams, dispatch, a short fit and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

import point_mesh_ref as R
from test_point_mesh import (DIRECTIONS, REDUCTIONS, SHAPES, case, check_case, check_collapsed, check_lattice, check_loss, host,
                             tensors)

pytestmark = pytest.mark.gpu


def run_all(p, v, f, seed=9, implementation='hip', first=0):
    """Every output of the three operators and both gradients for fixed per-pair upstream gradients (those of the images
    first, first + 1, ... of a batch of four): a tuple of tensors"""
    import torch
    import neural_renderer_amd as nr
    p = p.detach().requires_grad_(p.dim() == 3 and p.shape[0] == v.shape[0])
    v = v.detach().requires_grad_(True)
    gen = torch.Generator().manual_seed(seed)
    ds, fid, ws = nr.closest_surface_points(p, v, f, implementation)
    dc, pid, wc = nr.closest_cloud_points(p, v, f, implementation)
    B = v.shape[0]
    gs = torch.rand((4,) + tuple(ds.shape[-1:]), generator=gen)[first:first + B].to(ds.device) - 0.5
    gc = torch.rand((4,) + tuple(dc.shape[-1:]), generator=gen)[first:first + B].to(ds.device) - 0.5
    loss = nr.point_mesh_distance(p, v, f, 'both', 'mean', implementation)
    gl = (torch.rand((4,), generator=gen)[first:first + B] + 0.5).to(ds.device)
    total = (ds * gs).sum() + (dc * gc).sum() + (loss * gl).sum()
    grads = torch.autograd.grad(total, [p, v] if p.requires_grad else [v])
    return (ds, fid, ws, dc, pid, wc, loss) + tuple(grads)


def same_bits(a, b):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), k


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_kernels_against_the_float64_restatement(k):
    points, vertices, faces = case(k)
    check_case(points, vertices, faces, device='cuda', implementation='hip', what='hip %s' % (SHAPES[k],))


@pytest.mark.parametrize('direction', DIRECTIONS)
@pytest.mark.parametrize('reduction', REDUCTIONS)
def test_loss_against_the_float64_restatement(direction, reduction):
    for k in (1, 3, 5):
        points, vertices, faces = case(k)
        check_loss(points, vertices, faces, direction, reduction, device='cuda', implementation='hip', what='hip %s' % (SHAPES[k],))


def test_random_triangles_at_three_distances():
    vertices, faces = R.triangle_soup(11, 400)
    check_case(R.cloud_near(12, vertices, faces, 1500), vertices, faces, device='cuda', implementation='hip', what='hip soup')


def test_lattice_is_exact_on_the_device(monkeypatch):
    from neural_renderer_amd import point_mesh
    for split in (0, 1, 3):
        monkeypatch.setattr(point_mesh, '_SPLIT', split)
        check_lattice('cuda', 'hip')


def test_collapsed_faces_on_the_device():
    check_collapsed('cuda', 'hip')


def test_two_runs_and_an_image_alone_have_the_same_bits():
    for k in (2, 3):
        points, vertices, faces = case(k)
        p, v, f = tensors(points, vertices, faces, device='cuda')
        first = run_all(p, v, f)
        same_bits(first, run_all(p, v, f))
        b = vertices.shape[0] - 1
        alone = run_all(p if p.dim() == 2 else p[b:b + 1], v[b:b + 1], f, first=b)
        for x, y in zip(first, alone):
            if x.dim() == y.dim() and x.shape[0] == vertices.shape[0]:  # (a shared cloud has no batch axis and no gradient)
                same_bits((x[b:b + 1],), (y,))


def test_split_and_unsplit_agree_to_the_bit(monkeypatch):
    from neural_renderer_amd import _lib, point_mesh
    lib = _lib.load()
    for k in (5, 3, 2):
        B, N, F, _ = SHAPES[k]
        points, vertices, faces = case(k)
        p, v, f = tensors(points, vertices, faces, device='cuda')
        monkeypatch.setattr(point_mesh, '_SPLIT', 1)
        assert lib.nr_point_mesh_workspace_bytes(B, N, F, 0, 1) == 0
        unsplit = run_all(p, v, f)
        for split in (0, 2, 3, 1000):
            monkeypatch.setattr(point_mesh, '_SPLIT', split)
            same_bits(unsplit, run_all(p, v, f))
    assert lib.nr_point_mesh_workspace_bytes(1, 70, 5000, 0, 0) > 0      # (1, 70, 5000) splits its faces by itself
    assert lib.nr_point_mesh_workspace_bytes(2, 1027, 515, 1, 3) > 0


def test_non_finite_input_on_the_device():
    import torch
    import neural_renderer_amd as nr
    points, vertices, faces = case(1)
    bad, moved = vertices.copy(), vertices.copy()
    bad[:, 5] = np.nan
    moved[:, 5] = 1000.0
    p, v, f = tensors(points, bad, faces, device='cuda')
    vm = torch.tensor(moved, device='cuda')
    touched = torch.tensor((faces == 5).any(1), device='cuda')
    d, i, w = nr.closest_surface_points(p, v, f, 'hip')
    d2, i2, w2 = nr.closest_surface_points(p, vm, f, 'hip')
    assert not touched[i].any() and torch.isfinite(d).all()
    other = ~touched[i2]
    assert int(other.sum()) > other.numel() // 2
    assert torch.equal(d[other], d2[other]) and torch.equal(i[other], i2[other]) and torch.equal(w[other], w2[other])
    dc, ic, wc = nr.closest_cloud_points(p, v, f, 'hip')
    dc2, ic2, wc2 = nr.closest_cloud_points(p, vm, f, 'hip')
    keep = ~touched
    assert torch.equal(dc[:, keep], dc2[:, keep]) and torch.equal(ic[:, keep], ic2[:, keep]) and torch.equal(wc[:, keep], wc2[:, keep])
    assert (ic[:, touched] == 0).all() and not torch.isfinite(dc[:, touched]).any()
    pn = p.clone()
    pn[0, 3] = float('nan')
    d, i, w = nr.closest_surface_points(pn, torch.tensor(vertices, device='cuda'), f, 'hip')
    assert int(i[0, 3]) == 0 and not torch.isfinite(d[0, 3]) and int(i.min()) >= 0 and int(i.max()) < faces.shape[0]
    dc, ic, wc = nr.closest_cloud_points(pn, torch.tensor(vertices, device='cuda'), f, 'hip')
    assert not (ic[0] == 3).any() and torch.isfinite(dc).all()
    loss = nr.point_mesh_distance(pn.requires_grad_(True), v.requires_grad_(True), f, implementation='hip')
    loss.sum().backward()   # non-finite values flow through without leaving the buffers


def test_layouts_and_a_side_stream_have_the_dense_call_s_bits():
    import torch
    points, vertices, faces = case(2)
    p, v, f = tensors(points, vertices, faces, device='cuda')
    dense = run_all(p, v, f)
    assert all(float(t.detach().abs().sum()) > 0 for t in (dense[0], dense[-1], dense[-2]))

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
    torch.cuda.current_stream().wait_stream(side)
    same_bits(dense, on_side)


def test_grad_output_as_an_expanded_scalar():
    import torch
    import neural_renderer_amd as nr
    points, vertices, faces = case(2)
    p, v, f = tensors(points, vertices, faces, device='cuda', grad=True)
    nr.closest_surface_points(p, v, f, 'hip')[0].sum().backward()   # (the gradient of .sum() has stride 0)
    nr.point_mesh_distance(p, v, f, implementation='hip').sum().backward()
    got = (p.grad.clone(), v.grad.clone())
    p.grad = v.grad = None
    d = nr.closest_surface_points(p, v, f, 'hip')[0]
    d.backward(torch.ones_like(d))
    loss = nr.point_mesh_distance(p, v, f, implementation='hip')
    loss.backward(torch.ones_like(loss))
    same_bits(got, (p.grad, v.grad))


def test_dispatch(monkeypatch):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import _lib, point_mesh
    points, vertices, faces = case(1)
    p, v, f = tensors(points, vertices, faces, device='cuda')
    hip = nr.point_mesh_distance(p, v, f)
    eager = nr.point_mesh_distance(p, v, f, implementation='torch')
    want, bnd = R.loss(points, vertices, faces, 'both', 'mean', 2)
    assert (np.abs(host(hip).astype(np.float64) - host(eager)) <= 2 * bnd).all()
    with pytest.raises(ValueError) as err:
        nr.point_mesh_distance(p.double(), v.double(), f, implementation='hip')
    assert point_mesh._NEEDS in str(err.value)
    with pytest.raises(ValueError):   # a shared cloud that requires a gradient
        nr.point_mesh_distance(p[0].clone().requires_grad_(True), v, f, implementation='hip')

    def no_launch(*a, **k):
        raise AssertionError('a kernel was launched')

    calls = []
    launch = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: (calls.append(name), launch(name, *a, **k))[1])
    nr.point_mesh_distance(p, v, f, 'points_to_mesh')
    assert calls == ['nr_point_mesh_points_to_faces', 'nr_point_mesh_loss']
    del calls[:]
    nr.point_mesh_distance(p, v, f, 'mesh_to_points')
    assert calls == ['nr_point_mesh_faces_to_points', 'nr_point_mesh_loss']
    monkeypatch.setattr(_lib, 'launch', no_launch)
    assert nr.point_mesh_distance(p.double(), v.double(), f).dtype == torch.float64       # float64 on the device: plain torch
    assert nr.point_mesh_distance(p[0].clone().requires_grad_(True), v, f).requires_grad  # a shared learnable cloud too


def test_a_short_fit_descends():
    import torch
    import neural_renderer_amd as nr
    rng = np.random.default_rng(21)
    target = rng.normal(size=(2000, 3))
    target = torch.tensor(0.8 * target / np.linalg.norm(target, axis=1, keepdims=True) * np.array([1.0, 0.7, 0.5]),
                          dtype=torch.float32, device='cuda')
    sphere, faces = nr.icosphere(2, 0.5, device='cuda')
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=1e-2)
    losses = []
    for _ in range(11):
        optimizer.zero_grad()
        loss = nr.point_mesh_distance(target, vertices, faces) + 0.1 * nr.laplacian_loss(vertices, faces)
        loss.backward()
        assert torch.isfinite(vertices.grad).all() and float(vertices.grad.abs().sum()) > 0
        optimizer.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


def test_example_point_mesh_runs():
    """examples/example_point_mesh.py as a child process with 20 steps: it exits 0 and its last printed loss is below its first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    out = os.path.join(ex, 'data', 'example_point_mesh_test.obj')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_point_mesh.py'), '20', '-oo', out], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
