"""Point-cloud losses on the GPU (neural_renderer_amd/point_losses.py): the implementation is plain torch, so these tests
run it on the device -- where its index_add adds with atomics in no fixed order -- entry by entry against the float64
restatement of tests/point_loss_ref.py within its derived bounds, the exact lattice case, non-finite input, sampling with
a device generator, the chain into a mesh fit, what a graph capture refuses, and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

import point_loss_ref as R
from test_point_losses import DIRECTIONS, REDUCTIONS, check_chamfer, check_points, run_chamfer, run_points, surface_case

pytestmark = pytest.mark.gpu

# (B, N, M, shared y): one point, odd sizes, more points than a block of any reduction
SHAPES = ((1, 1, 1, False), (2, 63, 255, False), (3, 257, 65, False), (2, 1027, 515, True), (3, 1, 515, False))


def _cuda(a, **kw):
    import torch
    return torch.tensor(a, device='cuda', **kw)


def test_nearest_against_the_float64_restatement():
    import neural_renderer_amd as nr
    for k, (B, N, M, shared) in enumerate(SHAPES):
        x, y = R.clouds(100 + k, B, N, M, shared_y=shared)
        d, i = nr.nearest_points(_cuda(x), _cuda(y))
        assert d.dtype.is_floating_point and d.is_cuda and str(i.dtype) == 'torch.int64'
        R.check_nearest(d.cpu().numpy(), i.cpu().numpy(), x, y, what='cuda B%d N%d M%d shared=%s' % (B, N, M, shared))


@pytest.mark.parametrize('reduction', REDUCTIONS)
@pytest.mark.parametrize('direction', DIRECTIONS)
def test_chamfer_against_the_float64_restatement(direction, reduction):
    """Loss, grad_x and grad_y with upstream gradients that differ per image; the float32 chain's constant (K + 4) u holds
    for any order of the scattered additions."""
    for k, (B, N, M, shared) in enumerate(SHAPES):
        x, y = R.clouds(200 + k, B, N, M, shared_y=shared)
        yb = np.broadcast_to(y, (B, M, 3)).copy() if shared else y
        gl = np.array([0.7, -1.3, 2.1], np.float32)[:B]
        got = run_chamfer(x, y, gl, direction, reduction, device='cuda', y_grad=not shared)
        assert got[0].dtype == np.float32 and got[0].shape == (B,) and (got[2] is None) == shared
        check_chamfer(x, yb, gl, direction, reduction, got, extra=4, what='cuda B%d N%d M%d shared=%s' % (B, N, M, shared))


def test_lattice_is_exact_and_ties_go_to_the_lowest_index():
    import neural_renderer_amd as nr
    x, y = R.lattice()
    assert R.tied_rows(x, y) == 97
    for q, db in ((x, y), (y, x)):
        d_ref, i_ref = R.nearest(q[None], db[None])
        d, i = nr.nearest_points(_cuda(q), _cuda(db))
        assert np.array_equal(d.cpu().numpy().astype(np.float64), d_ref[0]) and np.array_equal(i.cpu().numpy(), i_ref[0])


def test_non_finite_points_stay_in_bounds():
    """A NaN point in y is nobody's nearest: every idx is in range and every row has the bits of the same call with that
    point moved far away."""
    import torch
    import neural_renderer_amd as nr
    x, y = R.clouds(600, 2, 300, 257)
    bad, moved = y.copy(), y.copy()
    bad[1, 7], moved[1, 7] = np.nan, 1000.0
    d1, i1 = nr.nearest_points(_cuda(x), _cuda(bad))
    d2, i2 = nr.nearest_points(_cuda(x), _cuda(moved))
    assert int(i1.min()) >= 0 and int(i1.max()) < 257 and not bool((i1[1] == 7).any())
    assert torch.equal(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))


@pytest.mark.parametrize('kw', [{}, {'skip_face': 1}, {'only_face': 2}])
def test_surface_points_against_the_float64_restatement(kw):
    vb, f, ids, w, g = surface_case(B=3, N=300, **kw)
    points, grad, _ = run_points(vb, f, ids, w, g, device='cuda')
    check_points(vb, f, ids, w, g, points, grad, what='cuda patch %s' % kw)
    assert (grad[:, 7] == 0).all()


def test_sample_surface_on_the_device():
    import torch
    import neural_renderer_amd as nr
    v, f = nr.icosphere(2)
    rng = np.random.default_rng(0)
    vb = (v.numpy()[None] * rng.uniform(0.5, 1.5, (3, 1, 1))).astype(np.float32)
    vt, ft = _cuda(vb), f.cuda()
    points, s = nr.sample_surface_points(vt, ft, 1500, torch.Generator(device='cuda').manual_seed(5))
    assert s.face_ids.is_cuda and s.face_ids.dtype == torch.int32 and tuple(points.shape) == (3, 1500, 3)
    ids, w = s.face_ids.cpu().numpy(), s.barycentric.cpu().numpy()
    R.check_samples(ids, w, s.segment_offsets.cpu().numpy(), len(f))
    value, mag = R.surface_points(vb, f.numpy(), ids, w)
    assert R._ratio(np.abs(points.cpu().numpy().astype(np.float64) - value), 3 * R.U * mag) <= 1.0
    again = nr.sample_surface(vt, ft, 1500, torch.Generator(device='cuda').manual_seed(5))
    assert torch.equal(again.face_ids, s.face_ids) and torch.equal(again.barycentric, s.barycentric)
    assert np.bincount(ids[0], minlength=len(f)).max() < 40  # 1500 samples on 320 equal faces: about 4.7 each


def test_dispatch():
    import torch
    import neural_renderer_amd as nr
    x, y = R.clouds(700, 2, 40, 50)
    loss = nr.chamfer_distance(_cuda(x, dtype=torch.float64), _cuda(y, dtype=torch.float64))
    ref = R.chamfer_loss(x, y, 'both', 'mean')
    assert loss.dtype == torch.float64 and (np.abs(loss.cpu().numpy() - ref) <= R.loss_bound(ref, R.U64)).all()
    with pytest.raises(ValueError):
        nr.chamfer_distance(_cuda(x), _cuda(y), implementation='hip')   # no kernels behind these functions
    xt, ys = _cuda(x, requires_grad=True), _cuda(y[0], requires_grad=True)
    nr.chamfer_distance(xt, ys).sum().backward()     # a shared learnable y: its gradient sums over the batch
    assert tuple(ys.grad.shape) == (50, 3) and tuple(xt.grad.shape) == (2, 40, 3)


def test_chain_into_a_mesh_fit(monkeypatch):
    """icosphere(2) -> sample_surface_points -> chamfer_distance to a fixed cloud, + laplacian_loss: the gradients reach the
    vertices, are finite, and ten Adam steps lower the loss.  Drawing and checking samples read values back, so inside a
    graph capture they raise (the capture state is simulated; nothing is captured)."""
    import torch
    import neural_renderer_amd as nr
    v, f = nr.icosphere(2, 0.6, device='cuda')
    target = _cuda(R.clouds(900, 1, 1, 2000)[1][0] * np.float32(0.4))
    vertices = torch.nn.Parameter(v.clone())
    samples = nr.sample_surface(vertices, f, 1500, torch.Generator(device='cuda').manual_seed(1))
    opt = torch.optim.Adam([vertices], lr=2e-2)
    losses = []
    for _ in range(11):
        opt.zero_grad()
        loss = nr.chamfer_distance(samples.points(vertices, f), target) + 0.1 * nr.laplacian_loss(vertices, f)
        loss.backward()
        assert bool(torch.isfinite(vertices.grad).all()) and float(vertices.grad.abs().sum()) > 0
        losses.append(float(loss))
        opt.step()
    print('chain: loss %.5f -> %.5f' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError):
        nr.SurfaceSamples(samples.face_ids, samples.barycentric, samples.num_faces)
    with pytest.raises(RuntimeError):
        nr.sample_surface(vertices, f, 16)


def test_example_chamfer_runs():
    """examples/example_chamfer.py as a child process with 20 steps: it exits 0 and its last printed loss is below its first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import make_data
    make_data.main()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    out = os.path.join(ex, 'data', 'example_chamfer_test.obj')
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_chamfer.py'), '20', '-oo', out], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
