"""Mesh losses on the GPU (include/nr_hip.h nr_laplacian_forward / _backward, nr_flatness_forward / _backward;
neural_renderer_amd/mesh_losses.py): both losses and both gradients entry by entry against the float64 restatement of
tests/mesh_loss_ref.py within the constants of tests/test_mesh_losses.py, bit-for-bit repetition, the batch against its
slices, the torch path, autograd plumbing next to a render, and graph capture."""
import numpy as np
import pytest

import mesh_loss_ref as R
from test_mesh_losses import CONSTANTS, loss_and_grad, ratios

pytestmark = pytest.mark.gpu

KINDS = ['laplacian', 'flatness']


def _fn(kind):
    import neural_renderer_amd as nr
    return nr.laplacian_loss if kind == 'laplacian' else nr.flatness_loss


def _check(kind, name, seed):
    v, f = R.inputs(name, seed)
    loss, grad = loss_and_grad(_fn(kind), v, f, _f32(), device='cuda', implementation='hip')
    rl, rg = ratios(kind, name, seed, loss, grad)
    print('%s %s seed %d: loss at %.3f of u M (C = %d), gradient at %.3f (C = %d)'
          % (kind, name, seed, rl, CONSTANTS[kind, 'loss'], rg, CONSTANTS[kind, 'grad']))
    assert rl <= CONSTANTS[kind, 'loss'] and rg <= CONSTANTS[kind, 'grad']
    return loss, grad


def _f32():
    import torch
    return torch.float32


@pytest.mark.parametrize('name', R.MESHES)
@pytest.mark.parametrize('kind', KINDS)
def test_against_the_float64_restatement(kind, name):
    """Every mesh, B = 3, every seed of the noisy ones.  Measured on the MI355X: see the lines this test prints
    (LAB-NOTEBOOK.md "Mesh losses" keeps the worst of a run)."""
    for seed in R.seeds_of(name):
        _check(kind, name, seed)


@pytest.mark.parametrize('name', R.ODD)
@pytest.mark.parametrize('kind', KINDS)
def test_odd_topology_and_several_blocks(kind, name):
    """'odd': an isolated vertex (delta = 0, gradient exactly 0: its magnitude is 0), a duplicated face, a face with a
    repeated index, an edge in three faces.  'blocks': 648 vertices / 1 920 quads, three / eight blocks of 256 per image, the
    last one partly filled: the block-order reduction."""
    for seed in R.seeds_of(name):
        loss, grad = _check(kind, name, seed)
        if name == 'odd':
            assert not grad[:, 42].any()


@pytest.mark.parametrize('kind', KINDS)
def test_degenerate_quads_stay_finite(kind):
    """A zero-length edge and an opposite vertex on its edge's line: finite, and within the same constants."""
    loss, grad = _check(kind, 'degenerate', 0)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()


@pytest.mark.parametrize('kind', KINDS)
def test_flat_grid_and_no_quads_on_the_kernels(kind):
    import torch
    v, f = R.inputs('grid_flat')
    loss, _ = loss_and_grad(_fn(kind), v, f, torch.float32, device='cuda', implementation='hip')
    if kind == 'flatness':
        assert (loss >= 0).all() and (loss <= 176 * 4e-6).all()
    # one triangle: no quad -- an exact 0 and exact zeros from the kernels too
    x = torch.tensor(v[:, :3].copy(), device='cuda', requires_grad=True)
    one = _fn('flatness')(x, torch.tensor([[0, 1, 2]], device='cuda'), implementation='hip')
    grad, = torch.autograd.grad(one.sum(), x)
    assert one.shape == (3,) and not one.any() and grad.shape == x.shape and not grad.any()


@pytest.mark.parametrize('kind', KINDS)
def test_two_runs_and_batch_slices_give_the_same_bits(kind):
    import torch
    v, f = R.inputs('blocks', 1)
    a = loss_and_grad(_fn(kind), v, f, torch.float32, device='cuda', implementation='hip')
    b = loss_and_grad(_fn(kind), v, f, torch.float32, device='cuda', implementation='hip')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    faces = torch.tensor(f, device='cuda')
    for k in range(v.shape[0]):   # every image alone: the same bits as inside the batch
        x = torch.tensor(v[k:k + 1], device='cuda', requires_grad=True)
        loss = _fn(kind)(x, faces, implementation='hip')
        grad, = torch.autograd.grad(loss[0] * float(R.UPSTREAM[k]), x)
        assert np.array_equal(loss.detach().cpu().numpy(), a[0][k:k + 1])
        assert np.array_equal(grad.cpu().numpy(), a[1][k:k + 1])


@pytest.mark.parametrize('kind', KINDS)
def test_hip_and_torch_agree(kind):
    """Within 2 C of the same magnitudes (each within C of the restatement)."""
    import torch
    for name in ('ico2', 'odd', 'blocks'):
        v, f = R.inputs(name, 2)
        ref = R.reference(kind, name, 2)
        hip = loss_and_grad(_fn(kind), v, f, torch.float32, device='cuda', implementation='hip')
        tor = loss_and_grad(_fn(kind), v, f, torch.float32, device='cuda', implementation='torch')
        default = loss_and_grad(_fn(kind), v, f, torch.float32, device='cuda')
        assert np.array_equal(default[0], hip[0]) and np.array_equal(default[1], hip[1])   # None picks the kernels here
        assert R.worst_ratio(hip[0], tor[0], ref.loss_mag) <= 2 * CONSTANTS[kind, 'loss']
        assert R.worst_ratio(hip[1], tor[1], ref.grad_mag) <= 2 * CONSTANTS[kind, 'grad']
        # other dtypes take the torch path on the device
        x64 = torch.tensor(v, dtype=torch.float64, device='cuda')
        l64 = _fn(kind)(x64, torch.tensor(f, device='cuda'))
        assert l64.dtype == torch.float64
        assert np.abs(l64.cpu().numpy() - ref.loss).max() <= 1e-12 * np.abs(ref.loss).max()


@pytest.mark.parametrize('kind', KINDS)
def test_single_mesh_gives_a_0_dim_loss(kind):
    import torch
    v, f = R.inputs('ico1', 3)
    faces = torch.tensor(f, device='cuda')
    x = torch.tensor(v[1], device='cuda', requires_grad=True)
    loss = _fn(kind)(x, faces, implementation='hip')
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    xb = torch.tensor(v[1:2], device='cuda', requires_grad=True)
    lb = _fn(kind)(xb, faces, implementation='hip')
    lb.sum().backward()
    assert torch.equal(loss.detach(), lb.detach()[0]) and torch.equal(x.grad, xb.grad[0])
    # a batch that is a view (Mesh.get_batch's expand) is read as it is
    xe = x.detach()[None].expand(2, -1, -1)
    assert torch.equal(_fn(kind)(xe, faces, implementation='hip'), lb.detach().expand(2))


@pytest.mark.parametrize('kind', KINDS)
def test_no_backward_launch_without_a_vertex_gradient(kind):
    """ctx.needs_input_grad: with vertices that require no gradient the loss is a constant of the graph, and a backward
    through what it is combined with launches neither backward kernel."""
    import torch
    from neural_renderer_amd import _lib
    lib = _lib.load()
    names = ('nr_laplacian_backward', 'nr_flatness_backward')
    real = {n: getattr(lib, n) for n in names}
    calls = []

    def counting(n):
        def call(*args):
            calls.append(n)
            return real[n](*args)
        return call
    v, f = R.inputs('ico1')
    faces = torch.tensor(f, device='cuda')
    try:
        for n in names:
            setattr(lib, n, counting(n))
        scale = torch.ones(3, device='cuda', requires_grad=True)
        loss = _fn(kind)(torch.tensor(v, device='cuda'), faces, implementation='hip')
        assert not loss.requires_grad
        (loss * scale).sum().backward()
        assert torch.equal(scale.grad, loss) and calls == []
        x = torch.tensor(v, device='cuda', requires_grad=True)     # ... and with one, exactly one launch
        (_fn(kind)(x, faces, implementation='hip') * scale).sum().backward()
        assert calls == ['nr_%s_backward' % kind]
    finally:
        for n in names:
            setattr(lib, n, real[n])


def test_regularisers_next_to_a_silhouette_loss():
    """One render_silhouettes loss plus both regularisers on the SAME vertices tensor: vertices.grad is the sum of the three
    gradients taken separately, within float addition: autograd's accumulation order is its own (two roundings of the sum
    of the three magnitudes on either side: 4 u), and the renderer's front-end scatters its face gradients into the vertices
    with float atomics, whose order differs from run to run: up to (n - 1) u of the sum of |terms| for the n <= 16 corner
    terms of a vertex, which 64 u of the largest silhouette gradient entry covers with room for cancellation."""
    import torch
    import neural_renderer_amd as nr
    v, f = R.inputs('ico2', 4)
    faces = torch.tensor(f, device='cuda')[None].expand(3, -1, -1)
    r = nr.Renderer()
    r.image_size = 64
    r.eye = nr.get_points_from_angles(2.732, 20, 40)
    target = torch.zeros((3, 64, 64), device='cuda')
    target[:, 16:48, 16:48] = 1

    def terms(x):
        return (((r.render_silhouettes(x, faces) - target) ** 2).sum(), 0.3 * nr.laplacian_loss(x, faces).sum(),
                0.1 * nr.flatness_loss(x, faces).sum())
    x = torch.tensor(v, device='cuda', requires_grad=True)
    sum(terms(x)).backward()
    parts = []
    for k in range(3):
        xk = torch.tensor(v, device='cuda', requires_grad=True)
        terms(xk)[k].backward()
        parts.append(xk.grad)
        assert parts[-1].abs().sum() > 0
    want = parts[0] + parts[1] + parts[2]
    mags = parts[0].abs() + parts[1].abs() + parts[2].abs()
    assert ((x.grad - want).abs() <= 2.0 ** -22 * mags + 2.0 ** -18 * parts[0].abs().max()).all()
    # the two regularisers alone: no atomics anywhere, so only the accumulation's roundings are left
    x2 = torch.tensor(v, device='cuda', requires_grad=True)
    (terms(x2)[1] + terms(x2)[2]).backward()
    assert ((x2.grad - (parts[1] + parts[2])).abs() <= 2.0 ** -23 * (parts[1].abs() + parts[2].abs())).all()


def test_graph_capture_equals_eager():
    """A step -- both losses and their gradients -- captured with neural_renderer_amd.graph.capture replays equal to eager.
    The tables are built on the host: one eager call with the same index tensor comes first, and without one a capture
    raises."""
    import torch
    import neural_renderer_amd as nr
    v, f = R.inputs('blocks', 3)
    vertices = torch.tensor(v, device='cuda', requires_grad=True)
    faces = torch.tensor(f, device='cuda')
    out = torch.zeros((2, 3), device='cuda')
    w = torch.tensor(R.UPSTREAM, dtype=torch.float32, device='cuda')

    def step():
        lap, flat = nr.laplacian_loss(vertices, faces), nr.flatness_loss(vertices, faces)
        out[0].copy_(lap)
        out[1].copy_(flat)
        return torch.autograd.grad(((lap + 0.5 * flat) * w).sum(), [vertices])
    with torch.no_grad():
        nr.laplacian_loss(vertices, faces)     # builds the tables (and checks the indices) eagerly
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        vertices.copy_(torch.tensor(R.inputs('blocks', 4)[0]))
    replay()
    torch.cuda.synchronize()
    got_out, got = out.clone(), grads[0][0].clone()
    eager = step()
    assert torch.equal(got_out, out) and torch.equal(got, eager[0])


def test_unknown_topology_raises_while_capturing(monkeypatch):
    """The tables are built on the host, which a capture cannot do: an index tensor the losses have not seen raises there
    (as vertex_colors._adjacency does).  The capture state is simulated; nothing is captured."""
    import torch
    import neural_renderer_amd as nr
    v, f = R.inputs('ico1')
    vertices, faces = torch.tensor(v, device='cuda'), torch.tensor(f, device='cuda')
    seen = torch.tensor(f, device='cuda')
    want = nr.laplacian_loss(vertices, seen)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='before the capture'):
        nr.laplacian_loss(vertices, faces)
    from neural_renderer_amd import mesh_losses
    with pytest.raises(RuntimeError, match='not built yet'):
        mesh_losses._tables(faces, 42)
    assert torch.equal(nr.laplacian_loss(vertices, seen), want)      # a known one goes through


def test_example_regularizers_first_steps():
    """examples/example_regularizers.py: example 2's fit with both terms added; a few steps run, every term stays finite
    and the sum goes down."""
    import os
    import sys
    import torch
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import make_data
    make_data.main()
    import example_regularizers
    data = os.path.join(ex, 'data')
    model = example_regularizers.Model(os.path.join(data, 'teapot.obj'), os.path.join(data, 'example2_ref.png'), 30.0, 0.01).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, terms = model()
        loss.backward()
        opt.step()
        assert all(bool(torch.isfinite(t)) for t in terms) and bool(torch.isfinite(model.vertices.grad).all())
        losses.append(float(loss.detach()))
    print('example_regularizers: loss %.2f -> %.2f (silhouette %.2f, laplacian %.4f, flatness %.2f at the end)'
          % (losses[0], losses[-1], float(terms[0]), float(terms[1]), float(terms[2])))
    assert losses[-1] < losses[0]
