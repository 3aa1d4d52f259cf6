"""The edge-length and the cotangent Laplacian loss on the GPU (include/nr_hip.h nr_edge_length_forward / _backward,
nr_cot_weights, nr_cot_apply; neural_renderer_amd/mesh_losses.py): both losses and both gradients entry by entry against the
float64 restatement of tests/mesh_edge_ref.py within the constants of tests/test_mesh_edge_losses.py, every target form,
bit-for-bit repetition, the batch against its slices, dispatch, launch counts, layouts and streams, graph capture and the
example."""
import numpy as np
import pytest

import mesh_edge_ref as E
import mesh_loss_ref as R
from test_mesh_edge_losses import call, constants, forms_of, loss_and_grad, ratios

pytestmark = pytest.mark.gpu


def _fn(kind):
    import neural_renderer_amd as nr
    return nr.edge_length_loss if kind == 'edge' else nr.cotangent_laplacian_loss


def _f32():
    import torch
    return torch.float32


def _hip(kind, name, seed, form, **kw):
    kw.setdefault('implementation', 'hip')
    return loss_and_grad(_fn(kind), kind, name, seed, form, _f32(), device='cuda', **kw)


def _check(kind, name, seed, form):
    loss, grad = _hip(kind, name, seed, form)
    rl, rg = ratios(kind, name, seed, form, loss, grad)
    C = constants(name)
    print('%s %s seed %d target %s: loss at %.3f of u M (C = %d), gradient at %.3f (C = %d)'
          % (kind, name, seed, form, rl, C[kind, 'loss'], rg, C[kind, 'grad']))
    assert rl <= C[kind, 'loss'] and rg <= C[kind, 'grad']
    return loss, grad


@pytest.mark.parametrize('name', R.MESHES + R.ODD + R.DEGENERATE)
@pytest.mark.parametrize('kind', E.KINDS)
def test_against_the_float64_restatement(kind, name):
    """Every mesh, B = 3, every seed of the noisy ones; the edge loss without a target (no square root) and with a [B,E] one.
    'odd': an isolated vertex (gradient exactly 0: its magnitude is 0), a duplicated face, a face with a repeated index, an
    edge in three faces.  'blocks': 648 vertices, three blocks of 256 per image, the last one partly filled: the block-order
    reduction.  'degenerate': a zero-length edge and a face without area, finite.  Measured on the MI355X: see the lines
    this test prints (LAB-NOTEBOOK.md "Mesh losses: edge length and cotangent Laplacian" keeps the worst of a run)."""
    for seed in R.seeds_of(name):
        for form in (('zero', 'BE') if kind == 'edge' else ('zero',)):
            loss, grad = _check(kind, name, seed, form)
            if name == 'odd':
                assert not grad[:, 42].any()
            if name == 'degenerate':
                assert np.isfinite(loss).all() and np.isfinite(grad).all()


@pytest.mark.parametrize('form', E.TARGETS)
@pytest.mark.parametrize('name', ['ico1', 'blocks'])
def test_every_target_form(name, form):
    import torch
    loss, grad = _check('edge', name, 1, form)
    # ... and the torch path on the device within 2 C of the same magnitudes (each within C of the restatement)
    ref = E.reference('edge', name, 1, form)
    tor = _hip('edge', name, 1, form, implementation='torch')
    C = constants(name)
    assert R.worst_ratio(loss, tor[0], ref.loss_mag) <= 2 * C['edge', 'loss']
    assert R.worst_ratio(grad, tor[1], ref.grad_mag) <= 2 * C['edge', 'grad']
    if form == 'E':   # a float64 target tensor is read as float32: the same bits
        v, f = R.inputs(name, 1)
        x = torch.tensor(v, device='cuda')
        t = torch.tensor(E.target(name, 1, 'E'), device='cuda')
        a = _fn('edge')(x, torch.tensor(f, device='cuda'), target=t.double(), implementation='hip')
        assert np.array_equal(a.cpu().numpy(), loss)


def test_rest_lengths_and_a_zero_length_edge_on_the_kernels():
    """A zero-length edge with a positive target: t^2 in the loss, exactly nothing in the gradient (the numbers of
    tests/test_mesh_edge_losses.py, all exact in float32)."""
    import torch
    faces = torch.tensor([[0, 1, 2]], device='cuda')
    x = torch.tensor([[0.5, 0.25, 0.0], [0.5, 0.25, 0.0], [1.5, 0.25, 0.0]], device='cuda', requires_grad=True)
    loss = _fn('edge')(x, faces, target=torch.tensor([0.75, 1.0, 1.0], device='cuda'), implementation='hip')
    grad, = torch.autograd.grad(loss, x)
    assert float(loss.detach()) == 0.75 ** 2 and not grad.any()
    loss = _fn('edge')(x, faces, target=0.75, implementation='hip')
    grad, = torch.autograd.grad(loss, x)
    assert float(loss.detach()) == 0.75 ** 2 + 2 * 0.25 ** 2
    assert torch.equal(grad.cpu(), torch.tensor([[-0.5, 0, 0], [-0.5, 0, 0], [1.0, 0, 0]]))
    # no edge at all: an exact 0 and exact zeros
    none = _fn('edge')(x, torch.tensor([[2, 2, 2]], device='cuda'), target=0.5, implementation='hip')
    grad, = torch.autograd.grad(none, x)
    assert float(none.detach()) == 0 and not grad.any()


@pytest.mark.parametrize('kind', E.KINDS)
def test_two_runs_and_batch_slices_give_the_same_bits(kind):
    import torch
    form = 'BE'
    a = _hip(kind, 'blocks', 1, form)
    b = _hip(kind, 'blocks', 1, form)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    v, f = R.inputs('blocks', 1)
    faces = torch.tensor(f, device='cuda')
    for k in range(v.shape[0]):   # every image alone: the same bits as inside the batch
        x = torch.tensor(v[k:k + 1], device='cuda', requires_grad=True)
        kw = {'target': torch.tensor(E.target('blocks', 1, 'BE')[k:k + 1], device='cuda')} if kind == 'edge' else {}
        loss = _fn(kind)(x, faces, implementation='hip', **kw)
        grad, = torch.autograd.grad(loss[0] * float(R.UPSTREAM[k]), x)
        assert np.array_equal(loss.detach().cpu().numpy(), a[0][k:k + 1])
        assert np.array_equal(grad.cpu().numpy(), a[1][k:k + 1])


@pytest.mark.parametrize('kind', E.KINDS)
def test_default_dispatch(kind):
    """None picks the kernels on float32 CUDA tensors; float64 on the device takes the torch path, as does a target that
    requires a gradient; the torch path agrees within 2 C."""
    import torch
    for name in ('ico2', 'odd'):
        for form in forms_of(kind)[-1:]:
            ref = E.reference(kind, name, 2, form)
            hip = _hip(kind, name, 2, form)
            default = _hip(kind, name, 2, form, implementation=None)
            assert np.array_equal(default[0], hip[0]) and np.array_equal(default[1], hip[1])
            tor = _hip(kind, name, 2, form, implementation='torch')
            C = constants(name)
            assert R.worst_ratio(hip[0], tor[0], ref.loss_mag) <= 2 * C[kind, 'loss']
            assert R.worst_ratio(hip[1], tor[1], ref.grad_mag) <= 2 * C[kind, 'grad']
            l64, g64 = loss_and_grad(_fn(kind), kind, name, 2, form, torch.float64, device='cuda')
            assert l64.dtype == np.float64
            assert np.abs(l64 - ref.loss).max() <= 1e-12 * np.abs(ref.loss).max()
            assert np.abs(g64 - ref.grad).max() <= 1e-12 * np.abs(ref.grad).max()
    if kind == 'edge':
        v, f = R.inputs('ico1')
        x, faces = torch.tensor(v, device='cuda'), torch.tensor(f, device='cuda')
        t = torch.tensor(E.target('ico1', 0, 'E'), device='cuda', requires_grad=True)
        _fn(kind)(x, faces, target=t).sum().backward()
        assert t.grad is not None and t.grad.abs().sum() > 0
        with pytest.raises(ValueError, match='requires no gradient'):
            _fn(kind)(x, faces, target=t, implementation='hip')


@pytest.mark.parametrize('kind', E.KINDS)
def test_launch_counts(kind):
    """ctx.needs_input_grad: with vertices that require no gradient the loss is a constant of the graph, nothing is kept and a
    backward through what it is combined with calls no entry; with one, exactly one backward entry is called (the cotangent
    loss's is nr_cot_apply a second time)."""
    import torch
    from neural_renderer_amd import _lib
    lib = _lib.load()
    names = ('nr_edge_length_forward', 'nr_edge_length_backward', 'nr_cot_weights', 'nr_cot_apply')
    forward = ['nr_edge_length_forward'] if kind == 'edge' else ['nr_cot_weights', 'nr_cot_apply']
    backward = ['nr_edge_length_backward'] if kind == 'edge' else ['nr_cot_apply']
    real = {n: getattr(lib, n) for n in names}
    calls = []

    def counting(n):
        def fn(*args):
            calls.append(n)
            return real[n](*args)
        return fn
    v, f = R.inputs('ico1')
    faces = torch.tensor(f, device='cuda')
    kw = {'target': 0.3} if kind == 'edge' else {}
    try:
        for n in names:
            setattr(lib, n, counting(n))
        scale = torch.ones(3, device='cuda', requires_grad=True)
        loss = _fn(kind)(torch.tensor(v, device='cuda'), faces, implementation='hip', **kw)
        assert not loss.requires_grad and calls == forward
        (loss * scale).sum().backward()
        assert torch.equal(scale.grad, loss) and calls == forward
        del calls[:]
        x = torch.tensor(v, device='cuda', requires_grad=True)
        out = _fn(kind)(x, faces, implementation='hip', **kw)
        assert calls == forward
        (out * scale).sum().backward()
        assert calls == forward + backward
    finally:
        for n in names:
            setattr(lib, n, real[n])


@pytest.mark.parametrize('kind', E.KINDS)
def test_layout_and_stream(kind):
    """A non-contiguous vertices tensor, an expanded batch view, a vertices tensor off the 16-byte grid and a non-default stream
    give the bits of the plain call."""
    import torch
    name, seed, form = 'blocks', 2, 'BE'
    v, f = R.inputs(name, seed)
    faces = torch.tensor(f, device='cuda')
    g = torch.tensor(R.UPSTREAM, dtype=torch.float32, device='cuda')

    def run(x, **kw):
        """x: a leaf or a view of one -> (loss, gradient with respect to x)"""
        loss = call(_fn(kind), kind, x, faces, name, seed, form, implementation='hip', **kw)
        grad, = torch.autograd.grad((loss * g[:loss.shape[0]]).sum(), x)
        return loss.detach().clone(), grad.clone()
    plain = run(torch.tensor(v, device='cuda', requires_grad=True))
    wide = torch.zeros((3, v.shape[1], 5), device='cuda')
    wide[:, :, 1:4] = torch.tensor(v, device='cuda')
    x = wide[:, :, 1:4].requires_grad_(True)                                # non-contiguous
    assert not x.is_contiguous()
    got = run(x)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    flat = torch.zeros((v.size + 1,), device='cuda')
    flat[1:] = torch.tensor(v, device='cuda').reshape(-1)
    x = flat[1:].reshape(v.shape).requires_grad_(True)                      # contiguous, 4 bytes off the 16-byte grid
    assert x.data_ptr() % 16 == 4
    got = run(x)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = run(torch.tensor(v, device='cuda', requires_grad=True))
    stream.synchronize()
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # an expanded batch view: every image is image 1, and equals it alone
    one = torch.tensor(v[1], device='cuda', requires_grad=True)
    t = torch.tensor(E.target(name, seed, 'E'), device='cuda')
    kw = {'target': t} if kind == 'edge' else {}
    alone = _fn(kind)(one, faces, implementation='hip', **kw)
    grad_alone, = torch.autograd.grad(alone, one)
    batch = _fn(kind)(one.detach()[None].expand(3, -1, -1), faces, implementation='hip', **kw)
    assert torch.equal(batch, alone.detach().expand(3))
    if kind == 'edge':   # ... and an expanded target [B,E]
        again = _fn(kind)(one, faces, implementation='hip', target=t[None].expand(1, -1))
        assert torch.equal(again, alone)
    assert bool(torch.isfinite(grad_alone).all())


def test_graph_capture_equals_eager():
    """A step -- both losses, the edge loss with rest lengths, and their gradients -- captured with
    neural_renderer_amd.graph.capture replays equal to eager.  The tables are built on the host: the only eager calls before the
    capture are under no_grad, with the same index tensor."""
    import torch
    import neural_renderer_amd as nr
    v, f = R.inputs('blocks', 3)
    vertices = torch.tensor(v, device='cuda', requires_grad=True)
    faces = torch.tensor(f, device='cuda')
    rest = torch.tensor(E.target('blocks', 3, 'E'), device='cuda')
    out = torch.zeros((3, 3), device='cuda')
    w = torch.tensor(R.UPSTREAM, dtype=torch.float32, device='cuda')

    def step():
        edge, rigid = nr.edge_length_loss(vertices, faces), nr.edge_length_loss(vertices, faces, target=rest)
        cot = nr.cotangent_laplacian_loss(vertices, faces)
        out[0].copy_(edge)
        out[1].copy_(rigid)
        out[2].copy_(cot)
        return torch.autograd.grad(((edge + 0.5 * rigid + 0.25 * cot) * w).sum(), [vertices])
    with torch.no_grad():
        nr.edge_length_loss(vertices, faces)             # builds the tables (and checks the indices) eagerly
        nr.cotangent_laplacian_loss(vertices, faces)
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
    assert bool((got_out > 0).all())


def test_unknown_topology_raises_while_capturing(monkeypatch):
    """The tables are built on the host, which a capture cannot do: an index tensor the losses have not seen raises there.
    The capture state is simulated; nothing is captured."""
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import mesh_losses, vertex_colors
    v, f = R.inputs('ico1')
    vertices, faces = torch.tensor(v, device='cuda'), torch.tensor(f, device='cuda')
    seen = torch.tensor(f, device='cuda')
    want = nr.edge_length_loss(vertices, seen, target=0.3), nr.cotangent_laplacian_loss(vertices, seen)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    for fn in (nr.edge_length_loss, nr.cotangent_laplacian_loss):
        with pytest.raises(RuntimeError, match='before the capture'):
            fn(vertices, faces)
    with pytest.raises(RuntimeError, match='not built yet'):
        mesh_losses._edge_tables(faces, 42)
    with pytest.raises(RuntimeError, match='not built yet'):
        vertex_colors._adjacency(faces, 42)
    assert torch.equal(nr.edge_length_loss(vertices, seen, target=0.3), want[0])      # a known one goes through
    assert torch.equal(nr.cotangent_laplacian_loss(vertices, seen), want[1])


def test_example_edge_regularizers_first_steps():
    """examples/example_edge_regularizers.py: a few steps of its fit run, every term stays finite and the total goes down."""
    import os
    import sys
    import torch
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import example_edge_regularizers as example
    terms_seen = []
    target = example.target_cloud(512, torch.device('cuda'))
    vertices, faces, losses = example.fit(target, 20, level=2, on_step=lambda i, loss, terms: terms_seen.append(terms))
    assert len(losses) == 20 and all(np.isfinite(t).all() for t in terms_seen) and np.isfinite(losses).all()
    assert bool(torch.isfinite(vertices).all())
    print('example_edge_regularizers: loss %.5f -> %.5f, longest / shortest edge %.3f'
          % (losses[0], losses[-1], example.edge_ratio(vertices, faces)))
    assert losses[-1] < losses[0]
