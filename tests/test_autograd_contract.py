"""The autograd contract without a GPU (tests/autograd_contract.py; the device's part is tests/test_autograd_contract_gpu.py):
the registry names every torch.autograd.Function of the package, every one of them refuses a second derivative, and the
properties P1, P2, P3, P6 and P7 as behaviour for _WindingTorch, the one custom Function that runs on CPU tensors -- in
float64, the plain call within the bounds of winding_ref.gradients, the variants equal to it bit for bit (the path has no
atomics: index_add_ on the CPU adds in index order)."""
import importlib

import numpy as np
import pytest
import torch

import autograd_contract as AC
import winding_ref as R
from test_winding import case, tensors

import neural_renderer_amd as nr


def test_the_registry_names_every_function_of_the_package():
    """A new torch.autograd.Function without a row (and without its ctx attributes in CTX) fails here."""
    found = AC.package_functions()
    rows = {c for row in AC.ROWS for c in row.classes}
    assert sorted(found) == sorted(rows), sorted(set(found) ^ rows)
    assert sorted(found) == sorted(AC.CTX)
    assert len(found) == 27
    assert len({row.name for row in AC.ROWS}) == len(AC.ROWS)
    on_device = {c for row in AC.GPU_ROWS for c in row.classes}
    assert rows - on_device == {'_GraphedRasterizeFunction', '_WindingTorch'}


def test_every_pinned_test_exists():
    for row in AC.ROWS:
        path, name = row.pinned.split('::')
        module = importlib.import_module(path[len('tests/'):-len('.py')])
        assert callable(getattr(module, name.split('[')[0], None)), row.pinned


@pytest.mark.parametrize('name', sorted(AC.CTX))
def test_backward_is_wrapped_once_differentiable(name):
    """The static form of P7: forward and backward are the wrappers of _util.once_differentiable (functools.wraps leaves the
    undecorated function on __wrapped__)."""
    cls = AC.package_functions()[name]
    assert callable(getattr(cls.backward, '__wrapped__', None)), name
    assert callable(getattr(cls.forward, '__wrapped__', None)), name
    assert cls.backward.__wrapped__.__qualname__ == name + '.backward'


def test_the_decorator_on_a_small_function():
    """A backward that fills a fresh buffer: its gradient taken with create_graph=True would pass for a constant.  Decorated,
    differentiating anything that depends on it raises -- with an upstream gradient that requires none (the plain sum of a
    gradient penalty) and when the input is no leaf -- and the first derivative has the undecorated function's bits."""
    from neural_renderer_amd import _util

    @_util.once_differentiable
    class Square(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k):
            ctx.save_for_backward(x.detach())
            ctx.k = k
            return x.detach() ** 2 * k

        @staticmethod
        def backward(ctx, g):
            out = torch.empty_like(g)
            out.copy_(2 * ctx.k * ctx.saved_tensors[0] * g)
            return out, None
    leaf = torch.arange(1.0, 5.0, dtype=torch.float64, requires_grad=True)
    for x in (leaf, leaf * 1.5):
        y = Square.apply(x, 3.0)
        g, = torch.autograd.grad(y.sum(), x, create_graph=True)
        assert torch.equal(g.detach(), 6 * x.detach()) and g.requires_grad
        for target in (x, leaf):
            with pytest.raises(RuntimeError, match='once_differentiable'):
                torch.autograd.grad(g.sum() + y.sum(), target, retain_graph=True)
        plain, = torch.autograd.grad(y.sum(), x, retain_graph=True)
        assert torch.equal(plain, g.detach()) and not plain.requires_grad
        torch.autograd.grad(y.sum(), leaf)   # the first derivative alone never raises


# ---------------------------------------------------------------------------------------------------------------------
# _WindingTorch on the CPU

K = 1   # test_winding.SHAPES[1]: B = 3, 63 points per image, 255 faces


def _upstream(B, N):
    return np.random.default_rng(1).uniform(-1, 1, (B, N)).astype(np.float32)


def _forward(want=('points', 'vertices')):
    points, vertices, faces = case(K)
    p, v, f = tensors(points, vertices, faces, torch.float64, 'cpu')
    p.requires_grad_('points' in want)
    v.requires_grad_('vertices' in want)
    w = nr.winding_number(p, v, f)
    return p, v, w, torch.tensor(_upstream(*w.shape), dtype=torch.float64)


@pytest.fixture(scope='module')
def plain():
    """(w, grad_points, grad_vertices) of the plain call, within the restatement's bounds."""
    points, vertices, faces = case(K)
    p, v, w, g = _forward()
    assert type(w.grad_fn).__name__ == '_WindingTorchBackward'
    gp, gv = torch.autograd.grad((w * g).sum(), [p, v])
    (rp, bp), (rv, bv) = R.gradients(points, vertices, faces, _upstream(*w.shape), vertices.shape[1], R.U64)
    ratios = R.ratio(gp.numpy(), rp, bp), R.ratio(gv.numpy(), rv, bv)
    print('_WindingTorch float64: grad_points at %.3f, grad_vertices at %.3f of the bound' % ratios)
    assert max(ratios) <= 1 and np.abs(rp).sum() > 0 and np.abs(rv).sum() > 0
    assert not torch.equal(g[0], g[1])
    return w.detach(), gp, gv


def test_winding_torch_p1_repeat(plain):
    p, v, w, g = _forward()
    loss = (w * g).sum()
    node = w.grad_fn
    watch = list(node.saved_tensors) + [p, v, w]
    for _ in range(2):
        before = [AC.bits(x) for x in watch]
        gp, gv = torch.autograd.grad(loss, [p, v], retain_graph=True)
        assert all(torch.equal(AC.bits(x), b) for x, b in zip(watch, before))
        assert torch.equal(gp, plain[1]) and torch.equal(gv, plain[2])


def test_winding_torch_p2_accumulate(plain):
    p, v, w, g = _forward()
    loss = (w * g).sum()
    loss.backward(retain_graph=True)
    first = p.grad.clone(), v.grad.clone()
    loss.backward(retain_graph=True)
    assert torch.equal(first[0], plain[1]) and torch.equal(first[1], plain[2])
    assert torch.equal(p.grad, 2 * first[0]) and torch.equal(v.grad, 2 * first[1])


@pytest.mark.parametrize('want', [('points',), ('vertices',)])
def test_winding_torch_p3_input_subsets(plain, want):
    p, v, w, g = _forward(want)
    assert torch.equal(w.detach(), plain[0])
    (w * g).sum().backward()
    for x, name, ref in ((p, 'points', plain[1]), (v, 'vertices', plain[2])):
        assert (torch.equal(x.grad, ref) if name in want else x.grad is None), name


def test_winding_torch_p3_no_input(plain):
    p, v, w, g = _forward(())
    assert not w.requires_grad and torch.equal(w, plain[0])


def test_winding_torch_p6_batch_isolation(plain):
    p, v, w, g = _forward()
    g[1] = 0
    gp, gv = torch.autograd.grad((w * g).sum(), [p, v])
    for got, ref in ((gp, plain[1]), (gv, plain[2])):
        assert bool(torch.isfinite(got).all()) and not bool(got[1].any()) and bool(ref[1].any())
        assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])


def test_winding_torch_p7_second_derivative_raises():
    p, v, w, g = _forward()
    gp, = torch.autograd.grad((w * g).sum(), p, create_graph=True)
    assert gp.requires_grad
    with pytest.raises(RuntimeError, match='once_differentiable'):
        torch.autograd.grad(gp.sum() + w.sum(), p)
