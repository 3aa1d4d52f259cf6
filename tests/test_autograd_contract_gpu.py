"""`-m gpu`: the autograd contract of every HIP-backed torch.autograd.Function, over the rows of tests/autograd_contract.py
(its docstring: what a row is, and where the plain call of every row is held to its restatement).

  P1 repeat            torch.autograd.grad twice over one retained graph: the same result by the row's kind, the plain call's
                       too, and no saved tensor, ctx attribute, input or output has another bit after a backward
  P2 accumulate        .backward(retain_graph=True) twice on leaves: .grad is 2 g.  Rasterize.grad_faces (rasterizer rows)
  P3 input subsets     every input alone and all but one: the chosen gradients are the full call's, the outputs its bits
  P4 output subsets    every subset of outputs receiving a gradient against explicit zeros for the others
  P5 interleave        two forwards on the same leaf, instance, index tensor, layout and caches, then backward
  P6 batch isolation   image 1's upstream gradient exact zeros: its rows exact zeros, the other images' unchanged
  P7 second derivative raises

Comparisons are Case.compare's of tests/test_layout_invariance_gpu.py by the gradient's kind (bits | order | close; integer
upstream gradients where float atomics add) -- nothing here has a tolerance of its own.  Every test prints its row's kinds and
the worst `order` / `close` value it saw.  Nothing here captures a graph or switches graph replay on:
_GraphedRasterizeFunction is documented to raise when a second forward comes before the backward ("a later forward of the
same shapes has replaced the residual maps") and is held by tests/test_hip_parity.py."""
import itertools

import pytest
import torch

import autograd_contract as AC
from autograd_contract import GPU_ROWS
from test_layout_invariance_gpu import _cuda

pytestmark = pytest.mark.gpu

rows = pytest.mark.parametrize('row', GPU_ROWS, ids=[r.name for r in GPU_ROWS])
# the rows whose call has more than one differentiable output
MULTI = [r for r in GPU_ROWS if r.raster or r.name.startswith(('rgbad', 'frontend')) or r.name == 'point_mesh_both']

_FULL = {}


def full(row):
    """The plain call of the row, once: ((outputs, gradients), the upstream gradients by output)."""
    if row.name not in _FULL:
        case = row.case()
        ref = AC.gradients(case)
        case.nontrivial(ref, row.name)
        assert all(int(o.shape[0]) >= 2 for o in ref[0].values() if torch.is_tensor(o) and o.is_floating_point())
        for w in case.upstream.values():   # upstream gradients that differ per image
            assert not torch.equal(w[0], w[1])
        _FULL[row.name] = (ref, dict(case.upstream))
    return _FULL[row.name]


def fresh(row, inputs=None):
    """(a Case of the row with the plain call's upstream gradients, the plain call's results)"""
    ref, upstream = full(row)
    case = row.case(inputs)
    case.upstream = dict(upstream)
    return case, ref


class _Same(object):
    """In place of a class: every construction gives the one instance (the calls of the cases build theirs inside)."""

    def __init__(self, cls):
        self.cls, self.obj, self.calls = cls, None, 0

    def __call__(self, *args, **kw):
        self.calls += 1
        if self.obj is None:
            self.obj = self.cls(*args, **kw)
        return self.obj


def share_instances(monkeypatch):
    import neural_renderer_amd as nr
    shared = {name: _Same(getattr(nr, name)) for name in ('Rasterize', 'Renderer')}
    for name, s in shared.items():
        monkeypatch.setattr(nr, name, s)
    return shared


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('row', [r for r in GPU_ROWS if r.check], ids=[r.name for r in GPU_ROWS if r.check])
def test_full_call_within_its_family_s_check(row):
    """Rows whose exact case no existing test holds: the family's own check function on the row's arrays."""
    row.check()


@rows
def test_p1_repeat(row):
    case, ref = fresh(row)
    t = AC.leaves_of(case)
    outs = AC.forward(case, t)
    loss = AC.loss_of(case, outs)
    names = [n for n in AC.names_of(t) if n in ref[1]]
    AC.same_outputs({k: (o.detach() if torch.is_tensor(o) else o) for k, o in outs.items()}, ref[0], row.name)
    nodes = {type(n).__name__[:-len('Backward')] for n in AC.package_nodes([o for _, o in AC.diff_outputs(outs)])}
    assert set(row.classes) <= nodes, (row.classes, nodes)
    watch = AC.residuals(row, [o for _, o in AC.diff_outputs(outs)])
    assert watch or not row.ctx
    watch += [('input ' + n, x) for n, x in t.items()] + [('output ' + k, o) for k, o in outs.items() if torch.is_tensor(o)]
    results = []
    for call in range(2):
        before = [AC.bits(x) for _, x in watch]
        results.append(torch.autograd.grad(loss, [t[n] for n in names], retain_graph=True))
        for (what, x), b in zip(watch, before):
            assert torch.equal(AC.bits(x), b), '%s: backward %d changed %s' % (row.name, call, what)
    for n, first, second in zip(names, *results):
        AC.same(case, n, second, first, '%s: the second backward over the retained graph' % row.name)
        AC.same(case, n, first, ref[1][n], '%s: the first backward against the plain call' % row.name)
    AC.report(case, 'P1 %s (%d residual tensors on %s)' % (row.name, len(watch) - len(t) - len(outs), sorted(nodes)))


@rows
def test_p2_accumulate(row, monkeypatch):
    """Rasterize.grad_faces holds what the last backward RETURNED, as an alias: after the first call AccumulateGrad has adopted
    that buffer as faces.grad, so both are one storage; the second call accumulates into that storage in place (an alias kept
    from the first call shows 2 g with it) and leaves its own result, g, on the instance in a buffer of its own."""
    shared = share_instances(monkeypatch)
    case, ref = fresh(row)
    t = AC.leaves_of(case)
    outs = AC.forward(case, t)
    loss = AC.loss_of(case, outs)
    names = [n for n in AC.names_of(t) if n in ref[1]]
    loss.backward(retain_graph=True)
    g = {n: t[n].grad.clone() for n in names}
    if row.raster:
        fn = shared['Rasterize'].obj
        first = fn.grad_faces
        assert first.data_ptr() == t['faces'].grad.data_ptr(), 'AccumulateGrad cloned the returned grad_faces'
        assert torch.equal(first, g['faces'])
    loss.backward(retain_graph=True)
    for n in names:
        AC.same(case, n, t[n].grad, 2 * g[n], '%s: .grad after two backward calls against twice the first' % row.name)
        AC.same(case, n, g[n], ref[1][n], '%s: .grad after one backward call against the plain call' % row.name)
    if row.raster:
        last = fn.grad_faces
        assert last.data_ptr() != t['faces'].grad.data_ptr()
        AC.same(case, 'faces', last, g['faces'], '%s: Rasterize.grad_faces after the second call: the returned gradient' % row.name)
        assert torch.equal(first, t['faces'].grad), 'the alias of the first call: the accumulated gradient'
    AC.report(case, 'P2 %s' % row.name)


@rows
def test_p3_input_subsets(row):
    case, ref = fresh(row)
    names = sorted(ref[1])
    subsets = [(n,) for n in names] + ([tuple(m for m in names if m != n) for n in names] if len(names) > 2 else [])
    for chosen in subsets:
        t = AC.leaves_of(case, chosen)
        outs = AC.forward(case, t)
        what = '%s: only %s ask for a gradient' % (row.name, ', '.join(chosen))
        AC.same_outputs({k: (o.detach() if torch.is_tensor(o) else o) for k, o in outs.items()}, ref[0], what)
        AC.loss_of(case, outs).backward()
        for n, x in t.items():
            if n in chosen:
                AC.same(case, n, x.grad, ref[1][n], what)
            else:
                assert x.grad is None, (what, n)
    t = AC.leaves_of(case, ())
    outs = AC.forward(case, t)
    assert not any(torch.is_tensor(o) and o.requires_grad for o in outs.values()), row.name
    AC.same_outputs(outs, ref[0], '%s: no input asks for a gradient' % row.name)
    AC.report(case, 'P3 %s (%d subsets)' % (row.name, len(subsets)))


@pytest.mark.parametrize('row', MULTI, ids=[r.name for r in MULTI])
def test_p4_output_subsets(row):
    case, ref = fresh(row)
    keys = sorted(case.upstream)
    assert len(keys) > 1
    count = 0
    for r in range(1, len(keys)):
        for only in itertools.combinations(keys, r):
            what = '%s: only %s receive a gradient' % (row.name, ', '.join(only))
            skipped = AC.gradients(case, only=only)
            zeros = AC.gradients(case, only=only, explicit_zeros=True)
            AC.same_outputs(skipped[0], ref[0], what)
            assert sorted(zeros[1]) == sorted(ref[1]) and any(float(g.abs().sum()) > 0 for g in skipped[1].values()), what
            for n, g in zeros[1].items():
                assert bool(torch.isfinite(g).all()), (what, n)
                if n in skipped[1]:
                    AC.same(case, n, skipped[1][n], g, what)
                else:   # no path from these outputs to the input: the explicit zeros give exact zeros
                    assert not bool(g.any()), (what, n)
            count += 1
    AC.report(case, 'P4 %s (%d subsets)' % (row.name, count))


@rows
def test_p5_interleave(row, monkeypatch):
    case, ref = fresh(row)
    vary = row.vary[0] if row.vary else None

    def pair(case):
        """The leaves of the two forwards: one object per input, but for the input in which they differ."""
        ta = AC.leaves_of(case)
        tb = dict(ta)
        if vary:
            tb[vary] = _cuda(row.vary[1](case.inputs[vary]), ta[vary].requires_grad)
            assert not torch.equal(tb[vary], ta[vary])
        return ta, tb

    def separate(second):
        t = pair(case)[second]
        outs = AC.forward(case, t)
        names = [n for n in AC.names_of(t) if n in ref[1]]
        grads = torch.autograd.grad(AC.loss_of(case, outs, second=bool(second)), [t[n] for n in names], allow_unused=True)
        return {k: (o.detach() if torch.is_tensor(o) else o) for k, o in outs.items()}, dict(zip(names, grads))
    (outs_a, ga), (outs_b, gb) = separate(0), separate(1)
    for n in ga:
        AC.same(case, n, ga[n], ref[1][n], '%s: the first forward alone is the plain call' % row.name)
    want = {n: (ga[n] if n == vary else ga[n] + gb[n]) for n in ga}
    if vary in ga:
        want[vary + ' of the second forward'] = gb[vary]

    shared = share_instances(monkeypatch)
    # (a case of its own: the first backward over its UVLayout -- the one that builds the inverse map -- comes after two forwards)
    joint = fresh(row)[0]
    for order in ('L1 + L2', 'L2 then L1'):
        ta, tb = pair(joint)
        fa, fb = AC.forward(joint, ta), AC.forward(joint, tb)   # both forwards before any backward
        for got, alone in ((fa, outs_a), (fb, outs_b)):
            AC.same_outputs({k: (o.detach() if torch.is_tensor(o) else o) for k, o in got.items()}, alone, row.name)
        la, lb = AC.loss_of(joint, fa), AC.loss_of(joint, fb, second=True)
        leaves = {n: ta[n] for n in ga}
        if vary in ga:
            leaves[vary + ' of the second forward'] = tb[vary]
        if order == 'L1 + L2':
            got = dict(zip(leaves, torch.autograd.grad(la + lb, list(leaves.values()))))
        else:
            lb.backward(retain_graph=True)
            la.backward(retain_graph=True)
            got = {n: x.grad for n, x in leaves.items()}
        for n, g in got.items():
            kind_of = vary if n.endswith(' of the second forward') else n
            AC.same(case, kind_of, g, want[n], '%s: %s after two forwards, gradient of %s' % (row.name, order, n))
    assert all(s.calls in (0, 4) for s in shared.values()), [(s.cls, s.calls) for s in shared.values()]
    AC.report(case, 'P5 %s (the forwards differ in %s)' % (row.name, vary or 'their upstream gradients'))


@rows
def test_p6_batch_isolation(row):
    case, ref = fresh(row)
    B = int(next(iter(case.upstream.values())).shape[0])
    keep = [b for b in range(B) if b != 1]
    outs, grads = AC.gradients(case, zero_image=1)
    AC.same_outputs(outs, ref[0], row.name)
    assert sorted(grads) == sorted(ref[1])
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()), (row.name, n)
        if n in row.shared:
            continue
        assert int(g.shape[0]) == B, (row.name, n)
        assert not bool(g[1].any()), '%s: image 1 of the gradient of %s is not exact zeros' % (row.name, n)
        AC.same(case, n, g[keep], ref[1][n][keep], '%s: the other images with image 1 zeroed' % row.name)
    batchless = [n for n in grads if n in row.shared]
    if batchless:   # one gradient for the batch: the call on the batch without image 1
        small = row.case({n: (a if n in row.shared else a[keep]) for n, a in case.inputs.items()})
        small.upstream = {k: w[keep].contiguous() for k, w in case.upstream.items()}
        alone = AC.gradients(small)[1]
        for n in batchless:
            AC.same(case, n, grads[n], alone[n], '%s: image 1 zeroed against the batch without it' % row.name)
    AC.report(case, 'P6 %s (B = %d%s)' % (row.name, B, ', shared: ' + ', '.join(batchless) if batchless else ''))


@rows
def test_p7_second_derivative_raises(row):
    case, ref = fresh(row)
    t = AC.leaves_of(case)
    outs = AC.forward(case, t)
    xs = [t[n] for n in AC.names_of(t) if n in ref[1]]
    g = torch.autograd.grad(AC.loss_of(case, outs), xs, create_graph=True)
    assert all(x.requires_grad for x in g), 'a gradient taken with create_graph=True passes for a constant'
    second = sum(x.sum() for x in g) + sum(o.sum() for _, o in AC.diff_outputs(outs))
    with pytest.raises(RuntimeError, match='once_differentiable'):
        torch.autograd.grad(second, xs, allow_unused=True)
