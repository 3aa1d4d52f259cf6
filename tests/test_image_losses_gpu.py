"""Image losses on the GPU (include/nr_hip.h nr_iou_loss_forward / _backward, nr_squared_error_forward / _backward;
neural_renderer_amd/image_losses.py): both losses and both gradients entry by entry against the float64 restatement of
tests/image_loss_ref.py within the constants of tests/test_image_losses.py, bit-for-bit repetition, the batch against its
slices, the torch path, views, the backward's launches, graph capture and the example's first steps."""
import numpy as np
import pytest

import image_loss_ref as R
from test_image_losses import CONSTANTS, KINDS, ratios

pytestmark = pytest.mark.gpu


def _f32():
    import torch
    return torch.float32


def _run(kind, case, **kw):
    """(loss, grad) of the public function on the device (implementation = 'hip' unless said otherwise)"""
    _, _, run, _, fn = KINDS[kind]
    kw.setdefault('implementation', 'hip')
    return run(fn, case, kw.pop('dtype', _f32()), device='cuda', **kw)


def _check(kind, case):
    loss, grad = _run(kind, case)
    rl, rg = ratios(kind, case, loss, grad)
    print('%s %s: loss at %.3f of u M (C = %d), gradient at %.3f (C = %d)'
          % (kind, case, rl, CONSTANTS[kind, 'loss'], rg, CONSTANTS[kind, 'grad']))
    assert loss.dtype == np.float32 and grad.dtype == np.float32
    assert rl <= CONSTANTS[kind, 'loss'] and rg <= CONSTANTS[kind, 'grad'], case
    return rl, rg


@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_against_the_float64_restatement(kind):
    """Every case of R.iou_cases() / R.se_cases(), none left out: B = 3 at 24 x 40 for 1 .. 4 levels and at 32 x 48 for 5 (not
    square, no multiple of the 64 x 16 tile, rows that end the 16-byte path before the tile does), 40 x 72, the widths 38
    and 37 that take the scalar path, binary and soft targets, shared and per image, C in {1, 3, 4} and [B,H,W] images, the
    mask absent, shared and per image, and B = 1."""
    cases = KINDS[kind][0]()
    worst = [max(rs) for rs in zip(*[_check(kind, case) for case in cases])]
    print('%s: %d cases, worst ratio loss %.3f, gradient %.3f' % (kind, len(cases), worst[0], worst[1]))


@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_several_workgroups_per_image(kind):
    """40 x 72 with the kernels' tiles of 64 x 16 pixels (one workgroup each, row-major): 2 x 3 = 6 workgroups per image, the
    right column 8 pixels wide, the last row of tiles 8 pixels high and the last workgroup an 8 x 8 corner -- the tile-order
    reduction over more than three partials with partly filled workgroups.  The sums of the last tile must be in the loss: an
    input that is zero outside that corner gives the restatement's loss there too."""
    import torch
    import neural_renderer_amd as nr
    H, W, levels = R.BIG
    assert (H // 16 + 1) * (W // 64 + 1) == 6 and H % 16 == 8 and W % 64 == 8
    for case in KINDS[kind][0]():
        if case[:3] == R.BIG:
            _check(kind, case)
    w = R.WEIGHTS[:levels]
    a = np.zeros((1, H, W), np.float32)
    a[:, 32:, 64:] = 0.75
    t = np.zeros((H, W), np.float32)
    t[34:, 66:] = 1
    x, y = torch.tensor(a, device='cuda'), torch.tensor(t, device='cuda')
    got = nr.silhouette_iou_loss(x, y, levels=levels, level_weights=w, implementation='hip').cpu().numpy()
    ref = R.iou_ref(a, t, w, g=(1.0,))
    assert R.worst_ratio(got, ref.loss, ref.loss_mag) <= CONSTANTS['iou', 'loss'] and (ref.loss < sum(w) - 0.5).all()
    got = nr.squared_error_loss(x, y, levels=levels, level_weights=w, implementation='hip').cpu().numpy()
    ref = R.se_ref(a, t, None, w, g=(1.0,))
    assert R.worst_ratio(got, ref.loss, ref.loss_mag) <= CONSTANTS['se', 'loss'] and (ref.loss > 1).all()


def test_exact_limits_on_the_kernels():
    import torch
    import neural_renderer_amd as nr
    w = (1.0, 0.5, 0.25, 2.0)
    a = torch.zeros((2, 16, 24), device='cuda', requires_grad=True)
    loss = nr.silhouette_iou_loss(a, torch.zeros((16, 24), device='cuda'), levels=4, level_weights=w, implementation='hip')
    assert loss.shape == (2,) and loss.dtype == torch.float32 and bool((loss == sum(w)).all())
    grad, = torch.autograd.grad(loss.sum(), a)
    assert not grad.any()
    t = torch.zeros((16, 24), device='cuda')
    t[8:16, 8:24] = 1
    loss = nr.silhouette_iou_loss(t[None].clone(), t, levels=4, level_weights=w, eps=1e-6, implementation='hip')
    want = sum(wl * 1e-6 / (128.0 / 4 ** l + 1e-6) for l, wl in enumerate(w))
    assert abs(float(loss[0]) - want) <= 2.0 ** -24 * want       # evaluated in double, rounded once
    x = torch.rand((2, 3, 16, 24), device='cuda')
    assert not nr.squared_error_loss(x, x.clone(), levels=3, implementation='hip').any()


# ---------------------------------------------------------------------------------------------------------------------
# the same bits

def _slice_case(kind, case, k):
    """the inputs of image k alone, as device tensors: (image (leaf), the other arguments, weights)"""
    import torch
    inputs = (R.iou_inputs if kind == 'iou' else R.se_inputs)(case)
    weights = inputs[-1]
    shared = case[4]
    dev = lambda a: None if a is None else torch.tensor(a, device='cuda')
    image = torch.tensor(inputs[0][k:k + 1], device='cuda', requires_grad=True)
    target = dev(inputs[1] if shared else inputs[1][k:k + 1])
    if kind == 'iou':
        return image, (target,), weights
    mask = inputs[2]
    if mask is not None and mask.ndim == 3:
        mask = mask[k:k + 1]
    return image, (target, dev(mask)), weights


@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_two_runs_and_batch_slices_give_the_same_bits(kind):
    import torch
    fn = KINDS[kind][4]
    picked = [c for c in KINDS[kind][0]() if c[:3] in (R.BIG, (32, 48, 5), (18, 38, 2)) and c[-1] == R.B]
    assert len(picked) >= 12
    for case in picked:
        first, second = _run(kind, case), _run(kind, case)
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]), case
        for k in range(R.B):   # every image alone: the same bits as inside the batch
            image, others, weights = _slice_case(kind, case, k)
            kw = dict(eps=R.EPS) if kind == 'iou' else {}
            loss = fn(image, *others, levels=len(weights), level_weights=weights, implementation='hip', **kw)
            grad, = torch.autograd.grad(loss[0] * float(R.UPSTREAM[k]), image)
            assert np.array_equal(loss.detach().cpu().numpy(), first[0][k:k + 1]), (case, k)
            assert np.array_equal(grad.cpu().numpy(), first[1][k:k + 1]), (case, k)


@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_hip_and_torch_agree(kind):
    """Within 2 C of the same magnitudes (each within C of the restatement); None picks the kernels; float64 tensors take the
    torch path on the device."""
    cases, reference = KINDS[kind][0](), KINDS[kind][1]
    for case in cases[::5] + cases[-2:]:
        ref = reference(case)
        hip, tor, default = _run(kind, case), _run(kind, case, implementation='torch'), _run(kind, case, implementation=None)
        assert np.array_equal(default[0], hip[0]) and np.array_equal(default[1], hip[1]), case
        assert R.worst_ratio(hip[0], tor[0], ref.loss_mag) <= 2 * CONSTANTS[kind, 'loss'], case
        assert R.worst_ratio(hip[1], tor[1], ref.grad_mag) <= 2 * CONSTANTS[kind, 'grad'], case
        import torch
        l64, g64 = _run(kind, case, implementation=None, dtype=torch.float64)
        assert l64.dtype == np.float64
        assert np.abs(l64 - ref.loss).max() <= 1e-12 * np.abs(ref.loss).max()
        assert np.abs(g64 - ref.grad).max() <= 1e-12 * np.abs(ref.grad).max()


def test_learnable_target_or_mask_takes_the_torch_path():
    import torch
    import neural_renderer_amd as nr
    x = torch.rand((2, 3, 8, 12), device='cuda', requires_grad=True)
    t = torch.rand((3, 8, 12), device='cuda', requires_grad=True)
    m = torch.rand((8, 12), device='cuda', requires_grad=True)
    nr.squared_error_loss(x, t, m, levels=2).sum().backward()
    assert all(z.grad is not None and bool(z.grad.abs().sum() > 0) for z in (x, t, m))
    with pytest.raises(ValueError, match='target or mask'):
        nr.squared_error_loss(x, t, implementation='hip')
    a = torch.rand((2, 8, 12), device='cuda')
    tt = torch.rand((8, 12), device='cuda', requires_grad=True)
    nr.silhouette_iou_loss(a, tt).sum().backward()
    assert bool(tt.grad.abs().sum() > 0)


# ---------------------------------------------------------------------------------------------------------------------
# views

def test_views_give_the_bits_of_their_contiguous_copies():
    """A rasterizer output (a view behind the image epilogue, or whatever it is), an expanded target, strided slices and a
    pointer that is not 16-byte aligned (the scalar path on a width that would take the vector path)."""
    import torch
    import neural_renderer_amd as nr
    import vertex_ref
    v, f = vertex_ref.icosphere(1)
    r = nr.Renderer()
    r.image_size = 32
    r.eye = nr.get_points_from_angles(2.732, 20, 40)
    vertices = torch.tensor(np.stack((v, 0.8 * v)).astype(np.float32), device='cuda')
    faces = torch.tensor(f.astype(np.int32), device='cuda')[None].expand(2, -1, -1)
    alpha = nr.rasterize_rgbad(r._frontend(vertices, faces)[0], None, 32, True, return_rgb=False, return_depth=False)['alpha']
    assert alpha.shape == (2, 32, 32) and bool((alpha > 0).any()) and bool((alpha < 1).any())
    target = torch.zeros((32, 32), device='cuda')
    target[8:24, 8:24] = 1
    expanded = target[None].expand(2, -1, -1)
    assert not expanded.is_contiguous()

    def both(fn, base, view, *others, **kw):
        """fn on view(leaf) and the arguments as they are, and on their contiguous copies: the same loss and the same
        gradient at the leaf, bit for bit"""
        out = []
        for contiguous in (False, True):
            leaf = base.detach().requires_grad_(True)    # (keeps base's strides: the rasterizer's output as it is)
            x, oth = view(leaf), others
            if contiguous:
                x, oth = x.contiguous(), tuple(o.contiguous() for o in others)
            loss = fn(x, *oth, implementation='hip', **kw)
            grad, = torch.autograd.grad((loss * torch.arange(1, loss.shape[0] + 1, device='cuda')).sum(), leaf)
            out.append((loss.detach(), grad))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        assert bool(out[0][1].abs().sum() > 0)
    both(nr.silhouette_iou_loss, alpha, lambda z: z, expanded, levels=4, level_weights=(1, 0.5, 0.25, 2))
    both(nr.silhouette_iou_loss, alpha, lambda z: z.transpose(1, 2), expanded, levels=3)
    wide, other = torch.rand((2, 3, 32, 72), device='cuda'), torch.rand((2, 3, 32, 72), device='cuda')
    mask = torch.rand((32, 64), device='cuda')[None].expand(2, -1, -1)
    both(nr.squared_error_loss, wide, lambda z: z[..., 4:68], other[0, :, :, 8:72], mask, levels=2)
    both(nr.squared_error_loss, wide, lambda z: z[..., ::2], other[..., 1::2], levels=3)
    # 64 floats wide, one float off the 16-byte grid: the same bits as the aligned copy
    flat = torch.rand((2 * 32 * 64 + 1,), device='cuda')
    off = flat[1:].view(2, 32, 64)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    for fn, args in ((nr.silhouette_iou_loss, (off, target.repeat(1, 2))), (nr.squared_error_loss, (off, target.repeat(1, 2)))):
        a = fn(*args, levels=3, implementation='hip')
        b = fn(args[0].clone(), args[1], levels=3, implementation='hip')
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the backward's launches

@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_no_backward_launch_without_an_image_gradient(kind):
    """ctx.needs_input_grad: with an image that requires no gradient the loss is a constant of the graph, nothing is kept, and
    a backward through what it is combined with launches neither backward kernel; with one, exactly one launch."""
    import torch
    from neural_renderer_amd import _lib
    import neural_renderer_amd as nr
    lib = _lib.load()
    names = ('nr_iou_loss_backward', 'nr_squared_error_backward')
    real = {n: getattr(lib, n) for n in names}
    calls = []

    def counting(n):
        def call(*args):
            calls.append(n)
            return real[n](*args)
        return call
    image = torch.rand((3, 24, 40), device='cuda')
    target = torch.rand((24, 40), device='cuda')
    fn = (lambda x: nr.silhouette_iou_loss(x, target, levels=3, implementation='hip')) if kind == 'iou' else \
        (lambda x: nr.squared_error_loss(x, target, target, levels=3, implementation='hip'))
    try:
        for n in names:
            setattr(lib, n, counting(n))
        scale = torch.ones(3, device='cuda', requires_grad=True)
        loss = fn(image)
        assert not loss.requires_grad and loss.grad_fn is None
        (loss * scale).sum().backward()
        assert torch.equal(scale.grad, loss) and calls == []
        x = image.clone().requires_grad_(True)
        (fn(x) * scale).sum().backward()
        assert calls == [names[0] if kind == 'iou' else names[1]] and bool(x.grad.abs().sum() > 0)
    finally:
        for n in names:
            setattr(lib, n, real[n])


# ---------------------------------------------------------------------------------------------------------------------
# graph capture, the example

def test_graph_capture_without_an_eager_call_first():
    """The functions hold no host tables: a step captured with neural_renderer_amd.graph.capture as the FIRST call of its
    shapes replays bit-equal to eager after the inputs change."""
    import torch
    import neural_renderer_amd as nr
    H, W = 48, 80     # (sizes no other test of this file uses: nothing of these shapes ran eagerly before)
    alpha = torch.tensor(R.alphas(H, W), device='cuda', requires_grad=True)
    image = torch.tensor(R.images(H, W, 3), device='cuda', requires_grad=True)
    target, mask = torch.tensor(R.targets(H, W, 'soft', True), device='cuda'), torch.tensor(R.masks(H, W, 'per'), device='cuda')
    itarget = torch.tensor(R.image_targets(H, W, 3, False), device='cuda')
    out = torch.zeros((2, 3), device='cuda')
    g = torch.tensor(R.UPSTREAM, dtype=torch.float32, device='cuda')

    def step():
        iou = nr.silhouette_iou_loss(alpha, target, levels=5, level_weights=R.WEIGHTS)
        se = nr.squared_error_loss(image, itarget, mask, levels=4, level_weights=R.WEIGHTS[:4])
        out[0].copy_(iou)
        out[1].copy_(se)
        return torch.autograd.grad(((iou + 0.5 * se) * g).sum(), [alpha, image])
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        alpha.copy_(torch.tensor(R.alphas(H, W, seed=1), device='cuda').flip(0))
        image.copy_(torch.tensor(R.images(H, W, 3, seed=1), device='cuda'))
    replay()
    torch.cuda.synchronize()
    got_out, got = out.clone(), [t.clone() for t in grads[0]]
    eager = step()
    assert torch.equal(got_out, out) and torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
    assert bool(got[0].abs().sum() > 0) and bool(got[1].abs().sum() > 0)


def test_example_silhouette_iou_first_steps():
    """examples/example_silhouette_iou.py: example 2's fit with the multi-scale IoU and both shape priors; 30 steps run, every
    term stays finite and the loss goes down."""
    import os
    import sys
    import torch
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import make_data
    make_data.main()
    import example_silhouette_iou
    data = os.path.join(ex, 'data')
    model = example_silhouette_iou.Model(os.path.join(data, 'teapot.obj'), os.path.join(data, 'example2_ref.png')).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, terms = model()
        loss.backward()
        opt.step()
        assert all(bool(torch.isfinite(t)) for t in terms) and bool(torch.isfinite(model.vertices.grad).all())
        losses.append(float(loss.detach()))
    print('example_silhouette_iou: loss %.4f -> %.4f (iou %.4f, laplacian %.4f, flatness %.2f at the end)'
          % ((losses[0], losses[-1]) + tuple(float(t.detach()) for t in terms)))
    assert losses[-1] < losses[0]
