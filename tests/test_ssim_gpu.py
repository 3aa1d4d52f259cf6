"""The SSIM loss on the GPU (include/nr_hip.h nr_ssim_loss_forward / _backward; neural_renderer_amd/image_losses.py): the
loss, the map and the gradient entry by entry against the float64 restatement of tests/ssim_ref.py within its constants, tile
borders, exact zeros, bit-for-bit repetition, the batch against its slices, views, the torch path, the backward's launches and
the example's first steps."""
import numpy as np
import pytest

import ssim_ref as R
from test_ssim import index_map, loss_and_grad, ratios, within

pytestmark = pytest.mark.gpu


def _f32():
    import torch
    return torch.float32


def _run(case, **kw):
    """(loss, grad) of ssim_loss on the device (implementation = 'hip' unless said otherwise)"""
    from neural_renderer_amd import image_losses as IL
    kw.setdefault('implementation', 'hip')
    return loss_and_grad(IL.ssim_loss, case, kw.pop('dtype', _f32()), device='cuda', **kw)


def _check(case):
    loss, grad = _run(case)
    smap = index_map(case, _f32(), device='cuda', implementation='hip')
    rl, rg, rs = ratios(case, loss, grad, smap)
    n = case[2]
    print('%s: loss at %.3f of u M (C = %d), gradient at %.3f (C = %d), map at %.3f (C = %d)'
          % (case, rl, R.c_loss(n), rg, R.c_grad(n), rs, R.c_map(n)))
    assert loss.dtype == np.float32 and grad.dtype == np.float32 and smap.dtype == np.float32
    assert within(case, rl, rg, rs), case
    return rl, rg, rs


def test_against_the_float64_restatement():
    """Every case of R.cases(), none left out: B = 3 with [B,H,W] images and C in {1, 3, 4} at 24 x 40, 40 x 72 (six tiles, the
    last an 8 x 8 corner), 18 x 38 and 7 x 37 (the scalar path), windows 3, 7 and 11 under both paddings and reductions, 5 x 9
    with window 11 under 'same', 11 x 11 with window 11 under 'valid' (one window), the target shared and per image, the
    mask absent, shared, per image and with one image's mask all 0, and B = 1; mixed-sign upstream gradients."""
    cases = R.cases()
    worst = [max(rs) for rs in zip(*[_check(case) for case in cases])]
    print('%d cases, worst ratio loss %.3f, gradient %.3f, map %.3f' % ((len(cases),) + tuple(worst)))


def test_all_zero_mask_gives_zero_loss_and_gradient():
    seen = 0
    for case in R.cases():
        if case[7] == 'zero':
            loss, grad = _run(case)
            k = min(1, case[9] - 1)
            assert loss[k] == 0 and not grad[k].any(), case
            seen += 1
    assert seen >= 4


def test_tile_borders():
    """x zero except one pixel at each of (15, 63) and (16, 64), y a constant, on 40 x 136: the four tiles that meet at
    (16, 64) each see both pixels through their halo.  The map and the gradient match the restatement there, under both
    paddings.  And an input that is non-zero only in the last partial tile of 40 x 72 shows up in the loss."""
    import torch
    import neural_renderer_amd as nr
    H, W = 40, 136
    x = np.zeros((1, 2, H, W), np.float32)
    x[0, 0, 15, 63], x[0, 0, 16, 64], x[0, 1, 15, 63], x[0, 1, 16, 64] = 0.8, 0.6, 0.3, 0.9
    y = np.full((2, H, W), 0.25, np.float32)
    for n, padding in ((11, 'same'), (11, 'valid'), (7, 'same'), (3, 'valid')):
        ref = R.ssim_ref(x, y, None, n, padding, 'sum', g=(1.0,))
        xt = torch.tensor(x, device='cuda', requires_grad=True)
        yt = torch.tensor(y, device='cuda')
        loss = nr.ssim_loss(xt, yt, window_size=n, padding=padding, reduction='sum', implementation='hip')
        grad, = torch.autograd.grad(loss.sum(), xt)
        smap = nr.ssim_index(xt.detach(), yt, window_size=n, padding=padding, implementation='hip')
        r = n // 2 if padding == 'valid' else 0
        box = (slice(None), slice(None), slice(10 - r, 22 - r), slice(58 - r, 70 - r))      # 6 pixels around (16, 64)
        assert (ref.smap[box] != ref.smap[0, 0, 0, 0]).any()
        assert R.worst_ratio(smap.cpu().numpy(), ref.smap, ref.smap_mag) <= R.c_map(n), (n, padding)
        assert R.worst_ratio(grad.cpu().numpy(), ref.grad, ref.grad_mag) <= R.c_grad(n), (n, padding)
        assert R.worst_ratio(loss.detach().cpu().numpy(), ref.loss, ref.loss_mag) <= R.c_loss(n), (n, padding)
    H, W = 40, 72
    a = np.full((1, H, W), 0.5, np.float32)
    t = a[0].copy()
    a[:, 34:, 66:] = 0.9
    for reduction in ('sum', 'mean'):
        ref = R.ssim_ref(a, t, None, 3, 'same', reduction, g=(1.0,))
        got = nr.ssim_loss(torch.tensor(a, device='cuda'), torch.tensor(t, device='cuda'), window_size=3, reduction=reduction,
                           implementation='hip').cpu().numpy()
        assert ref.loss[0] > (1.0 if reduction == 'sum' else 1e-3)
        assert R.worst_ratio(got, ref.loss, ref.loss_mag) <= R.c_loss(3)


def test_bit_equal_images_and_target_give_exactly_zero():
    import torch
    import neural_renderer_amd as nr
    torch.manual_seed(5)
    for x in (torch.rand((2, 3, 40, 72), device='cuda'), 0.9 + 1e-3 * torch.rand((2, 3, 40, 72), device='cuda'),
              torch.rand((2, 18, 38), device='cuda')):
        for n, padding in ((11, 'same'), (11, 'valid'), (5, 'same'), (3, 'valid')):
            for reduction in ('mean', 'sum'):
                loss = nr.ssim_loss(x, x.clone(), window_size=n, padding=padding, reduction=reduction, implementation='hip')
                assert not loss.any(), (n, padding, reduction)
                loss = nr.ssim_loss(x, x[0].clone(), torch.rand(x.shape[-2:], device='cuda'), window_size=n, padding=padding,
                                    reduction=reduction, implementation='hip')
                assert loss[0] == 0 and loss[1] > 0
            assert bool((nr.ssim_index(x, x.clone(), window_size=n, padding=padding, implementation='hip') == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# the same bits

def _picked():
    return [c for c in R.cases() if (c[0], c[1]) in ((40, 72), (18, 38), (5, 9)) and c[9] == R.B]


def test_two_runs_and_batch_slices_give_the_same_bits():
    import torch
    import neural_renderer_amd as nr
    picked = _picked()
    assert len(picked) >= 12
    for case in picked:
        H, W, n, padding, C, kind, shared, mk, reduction, batch = case
        first, second = _run(case), _run(case)
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]), case
        x, t, m = R.inputs(case)
        dev = lambda a: None if a is None else torch.tensor(a, device='cuda')
        for k in range(batch):     # every image alone: the same bits as inside the batch
            image = torch.tensor(x[k:k + 1], device='cuda', requires_grad=True)
            loss = nr.ssim_loss(image, dev(t if shared else t[k:k + 1]), dev(m if m is None or m.ndim == 2 else m[k:k + 1]),
                                window_size=n, padding=padding, reduction=reduction, implementation='hip')
            grad, = torch.autograd.grad(loss[0] * float(R.UPSTREAM[k]), image)
            assert np.array_equal(loss.detach().cpu().numpy(), first[0][k:k + 1]), (case, k)
            assert np.array_equal(grad.cpu().numpy(), first[1][k:k + 1]), (case, k)


def test_hip_and_torch_agree():
    """Within 2 C of the same magnitudes (each within C of the restatement); None picks the kernels; float64 tensors take the
    torch path on the device."""
    import torch
    cases = R.cases()
    for case in cases[::4] + cases[-3:]:
        ref, n = R.reference(case), case[2]
        hip, tor, default = _run(case), _run(case, implementation='torch'), _run(case, implementation=None)
        assert np.array_equal(default[0], hip[0]) and np.array_equal(default[1], hip[1]), case
        assert R.worst_ratio(hip[0], tor[0], ref.loss_mag) <= 2 * R.c_loss(n), case
        assert R.worst_ratio(hip[1], tor[1], ref.grad_mag) <= 2 * R.c_grad(n), case
        hmap, tmap = (index_map(case, _f32(), device='cuda', implementation=i) for i in ('hip', 'torch'))
        assert np.array_equal(index_map(case, _f32(), device='cuda'), hmap)
        assert R.worst_ratio(hmap, tmap, ref.smap_mag) <= 2 * R.c_map(n), case
        l64, g64 = _run(case, implementation=None, dtype=torch.float64)
        assert l64.dtype == np.float64
        assert np.abs(l64 - ref.loss).max() <= 1e-11 * ref.loss_mag.max()
        assert (np.abs(g64 - ref.grad) <= 1e-11 * ref.grad_mag + 1e-300).all()


def test_learnable_target_or_mask_takes_the_torch_path():
    import torch
    import neural_renderer_amd as nr
    x = torch.rand((2, 3, 12, 16), device='cuda', requires_grad=True)
    t = torch.rand((3, 12, 16), device='cuda', requires_grad=True)
    m = torch.rand((12, 16), device='cuda', requires_grad=True)
    nr.ssim_loss(x, t, m, window_size=5).sum().backward()
    assert all(z.grad is not None and bool(z.grad.abs().sum() > 0) for z in (x, t, m))
    with pytest.raises(ValueError, match='ssim_loss: the HIP kernels give no gradient to target or mask'):
        nr.ssim_loss(x, t, implementation='hip')
    with pytest.raises(ValueError, match='target or mask'):
        nr.ssim_loss(x, t.detach(), m, implementation='hip')


# ---------------------------------------------------------------------------------------------------------------------
# views

def test_views_give_the_bits_of_their_contiguous_copies():
    """Strided, transposed and expanded inputs, and a contiguous view 4 bytes off the 16-byte grid (the scalar path on a width
    that would take the vector path): each gives the bits of its contiguous copy."""
    import torch
    import neural_renderer_amd as nr
    torch.manual_seed(6)

    def both(base, view, *others, **kw):
        out = []
        for contiguous in (False, True):
            leaf = base.detach().requires_grad_(True)
            x, oth = view(leaf), others
            if contiguous:
                x, oth = x.contiguous(), tuple(o.contiguous() for o in others)
            loss = nr.ssim_loss(x, *oth, implementation='hip', **kw)
            grad, = torch.autograd.grad((loss * torch.arange(1, loss.shape[0] + 1, device='cuda')).sum(), leaf)
            smap = nr.ssim_index(x.detach(), oth[0], implementation='hip', **{k: v for k, v in kw.items() if k != 'reduction'})
            out.append((loss.detach(), grad, smap))
        assert all(torch.equal(p, q) for p, q in zip(*out))
        assert bool(out[0][1].abs().sum() > 0)
    wide, other = torch.rand((2, 3, 32, 72), device='cuda'), torch.rand((2, 3, 32, 72), device='cuda')
    mask = torch.rand((32, 64), device='cuda')[None].expand(2, -1, -1)
    assert not mask.is_contiguous()
    both(wide, lambda z: z[..., 4:68], other[0, :, :, 8:72], mask, window_size=7)                      # strided slices
    both(wide, lambda z: z[..., ::2], other[..., 1::2], window_size=11, padding='valid', reduction='sum')
    both(wide, lambda z: z.transpose(2, 3), other.transpose(2, 3), window_size=5, padding='valid')      # transposed
    both(wide, lambda z: z, other[0][None].expand(2, -1, -1, -1), window_size=3)                        # expanded
    # 64 floats wide, one float off the 16-byte grid: the same bits as the aligned copy
    flat = torch.rand((2 * 32 * 64 + 1,), device='cuda')
    off = flat[1:].view(2, 32, 64)
    target = torch.rand((32, 64), device='cuda')
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    leaf = off.detach().requires_grad_(True)
    assert leaf.data_ptr() % 16 == 4
    copy = off.clone().requires_grad_(True)
    assert copy.data_ptr() % 16 == 0
    a, b = (nr.ssim_loss(z, target, target, implementation='hip') for z in (leaf, copy))
    ga, gb = torch.autograd.grad(a.sum(), leaf)[0], torch.autograd.grad(b.sum(), copy)[0]
    assert torch.equal(a, b) and torch.equal(ga, gb) and bool(ga.abs().sum() > 0)
    assert torch.equal(nr.ssim_index(off, target, implementation='hip'), nr.ssim_index(off.clone(), target, implementation='hip'))


# ---------------------------------------------------------------------------------------------------------------------
# the backward's launches

def test_no_backward_launch_without_an_image_gradient():
    """ctx.needs_input_grad: with images that require no gradient the loss is a constant of the graph, nothing is kept (the
    forward is not asked for its three maps), and a backward through what it is combined with launches no backward kernel;
    with one, exactly one launch."""
    import torch
    from neural_renderer_amd import _lib
    import neural_renderer_amd as nr
    lib = _lib.load()
    names = ('nr_ssim_loss_forward', 'nr_ssim_loss_backward')
    real = {n: getattr(lib, n) for n in names}
    calls = []

    def counting(n):
        def call(*args):
            calls.append((n, args))
            return real[n](*args)
        return call
    image = torch.rand((3, 24, 40), device='cuda')
    target = torch.rand((24, 40), device='cuda')
    fn = lambda x: nr.ssim_loss(x, target, target, window_size=7, implementation='hip')
    try:
        for n in names:
            setattr(lib, n, counting(n))
        scale = torch.ones(3, device='cuda', requires_grad=True)
        loss = fn(image)
        assert not loss.requires_grad and loss.grad_fn is None
        (loss * scale).sum().backward()
        assert torch.equal(scale.grad, loss) and [c[0] for c in calls] == [names[0]]
        assert calls[0][1][8] is None and calls[0][1][9] is None          # grad_maps, scales: nothing to keep
        del calls[:]
        x = image.clone().requires_grad_(True)
        (fn(x) * scale).sum().backward()
        assert [c[0] for c in calls] == list(names) and bool(x.grad.abs().sum() > 0)
        assert calls[0][1][8] is not None and calls[0][1][9] is not None
    finally:
        for n in names:
            setattr(lib, n, real[n])


# ---------------------------------------------------------------------------------------------------------------------
# the example

def test_example_ssim_first_steps():
    """examples/example_ssim.py: vertex colours fitted to a target picture under squared error + lambda SSIM; 30 steps run,
    every term stays finite and the loss goes down."""
    import os
    import sys
    import torch
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import example_ssim
    model = example_ssim.Model().cuda()
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, terms = model()
        loss.backward()
        opt.step()
        assert all(bool(torch.isfinite(t)) for t in terms) and bool(torch.isfinite(model.colors.grad).all())
        losses.append(float(loss.detach()))
    print('example_ssim: loss %.4f -> %.4f (squared error %.5f, 1 - SSIM %.4f at the end)'
          % ((losses[0], losses[-1]) + tuple(float(t.detach()) for t in terms)))
    assert losses[-1] < losses[0]
