"""The SSIM loss without a GPU (neural_renderer_amd/image_losses.py ssim_loss / ssim_loss_torch / ssim_index): the float64
restatement of tests/ssim_ref.py against finite differences, the plain-torch paths against the restatement within the
constants the GPU test uses, exact values, two deliberately wrong restatements that the bounds must refuse, argument errors and
the C ABI's error codes."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_ref as R
from neural_renderer_amd import image_losses as IL


def _tensor(a, dtype, device):
    return None if a is None else torch.tensor(a, dtype=dtype, device=device)


def loss_and_grad(fn, case, dtype, device='cpu', **kw):
    """(loss [B], grad, the shape of images) as numpy for the upstream R.UPSTREAM"""
    H, W, n, padding, C, kind, shared, mk, reduction, batch = case
    x, t, m = R.inputs(case)
    x = torch.tensor(x, dtype=dtype, device=device, requires_grad=True)
    loss = fn(x, _tensor(t, dtype, device), _tensor(m, dtype, device), window_size=n, padding=padding, reduction=reduction, **kw)
    g = torch.tensor(R.UPSTREAM[:batch], dtype=loss.dtype, device=device)
    grad, = torch.autograd.grad((loss * g).sum(), x)
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


def index_map(case, dtype, device='cpu', **kw):
    x, t, _ = R.inputs(case)
    return IL.ssim_index(_tensor(x, dtype, device), _tensor(t, dtype, device), window_size=case[2], padding=case[3], **kw).cpu().numpy()


def ratios(case, loss, grad, smap=None):
    """worst |got - ref| / (u M) of the loss, the gradient and (given) the map"""
    ref = R.reference(case)
    out = (R.worst_ratio(loss, ref.loss, ref.loss_mag), R.worst_ratio(grad, ref.grad, ref.grad_mag))
    return out + ((R.worst_ratio(smap, ref.smap, ref.smap_mag),) if smap is not None else ())


def within(case, rl, rg, rs=None):
    n = case[2]
    return rl <= R.c_loss(n) and rg <= R.c_grad(n) and (rs is None or rs <= R.c_map(n))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, and the torch paths against it

def test_window():
    for n in (3, 5, 7, 9, 11):
        w = R.window(n)
        assert np.array_equal(w, np.array(IL.ssim_window(n, 1.5))) and np.array_equal(w, w.astype(np.float32).astype(np.float64))
        assert abs(w.sum() - 1) <= n * 2.0 ** -25 and np.array_equal(w, w[::-1]) and w.argmax() == n // 2
    assert abs(R.window(11)[5] - 0.26601) < 1e-4       # the centre tap of the usual 11-tap window at sigma 1.5


def test_restatement_against_finite_differences():
    """Central differences of the float64 restatement's loss against its closed-form gradient on small images, for both
    paddings and reductions, with and without a mask.  S is a rational function of the pixels with b1 b2 >= C1 C2 > 0; with
    h = 1e-6 the truncation and the rounding (1e-16 |f| / h) both stay below 1e-6 of the largest gradient entry."""
    h = 1e-6
    for n, padding, reduction, mk, C in ((3, 'same', 'mean', 'per', 2), (5, 'valid', 'sum', 'none', 1), (7, 'same', 'sum', 'shared', 1),
                                         (5, 'valid', 'mean', 'per', 2)):
        x = R.images(8, 10, C, 'noise').astype(np.float64)
        t, m = R.image_targets(8, 10, C, 'noise', True), R.masks(8, 10, mk)
        ref = R.ssim_ref(x, t, m, n, padding, reduction)
        fd = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            fd[idx] = ((R.ssim_value(xp, t, m, n, padding, reduction) - R.ssim_value(xm, t, m, n, padding, reduction)) / (2 * h)
                       * R.UPSTREAM).sum()
        assert np.abs(ref.grad).max() > 1e-3
        assert np.abs(fd - ref.grad).max() <= 1e-6 * np.abs(ref.grad).max(), (n, padding, reduction)


def test_float64_torch_path_equals_the_restatement():
    for case in R.cases():
        ref = R.reference(case)
        loss, grad = loss_and_grad(IL.ssim_loss_torch, case, torch.float64)
        smap = index_map(case, torch.float64)
        assert loss.dtype == np.float64 and grad.shape == ref.grad.shape and smap.shape == ref.smap.shape
        # (against the magnitudes: the flat images' gradients and maps cancel to 1e-4 of their terms)
        assert np.abs(loss - ref.loss).max() <= 1e-11 * ref.loss_mag.max(), case
        assert (np.abs(grad - ref.grad) <= 1e-11 * ref.grad_mag + 1e-300).all(), case
        assert (np.abs(smap - ref.smap) <= 1e-11 * ref.smap_mag).all(), case


def test_float32_torch_path_stays_within_the_constants():
    """The constants the GPU test holds the kernels to (R.c_loss, R.c_grad, R.c_map), on every case."""
    worst = [(0.0, None)] * 3
    for case in R.cases():
        loss, grad = loss_and_grad(IL.ssim_loss_torch, case, torch.float32)
        rs = ratios(case, loss, grad, index_map(case, torch.float32))
        worst = [max(w, (r, case)) for w, r in zip(worst, rs)]
        assert within(case, *rs), (case, rs)
    print('float32 torch path: worst ratio loss %.3f %s, gradient %.3f %s, map %.3f %s' % (worst[0] + worst[1] + worst[2]))


def test_all_zero_mask_gives_zero_loss_and_gradient():
    case = [c for c in R.cases() if c[7] == 'zero' and c[8] == 'mean'][0]
    for dtype in (torch.float32, torch.float64):
        loss, grad = loss_and_grad(IL.ssim_loss_torch, case, dtype)
        assert loss[1] == 0 and not grad[1].any() and loss[0] > 0 and grad[0].any()
    ref = R.reference(case)
    assert ref.loss[1] == 0 and not ref.grad[1].any() and ref.loss_mag[1] == 0 and not ref.grad_mag[1].any()


def test_default_implementation_on_cpu_is_the_torch_path():
    case = R.cases()[5]
    for kw in ({}, {'implementation': 'torch'}):
        assert all(np.array_equal(p, q) for p, q in zip(loss_and_grad(IL.ssim_loss, case, torch.float32, **kw),
                                                        loss_and_grad(IL.ssim_loss_torch, case, torch.float32)))


def test_exported_names():
    import neural_renderer
    import neural_renderer_amd as nr
    for name in ('ssim_loss', 'ssim_index'):
        assert getattr(nr, name) is getattr(IL, name) and getattr(neural_renderer, name) is getattr(IL, name) and name in nr.__all__


# ---------------------------------------------------------------------------------------------------------------------
# exact values

@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_an_image_with_itself_and_two_constants(dtype):
    x = torch.rand((2, 3, 16, 24), dtype=dtype)
    for padding in ('same', 'valid'):
        S = IL.ssim_index(x, x.clone(), window_size=7, padding=padding)
        assert S.shape == ((2, 3, 16, 24) if padding == 'same' else (2, 3, 10, 18)) and bool((S == 1).all())
        assert not IL.ssim_loss(x, x.clone(), window_size=7, padding=padding).any()
    assert IL.ssim_index(x[:, 0], x[0, 0], window_size=3).shape == (2, 16, 24)       # [B,H,W] images: no channel axis
    # two constant images under 'valid': mu = the constants, every variance 0 -- S = (2ab + C1) / (a^2 + b^2 + C1)
    a, b, c1 = 0.75, 0.5, 0.01 ** 2
    S = IL.ssim_index(torch.full((1, 1, 12, 14), a, dtype=dtype), torch.full((1, 12, 14), b, dtype=dtype), padding='valid')
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    ref = R.ssim_ref(np.full((1, 1, 12, 14), a), np.full((1, 12, 14), b), None, 11, 'valid')
    # (the float32 taps sum to s = 1 + O(2^-25), not 1: mu = a s^2, G*(x^2) = a^2 s^2, so sxx = a^2 s^2 (1 - s^2) instead of 0 --
    # a relative (a + b)^2 |1 - s^2| / C2 on a2 / b2 and 2 |s^4 - 1| on a1 / b1 at the most)
    dev = abs(R.window(11).sum() ** 2 - 1)
    assert 0 < dev < 1e-6 and S.shape == (1, 1, 2, 4)
    assert np.abs(ref.smap - want).max() <= 1.01 * want * ((a + b) ** 2 * dev / 0.03 ** 2 + 4 * dev)
    assert np.abs(S.numpy() - ref.smap).max() <= R.c_map(11) * eps * ref.smap_mag.max()
    loss = IL.ssim_loss(torch.full((1, 1, 12, 14), a, dtype=dtype), torch.full((1, 12, 14), b, dtype=dtype), padding='valid')
    assert abs(float(loss[0]) - ref.loss[0]) <= R.c_loss(11) * eps * ref.loss_mag.max()


def test_shapes():
    x = torch.rand(3, 2, 12, 14)
    for target in (torch.rand(3, 2, 12, 14), torch.rand(2, 12, 14)):
        for mask in (None, torch.rand(12, 14), torch.rand(3, 12, 14)):
            for kw in ({}, {'padding': 'valid', 'window_size': 5}, {'reduction': 'sum'}):
                assert IL.ssim_loss(x, target, mask, **kw).shape == (3,)
    y, t = torch.rand(3, 12, 14), torch.rand(3, 12, 14)
    assert torch.equal(IL.ssim_loss(y, t, t[1]), IL.ssim_loss(y[:, None], t[:, None], t[1]))
    tt = torch.rand(12, 14, requires_grad=True)      # a learnable target takes the torch path's autograd
    IL.ssim_loss(y, tt).sum().backward()
    assert tt.grad is not None and tt.grad.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the bounds refuse wrong restatements

def test_the_bounds_refuse_two_wrong_restatements():
    """On the inputs of the cases themselves: (1) a window whose outermost tap is dropped and the rest renormalised (n - 1
    taps side by side with the right centre: the last tap 0); (2) 'same' answered with the 'valid' values where both have a
    window -- the interior -- and nothing (0) on the border.  Both must fail the loss, map and gradient bounds."""
    checked = 0
    for case in R.cases():
        H, W, n, padding, C, kind, shared, mk, reduction, batch = case
        if (H, W) != (24, 40) or mk == 'zero' or batch != R.B:
            continue
        x, t, m = R.inputs(case)
        ref = R.reference(case)
        taps = R.window(n).copy()
        taps[-1] = 0
        wrong = R.ssim_ref(x, t, m, n, padding, reduction, taps=taps / taps.sum())
        rs = ratios(case, wrong.loss, wrong.grad, wrong.smap)
        # (nearly flat images hardly see the window at all -- away from a 'same' border every normalised window gives the same
        # means, and the variances are 1e-6 --: the first wrong restatement is told apart on the inputs with structure)
        # The loss is measured against sum |m| (1 + M_S), about 1 per window, and 1 - S of a target 2 % away is 1e-3: there a
        # wrong window moves the loss by less than the bound, and it is the map and the gradient that tell it apart.
        assert kind == 'flat' or (rs[1] > R.c_grad(n) and rs[2] > R.c_map(n) and (rs[0] > R.c_loss(n) or kind == 'near')), (case, rs)
        checked += 1
        if padding != 'same':
            continue
        r = n // 2
        valid = R.ssim_ref(x, t, m, n, 'valid', reduction)
        smap = np.zeros_like(ref.smap)
        smap[..., r:H - r, r:W - r] = valid.smap
        assert R.worst_ratio(smap[..., r:H - r, r:W - r], ref.smap[..., r:H - r, r:W - r], ref.smap_mag[..., r:H - r, r:W - r]) <= 1e-6
        assert R.worst_ratio(smap, ref.smap, ref.smap_mag) > R.c_map(n), case
        if m is None and reduction == 'sum':    # the loss that this map gives
            loss = (1 - smap).reshape(batch, -1).sum(1)
            assert R.worst_ratio(loss, ref.loss, ref.loss_mag) > R.c_loss(n), case
        checked += 1
    assert checked >= 12


# ---------------------------------------------------------------------------------------------------------------------
# errors

def test_argument_errors():
    x, xt, m = torch.rand(3, 2, 24, 40), torch.rand(2, 24, 40), torch.rand(24, 40)
    for fn in (IL.ssim_loss, IL.ssim_loss_torch, IL.ssim_index):
        name = fn.__name__
        args = (x, xt) if fn is IL.ssim_index else (x, xt, m)
        for bad in (2, 4, 13, 1, 0, -3, 7.0, None, torch.tensor(7)):
            with pytest.raises(ValueError, match=name + ': window_size'):
                fn(*args, window_size=bad)
        for key in ('sigma', 'data_range'):
            for bad in (0, -1.0, float('nan')):
                with pytest.raises(ValueError, match='%s: %s' % (name, key)):
                    fn(*args, **{key: bad})
        for key in ('sigma', 'data_range', 'k1', 'k2'):
            with pytest.raises(ValueError, match='%s: %s must be a host number' % (name, key)):
                fn(*args, **{key: torch.tensor(1.0)})
        with pytest.raises(ValueError, match=name + ': padding'):
            fn(*args, padding='reflect')
        with pytest.raises(ValueError, match=name + ": with padding = 'valid'"):
            fn(x[..., :9], xt[..., :9], padding='valid')       # 9 wide: no 11-tap window fits
        with pytest.raises(ValueError, match=name + ': target'):
            fn(x, xt[..., :39], *args[2:])
        with pytest.raises(ValueError, match=name + ': target'):
            fn(x, xt.double(), *args[2:])
        with pytest.raises(ValueError, match=name):
            fn(x.long(), *args[1:])
    for fn in (IL.ssim_loss, IL.ssim_loss_torch):
        with pytest.raises(ValueError, match=fn.__name__ + ': reduction'):
            fn(x, xt, m, reduction='none')
        for bad in (torch.rand(2, 24, 40), torch.rand(24, 39), m.double()):
            with pytest.raises(ValueError, match=fn.__name__ + ': mask'):
                fn(x, xt, bad)
    for fn, args in ((IL.ssim_loss, (x, xt, m)), (IL.ssim_index, (x, xt))):
        with pytest.raises(ValueError, match='implementation'):
            fn(*args, implementation='cuda')
        with pytest.raises(ValueError, match=fn.__name__ + ': the HIP kernels take float32 CUDA tensors'):
            fn(*args, implementation='hip')                   # CPU tensors do not fit the kernels
        with pytest.raises(ValueError, match='HIP'):
            fn(*(z.double() for z in args), implementation='hip')


def test_entry_points_return_error_codes_without_a_gpu():
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    # host only: two doubles per (image, tile of 64 x 16 window centres)
    assert lib.nr_ssim_workspace_bytes(3, 24, 40, 11, 0) == 3 * 2 * 2 * 8
    assert lib.nr_ssim_workspace_bytes(3, 40, 72, 7, 0) == 3 * 6 * 2 * 8
    assert lib.nr_ssim_workspace_bytes(3, 40, 72, 11, 1) == 3 * 2 * 2 * 8          # 30 x 62 centres
    assert lib.nr_ssim_workspace_bytes(64, 256, 256, 11, 0) == 64 * 64 * 2 * 8
    for B, H, W, n, valid in ((0, 8, 8, 3, 0), (65536, 8, 8, 3, 0), (1, 0, 8, 3, 0), (1, 8, 8, 1, 0), (1, 8, 8, 4, 0),
                              (1, 8, 8, 13, 0), (1, 10, 40, 11, 1), (1, 32769, 8, 3, 0)):
        assert lib.nr_ssim_workspace_bytes(B, H, W, n, valid) == 0, (B, H, W, n, valid)
        assert lib.nr_ssim_loss_forward(1, 1, None, 1, 0, (ctypes.c_float * 11)(), 1, None, None, None, B, 3, H, W, n, valid, 1,
                                        1e-4, 9e-4, 1, 1 << 30, None) == -2, (B, H, W, n, valid)
        assert lib.nr_ssim_loss_backward(1, 1, None, 1, 0, (ctypes.c_float * 11)(), 1, 1, 1, 1, B, 3, H, W, n, valid, None) == -2
    w = (ctypes.c_float * 11)(*IL.ssim_window(11, 1.5))
    # NULL pointers (NR_E_NULL = -1), sizes (-2), workspace (-3): all before any launch

    def forward(images, target, window, loss, maps, scales, B, C, H, W, workspace, workspace_bytes):
        return lib.nr_ssim_loss_forward(images, target, None, 1, 0, window, loss, None, maps, scales, B, C, H, W, 11, 0, 1, 1e-4, 9e-4,
                                        workspace, workspace_bytes, None)
    assert forward(None, None, None, None, None, None, 1, 3, 16, 16, None, 0) == -1
    assert forward(1, 1, None, 1, None, None, 1, 3, 16, 16, 1, 64) == -1          # no window
    assert forward(1, 1, w, 1, 1, None, 1, 3, 16, 16, 1, 64) == -1                # the maps without k per image
    assert forward(1, 1, w, 1, None, 1, 1, 3, 16, 16, 1, 64) == -1
    assert forward(1, 1, w, 1, None, None, 1, 0, 16, 16, 1, 64) == -2             # no channel
    assert forward(1, 1, w, 1, None, None, 3, 3, 24, 40, None, 0) == -3
    assert forward(1, 1, w, 1, None, None, 3, 3, 24, 40, 1, 3 * 2 * 2 * 8 - 1) == -3
    assert lib.nr_ssim_loss_backward(None, None, None, 1, 0, None, None, None, None, None, 1, 3, 16, 16, 11, 0, None) == -1
    assert lib.nr_ssim_loss_backward(1, 1, None, 1, 0, w, None, 1, 1, 1, 1, 3, 16, 16, 11, 0, None) == -1     # no saved maps
    assert lib.nr_ssim_loss_backward(1, 1, None, 1, 0, w, 1, 1, 1, None, 1, 3, 16, 16, 11, 0, None) == -1
    assert lib.nr_ssim_loss_backward(1, 1, None, 1, 0, w, 1, 1, 1, 1, 1, 4, 32768, 32768, 11, 0, None) == -2   # 2^32 elements
