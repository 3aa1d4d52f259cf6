"""Image losses without a GPU (neural_renderer_amd/image_losses.py): the float64 restatement of tests/image_loss_ref.py against
finite differences, the plain-torch paths against the restatement, the exact limits, argument errors and the C ABI's error
codes."""
import numpy as np
import pytest
import torch

import image_loss_ref as R
from neural_renderer_amd import image_losses as IL

# The four constants C of the checks |got - ref| <= C u M (tests/image_loss_ref.py): 4 x the worst ratio the float32 torch
# path shows against the float64 restatement over R.iou_cases() / R.se_cases() -- every size and level count, binary and soft
# targets, shared and per image, C in {-, 1, 3, 4}, no / shared / per-image masks, B = 3 and B = 1 --, rounded up to a power
# of two.  The float32 torch path must stay within C / 4 (test_float32_torch_paths_stay_within_a_quarter); the factor 4 is for
# a kernel that orders the same operations differently.
#                  measured worst float32 ratio
C_IOU_LOSS = 4     # 0.996  (18 x 38, 2 levels, a soft target shared by the batch; the others stay below 0.86)
C_IOU_GRAD = 16    # 3.892  (40 x 72, 3 levels, soft targets per image)
C_SE_LOSS = 16     # 3.129  (18 x 38, 2 levels, C = 3, shared target, per-image mask)
C_SE_GRAD = 16     # 3.856  (24 x 40, 2 levels, C = 3, shared target, shared mask)
CONSTANTS = {('iou', 'loss'): C_IOU_LOSS, ('iou', 'grad'): C_IOU_GRAD, ('se', 'loss'): C_SE_LOSS, ('se', 'grad'): C_SE_GRAD}


def _tensor(a, dtype, device):
    return None if a is None else torch.tensor(a, dtype=dtype, device=device)


def iou_loss_and_grad(fn, case, dtype, device='cpu', **kw):
    """(loss [B], grad [B,H,W]) as numpy for the upstream R.UPSTREAM"""
    alpha, target, weights = R.iou_inputs(case)
    a = torch.tensor(alpha, dtype=dtype, device=device, requires_grad=True)
    loss = fn(a, _tensor(target, dtype, device), levels=len(weights), level_weights=weights, eps=R.EPS, **kw)
    g = torch.tensor(R.UPSTREAM[:a.shape[0]], dtype=loss.dtype, device=device)
    grad, = torch.autograd.grad((loss * g).sum(), a)
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


def se_loss_and_grad(fn, case, dtype, device='cpu', **kw):
    x, target, mask, weights = R.se_inputs(case)
    x = torch.tensor(x, dtype=dtype, device=device, requires_grad=True)
    loss = fn(x, _tensor(target, dtype, device), _tensor(mask, dtype, device), levels=len(weights), level_weights=weights, **kw)
    g = torch.tensor(R.UPSTREAM[:x.shape[0]], dtype=loss.dtype, device=device)
    grad, = torch.autograd.grad((loss * g).sum(), x)
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


KINDS = {'iou': (R.iou_cases, R.iou_reference, iou_loss_and_grad, IL.silhouette_iou_loss_torch, IL.silhouette_iou_loss),
         'se': (R.se_cases, R.se_reference, se_loss_and_grad, IL.squared_error_loss_torch, IL.squared_error_loss)}


def ratios(kind, case, loss, grad):
    ref = KINDS[kind][1](case)
    return R.worst_ratio(loss, ref.loss, ref.loss_mag), R.worst_ratio(grad, ref.grad, ref.grad_mag)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, and the torch paths against it

def test_restatement_against_finite_differences():
    """Central differences of the float64 restatement's values against its closed-form gradients on small images with three
    levels.  Both losses are polynomials of degree <= 2 in the input up to the IoU's division: with h = 1e-6 the truncation
    (h^2 |f'''|) and the rounding (1e-16 |f| / h) both stay below 1e-8 of the largest gradient entry."""
    w = R.WEIGHTS[:3]
    alpha, target = R.alphas(16, 16).astype(np.float64), R.targets(16, 16, 'soft', False)
    x, xt, m = R.images(8, 12, 2).astype(np.float64), R.image_targets(8, 12, 2, True), R.masks(8, 12, 'per')
    h = 1e-6
    for value, ref, z in ((lambda z: R.iou_value(z, target, w), R.iou_ref(alpha, target, w), alpha),
                          (lambda z: R.se_value(z, xt, m, w), R.se_ref(x, xt, m, w), x)):
        fd = np.zeros_like(z)
        for idx in np.ndindex(*z.shape):
            zp, zm = z.copy(), z.copy()
            zp[idx] += h
            zm[idx] -= h
            fd[idx] = ((value(zp) - value(zm)) / (2 * h) * R.UPSTREAM).sum()
        assert np.abs(ref.grad).max() > 1e-3
        assert np.abs(fd - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max()


@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_float64_torch_paths_equal_the_restatement(kind):
    cases, reference, run, torch_fn, _ = KINDS[kind]
    for case in cases():
        ref = reference(case)
        loss, grad = run(torch_fn, case, torch.float64)
        assert loss.dtype == np.float64 and grad.shape == ref.grad.shape
        assert np.abs(loss - ref.loss).max() <= 1e-12 * np.abs(ref.loss).max(), case
        assert np.abs(grad - ref.grad).max() <= 1e-12 * np.abs(ref.grad).max(), case


@pytest.mark.parametrize('kind', ['iou', 'se'])
def test_float32_torch_paths_stay_within_a_quarter(kind):
    cases, _, run, torch_fn, _ = KINDS[kind]
    worst = [(0.0, None), (0.0, None)]
    for case in cases():
        rl, rg = ratios(kind, case, *run(torch_fn, case, torch.float32))
        worst = [max(worst[0], (rl, case)), max(worst[1], (rg, case))]
    print('%s, float32 torch path: worst ratio loss %.3f %s, gradient %.3f %s' % ((kind,) + worst[0] + worst[1]))
    assert worst[0][0] <= CONSTANTS[kind, 'loss'] / 4 and worst[1][0] <= CONSTANTS[kind, 'grad'] / 4


def test_default_implementation_on_cpu_is_the_torch_path():
    case = R.iou_cases()[5]
    assert all(np.array_equal(p, q) for p, q in zip(iou_loss_and_grad(IL.silhouette_iou_loss, case, torch.float32),
                                                    iou_loss_and_grad(IL.silhouette_iou_loss_torch, case, torch.float32)))
    case = R.se_cases()[17]
    assert all(np.array_equal(p, q) for p, q in zip(se_loss_and_grad(IL.squared_error_loss, case, torch.float32),
                                                    se_loss_and_grad(IL.squared_error_loss_torch, case, torch.float32)))
    assert all(np.array_equal(p, q) for p, q in zip(se_loss_and_grad(IL.squared_error_loss, case, torch.float32),
                                                    se_loss_and_grad(IL.squared_error_loss, case, torch.float32,
                                                                     implementation='torch')))


def test_exported_names():
    import neural_renderer
    import neural_renderer_amd as nr
    assert nr.silhouette_iou_loss is IL.silhouette_iou_loss and nr.squared_error_loss is IL.squared_error_loss
    assert neural_renderer.silhouette_iou_loss is IL.silhouette_iou_loss
    assert neural_renderer.squared_error_loss is IL.squared_error_loss
    assert 'silhouette_iou_loss' in nr.__all__ and 'squared_error_loss' in nr.__all__


# ---------------------------------------------------------------------------------------------------------------------
# exact values

@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_empty_silhouettes_and_equal_binary_silhouettes(dtype):
    w = (1.0, 0.5, 0.25, 2.0)
    # two empty silhouettes: every level is 1 - 0 / eps = 1, the loss exactly sum w_l, the gradient zero
    a = torch.zeros((2, 16, 24), dtype=dtype, requires_grad=True)
    loss = IL.silhouette_iou_loss(a, torch.zeros((16, 24), dtype=dtype), levels=4, level_weights=w)
    assert loss.shape == (2,) and loss.dtype == dtype and (loss == sum(w)).all()
    grad, = torch.autograd.grad(loss.sum(), a)
    assert not grad.any()
    ref = R.iou_ref(np.zeros((2, 16, 24)), np.zeros((16, 24)), w, g=(1.0, 1.0))
    assert (ref.loss == sum(w)).all() and not ref.grad.any()
    # alpha == target, binary, on whole 8 x 8 blocks: a_l = t_l stays binary on every level, I_l = U_l, and the loss is
    # sum_l w_l eps / (U_l + eps)
    t = torch.zeros((16, 24), dtype=dtype)
    t[8:16, 8:24] = 1
    loss = IL.silhouette_iou_loss(t[None].clone(), t, levels=4, level_weights=w, eps=1e-6)
    want = sum(wl * 1e-6 / (128.0 / 4 ** l + 1e-6) for l, wl in enumerate(w))
    tol = 4 * sum(w) * (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53)   # 1 - I / (U + eps) is rounded near 1
    assert abs(float(loss[0]) - want) <= tol and float(loss[0]) < 2e-6
    assert abs(R.iou_value(t[None].numpy(), t.numpy(), w)[0] - want) <= 1e-15
    # the squared error of an image with itself
    x = torch.rand((2, 3, 16, 24), dtype=dtype)
    assert not IL.squared_error_loss(x, x.clone(), levels=3).any()


def test_shapes():
    a, t = torch.rand(3, 8, 12), torch.rand(3, 8, 12)
    assert IL.silhouette_iou_loss(a, t).shape == (3,) and IL.silhouette_iou_loss(a, t[0], levels=3).shape == (3,)
    x = torch.rand(3, 2, 8, 12)
    for target in (torch.rand(3, 2, 8, 12), torch.rand(2, 8, 12)):
        for mask in (None, torch.rand(8, 12), torch.rand(3, 8, 12)):
            assert IL.squared_error_loss(x, target, mask, levels=2).shape == (3,)
    # [B,H,W] images are one channel
    y = torch.rand(3, 8, 12)
    assert torch.equal(IL.squared_error_loss(y, t, t[1]), IL.squared_error_loss(y[:, None], t[:, None], t[1]))
    assert torch.equal(IL.squared_error_loss(y, t[0]), IL.squared_error_loss(y[:, None], t[0][None]))
    # a learnable target takes the torch path's autograd
    tt = torch.rand(8, 12, requires_grad=True)
    IL.squared_error_loss(y, tt).sum().backward()
    assert tt.grad is not None and tt.grad.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# errors

def test_argument_errors():
    a, t = torch.rand(3, 24, 40), torch.rand(3, 24, 40)
    x, xt, m = torch.rand(3, 2, 24, 40), torch.rand(2, 24, 40), torch.rand(24, 40)
    calls = [(fn, (a, t)) for fn in (IL.silhouette_iou_loss, IL.silhouette_iou_loss_torch)] + \
            [(fn, (x, xt, m)) for fn in (IL.squared_error_loss, IL.squared_error_loss_torch)]
    for fn, args in calls:
        with pytest.raises(ValueError, match='levels'):     # 24 x 40 is no multiple of 16
            fn(*args, levels=5)
        for levels in (0, 6, 2.0, None):
            with pytest.raises(ValueError, match='levels'):
                fn(*args, levels=levels)
        for weights in ((1.0,), (1.0, 2.0, 3.0), ()):
            with pytest.raises(ValueError, match='level_weights'):
                fn(*args, levels=2, level_weights=weights)
        with pytest.raises(ValueError, match='level_weights'):
            fn(*args, levels=2, level_weights=torch.ones(2))
        with pytest.raises(ValueError, match='target'):
            fn(args[0], args[1][..., :39], *args[2:])
        with pytest.raises(ValueError, match='target'):
            fn(args[0], args[1].double(), *args[2:])
        with pytest.raises(ValueError, match='target'):
            fn(args[0], args[1].to('meta'), *args[2:])
        with pytest.raises(ValueError):
            fn(args[0].long(), *args[1:])
        with pytest.raises(ValueError):
            fn(args[0].numpy(), *args[1:])
    for fn in (IL.silhouette_iou_loss, IL.silhouette_iou_loss_torch):
        with pytest.raises(ValueError, match='alpha'):
            fn(x, x)                                          # [B,C,H,W] is no alpha
        with pytest.raises(ValueError, match='target'):
            fn(a, t[:2])
    for fn in (IL.squared_error_loss, IL.squared_error_loss_torch):
        for bad in (torch.rand(2, 24, 40), torch.rand(3, 2, 24, 40), torch.rand(24, 39), m.double()):
            with pytest.raises(ValueError, match='mask'):
                fn(x, xt, bad)
        with pytest.raises(ValueError, match='target'):
            fn(x, torch.rand(3, 24, 40))                      # neither [B,C,H,W] nor [C,H,W]
    for fn, args in calls[::2]:
        with pytest.raises(ValueError, match='implementation'):
            fn(*args, implementation='cuda')
        with pytest.raises(ValueError, match='HIP'):
            fn(*args, implementation='hip')                   # CPU tensors do not fit the kernels
        with pytest.raises(ValueError, match='HIP'):
            fn(*(z.double() for z in args), implementation='hip')


def test_new_entry_points_return_error_codes_without_a_gpu():
    import ctypes
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    # host only: one double per (image, tile of 64 x 16, sum), 2 levels sums at the most
    assert lib.nr_image_loss_workspace_bytes(3, 24, 40, 4) == 3 * 2 * 8 * 8
    assert lib.nr_image_loss_workspace_bytes(3, 40, 72, 3) == 3 * 6 * 6 * 8
    assert lib.nr_image_loss_workspace_bytes(64, 256, 256, 1) == 64 * 64 * 2 * 8
    assert lib.nr_image_loss_workspace_bytes(0, 8, 8, 1) == 0 and lib.nr_image_loss_workspace_bytes(65536, 8, 8, 1) == 0
    assert lib.nr_image_loss_workspace_bytes(1, 8, 8, 0) == 0 and lib.nr_image_loss_workspace_bytes(1, 8, 8, 6) == 0
    assert lib.nr_image_loss_workspace_bytes(1, 24, 40, 5) == 0 and lib.nr_image_loss_workspace_bytes(1, 0, 8, 1) == 0
    w = (ctypes.c_double * 5)(1, 1, 1, 1, 1)
    # NULL pointers (NR_E_NULL = -1), sizes (-2), workspace (-3): all before any launch
    assert lib.nr_iou_loss_forward(None, None, 1, None, None, None, 1, 8, 8, 1, 1e-6, None, 0, None) == -1
    assert lib.nr_iou_loss_forward(1, 1, 1, None, 1, None, 1, 8, 8, 1, 1e-6, 1, 64, None) == -1       # no weights
    assert lib.nr_iou_loss_forward(1, 1, 1, w, None, None, 1, 8, 8, 1, 1e-6, 1, 64, None) == -1
    for B, H, W, L in ((0, 8, 8, 1), (65536, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, 0), (1, 8, 8, 6), (1, 24, 40, 5),
                       (1, 8, 12, 4), (1, 32769, 8, 1)):
        assert lib.nr_iou_loss_forward(1, 1, 1, w, 1, None, B, H, W, L, 1e-6, 1, 1 << 30, None) == -2, (B, H, W, L)
        assert lib.nr_iou_loss_backward(1, 1, 1, w, 1, 1, B, H, W, L, 1e-6, None) == -2, (B, H, W, L)
        assert lib.nr_squared_error_forward(1, 1, None, 1, 0, w, 1, B, 3, H, W, L, 1, 1 << 30, None) == -2, (B, H, W, L)
        assert lib.nr_squared_error_backward(1, 1, None, 1, 0, w, 1, 1, B, 3, H, W, L, None) == -2, (B, H, W, L)
    assert lib.nr_iou_loss_forward(1, 1, 1, w, 1, None, 3, 24, 40, 4, 1e-6, None, 0, None) == -3
    assert lib.nr_iou_loss_forward(1, 1, 1, w, 1, None, 3, 24, 40, 4, 1e-6, 1, 3 * 2 * 8 * 8 - 1, None) == -3
    assert lib.nr_iou_loss_backward(None, 1, None, None, None, None, 1, 8, 8, 1, 1e-6, None) == -1
    assert lib.nr_iou_loss_backward(1, 1, None, w, 1, 1, 1, 8, 8, 1, 1e-6, None) == -1                 # no saved sums
    assert lib.nr_iou_loss_backward(1, 1, 1, w, 1, None, 1, 8, 8, 1, 1e-6, None) == -1
    assert lib.nr_squared_error_forward(None, None, None, 1, 0, None, None, 1, 3, 8, 8, 1, None, 0, None) == -1
    assert lib.nr_squared_error_forward(1, None, None, 1, 0, w, 1, 1, 3, 8, 8, 1, 1, 64, None) == -1
    assert lib.nr_squared_error_forward(1, 1, None, 1, 0, w, 1, 1, 0, 8, 8, 1, 1, 64, None) == -2      # no channel
    assert lib.nr_squared_error_forward(1, 1, None, 1, 0, w, 1, 1, 4, 32768, 32768, 1, 1, 1 << 40, None) == -2   # 2^32 elements
    assert lib.nr_squared_error_forward(1, 1, None, 1, 0, w, 1, 2, 3, 24, 40, 2, None, 0, None) == -3
    assert lib.nr_squared_error_backward(None, None, None, 1, 0, None, None, None, 1, 3, 8, 8, 1, None) == -1
    assert lib.nr_squared_error_backward(1, 1, None, 1, 0, w, 1, None, 1, 3, 8, 8, 1, None) == -1
    assert lib.nr_squared_error_backward(1, 1, None, 1, 0, w, 1, 1, 1, 0, 8, 8, 1, None) == -2
