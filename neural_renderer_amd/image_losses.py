"""The objective of a mesh fit on images (not in the reference's library): the silhouette IoU loss of its paper (Neural 3D
Mesh Renderer, section 5) and a masked squared error, both optionally on an image pyramid, one loss per image.

`silhouette_iou_loss(alpha, target)` takes alpha [B,H,W] and a target [B,H,W] or [H,W]; `squared_error_loss(images, target,
mask)` takes images [B,C,H,W] or [B,H,W], a target of the same shape or that shape without the batch axis, and a mask [B,H,W]
or [H,W] that applies to every channel.  A target or mask without the batch axis is shared by the batch and read once, not
expanded.  Both return float [B] and are once-differentiable in `alpha` / `images` only.

Definitions.  P_0(z) = z; P_l(z) is the 2 x 2 mean of P_(l-1)(z), (((p00 + p01) + p10) + p11) * 0.25 with the upper row
first.  `levels` in 1 .. 5 is the number of pyramid levels, `level_weights` a sequence of `levels` host numbers w_l (default:
all 1); H and W must be multiples of 2^(levels - 1).
    IoU, a_l = P_l(alpha), t_l = P_l(target):   I_l = sum a_l t_l,   U_l = sum (a_l + t_l - a_l t_l),
        loss_b = sum_l w_l (1 - I_l / (U_l + eps))
      (two empty silhouettes: exactly sum_l w_l, and a zero gradient);
    squared error, d = mask (images - target) (no mask: 1), d_l = P_l(d):   loss_b = sum_l w_l sum_{c,P} d_l^2
      (the level sums carry no implicit rescaling: the weights are the caller's).

On CUDA float32 tensors with B <= 65535 (and fewer than 2^31 elements per image, H, W <= 32768) both run as HIP kernels in
both directions (nr_iou_loss_* / nr_squared_error_*, csrc/nr_image_losses.hip): one pass over the inputs that forms every
level of a tile on chip, sums in double in a fixed order, no atomics -- the results repeat bit for bit, and an image alone
gives the bits it has inside a batch.  The kernels give no gradient to `target` or `mask`: a target or mask that requires
grad, and everything else that does not fit, takes the plain-torch implementations `silhouette_iou_loss_torch` /
`squared_error_loss_torch` (any device, any float dtype, avg_pool2d), which are also the kernels' second yardstick in the
tests.  The functions hold no host tables: a first call inside graph.capture works without an eager step before it.

`ssim_loss(images, target, mask)` is the structural term that a photometric fit pairs with the squared error,
(1 - lambda) L_pix + lambda (1 - SSIM); `ssim_index` returns the map itself.  Inputs as in squared_error_loss.  The window is
w[k] ~ exp(-(k - R)^2 / 2 sigma^2), k = 0 .. n - 1, n = window_size = 2R + 1 odd in 3 .. 11, computed in double, normalised to
sum 1 and rounded to float32 (`ssim_window`); the 2-D window is w (x) w and G*z the windowed sum of z.  padding = 'same': z
reads as 0 outside the image and every pixel is a window centre (Hq x Wq = H x W); 'valid': only the windows inside the image
(Hq x Wq = (H - 2R) x (W - 2R)).  Per channel and window centre q
    mu_x = G*x, mu_y = G*y, sxx = G*(x^2) - mu_x^2, syy = G*(y^2) - mu_y^2, sxy = G*(x y) - mu_x mu_y,
    a1 = 2 mu_x mu_y + C1, a2 = 2 sxy + C2, b1 = mu_x^2 + mu_y^2 + C1, b2 = sxx + syy + C2,
    S = (a1 a2) / (b1 b2),  C1 = (k1 data_range)^2,  C2 = (k2 data_range)^2,
    loss_b = k sum_{c,q} m_b(q) (1 - S_c(q)),
m the mask at the window's centre pixel (None: 1), k = 1 for reduction = 'sum' and 1 / (C sum_q m_b(q)) for 'mean'; an image
whose mask sums to 0 has loss 0 and a zero gradient.  On float32 CUDA tensors it runs as HIP kernels in both directions
(nr_ssim_loss_*, csrc/nr_ssim.hip): one fused pass per direction, sums in double in a fixed order, no atomics; images bit-equal
to the target give a loss of exactly 0.  With a gradient to follow the forward keeps three float maps [B,C,Hq,Wq] for the
backward.  `ssim_loss_torch` is the same in plain torch (the windowed sums tap by tap on shifted slices, autograd)."""
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib, _util

MAX_LEVELS = 5
MAX_WINDOW = 11


# ---------------------------------------------------------------------------------------------------------------------
# checks shared by both implementations

def _levels(name, levels, level_weights, H, W):
    """-> (levels, weights: tuple of floats)"""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError('%s: levels must be an integer in 1 .. %d, got %r' % (name, MAX_LEVELS, levels))
    if level_weights is None:
        weights = (1.0,) * levels
    else:
        if torch.is_tensor(level_weights):
            raise ValueError('%s: level_weights must be a sequence of host numbers, not a tensor' % name)
        weights = tuple(float(w) for w in level_weights)
        if len(weights) != levels:
            raise ValueError('%s: level_weights has %d entries for levels = %d' % (name, len(weights), levels))
    step = 1 << (levels - 1)
    if H % step or W % step:
        raise ValueError('%s: with levels = %d the height and width of the images must be multiples of %d, got %d x %d'
                         % (name, levels, step, H, W))
    return levels, weights


def _same_kind(name, what, t, like):
    if not (torch.is_tensor(t) and t.is_floating_point()):
        raise ValueError('%s: %s must be a float tensor' % (name, what))
    if t.device != like.device or t.dtype != like.dtype:
        raise ValueError('%s: %s must have the dtype and device of the images (%s on %s), got %s on %s'
                         % (name, what, like.dtype, like.device, t.dtype, t.device))


def _check(name, what, images, target, mask):
    """-> (images [B,C,H,W], target [B or 1,C,H,W], mask [B or 1,1,H,W] or None): shape / dtype / device checks; the
    results are views."""
    if not (torch.is_tensor(images) and images.is_floating_point() and images.dim() in (3, 4) and min(images.shape) >= 1):
        raise ValueError('%s: %s must be a non-empty float tensor %s' % (name, what, '[batch size, height, width]' if
                         what == 'alpha' else '[batch size, channels, height, width] or [batch size, height, width]'))
    _same_kind(name, 'target', target, images)
    if tuple(target.shape) == tuple(images.shape):
        target = target if images.dim() == 4 else target[:, None]
    elif tuple(target.shape) == tuple(images.shape[1:]):
        target = target[None] if images.dim() == 4 else target[None, None]
    else:
        raise ValueError('%s: target must have the shape of %s %s or that shape without the batch axis, got %s'
                         % (name, what, tuple(images.shape), tuple(target.shape)))
    if images.dim() == 3:
        images = images[:, None]
    if mask is not None:
        _same_kind(name, 'mask', mask, images)
        hw = tuple(images.shape[2:])
        if tuple(mask.shape) == (images.shape[0],) + hw:
            mask = mask[:, None]
        elif tuple(mask.shape) == hw:
            mask = mask[None, None]
        else:
            raise ValueError('%s: mask must be [batch size, height, width] or [height, width] of the images %s, got %s'
                             % (name, tuple(images.shape), tuple(mask.shape)))
    return images, target, mask


def _use_hip(name, implementation, images, others):
    B, C, H, W = images.shape
    fits = (images.is_cuda and images.dtype == torch.float32 and B <= 65535 and C * H * W < 2 ** 31 and H <= 32768
            and W <= 32768)
    learnable = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in others)
    hip = _util.takes_hip(name, implementation, fits, 'the HIP kernels take float32 CUDA tensors with a batch size of 65535 at '
                          'most')
    if implementation == 'hip' and learnable:
        raise ValueError('%s: the HIP kernels give no gradient to target or mask' % name)
    return hip and not learnable


# ---------------------------------------------------------------------------------------------------------------------
# plain torch

def _iou_torch(a, t, weights, eps):
    loss = 0
    for l, w in enumerate(weights):
        if l:
            a, t = F.avg_pool2d(a, 2), F.avg_pool2d(t, 2)
        p = a * t
        loss = loss + w * (1 - p.sum((1, 2, 3)) / ((a + t - p).sum((1, 2, 3)) + eps))
    return loss


def _se_torch(x, t, m, weights):
    d = x - t
    if m is not None:
        d = m * d
    loss = 0
    for l, w in enumerate(weights):
        if l:
            d = F.avg_pool2d(d, 2)
        loss = loss + w * (d * d).sum((1, 2, 3))
    return loss


def silhouette_iou_loss_torch(alpha, target, levels=1, level_weights=None, eps=1e-6):
    """silhouette_iou_loss in plain torch (any device, any float dtype), differentiable by torch's autograd."""
    name = 'silhouette_iou_loss_torch'
    if torch.is_tensor(alpha) and alpha.dim() != 3:
        raise ValueError('%s: alpha must be a float tensor [batch size, height, width]' % name)
    a, t, _ = _check(name, 'alpha', alpha, target, None)
    levels, weights = _levels(name, levels, level_weights, a.shape[2], a.shape[3])
    return _iou_torch(a, t, weights, float(eps))


def squared_error_loss_torch(images, target, mask=None, levels=1, level_weights=None):
    """squared_error_loss in plain torch (any device, any float dtype), differentiable by torch's autograd."""
    name = 'squared_error_loss_torch'
    x, t, m = _check(name, 'images', images, target, mask)
    levels, weights = _levels(name, levels, level_weights, x.shape[2], x.shape[3])
    return _se_torch(x, t, m, weights)


# ---------------------------------------------------------------------------------------------------------------------
# HIP

def _weights_array(weights):
    return (ctypes.c_double * MAX_LEVELS)(*weights)


@_util.once_differentiable
class _IoULoss(torch.autograd.Function):
    """forward(ctx, alpha [B,1,H,W], target [B or 1,1,H,W], weights, eps) -> loss [B]; the target and the 2 levels sums of
    every image are kept for the backward when one can follow."""

    @staticmethod
    def forward(ctx, alpha, target, weights, eps):
        a, t = alpha.detach().contiguous(), target.detach().contiguous()
        dev = a.device
        B, _, H, W = a.shape
        levels = len(weights)
        want = ctx.needs_input_grad[0]
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        sums = torch.empty((B, 2 * levels), dtype=torch.float64, device=dev) if want else None
        _lib.launch('nr_iou_loss_forward', dev, a.data_ptr(), t.data_ptr(), int(t.shape[0] != 1 or B == 1),
                    _weights_array(weights), loss.data_ptr(), _lib.ptr(sums), B, H, W, levels, eps,
                    workspace_bytes=_lib.workspace_bytes('nr_image_loss_workspace_bytes', B, H, W, levels))
        if want:
            ctx.save_for_backward(t, sums)
        ctx.weights, ctx.eps, ctx.shape = weights, eps, (B, H, W)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        t, sums = ctx.saved_tensors
        dev = t.device
        B, H, W = ctx.shape
        g = grad_loss.contiguous()
        grad = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        _lib.launch('nr_iou_loss_backward', dev, t.data_ptr(), int(t.shape[0] != 1 or B == 1), sums.data_ptr(),
                    _weights_array(ctx.weights), g.data_ptr(), grad.data_ptr(), B, H, W, len(ctx.weights), ctx.eps)
        return grad, None, None, None


@_util.once_differentiable
class _SquaredError(torch.autograd.Function):
    """forward(ctx, images [B,C,H,W], target [B or 1,C,H,W], mask [B or 1,1,H,W] or None, weights) -> loss [B]; the backward
    recomputes the differences from the inputs."""

    @staticmethod
    def forward(ctx, images, target, mask, weights):
        x, t = images.detach().contiguous(), target.detach().contiguous()
        m = None if mask is None else mask.detach().contiguous()
        dev = x.device
        B, C, H, W = x.shape
        levels = len(weights)
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.launch('nr_squared_error_forward', dev, x.data_ptr(), t.data_ptr(), _lib.ptr(m), int(t.shape[0] != 1 or B == 1),
                    int(m is not None and (m.shape[0] != 1 or B == 1)), _weights_array(weights), loss.data_ptr(), B, C, H, W,
                    levels, workspace_bytes=_lib.workspace_bytes('nr_image_loss_workspace_bytes', B, H, W, levels))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(*((x, t) if m is None else (x, t, m)))
        ctx.weights = weights
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        x, t = ctx.saved_tensors[:2]
        m = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        dev = x.device
        B, C, H, W = x.shape
        g = grad_loss.contiguous()
        grad = torch.empty_like(x)
        _lib.launch('nr_squared_error_backward', dev, x.data_ptr(), t.data_ptr(), _lib.ptr(m),
                    int(t.shape[0] != 1 or B == 1), int(m is not None and (m.shape[0] != 1 or B == 1)),
                    _weights_array(ctx.weights), g.data_ptr(), grad.data_ptr(), B, C, H, W, len(ctx.weights))
        return grad, None, None, None


def silhouette_iou_loss(alpha, target, levels=1, level_weights=None, eps=1e-6, implementation=None):
    """sum_l w_l (1 - I_l / (U_l + eps)) per image (see the module docstring): [B] from alpha [B,H,W] and a target [B,H,W]
    or [H,W] (one target for the batch).  The values are taken as given: the IoU expects them in [0, 1] (an anti-aliased
    silhouette and a binary or soft mask); outside that range the formula is evaluated all the same.  Differentiable (once)
    in alpha only.  `implementation`: None picks the HIP kernels when the call fits them, 'torch' / 'hip' force one ('hip'
    raises when the call does not fit)."""
    name = 'silhouette_iou_loss'
    if torch.is_tensor(alpha) and alpha.dim() != 3:
        raise ValueError('%s: alpha must be a float tensor [batch size, height, width]' % name)
    a, t, _ = _check(name, 'alpha', alpha, target, None)
    levels, weights = _levels(name, levels, level_weights, a.shape[2], a.shape[3])
    if _use_hip(name, implementation, a, (target,)):
        return _IoULoss.apply(a, t, weights, float(eps))
    return _iou_torch(a, t, weights, float(eps))


def squared_error_loss(images, target, mask=None, levels=1, level_weights=None, implementation=None):
    """sum_l w_l sum_{c,P} P_l(mask (images - target))^2 per image (see the module docstring): [B] from images [B,C,H,W] or
    [B,H,W], a target of that shape or without its batch axis, and a mask [B,H,W] or [H,W] (None: 1) that applies to every
    channel.  Differentiable (once) in images only; `implementation` as in silhouette_iou_loss."""
    name = 'squared_error_loss'
    x, t, m = _check(name, 'images', images, target, mask)
    levels, weights = _levels(name, levels, level_weights, x.shape[2], x.shape[3])
    if _use_hip(name, implementation, x, (target, mask)):
        return _SquaredError.apply(x, t, m, weights)
    return _se_torch(x, t, m, weights)


# ---------------------------------------------------------------------------------------------------------------------
# SSIM

def ssim_window(window_size, sigma):
    """The taps w[k] ~ exp(-(k - R)^2 / 2 sigma^2) of the SSIM window: computed in double, normalised to sum 1, rounded to
    float32 -- a tuple of `window_size` floats that float32 holds exactly."""
    R = window_size // 2
    taps = [math.exp(-((k - R) ** 2) / (2.0 * sigma * sigma)) for k in range(window_size)]
    total = math.fsum(taps)
    return tuple(float(torch.tensor(t / total, dtype=torch.float64).to(torch.float32)) for t in taps)


def _host_number(name, what, value):
    if torch.is_tensor(value) or isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError('%s: %s must be a host number, got %r' % (name, what, type(value).__name__))
    return float(value)


def _ssim_arguments(name, x, window_size, sigma, data_range, k1, k2, padding, reduction):
    """-> (window: tuple of floats, C1, C2, valid, mean)"""
    if torch.is_tensor(window_size) or isinstance(window_size, bool) or not isinstance(window_size, int) \
            or not 3 <= window_size <= MAX_WINDOW or window_size % 2 == 0:
        raise ValueError('%s: window_size must be an odd integer in 3 .. %d, got %r' % (name, MAX_WINDOW, window_size))
    sigma, data_range = _host_number(name, 'sigma', sigma), _host_number(name, 'data_range', data_range)
    k1, k2 = _host_number(name, 'k1', k1), _host_number(name, 'k2', k2)
    if not sigma > 0:
        raise ValueError('%s: sigma must be positive, got %r' % (name, sigma))
    if not data_range > 0:
        raise ValueError('%s: data_range must be positive, got %r' % (name, data_range))
    if padding not in ('same', 'valid'):
        raise ValueError("%s: padding must be 'same' or 'valid', got %r" % (name, padding))
    if reduction not in ('mean', 'sum'):
        raise ValueError("%s: reduction must be 'mean' or 'sum', got %r" % (name, reduction))
    H, W = x.shape[2:]
    if padding == 'valid' and (H < window_size or W < window_size):
        raise ValueError("%s: with padding = 'valid' the images must be at least window_size = %d high and wide, got %d x %d"
                         % (name, window_size, H, W))
    return ssim_window(window_size, sigma), (k1 * data_range) ** 2, (k2 * data_range) ** 2, padding == 'valid', reduction == 'mean'


def _window_sums(z, window, valid):
    """G*z over the last two axes, tap by tap on shifted slices, rows then columns: sum_k w[k] z(q - R + k).  Not conv2d: on
    the GPU the backward of a grouped conv2d is not exact where every term is 0 (DESIGN "Image losses: SSIM"), and a pixel
    out of reach of the mask must get a gradient of exactly 0."""
    n, R = len(window), len(window) // 2
    if not valid:
        z = F.pad(z, (R, R, R, R))
    Hq, Wq = z.shape[-2] - 2 * R, z.shape[-1] - 2 * R
    rows = window[0] * z[..., :, 0:Wq]
    for k in range(1, n):
        rows = rows + window[k] * z[..., :, k:k + Wq]
    out = window[0] * rows[..., 0:Hq, :]
    for k in range(1, n):
        out = out + window[k] * rows[..., k:k + Hq, :]
    return out


def _ssim_map_torch(x, t, window, c1, c2, valid):
    """S [B,C,Hq,Wq]: the five windowed sums as one stack."""
    C = x.shape[1]
    t = t.expand_as(x)
    z = _window_sums(torch.cat((x, t, x * x, t * t, x * t), 1), window, valid)
    mux, muy, gxx, gyy, gxy = z.split(C, 1)
    pxx, pyy, pxy = mux * mux, muy * muy, mux * muy
    sxx, syy, sxy = gxx - pxx, gyy - pyy, gxy - pxy
    return (((pxy + pxy) + c1) * ((sxy + sxy) + c2)) / (((pxx + pyy) + c1) * ((sxx + syy) + c2))


def _ssim_torch(x, t, m, window, c1, c2, valid, mean):
    S = _ssim_map_torch(x, t, window, c1, c2, valid)
    C, R = x.shape[1], len(window) // 2
    if m is None:
        total = (1 - S).sum((1, 2, 3))
        return total / (C * S.shape[2] * S.shape[3]) if mean else total
    if valid:
        m = m[:, :, R:m.shape[2] - R, R:m.shape[3] - R]
    total = (m * (1 - S)).sum((1, 2, 3))
    if not mean:
        return total
    msum = m.sum((1, 2, 3)).expand(x.shape[0])
    ok = msum != 0
    return torch.where(ok, total / (C * torch.where(ok, msum, torch.ones_like(msum))), torch.zeros_like(total))


def _ssim_launch(x, t, m, window, c1, c2, valid, mean, want_map, want_grad):
    """nr_ssim_loss_forward on contiguous x [B,C,H,W], t [B or 1,C,H,W], m [B or 1,1,H,W] or None -> (loss [B], S or None,
    (maps [3,B,C,Hq,Wq], scales [B]) or None)"""
    dev = x.device
    B, C, H, W = x.shape
    n = len(window)
    Hq, Wq = (H - n + 1, W - n + 1) if valid else (H, W)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    smap = torch.empty((B, C, Hq, Wq), dtype=torch.float32, device=dev) if want_map else None
    maps = torch.empty((3, B, C, Hq, Wq), dtype=torch.float32, device=dev) if want_grad else None
    scales = torch.empty((B,), dtype=torch.float64, device=dev) if want_grad else None
    _lib.launch('nr_ssim_loss_forward', dev, x.data_ptr(), t.data_ptr(), _lib.ptr(m), int(t.shape[0] != 1 or B == 1),
                int(m is not None and (m.shape[0] != 1 or B == 1)), (ctypes.c_float * n)(*window), loss.data_ptr(),
                _lib.ptr(smap), _lib.ptr(maps), _lib.ptr(scales), B, C, H, W, n, int(valid), int(mean), c1, c2,
                workspace_bytes=_lib.workspace_bytes('nr_ssim_workspace_bytes', B, H, W, n, int(valid)))
    return loss, smap, ((maps, scales) if want_grad else None)


@_util.once_differentiable
class _SSIMLoss(torch.autograd.Function):
    """forward(ctx, images [B,C,H,W], target [B or 1,C,H,W], mask [B or 1,1,H,W] or None, window, c1, c2, valid, mean) ->
    loss [B]; when a backward can follow, the inputs, the forward's three maps M1, M2, M3 and k per image are kept for it."""

    @staticmethod
    def forward(ctx, images, target, mask, window, c1, c2, valid, mean):
        x, t = images.detach().contiguous(), target.detach().contiguous()
        m = None if mask is None else mask.detach().contiguous()
        want = ctx.needs_input_grad[0]
        loss, _, saved = _ssim_launch(x, t, m, window, c1, c2, valid, mean, False, want)
        if want:
            ctx.save_for_backward(*((x, t) + saved + (() if m is None else (m,))))
        ctx.window, ctx.valid = window, valid
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        x, t, maps, scales = ctx.saved_tensors[:4]
        m = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        dev = x.device
        B, C, H, W = x.shape
        n = len(ctx.window)
        g = grad_loss.contiguous()
        grad = torch.empty_like(x)
        _lib.launch('nr_ssim_loss_backward', dev, x.data_ptr(), t.data_ptr(), _lib.ptr(m), int(t.shape[0] != 1 or B == 1),
                    int(m is not None and (m.shape[0] != 1 or B == 1)), (ctypes.c_float * n)(*ctx.window), maps.data_ptr(),
                    scales.data_ptr(), g.data_ptr(), grad.data_ptr(), B, C, H, W, n, int(ctx.valid))
        return (grad,) + (None,) * 7


def ssim_loss_torch(images, target, mask=None, window_size=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, padding='same',
                    reduction='mean'):
    """ssim_loss in plain torch (any device, any float dtype): the windowed sums tap by tap on shifted slices with zero padding
    or none, differentiable by torch's autograd."""
    name = 'ssim_loss_torch'
    x, t, m = _check(name, 'images', images, target, mask)
    window, c1, c2, valid, mean = _ssim_arguments(name, x, window_size, sigma, data_range, k1, k2, padding, reduction)
    return _ssim_torch(x, t, m, window, c1, c2, valid, mean)


def ssim_loss(images, target, mask=None, window_size=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, padding='same',
              reduction='mean', implementation=None):
    """k sum_{c,q} mask(q) (1 - S_c(q)) per image (see the module docstring): [B] from images [B,C,H,W] or [B,H,W], a target
    of that shape or without its batch axis (shared, read in place), and a mask [B,H,W] or [H,W] (None: 1) taken at the
    window's centre pixel.  window_size odd in 3 .. 11, sigma, data_range, k1, k2 host numbers; padding 'same' | 'valid';
    reduction 'mean' (k = 1 / (C sum mask)) | 'sum' (k = 1).  Differentiable (once) in images only; `implementation` as in
    silhouette_iou_loss.  Graph capture is not tested with this operator; the README's advice applies: capture a whole step
    with neural_renderer_amd.graph.capture before any eager backward on the same leaves, or make the eager calls under
    no_grad."""
    name = 'ssim_loss'
    x, t, m = _check(name, 'images', images, target, mask)
    window, c1, c2, valid, mean = _ssim_arguments(name, x, window_size, sigma, data_range, k1, k2, padding, reduction)
    if _use_hip(name, implementation, x, (target, mask)):
        return _SSIMLoss.apply(x, t, m, window, c1, c2, valid, mean)
    return _ssim_torch(x, t, m, window, c1, c2, valid, mean)


def ssim_index(images, target, window_size=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, padding='same',
               implementation=None):
    """The map S of ssim_loss, [B,C,Hq,Wq] (images [B,H,W]: [B,Hq,Wq]), for evaluation: no gradient."""
    name = 'ssim_index'
    x, t, _ = _check(name, 'images', images, target, None)
    window, c1, c2, valid, _ = _ssim_arguments(name, x, window_size, sigma, data_range, k1, k2, padding, 'mean')
    with torch.no_grad():
        if _use_hip(name, implementation, x, ()):
            S = _ssim_launch(x.contiguous(), t.contiguous(), None, window, c1, c2, valid, True, True, False)[1]
        else:
            S = _ssim_map_torch(x, t, window, c1, c2, valid)
    return S[:, 0] if images.dim() == 3 else S
