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
tests.  The functions hold no host tables: a first call inside graph.capture works without an eager step before it."""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib, _util

MAX_LEVELS = 5


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
