"""The yardstick of the image losses (neural_renderer_amd/image_losses.py): seeded inputs, and a float64 NumPy restatement of
the two definitions -- loops over the levels, no torch -- with the closed-form gradients for an upstream g_b and, with every
value, the magnitude its float32 evaluation is measured against.

P_0(z) = z, P_l(z) the 2 x 2 mean of P_(l-1)(z), (((p00 + p01) + p10) + p11) * 0.25, upper row first.
  IoU:  a_l = P_l(alpha), t_l = P_l(target), I_l = sum a_l t_l, U_l = sum (a_l + t_l - a_l t_l),
    loss_b = sum_l w_l (1 - I_l / (U_l + eps)),
    d loss_b / d alpha(p) = -sum_l w_l 4^-l [t_l(P) (U_l + eps) - I_l (1 - t_l(P))] / (U_l + eps)^2,  P the level-l block of p
  squared error:  d = mask (images - target), d_l = P_l(d),  loss_b = sum_l w_l sum_{c,P} d_l^2,
    d loss_b / d images(c, p) = sum_l 2 w_l 4^-l mask(p) d_l(c, P)

u = 2^-24.  A check is |got - ref| <= C u M for every entry, exact equality where M = 0 (`worst_ratio`).
  IoU loss           M = sum_l |w_l| (1 + I_l / (U_l + eps))
  IoU gradient       M = the gradient's sum with both bracket terms taken absolute (and |g_b w_l|)
  squared-error loss M = sum_l |w_l| sum d_l^2
  squared-error grad M = sum_l 2 |w_l g_b| 4^-l |mask| P_l(|d|)
"""
import functools
import itertools

import numpy as np

U = 2.0 ** -24
UPSTREAM = np.array([1.0, -0.5, 2.0])          # mixed signs, one per image
WEIGHTS = (1.0, 0.5, 0.25, 2.0, 0.75)          # of mixed size; a case takes the first `levels`
EPS = 1e-6
B = 3

# (H, W, levels).  24 x 40 and 32 x 48: not square, no multiple of the kernels' 64 x 16 tile, rows that end the 16-byte path
# before the tile does.  40 x 72: see test_image_losses_gpu.test_several_workgroups_per_image.  18 x 38 and 7 x 37: widths
# that are no multiple of 4 -- the kernels' scalar path.
SIZES = ((24, 40, 1), (24, 40, 2), (24, 40, 3), (24, 40, 4), (32, 48, 5), (40, 72, 3), (18, 38, 2), (7, 37, 1))
BIG = (40, 72, 3)


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def _disc(H, W, cy, cx, radius, band):
    """1 inside a disc, 0 outside, a linear ramp of `band` pixels across its edge: what an anti-aliased silhouette is."""
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
    dist = np.sqrt((y - cy * H) ** 2 + (x - cx * W) ** 2)
    return np.clip((radius * min(H, W) - dist) / band + 0.5, 0.0, 1.0)


def alphas(H, W, batch=B, seed=0):
    """float32 [batch,H,W]: an all-0 region, an all-1 region and a fractional band between them"""
    rng = np.random.default_rng(7300 + seed)
    out = np.stack([_disc(H, W, 0.5 + 0.08 * k, 0.45 + 0.05 * k, 0.3 + 0.03 * k, 2.5 + k) for k in range(batch)])
    band = (out > 0) & (out < 1)
    out[band] = np.clip(out[band] + rng.uniform(-0.1, 0.1, size=int(band.sum())), 0.01, 0.99)
    assert (out == 0).any() and (out == 1).any() and band.any()
    return np.ascontiguousarray(out.astype(np.float32))


def targets(H, W, kind, shared, batch=B):
    """float32 [batch,H,W] or, shared, [H,W]: 'binary' (0 / 1) or 'soft' (with a ramp)"""
    n = 1 if shared else batch
    out = np.stack([_disc(H, W, 0.45 - 0.04 * k, 0.55 - 0.03 * k, 0.33 - 0.02 * k, 3.0) for k in range(n)])
    if kind == 'binary':
        out = (out > 0.5).astype(np.float64)
    out = out.astype(np.float32)
    return np.ascontiguousarray(out[0] if shared else out)


def images(H, W, C, batch=B, seed=0):
    """float32 [batch,C,H,W] (C = 0: [batch,H,W]) uniform in [0, 1)"""
    rng = np.random.default_rng(7400 + seed)
    shape = (batch, H, W) if C == 0 else (batch, C, H, W)
    return rng.uniform(size=shape).astype(np.float32)


def image_targets(H, W, C, shared, batch=B, seed=0):
    rng = np.random.default_rng(7500 + seed)
    shape = ((H, W) if C == 0 else (C, H, W))
    return rng.uniform(size=shape if shared else (batch,) + shape).astype(np.float32)


def masks(H, W, kind, batch=B, seed=0):
    """None, [H,W] ('shared') or [batch,H,W] ('per'): a third zeros, a third ones, a third fractions"""
    if kind == 'none':
        return None
    rng = np.random.default_rng(7600 + seed)
    shape = (H, W) if kind == 'shared' else (batch, H, W)
    m = rng.uniform(size=shape)
    pick = rng.integers(0, 3, size=shape)
    return np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, m)).astype(np.float32)


def iou_cases():
    """(H, W, levels, target kind, target shared, batch size)"""
    out = [s + tk for s in SIZES for tk in itertools.product(('binary', 'soft'), (False, True), (B,))]
    return out + [(24, 40, 4, 'soft', False, 1), (40, 72, 3, 'binary', True, 1)]


def se_cases():
    """(H, W, levels, C (0: images [B,H,W]), target shared, mask kind, batch size)"""
    out = [s + k for s in SIZES for k in itertools.product((0, 1, 3, 4), (False, True), ('none', 'shared', 'per'), (B,))]
    return out + [(24, 40, 4, 3, False, 'per', 1), (40, 72, 3, 4, True, 'shared', 1)]


@functools.lru_cache(maxsize=None)
def iou_inputs(case):
    """(alpha, target, weights) of an iou_cases() entry; treat as read-only"""
    H, W, levels, kind, shared, batch = case
    return alphas(H, W, batch), targets(H, W, kind, shared, batch), WEIGHTS[:levels]


@functools.lru_cache(maxsize=None)
def se_inputs(case):
    """(images, target, mask, weights) of an se_cases() entry; treat as read-only"""
    H, W, levels, C, shared, mkind, batch = case
    return images(H, W, C, batch), image_targets(H, W, C, shared, batch), masks(H, W, mkind, batch), WEIGHTS[:levels]


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement

class Result(object):
    """loss [B], its magnitude [B]; grad (the shape of the input) for the upstream g, its magnitude"""

    def __init__(self, loss, loss_mag, grad, grad_mag):
        self.loss, self.loss_mag, self.grad, self.grad_mag = loss, loss_mag, grad, grad_mag


def pool(z):
    """the 2 x 2 mean over the last two axes, upper row first"""
    return (((z[..., 0::2, 0::2] + z[..., 0::2, 1::2]) + z[..., 1::2, 0::2]) + z[..., 1::2, 1::2]) * 0.25


def unpool(z, l):
    """every level-l value at the pixels of its block"""
    return np.repeat(np.repeat(z, 2 ** l, axis=-2), 2 ** l, axis=-1)


def _check_levels(H, W, weights):
    levels = len(weights)
    assert 1 <= levels <= 5 and H % 2 ** (levels - 1) == 0 and W % 2 ** (levels - 1) == 0


def iou_value(alpha, target, weights, eps=EPS):
    """loss [B] alone (for the finite differences)"""
    a = np.asarray(alpha, np.float64)
    t = np.broadcast_to(np.asarray(target, np.float64), a.shape)
    loss = np.zeros(a.shape[0])
    for l, w in enumerate(weights):
        if l:
            a, t = pool(a), pool(t)
        loss = loss + w * (1 - (a * t).sum((1, 2)) / ((a + t - a * t).sum((1, 2)) + eps))
    return loss


def iou_ref(alpha, target, weights, g=UPSTREAM, eps=EPS):
    a = np.asarray(alpha, np.float64)
    t = np.broadcast_to(np.asarray(target, np.float64), a.shape)
    _check_levels(a.shape[1], a.shape[2], weights)
    g = np.asarray(g, np.float64)[:a.shape[0]]
    loss, loss_mag = np.zeros(a.shape[0]), np.zeros(a.shape[0])
    grad, grad_mag = np.zeros(a.shape), np.zeros(a.shape)
    for l, w in enumerate(weights):
        if l:
            a, t = pool(a), pool(t)
        I = (a * t).sum((1, 2))
        Ue = (a + t - a * t).sum((1, 2)) + eps
        loss += w * (1 - I / Ue)
        loss_mag += abs(w) * (1 + I / Ue)
        k = (g * w * 0.25 ** l / Ue ** 2)[:, None, None]
        tl, I, Ue = unpool(t, l), I[:, None, None], Ue[:, None, None]
        grad += -k * (tl * Ue - I * (1 - tl))
        grad_mag += np.abs(k) * (np.abs(tl * Ue) + np.abs(I * (1 - tl)))
    return Result(loss, loss_mag, grad, grad_mag)


def _difference(images, target, mask):
    """(d [B,C,H,W], mask [B,1,H,W] or 1.0, the shape of images)"""
    x = np.asarray(images, np.float64)
    shape = x.shape
    t = np.asarray(target, np.float64)
    if x.ndim == 3:
        x, t = x[:, None], (t[:, None] if t.ndim == 3 else t[None, None])
    elif t.ndim == 3:
        t = t[None]
    m = 1.0
    if mask is not None:
        m = np.asarray(mask, np.float64)
        m = m[:, None] if m.ndim == 3 else m[None, None]
    return np.broadcast_to(m * (x - t), x.shape), m, shape


def se_value(images, target, mask, weights):
    d, _, _ = _difference(images, target, mask)
    loss = np.zeros(d.shape[0])
    for l, w in enumerate(weights):
        if l:
            d = pool(d)
        loss = loss + w * (d * d).sum((1, 2, 3))
    return loss


def se_ref(images, target, mask, weights, g=UPSTREAM):
    d, m, shape = _difference(images, target, mask)
    _check_levels(d.shape[2], d.shape[3], weights)
    g = np.asarray(g, np.float64)[:d.shape[0]][:, None, None, None]
    ad = np.abs(d)
    loss, grad, grad_mag = np.zeros(d.shape[0]), np.zeros(d.shape), np.zeros(d.shape)
    loss_mag = np.zeros(d.shape[0])
    for l, w in enumerate(weights):
        if l:
            d, ad = pool(d), pool(ad)
        s = (d * d).sum((1, 2, 3))
        loss += w * s
        loss_mag += abs(w) * s
        grad += 2 * w * g * 0.25 ** l * m * unpool(d, l)
        grad_mag += 2 * np.abs(w * g) * 0.25 ** l * np.abs(m) * unpool(ad, l)
    return Result(loss, loss_mag, grad.reshape(shape), grad_mag.reshape(shape))


@functools.lru_cache(maxsize=None)
def iou_reference(case):
    """The restatement on iou_inputs(case), computed once and shared."""
    alpha, target, weights = iou_inputs(case)
    return iou_ref(alpha, target, weights)


@functools.lru_cache(maxsize=None)
def se_reference(case):
    x, t, m, weights = se_inputs(case)
    return se_ref(x, t, m, weights)


def worst_ratio(got, ref, mag):
    """max |got - ref| / (u M) over the entries with M > 0; where M = 0 the entries must be equal."""
    got, ref, mag = (np.asarray(t, np.float64) for t in (got, ref, mag))
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.array_equal(got[zero], ref[zero]), 'entries of magnitude 0 differ'
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / (U * mag[~zero])).max())
