"""Test-side restatement of the soft silhouette (include/nr_hip.h: nr_soft_silhouette_*; DESIGN "Soft silhouettes") in
float64 NumPy: forward, Q and the analytic gradient, with the term magnitudes and the per-entry bounds of a float32 run.

  restate(faces, S, sigma, near, far, g, adds)   -> Result: alpha, Q, grad_faces, their magnitudes and bounds, the doubt share
  geometry(xy, on, S, sigma)                     the pairs' geometry and its rounding terms, also soft_render_ref's front
  sphere_faces(level, B)                         the projected icosphere of the checked cases
  worst_ratio(got, ref, bound)                   max |got - ref| / bound, 0 / 0 = 0, x / 0 = inf

The definition is the header's.  Everything is computed per (pixel, face) pair on arrays [3 segments, S*S pixels, F faces];
rows are internal (row 0 at the bottom) and flipped on the way in (g) and out (alpha, Q, the bound).

The float32 operation sequence that the bounds count (csrc/nr_soft_pair.h: soft_segment, soft_pair; csrc/nr_soft_silhouette.hip:
the two kernels), u = 2^-24, first order, every difference and sum propagated with absolute values:

  p        the pixel centre is the float32 rounding of (2 i + 1 - S) / S:                       dp = u |p|
  per segment a -> b:  e = b - a, w = p - a (a rounding each, w also dp);  dot = wx ex + wy ey;  ee = ex ex + ey ey
           ddot = 4 u (|wx ex| + |wy ey|) + u (|ex| |px| + |ey| |py|),  ee: 4 u relative
  t        = dot / ee clamped:  dt = ddot / ee + 5 u |t|, and 0 where the unclamped value misses [0, 1] by more than that
  r        = p - c as (1 - t) w + t v, v = p - b (a rounding, and dp), 1 - t a rounding:
           dr0 = u (3 (1 - t) |w| + 2 t |v| + |r| + |p|) per component, t taken as exact
  d2       = rx rx + ry ry:  dd2 = 2 |rx| dr0x + 2 |ry| dr0y + 2 u d2.  dt does not enter at first order: d d2 / dt = -2 r . e,
           which is 0 for a free t (r orthogonal to e) -- the cancellation magnitude of d2 is the |w|, |v| and |p| against a
           small |r| in dr0 --, and a clamped t is exact
  x        = s d2 (1 / sigma), 1 / sigma a float32 constant:  dx = dd2 / sigma + 2 u |x|
  1 - D    = 1 / (1 + e^x): e^x relative dx + 2 E u (expf within E ulp, E = 2 ASSUMED: no accuracy table ships with the
           toolchain), the sum D times that + u, the division u:  rel = D (dx + 2 E u) + 2 u.  A pair with x <= -17.5 has
           e^x < 2^-25 and its float32 factor is exactly 1: no rounding, its whole D is in allowance 1
  Q        the running product, one rounding per live factor; alpha = 1 - Q one more:
           dQ = Q (sum rel + n_live u + allowances) + n 2^-149,  dalpha = dQ + u alpha + 2^-52 (the restatement's own 1 - Q)
  backward per pair: G = g Q (the STORED Q: its dQ / Q enters), D = 1 / (1 + e^-x): (1 - D) (dx + 2 E u) + 2 u relative,
           C = (G D) (1 / sigma) with its sign: rel_C = dQ / Q + 4 u + rel_D;  ca = (-2 (1 - t)) C, cb = (-2 t) C, the terms
           ca r, cb r:  |term| (rel_C + 3 u) + 2 |C| (|r| dt + (1 - t | t) (dr0 + |e| dt))
  sums     one addition per pixel and entry in a lane (ceil(box pixels / 64) <= ceil(S^2 / 64) along a lane), then the six
           levels of the lane tree: gamma_adds of the sum of |terms|, adds = ceil(S^2 / 64) + 6 (`adds`: another count for
           another order, e.g. S^2 for torch's sum)

The two allowances of the issue.  (1) A pair that the kernel may leave out -- outside, d2 >= 16 sigma (the kernel's box
starts beyond 17) -- adds Q D to its pixel (taken exactly: Q (1 / (1 - D) - 1), which is Q D to first order) and the absolute
value of its gradient terms to their entries.  (2) A pair in doubt -- the second-nearest segment has another nearest point and
a d2 within 1e-4 relative, or an edge function lies within 1e-6 of its own term magnitude of 0 (a magnitude of exactly 0 is no
doubt: that edge function is 0 in every arithmetic) -- adds BOTH candidates' gradient terms to the entries they touch (the
other segment's terms; the terms with the other sign of x, i.e. with 1 - D for D).  `doubt_share` is their share of the
contributing pairs.  Forward, a pair in segment doubt needs nothing: min_k d2 is the same whichever candidate wins, within dx.
A pair in edge doubt whose side can really flip -- no edge function exactly 0, the ones not in doubt of one sign -- has its
ln(1 - D) off by |x| exactly; that goes to the bound of its own pixel's alpha and Q and nowhere else (d2 is next to 0 there).
A third allowance, for zero-area faces only, which rule (2) does not reach: two of their segments overlap, so the second-nearest
segment can have the SAME nearest point and d2 and yet hand the gradient to other vertices (on a triangle with an area this
happens only at a shared vertex, where both segments give everything to that vertex).  Which of the two wins is decided by the
last bit of d2: such a pair adds both candidates' gradient terms, as in (2); alpha is the same either way.
"""
import types

import numpy as np

import vertex_ref

U = 2.0 ** -24
EXP_ULP = 2.0       # assumed (module docstring)
TINY = 2.0 ** -149  # the spacing of float32 denormals
LIVE_X = -17.5      # below: e^x < 2^-25, the float32 factor is exactly 1
OMIT = 16.0         # a pair outside with d2 >= OMIT sigma may be left out (the kernel: beyond 17)
SEG_DOUBT = 1e-4
EDGE_DOUBT = 1e-6


def gamma(k):
    return k * U / (1.0 - k * U)


def kernel_adds(S):
    return -(-S * S // 64) + 6


class Result(object):
    pass


def geometry(xy, on, S, sigma):
    """The front that the three restatements share: xy [F,3,2] of the faces (0 where a face does not contribute), on [F],
    -> a namespace of arrays [3 segments, P = S*S pixels, F faces] or [P,F]: the segments' geometry (px, py, ex, ey, wx, wy, vx,
    vy, ee, t_raw, t, cx, cy, rx, ry, d2s, cr), the chosen segment (k, pick(a, kk=k)), the pair (d2, inside, s, x, onp), the
    chosen segment's rounding terms of the module docstring (tk, rxk, ryk, exk, eyk, eek, t_rawk, apx, apy, ddot, dt_full --
    before the clamp's exactness --, dt, dr0x, dr0y, dd2, dx), the second candidate (k2, d22, apart: it has another nearest
    point) and the edge doubt (emag, near0)."""
    c1 = (2.0 * np.arange(S) + 1 - S) / S
    px = np.tile(c1, S)[:, None]       # [P,1], P = yi * S + xi
    py = np.repeat(c1, S)[:, None]
    A = np.stack([xy[:, k] for k in range(3)])             # [3,F,2]: a of segment k
    Bv = np.stack([xy[:, (k + 1) % 3] for k in range(3)])  # b of segment k
    ax, ay, bx, by = A[:, None, :, 0], A[:, None, :, 1], Bv[:, None, :, 0], Bv[:, None, :, 1]   # [3,1,F]
    ex, ey = bx - ax, by - ay
    wx, wy = px[None] - ax, py[None] - ay                  # [3,P,F]
    dot, ee = wx * ex + wy * ey, ex * ex + ey * ey
    pos = ee > 0
    with np.errstate(all='ignore'):
        t_raw = np.where(pos, dot / np.where(pos, ee, 1.0), 0.0)
    t = np.clip(t_raw, 0.0, 1.0)
    cx, cy = ax + t * ex, ay + t * ey                     # (the nearest point: for the doubt test only)
    vx, vy = px[None] - bx, py[None] - by
    rx, ry = (1 - t) * wx + t * vx, (1 - t) * wy + t * vy
    d2s = rx * rx + ry * ry
    cr = ex * wy - ey * wx
    k = np.argmin(d2s, 0)                                  # the lowest k on a tie
    pick = lambda a, kk=None: np.take_along_axis(np.broadcast_to(a, d2s.shape), (k if kk is None else kk)[None], 0)[0]
    d2 = pick(d2s)
    inside = (cr > 0).all(0) | (cr < 0).all(0)
    s = np.where(inside, 1.0, -1.0)
    x = s * d2 / sigma
    onp = np.broadcast_to(on[None, :], x.shape)

    # ---- the chosen segment's rounding terms
    tk, rxk, ryk, exk, eyk = pick(t), pick(rx), pick(ry), pick(ex), pick(ey)
    eek, t_rawk = pick(ee), pick(t_raw)
    apx, apy = np.abs(px), np.abs(py)
    ddot = 4 * U * pick(np.abs(wx * ex) + np.abs(wy * ey)) + U * (np.abs(exk) * apx + np.abs(eyk) * apy)
    with np.errstate(all='ignore'):
        dt_full = np.where(eek > 0, ddot / np.where(eek > 0, eek, 1.0), 0.0) + 5 * U * np.abs(t_rawk)
    dt = np.where((t_rawk < -dt_full) | (t_rawk > 1 + dt_full), 0.0, dt_full)
    dr0x = U * (3 * (1 - tk) * np.abs(pick(wx)) + 2 * tk * np.abs(pick(vx)) + np.abs(rxk) + apx)
    dr0y = U * (3 * (1 - tk) * np.abs(pick(wy)) + 2 * tk * np.abs(pick(vy)) + np.abs(ryk) + apy)
    dd2 = 2 * np.abs(rxk) * dr0x + 2 * np.abs(ryk) * dr0y + 2 * U * d2
    dx = dd2 / sigma + 2 * U * np.abs(x)

    # ---- the second candidate, the edge functions next to 0
    d2_other = np.where(np.arange(3)[:, None, None] == k[None], np.inf, d2s)
    k2 = np.argmin(d2_other, 0)
    d22 = pick(d2s, k2)
    apart = np.hypot(pick(cx, k2) - pick(cx), pick(cy, k2) - pick(cy)) > 1e-12 * (1 + np.abs(pick(cx)) + np.abs(pick(cy)))
    # an edge function in doubt: within 1e-6 of its own term magnitude of 0.  A magnitude of exactly 0 (a zero-length
    # segment, a pixel on the segment's first end) is no doubt: the edge function is 0 in every arithmetic, the pair outside
    emag = np.abs(ex * wy) + np.abs(ey * wx)
    near0 = (emag > 0) & (np.abs(cr) <= EDGE_DOUBT * emag)
    return types.SimpleNamespace(
        px=px, py=py, ex=ex, ey=ey, wx=wx, wy=wy, vx=vx, vy=vy, ee=ee, t_raw=t_raw, t=t, cx=cx, cy=cy, rx=rx, ry=ry, d2s=d2s,
        cr=cr, k=k, pick=pick, d2=d2, inside=inside, s=s, x=x, onp=onp, tk=tk, rxk=rxk, ryk=ryk, exk=exk, eyk=eyk, eek=eek,
        t_rawk=t_rawk, apx=apx, apy=apy, ddot=ddot, dt_full=dt_full, dt=dt, dr0x=dr0x, dr0y=dr0y, dd2=dd2, dx=dx, k2=k2, d22=d22,
        apart=apart, emag=emag, near0=near0)


def _image(fc, S, sigma, near, far, g, adds):
    """One image: fc [F,3,3] float64, g [S,S] internal rows or None."""
    F = fc.shape[0]
    with np.errstate(all='ignore'):
        on = np.isfinite(fc).all((1, 2)) & (fc[:, :, 2] >= near).all(1) & (fc[:, :, 2] <= far).all(1)
    G = geometry(np.where(on[:, None, None], fc[:, :, :2], 0.0), on, S, sigma)
    t, rx, ry, cr, k, d2, s, x, onp = G.t, G.rx, G.ry, G.cr, G.k, G.d2, G.s, G.x, G.onp
    tk, rxk, ryk, exk, eyk, dt, dr0x, dr0y, dx = G.tk, G.rxk, G.ryk, G.exk, G.eyk, G.dt, G.dr0x, G.dr0y, G.dx
    k2, d22, apart, emag, near0 = G.k2, G.d22, G.apart, G.emag, G.near0
    pick2 = lambda a: G.pick(a, k2)
    with np.errstate(all='ignore'):
        D = np.where(onp, 1.0 / (1.0 + np.exp(-x)), 0.0)
        # Q = the product of 1 / (1 + e^x) and alpha = 1 - Q, through the logarithms: in float64 the plain product and the
        # subtraction would leave alpha no better than 2^-53 F, which is the size of the far pixels' alpha
        ln_q = -np.where(onp, np.logaddexp(0.0, x), 0.0).sum(1)
        Q, alpha = np.exp(ln_q), -np.expm1(ln_q)

    # ---- doubt
    seg_doubt = onp & apart & (d22 - d2 <= SEG_DOUBT * d22)
    edge_doubt = onp & near0.any(0)
    doubt = seg_doubt | edge_doubt
    # ... whose sign decides inside or outside: no edge function is exactly 0 and the ones not in doubt agree in sign
    can_flip = edge_doubt & ~(emag == 0).any(0) & ((near0 | (cr > 0)).all(0) | (near0 | (cr < 0)).all(0))
    # allowance 3: the overlapping segments of a zero-area face -- the same nearest point on two segments that hand its
    # gradient to different vertices
    share = lambda kk, tt: np.stack([np.where(kk == v, 1 - tt, 0.0) + np.where((kk + 1) % 3 == v, tt, 0.0) for v in range(3)])
    overlap = onp & ~apart & (d22 - d2 <= SEG_DOUBT * d22) & (np.abs(share(k, tk) - share(k2, pick2(t))).max(0) > 1e-9)
    omit = onp & (s < 0) & (d2 >= OMIT * sigma)
    live = onp & (x > LIVE_X)

    # ---- forward bound
    rel_f = np.where(live, D * (dx + 2 * EXP_ULP * U) + 2 * U, 0.0)
    with np.errstate(all='ignore'):
        left_out = np.where(omit, np.logaddexp(0.0, x), 0.0)   # -ln(1 - D) = D to first order
    n_live = live.sum(1)
    rel_Q = rel_f.sum(1) + n_live * U + np.expm1(left_out.sum(1))   # (the last: exact for the pairs left out)
    dQ = Q * rel_Q + F * TINY                          # what the gradient terms of the pixel carry as dQ / Q
    # a pair whose side can flip has ln(1 - D) off by |x| exactly (d2 is next to 0 there): the pixel's own alpha and Q only
    dQ_flip = dQ + Q * np.where(can_flip, np.abs(x), 0.0).sum(1)
    dalpha = dQ_flip + U * alpha + 2.0 ** -52          # (the last: this float64 subtraction's own rounding)

    res = Result()
    img = lambda a: a.reshape(S, S)[::-1]
    res.alpha, res.Q, res.alpha_bound, res.Q_bound = img(alpha), img(Q), img(dalpha), img(dQ_flip)
    res.pairs, res.doubt = int(onp.sum()), int(doubt.sum())
    res.d2_min = img(np.where(onp, d2, np.inf).min(1))     # the squared distance to the nearest edge of any contributing face
    res.grad = res.grad_mag = res.grad_bound = None
    if g is None:
        return res

    # ---- gradient, magnitudes, bound
    gq = (g.reshape(-1) * Q)[:, None]                      # G [P,1]
    C = gq * D * s / sigma                                 # dL/dd2
    rel_D = (1 - D) * (dx + 2 * EXP_ULP * U) + 2 * U
    with np.errstate(all='ignore'):
        rel_C = np.where(Q > 0, dQ / np.where(Q > 0, Q, 1.0), 0.0)[:, None] + 4 * U + rel_D
    grad, mag, bound = np.zeros((F, 3, 3)), np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
    absC = np.abs(C)
    under = 8 * TINY * (1 + np.abs(g).max()) * (1 + 1 / sigma) * (1 + max(np.abs(rxk).max(), np.abs(ryk).max()))
    fidx = np.broadcast_to(np.arange(F)[None, :], x.shape)

    def scatter(dst, vert, comp, val):
        np.add.at(dst, (fidx.reshape(-1), vert.reshape(-1), comp), val.reshape(-1))

    va, vb = k, (k + 1) % 3
    for comp, (r, dr0, e) in enumerate(((rxk, dr0x, exk), (ryk, dr0y, eyk))):
        ta, tb = -2 * (1 - tk) * r * C, -2 * tk * r * C
        drf = dr0 + np.abs(e) * dt
        ea = np.abs(ta) * (rel_C + 3 * U) + 2 * absC * (np.abs(r) * dt + (1 - tk) * drf) + under
        eb = np.abs(tb) * (rel_C + 3 * U) + 2 * absC * (np.abs(r) * dt + tk * drf) + under
        ea = np.where(onp, ea, 0.0) + np.where(omit | doubt | overlap, np.abs(ta), 0.0)
        eb = np.where(onp, eb, 0.0) + np.where(omit | doubt | overlap, np.abs(tb), 0.0)
        scatter(grad, va, comp, ta)
        scatter(grad, vb, comp, tb)
        scatter(mag, va, comp, np.abs(ta))
        scatter(mag, vb, comp, np.abs(tb))
        scatter(bound, va, comp, ea)
        scatter(bound, vb, comp, eb)
    # the other candidates of the pairs in doubt
    C_flip = gq * (1 - D) / sigma                          # |C| with the other sign of x
    t2, va2, vb2 = pick2(t), k2, (k2 + 1) % 3
    for comp, (r, r2) in enumerate(((rxk, pick2(rx)), (ryk, pick2(ry)))):
        z = np.zeros_like(r)
        scatter(bound, va, comp, np.where(edge_doubt, np.abs(2 * (1 - tk) * r * C_flip), z))
        scatter(bound, vb, comp, np.where(edge_doubt, np.abs(2 * tk * r * C_flip), z))
        big = np.maximum(absC, np.where(edge_doubt, np.abs(C_flip), 0.0))
        scatter(bound, va2, comp, np.where(seg_doubt | overlap, np.abs(2 * (1 - t2) * r2) * big, z))
        scatter(bound, vb2, comp, np.where(seg_doubt | overlap, np.abs(2 * t2 * r2) * big, z))
    res.grad, res.grad_mag, res.grad_bound = grad, mag, bound + gamma(adds) * mag
    return res


def restate(faces, S, sigma, near=0.1, far=100.0, g=None, adds=None):
    """faces [B,F,3,3] (float32 values), g [B,S,S] the upstream gradient of alpha (row 0 the top row) or None -> Result with
    alpha, Q, alpha_bound, Q_bound, d2_min [B,S,S] (row 0 the top row), grad, grad_mag, grad_bound [B,F,3,3] (with g), pairs, doubt
    (the numbers of contributing pairs and of pairs in doubt per image) and doubt_share."""
    fc = np.asarray(faces, np.float64)
    adds = kernel_adds(S) if adds is None else adds
    per = [_image(fc[b], S, float(sigma), near, far, None if g is None else np.asarray(g, np.float64)[b][::-1], adds)
           for b in range(fc.shape[0])]
    out = Result()
    for name in ('alpha', 'Q', 'alpha_bound', 'Q_bound', 'd2_min') + (() if g is None else ('grad', 'grad_mag', 'grad_bound')):
        setattr(out, name, np.stack([getattr(r, name) for r in per]))
    out.pairs, out.doubt = [r.pairs for r in per], [r.doubt for r in per]
    out.doubt_share = max([r.doubt / r.pairs for r in per if r.pairs] or [0.0])
    return out


def worst_ratio(got, ref, bound):
    """max over the entries of |got - ref| / bound, 0 / 0 = 0 and x / 0 = inf (a NaN counts as inf)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    bound = np.broadcast_to(bound, d.shape)
    with np.errstate(all='ignore'):
        r = np.where(d == 0, 0.0, d / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the checked cases

def _rotation():
    a, b = 0.37, 0.23
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return rx @ ry


def project(vertices, distance=2.732, angle=30.0):
    """look_at from (0, 0, -distance) at the origin, then the perspective of viewing angle `angle`: [.., 3] -> [.., 3]."""
    v = np.asarray(vertices, np.float64)
    z = v[..., 2] + distance
    w = np.tan(np.radians(angle))
    return np.stack((v[..., 0] / z / w, v[..., 1] / z / w, z), -1)


def sphere_faces(level, B=1, seed=0, radius=0.8):
    """[B,F,3,3] float32: icosphere(level) of radius 0.8, rotated 0.37 rad about y then 0.23 about x, projected; the images
    after the first are jittered per vertex (per-image geometry)."""
    v, f = vertex_ref.icosphere(level)
    v = radius * v @ _rotation().T
    rng = np.random.default_rng(700 + seed)
    vb = np.stack([v + (rng.normal(scale=0.03, size=v.shape) if b else 0.0) for b in range(B)])
    return project(vb)[:, f].astype(np.float32)
