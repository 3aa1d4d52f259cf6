"""Test-side restatement of soft colour rendering (include/nr_hip.h: nr_soft_render_*, nr_soft_corners_*; DESIGN "Soft colour
rendering") in float64 NumPy: forward, Q and the ANALYTIC gradient to faces (x, y, z) and colours -- one per face, colors
[B|1,F,3], or one per corner, [B|1,F,3,3] --, with the term magnitudes and the per-entry bounds of a float32 run.

  restate(faces, colors, S, sigma, gamma, near, far, eps, background, g, adds, variant)  -> Result
  hard_image(faces, colors, S, background)   the hard rasterizer's definition of a corner-colour scene, float64 (no anti-aliasing)
  sphere_faces, worst_ratio, gamma_k (soft_ref's gamma), kernel_adds                     from tests/soft_ref.py

The definition is the header's.  Everything is computed per (pixel, face) pair on arrays [3, S*S pixels, F faces]; rows are
internal (row 0 at the bottom) and flipped on the way in (g) and out (rgba, Q, the mask, the bounds).

Masked pixels.  A pair in cutoff doubt (outside, |d2 / (17 sigma) - 1| < 1e-4) or in edge doubt (soft_ref's rule: an edge
function within 1e-6 of its own term magnitude of 0) may be taken in one arithmetic and not in the other, or change sides,
which changes the normaliser of its whole pixel.  Such a pixel is found from the inputs alone (`mask`); restate() sets the
incoming gradient to 0 there (`g`, to be handed to the implementation) and the tests skip its forward comparison.
`masked_share`: masked pixels / pixels with at least one taken pair.

The float32 operation sequence that the bounds count (csrc/nr_soft_pair.h, csrc/nr_soft_render.hip), u = 2^-24, first order,
every difference and sum propagated with absolute values.  p, e, w, dot, ee, t, r, d2, x and their dp, ddot, dt, dr0, dd2, dx
are soft_ref.geometry's.  Then, for one colour per face:

  c_j      = ex wy - ey wx:  dc_j = 3 u (|ex wy| + |ey wx|) + u (|ex| |py| + |ey| |px|) + u |c_j|
  A        = (c_0 + c_1) + c_2 (one sign inside):  dA = sum dc_j + 2 u |A|;  1 / A: dA / |A| + u relative
  lambda   inside c_j (1 / A):  dl = dc_j / |A| + lambda (dA / |A| + 2 u);  outside 1 - t: dt + u (1 - t), t: dt
  1 / z_k  a rounding;  iz = (l0 iz0 + l1 iz1) + l2 iz2, positive terms:  diz = sum dl_k / z_k + 4 u iz
  zp       = 1 / iz:  dzp = zp (diz / iz + u);  zn = (far - zp) (1 / (far - near)), far and the reciprocal float32 constants:
           dzn = (dzp + u |far|) / (far - near) + 3 u |zn|
  m        the maximum of the float32 zn themselves (and of the float32 eps): one float, common to every weight of the
           pixel.  rgb and W = w / Z are ratios of weights: a common shift of m cancels EXACTLY, so m counts as exact and the
           weights carry their own errors only
  w_f      = D expf((zn - m) (1 / gamma)):  the exponent  darg = dzn / gamma + 3 u |arg| -- the amplification of the depth's
           rounding by 1 / gamma is inherent to the definition --, expf within E ulp (E = 2 ASSUMED, as in soft_ref), D as in
           soft_ref's backward: rel_D = (1 - D) (dx + 2 E u) + 2 u;  rho_f = rel_D + darg + 2 E u + u
  w_b      = expf((eps - m) (1 / gamma)):  rho_b = u |eps| / gamma + 3 u |arg_b| + 2 E u
  Z, rgb   n + 1 terms in order, then the division:
           drgb_c = sum_i (w_i / Z) |C_ic - rgb_c| rho_i + gamma(n + 2) (|rgb_c| + sum_i (w_i / Z) |C_ic|)
                    + 2 u sum_i (w_i / Z) |C_ic| + u |rgb_c|           (the products w C and the background's rounding)
  Q, alpha as soft_ref over the taken pairs (nothing is left out: the cutoff is the definition's)
  backward per taken pair; the kernel recomputes the forward's own w_f bit for bit and divides by the STORED Z:
           rel_W = rho_f + sum_i (w_i / Z) rho_i + gamma(n + 2) + u
           h = (gr (Cr - R) + gg (Cg - G)) + gb (Cb - B), the STORED rgb:  dh = sum_c |g_c| drgb_c + 4 u sum_c |g_c| |C_c - rgb_c|
           hW = h W:  dhW = dh W + |hW| (rel_W + u);  the colour terms W g_c: rel_W + u relative
           dL/dx = hW (1 - D) + (ga Q) D: the first  dhW (1 - D) + |.| (rel_(1-D) + u), the second |.| (dQ / Q + rel_D + 2 u),
           the sum u (|.| + |.|);  C = dL/dx (1 / sigma) with its sign: two more roundings
           diz = ((hW (1 / gamma)) (1 / (far - near))) (zp zp):  ddiz = dhW zp^2 / (gamma (far - near)) + |diz| (6 u + 2 dzp / zp)
           z:      -(diz lambda_k) (iz_k iz_k):  ddiz lambda_k / z_k^2 + |diz| dl_k / z_k^2 + 5 u |term|
           free t: T = (diz (iz_b - iz_a)) / ee:  dT = ddiz |iz_b - iz_a| / ee + |diz| u (iz_a + iz_b) / ee + 7 u |T|; the terms
                   -+T r and -(1 - t | t) T e with dr = dr0 + |e| dt, dt and a rounding of 1 - t
           inside: q_j = (diz (1 / A)) (iz_(j+2) - iz):  dq_j = (ddiz |X_j| + |diz| (d iz + u iz_(j+2) + u |X_j|)) / |A|
                   + |q_j| (dA / |A| + 3 u);  the terms q_j (p - v) with d(p - v) = u (|p| + |p - v|)
           a pixel's value of an entry is put together from these with at most six roundings: 6 u of the sum of |terms|
  sums     as soft_ref: gamma(adds) of the sum of |terms|, adds = ceil(S^2 / 64) + 6 for the kernel.

Doubt, local to the face's own gradient entries (`doubt_share`, of the taken pairs): a pair in segment doubt (soft_ref's rule)
may hold the OTHER candidate's terms instead of its own, so it adds the magnitudes of both: its own d2 and t terms (and z
terms, outside) and the other candidate's; an outside pair whose unclamped t lies within dt of 0 or 1 (the clamp can go either
way) adds the free-t terms, present or not.  Near the end of an edge the two candidates are a free t on one segment and a
clamped t on the next: the same nearest point within the doubt, but the whole free-t term apart.  Forward, an outside pair in
segment doubt adds |iz of the other candidate's nearest point - iz| to d iz: continuous across the tie, but more than a
rounding inside the doubt band.

What the corner colours add to the float32 operation sequence (csrc/nr_soft_render.hip, the <true> instantiations):

  u_k      = lambda_k iz_k (pair_depth's own products):  du_k = dl_k / z_k + 2 u u_k
  mu_k     = u_k zp:  dmu_k = du_k zp + u_k dzp + u mu_k
  C(p)_c   = (mu_0 C_0c + mu_1 C_1c) + mu_2 C_2c:  dC_c = sum_k dmu_k |C_kc| + 3 u sum_k mu_k |C_kc|; an outside pair in segment
           doubt adds |C(p) of the other candidate's nearest point - C(p)|, as d iz takes |iz2 - iz|
  rgb      the flat drgb_c with C_ic = C_i(p)_c, plus sum_i (w_i / Z) dC_ic
  backward per taken pair: h = (gr (C(p)_r - R) + gg (C(p)_g - G)) + gb (C(p)_b - B):  dh gains sum_c |g_c| dC_c
           colours: (W g_c) mu_k:  |.| (rel_W + 2 u) + |W g_c| dmu_k
           e_k = (gr (C_kr - C(p)_r) + gg (..)) + gb (..):  de_k = sum_c |g_c| dC_c + 4 u sum_c |g_c| |C_kc - C(p)_c|
           E_k = (W zp) e_k:  dE_k = W zp de_k + |E_k| (rel_W + dzp / zp + 2 u)
           z:      -((diz + E_k) lambda_k) (iz_k iz_k):  (ddiz + dE_k + u (|diz| + |E_k|)) lambda_k / z_k^2
                   + (|diz| + |E_k|) dl_k / z_k^2 + 5 u (|diz| + |E_k|) lambda_k / z_k^2
           free t: T = (diz (iz_b - iz_a) + (E_b iz_b - E_a iz_a)) / ee:  the flat dT of the first product, plus
                   (dE_b iz_b + dE_a iz_a + 3 u (|E_b| iz_b + |E_a| iz_a)) / ee, plus 7 u of the magnitude
                   Tmag = (|diz (iz_b - iz_a)| + |E_b| iz_b + |E_a| iz_a) / ee, which stands where |T| stood
           inside: q_j = (diz (1 / A)) (iz_v - iz) + (E_v iz_v) (1 / A), v = (j + 2) mod 3:  the flat dq_j of the first
                   term, plus dE_v iz_v / |A| + |second| (dA / |A| + 4 u) + u (|first| + |second|); |first| + |second| stands
                   where |q_j| stood
  Every magnitude (`_mag`) counts the parts of a cancelling sum separately, as above.

  Not the flat formulas with E = 0, so _image asks the layout there: the u (|diz| + |E_k|) of z and the u (|first| + |second|)
  of q_j (the additions diz + E_k and first + second), the colour bound (rel_W + 2 u and dmu_k), the underflow scale's 1 / z.

Doubt, with corner colours: a pair in segment doubt adds the other candidate's terms with ITS free-t magnitude (E at its two
ends); its z terms with (|diz| + |E_k| + dE_k).  Near the end of an edge the two candidates' nearest points coincide within
the doubt, so do their colours: what is apart is the free-t term, d_b iz_b - d_a iz_a, whole.

`variant`: a deliberately wrong restatement for the sensitivity tests.  Either layout: 'no_z' (z gradients zeroed),
'no_background' (w_b left out of Z), 'no_1mD' (the 1 - D factor dropped from dL/dx).  Corner colours only (ValueError for a
flat colour): 'affine' (mu = lambda: screen-space interpolation), 'rotated' (corner k takes the colour of corner k + 1),
'no_colour_path' (every E_k = 0: the colour's way into x, y, z cut).
"""
import numpy as np

import soft_ref
from soft_ref import EDGE_DOUBT, EXP_ULP, LIVE_X, SEG_DOUBT, TINY, U, kernel_adds, sphere_faces, worst_ratio  # noqa: F401

gamma_k = soft_ref.gamma
REACH = 17.0
CUT_DOUBT = 1e-4
CORNER_VARIANTS = ('affine', 'rotated', 'no_colour_path')


class Result(object):
    pass


def _image(fc, col, S, sigma, gam, near, far, eps, bg, g, adds, variant):
    """One image: fc [F,3,3], col [F,3 rgb] or [F,3 corners,3 rgb] float64, g [4,S,S] internal rows or None."""
    F = fc.shape[0]
    rng = far - near
    corners = col.ndim == 3
    if variant == 'rotated':
        col = col[:, (1, 2, 0)]
    with np.errstate(all='ignore'):
        area = (fc[:, 1, 0] - fc[:, 0, 0]) * (fc[:, 2, 1] - fc[:, 0, 1]) - (fc[:, 2, 0] - fc[:, 0, 0]) * (fc[:, 1, 1] - fc[:, 0, 1])
        on = np.isfinite(fc).all((1, 2)) & (fc[:, :, 2] >= near).all(1) & (fc[:, :, 2] <= far).all(1) & (area != 0)
    izv = 1.0 / np.where(on[:, None], fc[:, :, 2], 1.0)      # [F,3]
    G = soft_ref.geometry(np.where(on[:, None, None], fc[:, :, :2], 0.0), on, S, sigma)
    ex, ey, wx, wy, ee, t, rx, ry, cr, k, pick = G.ex, G.ey, G.wx, G.wy, G.ee, G.t, G.rx, G.ry, G.cr, G.k, G.pick
    d2, inside, s, x, onp, shape = G.d2, G.inside, G.s, G.x, G.onp, G.d2s.shape
    tk, rxk, ryk, exk, eyk, eek, t_rawk, apx, apy = G.tk, G.rxk, G.ryk, G.exk, G.eyk, G.eek, G.t_rawk, G.apx, G.apy
    dt_full, dt, dr0x, dr0y, dx, k2, d22 = G.dt_full, G.dt, G.dr0x, G.dr0y, G.dx, G.k2, G.d22
    taken = onp & (inside | (d2 <= REACH * sigma))

    # ---- depth
    role_a = [k == j for j in range(3)]
    role_b = [(k + 1) % 3 == j for j in range(3)]
    share = [np.where(role_a[j], 1 - tk, 0.0) + np.where(role_b[j], tk, 0.0) for j in range(3)]
    Asum = cr.sum(0)
    As = np.where(inside, Asum, 1.0)
    src = (1, 2, 0)   # lambda_j = c_src[j] / A
    lam = [np.where(inside, cr[src[j]] / As, share[j]) for j in range(3)]
    dc = 3 * U * (np.abs(ex * wy) + np.abs(ey * wx)) + U * (np.abs(ex) * apy[None] + np.abs(ey) * apx[None]) + U * np.abs(cr)
    dA = dc.sum(0) + 2 * U * np.abs(Asum)
    dlam = [np.where(inside, dc[src[j]] / np.abs(As) + np.abs(lam[j]) * (dA / np.abs(As) + 2 * U),
                     np.where(role_a[j], dt + U * (1 - tk), 0.0) + np.where(role_b[j], dt, 0.0)) for j in range(3)]
    izj = [izv[None, :, j] for j in range(3)]
    uj = [lam[j] * izj[j] for j in range(3)]
    iz = uj[0] + uj[1] + uj[2]
    d_iz = dlam[0] * izj[0] + dlam[1] * izj[1] + dlam[2] * izj[2] + 4 * U * iz
    # segment doubt, outside: the other candidate's nearest point has another depth
    share2 = [np.where(k2 == j, 1 - pick(t, k2), 0.0) + np.where((k2 + 1) % 3 == j, pick(t, k2), 0.0) for j in range(3)]
    differ = np.max([np.abs(share[j] - share2[j]) for j in range(3)], 0) > 1e-9
    seg_doubt = taken & (d22 - d2 <= SEG_DOUBT * d22) & (G.apart | differ)
    iz2 = share2[0] * izj[0] + share2[1] * izj[1] + share2[2] * izj[2]
    d_iz = d_iz + np.where(seg_doubt & ~inside, np.abs(iz2 - iz), 0.0)
    zp = 1.0 / iz
    dzp = zp * (d_iz / iz + U)
    zn = (far - zp) / rng
    dzn = (dzp + U * abs(far)) / rng + 3 * U * np.abs(zn)

    # ---- the colour at the pixel, Cp[channel]: the face's own, or the corners' with the weights mu_k
    if corners:
        mu = lam if variant == 'affine' else [uj[j] * zp for j in range(3)]
        dmu = [(dlam[j] * izj[j] + 2 * U * np.abs(uj[j])) * zp + np.abs(uj[j]) * dzp + U * np.abs(mu[j]) for j in range(3)]
        ck = [[col[None, :, j, c] for c in range(3)] for j in range(3)]           # ck[corner][channel]: [1,F]
        Cp = [mu[0] * ck[0][c] + mu[1] * ck[1][c] + mu[2] * ck[2][c] for c in range(3)]   # [P,F]
        zp2 = 1.0 / iz2
        Cp2 = [sum(share2[j] * izj[j] * zp2 * ck[j][c] for j in range(3)) for c in range(3)]
        dCp = [sum(dmu[j] * np.abs(ck[j][c]) + 3 * U * np.abs(mu[j] * ck[j][c]) for j in range(3))
               + np.where(seg_doubt & ~inside, np.abs(Cp2[c] - Cp[c]), 0.0) for c in range(3)]
    else:
        Cp, dCp = [col[None, :, c] for c in range(3)], [0.0] * 3                  # (an input: no rounding of its own)

    # ---- aggregation
    with np.errstate(all='ignore'):
        D = np.where(taken, 1.0 / (1.0 + np.exp(-x)), 0.0)
        oneD = np.where(taken, 1.0 / (1.0 + np.exp(x)), 0.0)
        m = np.maximum(eps, np.where(taken, zn, -np.inf).max(1))              # [P]
        arg = np.where(taken, (zn - m[:, None]) / gam, 0.0)
        w = np.where(taken, D * np.exp(arg), 0.0)
        arg_b = (eps - m) / gam
        wb = np.exp(arg_b)
        Z = (0.0 if variant == 'no_background' else wb) + w.sum(1)
        rgb = np.stack([(wb * bg[c] + (w * Cp[c]).sum(1)) / Z for c in range(3)])   # [3,P]
        ln_q = -np.where(taken, np.logaddexp(0.0, x), 0.0).sum(1)
        Q, alpha = np.exp(ln_q), -np.expm1(ln_q)
        wn, wbn = w / Z[:, None], wb / Z
    n = taken.sum(1)
    rel_D = (1 - D) * (dx + 2 * EXP_ULP * U) + 2 * U
    rel_1mD = D * (dx + 2 * EXP_ULP * U) + 2 * U
    rho = np.where(taken, rel_D + dzn / gam + 3 * U * np.abs(arg) + 2 * EXP_ULP * U + U, 0.0)
    rho_b = U * abs(eps) / gam + 3 * U * np.abs(arg_b) + 2 * EXP_ULP * U
    gsum = gamma_k(n + 2)
    cmax = 1 + np.abs(col).max() + max(np.abs(bg))
    scale = (1 + 1 / sigma) * (1 + 1 / gam) * (1 + 1 / abs(rng)) * (1 + izv.max() ** 2) * cmax
    if corners:
        scale = scale * (1 + 1 / izv.min())
    with np.errstate(all='ignore'):
        tiny_f = 2.0 ** -126 * (n + 1) / Z * cmax
    drgb = []
    for c in range(3):
        cmag = (wn * np.abs(Cp[c])).sum(1) + wbn * abs(bg[c])
        drgb.append((wn * np.abs(Cp[c] - rgb[c][:, None]) * rho).sum(1) + wbn * np.abs(bg[c] - rgb[c]) * rho_b
                    + (wn * dCp[c]).sum(1) + gsum * (np.abs(rgb[c]) + cmag) + 2 * U * cmag + U * np.abs(rgb[c]) + tiny_f)
    drgb = np.stack(drgb)
    rho_bar = (wn * rho).sum(1) + wbn * rho_b + gsum
    live = taken & (x > LIVE_X)
    rel_f = np.where(live, rel_1mD, 0.0)
    dQ = Q * (rel_f.sum(1) + live.sum(1) * U) + F * TINY
    dalpha = dQ + U * alpha + 2.0 ** -52

    # ---- masked pixels and doubt
    cut_doubt = onp & ~inside & (np.abs(d2 / (REACH * sigma) - 1) < CUT_DOUBT)
    edge_doubt = onp & G.near0.any(0)
    mask = (cut_doubt | edge_doubt).any(1)                                    # [P]
    outside = taken & ~inside
    near_clamp = outside & (eek > 0) & (np.minimum(np.abs(t_rawk), np.abs(t_rawk - 1)) <= dt_full)
    doubt = (seg_doubt | near_clamp) & ~mask[:, None]

    res = Result()
    img = lambda a: a.reshape(a.shape[:-1] + (S, S))[..., ::-1, :]
    res.rgba, res.rgba_bound = img(np.concatenate((rgb, alpha[None]))), img(np.concatenate((drgb, dalpha[None])))
    res.Q, res.mask = img(Q), img(mask)
    res.edge_d2 = img(np.where(onp, d2, np.inf).min(1))                       # the squared distance to the nearest edge of any face
    res.pairs, res.doubt = int(taken.sum()), int(doubt.sum())
    res.masked, res.with_pair = int(mask.sum()), int(taken.any(1).sum())
    if g is None:
        return res

    # ---- gradient, magnitudes, bound
    g = np.where(mask[None], 0.0, g.reshape(4, -1))                           # [4,P]
    res.g = img(g)
    gc = [g[c][:, None] for c in range(3)]
    ga = g[3][:, None]
    dev = [Cp[c] - rgb[c][:, None] for c in range(3)]
    h = gc[0] * dev[0] + gc[1] * dev[1] + gc[2] * dev[2]
    hmag = sum(np.abs(gc[c] * dev[c]) for c in range(3))
    gdC = sum(np.abs(gc[c]) * dCp[c] for c in range(3))
    dh = sum(np.abs(gc[c]) * drgb[c][:, None] for c in range(3)) + gdC + 4 * U * hmag
    W = wn
    rel_W = rho + rho_bar[:, None] + U
    hW = h * W
    dhW = dh * W + np.abs(hW) * (rel_W + U)
    under = 64 * TINY * (1 + np.abs(g).max()) * scale * (1 + max(np.abs(rxk).max(), np.abs(ryk).max()))
    t1v = hW if variant == 'no_1mD' else hW * oneD
    t2v = ga * Q[:, None] * D
    with np.errstate(all='ignore'):
        relQ = np.where(Q > 0, dQ / np.where(Q > 0, Q, 1.0), 0.0)[:, None]
    dt1 = dhW * oneD + np.abs(t1v) * (rel_1mD + U)
    dt2 = np.abs(t2v) * (relQ + rel_D + 2 * U)
    C = (t1v + t2v) * s / sigma
    Cmag = (np.abs(t1v) + np.abs(t2v)) / sigma
    dC = (dt1 + dt2 + U * (np.abs(t1v) + np.abs(t2v))) / sigma + 2 * U * Cmag
    dz_ = np.where(taken, hW / gam / rng * zp * zp, 0.0)                      # dL/d iz through zn
    ddz = np.where(taken, dhW * zp * zp / (gam * abs(rng)) + np.abs(dz_) * (6 * U + 2 * dzp / zp), 0.0)
    # E_k: what corner k's colour adds to dL/d iz; a flat colour adds an exact 0, and every term below that carries an E is
    # the flat term plus exact zeros.  Where the corner BOUND is not the flat one plus zeros, the layout is asked
    if corners:
        Wz = np.where(taken, W * zp, 0.0)
        ek = [sum(gc[c] * (ck[j][c] - Cp[c]) for c in range(3)) for j in range(3)]
        ekmag = [sum(np.abs(gc[c] * (ck[j][c] - Cp[c])) for c in range(3)) for j in range(3)]
        E = [np.zeros_like(Wz) if variant == 'no_colour_path' else Wz * ek[j] for j in range(3)]
        dE = [np.where(taken, Wz * (gdC + 4 * U * ekmag[j]) + np.abs(Wz * ek[j]) * (rel_W + dzp / zp + 2 * U), 0.0) for j in range(3)]
        Eabs = [np.abs(Wz * ek[j]) for j in range(3)]
    else:
        E = dE = Eabs = [np.zeros(shape[1:])] * 3

    grad, mag, bound = np.zeros((F, 3, 3)), np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
    ones = np.ones(shape)
    rot = lambda a: [a[1], a[2], a[0]]
    iza, izb = pick(np.stack(izj) * ones), pick(np.stack(rot(izj)) * ones)
    Ea, Eb = pick(np.stack(E)), pick(np.stack(rot(E)))
    Eaa, Eba = pick(np.stack(Eabs)), pick(np.stack(rot(Eabs)))
    dEa, dEb = pick(np.stack(dE)), pick(np.stack(rot(dE)))
    free = outside & (tk > 0) & (tk < 1)
    ees = np.where(eek > 0, eek, 1.0)
    with np.errstate(all='ignore'):
        ok = outside & (eek > 0)
        Tany = np.where(ok, (dz_ * (izb - iza) + (Eb * izb - Ea * iza)) / ees, 0.0)
        Tanymag = np.where(ok, (np.abs(dz_ * (izb - iza)) + Eba * izb + Eaa * iza) / ees, 0.0)
        dT = np.where(free, (ddz * np.abs(izb - iza) + np.abs(dz_) * U * (iza + izb)
                             + dEb * izb + dEa * iza + 3 * U * (Eba * izb + Eaa * iza)) / ees + 7 * U * Tanymag, 0.0)
    T = np.where(free, Tany, 0.0)
    Tmag = np.where(free, Tanymag, 0.0)
    # inside: q_j = dL/dc_j, c_j weighs vertex v = (j + 2) mod 3
    X = [izj[(j + 2) % 3] - iz for j in range(3)]
    it = inside & taken
    q1 = [np.where(it, dz_ * X[j] / As, 0.0) for j in range(3)]
    qs = [np.where(it, E[(j + 2) % 3] * izj[(j + 2) % 3] / As, 0.0) for j in range(3)]
    qsa = [np.where(it, Eabs[(j + 2) % 3] * izj[(j + 2) % 3] / np.abs(As), 0.0) for j in range(3)]
    q = [q1[j] + qs[j] for j in range(3)]
    qmag = [np.abs(q1[j]) + qsa[j] for j in range(3)]
    dq = [np.where(it, (ddz * np.abs(X[j]) + np.abs(dz_) * (d_iz + U * izj[(j + 2) % 3] + U * np.abs(X[j]))) / np.abs(As)
                   + np.abs(q1[j]) * (dA / np.abs(As) + 3 * U), 0.0) for j in range(3)]
    if corners:   # (the second product, and the addition of the two: not in the flat bound)
        dq = [np.where(it, dq[j] + dE[(j + 2) % 3] * izj[(j + 2) % 3] / np.abs(As) + qsa[j] * (dA / np.abs(As) + 4 * U)
                       + U * qmag[j], 0.0) for j in range(3)]
    # the other candidate of a pair in segment doubt
    t2k, ee2 = pick(t, k2), pick(ee, k2)
    iza2, izb2 = pick(np.stack(izj) * ones, k2), pick(np.stack(rot(izj)) * ones, k2)
    Ea2 = pick(np.stack(Eabs), k2) + pick(np.stack(dE), k2)
    Eb2 = pick(np.stack(rot(Eabs)), k2) + pick(np.stack(rot(dE)), k2)
    with np.errstate(all='ignore'):
        T2 = np.where(outside & (ee2 > 0) & (t2k > 0) & (t2k < 1),
                      (np.abs(dz_ * (izb2 - iza2)) + Eb2 * izb2 + Ea2 * iza2) / np.where(ee2 > 0, ee2, 1.0), 0.0)
    for j in range(3):
        any_role = role_a[j] | role_b[j]
        sgn = np.where(role_a[j], -1.0, 0.0) + np.where(role_b[j], 1.0, 0.0)
        ja, jb = (j + 2) % 3, (j + 1) % 3   # x: q_ja P_ja.y - q_j P_jb.y;  y: q_j P_jb.x - q_ja P_ja.x
        for comp, (r, dr0, e, r2, e2) in enumerate(((rxk, dr0x, exk, pick(rx, k2), pick(ex, k2)),
                                                    (ryk, dr0y, eyk, pick(ry, k2), pick(ey, k2)))):
            drf = dr0 + np.abs(e) * dt
            # d2
            v1 = -2 * share[j] * r * C
            m1 = 2 * share[j] * np.abs(r) * Cmag
            e1 = 2 * share[j] * np.abs(r) * dC + 3 * U * m1 + 2 * Cmag * (np.where(any_role, np.abs(r) * dt, 0.0) + share[j] * drf)
            # a free t
            v2 = sgn * T * r - share[j] * T * e
            m2 = np.abs(sgn) * Tmag * np.abs(r) + share[j] * Tmag * np.abs(e)
            e2_ = np.abs(sgn) * (dT * np.abs(r) + Tmag * drf) + share[j] * (dT + 2 * U * Tmag) * np.abs(e) \
                + np.abs(sgn) * Tmag * dt * np.abs(e)
            # inside
            if comp == 0:
                Pa, Pb, sa, sb = wy[ja], wy[jb], 1.0, -1.0
                pa_abs = apy
            else:
                Pa, Pb, sa, sb = wx[ja], wx[jb], -1.0, 1.0
                pa_abs = apx
            v3 = sa * q[ja] * Pa + sb * q[j] * Pb
            m3 = qmag[ja] * np.abs(Pa) + qmag[j] * np.abs(Pb)
            e3 = dq[ja] * np.abs(Pa) + dq[j] * np.abs(Pb) + qmag[ja] * U * (pa_abs + np.abs(Pa)) \
                + qmag[j] * U * (pa_abs + np.abs(Pb)) + U * m3
            mm = m1 + m2 + m3
            err = np.where(taken, e1 + e2_ + e3 + 6 * U * mm + under, 0.0)
            # in doubt: the float32 run may hold the other candidate's terms INSTEAD of these -- both are added
            err = err + np.where(doubt & seg_doubt, m1 + m2 + 2 * share2[j] * np.abs(r2) * Cmag + T2 * (np.abs(r2) + np.abs(e2)), 0.0)
            err = err + np.where(doubt & near_clamp, m2 + np.where(any_role, Tanymag * (np.abs(r) + np.abs(e)), 0.0), 0.0)
            grad[:, j, comp] = (v1 + v2 + v3).sum(0)
            mag[:, j, comp] = mm.sum(0)
            bound[:, j, comp] = err.sum(0)
        # z
        sq = izj[j] * izj[j]
        dk, dkmag = dz_ + E[j], np.abs(dz_) + Eabs[j]
        vz = -(dk * lam[j]) * sq
        vzmag = dkmag * np.abs(lam[j]) * sq
        ddk = ddz + dE[j] + U * dkmag if corners else ddz   # (the addition diz + E_k: not in the flat bound)
        ez = np.where(taken, ddk * np.abs(lam[j]) * sq + dkmag * dlam[j] * sq + 5 * U * vzmag + under, 0.0)
        ez = ez + np.where(doubt & seg_doubt & outside, vzmag + (dkmag + dE[j]) * share2[j] * sq, 0.0)
        grad[:, j, 2] = 0.0 if variant == 'no_z' else vz.sum(0)
        mag[:, j, 2] = vzmag.sum(0)
        bound[:, j, 2] = ez.sum(0)
    gcol, gcol_mag, gcol_bound = np.zeros(col.shape), np.zeros(col.shape), np.zeros(col.shape)
    for c in range(3):
        Wg = W * gc[c]
        if not corners:
            gcol[:, c], gcol_mag[:, c] = Wg.sum(0), np.abs(Wg).sum(0)
            gcol_bound[:, c] = np.where(taken, np.abs(Wg) * (rel_W + U) + under, 0.0).sum(0)
            continue
        for j in range(3):
            jj = (j + 1) % 3 if variant == 'rotated' else j    # (back to the caller's corner order)
            v = Wg * mu[j]
            gcol[:, jj, c], gcol_mag[:, jj, c] = v.sum(0), np.abs(v).sum(0)
            e = np.abs(v) * (rel_W + 2 * U) + np.abs(Wg) * dmu[j] + under
            # (an outside pair in segment doubt may weigh the corners as the other candidate does)
            e = e + np.where(doubt & seg_doubt & outside, np.abs(v) + np.abs(Wg) * share2[j] * izj[j] * zp2, 0.0)
            gcol_bound[:, jj, c] = np.where(taken, e, 0.0).sum(0)
    ga_ = gamma_k(adds)
    res.grad_faces, res.grad_faces_mag, res.grad_faces_bound = grad, mag, bound + ga_ * mag
    res.grad_colors, res.grad_colors_mag, res.grad_colors_bound = gcol, gcol_mag, gcol_bound + ga_ * gcol_mag
    return res


def restate(faces, colors, S, sigma, gamma, near=0.1, far=100.0, eps=1e-3, background=(0.0, 0.0, 0.0), g=None, adds=None,
            variant=None):
    """faces [B,F,3,3], colors [B,F,3] or [1,F,3] -- or [B,F,3,3] or [1,F,3,3]: face, corner, rgb -- (float32 values), g
    [B,4,S,S] the upstream gradient of rgba (row 0 the top row) or None -> Result with rgba, rgba_bound [B,4,S,S], Q, mask,
    edge_d2 (the squared distance of the pixel centre to the nearest edge of any contributing face) [B,S,S] (row 0 the top
    row); with g: g (the gradient with the masked pixels set to 0: hand THIS to the implementation), grad_faces [B,F,3,3] and
    grad_colors, shaped as colors (per image, also for shared colours: shared_colors adds them) with their _mag and _bound;
    pairs, doubt, masked, with_pair per image, doubt_share and masked_share (the largest of the images).  `variant`: the
    module docstring's."""
    fc, col = np.asarray(faces, np.float64), np.asarray(colors, np.float64)
    if variant in CORNER_VARIANTS and col.ndim == 3:
        raise ValueError('variant %r needs corner colours' % variant)
    B = fc.shape[0]
    col = np.broadcast_to(col, (B,) + col.shape[1:])
    adds = kernel_adds(S) if adds is None else adds
    bg = [float(c) for c in background]
    per = [_image(fc[b], col[b], S, float(sigma), float(gamma), float(near), float(far), float(eps), bg,
                  None if g is None else np.asarray(g, np.float64)[b][:, ::-1], adds, variant) for b in range(B)]
    out = Result()
    names = ('rgba', 'rgba_bound', 'Q', 'mask', 'edge_d2')
    if g is not None:
        names += ('g', 'grad_faces', 'grad_faces_mag', 'grad_faces_bound', 'grad_colors', 'grad_colors_mag', 'grad_colors_bound')
    for name in names:
        setattr(out, name, np.stack([getattr(r, name) for r in per]))
    for name in ('pairs', 'doubt', 'masked', 'with_pair'):
        setattr(out, name, [getattr(r, name) for r in per])
    out.doubt_share = max([r.doubt / r.pairs for r in per if r.pairs] or [0.0])
    out.masked_share = max([r.masked / r.with_pair for r in per if r.with_pair] or [0.0])
    return out


def shared_colors(res):
    """(grad, bound) of colours shared by the batch: the per-image gradients added in float64 and rounded once."""
    total = res.grad_colors.sum(0, keepdims=True)
    return total, res.grad_colors_bound.sum(0, keepdims=True) + U * np.abs(total)


def masked_ratio(got, ref, bound, mask):
    """worst_ratio of an image [B,C,S,S] over the pixels outside mask [B,S,S]."""
    keep = ~np.broadcast_to(mask[:, None], ref.shape)
    return worst_ratio(np.asarray(got, np.float64)[keep], ref[keep], bound[keep])


def hard_image(faces, colors, S, background=(0.0, 0.0, 0.0)):
    """The hard rasterizer's definition in float64, no anti-aliasing: at a pixel centre the face with the smallest depth zp
    among those that hold the centre strictly inside, its corner colours interpolated perspective-correctly; the background
    elsewhere.  faces [B,F,3,3], colors [B|1,F,3,3] -> rgb [B,3,S,S], row 0 the top row."""
    fc, col = np.asarray(faces, np.float64), np.asarray(colors, np.float64)
    B = fc.shape[0]
    col = np.broadcast_to(col, (B,) + col.shape[1:])
    c1 = (2.0 * np.arange(S) + 1 - S) / S
    px, py = np.tile(c1, S)[:, None], np.repeat(c1, S)[:, None]
    out = np.zeros((B, 3, S, S))
    for b in range(B):
        x, y, iz = fc[b, :, :, 0], fc[b, :, :, 1], 1.0 / fc[b, :, :, 2]
        edge = lambda i, j: (x[None, :, j] - x[None, :, i]) * (py - y[None, :, i]) - (y[None, :, j] - y[None, :, i]) * (px - x[None, :, i])
        c = [edge(0, 1), edge(1, 2), edge(2, 0)]
        inside = ((c[0] > 0) & (c[1] > 0) & (c[2] > 0)) | ((c[0] < 0) & (c[1] < 0) & (c[2] < 0))
        A = np.where(inside, c[0] + c[1] + c[2], 1.0)
        lam = [c[1] / A, c[2] / A, c[0] / A]
        u = [lam[j] * iz[None, :, j] for j in range(3)]
        zp = np.where(inside, 1.0 / np.where(inside, u[0] + u[1] + u[2], 1.0), np.inf)
        first = zp.argmin(1)
        hit = inside.any(1)
        rows = np.arange(S * S)
        zf = np.where(hit, zp[rows, first], 1.0)
        for ch in range(3):
            at = sum(u[j][rows, first] * zf * col[b, first, j, ch] for j in range(3))
            out[b, ch] = np.where(hit, at, float(background[ch])).reshape(S, S)[::-1]
    return out
