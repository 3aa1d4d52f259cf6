"""Test-side restatement of soft colour rendering with CORNER colours (include/nr_hip.h: nr_soft_corners_*; DESIGN "Soft colour
rendering", Corner colours) in float64 NumPy: forward, Q and the ANALYTIC gradient to faces (x, y, z) and to the nine colour
entries of a face, with the term magnitudes and the per-entry bounds of a float32 run.

  restate(faces, colors [B|1,F,3,3], S, sigma, gamma, near, far, eps, background, g, adds, variant)  -> Result
  hard_image(faces, colors, S, background)   the hard rasterizer's definition of the same scene, float64 (no anti-aliasing)
  shared_colors, masked_ratio, worst_ratio, sphere_faces, kernel_adds, gamma_k, U            from tests/soft_render_ref.py

Everything that soft_render_ref.py's docstring says holds here, term for term: the arrays [3, S*S pixels, F faces], the
masked-pixel rule, the doubt rule, the assumptions (expf within 2 ulp ASSUMED, division correctly rounded), u = 2^-24, first
order.  What the corner colours add to the float32 operation sequence (csrc/nr_soft_render.hip, the <true> instantiations):

  u_k      = lambda_k iz_k (pair_depth's own products):  du_k = dl_k / z_k + 2 u u_k
  mu_k     = u_k zp:  dmu_k = du_k zp + u_k dzp + u mu_k
  C(p)_c   = (mu_0 C_0c + mu_1 C_1c) + mu_2 C_2c:  dC_c = sum_k dmu_k |C_kc| + 3 u sum_k mu_k |C_kc|; an outside pair in segment
           doubt adds |C(p) of the other candidate's nearest point - C(p)|, as d iz takes |iz2 - iz|
  rgb      soft_render_ref's drgb_c with C_ic = C_i(p)_c, plus sum_i (w_i / Z) dC_ic
  backward per taken pair: h = (gr (C(p)_r - R) + gg (C(p)_g - G)) + gb (C(p)_b - B):  dh gains sum_c |g_c| dC_c
           colours: (W g_c) mu_k:  |.| (rel_W + 2 u) + |W g_c| dmu_k
           e_k = (gr (C_kr - C(p)_r) + gg (..)) + gb (..):  de_k = sum_c |g_c| dC_c + 4 u sum_c |g_c| |C_kc - C(p)_c|
           E_k = (W zp) e_k:  dE_k = W zp de_k + |E_k| (rel_W + dzp / zp + 2 u)
           z:      -((diz + E_k) lambda_k) (iz_k iz_k):  (ddiz + dE_k + u (|diz| + |E_k|)) lambda_k / z_k^2
                   + (|diz| + |E_k|) dl_k / z_k^2 + 5 u (|diz| + |E_k|) lambda_k / z_k^2
           free t: T = (diz (iz_b - iz_a) + (E_b iz_b - E_a iz_a)) / ee:  soft_render_ref's dT of the first product, plus
                   (dE_b iz_b + dE_a iz_a + 3 u (|E_b| iz_b + |E_a| iz_a)) / ee, plus 7 u of the magnitude
                   Tmag = (|diz (iz_b - iz_a)| + |E_b| iz_b + |E_a| iz_a) / ee, which stands where |T| stood
           inside: q_j = (diz (1 / A)) (iz_v - iz) + (E_v iz_v) (1 / A), v = (j + 2) mod 3:  soft_render_ref's dq_j of the first
                   term, plus dE_v iz_v / |A| + |second| (dA / |A| + 4 u) + u (|first| + |second|); |first| + |second| stands
                   where |q_j| stood
  Every magnitude (`_mag`) counts the parts of a cancelling sum separately, as above.

Doubt: a pair in segment doubt adds the other candidate's terms with ITS free-t magnitude (E at its two ends); its z terms
with (|diz| + |E_k| + dE_k).  Near the end of an edge the two candidates' nearest points coincide within the doubt, so do
their colours: what is apart is the free-t term, d_b iz_b - d_a iz_a, whole.

`variant`: a deliberately wrong restatement for the sensitivity tests -- 'affine' (mu = lambda: screen-space interpolation),
'rotated' (corner k takes the colour of corner k + 1), 'no_colour_path' (every E_k = 0: the colour's way into x, y, z cut).
"""
import numpy as np

import soft_render_ref as R
from soft_render_ref import (CUT_DOUBT, EDGE_DOUBT, EXP_ULP, LIVE_X, REACH, SEG_DOUBT, TINY, U, Result, gamma_k,  # noqa: F401
                             kernel_adds, masked_ratio, shared_colors, sphere_faces, worst_ratio)


def _image(fc, col, S, sigma, gam, near, far, eps, bg, g, adds, variant):
    """One image: fc [F,3,3], col [F,3 corners,3 rgb] float64, g [4,S,S] internal rows or None."""
    F = fc.shape[0]
    rng = far - near
    if variant == 'rotated':
        col = col[:, (1, 2, 0)]
    with np.errstate(all='ignore'):
        area = (fc[:, 1, 0] - fc[:, 0, 0]) * (fc[:, 2, 1] - fc[:, 0, 1]) - (fc[:, 2, 0] - fc[:, 0, 0]) * (fc[:, 1, 1] - fc[:, 0, 1])
        on = np.isfinite(fc).all((1, 2)) & (fc[:, :, 2] >= near).all(1) & (fc[:, :, 2] <= far).all(1) & (area != 0)
    xy = np.where(on[:, None, None], fc[:, :, :2], 0.0)
    izv = 1.0 / np.where(on[:, None], fc[:, :, 2], 1.0)      # [F,3]
    c1 = (2.0 * np.arange(S) + 1 - S) / S
    px = np.tile(c1, S)[:, None]       # [P,1], P = yi * S + xi
    py = np.repeat(c1, S)[:, None]
    A_ = np.stack([xy[:, k] for k in range(3)])            # [3,F,2]: a of segment k
    Bv = np.stack([xy[:, (k + 1) % 3] for k in range(3)])  # b of segment k
    ax, ay, bx, by = A_[:, None, :, 0], A_[:, None, :, 1], Bv[:, None, :, 0], Bv[:, None, :, 1]   # [3,1,F]
    ex, ey = bx - ax, by - ay
    wx, wy = px[None] - ax, py[None] - ay                  # [3,P,F]
    dot, ee = wx * ex + wy * ey, ex * ex + ey * ey
    pos = ee > 0
    with np.errstate(all='ignore'):
        t_raw = np.where(pos, dot / np.where(pos, ee, 1.0), 0.0)
    t = np.clip(t_raw, 0.0, 1.0)
    cx, cy = ax + t * ex, ay + t * ey
    vx, vy = px[None] - bx, py[None] - by
    rx, ry = (1 - t) * wx + t * vx, (1 - t) * wy + t * vy
    d2s = rx * rx + ry * ry
    cr = ex * wy - ey * wx
    k = np.argmin(d2s, 0)                                  # the lowest k on a tie
    shape = d2s.shape
    pick = lambda a, kk=None: np.take_along_axis(np.broadcast_to(a, shape), (k if kk is None else kk)[None], 0)[0]
    d2 = pick(d2s)
    inside = (cr > 0).all(0) | (cr < 0).all(0)
    s = np.where(inside, 1.0, -1.0)
    x = s * d2 / sigma
    onp = np.broadcast_to(on[None, :], x.shape)
    taken = onp & (inside | (d2 <= REACH * sigma))

    # ---- soft_ref's rounding terms of the chosen segment
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
    d2_other = np.where(np.arange(3)[:, None, None] == k[None], np.inf, d2s)
    k2 = np.argmin(d2_other, 0)
    d22 = pick(d2s, k2)
    apart = np.hypot(pick(cx, k2) - pick(cx), pick(cy, k2) - pick(cy)) > 1e-12 * (1 + np.abs(pick(cx)) + np.abs(pick(cy)))
    share2 = [np.where(k2 == j, 1 - pick(t, k2), 0.0) + np.where((k2 + 1) % 3 == j, pick(t, k2), 0.0) for j in range(3)]
    differ = np.max([np.abs(share[j] - share2[j]) for j in range(3)], 0) > 1e-9
    seg_doubt = taken & (d22 - d2 <= SEG_DOUBT * d22) & (apart | differ)
    iz2 = share2[0] * izj[0] + share2[1] * izj[1] + share2[2] * izj[2]
    d_iz = d_iz + np.where(seg_doubt & ~inside, np.abs(iz2 - iz), 0.0)
    zp = 1.0 / iz
    dzp = zp * (d_iz / iz + U)
    zn = (far - zp) / rng
    dzn = (dzp + U * abs(far)) / rng + 3 * U * np.abs(zn)

    # ---- the colour at the pixel
    mu = lam if variant == 'affine' else [uj[j] * zp for j in range(3)]
    dmu = [(dlam[j] * izj[j] + 2 * U * np.abs(uj[j])) * zp + np.abs(uj[j]) * dzp + U * np.abs(mu[j]) for j in range(3)]
    ck = [[col[None, :, j, c] for c in range(3)] for j in range(3)]           # ck[corner][channel]: [1,F]
    Cp = [mu[0] * ck[0][c] + mu[1] * ck[1][c] + mu[2] * ck[2][c] for c in range(3)]   # [P,F]
    zp2 = 1.0 / iz2
    Cp2 = [sum(share2[j] * izj[j] * zp2 * ck[j][c] for j in range(3)) for c in range(3)]
    dCp = [sum(dmu[j] * np.abs(ck[j][c]) + 3 * U * np.abs(mu[j] * ck[j][c]) for j in range(3))
           + np.where(seg_doubt & ~inside, np.abs(Cp2[c] - Cp[c]), 0.0) for c in range(3)]

    # ---- aggregation
    with np.errstate(all='ignore'):
        D = np.where(taken, 1.0 / (1.0 + np.exp(-x)), 0.0)
        oneD = np.where(taken, 1.0 / (1.0 + np.exp(x)), 0.0)
        m = np.maximum(eps, np.where(taken, zn, -np.inf).max(1))              # [P]
        arg = np.where(taken, (zn - m[:, None]) / gam, 0.0)
        w = np.where(taken, D * np.exp(arg), 0.0)
        arg_b = (eps - m) / gam
        wb = np.exp(arg_b)
        Z = wb + w.sum(1)
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
    scale = (1 + 1 / sigma) * (1 + 1 / gam) * (1 + 1 / abs(rng)) * (1 + izv.max() ** 2) * cmax * (1 + 1 / izv.min())
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
    emag = np.abs(ex * wy) + np.abs(ey * wx)
    near0 = (emag > 0) & (np.abs(cr) <= EDGE_DOUBT * emag)
    edge_doubt = onp & near0.any(0)
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
    t1v = hW * oneD
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
    # E_k: what corner k's colour adds to dL/d iz
    Wz = np.where(taken, W * zp, 0.0)
    ek = [sum(gc[c] * (ck[j][c] - Cp[c]) for c in range(3)) for j in range(3)]
    ekmag = [sum(np.abs(gc[c] * (ck[j][c] - Cp[c])) for c in range(3)) for j in range(3)]
    if variant == 'no_colour_path':
        E = [np.zeros_like(Wz) for j in range(3)]
    else:
        E = [Wz * ek[j] for j in range(3)]
    dE = [np.where(taken, Wz * (gdC + 4 * U * ekmag[j]) + np.abs(Wz * ek[j]) * (rel_W + dzp / zp + 2 * U), 0.0) for j in range(3)]
    Eabs = [np.abs(Wz * ek[j]) for j in range(3)]

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
                   + np.abs(q1[j]) * (dA / np.abs(As) + 3 * U)
                   + dE[(j + 2) % 3] * izj[(j + 2) % 3] / np.abs(As) + qsa[j] * (dA / np.abs(As) + 4 * U) + U * qmag[j], 0.0)
          for j in range(3)]
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
        ez = np.where(taken, (ddz + dE[j] + U * dkmag) * np.abs(lam[j]) * sq + dkmag * dlam[j] * sq + 5 * U * vzmag + under, 0.0)
        ez = ez + np.where(doubt & seg_doubt & outside, vzmag + (dkmag + dE[j]) * share2[j] * sq, 0.0)
        grad[:, j, 2] = vz.sum(0)
        mag[:, j, 2] = vzmag.sum(0)
        bound[:, j, 2] = ez.sum(0)
    gcol, gcol_mag, gcol_bound = np.zeros((F, 3, 3)), np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
    for j in range(3):
        jj = (j + 1) % 3 if variant == 'rotated' else j    # (back to the caller's corner order)
        for c in range(3):
            Wg = W * gc[c]
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
    """faces [B,F,3,3], colors [B,F,3,3] or [1,F,3,3] (float32 values; face, corner, rgb), g [B,4,S,S] the upstream gradient
    of rgba (row 0 the top row) or None -> Result as soft_render_ref.restate's, grad_colors [B,F,3,3] (per image, also for
    shared colours: soft_render_ref.shared_colors adds them), and edge_d2 [B,S,S], the squared distance of the pixel centre
    to the nearest edge of any contributing face."""
    fc, col = np.asarray(faces, np.float64), np.asarray(colors, np.float64)
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
