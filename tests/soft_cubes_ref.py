"""Test-side restatement of soft colour rendering with texture cubes sampled at the pixel (include/nr_hip.h: nr_soft_cubes_*;
DESIGN "Soft colour rendering", Texture cubes) in float64 NumPy: forward, Q and the ANALYTIC gradient to faces (x, y, z), to
the cubes and to the per-face light, with the term magnitudes and the per-entry bounds of a float32 run.

  restate(faces, textures, light, S, sigma, gamma, near, far, eps, background, texture_eps, g, adds, variant)  -> Result
  hard_image(faces, textures, light, S, background, texture_eps)   the hard rasterizer's definition of the same scene, float64
  shared(res, name)                                     the gradients of shared cubes / shared light: sums over the batch

Everything up to the colour of a pair -- the geometry, the depth, the aggregation, the masked pixels, the segment doubt, the
whole float32 operation sequence and the way every bound is counted (u = 2^-24, first order, every difference and sum
propagated with absolute values) -- is tests/soft_render_ref.py's, its corner-colour sequence included: read its docstring
first.  This file restates that sequence on soft_ref.geometry (soft_render_ref._image is one function and is not edited) with
the colour of a pair replaced (csrc/nr_soft_render.hip: cube_texel, cube_slopes, the <CUBE> instantiations):

  v_k      = mu_k (ts - 1), max with 0, min with hi = (ts - 1) - texture_eps (in double, rounded): the clamps move a value towards
           the exact range,  dv_k = (ts - 1) dmu_k + u |v_k|, plus u hi where the upper clamp may act (the rounding of hi)
  i_k, fr_k = (int)v_k, v_k - i_k: exact in float32 (a float minus its own integer part):  dfr_k = dv_k;  1 - fr_k: dv_k + u |1 - fr_k|
  w_pn     = (f_0 f_1) f_2, f_k the factor bit k of pn picks:  dw_pn = df_0 |f_1 f_2| + |f_0| df_1 |f_2| + |f_0 f_1| df_2 + 2 u |w_pn|
  T_c      = ((0 + w_0 tex_0c) + w_1 tex_1c) + ...: eight products, seven additions that round:
           dT_c = sum_pn |tex_pnc| dw_pn + 8 u sum_pn |w_pn tex_pnc|;  a tap outside the cube is no term
  C(p)_c   = L_c T_c:  dC_c = |L_c| dT_c + u |C_c|; an outside pair in segment doubt adds |L_c| |T_c at the other candidate's
           nearest point - T_c|, as soft_render_ref's dC takes |C(p)2 - C(p)|
  rgb, h   soft_render_ref's, with this C(p) and dC
  backward per taken pair:
           D_kc = sum of four (f_a f_b) (tex_up - tex_lo)_c, a and b the other two dimensions:  Dmag_kc = sum |f_a f_b| |tex_up - tex_lo|,
                  dD_kc = sum (df_a |f_b| + |f_a| df_b) |tex_up - tex_lo| + 6 u Dmag_kc   (a difference, two products, three additions)
           a_c  = g_c L_c, G_k = ((a_r D_kr + a_g D_kg) + a_b D_kb) (ts - 1):  Gmag_k = (ts - 1) sum_c |a_c| Dmag_kc,
                  dG_k = (ts - 1) sum_c |a_c| (dD_kc + 5 u Dmag_kc)
           Gm   = (mu_0 G_0 + mu_1 G_1) + mu_2 G_2:  Gmmag = sum mu_k Gmag_k,  dGm = sum (dmu_k Gmag_k + mu_k dG_k + 3 u mu_k Gmag_k)
           e_k  = G_k - Gm:  ekmag = Gmag_k + Gmmag,  de_k = dG_k + dGm + u ekmag
           E_k  = (W zp) e_k:  dE_k = W zp de_k + |E_k| (rel_W + dzp / zp + 2 u) -- and from here on every line is
                  soft_render_ref's corner-colour sequence with these E_k, dE_k
           light:  (W g_c) T_c:  |.| (rel_W + 2 u) + |W g_c| dT_c
           cubes:  ((W g_c) L_c) w_pn, the last product exact in double:  |W g_c L_c| (|w_pn| (rel_W + 2 u) + dw_pn); the double
                  additions count 2^-52 of the magnitudes; each sum is rounded once: u |sum|

Tap doubt (`tap_doubt_share`, of the taken pairs): a pair whose v_k lies within dv_k of an interior integer 1 .. ts - 2 may take
either cell.  T is continuous across the cells (the difference of the two cells' values at this v is added to dT all the same);
D_k belongs to one cell or the other: the magnitudes of both are added to dD; the pair's cube terms are added to the bounds of
the entries both cells touch.  An outside pair in segment doubt adds the terms of the other candidate's nearest point
likewise.  No doubt at 0: the clamp and (int) agree on both sides, and an outside pair has its third lambda exactly 0.  No doubt
at the upper clamp: texture_eps = 1e-3 keeps v_k a thousand roundings below ts - 1.

Masked pixels and segment doubt are soft_render_ref's: they depend on the geometry alone.

`variant`: a deliberately wrong restatement for the sensitivity tests: 'affine' (mu = lambda: screen-space weights),
'no_texture_geometry' (every E_k = 0: the texture's way into x, y, z cut), 'transposed' (axes 0 and 2 of the cube exchanged),
'unweighted_light' (dL/dL_fc += W g_c, without T_f(p)_c).
"""
import types

import numpy as np

import soft_ref
from soft_ref import EXP_ULP, LIVE_X, SEG_DOUBT, TINY, U, kernel_adds, sphere_faces, worst_ratio  # noqa: F401
from soft_render_ref import CUT_DOUBT, REACH, Result, gamma_k, masked_ratio  # noqa: F401

VARIANTS = ('affine', 'no_texture_geometry', 'transposed', 'unweighted_light')
OTHER = ((1, 2), (0, 2), (0, 1))   # the other two dimensions of k, ascending


def _sample(tex, hi, mu, transposed=False, src=None):
    """The lookup of tex [F,T,3] at the weights mu (three arrays [P,F]) -> v, cell, fr, the factors f[k] = (1 - fr_k, fr_k), the
    eight taps (flat [P,F] clipped into the cube, inside, w, texel [P,F,3] with zeros outside) and T [3 channels], Dmag[k][c].
    src: the positions the cells are taken from (the other side of an integer)."""
    F, T = tex.shape[:2]
    ts = int(round(T ** (1.0 / 3)))
    v = [np.minimum(np.maximum(np.nan_to_num(m_ * (ts - 1.0)), 0.0), hi) for m_ in mu]
    cell = [np.trunc(v[k] if src is None else src[k]).astype(np.int64) for k in range(3)]
    fr = [v[k] - cell[k] for k in range(3)]
    f = [(1 - fr[k], fr[k]) for k in range(3)]
    s = types.SimpleNamespace(v=v, cell=cell, fr=fr, f=f, flat=[], inside=[], w=[], tx=[])
    fidx = np.arange(F)[None]
    for pn in range(8):
        bit = [(pn >> k) & 1 for k in range(3)]
        idx = [cell[k] + bit[k] for k in range(3)]
        flat = (idx[2] * ts + idx[1]) * ts + idx[0] if transposed else (idx[0] * ts + idx[1]) * ts + idx[2]
        inside = (flat < T) & (flat >= 0)
        flat = np.clip(flat, 0, T - 1)
        s.flat.append(flat)
        s.inside.append(inside)
        s.w.append((f[0][bit[0]] * f[1][bit[1]]) * f[2][bit[2]])
        s.tx.append(np.where(inside[..., None], tex[fidx, flat], 0.0))
    s.T = [sum(s.tx[pn][..., c] * s.w[pn] for pn in range(8)) for c in range(3)]
    s.D, s.Dmag = [], []
    for k in range(3):
        ka, kb = OTHER[k]
        D, Dm = [0.0] * 3, [0.0] * 3
        for jb in range(2):
            for ja in range(2):
                lo = (ja << ka) | (jb << kb)
                up = lo | (1 << k)
                for c in range(3):
                    diff = s.tx[up][..., c] - s.tx[lo][..., c]
                    D[c] = D[c] + (f[ka][ja] * f[kb][jb]) * diff
                    Dm[c] = Dm[c] + np.abs(f[ka][ja] * f[kb][jb]) * np.abs(diff)
        s.D.append(D)
        s.Dmag.append(Dm)
    return s


def _image(fc, tex, light, S, sigma, gam, near, far, eps, bg, teps, g, adds, variant):
    """One image: fc [F,3,3], tex [F,T,3], light [F,3] float64, g [4,S,S] internal rows or None."""
    F, Tn = tex.shape[:2]
    ts = int(round(Tn ** (1.0 / 3)))
    hi = (ts - 1.0) - teps
    rng = far - near
    tr = variant == 'transposed'
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

    # ---- depth (soft_render_ref)
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
    share2 = [np.where(k2 == j, 1 - pick(t, k2), 0.0) + np.where((k2 + 1) % 3 == j, pick(t, k2), 0.0) for j in range(3)]
    differ = np.max([np.abs(share[j] - share2[j]) for j in range(3)], 0) > 1e-9
    seg_doubt = taken & (d22 - d2 <= SEG_DOUBT * d22) & (G.apart | differ)
    iz2 = share2[0] * izj[0] + share2[1] * izj[1] + share2[2] * izj[2]
    d_iz = d_iz + np.where(seg_doubt & ~inside, np.abs(iz2 - iz), 0.0)
    zp = 1.0 / iz
    dzp = zp * (d_iz / iz + U)
    zn = (far - zp) / rng
    dzn = (dzp + U * abs(far)) / rng + 3 * U * np.abs(zn)

    # ---- masked pixels and the geometry's doubt (soft_render_ref)
    cut_doubt = onp & ~inside & (np.abs(d2 / (REACH * sigma) - 1) < CUT_DOUBT)
    edge_doubt = onp & G.near0.any(0)
    mask = (cut_doubt | edge_doubt).any(1)                                    # [P]
    outside = taken & ~inside
    near_clamp = outside & (eek > 0) & (np.minimum(np.abs(t_rawk), np.abs(t_rawk - 1)) <= dt_full)
    doubt = (seg_doubt | near_clamp) & ~mask[:, None]
    seg_out = seg_doubt & ~inside

    # ---- the colour at the pixel: L_f T_f(p)
    mu = lam if variant == 'affine' else [uj[j] * zp for j in range(3)]
    dmu = [(dlam[j] * izj[j] + 2 * U * np.abs(uj[j])) * zp + np.abs(uj[j]) * dzp + U * np.abs(mu[j]) for j in range(3)]
    sm = _sample(tex, hi, mu, tr)
    dv = [(ts - 1.0) * dmu[j] + U * np.abs(sm.v[j]) for j in range(3)]
    dv = [dv[j] + np.where(sm.v[j] >= hi - dv[j], U * hi, 0.0) for j in range(3)]
    df = [(dv[j] + U * np.abs(sm.f[j][0]), dv[j]) for j in range(3)]         # df[k][bit]
    bits = [[(pn >> k) & 1 for k in range(3)] for pn in range(8)]
    dw = []
    for pn in range(8):
        f0, f1, f2 = [np.abs(sm.f[k][bits[pn][k]]) for k in range(3)]
        d0, d1, d2_ = [df[k][bits[pn][k]] for k in range(3)]
        dw.append(d0 * f1 * f2 + f0 * d1 * f2 + f0 * f1 * d2_ + 2 * U * np.abs(sm.w[pn]))
    # tap doubt: the other side of an interior integer
    near_n = [np.rint(sm.v[j]) for j in range(3)]
    tdk = [(np.abs(sm.v[j] - near_n[j]) <= dv[j]) & (near_n[j] >= 1) & (near_n[j] <= ts - 2) for j in range(3)]
    tex_doubt = taken & (tdk[0] | tdk[1] | tdk[2]) & ~mask[:, None]
    alt = _sample(tex, hi, mu, tr, [np.where(tdk[j], np.where(sm.v[j] >= near_n[j], near_n[j] - 0.25, near_n[j] + 0.25), sm.v[j])
                                    for j in range(3)])
    # the other candidate's nearest point of an outside pair in segment doubt
    zp2 = 1.0 / iz2
    sm2 = _sample(tex, hi, share2 if variant == 'affine' else [share2[j] * izj[j] * zp2 for j in range(3)], tr)
    T = sm.T
    dT = [sum(np.abs(sm.tx[pn][..., c]) * dw[pn] + 8 * U * np.abs(sm.tx[pn][..., c] * sm.w[pn]) for pn in range(8))
          + np.where(tex_doubt, np.abs(alt.T[c] - sm.T[c]), 0.0)
          + np.where(seg_out, np.abs(sm2.T[c] - sm.T[c]), 0.0) for c in range(3)]
    Lc = [light[None, :, c] for c in range(3)]
    Cp = [Lc[c] * T[c] for c in range(3)]
    dCp = [np.abs(Lc[c]) * dT[c] + U * np.abs(Cp[c]) for c in range(3)]

    # ---- aggregation (soft_render_ref)
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
    imax = np.abs(tex).max()
    cmax = 1 + np.abs(light).max() * imax * 8 + max(np.abs(bg))
    scale = (1 + 1 / sigma) * (1 + 1 / gam) * (1 + 1 / abs(rng)) * (1 + izv.max() ** 2) * cmax * (1 + 1 / izv.min()) * ts
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

    res = Result()
    img = lambda a: a.reshape(a.shape[:-1] + (S, S))[..., ::-1, :]
    res.rgba, res.rgba_bound = img(np.concatenate((rgb, alpha[None]))), img(np.concatenate((drgb, dalpha[None])))
    res.Q, res.mask = img(Q), img(mask)
    res.edge_d2 = img(np.where(onp, d2, np.inf).min(1))
    res.pairs, res.doubt, res.tap_doubt = int(taken.sum()), int(doubt.sum()), int(tex_doubt.sum())
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

    # E_k: what the texture adds to dL/d iz at corner k
    both = tex_doubt | (seg_out & ~mask[:, None])
    a = [gc[c] * Lc[c] for c in range(3)]
    Gk, Gmag, dG = [], [], []
    for k in range(3):
        ka, kb = OTHER[k]
        dD = []
        for c in range(3):
            e = 0.0
            for jb in range(2):
                for ja in range(2):
                    lo = (ja << ka) | (jb << kb)
                    diff = np.abs(sm.tx[lo | (1 << k)][..., c] - sm.tx[lo][..., c])
                    e = e + (df[ka][ja] * np.abs(sm.f[kb][jb]) + np.abs(sm.f[ka][ja]) * df[kb][jb]) * diff
            dD.append(e + 6 * U * sm.Dmag[k][c] + np.where(tex_doubt, sm.Dmag[k][c] + alt.Dmag[k][c], 0.0)
                      + np.where(seg_out, sm.Dmag[k][c] + sm2.Dmag[k][c], 0.0))
        Gk.append(sum(a[c] * sm.D[k][c] for c in range(3)) * (ts - 1.0))
        Gmag.append((ts - 1.0) * sum(np.abs(a[c]) * sm.Dmag[k][c] for c in range(3)))
        dG.append((ts - 1.0) * sum(np.abs(a[c]) * (dD[c] + 5 * U * sm.Dmag[k][c]) for c in range(3)))
    Gm = mu[0] * Gk[0] + mu[1] * Gk[1] + mu[2] * Gk[2]
    Gmmag = sum(np.abs(mu[j]) * Gmag[j] for j in range(3))
    dGm = sum(dmu[j] * Gmag[j] + np.abs(mu[j]) * dG[j] + 3 * U * np.abs(mu[j]) * Gmag[j] for j in range(3))
    Wz = np.where(taken, W * zp, 0.0)
    ek = [Gk[j] - Gm for j in range(3)]
    de = [dG[j] + dGm + U * (Gmag[j] + Gmmag) for j in range(3)]
    E = [np.zeros_like(Wz) if variant == 'no_texture_geometry' else Wz * ek[j] for j in range(3)]
    Eabs = [np.abs(Wz * ek[j]) for j in range(3)]
    dE = [np.where(taken, Wz * de[j] + Eabs[j] * (rel_W + dzp / zp + 2 * U), 0.0) for j in range(3)]

    grad, mag, bound = np.zeros((F, 3, 3)), np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
    ones = np.ones(shape)
    rot = lambda v: [v[1], v[2], v[0]]
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
        dTt = np.where(free, (ddz * np.abs(izb - iza) + np.abs(dz_) * U * (iza + izb)
                              + dEb * izb + dEa * iza + 3 * U * (Eba * izb + Eaa * iza)) / ees + 7 * U * Tanymag, 0.0)
    Tt = np.where(free, Tany, 0.0)
    Tmag = np.where(free, Tanymag, 0.0)
    Xj = [izj[(j + 2) % 3] - iz for j in range(3)]
    it = inside & taken
    q1 = [np.where(it, dz_ * Xj[j] / As, 0.0) for j in range(3)]
    qs = [np.where(it, E[(j + 2) % 3] * izj[(j + 2) % 3] / As, 0.0) for j in range(3)]
    qsa = [np.where(it, Eabs[(j + 2) % 3] * izj[(j + 2) % 3] / np.abs(As), 0.0) for j in range(3)]
    q = [q1[j] + qs[j] for j in range(3)]
    qmag = [np.abs(q1[j]) + qsa[j] for j in range(3)]
    dq = [np.where(it, (ddz * np.abs(Xj[j]) + np.abs(dz_) * (d_iz + U * izj[(j + 2) % 3] + U * np.abs(Xj[j]))) / np.abs(As)
                   + np.abs(q1[j]) * (dA / np.abs(As) + 3 * U)
                   + dE[(j + 2) % 3] * izj[(j + 2) % 3] / np.abs(As) + qsa[j] * (dA / np.abs(As) + 4 * U) + U * qmag[j], 0.0)
          for j in range(3)]
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
        ja, jb = (j + 2) % 3, (j + 1) % 3
        for comp, (r, dr0, e, r2, e2) in enumerate(((rxk, dr0x, exk, pick(rx, k2), pick(ex, k2)),
                                                    (ryk, dr0y, eyk, pick(ry, k2), pick(ey, k2)))):
            drf = dr0 + np.abs(e) * dt
            v1 = -2 * share[j] * r * C
            m1 = 2 * share[j] * np.abs(r) * Cmag
            e1 = 2 * share[j] * np.abs(r) * dC + 3 * U * m1 + 2 * Cmag * (np.where(any_role, np.abs(r) * dt, 0.0) + share[j] * drf)
            v2 = sgn * Tt * r - share[j] * Tt * e
            m2 = np.abs(sgn) * Tmag * np.abs(r) + share[j] * Tmag * np.abs(e)
            e2_ = np.abs(sgn) * (dTt * np.abs(r) + Tmag * drf) + share[j] * (dTt + 2 * U * Tmag) * np.abs(e) \
                + np.abs(sgn) * Tmag * dt * np.abs(e)
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
            err = err + np.where(doubt & seg_doubt, m1 + m2 + 2 * share2[j] * np.abs(r2) * Cmag + T2 * (np.abs(r2) + np.abs(e2)), 0.0)
            err = err + np.where(doubt & near_clamp, m2 + np.where(any_role, Tanymag * (np.abs(r) + np.abs(e)), 0.0), 0.0)
            grad[:, j, comp] = (v1 + v2 + v3).sum(0)
            mag[:, j, comp] = mm.sum(0)
            bound[:, j, comp] = err.sum(0)
        sq = izj[j] * izj[j]
        dk, dkmag = dz_ + E[j], np.abs(dz_) + Eabs[j]
        vz = -(dk * lam[j]) * sq
        vzmag = dkmag * np.abs(lam[j]) * sq
        ddk = ddz + dE[j] + U * dkmag
        ez = np.where(taken, ddk * np.abs(lam[j]) * sq + dkmag * dlam[j] * sq + 5 * U * vzmag + under, 0.0)
        ez = ez + np.where(doubt & seg_doubt & outside, vzmag + (dkmag + dE[j]) * share2[j] * sq, 0.0)
        grad[:, j, 2] = vz.sum(0)
        mag[:, j, 2] = vzmag.sum(0)
        bound[:, j, 2] = ez.sum(0)

    # ---- light and images
    Pn = F * Tn
    gl, gl_mag, gl_bound = np.zeros((F, 3)), np.zeros((F, 3)), np.zeros((F, 3))
    gi, gi_mag, gi_bound = np.zeros((Pn, 3)), np.zeros((Pn, 3)), np.zeros((Pn, 3))
    face0 = (np.arange(F) * Tn)[None]

    def scatter(smp, pn, vals, where):
        sel = where & smp.inside[pn]
        return np.bincount((face0 + smp.flat[pn])[sel], weights=np.broadcast_to(vals, shape[1:])[sel], minlength=Pn)
    for c in range(3):
        Wg = W * gc[c]
        v = Wg if variant == 'unweighted_light' else Wg * T[c]
        gl[:, c], gl_mag[:, c] = v.sum(0), np.abs(Wg * T[c]).sum(0)
        e = np.abs(Wg * T[c]) * (rel_W + 2 * U) + np.abs(Wg) * dT[c] + under
        gl_bound[:, c] = np.where(taken, e, 0.0).sum(0)
        WgL = Wg * Lc[c]
        for pn in range(8):
            term = WgL * sm.w[pn]
            gi[:, c] += scatter(sm, pn, term, taken)
            gi_mag[:, c] += scatter(sm, pn, np.abs(term), taken)
            gi_bound[:, c] += scatter(sm, pn, np.abs(WgL) * (np.abs(sm.w[pn]) * (rel_W + 2 * U) + dw[pn]) + under
                                      + np.where(both, np.abs(term), 0.0), taken)
            gi_bound[:, c] += scatter(alt, pn, np.abs(WgL * alt.w[pn]), tex_doubt)
            gi_bound[:, c] += scatter(sm2, pn, np.abs(WgL * sm2.w[pn]), seg_out & ~mask[:, None])
    ga_ = gamma_k(adds)
    res.grad_faces, res.grad_faces_mag, res.grad_faces_bound = grad, mag, bound + ga_ * mag
    res.grad_light, res.grad_light_mag, res.grad_light_bound = gl, gl_mag, gl_bound + ga_ * gl_mag
    shp = (F, ts, ts, ts, 3)   # ('transposed' reads and scatters at the exchanged index of the caller's own layout)
    res.grad_textures, res.grad_textures_mag = gi.reshape(shp), gi_mag.reshape(shp)
    res.grad_textures_bound = (gi_bound + U * np.abs(gi) + 2.0 ** -52 * gi_mag).reshape(shp)
    return res


def restate(faces, textures, light, S, sigma, gamma, near=0.1, far=100.0, eps=1e-3, background=(0.0, 0.0, 0.0), texture_eps=1e-3,
            g=None, adds=None, variant=None):
    """faces [B,F,3,3], textures [B|1,F,ts,ts,ts,3], light [B|1,F,3] or None (float32 values), g [B,4,S,S] the upstream
    gradient of rgba (row 0 the top row) or None -> Result with rgba, rgba_bound [B,4,S,S], Q, mask, edge_d2 [B,S,S]; with g:
    g (the gradient with the masked pixels set to 0: hand THIS to the implementation), grad_faces [B,F,3,3], grad_light
    [B,F,3] and grad_textures [B,F,ts,ts,ts,3] PER IMAGE of the batch (shared() adds them) with their _mag and _bound; pairs,
    doubt, tap_doubt, masked, with_pair per image, doubt_share, tap_doubt_share and masked_share (the largest of the images)."""
    fc, tx = np.asarray(faces, np.float64), np.asarray(textures, np.float64)
    if variant is not None and variant not in VARIANTS:
        raise ValueError('unknown variant %r' % (variant,))
    B, F = fc.shape[:2]
    lt = np.ones((1, F, 3)) if light is None else np.asarray(light, np.float64)
    lt, tx = np.broadcast_to(lt, (B, F, 3)), np.broadcast_to(tx, (B,) + tx.shape[1:])
    adds = kernel_adds(S) if adds is None else adds
    bg = [float(c) for c in background]
    per = [_image(fc[b], tx[b].reshape(F, -1, 3), lt[b], S, float(sigma), float(gamma), float(near), float(far), float(eps), bg,
                  float(texture_eps), None if g is None else np.asarray(g, np.float64)[b][:, ::-1], adds, variant) for b in range(B)]
    out = Result()
    names = ('rgba', 'rgba_bound', 'Q', 'mask', 'edge_d2')
    if g is not None:
        names += ('g',) + tuple(n_ + s_ for n_ in ('grad_faces', 'grad_light', 'grad_textures') for s_ in ('', '_mag', '_bound'))
    for name in names:
        setattr(out, name, np.stack([getattr(r, name) for r in per]))
    for name in ('pairs', 'doubt', 'tap_doubt', 'masked', 'with_pair'):
        setattr(out, name, [getattr(r, name) for r in per])
    out.doubt_share = max([r.doubt / r.pairs for r in per if r.pairs] or [0.0])
    out.tap_doubt_share = max([r.tap_doubt / r.pairs for r in per if r.pairs] or [0.0])
    out.masked_share = max([r.masked / r.with_pair for r in per if r.with_pair] or [0.0])
    return out


def shared(res, name):
    """(grad, mag, bound) of `name` ('grad_textures' or 'grad_light') shared by the batch: the per-image gradients, each
    rounded once, added in float64 and rounded once more."""
    total = getattr(res, name).sum(0, keepdims=True)
    return (total, getattr(res, name + '_mag').sum(0, keepdims=True),
            getattr(res, name + '_bound').sum(0, keepdims=True) + U * np.abs(total))


def hard_image(faces, textures, light, S, background=(0.0, 0.0, 0.0), texture_eps=1e-3):
    """The hard rasterizer's definition in float64, no anti-aliasing: at a pixel centre the face with the smallest depth zp
    among those that hold the centre strictly inside, its cube sampled at the perspective-correct weights (compute_taps'
    sequence), times its light; the background elsewhere.  faces [B,F,3,3], textures [B|1,F,ts,ts,ts,3], light [B|1,F,3] ->
    rgb [B,3,S,S], row 0 the top row."""
    fc, tx = np.asarray(faces, np.float64), np.asarray(textures, np.float64)
    B, F = fc.shape[:2]
    ts = tx.shape[2]
    lt, tx = np.broadcast_to(np.asarray(light, np.float64), (B, F, 3)), np.broadcast_to(tx, (B,) + tx.shape[1:])
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
        zf = np.where(inside, zp, 1.0)
        sm = _sample(tx[b].reshape(F, -1, 3), (ts - 1.0) - texture_eps, [u[j] * zf for j in range(3)])
        first = zp.argmin(1)
        hit = inside.any(1)
        rows = np.arange(S * S)
        for ch in range(3):
            at = (lt[b][None, :, ch] * sm.T[ch])[rows, first]
            out[b, ch] = np.where(hit, at, float(background[ch])).reshape(S, S)[::-1]
    return out
