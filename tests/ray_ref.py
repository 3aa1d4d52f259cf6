"""Float64 restatement of neural_renderer_amd/ray_mesh.py (DESIGN "Ray casting"), in NumPy, independent of the product's code --
the yardstick of tests/test_ray_mesh.py and test_ray_mesh_gpu.py -- with the bounds, the ambiguous rays, the gradients and the
ray generator.  u = 2^-24 in float32, 2^-53 in float64.

The definition (csrc/nr_ray_triangle.h).  e1 = v1 - v0, e2 = v2 - v0, pvec = d x e2, det = e1 . pvec, tvec = o - v0, qvec = tvec x e1,
s = sign(det), D = |det|, U = s (tvec . pvec), V = s (d . qvec), T = s (e2 . qvec); a hit iff D > 0, U >= 0, V >= 0, U + V <= D, with
cull det > 0, and near <= t < far for t = T / D; w1 = U / D, w2 = V / D, w0 = max(1 - w1 - w2, 0); the first hit is the smallest t,
the lowest face on a tie.

Bounds, by counting roundings relative to each term's MAGNITUDE (the sum of the absolute values of the products that make it
up), since every quantity here is a sum of products that may cancel.  The inputs are exact.  |x| is taken per component.
  e1, e2, tvec   one rounding each: u |e1_c|, ...
  pvec_c = d_a e2_b - d_b e2_a    e2's rounding, a product, the subtraction: 3 u Mp_c,   Mp_c = |d_a e2_b| + |d_b e2_a|
  qvec_c = tvec_a e1_b - ...      both factors rounded, a product, the subtraction: 4 u Mq_c,   Mq_c = |tvec_a e1_b| + |tvec_b e1_a|
  det = (e1_0 p_0 + e1_1 p_1) + e1_2 p_2   per term p's 3, e1's 1, the product, two additions: 7 u M_det,   M_det = sum |e1_c| Mp_c
  U = tvec . pvec   likewise 7 u M_U, M_U = sum |tvec_c| Mp_c;      V = d . qvec   4 + 1 + 2 = 7 u M_V, M_V = sum |d_c| Mq_c
  T = e2 . qvec     4 + 1 + 1 + 2 = 8 u M_T, M_T = sum |e2_c| Mq_c;   U + V one more: u (M_U + M_V)
KN = 8 covers each of them.  A quotient x / D, D clear of its own error: (err_x + |x / D| err_D) / (D - err_D) + u |x / D|.
  t:  (KN u (M_T + |t| M_det)) / (D - err_D) + u |t|;    w1, w2 likewise from M_U, M_V;    w0 = (1 - w1) - w2: their two bounds + 2 u.
  The weights are >= 0 and sum to 1 within 4 u: (1 - w1) and its difference with w2 are one rounding each of numbers below 1,
  and where the difference is clipped at 0 the quotients exceed 1 together by at most their own two roundings.

Ambiguous rays.  In float64, with the margins above, a pair is CLEAR when it is decided with room to spare: inside (D > err_D,
U > err_U, V > err_V, D - U - V > err_U + err_V + err_D + u (M_U + M_V)) with t in range (near + err_t <= t < far - err_t), or
outside by any one test with the same room.  With |det| <= err_D the sign itself is open; the pair can only be a hit when both
|u| and |v| are within err_U + err_V + 2 err_D of 0 (the computed U and V then have one sign and sum below the computed D),
otherwise it is clearly none.  The robust first hit is the nearest clear hit.  A ray is ambiguous when a pair that is not
clear -- near an edge, near `near` or `far`, or with an open sign -- or a clear hit of ANOTHER face has a t (where it has one)
not clearly behind the robust first hit, t - err_t <= t_rob + err_t_rob.  Such a ray is left out of the id and hit / miss
comparison; the reported face's own float64 t must still match the reported t.  At most CAP = 2 % of the rays of a case may
be left out.

Gradients (the differentiable tail: t_d = ((v0 - o) . n) / (d . n), n = e1 x e2, through torch's autograd).  With N = (v0 - o) . n,
Dn = d . n, t = N / Dn, p = o + t d and the plane's weights w_k of p:  dt/do = -n / Dn,  dt/dd = -t n / Dn,  dt/dv_k = w_k n / Dn.
autograd computes them as grad_N = g / Dn, grad_Dn = -g N / Dn^2, grad_n = grad_N (v0 - o) + grad_Dn d  (= (g / Dn)(v0 - p): a difference
of two vectors that cancel, so its error is relative to |v0 - o| + |t d|, not to |v0 - p|), grad_e1 = e2 x grad_n, grad_e2 = grad_n x e1,
grad_v1 = grad_e1, grad_v2 = grad_e2, grad_v0 = grad_N n - grad_e1 - grad_e2, grad_o = -grad_N n, grad_d = grad_Dn n.  Magnitudes: Mn_c = |e1_a e2_b| +
|e1_b e2_a| (n: 4 u Mn_c), M_Dn = sum |d_c| Mn_c (Dn: 7 u M_Dn), M_N = sum |(v0 - o)_c| Mn_c (N: 8 u M_N); rho = M_Dn / |Dn| >= 1 is the
condition of the denominator (large for a grazing ray) and tau = M_N / |Dn| >= |t|.
  grad_N n_c:  the quotient's (7 rho + 1) u, n's 4 u Mn_c, the product:   <= 13 rho u |g / Dn| Mn_c
  grad_Dn:     N's 8 u M_N / Dn^2, Dn^2's 2 (7 rho) u, two quotients, a product:   so grad_Dn d_c and grad_Dn n_c carry <= 27 rho u of
               |g| tau / |Dn| times |d_c| resp. Mn_c
  grad_n_c:    <= 27 rho u G_c,   G_c = |g / Dn| (|(v0 - o)_c| + tau |d_c|)   (the first part's 11 rho u, the second's 27 rho u, the sum)
  grad_e:      the other edge's rounding, a product, the subtraction:   (27 rho + 3) u x(|e|, G)_c,   x(a, b)_c = a_a b_b + a_b b_a
  grad_v0:     the three uses of v0 summed: 2 more
so a term of an entry is bounded by (KG rho + KE + K) u x its magnitude, KG = 27, KE = 5, K the number of terms autograd adds
into the entry (rays per vertex; images for rays shared by the batch; rays for one origin), with the magnitudes
  o: |g / Dn| Mn_c;   d: |g| tau / |Dn| Mn_c;   v1: x(|e2|, G)_c;   v2: x(|e1|, G)_c;   v0: their sum + |g / Dn| Mn_c.
An entry that no hit reaches must be exactly 0."""
import numpy as np

import point_mesh_ref as PM

U = 2.0 ** -24
U64 = 2.0 ** -53
KN = 8.0
KG, KE = 27.0, 5.0
CAP = 0.02


def _image(t, b):
    t = np.asarray(t)
    return t if t.ndim == 2 else (t[0] if t.shape[0] == 1 else t[b])


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def _xmag(a, b):
    """the magnitude of a cross product: |a_a| |b_b| + |a_b| |b_a| per component"""
    a, b = np.abs(a), np.abs(b)
    return np.stack((a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), -1)


def _dot(a, b):
    return (a * b).sum(-1)


def pair_terms(o, d, v0, v1, v2):
    """The float64 quantities of the pairs (broadcast against each other, [..., 3] each) and their magnitudes"""
    o, d, v0, v1, v2 = (np.asarray(t, np.float64) for t in (o, d, v0, v1, v2))
    e1, e2, tv = v1 - v0, v2 - v0, o - v0
    p, q = _cross(d, e2), _cross(tv, e1)
    Mp, Mq = _xmag(d, e2), _xmag(tv, e1)
    with np.errstate(invalid='ignore'):
        out = dict(det=_dot(e1, p), u=_dot(tv, p), v=_dot(d, q), T=_dot(e2, q),
                   M_det=_dot(np.abs(e1), Mp), M_U=_dot(np.abs(tv), Mp), M_V=_dot(np.abs(d), Mq), M_T=_dot(np.abs(e2), Mq))
    return out


def quotient_bound(x, M_x, D, M_det, u):
    """the bound of x / D from x's and D's magnitudes (module docstring); inf where D is not clear of its own error"""
    err_D = KN * u * M_det
    room = D - err_D
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.abs(x) / D
        b = KN * u * (M_x + q * M_det) / room + u * q
    return np.where(room > 0, b, np.inf)


def classify(terms, near, far, cull, u):
    """-> (t [n,F], err_t, clear_hit, open): `open` marks the pairs that are neither a clear hit nor clearly none; their t is
    -inf where the sign of det is open (they threaten every hit)"""
    det, M_det, M_U, M_V, M_T = terms['det'], terms['M_det'], terms['M_U'], terms['M_V'], terms['M_T']
    s = np.where(det < 0, -1.0, 1.0)
    D, Uq, Vq, Tq = np.abs(det), s * terms['u'], s * terms['v'], s * terms['T']
    e_D, e_U, e_V = KN * u * M_det, KN * u * M_U, KN * u * M_V
    e_S = e_U + e_V + e_D + u * (M_U + M_V)
    finite = np.isfinite(det) & np.isfinite(Uq) & np.isfinite(Vq) & np.isfinite(Tq)
    sign_open = finite & (D <= e_D)
    # an open sign: a hit is possible only with both numerators at the origin's margin; collapsed faces with everything exactly
    # 0 (e1 = 0 or e2 = 0) are clearly none
    near_zero = (np.abs(terms['u']) <= e_U + e_V + 2 * e_D) & (np.abs(terms['v']) <= e_U + e_V + 2 * e_D) & (M_det > 0)
    sign_threat = sign_open & near_zero
    known = finite & ~sign_open
    culled = known & (det < 0) if cull else np.zeros(det.shape, bool)
    inside = known & ~culled & (Uq > e_U) & (Vq > e_V) & (D - Uq - Vq > e_S)
    outside = ~finite | culled | (sign_open & ~near_zero) | (known & ((Uq < -e_U) | (Vq < -e_V) | (Uq + Vq - D > e_S)))
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(known, Tq / np.where(D > 0, D, 1.0), -np.inf)
    err_t = np.where(known, quotient_bound(Tq, M_T, D, M_det, u), np.inf)
    err_t = np.where(np.isfinite(err_t), err_t, np.inf)
    with np.errstate(invalid='ignore'):
        in_range = (t - err_t >= near) & (t + err_t < far)
        out_range = (t + err_t < near) | (t - err_t >= far)
    clear_hit = inside & in_range
    clear_none = outside | (known & out_range)
    open_ = ~clear_hit & ~clear_none
    t = np.where(sign_threat, -np.inf, t)
    return t, err_t, clear_hit, open_


def analyse(origins, directions, vertices, faces, near=0.0, far=np.inf, cull=False, u=U, B=None):
    """-> (ids [B,R] the robust first hit or -1, ambiguous [B,R] bool)"""
    origins, directions, vertices = np.asarray(origins), np.asarray(directions), np.asarray(vertices)
    B = B or max(1 if t.ndim == 2 else t.shape[0] for t in (origins, directions, vertices))
    ids, amb = [], []
    for b in range(B):
        d = np.asarray(_image(directions, b), np.float64)
        o = np.broadcast_to(np.asarray(_image(origins, b), np.float64), d.shape)   # (one origin [1,3] for the rays of an image)
        v0, v1, v2 = PM.corners(vertices, faces, b)
        row_id, row_amb = [], []
        for r0 in range(0, d.shape[0], 256):
            terms = pair_terms(o[r0:r0 + 256, None], d[r0:r0 + 256, None], v0[None], v1[None], v2[None])
            t, err_t, clear_hit, open_ = classify(terms, near, far, cull, u)
            t_hit = np.where(clear_hit, t, np.inf)
            first = t_hit.argmin(1)
            rows = np.arange(t.shape[0])
            t_rob = t_hit[rows, first]
            horizon = np.where(np.isfinite(t_rob), t_rob + np.where(clear_hit, err_t, 0.0)[rows, first], np.inf)
            others = clear_hit.copy()
            others[rows, first] = False
            with np.errstate(invalid='ignore'):
                threat = (open_ | others) & ~(t - err_t > horizon[:, None])
            row_id.append(np.where(np.isfinite(t_rob), first, -1))
            row_amb.append(threat.any(1))
        ids.append(np.concatenate(row_id))
        amb.append(np.concatenate(row_amb))
    return np.stack(ids), np.stack(amb)


def gathered(origins, directions, vertices, faces, ids):
    """(o, d, v0, v1, v2) [B,R,3] float64 of the pairs (ray, face ids); ids < 0 take face 0 (mask them)"""
    ids = np.asarray(ids)
    B, R = ids.shape
    out = [np.empty((B, R, 3)) for _ in range(5)]
    for b in range(B):
        f = np.where(ids[b] >= 0, ids[b], 0)
        c = PM.corners(vertices, faces, b)
        rows = (np.broadcast_to(np.asarray(_image(origins, b), np.float64), (R, 3)),
                np.broadcast_to(np.asarray(_image(directions, b), np.float64), (R, 3)), c[0][f], c[1][f], c[2][f])
        for dst, src in zip(out, rows):
            dst[b] = src
    return out


def pair_values(origins, directions, vertices, faces, ids, u=U):
    """For the pairs (ray, face ids): -> (t, w [B,R,3], bound_t, bound_w [B,R,3]) in float64 (garbage where ids < 0)"""
    o, d, v0, v1, v2 = gathered(origins, directions, vertices, faces, ids)
    tm = pair_terms(o, d, v0, v1, v2)
    s = np.where(tm['det'] < 0, -1.0, 1.0)
    D = np.abs(tm['det'])
    D1 = np.where(D > 0, D, 1.0)
    t, w1, w2 = s * tm['T'] / D1, s * tm['u'] / D1, s * tm['v'] / D1
    b_t = quotient_bound(tm['T'], tm['M_T'], D, tm['M_det'], u)
    b_1, b_2 = quotient_bound(tm['u'], tm['M_U'], D, tm['M_det'], u), quotient_bound(tm['v'], tm['M_V'], D, tm['M_det'], u)
    w = np.stack((np.maximum(1 - w1 - w2, 0.0), w1, w2), -1)
    return t, w, b_t, np.stack((b_1 + b_2 + 2 * u, b_1, b_2), -1)


def check_hits(t, ids, w, origins, directions, vertices, faces, near=0.0, far=np.inf, cull=False, u=U, what='', analysis=None):
    """The checks of a result (module docstring); prints and returns (share left out, worst t ratio, worst weight ratio)."""
    t, ids, w = np.asarray(t, np.float64), np.asarray(ids), np.asarray(w, np.float64)
    F = faces.shape[0]
    assert t.shape == ids.shape and w.shape == ids.shape + (3,), (t.shape, ids.shape, w.shape)
    assert ids.min() >= -1 and ids.max() < F, (what, int(ids.min()), int(ids.max()), F)
    want, amb = analysis if analysis is not None else analyse(origins, directions, vertices, faces, near, far, cull, u, ids.shape[0])
    share = float(amb.mean())
    hit = ids >= 0
    # a miss: +inf, -1, zeros; a hit: a finite t in range
    assert np.isposinf(t[~hit]).all() and (w[~hit] == 0).all(), what
    assert np.isfinite(t[hit]).all() and (t[hit] >= near).all() and (t[hit] < far).all(), what
    assert (w >= 0).all() and (np.abs(w[hit].sum(1) - 1) <= 4 * u).all(), (what, w.min())
    keep = ~amb
    assert share <= CAP, (what, share)
    assert np.array_equal(ids[keep], want[keep]), (what, int((ids[keep] != want[keep]).sum()))
    t64, w64, b_t, b_w = pair_values(origins, directions, vertices, faces, ids, u)
    r_t = PM._ratio(np.abs(t - t64)[hit], b_t[hit])
    r_w = PM._ratio(np.abs(w - w64)[hit], b_w[hit])
    print('%s left out %.4f hits %.3f t ratio %.4f weight ratio %.4f' % (what, share, float(hit.mean()), r_t, r_w))
    assert r_t <= 1.0 and r_w <= 1.0, (what, r_t, r_w)
    return share, r_t, r_w


def gradients(origins, directions, vertices, faces, ids, g, u=U):
    """The gradients of sum g t from the hits `ids` of the result under test, g [B,R]:
    -> ((grad_o, bound), (grad_d, bound), (grad_v [B,Nv,3], bound)), grad_o and grad_d per ray [B,R,3] with K = 1 -- a caller whose
    rays are shared sums them with `shared_sum`"""
    ids, g = np.asarray(ids), np.asarray(g, np.float64)
    B, R = ids.shape
    hit = ids >= 0
    o, d, v0, v1, v2 = gathered(origins, directions, vertices, faces, ids)
    e1, e2, a = v1 - v0, v2 - v0, v0 - o
    n, Mn = _cross(e1, e2), _xmag(e1, e2)
    Dn, N = _dot(d, n), _dot(a, n)
    Dn1 = np.where(hit & (Dn != 0), Dn, 1.0)
    M_Dn, M_N = _dot(np.abs(d), Mn), _dot(np.abs(a), Mn)
    rho, tau = M_Dn / np.abs(Dn1), M_N / np.abs(Dn1)
    t = N / Dn1
    gq = np.where(hit, g / Dn1, 0.0)[..., None]
    p = o + t[..., None] * d
    # the plane's weights of the hit point
    nn = np.where(hit, _dot(n, n), 1.0)[..., None]
    w1 = (_cross(p - v0, e2) * n).sum(-1, keepdims=True) / nn
    w2 = (_cross(e1, p - v0) * n).sum(-1, keepdims=True) / nn
    w0 = 1 - w1 - w2
    grad_o, grad_d = -gq * n, -gq * t[..., None] * n
    G = np.abs(gq) * (np.abs(a) + tau[..., None] * np.abs(d))
    mag_o = np.abs(gq) * Mn
    mag_d = np.abs(gq) * tau[..., None] * Mn
    mags = (_xmag(e2, G) + _xmag(e1, G) + mag_o, _xmag(e2, G), _xmag(e1, G))
    factor = np.where(hit, KG * rho + KE, 0.0)[..., None]
    Nv = np.asarray(vertices).shape[-2]
    gv, fv, mv, kv = np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3)), np.zeros((B, Nv), np.int64)
    for b in range(B):
        f = ids[b][hit[b]]
        for k, wk in enumerate((w0, w1, w2)):
            vk = faces[f, k]
            np.add.at(gv[b], vk, (wk[b] * gq[b] * n[b])[hit[b]])
            np.add.at(fv[b], vk, (factor[b] * mags[k][b])[hit[b]])
            np.add.at(mv[b], vk, mags[k][b][hit[b]])
            np.add.at(kv[b], vk, 1)
    bound_v = u * (fv + kv[..., None] * mv)
    return ((grad_o, u * (factor + 1) * mag_o), (grad_d, u * (factor + 1) * mag_d), (gv, bound_v))


def shared_sum(value, bound, axis, u=U):
    """the sum autograd takes over `axis` of per-ray gradients (rays shared by the batch: 0; one origin for the rays: 1): the
    bounds add, plus one accumulation per term on the terms' absolute values"""
    n = value.shape[axis]
    return value.sum(axis, keepdims=True), bound.sum(axis, keepdims=True) + n * u * np.abs(value).sum(axis, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# cases

def rays(seed, vertices, faces, R, shared=False):
    """(origins, directions) [B,R,3] float32 ([R,3] shared) over a mesh: two rays in three aimed from origins at |z| in [0.8, 2],
    x, y in [-1.5, 1.5], at interior points (weights >= 0.05) of random faces, the third with a random direction; all lengths
    scaled by [0.5, 2]"""
    rng = np.random.default_rng(seed)
    B = 1 if shared else vertices.shape[0]
    o = np.empty((B, R, 3), np.float32)
    d = np.empty((B, R, 3), np.float32)
    for b in range(B):
        v = vertices[b].astype(np.float64)
        org = np.concatenate((rng.uniform(-1.5, 1.5, (R, 2)), (rng.uniform(0.8, 2.0, R) * rng.choice((-1.0, 1.0), R))[:, None]), 1)
        f = rng.integers(0, faces.shape[0], R)
        w = 0.05 + 0.85 * rng.dirichlet((1, 1, 1), R)
        aimed = (w[:, :, None] * v[faces[f]]).sum(1) - org
        free = rng.normal(size=(R, 3))
        free /= np.linalg.norm(free, axis=1, keepdims=True)
        direction = np.where((np.arange(R) % 3 == 2)[:, None], free, aimed) * rng.uniform(0.5, 2.0, (R, 1))
        o[b], d[b] = org, direction
    return (o[0], d[0]) if shared else (o, d)


# ---------------------------------------------------------------------------------------------------------------------
# the rasterizer's depth at a pixel centre, for the cross-check of the two kernels

def raster_depth_bound(corners, eye, rot, tangent, S, xi, yi, zp, u=U):
    """The bound of the rasterizer's float32 depth at the pixel (column xi, internal row yi) of the face with world-space
    `corners` [n,3,3], against the exact depth zp [n] (float64), for the camera c = (v - eye) rot^T, x / z / tangent.  Counted
    on the chain of rasterize.py (nr_forward.hip): with m_k = sum_j |v_kj - eye_j|
      camera coordinates   a subtraction, a product, two additions, and the rotation's own entries (rebuilt in float32 by the
                           front-end and by camera_rays, a few u apart): eps_c = 8 u m_k
      NDC                  two quotients: eps_n = eps_c (1 + |ndc| tangent) / (z tangent) + 2 u |ndc|
      pixel units          P = 0.5 (ndc S + S - 1): eps_P = S eps_n / 2 + 3 u S
      weights              w_k = (a_k xi + b_k yi + c_k) / den, a_k = P_iy - P_jy, b_k = P_jx - P_ix, c_k = P_ix P_jy - P_jx P_iy: five
                           roundings on the magnitude Mnum_k = (|P_iy| + |P_jy|) xi + (|P_ix| + |P_jx|) yi + |P_ix P_jy| + |P_jx P_iy|,
                           and the corners' eps_P: eps_P (2 (xi + yi) + |P_i|_1 + |P_j|_1); den likewise, 4 u Mden + 2 eps_P sum |P_k|_1;
                           d_w_k = (d_num_k + |w_k| d_den) / (|den| - d_den)  -- on a face far below a pixel this is the large term
      clamp, normalise     d_w~_k = d_w_k + w_k sum_j d_w_j + 2 u; the normalised weights sum to 1 within 3 u on both sides
      zp = 1 / sum w~_k / z_k    sum_k d_w~_k |1 / z_k - 1 / zp| + sum_k w_k eps_c / z_k^2 + 7 u / zp on the sum, times zp^2, + u zp
    inf where the face is too small on the screen to bound (|den| <= d_den)."""
    corners, eye, rot = np.asarray(corners, np.float64), np.asarray(eye, np.float64), np.asarray(rot, np.float64)
    rel = corners - eye
    cam = rel @ rot.T
    m = np.abs(rel).sum(-1)
    z = cam[..., 2]
    eps_c = 8 * u * m
    ndc = cam[..., :2] / (z * tangent)[..., None]
    eps_n = (eps_c * (1 + np.abs(ndc).max(-1) * tangent) / (np.abs(z) * tangent)) + 2 * u * np.abs(ndc).max(-1)
    P = 0.5 * (ndc * S + S - 1)
    eps_P = (0.5 * S * eps_n + 3 * u * S).max(-1)
    xi, yi = np.asarray(xi, np.float64), np.asarray(yi, np.float64)
    l1 = np.abs(P).sum(-1)
    num, d_num = [], []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        a, b = P[:, i, 1] - P[:, j, 1], P[:, j, 0] - P[:, i, 0]
        c = P[:, i, 0] * P[:, j, 1] - P[:, j, 0] * P[:, i, 1]
        M = (np.abs(P[:, i, 1]) + np.abs(P[:, j, 1])) * xi + (np.abs(P[:, i, 0]) + np.abs(P[:, j, 0])) * yi \
            + np.abs(P[:, i, 0] * P[:, j, 1]) + np.abs(P[:, j, 0] * P[:, i, 1])
        num.append(a * xi + b * yi + c)
        d_num.append(5 * u * M + eps_P * (2 * (xi + yi) + l1[:, i] + l1[:, j]))
    num, d_num = np.stack(num, 1), np.stack(d_num, 1)
    den = num.sum(1)
    Mden = sum(np.abs(P[:, k, 0]) * (np.abs(P[:, (k + 1) % 3, 1]) + np.abs(P[:, (k + 2) % 3, 1])) for k in range(3))
    d_den = 4 * u * Mden + 2 * eps_P * l1.sum(1)
    room = np.abs(den) - d_den
    with np.errstate(divide='ignore', invalid='ignore'):
        w = num / den[:, None]
        d_w = (d_num + np.abs(w) * d_den[:, None]) / room[:, None]
        d_wn = d_w + np.abs(w) * d_w.sum(1, keepdims=True) + 2 * u
        zp = np.asarray(zp, np.float64)
        d_inv = (d_wn * np.abs(1 / z - 1 / zp[:, None])).sum(1) + (np.abs(w) * eps_c / z ** 2).sum(1) + 7 * u / zp
        bound = zp ** 2 * d_inv + u * zp
    return np.where(room > 0, bound, np.inf)


MISMATCH_CAP = 0.01


def check_depth_maps(depth, t, ids, bound_t, origins, directions, vertices, faces, eye, rot, tangent, S, far, what=''):
    """The rasterizer's depth maps [B,S,S] (`far` where nothing is drawn) against the rays through the pixel centres, t and ids
    [B,S*S] with their bounds: pixels where one side hits and the other does not, or where the depths differ by more than the
    bound of the two formulas, are at most MISMATCH_CAP of the image; -> (their share, the worst ratio elsewhere)"""
    depth, t, ids = np.asarray(depth, np.float64), np.asarray(t, np.float64), np.asarray(ids)
    B = ids.shape[0]
    depth = depth.reshape(B, S * S)
    drawn, hit = depth < far, ids >= 0
    both = drawn & hit
    o, d, v0, v1, v2 = gathered(origins, directions, vertices, faces, ids)
    t64 = pair_values(origins, directions, vertices, faces, ids)[0]
    ratio = np.zeros(ids.shape)
    rows, cols = np.divmod(np.arange(S * S), S)
    for b in range(B):
        k = both[b]
        corners = np.stack((v0[b][k], v1[b][k], v2[b][k]), 1)
        bound = raster_depth_bound(corners, np.asarray(eye, np.float64).reshape(-1, 3)[b if np.asarray(eye).ndim == 2 else 0],
                                   rot[b], tangent, S, cols[k], (S - 1 - rows)[k], t64[b][k]) + bound_t[b][k]
        with np.errstate(invalid='ignore'):
            ratio[b][k] = np.abs(depth[b][k] - t[b][k]) / bound
    bad = (drawn != hit) | (both & ~(ratio <= 1.0))
    share = float(bad.mean())
    worst = float(ratio[both & ~bad].max()) if (both & ~bad).any() else 0.0
    print('%s pixels drawn %.3f, mismatched %.4f, worst depth ratio elsewhere %.4f' % (what, float(drawn.mean()), share, worst))
    assert share <= MISMATCH_CAP, (what, share)
    return share, worst
