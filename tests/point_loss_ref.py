"""Float64 restatement of neural_renderer_amd/point_losses.py (DESIGN "Point-cloud losses"), in NumPy with dense matrices and
plain loops, independent of the product's code -- the yardstick of tests/test_point_losses.py and test_point_losses_gpu.py --
and the error bounds of the float32 kernels, each derived from the operation chain, none tuned.  u = 2^-24.

dist2.  d = fma(dx, dx, fma(dy, dy, dz dz)) of dx = fl(x - y): the dz term carries its difference's rounding twice
  (squared), its product's and the two fused additions': (1 + u)^5, the other terms fewer.  All terms are non-negative, so
  |d^ - d| <= gamma_5 d with gamma_k = k u / (1 - k u).  The minimum over j of perturbed values lies within the same factor
  of the minimum, so the bound holds against the float64 minimum.  (The unfused chain of the torch path: the same count.)
idx.  A near-tie may legitimately resolve differently in float32, so the index is not compared: it must lie in [0, M), and
  the float64 distance to the chosen point must be within 2 gamma_5 d_min of the float64 minimum (the chosen point's float32
  distance is at most the true nearest's: d_k (1 - gamma_5) <= d_min (1 + gamma_5)).
loss.  wx sum_i d^_i + wy sum_j d^_j in double, rounded once: gamma_5 L + u L (1 + gamma_5), plus 2^-40 L for the double sums.
gradients.  They are discontinuous in the assignment, so the restatement takes the assignments a, c from the result under
  test (after the idx check accepted them).  An entry with K scattered terms is acc = s_own (p - o_a), then K fused
  multiply-adds of s_j (p - o_j): every term carries its coefficient's rounding (1) and its difference's (1), the first its
  product's (1), and each of the K accumulations one rounding of a partial sum that the entry's magnitude -- the sum of the
  absolute terms -- bounds: (K + 3) u x magnitude.
surface points.  fma(w2, v2, fma(w1, v1, w0 v0)): 3 roundings, 3 u x (|w0 v0| + |w1 v1| + |w2 v2|).  A vertex entry: `terms`
  fused multiply-adds from 0, (terms + 2) u x magnitude (terms u would do; the slack is the issue's).
The plain-torch path in float32 has its own chain: a coefficient (1), a difference (1), a product (1), K accumulations and
  one addition of the own term to the scattered sum: (K + 4) u; for surface points products and two additions, 3 u, and for
  their vertex entries a product and an accumulation per term, (terms + 2) u.  In float64 the same with u = 2^-53."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


# ---------------------------------------------------------------------------------------------------------------------
# test data

def clouds(seed, B, N, M, shared_y=False):
    """x [B,N,3], y [B,M,3] (or [M,3]) float32: points of the unit cube, y around x so that distances spread over decades"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (M, 3) if shared_y else (B, M, 3)).astype(np.float32)
    return x, y


def lattice(seed=7, N=300, M=517):
    """Integer coordinates in [-8, 8]: every float32 operation of the distance is exact, and many rows have tied minima."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, (N, 3)).astype(np.float32), rng.integers(-8, 9, (M, 3)).astype(np.float32))


def tied_rows(x, y):
    """the number of rows of x whose minimum is attained more than once"""
    d = dist_matrix(x, y)
    return int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())


def lattice_scatter(seed=11, few=7, many=600):
    """`few` integer points far apart and `many` integer points around them: every one of the many has one of the few as its
    nearest (long scatter lists, K near many / few), and each of the few one of the many."""
    rng = np.random.default_rng(seed)
    centres = (np.array([[i % 2, (i // 2) % 2, i // 4] for i in range(few)]) * 40 - 20).astype(np.float32)
    owner = rng.integers(0, few, many)
    pts = centres[owner] + rng.integers(-6, 7, (many, 3)).astype(np.float32)
    return centres, pts.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# nearest neighbour

def dist_matrix(x, y):
    """[N,M] float64 squared distances of x [N,3] and y [M,3]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    for n0 in range(0, x.shape[0], 4096):
        d = x[n0:n0 + 4096, None, :] - y[None, :, :]
        out[n0:n0 + 4096] = (d * d).sum(2)
    return out


def _image(y, b):
    return y if y.ndim == 2 else (y[0] if y.shape[0] == 1 else y[b])


def nearest(x, y):
    """-> (d_min [B,N] float64, argmin [B,N], first occurrence) for x [B,N,3], y [B,M,3] | [1,M,3] | [M,3]"""
    d_min, arg = np.empty(x.shape[:2]), np.empty(x.shape[:2], np.int64)
    for b in range(x.shape[0]):
        for n0 in range(0, x.shape[1], 4096):  # (rows of the matrix in blocks: the whole of it need not fit)
            m = dist_matrix(x[b, n0:n0 + 4096], _image(y, b))
            d_min[b, n0:n0 + 4096], arg[b, n0:n0 + 4096] = m.min(1), m.argmin(1)
    return d_min, arg


def chosen_distance(x, y, idx):
    """float64 squared distance of every x to the y it was given: [B,N]"""
    out = np.empty(idx.shape)
    for b in range(x.shape[0]):
        diff = x[b].astype(np.float64) - _image(y, b).astype(np.float64)[idx[b]]
        out[b] = (diff * diff).sum(1)
    return out


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.nan))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def check_assignment(idx, x, y, u=U, what=''):
    """idx [B,N] in [0, M), and the float64 distance to the chosen point within 2 gamma_5 d_min of the float64 minimum.
    -> (the worst ratio to that bound, d_min)"""
    M = _image(y, 0).shape[0]
    idx = np.asarray(idx)
    assert idx.shape == x.shape[:2], (idx.shape, x.shape)
    assert idx.min() >= 0 and idx.max() < M, (what, int(idx.min()), int(idx.max()), M)
    d_min, _ = nearest(x, y)
    r_i = _ratio(chosen_distance(x, y, idx) - d_min, 2 * gamma(5, u) * d_min)
    assert r_i <= 1.0, (what, r_i)
    return r_i, d_min


def check_nearest(dist2, idx, x, y, u=U, what=''):
    """dist2 within gamma_5 d_min of the float64 minimum, and check_assignment.  Prints and returns the two worst ratios."""
    assert np.asarray(dist2).shape == x.shape[:2], np.asarray(dist2).shape
    r_i, d_min = check_assignment(idx, x, y, u, what)
    r_d = _ratio(np.abs(np.asarray(dist2, np.float64) - d_min), gamma(5, u) * d_min)
    print('%s dist2 ratio %.3f idx ratio %.3f' % (what, r_d, r_i))
    assert r_d <= 1.0, (what, r_d)
    return r_d, r_i


# ---------------------------------------------------------------------------------------------------------------------
# chamfer

def weights(N, M, reduction):
    return (1.0 / N, 1.0 / M) if reduction == 'mean' else (1.0, 1.0)


def chamfer_loss(x, y, direction, reduction):
    """-> loss [B] float64 from the float64 minima"""
    B, N = x.shape[:2]
    M = _image(y, 0).shape[0]
    wx, wy = weights(N, M, reduction)
    loss = np.zeros(B)
    if direction in ('both', 'x_to_y'):
        loss += wx * nearest(x, y)[0].sum(1)
    if direction in ('both', 'y_to_x'):
        yb = np.stack([_image(y, b) for b in range(B)])
        loss += wy * nearest(yb, x)[0].sum(1)
    return loss


def loss_bound(loss, u=U):
    return (gamma(5, u) + u * (1 + gamma(5, u)) + 2.0 ** -40) * np.abs(loss)


def side_gradient(P, O, own, other, s_own, s_oth):
    """The gradient of cloud P [Np,3] against O [No,3] of ONE image: own [Np] = a(i) or None, other [No] = c(j) or None,
    s_own [Np] / s_oth [No] the float64 coefficients (2 w g).  -> (value [Np,3], magnitude [Np,3], K [Np])."""
    P, O = np.asarray(P, np.float64), np.asarray(O, np.float64)
    value, mag, K = np.zeros(P.shape), np.zeros(P.shape), np.zeros(P.shape[0], np.int64)
    if own is not None:
        t = np.asarray(s_own)[:, None] * (P - O[own])
        value += t
        mag += np.abs(t)
    if other is not None:
        t = np.asarray(s_oth)[:, None] * (P[other] - O)
        np.add.at(value, other, t)  # (unbuffered: repeated indices all count)
        np.add.at(mag, other, np.abs(t))
        K = np.bincount(other, minlength=P.shape[0])
    return value, mag, K


def chamfer_gradients(x, y, a, c, direction, reduction, gl):
    """From the assignments of the result under test (a [B,N] or None, c [B,M] or None) and the upstream gl [B]:
    -> ((grad_x, mag_x, K_x), (grad_y, mag_y, K_y)), each [B,.,3] / [B,.]; y batched [B,M,3]."""
    B, N = x.shape[:2]
    M = y.shape[1]
    wx, wy = weights(N, M, reduction)
    xy, yx = direction in ('both', 'x_to_y'), direction in ('both', 'y_to_x')
    gx, gy = [], []
    for b in range(B):
        sx, sy = np.full(N, 2 * wx * float(gl[b])), np.full(M, 2 * wy * float(gl[b]))
        gx.append(side_gradient(x[b], y[b], a[b] if xy else None, c[b] if yx else None, sx, sy))
        gy.append(side_gradient(y[b], x[b], c[b] if yx else None, a[b] if xy else None, sy, sx))
    return tuple(tuple(np.stack([g[k] for g in side]) for k in range(3)) for side in (gx, gy))


def gradient_ratio(got, value, mag, K, extra=3, u=U):
    """the worst |got - value| / ((K + extra) u magnitude) over the entries"""
    return _ratio(np.abs(np.asarray(got, np.float64) - value), (K[..., None] + extra) * u * mag)


def scatter_emulated(P, O, own, other, s_own, s_oth):
    """side_gradient in the kernel's float32 order -- acc = s_own (p - o_a), then fma(s_j, p - o_j, acc) for j ASCENDING --
    emulated in float64, for LATTICE data only: with integer coordinates every difference is exact, a product s d has at most
    29 significant bits, and acc and the products are multiples of one grid (the ulp of s) below 2^12 |s|, so s d + acc is
    exact in float64 and one rounding to float32 is the fused multiply-add's.  s_own / s_oth: float32 scalars."""
    P, O = np.asarray(P, np.float64), np.asarray(O, np.float64)
    acc = np.zeros(P.shape, np.float32)
    if own is not None:
        acc = (np.float64(s_own) * (P - O[own])).astype(np.float32)
    if other is not None:
        for j in range(O.shape[0]):
            i = other[j]
            acc[i] = (np.float64(s_oth) * (P[i] - O[j]) + acc[i].astype(np.float64)).astype(np.float32)
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# surface points

MESHES = {
    # a square of two faces, a third face on its own and vertex 7 in no face
    'patch': (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 2], [9, 9, 9]], np.float32),
              np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)),
}


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def given_samples(seed, B, N, num_faces, only_face=None, skip_face=None):
    """face ids [B,N] ascending and barycentric weights [B,N,3] float32 as sample_surface makes them"""
    rng = np.random.default_rng(seed)
    allowed = [f for f in range(num_faces) if f != skip_face] if only_face is None else [only_face]
    ids = np.sort(rng.choice(allowed, (B, N)), axis=1).astype(np.int32)
    r = rng.uniform(0, 1, (B, N, 2)).astype(np.float32)
    s = np.sqrt(r[..., 0])
    w = np.stack((1 - s, s * (1 - r[..., 1]), s * r[..., 1]), axis=2).astype(np.float32)
    return ids, w


def surface_points(vertices, faces, ids, w):
    """-> (points [B,N,3], magnitude) float64 for vertices [B,Nv,3]"""
    v, w = np.asarray(vertices, np.float64), np.asarray(w, np.float64)
    value, mag = np.zeros(ids.shape + (3,)), np.zeros(ids.shape + (3,))
    for b in range(ids.shape[0]):
        for n in range(ids.shape[1]):
            for k in range(3):
                t = w[b, n, k] * v[b, faces[ids[b, n], k]]
                value[b, n] += t
                mag[b, n] += np.abs(t)
    return value, mag


def surface_gradients(faces, ids, w, g, num_vertices):
    """-> (grad_vertices [B,Nv,3], magnitude, terms [B,Nv]) float64 for the upstream g [B,N,3]"""
    w, g = np.asarray(w, np.float64), np.asarray(g, np.float64)
    B, N = ids.shape
    value, mag = np.zeros((B, num_vertices, 3)), np.zeros((B, num_vertices, 3))
    terms = np.zeros((B, num_vertices), np.int64)
    for b in range(B):
        for n in range(N):
            for k in range(3):
                v = faces[ids[b, n], k]
                t = w[b, n, k] * g[b, n]
                value[b, v] += t
                mag[b, v] += np.abs(t)
                terms[b, v] += 1
    return value, mag, terms


def check_samples(ids, w, offsets, num_faces, u=U):
    """The structure of a SurfaceSamples: ids in range and ascending, weights non-negative and summing to 1 within 2 u,
    offsets consistent with the ids."""
    ids, w, offsets = np.asarray(ids), np.asarray(w, np.float64), np.asarray(offsets)
    assert ids.min() >= 0 and ids.max() < num_faces
    assert (np.diff(ids, axis=1) >= 0).all()
    assert (w >= 0).all() and np.abs(w.sum(2) - 1).max() <= 2 * u, np.abs(w.sum(2) - 1).max()
    assert offsets.shape == (ids.shape[0], num_faces + 1)
    for b in range(ids.shape[0]):
        assert np.array_equal(offsets[b], np.concatenate(([0], np.cumsum(np.bincount(ids[b], minlength=num_faces)))))
