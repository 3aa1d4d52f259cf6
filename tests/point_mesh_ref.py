"""Float64 restatement of neural_renderer_amd/point_mesh.py (DESIGN "Point-to-mesh distance"), in NumPy, independent of the
product's code -- the yardstick of tests/test_point_mesh.py and test_point_mesh_gpu.py -- with the bounds, the lattice and the
case generators.  u = 2^-24 in float32, 2^-53 in float64.

The distance of a pair here: the minimum of the three edge segments and, when the triangle has a normal and the foot of the
perpendicular lies inside, the distance to the plane -- through cross products, where the product uses Gram-Schmidt.

dist2.  The error of a float32 closest-point chain is not relative to d^2: near the surface it is ~ u d L, L = |p - v0| + |e1| +
  |e2| of the face.  The bound of an entry is  K1 u (d^2 + d L) + K2 (u L)^2  -- the issue's k [u (d^2 + d L) + (u L)^2] with
  k = max(K1, K2), kept as two coefficients because it is tighter --, counted on the chain of csrc/nr_point_triangle.h:
  (i)   ap, ab, ac, e are one rounding each and bp = ap - ab one more: the point and the candidate's feature are displaced by
        at most 3 u L, so the distance by as much: 6 u d L + 9 (u L)^2;
  (ii)  a segment's parameter t = dot * (1 / |e|^2): the dot's three roundings (3 u |e| |q|), |e|^2's three, the reciprocal's and
        the product's (5 u t): the closest point moves along the edge by at most (3 |q| + 5 |e|) u <= 8 u L, and along a line
        the squared distance grows by the square of that: 64 (u L)^2.  The plane's point is (d1 / aa) ab + y g: along ab as a
        segment, 8 u L; along g by the dot's 3 u |ap| and by g's own rounding, |nu| <= 3 u |ac|, which enters y as
        nu . ap / |g|^2: (5 + 3 / s) u L with s = |g| / |ac| the sine of the angle at corner 0; both: (64 + (5 + 3 / s)^2) (u L)^2,
        260 for s >= 1/3, which the generators below guarantee.  A face below that (a collapsed one: s = 0) is covered by
        its segments: every candidate is the distance to a point OF the triangle, so the minimum of the four is never
        below the truth by more than (i), (iii), (iv) and never above the best segment;
  (iii) r: two products and two subtractions per component, |r^ - r| <= 2 u (L + d): 4 u d L + 4 u d^2 + 16 (u L)^2;
  (iv)  the dot r . r: three roundings on non-negative terms, 3 u d^2.
  K1 = 6 + 4 = 10 (>= 4 + 3), K2 = 9 + 260 + 16 = 285.  The plain-torch path recomputes r as ((p - v0) - w1 (v1 - v0)) - w2 (v2 - v0):
  the same counts.
ids.  A near-tie may resolve differently in float32, so the id is not compared: it must be in range, and the float64
  distance of the returned point, c = v0 + w1 (v1 - v0) + w2 (v2 - v0) -- the weights' defect from 1, at most 4 u, goes to corner
  0, as the bound is relative to the triangle and not to the coordinates --, within bound(nearest face) + bound(chosen face) of
  the float64 minimum: the chosen pair's float32 distance is at most the nearest's.  Weights: w_k >= 0, |sum - 1| <= 4 u.
loss.  The weighted sums in double, rounded once: the entries' bounds summed, plus (u + 2^-40) |loss|.
gradients.  Assignments are discontinuous, so ids and weights come from the result under test, after the checks above
  accepted them.  A term is coef * r_c, coef = 2 g (points) or -2 g w_k (vertices), r = ((p - v0) - w1 (v1 - v0)) - w2 (v2 - v0); its
  magnitude |coef| (|p - v0| + |w1 (v1 - v0)| + |w2 (v2 - v0)|)_c.  Roundings per term: r's four (a difference, a product, two
  subtractions at most), g's two (the loss's weight and its product with the upstream), w_k's product and the term's: 8; K
  terms add K accumulations in any order: (K + 8) u x the sum of the magnitudes."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
K1, K2 = 10.0, 285.0
MIN_SINE = 1.0 / 3.0
GRAD_EXTRA = 8


# ---------------------------------------------------------------------------------------------------------------------
# the distance

def _seg(p, u0, e):
    """[n,F] squared distance of p [n,3] to the segments u0 + t e, t in [0,1] ([F,3] each)"""
    q = p[:, None, :] - u0[None]
    ee = (e * e).sum(1)
    t = np.where(ee > 0, (q * e[None]).sum(2) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    r = q - t[..., None] * e[None]
    return (r * r).sum(2)


def pair_matrix(p, v0, v1, v2):
    """[n,F] float64 squared distances of the points p [n,3] to the triangles (v0, v1, v2) [F,3]"""
    p, v0, v1, v2 = (np.asarray(t, np.float64) for t in (p, v0, v1, v2))
    d = np.minimum(np.minimum(_seg(p, v0, v1 - v0), _seg(p, v0, v2 - v0)), _seg(p, v1, v2 - v1))
    n = np.cross(v1 - v0, v2 - v0)
    nn = (n * n).sum(1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    ap = p[:, None, :] - v0[None]
    w1 = (np.cross(ap, (v2 - v0)[None]) * n[None]).sum(2) / nn1
    w2 = (np.cross((v1 - v0)[None], ap) * n[None]).sum(2) / nn1
    inside = ok[None] & (w1 >= 0) & (w2 >= 0) & (w1 + w2 <= 1)
    plane = (ap * n[None]).sum(2) ** 2 / nn1
    return np.where(inside, np.minimum(d, plane), d)


def _image(t, b):
    return t if t.ndim == 2 else (t[0] if t.shape[0] == 1 else t[b])


def corners(vertices, faces, b):
    v = np.asarray(_image(vertices, b), np.float64)
    return v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]


def nearest(points, vertices, faces, to_points=False, B=None):
    """-> (d_min, argmin first occurrence): [B,N] over the faces, or with to_points [B,F] over the points"""
    B = B or max(1 if points.ndim == 2 else points.shape[0], 1 if vertices.ndim == 2 else vertices.shape[0])
    d_min, arg = [], []
    for b in range(B):
        p = np.asarray(_image(points, b), np.float64)
        v0, v1, v2 = corners(vertices, faces, b)
        dm, am = [], []
        for n0 in range(0, p.shape[0], 2048):
            m = pair_matrix(p[n0:n0 + 2048], v0, v1, v2)
            dm.append(m)
        m = np.concatenate(dm, 0)
        if to_points:
            m = m.T
        d_min.append(m.min(1))
        arg.append(m.argmin(1))
    return np.stack(d_min), np.stack(arg)


def pair_geometry(points, vertices, faces, point_of, face_of, w):
    """For the pairs (point point_of[b,r], face face_of[b,r]) with weights w [B,R,3] (float64 views of the result under test):
    -> (r [B,R,3] = (p - v0) - w1 e1 - w2 e2, its magnitude per component, L [B,R])"""
    w = np.asarray(w, np.float64)
    B = w.shape[0]
    r, mag, L = np.empty(w.shape), np.empty(w.shape), np.empty(w.shape[:2])
    for b in range(B):
        p = np.asarray(_image(points, b), np.float64)[point_of[b]]
        v0, v1, v2 = (c[face_of[b]] for c in corners(vertices, faces, b))
        a, e1, e2 = p - v0, v1 - v0, v2 - v0
        r[b] = a - w[b, :, 1:2] * e1 - w[b, :, 2:3] * e2
        mag[b] = np.abs(a) + np.abs(w[b, :, 1:2] * e1) + np.abs(w[b, :, 2:3] * e2)
        L[b] = np.linalg.norm(a, axis=1) + np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
    return r, mag, L


def bound(d2, L, u=U):
    d = np.sqrt(np.maximum(d2, 0.0))
    return K1 * u * (d2 + d * L) + K2 * (u * L) ** 2


def _ratio(err, bnd):
    err, bnd = np.asarray(err, np.float64), np.asarray(bnd, np.float64)
    r = np.where(err <= 0, 0.0, err / np.where(bnd > 0, bnd, np.nan))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def rows_and_ids(ids, to_points):
    """(point_of, face_of) [B,R] of the pairs of a result: rows are points (ids faces) or, to_points, faces (ids points)"""
    ids = np.asarray(ids)
    own = np.broadcast_to(np.arange(ids.shape[1])[None], ids.shape)
    return (ids, own) if to_points else (own, ids)


def check_closest(dist2, ids, w, points, vertices, faces, u=U, what='', to_points=False):
    """The checks of an entry (module docstring); prints and returns the two worst ratios (assignment, dist2)."""
    dist2, ids, w = np.asarray(dist2, np.float64), np.asarray(ids), np.asarray(w, np.float64)
    B = ids.shape[0]
    cols = (_image(points, 0).shape[0]) if to_points else faces.shape[0]
    assert dist2.shape == ids.shape and w.shape == ids.shape + (3,), (dist2.shape, ids.shape, w.shape)
    assert ids.min() >= 0 and ids.max() < cols, (what, int(ids.min()), int(ids.max()), cols)
    assert (w >= 0).all() and np.abs(w.sum(2) - 1).max() <= 4 * u, (what, w.min(), np.abs(w.sum(2) - 1).max())
    d_min, arg = nearest(points, vertices, faces, to_points, B)
    point_of, face_of = rows_and_ids(ids, to_points)
    r, _, L = pair_geometry(points, vertices, faces, point_of, face_of, w)
    d_c = (r * r).sum(2)
    pn, fn = rows_and_ids(arg, to_points)
    L_near = pair_geometry(points, vertices, faces, pn, fn, np.zeros(w.shape))[2]
    r_a = _ratio(d_c - d_min, bound(d_min, L_near, u) + bound(d_c, L, u))
    r_d = _ratio(np.abs(dist2 - d_c), bound(d_c, L, u))
    print('%s assignment ratio %.4f dist2 ratio %.4f' % (what, r_a, r_d))
    # (a point of the mesh is never nearer than the minimum, but for the weights' rounding: sum w <= 1 + 4 u)
    assert _ratio(d_min - d_c, bound(d_min, L_near, u)) <= 1.0, what
    assert r_a <= 1.0, (what, r_a)
    assert r_d <= 1.0, (what, r_d)
    return r_a, r_d


# ---------------------------------------------------------------------------------------------------------------------
# loss and gradients

def weights(N, F, reduction):
    return (1.0 / N, 1.0 / F) if reduction == 'mean' else (1.0, 1.0)


def loss(points, vertices, faces, direction, reduction, B=None, u=U):
    """-> (loss [B] float64 from the float64 minima, its bound)"""
    N, F = _image(points, 0).shape[0], faces.shape[0]
    wp, wf = weights(N, F, reduction)
    total, bnd = 0.0, 0.0
    for to_points, wgt in ((False, wp), (True, wf)):
        if direction in ('both', 'mesh_to_points' if to_points else 'points_to_mesh'):
            d_min, arg = nearest(points, vertices, faces, to_points, B)
            pn, fn = rows_and_ids(arg, to_points)
            L = pair_geometry(points, vertices, faces, pn, fn, np.zeros(arg.shape + (3,)))[2]
            total = total + wgt * d_min.sum(1)
            bnd = bnd + wgt * bound(d_min, L, u).sum(1)
    return total, bnd + (u + 2.0 ** -40) * np.abs(total)


def gradients(points, vertices, faces, surface, cloud, num_vertices):
    """The gradients of sum g dist2 from the pairs of the result under test: surface = (face_ids [B,N], w [B,N,3], g [B,N]) or
    None, cloud = (point_ids [B,F], w [B,F,3], g [B,F]) or None; points [B,N,3] batched.
    -> ((grad_points, magnitude, K [B,N]), (grad_vertices, magnitude, K [B,Nv]))"""
    some = surface if surface is not None else cloud
    B = np.asarray(some[0]).shape[0]
    N = _image(points, 0).shape[0]
    gp, mp, kp = np.zeros((B, N, 3)), np.zeros((B, N, 3)), np.zeros((B, N), np.int64)
    gv, mv, kv = np.zeros((B, num_vertices, 3)), np.zeros((B, num_vertices, 3)), np.zeros((B, num_vertices), np.int64)
    for part, to_points in ((surface, False), (cloud, True)):
        if part is None:
            continue
        ids, w, g = np.asarray(part[0]), np.asarray(part[1], np.float64), np.asarray(part[2], np.float64)
        point_of, face_of = rows_and_ids(ids, to_points)
        r, mag, _ = pair_geometry(points, vertices, faces, point_of, face_of, w)
        for b in range(B):
            t = 2 * g[b][:, None] * r[b]
            m = 2 * np.abs(g[b])[:, None] * mag[b]
            np.add.at(gp[b], point_of[b], t)
            np.add.at(mp[b], point_of[b], m)
            np.add.at(kp[b], point_of[b], 1)
            for k in range(3):
                vk = faces[face_of[b], k]
                np.add.at(gv[b], vk, -w[b, :, k:k + 1] * t)
                np.add.at(mv[b], vk, w[b, :, k:k + 1] * m)
                np.add.at(kv[b], vk, 1)
    return (gp, mp, kp), (gv, mv, kv)


def gradient_ratio(got, value, mag, K, u=U):
    """the worst |got - value| / ((K + GRAD_EXTRA) u magnitude) over the entries (0 / 0 counts as 0)"""
    return _ratio(np.abs(np.asarray(got, np.float64) - value), (K[..., None] + GRAD_EXTRA) * u * mag)


# ---------------------------------------------------------------------------------------------------------------------
# cases

def corner_sine(v0, v1, v2):
    """the sine of the angle at corner 0 of every face"""
    e1, e2 = np.asarray(v1, np.float64) - v0, np.asarray(v2, np.float64) - v0
    den = np.linalg.norm(e1, axis=-1) * np.linalg.norm(e2, axis=-1)
    return np.linalg.norm(np.cross(e1, e2), axis=-1) / np.where(den > 0, den, 1.0)


def grid_mesh(seed, B, F):
    """A jittered height field cut into triangles, the first F of them: vertices [B,Nv,3] float32 (shared corners, and with
    F odd or small some vertices in no face), faces [F,3] int32; every corner-0 sine >= MIN_SINE (asserted)."""
    rng = np.random.default_rng(seed)
    n = int(np.ceil(np.sqrt((F + 1) // 2))) + 1
    h = 2.0 / (n - 1)
    gx, gy = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing='ij')
    base = np.stack((gx, gy, 0.3 * np.sin(2 * gx) * np.cos(3 * gy)), -1).reshape(-1, 3)
    v = (base[None] + rng.uniform(-0.15 * h, 0.15 * h, (B, n * n, 3))).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.stack((np.stack((a, b, c), 1), np.stack((a, c, d), 1)), 1).reshape(-1, 3)[:F].astype(np.int32)
    assert faces.shape[0] == F
    for i in range(B):
        assert corner_sine(v[i][faces[:, 0]], v[i][faces[:, 1]], v[i][faces[:, 2]]).min() >= MIN_SINE
    return v, faces


def cloud_near(seed, vertices, faces, N, shared=False):
    """points [B,N,3] float32 (or [N,3]): random points of random faces moved off the surface by 1, 0.05 and 1e-3 in turn"""
    rng = np.random.default_rng(seed)
    B = 1 if shared else vertices.shape[0]
    out = np.empty((B, N, 3), np.float32)
    for b in range(B):
        f = rng.integers(0, faces.shape[0], N)
        w = rng.dirichlet((1, 1, 1), N)
        v = vertices[b].astype(np.float64)
        c = (w[:, :, None] * v[faces[f]]).sum(1)
        direction = rng.normal(size=(N, 3))
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        out[b] = c + np.array([1.0, 0.05, 1e-3])[np.arange(N) % 3][:, None] * direction
    return out[0] if shared else out


def triangle_soup(seed, F):
    """F random triangles, centres in [-1,1]^3 and corners within +-0.15, corner-0 sine >= MIN_SINE: vertices [1,3F,3], faces"""
    rng = np.random.default_rng(seed)
    tris = []
    while len(tris) < F:
        t = rng.uniform(-1, 1, (1, 3)) + rng.uniform(-0.15, 0.15, (3, 3))
        t = t.astype(np.float32)
        if corner_sine(t[0], t[1], t[2]) >= MIN_SINE:
            tris.append(t)
    return np.concatenate(tris)[None], np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def lattice():
    """The surface of the cube [-4,4]^3, every side cut into 2 x 2 squares of side 4 and each square into two right triangles:
    26 vertices, 48 faces; and 300 integer points of [-6,6]^3.  Every leg is 4, every hypotenuse^2 32, so every float32
    operation of the chain is exact.  -> (points [300,3], vertices [26,3], faces [48,3])"""
    coords = (-4.0, 0.0, 4.0)
    index, verts = {}, []
    for x in coords:
        for y in coords:
            for z in coords:
                if max(abs(x), abs(y), abs(z)) == 4.0:
                    index[(x, y, z)] = len(verts)
                    verts.append((x, y, z))
    faces = []
    for axis in range(3):
        for side in (-4.0, 4.0):
            for i in range(2):
                for j in range(2):
                    def at(di, dj):
                        c = [0.0, 0.0, 0.0]
                        c[axis] = side
                        c[(axis + 1) % 3] = coords[i + di]
                        c[(axis + 2) % 3] = coords[j + dj]
                        return index[tuple(c)]
                    faces.append((at(0, 0), at(1, 0), at(1, 1)))
                    faces.append((at(0, 0), at(1, 1), at(0, 1)))
    points = np.random.default_rng(0).integers(-6, 7, (300, 3)).astype(np.float32)
    return points, np.array(verts, np.float32), np.array(faces, np.int32)


def tied_rows(m):
    """the number of rows of the matrix m whose minimum is attained more than once"""
    return int(((m == m.min(1, keepdims=True)).sum(1) > 1).sum())


def collapsed_faces(seed=3):
    """The six shapes (a,a,a), (a,b,a), (a,a,b), (a,b,b), (a,b,midpoint), (a, a/4 + 3b/4, b) as a mesh of their own:
    vertices [1,18,3] float32, faces [6,3]"""
    rng = np.random.default_rng(seed)
    tris = []
    for shape in range(6):
        a, b = rng.uniform(-1, 1, 3).astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32)
        mid, q = (0.5 * (a + b)).astype(np.float32), (0.25 * a + 0.75 * b).astype(np.float32)
        tris.append([(a, a, a), (a, b, a), (a, a, b), (a, b, b), (a, b, mid), (a, q, b)][shape])
    v = np.array(tris, np.float32).reshape(1, 18, 3)
    return v, np.arange(18, dtype=np.int32).reshape(6, 3)


def with_collapsed(vertices, faces, seed=5):
    """the mesh with the six collapsed shapes spliced in among its faces (their corners taken from its own vertices where the
    shape allows: a and b are vertices of the mesh, the two inner points are appended)"""
    rng = np.random.default_rng(seed)
    B, Nv = vertices.shape[:2]
    ia, ib = (int(i) for i in rng.choice(Nv, 2, replace=False))
    a, b = vertices[:, ia], vertices[:, ib]
    extra = np.stack(((0.5 * (a + b)).astype(np.float32), (0.25 * a + 0.75 * b).astype(np.float32)), 1)
    v = np.concatenate((vertices, extra), 1)
    new = np.array([(ia, ia, ia), (ia, ib, ia), (ia, ia, ib), (ia, ib, ib), (ia, ib, Nv), (ia, Nv + 1, ib)], np.int32)
    where = np.sort(rng.choice(faces.shape[0] + 1, 6))
    return v, np.insert(faces, where, new, axis=0)
