"""Float64 restatement of neural_renderer_amd/winding.py (DESIGN "Winding numbers"), in NumPy, independent of the product's code
-- the yardstick of tests/test_winding.py and test_winding_gpu.py -- with the bounds and the case generators.  u = 2^-24 in
float32, 2^-53 in float64.

A pair: A = v0 - p, B = v1 - p, C = v2 - p, num = A . (B x C), den = la lb lc + (A.B) lc + (B.C) la + (C.A) lb, Omega = 2 atan2(num,
den).  M = la lb lc, h = hypot(num, den), c = M / h: the conditioning of the angle -- the errors of num and den are relative to
M, not to themselves, and the angle moves by hypot(dnum, dden) / h <= (|dnum| + |dden|) / h.

w.  bound = (1 / 4 pi) sum_f u (K1 c_f + K2 |Omega_f|) + u |w|, counted on the chain of csrc/nr_solid_angle.h (first order in u):
  A, B, C        one rounding per component.
  n = B x C      a component is a difference of two products: inputs 2, product 1, difference 1: 4 u (|B_j C_k| + |B_k C_j|), and
                 |B_j C_k| + |B_k C_j| <= sqrt(B_j^2 + B_k^2) sqrt(C_j^2 + C_k^2) <= lb lc.
  num            (A0 n0 + A1 n1) + A2 n2: n's 4, A's 1, the product's 1, two additions: 8 u sum_c |A_c| lb lc <= 8 sqrt(3) u M:
                 KNUM = 13.9.
  la             dot(A, A): the components' 2, the product's 1, two additions 2: 5 u on positive terms; the root halves it and
                 rounds once: 3.5 u.
  den            (la lb) lc: 3 x 3.5 + 2 = 12.5 u M.  ab = dot(A, B): inputs 2, product 1, additions 2: 5 u la lb; ab lc adds lc's
                 3.5 and the product's 1 on |ab| <= la lb: 9.5 u M, three times.  The three additions round sums of at most 2 M, 3 M
                 and 4 M: 9 u M.  KDEN = 12.5 + 28.5 + 9 = 50.
  K1 = 2 (KNUM + KDEN) = 127.8 (Omega = 2 atan2).  K2 is atan2f's own error relative to the angle (the doubling is exact, the
  sums are in double, the final scaling and rounding are the u |w|).  ROCm's installed headers and documents state no
  accuracy for the device function, so the CPU libm's documented bound is the source: glibc's manual ("Known Maximum Errors
  in Math Functions") lists atan2f at 2 ulp on x86_64 at the most.  Doubled, because the device library is another
  implementation: 4 ulp = 8 u relative: K2 = 8.
  The bound is meaningful only away from the surface: `winding` callers assert bound <= MAX_BOUND = 1e-2, a hundredth of the
  inside / outside step, on every entry -- a condition on the inputs.

gradients.  g_A = kn (B x C) - kd dA, kn = 2 den / s, kd = 2 num / s, s = h^2, dA = ((A / la) (lb lc + B.C) + B lc) + C lb; the natural
  size of corner A's gradient is G_A = 2 lb lc / h (cyclic), and a component's error is u G_A (K3 c + K4):
  s              ds / s <= 2 (KNUM + KDEN) u c + 3 u.
  kn, kd         |dkn| <= (2 / h) u (KDEN c + 2 (KNUM + KDEN) c + 5), |dkd| <= (2 / h) u (KNUM c + 2 (KNUM + KDEN) c + 5).
  dA             1 / la: 4.5; (A / la): 6.5; ma = lb lc + B.C: 15 u lb lc; (A / la) ma: 30 u lb lc; B lc and C lb: 5.5 u lb lc each; two
                 additions of at most 3 and 4 lb lc: 7: 48 u lb lc, and |dA_c| <= 4 lb lc.
  g_A            dkn |n| + |kn| dn + dkd |dA| + |kd| ddA + 3 u (|kn n| + |kd dA|)
                 <= u G_A [(KDEN + 2 S) c + 5 + 6 + 4 ((KNUM + 2 S) c + 5) + 48 + 15], S = KNUM + KDEN:
                 K3 = (KDEN + 2 S) + 4 (KNUM + 2 S) = 177.7 + 566.3 = 744.0, K4 = 94; and |g_A,c| <= 5 G_A.
  grad_points    -((g_A + g_B) + g_C): two additions on at most 5 (G_A + G_B + G_C): + 10; the sum over the faces in double, times
                 g / 4 pi (one product in double, one rounding): (|g| / 4 pi) sum_f u (K3 c_f + K4 + 10) (G_A + G_B + G_C) + 2 u |value|.
  grad_vertices  a corner's term g_i g_k,c: the product's rounding on at most 5 G_k: + 5; summed over the points in double, scaled
                 and rounded once (u |corner|), then the corners of a vertex are added in float32 in table order: deg(v) u sum
                 |corner|.  bound = sum over the corners (f, k) of v of [(1 / 4 pi) sum_i |g_i| u (K3 c_fi + K4 + 5) G_k,fi +
                 u |corner|] + deg(v) u sum |corner|.
A face with two corners equal as positions contributes nothing; num = den = 0 gives Omega = 0 and no gradient; la = 0 uses A / la
:= 0."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
KNUM, KDEN = 8.0 * np.sqrt(3.0), 50.0
K1, K2 = 2.0 * (KNUM + KDEN), 8.0
K3 = (KDEN + 2.0 * (KNUM + KDEN)) + 4.0 * (KNUM + 2.0 * (KNUM + KDEN))
K4 = 94.0
MAX_BOUND = 1e-2
INV_4PI = 1.0 / (4.0 * np.pi)
CHUNK = 512


def _image(t, b):
    return t if t.ndim == 2 else (t[0] if t.shape[0] == 1 else t[b])


def corners(vertices, faces, b):
    v = np.asarray(_image(vertices, b), np.float64)
    return v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]


def skipped(v0, v1, v2):
    return (v0 == v1).all(1) | (v1 == v2).all(1) | (v2 == v0).all(1)


class Pairs(object):
    """the pair quantities of points p [n,3] and corners [F,3] in float64: arrays [n,F] or [n,F,3]"""

    def __init__(self, p, v0, v1, v2):
        p = np.asarray(p, np.float64)[:, None, :]
        self.A, self.B, self.C = v0[None] - p, v1[None] - p, v2[None] - p
        self.la, self.lb, self.lc = (np.linalg.norm(t, axis=2) for t in (self.A, self.B, self.C))
        self.num = (self.A * np.cross(self.B, self.C)).sum(2)
        self.ab, self.bc, self.ca = (self.A * self.B).sum(2), (self.B * self.C).sum(2), (self.C * self.A).sum(2)
        self.M = self.la * self.lb * self.lc
        self.den = self.M + self.ab * self.lc + self.bc * self.la + self.ca * self.lb
        self.h = np.hypot(self.num, self.den)
        self.keep = ~skipped(v0, v1, v2)[None] & np.ones(self.h.shape, bool)

    def omega(self):
        return np.where(self.keep & (self.h != 0), 2.0 * np.arctan2(self.num, self.den), 0.0)  # (a NaN stays a NaN)

    def conditioning(self):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(self.keep, np.where(self.h != 0, self.M / self.h, np.inf), 0.0)

    def gradient(self):
        """-> (g [3][n,F,3]: dOmega/dv_k, G [3][n,F]: 2 l l / h of corner k); zeros on skipped faces and where h = 0"""
        ok = self.keep & (self.h != 0)
        s = np.where(ok, self.h ** 2, 1.0)
        kn, kd = (2.0 * self.den / s)[..., None], (2.0 * self.num / s)[..., None]
        out, size = [], []
        for (X, lx), (Y, ly), (Z, lz), yz in (((self.A, self.la), (self.B, self.lb), (self.C, self.lc), self.bc),
                                               ((self.B, self.lb), (self.C, self.lc), (self.A, self.la), self.ca),
                                               ((self.C, self.lc), (self.A, self.la), (self.B, self.lb), self.ab)):
            unit = X * np.where(lx > 0, 1.0 / np.where(lx > 0, lx, 1.0), 0.0)[..., None]
            dden = unit * (ly * lz + yz)[..., None] + Y * lz[..., None] + Z * ly[..., None]
            out.append(np.where(ok[..., None], kn * np.cross(Y, Z) - kd * dden, 0.0))
            size.append(np.where(ok, 2.0 * ly * lz / np.where(ok, self.h, 1.0), 0.0))
        return out, size


def _batch(points, vertices):
    return max(1 if points.ndim == 2 else points.shape[0], 1 if vertices.ndim == 2 else vertices.shape[0])


def winding(points, vertices, faces, u=U):
    """-> (w [B,N] float64, bound [B,N])"""
    B = _batch(points, vertices)
    w, bnd = [], []
    for b in range(B):
        p = np.asarray(_image(points, b), np.float64)
        v0, v1, v2 = corners(vertices, faces, b)
        wb, bb = np.empty(p.shape[0]), np.empty(p.shape[0])
        for n0 in range(0, p.shape[0], CHUNK):
            P = Pairs(p[n0:n0 + CHUNK], v0, v1, v2)
            om = P.omega()
            wb[n0:n0 + CHUNK] = om.sum(1) * INV_4PI
            bb[n0:n0 + CHUNK] = INV_4PI * u * (K1 * P.conditioning() + K2 * np.abs(om)).sum(1)
        w.append(wb)
        bnd.append(bb + u * np.abs(wb))
    return np.stack(w), np.stack(bnd)


def gradients(points, vertices, faces, g, num_vertices, u=U):
    """The gradients of sum g w for upstream g [B,N]; points [B,N,3] batched (broadcast a shared cloud first).
    -> ((grad_points [B,N,3], bound), (grad_vertices [B,Nv,3], bound))"""
    g = np.asarray(g, np.float64)
    B, N = g.shape
    F = faces.shape[0]
    gp, bp = np.zeros((B, N, 3)), np.zeros((B, N, 3))
    gv, bv = np.zeros((B, num_vertices, 3)), np.zeros((B, num_vertices, 3))
    degree = np.bincount(faces.reshape(-1), minlength=num_vertices).astype(np.float64)
    for b in range(B):
        p = np.asarray(_image(points, b), np.float64)
        v0, v1, v2 = corners(vertices, faces, b)
        corner, cb = np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
        for n0 in range(0, N, CHUNK):
            P = Pairs(p[n0:n0 + CHUNK], v0, v1, v2)
            gk, size = P.gradient()
            c = np.where(np.isfinite(P.conditioning()), P.conditioning(), 0.0)
            gb = g[b, n0:n0 + CHUNK]
            gp[b, n0:n0 + CHUNK] = -(gk[0] + gk[1] + gk[2]).sum(1) * (gb * INV_4PI)[:, None]
            bp[b, n0:n0 + CHUNK] = ((np.abs(gb) * INV_4PI * u)[:, None]
                                    * ((K3 * c + K4 + 10.0) * (size[0] + size[1] + size[2])).sum(1)[:, None])
            for k in range(3):
                corner[:, k] += (gb[:, None, None] * gk[k]).sum(0) * INV_4PI
                cb[:, k] += ((np.abs(gb)[:, None] * INV_4PI * u) * (K3 * c + K4 + 5.0) * size[k]).sum(0)[:, None]
        bp[b] += 2.0 * u * np.abs(gp[b])
        cb += u * np.abs(corner)
        flat = faces.reshape(-1)
        np.add.at(gv[b], flat, corner.reshape(3 * F, 3))
        np.add.at(bv[b], flat, cb.reshape(3 * F, 3))
        mag = np.zeros((num_vertices, 3))
        np.add.at(mag, flat, np.abs(corner).reshape(3 * F, 3))
        bv[b] += degree[:, None] * u * mag
    return (gp, bp), (gv, bv)


def ratio(got, value, bnd):
    """the worst |got - value| / bound over the entries (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, np.float64) - value)
    bnd = np.broadcast_to(np.asarray(bnd, np.float64), err.shape)
    r = np.where(err <= 0, 0.0, err / np.where(bnd > 0, bnd, np.nan))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# cases

def icosphere(level, radius=1.0):
    """An icosphere with outward faces, built here: vertices [Nv,3] float32 on the sphere, faces [F,3] int32 (20 x 4^level)"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (radius * np.array(v)).astype(np.float32), np.array(f, np.int32)


def cube(half=4.0):
    """the cube [-half, half]^3 in 12 outward triangles"""
    s = half
    v = np.array([(x, y, z) for x in (-s, s) for y in (-s, s) for z in (-s, s)], np.float32)
    f = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], np.int32)
    return v, f


def batch_of(vertices, B, seed, jitter=0.01):
    """[B,Nv,3] float32: the vertices with a per-image jitter (relative to their extent)"""
    rng = np.random.default_rng(seed)
    return (vertices[None] + jitter * np.abs(vertices).max() * rng.uniform(-1, 1, (B,) + vertices.shape)).astype(np.float32)


def shell_points(seed, N, radius=1.0, B=None, gap=0.15):
    """[B,N,3] float32 ([N,3] with B None): random directions at radii in [0.2, 1 - gap] and [1 + gap, 2] x radius in turn --
    off a sphere-like surface of that radius by at least gap x radius"""
    rng = np.random.default_rng(seed)
    shape = (N,) if B is None else (B, N)
    d = rng.normal(size=shape + (3,))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    inner = rng.uniform(0.2, 1.0 - gap, shape)
    outer = rng.uniform(1.0 + gap, 2.0, shape)
    r = np.where(np.arange(N) % 2 == 0, inner, outer)
    return (radius * r[..., None] * d).astype(np.float32)
