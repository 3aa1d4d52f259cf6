"""Test-side restatement of the fused geometry + lighting front-end (include/nr_hip.h: "Fused geometry + lighting front-end",
"Projection camera"; nr_frontend_forward / _backward, their _light and _projection variants) in NumPy, written from the
header's contract; it does not import the package.

  forward(...)   faces_out [B,F,3,3] and the lit textures [B,F,ts,ts,ts,3] or the light colours [B,F,3], in the given dtype
                 and in the header's operation order, each with its sums of |terms|
  adjoint(...)   the adjoint at the cotangents (any of them None = zeros): the gradients of vertices, textures, eye or K, R, t,
                 each in its parameter's layout, with every entry's sum of |terms| M and the number n of addends that reach it
                 (face corners per vertex, images per shared camera parameter, 1 for what is stored)
  the meshes, cameras, lights and cotangents that tests/test_frontend_ref.py and tests/test_frontend_entrywise_gpu.py share

The magnitudes are carried by the arithmetic itself, as a running error analysis (Higham, Accuracy and Stability of Numerical
Algorithms, 3.3): a V holds a value in the working dtype and, in float64, the magnitude m of its first-order rounding error
in units of u, |fl(x) - x| <= u m, which every operation propagates without cancellation and to which it adds its own
rounding, the size of its result --
  a +- b -> m_a + m_b + |a +- b|;   a b -> m_a |b| + |a| m_b + |a b|;   a / b -> m_a / |b| + |a| m_b / b^2 + |a / b|;
  sqrt(q) -> m_q / (2 sqrt(q)) + sqrt(q);   where(c, a, 0) -> m_a or 0;   a sum -> the sum of the m and of the |terms|.
An input is exact, m = 0: the vertices, textures, camera and light parameters and the cotangents are float32 numbers, so
the difference of two of them carries one rounding, not the size of its operands.  An entry that no term reaches has
m = 0, and so has a copy of an input.  For a scattered entry the sum of |terms| is part of m, so the same M serves the
second term of the bound, Higham's gamma(n - 1) M for n float addends in any order.  A float32 evaluation of the same
chain in another order of its sums differs from the float64 one by a small multiple of u m, entry by entry; the multiple
is measured in tests/test_frontend_ref.py.
"""
import math

import numpy as np

import helpers
import lights_ref
import projection_ref

NORM_EPS = 1e-5
U = 2.0 ** -24
UP = (0.0, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# values with magnitudes

class V(object):
    __array_ufunc__ = None  # ndarray (op) V defers to V

    def __init__(self, v, m=None):
        self.v = np.asarray(v)
        self.m = np.zeros(self.v.shape) if m is None else np.asarray(m, np.float64)

    def _lift(self, o):
        if isinstance(o, V):
            return o
        v = np.asarray(o, self.v.dtype)  # a constant: exact when float32 holds it, else rounded once
        return V(v, np.where(np.asarray(o, np.float32).astype(np.float64) == np.asarray(o, np.float64), 0.0, np.abs(v)))

    def _a(self):
        return np.abs(self.v).astype(np.float64)

    def __add__(self, o):
        o = self._lift(o)
        r = self.v + o.v
        return V(r, self.m + o.m + np.abs(r))

    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        r = self.v - o.v
        return V(r, self.m + o.m + np.abs(r))

    def __rsub__(self, o):
        o = self._lift(o)
        r = o.v - self.v
        return V(r, self.m + o.m + np.abs(r))

    def __neg__(self):
        return V(-self.v, self.m)

    def __mul__(self, o):
        o = self._lift(o)
        r = self.v * o.v
        return V(r, self.m * o._a() + self._a() * o.m + np.abs(r))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        r = self.v / o.v
        return V(r, self.m / o._a() + self._a() * o.m / np.square(o._a()) + np.abs(r))

    def __getitem__(self, k):
        return V(self.v[k], self.m[k])

    def sum(self, axis):
        return V(self.v.sum(axis), self.m.sum(axis) + np.abs(self.v).astype(np.float64).sum(axis))

    def transpose(self, *axes):
        return V(self.v.transpose(*axes), self.m.transpose(*axes))

    def reshape(self, *shape):
        return V(self.v.reshape(*shape), self.m.reshape(*shape))


def stack(items, axis=-1):
    return V(np.stack([x.v for x in items], axis=axis), np.stack([x.m for x in items], axis=axis))


def where(cond, a):
    """a where cond, else an exact 0."""
    return V(np.where(cond, a.v, np.zeros((), a.v.dtype)), np.where(cond, a.m, 0.0))


def broadcast(a, shape):
    return V(np.broadcast_to(a.v, shape), np.broadcast_to(a.m, shape))


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                  a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]))


def norm3(x):
    q = dot3(x, x)
    r = np.sqrt(q.v)
    rd = r.astype(np.float64)
    return V(r, np.where(rd > 0, q.m / (2.0 * rd) + rd, np.sqrt(q.m)))  # (at 0 the square root is Hoelder, not Lipschitz)


def normalize(x):
    """chainer's normalize: x / (|x| + 1e-5)."""
    s = norm3(x) + NORM_EPS
    return x / s[..., None]


def normalize_bwd(x, g):
    """g_x = g / (r + eps) - x (g . x) / ((r + eps)^2 r); the second term is absent at r = 0."""
    r = norm3(x)
    s = r + NORM_EPS
    k = where(r.v > 0, dot3(g, x) / ((s * s) * r))
    return g / s[..., None] - x * k[..., None]


# ---------------------------------------------------------------------------------------------------------------------
# the pieces of the front-end

def _idx(faces, B):
    idx = np.asarray(faces, np.int64)
    if idx.ndim == 2:
        idx = idx[None]
    return np.broadcast_to(idx, (B,) + idx.shape[1:])


def _per_image(p, B, shape, dt):
    """(p as [B] + shape in dt, shared?)"""
    p = np.asarray(p, dt)
    if p.shape == shape:
        return np.broadcast_to(p, (B,) + shape), True
    assert p.shape == (B,) + shape, (p.shape, shape)
    return p, False


def tan_width(angle):
    """tan(viewing_angle / 180 * 3.1416) as the host computes it, in float32 (nr_camera.width)."""
    return np.tan(np.float32(angle) / np.float32(180.) * np.float32(3.1416), dtype=np.float32)


def _basis(cam, B, dt):
    """look_at / look: (eye V [B,3], shared?, d, cx, cy the vectors before their normalisation, r V [B,3,3] rows x, y, z)."""
    e, shared = _per_image(cam['eye'], B, (3,), dt)
    eye = V(e)
    up = V(np.broadcast_to(np.asarray(UP, dt), (B, 3)))
    if cam['mode'] == 'look_at':
        d = np.zeros(3, dt) - eye  # `at` is the origin
    else:
        d = V(np.broadcast_to(np.asarray(cam['direction'], np.float32).astype(dt), (B, 3)))
    z = normalize(d)
    cx = cross(up, z)
    x = normalize(cx)
    cy = cross(z, x)
    y = normalize(cy)
    return eye, shared, up, d, cx, cy, stack((x, y, z), axis=1)


def _rotate(r, t):
    """[B,3,3] applied to [B,Nf,3,3(xyz)] points: ((t0 r_i0 + t1 r_i1) + t2 r_i2)."""
    return stack([(t[..., 0] * r[:, i, 0][:, None, None] + t[..., 1] * r[:, i, 1][:, None, None])
                  + t[..., 2] * r[:, i, 2][:, None, None] for i in range(3)])


def _look(cam, W, dt):
    """The look_at / look camera on the gathered corners W [B,Nf,3,3]: (out, what the backward needs)."""
    B = W.v.shape[0]
    eye, shared, up, d, cx, cy, r = _basis(cam, B, dt)
    t = W - eye[:, None, None, :]
    c = _rotate(r, t)
    if cam['perspective']:
        width = V(np.asarray(tan_width(cam['angle'])).astype(dt))
        out = stack((c[..., 0] / c[..., 2] / width, c[..., 1] / c[..., 2] / width, c[..., 2]))
    else:
        width = None
        out = c
    return out, dict(eye=eye, shared=shared, up=up, d=d, cx=cx, cy=cy, r=r, t=t, c=c, width=width)


def _look_bwd(cam, S, g):
    """g [B,Nf,3,3] the cotangent of `out` -> (g_w [B,Nf,3,3], g_eye V [B,3])."""
    c, r, t = S['c'], S['r'], S['t']
    if cam['perspective']:
        zw = c[..., 2] * S['width']
        gc = stack((g[..., 0] / zw, g[..., 1] / zw,
                    g[..., 2] - (g[..., 0] * c[..., 0] + g[..., 1] * c[..., 1]) / (c[..., 2] * zw)))
    else:
        gc = g
    # c = R (w - eye): g_w = R^T g_c, g_eye -= g_w, g_R[i][j] = sum g_c[i] (w - eye)[j]
    gw = stack([(gc[..., 0] * r[:, 0, j][:, None, None] + gc[..., 1] * r[:, 1, j][:, None, None])
                + gc[..., 2] * r[:, 2, j][:, None, None] for j in range(3)])
    ge = -gw.sum((1, 2))
    if cam['mode'] == 'look_at':  # R depends on eye only here
        gR = stack([stack([(gc[..., i] * t[..., j]).sum((1, 2)) for j in range(3)]) for i in range(3)], axis=1)  # [B,3,3]
        gx, gy, gz = gR[:, 0], gR[:, 1], gR[:, 2]
        x, z = r[:, 0], r[:, 2]
        gcy = normalize_bwd(S['cy'], gy)          # y = N(cy), cy = z x x
        gz = gz + cross(x, gcy)
        gx = gx + cross(gcy, z)
        gcx = normalize_bwd(S['cx'], gx)          # x = N(cx), cx = up x z
        gz = gz + cross(gcx, S['up'])
        ge = ge - normalize_bwd(S['d'], gz)       # z = N(d), d = at - eye
    return gw, ge


def _projection_camera(cam, B, dt):
    K, Ks = _per_image(cam['K'], B, (3, 3), dt)
    R, Rs = _per_image(cam['R'], B, (3, 3), dt)
    t = np.asarray(cam['t'], dt)
    if t.ndim == 3:  # [B,1,3]
        t = t[:, 0]
    t, ts_ = _per_image(t, B, (3,), dt)
    d = None if cam.get('dist') is None else V(_per_image(cam['dist'], B, (5,), dt)[0])
    return V(K), Ks, V(R), Rs, V(t), ts_, d, V(np.asarray(np.float32(cam['orig_size'])).astype(dt))


def _project(cam, W, dt):
    """The projection camera of the header, line by line."""
    B = W.v.shape[0]
    K, Ks, R, Rs, t, ts_, d, S = _projection_camera(cam, B, dt)

    def per(a):  # a per-image scalar against [B,Nf,3]
        return a[:, None, None]
    c = stack([((R[:, i, 0][:, None, None] * W[..., 0] + R[:, i, 1][:, None, None] * W[..., 1])
                + R[:, i, 2][:, None, None] * W[..., 2]) + t[:, i][:, None, None] for i in range(3)])
    xp, yp = c[..., 0] / c[..., 2], c[..., 1] / c[..., 2]
    st = dict(K=K, Ks=Ks, R=R, Rs=Rs, ts=ts_, d=d, S=S, c=c, xp=xp, yp=yp)
    if d is not None:
        k1, k2, p1, p2, k3 = (per(d[:, i]) for i in range(5))
        x, y = xp, yp
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        rad = ((1.0 + k1 * r2) + k2 * r4) + k3 * r6
        xd = (x * rad + 2.0 * p1 * x * y) + p2 * (r2 + 2.0 * x * x)
        yd = (y * rad + p1 * (r2 + 2.0 * y * y)) + 2.0 * p2 * x * y
        st.update(r2=r2, rad=rad)
    else:
        xd, yd = xp, yp
    u = (per(K[:, 0, 0]) * xd + per(K[:, 0, 1]) * yd) + per(K[:, 0, 2])
    v = (per(K[:, 1, 0]) * xd + per(K[:, 1, 1]) * yd) + per(K[:, 1, 2])
    st.update(xd=xd, yd=yd)
    return stack(((2.0 * u - S) / S, (S - 2.0 * v) / S, c[..., 2])), st


def _project_bwd(st, W, g):
    """-> (g_w [B,Nf,3,3], g_K [B,3,3] (row 2 exactly 0), g_R [B,3,3], g_t [B,3]) per image."""
    K, R, d, S, c, xp, yp, xd, yd = (st[n] for n in ('K', 'R', 'd', 'S', 'c', 'xp', 'yp', 'xd', 'yd'))

    def per(a):
        return a[:, None, None]
    gu = 2.0 * g[..., 0] / S
    gv = -2.0 * g[..., 1] / S
    zero = V(np.zeros(gu.v.shape[0], gu.v.dtype))
    gK = stack([stack([(gu * xd).sum((1, 2)), (gu * yd).sum((1, 2)), gu.sum((1, 2))]),
                stack([(gv * xd).sum((1, 2)), (gv * yd).sum((1, 2)), gv.sum((1, 2))]),
                stack([zero, zero, zero])], axis=1)
    gxd = gu * per(K[:, 0, 0]) + gv * per(K[:, 1, 0])
    gyd = gu * per(K[:, 0, 1]) + gv * per(K[:, 1, 1])
    gxp, gyp = gxd, gyd
    if d is not None:  # the Jacobian of (x'', y'') by (x', y'); it is symmetric
        k1, k2, p1, p2, k3 = (per(d[:, i]) for i in range(5))
        x, y, r2, rad = xp, yp, st['r2'], st['rad']
        drad = (k1 + 2.0 * k2 * r2) + 3.0 * k3 * (r2 * r2)
        jxx = ((rad + 2.0 * x * x * drad) + 2.0 * p1 * y) + 6.0 * p2 * x
        jxy = ((2.0 * x * y * drad) + 2.0 * p1 * x) + 2.0 * p2 * y
        jyy = ((rad + 2.0 * y * y * drad) + 6.0 * p1 * y) + 2.0 * p2 * x
        gxp = gxd * jxx + gyd * jxy
        gyp = gxd * jxy + gyd * jyy
    gc = stack((gxp / c[..., 2], gyp / c[..., 2], g[..., 2] - (gxp * xp + gyp * yp) / c[..., 2]))
    gw = stack([(gc[..., 0] * R[:, 0, j][:, None, None] + gc[..., 1] * R[:, 1, j][:, None, None])
                + gc[..., 2] * R[:, 2, j][:, None, None] for j in range(3)])
    gR = stack([stack([(gc[..., i] * W[..., j]).sum((1, 2)) for j in range(3)]) for i in range(3)], axis=1)
    gt = stack([gc[..., i].sum((1, 2)) for i in range(3)])
    return gw, gK, gR, gt


def _face_light(W, light, dt):
    """(colour of every face, of its reversed copy [B,Nf,3], the normal before normalisation, n_hat . d); the last two are
    None without a directional term."""
    f = lambda x: np.asarray(x, np.float32).astype(dt)
    ia, idir, ca, cd, d = (f(light[n]) for n in ('ia', 'id', 'ca', 'cd', 'dir'))
    shape = W.v.shape[:2] + (3,)
    amb = V(ia) * V(ca) if ia != 0 else V(np.zeros(3, dt))
    if idir == 0:
        amb = broadcast(amb, shape)
        return amb, amb, None, None
    v10, v12 = W[:, :, 0] - W[:, :, 1], W[:, :, 2] - W[:, :, 1]
    n = cross(v10, v12)
    dot = dot3(normalize(n), V(d))
    cos_f, cos_b = where(dot.v > 0, dot), where(-dot.v > 0, -dot)
    lf = amb + V(idir) * (V(cd) * cos_f[..., None])
    lb = amb + V(idir) * (V(cd) * cos_b[..., None])
    return lf, lb, n, dot


def _gather(v, idx):
    return v[np.arange(v.shape[0])[:, None, None], idx]


def _flip(a):
    """The reversed copy of faces [B,Nf,3,3]: corners in reverse order."""
    return V(a.v[:, :, ::-1], a.m[:, :, ::-1])


def _cat(a, b):
    return np.concatenate((a.v, b.v), axis=1), np.concatenate((a.m, b.m), axis=1)


def forward(vertices, faces, textures, cam, light, fill_back, colors=False, dt=np.float64):
    """-> {'faces': (faces_out, M), 'textures': (textures_out, M) | 'light': (light_out, M)}; the second entry is absent
    without textures and colours."""
    v = np.asarray(vertices, dt)
    idx = _idx(faces, v.shape[0])
    W = V(_gather(v, idx))
    with np.errstate(all='ignore'):
        out = (_project(cam, W, dt) if cam['mode'] == 'projection' else _look(cam, W, dt))[0]
        res = {'faces': _cat(out, _flip(out)) if fill_back else (out.v, out.m)}
        if textures is not None or colors:
            lf, lb, _, _ = _face_light(W, light, dt)
            if colors:
                res['light'] = _cat(lf, lb) if fill_back else (lf.v, lf.m)
            else:
                tex = V(np.asarray(textures, dt))
                of = tex * lf[:, :, None, None, None, :]
                res['textures'] = _cat(of, tex.transpose(0, 1, 4, 3, 2, 5) * lb[:, :, None, None, None, :]) if fill_back \
                    else (of.v, of.m)
    return res


def adjoint(vertices, faces, textures, cam, light, fill_back, g_faces=None, g_textures_out=None, g_light=None,
            dt=np.float64):
    """-> {name: (gradient, M, n)} for 'vertices', 'textures' (with textures and g_textures_out) and 'eye' or 'K', 'R', 't';
    n is an array like the gradient, or 1."""
    v = np.asarray(vertices, dt)
    B, Nv = v.shape[:2]
    idx = _idx(faces, B)
    Nf = idx.shape[1]
    W = V(_gather(v, idx))
    F = 2 * Nf if fill_back else Nf
    cot = lambda g, shape: V(np.zeros(shape, dt) if g is None else np.asarray(g, dt).reshape(shape))
    gf = cot(g_faces, (B, F, 3, 3))
    res = {}
    with np.errstate(all='ignore'):
        gw = V(np.zeros((B, Nf, 3, 3), dt))
        # ---- textures / lighting ----
        glf = glb = None
        if textures is not None and g_textures_out is not None:
            tex = V(np.asarray(textures, dt))
            gt = cot(g_textures_out, (B, F) + tex.v.shape[2:])
            lf, lb, n, dot = _face_light(W, light, dt)
            a = gt[:, :Nf]
            res['textures'] = a * lf[:, :, None, None, None, :]
            glf = (a * tex).sum((2, 3, 4))
            if fill_back:
                bb = gt[:, Nf:].transpose(0, 1, 4, 3, 2, 5)
                res['textures'] = res['textures'] + bb * lb[:, :, None, None, None, :]
                glb = (bb * tex).sum((2, 3, 4))
        elif g_light is not None:
            gl = cot(g_light, (B, F, 3))
            lf, lb, n, dot = _face_light(W, light, dt)
            glf = gl[:, :Nf]
            if fill_back:
                glb = gl[:, Nf:]
        if glf is not None and n is not None:
            f32 = lambda x: np.asarray(x, np.float32).astype(dt)
            idir, cd, d = V(f32(light['id'])), V(f32(light['cd'])), V(f32(light['dir']))
            gdot = where(dot.v > 0, idir * dot3(cd, glf))  # light = amb + id (cd cos): d loss / d cos, through the relu
            if glb is not None:
                gdot = gdot - where(-dot.v > 0, idir * dot3(cd, glb))
            gn = normalize_bwd(n, gdot[..., None] * d)
            v10, v12 = W[:, :, 0] - W[:, :, 1], W[:, :, 2] - W[:, :, 1]
            ga, gb = cross(v12, gn), cross(gn, v10)  # n = v10 x v12
            gw = stack((ga, -(ga + gb), gb), axis=2)
        # ---- geometry ----
        g = gf[:, :Nf] + _flip(gf[:, Nf:]) if fill_back else gf
        if cam['mode'] == 'projection':
            out, st = _project(cam, W, dt)
            gwk, gK, gR, gt_ = _project_bwd(st, W, g)
            for name, gr, shared in (('K', gK, st['Ks']), ('R', gR, st['Rs']), ('t', gt_, st['ts'])):
                res[name] = gr.sum(0) if shared else gr
            counts = {'K': st['Ks'], 'R': st['Rs'], 't': st['ts']}
        else:
            out, st = _look(cam, W, dt)
            gwk, ge = _look_bwd(cam, st, g)
            res['eye'] = ge.sum(0) if st['shared'] else ge
            counts = {'eye': st['shared']}
        gw = gw + gwk
        gv, gvm = np.zeros((B, Nv, 3), dt), np.zeros((B, Nv, 3))
        where_ = (np.arange(B)[:, None, None], idx)
        np.add.at(gv, where_, gw.v)
        np.add.at(gvm, where_, gw.m + np.abs(gw.v))
        valence = np.zeros((B, Nv), np.int64)
        np.add.at(valence, where_, 1)
    out = {'vertices': (gv, gvm, np.broadcast_to(valence[:, :, None], gv.shape))}
    for name, gr in res.items():
        shape = np.shape(cam['t']) if name == 't' else gr.v.shape  # (t may be [B,1,3])
        out[name] = (gr.v.astype(dt).reshape(shape), gr.m.reshape(shape), B if counts.get(name, False) else 1)
    return out


def bound(M, n, C):
    """C u M + gamma(n - 1) M: C from the restatement's own float32 error, the second term Higham's bound for n addends in
    any order (float atomics)."""
    return C * U * M + helpers.gamma(np.maximum(np.asarray(n, np.float64) - 1.0, 0.0)) * M


def worst_ratio(got, ref, M, n=1, C=1.0):
    """max |got - ref| / bound(M, n, C); an entry with M = 0 must be equal (inf otherwise).  With C = 1 and n = 1 this is
    |got - ref| / (u M)."""
    got, ref, M = (np.asarray(x, np.float64) for x in (got, ref, M))
    assert got.shape == ref.shape == M.shape, (got.shape, ref.shape, M.shape)
    if not np.isfinite(got).all() or not np.isfinite(M).all():
        return np.inf
    err = np.abs(got - ref)
    b = np.broadcast_to(bound(M, n, C), M.shape)
    with np.errstate(all='ignore'):
        ratio = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the cases

B = 3
MESHES = ('one', 'fan', 'odd', 'ico3')
TS = {'one': (1, 2, 3, 5), 'fan': (1, 2, 3, 5), 'odd': (1, 2, 3, 5), 'ico3': (2,)}
LIGHTS = {'host': dict(ia=0.4, id=0.6, ca=(1.0, 0.9, 0.8), cd=(0.7, 1.0, 0.6), dir=(0.3, 0.8, -0.5))}  # test_frontend_gpu._renderer
LIGHTS['no_ambient'] = dict(LIGHTS['host'], ia=0.0)
LIGHTS['no_directional'] = dict(LIGHTS['host'], id=0.0)
LOOK_CAMERAS = ('look_at_10', 'look_at_30', 'look_at_45.5', 'look_at_30_shared', 'look_at_ortho', 'look_at_ortho_shared',
                'look_at_pole', 'look', 'look_shared')
PROJECTION_CAMERAS = tuple('projection_%s%s' % (layout, '_dist' if dist else '') for layout in ('shared', 'per_image', 'mixed')
                           for dist in (True, False)) + ('projection_t_b13_dist',)
CAMERAS = LOOK_CAMERAS + PROJECTION_CAMERAS
# The noise seed of every mesh (lights_ref.MESH_SEED explains the search): no normal within 1e-4 of perpendicular to the
# host light's direction.
MESH_SEED = {'one': 0, 'fan': 0, 'odd': 0, 'ico3': 0}
ORIG_SIZE = 256.0


def points_from_angles(distance, elevation, azimuth):
    e, a = math.radians(elevation), math.radians(azimuth)
    return (distance * math.cos(e) * math.sin(a), distance * math.sin(e), -distance * math.cos(e) * math.cos(a))


def _tilt(v):
    a, c = 0.37, 0.21
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return v @ (Rz @ Rx).T


def mesh(name, seed=None):
    """(vertices [B,Nv,3] float32 with noise per image, faces [Nf,3] int32).  'one': a single face; 'fan': 65 faces around
    vertex 0, a shallow cone -- one mesh over the 32 / 33 / 64 / 65 edges of the 32-face blocks, with a vertex of valence 65;
    'odd' and 'ico3': lights_ref.mesh (an isolated vertex, a repeated index and a zero-area face in 82 faces; 1 280 faces)."""
    seed = MESH_SEED[name] if seed is None else seed
    if name in ('odd', 'ico3'):
        return lights_ref.mesh(name, seed)
    rng = np.random.RandomState(4000 + seed)
    if name == 'one':
        v = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, -0.2], [0.1, 0.7, 0.15]])
        f = np.array([[0, 1, 2]], np.int32)
    else:
        ang = 2 * np.pi * np.arange(65) / 65
        rim = np.stack((0.8 * np.cos(ang), 0.8 * np.sin(ang), 0.1 * np.cos(3 * ang)), axis=1)
        v = np.concatenate((np.array([[0.0, 0.0, 0.35]]), rim), axis=0)
        f = np.stack((np.zeros(65, np.int32), 1 + np.arange(65), 1 + (np.arange(65) + 1) % 65), axis=1).astype(np.int32)
    v = v[None] + rng.uniform(-0.03, 0.03, (B,) + v.shape)
    return _tilt(v).astype(np.float32), f


def camera(name):
    """The camera of a case as a dict: mode, and eye / perspective / angle / direction, or K, R, t, dist, orig_size."""
    if name.startswith('projection'):
        layout = name.split('_')[1]
        dist = name.endswith('_dist')
        per = projection_ref.camera(B, seed=32, per_image=True, distortion=True, orig_size=ORIG_SIZE)
        one = projection_ref.camera(B, seed=33, per_image=False, distortion=True, orig_size=ORIG_SIZE)
        pick = {'shared': (one, one, one, one), 'per': (per, per, per, per), 'mixed': (one, per, per, one),
                't': (per, per, per, per)}[layout]
        K, R, t, d = (src[i] for i, src in enumerate(pick))
        if layout == 't':
            t = t[:, None, :]
        return dict(mode='projection', K=K, R=R, t=t, dist=d if dist else None, orig_size=ORIG_SIZE)
    shared = name.endswith('_shared')
    if name.startswith('look_at'):
        if name == 'look_at_pole':  # |up x z| = cos(elevation): 1.7e-3 at 89.9 degrees, where chainer's + 1e-5 shows
            eyes = [points_from_angles(2.732, e, a) for e, a in ((89.9, 30.0), (89.5, 160.0), (88.0, 290.0))]
        else:
            eyes = [points_from_angles(2.732, 20.0 + 5 * i, 70.0 * i) for i in range(B)]
        eyes = np.asarray(eyes, np.float32)
        ortho = 'ortho' in name
        angle = 30.0 if ortho or name == 'look_at_pole' else float(name.split('_')[2])
        return dict(mode='look_at', eye=eyes[1] if shared else eyes, perspective=not ortho, angle=angle)
    direction = 3.0 * np.array([0.2, -0.1, 1.0])  # not unit length
    unit = direction / np.linalg.norm(direction)
    eyes = np.asarray([-2.732 * unit + 0.1 * np.array([i - 1.0, 0.5 * i, -0.3 * i]) for i in range(B)], np.float32)
    return dict(mode='look', eye=eyes[1] if shared else eyes, perspective=True, angle=30.0,
                direction=direction.astype(np.float32))


def learnable(cam):
    """The names of the camera parameters that take a gradient."""
    return ('K', 'R', 't') if cam['mode'] == 'projection' else ('eye',)


def all_cases():
    """(mesh, camera, variant, ts, fill_back, faces per image?, light): every mesh under every camera with every variant --
    geometry only, light colours, lit textures at each texture size of the mesh.  fill_back and the topology's layout rotate
    with the camera and the variant, so that every mesh meets each of their four combinations with every variant and under
    every camera.  Then the two lights with one term switched off, once per mesh under one camera of each kind."""
    combos = ((True, False), (False, True), (True, True), (False, False))
    for name in MESHES:
        options = [('geometry', 0), ('colors', 0)] + [('textures', ts) for ts in TS[name]]
        for ci, cname in enumerate(CAMERAS):
            for oi, (variant, ts) in enumerate(options):
                fill_back, per_batch = combos[(ci + oi) % 4]
                yield name, cname, variant, ts, fill_back, per_batch, 'host'
        for lname in ('no_ambient', 'no_directional'):
            for cname in ('look_at_30', 'projection_mixed_dist'):
                yield name, cname, 'colors', 0, True, False, lname
                yield name, cname, 'textures', 2, True, True, lname


def case_inputs(case):
    """dict(vertices, faces, textures | None, cam, light | None, fill_back, colors, g_faces, g_textures_out | None,
    g_light | None) of a case; float32 arrays."""
    name, cname, variant, ts, fill_back, per_batch, lname = case
    v, f = mesh(name)
    Nf = f.shape[0]
    F = 2 * Nf if fill_back else Nf
    tex = None
    if variant == 'textures':
        tex = np.random.RandomState(5000 + ts).uniform(0, 1, (B, Nf, ts, ts, ts, 3)).astype(np.float32)
    return dict(vertices=v, faces=lights_ref.faces_per_image(f) if per_batch else f, textures=tex, cam=camera(cname),
                light=None if variant == 'geometry' else LIGHTS[lname], fill_back=fill_back, colors=variant == 'colors',
                g_faces=lights_ref.upstream((B, F, 3, 3), seed=1),
                g_textures_out=lights_ref.upstream((B, F, ts, ts, ts, 3), seed=2) if variant == 'textures' else None,
                g_light=lights_ref.upstream((B, F, 3), seed=3) if variant == 'colors' else None)


def evaluate(inp, dt=np.float64):
    """(forward(...), adjoint(...)) of case_inputs' dict."""
    fw = forward(inp['vertices'], inp['faces'], inp['textures'], inp['cam'], inp['light'], inp['fill_back'], inp['colors'], dt)
    ad = adjoint(inp['vertices'], inp['faces'], inp['textures'], inp['cam'], inp['light'], inp['fill_back'], inp['g_faces'],
                 inp['g_textures_out'], inp['g_light'], dt)
    return fw, ad


def conditions(inp):
    """(min |n_hat . d| over the normals that are not exactly zero (inf without one), min camera depth, min |up x z| (inf
    for the projection camera)) of a case's inputs, in float64."""
    v = np.asarray(inp['vertices'], np.float64)
    W = V(_gather(v, _idx(inp['faces'], v.shape[0])))
    dots = np.inf
    with np.errstate(all='ignore'):
        if inp['light'] is not None and inp['light']['id'] != 0:
            _, _, n, dot = _face_light(W, inp['light'], np.float64)
            live = norm3(n).v > 0
            dots = float(np.abs(dot.v[live]).min()) if live.any() else np.inf
        if inp['cam']['mode'] == 'projection':
            depth, pole = _project(inp['cam'], W, np.float64)[1]['c'].v[..., 2].min(), np.inf
        else:
            _, st = _look(inp['cam'], W, np.float64)
            depth, pole = st['c'].v[..., 2].min(), float(norm3(st['cx']).v.min())
    return dots, float(depth), pole
