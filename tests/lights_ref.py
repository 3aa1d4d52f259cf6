"""Test-side restatement of learnable lights (include/nr_hip.h: nr_light_colors_forward / _backward) in NumPy, written from
the header's formulas; it does not import the package.

  light(...)     the light colours [B,F,3] (flat) / [B,F,3,3] (smooth) in the given dtype, in the kernels' operation order
                 (normal sums in ascending (face, corner) order), and their sums of |terms|
  adjoint(...)   the adjoint at g: the gradient of the vertices and of the six parameters (each in its parameter's layout), and
                 for every entry the sum of |terms| M -- absolute values propagated through every sum and difference, so that a
                 float32 evaluation of the same chain stays within a small multiple of u M
  the meshes, parameter layouts and upstream weights that tests/test_lights.py and tests/test_lights_gpu.py share
"""
import numpy as np

import vertex_ref

NORM_EPS = 1e-5
NAMES = ('intensity_ambient', 'intensity_directional', 'color_ambient', 'color_directional', 'direction', 'sh')
SHAPES = {'intensity_ambient': (), 'intensity_directional': (), 'color_ambient': (3,), 'color_directional': (3,),
          'direction': (3,), 'sh': (9, 3)}
C0, C1, C2, C3, C4 = (np.float32(x) for x in (0.282095, 0.488603, 1.092548, 0.315392, 0.546274))  # float32 literals
U = 2.0 ** -24


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return vertex_ref._cross(a, b)


def _abs_cross(a, b):
    return vertex_ref._abs_cross(a, b)


def basis(u, dt):
    """Y_0 .. Y_8 [...,9] at u [...,3], and their magnitudes (the sums of |terms| of Y6 and Y8)."""
    c0, c1, c2, c3, c4 = (dt(c) for c in (C0, C1, C2, C3, C4))
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    Y = np.stack((np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (dt(3) * z * z - dt(1)),
                  c2 * x * z, c4 * (x * x - y * y)), axis=-1)
    mag = np.abs(Y)
    mag[..., 6] = c3 * (dt(3) * z * z + dt(1))
    mag[..., 8] = c4 * (x * x + y * y)
    return Y.astype(dt), mag


def per_image(P, B, dt):
    """The six parameters broadcast to one per image (sh may be None), as dt."""
    out = []
    for name in NAMES:
        p = P[name]
        if p is None:
            out.append(None)
            continue
        p = np.asarray(p, dt)
        if p.shape == SHAPES[name] or (SHAPES[name] == () and p.shape == (1,)):
            p = np.broadcast_to(p.reshape(SHAPES[name]), (B,) + SHAPES[name])
        assert p.shape == (B,) + SHAPES[name], (name, p.shape)
        out.append(p)
    return out


def _idx(faces, B):
    return vertex_ref._idx(faces, B)


def _normals(v, ix, smooth, dt):
    """(N [items,3] the normals the light is evaluated at, the faces' v10, v12)."""
    w = v[ix]
    v10, v12 = w[:, 0] - w[:, 1], w[:, 2] - w[:, 1]
    n = _cross(v10, v12)
    if not smooth:
        return n, v10, v12
    m = np.zeros((v.shape[0], 3), dt)
    np.add.at(m, ix.reshape(-1), np.repeat(n, 3, axis=0))  # unbuffered, element by element: ascending (face, corner), as the kernels
    return m, v10, v12


def _unit(N, d, dt):
    r = np.sqrt(_dot(N, N))
    nh = N / (r + dt(NORM_EPS))[..., None]
    return r, nh, _dot(nh, d), np.abs(nh) @ np.abs(d)


def _seen(u, cosv, cos_mag, ia, idir, ca, cd, sh, dt):
    """L(u) [N,3] and its sum of |terms|."""
    amb = ia * ca
    light = amb + idir * (cd * cosv[:, None])
    mag = np.abs(amb) + np.abs(idir) * (np.abs(cd) * cos_mag[:, None])
    if sh is not None:
        Y, Ym = basis(u, dt)
        for k in range(9):
            light = light + sh[k] * Y[:, k, None]
            mag = mag + np.abs(sh[k]) * Ym[:, k, None]
    return light.astype(dt), mag


def light(vertices, faces, P, fill_back, smooth, dt=np.float64):
    """-> (light, M) with the layout of nr_light_colors_forward's light_out."""
    v = np.asarray(vertices, dt)
    B = v.shape[0]
    idx = _idx(faces, B)
    Nf = idx.shape[1]
    ia, idir, ca, cd, d, sh = per_image(P, B, dt)
    F = 2 * Nf if fill_back else Nf
    out = np.zeros((B, F, 3, 3) if smooth else (B, F, 3), dt)
    mag = np.zeros(out.shape)
    with np.errstate(all='ignore'):
        for b in range(B):
            ix = idx[b]
            N, _, _ = _normals(v[b], ix, smooth, dt)
            _, nh, dot, absdot = _unit(N, d[b], dt)
            s = None if sh is None else sh[b]
            zero = dt(0)
            lf, mf = _seen(nh, np.fmax(dot, zero), np.where(dot > 0, absdot, 0), ia[b], idir[b], ca[b], cd[b], s, dt)
            lb, mb = _seen(-nh, np.fmax(-dot, zero), np.where(-dot > 0, absdot, 0), ia[b], idir[b], ca[b], cd[b], s, dt)
            if smooth:
                out[b, :Nf], mag[b, :Nf] = lf[ix], mf[ix]
                if fill_back:
                    out[b, Nf:], mag[b, Nf:] = lb[ix][:, ::-1], mb[ix][:, ::-1]
            else:
                out[b, :Nf], mag[b, :Nf] = lf, mf
                if fill_back:
                    out[b, Nf:], mag[b, Nf:] = lb, mb
    return out, mag


def normal_dots(vertices, faces, P, smooth):
    """n . d of every normal that is not exactly zero, in float64 (the tests assert |.| >= 1e-4 on their inputs)."""
    v = np.asarray(vertices, np.float64)
    B = v.shape[0]
    idx = _idx(faces, B)
    d = per_image(P, B, np.float64)[4]
    out = []
    for b in range(B):
        N, _, _ = _normals(v[b], idx[b], smooth, np.float64)
        r, _, dot, _ = _unit(N, d[b], np.float64)
        out.append(dot[r > 0])
    return np.concatenate(out)


def _sh_bwd(u, G, Gm, sh, dt):
    """d (sum_c G_c sum_k sh[k,c] Y_k(u)) / du [N,3] and its sum of |terms|."""
    c1, c2, c3, c4 = (dt(c) for c in (C1, C2, C3, C4))
    A, Am = G @ sh.T, Gm @ np.abs(sh).T  # [N,9]
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    two, six = dt(2), dt(6)
    g = np.stack((((c1 * A[:, 3] + (c2 * y) * A[:, 4]) + (c2 * z) * A[:, 7]) + ((two * c4) * x) * A[:, 8],
                  ((c1 * A[:, 1] + (c2 * x) * A[:, 4]) + (c2 * z) * A[:, 5]) - ((two * c4) * y) * A[:, 8],
                  ((c1 * A[:, 2] + (c2 * y) * A[:, 5]) + ((six * c3) * z) * A[:, 6]) + (c2 * x) * A[:, 7]), axis=-1)
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    m = np.stack((c1 * Am[:, 3] + c2 * ay * Am[:, 4] + c2 * az * Am[:, 7] + two * c4 * ax * Am[:, 8],
                  c1 * Am[:, 1] + c2 * ax * Am[:, 4] + c2 * az * Am[:, 5] + two * c4 * ay * Am[:, 8],
                  c1 * Am[:, 2] + c2 * ay * Am[:, 5] + six * c3 * az * Am[:, 6] + c2 * ax * Am[:, 7]), axis=-1)
    return g, m


def adjoint(vertices, faces, P, fill_back, smooth, g, dt=np.float64):
    """-> {'vertices': (grad [B,Nv,3], M), name: (grad, M) for the six parameters in their own layouts (sh None: absent)}."""
    v = np.asarray(vertices, dt)
    g = np.asarray(g, dt)
    B, Nv = v.shape[:2]
    idx = _idx(faces, B)
    Nf = idx.shape[1]
    ia, idir, ca, cd, d, sh = per_image(P, B, dt)
    gv, gvm = np.zeros((B, Nv, 3), dt), np.zeros((B, Nv, 3))
    grads = {n: (np.zeros((B,) + SHAPES[n], dt), np.zeros((B,) + SHAPES[n])) for n in NAMES if P[n] is not None}
    with np.errstate(all='ignore'):
        for b in range(B):
            ix = idx[b]
            N, v10, v12 = _normals(v[b], ix, smooth, dt)
            n_items = N.shape[0]
            Gf, Gb = np.zeros((n_items, 3), dt), np.zeros((n_items, 3), dt)
            Gfm, Gbm = np.zeros((n_items, 3)), np.zeros((n_items, 3))
            if smooth:
                for k in range(3):
                    np.add.at(Gf, ix[:, k], g[b, :Nf, k])
                    np.add.at(Gfm, ix[:, k], np.abs(g[b, :Nf, k]))
                    if fill_back:
                        np.add.at(Gb, ix[:, k], g[b, Nf:, 2 - k])
                        np.add.at(Gbm, ix[:, k], np.abs(g[b, Nf:, 2 - k]))
            else:
                Gf, Gfm = g[b, :Nf], np.abs(g[b, :Nf])
                if fill_back:
                    Gb, Gbm = g[b, Nf:], np.abs(g[b, Nf:])
            r, nh, dot, absdot = _unit(N, d[b], dt)
            gnh, gnhm = np.zeros((n_items, 3), dt), np.zeros((n_items, 3))
            S1, S1m, Sc, Scm = (np.zeros(3) for _ in range(4))
            SY, SYm, T, Tm = np.zeros((9, 3)), np.zeros((9, 3)), np.zeros(3), np.zeros(3)
            for sign, G, Gm in ((1, Gf, Gfm), (-1, Gb, Gbm)):
                if sign < 0 and not fill_back:
                    continue
                u, dots = (nh, dot) if sign > 0 else (-nh, -dot)
                active = dots > 0
                cosv, cosm = np.fmax(dots, dt(0)), np.where(active, absdot, 0)
                S1, S1m = S1 + G.sum(0), S1m + Gm.sum(0)
                Sc, Scm = Sc + (cosv[:, None] * G).sum(0), Scm + (cosm[:, None] * Gm).sum(0)
                gcd, gcdm = G @ cd[b], Gm @ np.abs(cd[b])
                T = T + (np.where(active, gcd, 0)[:, None] * u).sum(0)
                Tm = Tm + (np.where(active, gcdm, 0)[:, None] * np.abs(u)).sum(0)
                gu = np.where(active, idir[b] * gcd, 0)[:, None] * d[b]
                gum = np.where(active, np.abs(idir[b]) * gcdm, 0)[:, None] * np.abs(d[b])
                if sh is not None:
                    Y, Ym = basis(u, dt)
                    SY, SYm = SY + Y.T @ G, SYm + Ym.T @ Gm
                    a, am = _sh_bwd(u, G, Gm, sh[b], dt)
                    gu, gum = gu + a, gum + am
                gnh, gnhm = gnh + sign * gu, gnhm + gum
            # normalisation: g_N = g / (r + eps) - N (g . N) / ((r + eps)^2 r); nothing at N = 0
            s = r + dt(NORM_EPS)
            ok = r > 0
            k = np.where(ok, _dot(gnh, N) / (s * s * r), 0)
            km = np.where(ok, (gnhm * np.abs(N)).sum(-1) / (s * s * r), 0)
            gN = np.where(ok[:, None], gnh / s[:, None] - N * k[:, None], 0)
            gNm = np.where(ok[:, None], gnhm / s[:, None] + np.abs(N) * km[:, None], 0)
            if smooth:
                gN, gNm = (gN[ix[:, 0]] + gN[ix[:, 1]]) + gN[ix[:, 2]], gNm[ix].sum(1)
            ga, gb = _cross(v12, gN), _cross(gN, v10)
            gam, gbm = _abs_cross(v12, gNm), _abs_cross(gNm, v10)
            for kk, (t, tm) in enumerate(((ga, gam), (-(ga + gb), gam + gbm), (gb, gbm))):
                np.add.at(gv[b], ix[:, kk], t)
                np.add.at(gvm[b], ix[:, kk], tm)
            # the parameters, from the 36 sums
            per = {'intensity_ambient': (S1 @ ca[b], S1m @ np.abs(ca[b])), 'color_ambient': (ia[b] * S1, np.abs(ia[b]) * S1m),
                   'intensity_directional': (Sc @ cd[b], Scm @ np.abs(cd[b])),
                   'color_directional': (idir[b] * Sc, np.abs(idir[b]) * Scm),
                   'direction': (idir[b] * T, np.abs(idir[b]) * Tm), 'sh': (SY, SYm)}
            for n in grads:
                grads[n][0][b], grads[n][1][b] = per[n]
    out = {'vertices': (gv, gvm)}
    for n, (gr, m) in grads.items():
        shape = np.asarray(P[n]).shape
        if shape == SHAPES[n] or (SHAPES[n] == () and shape == (1,)):  # shared: the images added up
            gr, m = gr.sum(0).reshape(shape), m.sum(0).reshape(shape)
        out[n] = (gr.astype(dt), m)
    return out


def worst_ratio(got, ref, mag):
    """max |got - ref| / (u M); entries with M = 0 must be equal (inf otherwise)."""
    got, ref, mag = (np.asarray(x, np.float64) for x in (got, ref, mag))
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return np.inf
    with np.errstate(all='ignore'):
        ratio = np.where(mag > 0, err / (U * mag), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the cases

B = 3
MESHES = ('tetra', 'ico1', 'ico3', 'odd')
LAYOUTS = ('shared', 'per_image', 'mixed')


def mesh(name, seed=0):
    """(vertices [B,Nv,3] float32 with float noise, faces [Nf,3] int32).  'odd': icosphere(1) plus an isolated vertex, a face
    with a repeated index and a zero-area face -- two of its corners are distinct vertices at one and the same position, so
    its normal is exactly zero in every precision."""
    rng = np.random.RandomState(1000 + seed)
    if name == 'tetra':
        v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * 0.6
        f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    else:
        v, f = vertex_ref.icosphere(3 if name == 'ico3' else 1)
    v = v[None] + rng.uniform(-0.03, 0.03, (B,) + v.shape) * (0.25 if name == 'ico3' else 1.0)
    # a tilt, so that no normal is perpendicular to a direction along an axis
    a, c = 0.37, 0.21
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    v = (v @ (Rz @ Rx).T).astype(np.float32)
    if name == 'odd':
        Nv = v.shape[1]
        extra = np.stack((np.full((B, 3), 0.25, np.float32), v[:, 5]), axis=1)  # Nv: isolated; Nv + 1: a copy of vertex 5
        v = np.concatenate((v, extra), axis=1)
        f = np.concatenate((f, np.array([[0, 3, 3], [5, Nv + 1, 7]], np.int32)), axis=0)
    return v, f


def faces_per_image(f):
    """[B,Nf,3]: image 1 has every face rotated by one corner, image 2 the faces in reverse order (other tables)."""
    return np.stack((f, np.roll(f, 1, axis=1), f[::-1])).astype(np.int32)


def params(layout, with_sh, seed=0):
    """The six parameters as float32 arrays; `layout`: all shared, all one per image, or mixed."""
    rng = np.random.RandomState(2000 + seed)
    per = {'shared': (), 'per_image': NAMES, 'mixed': ('intensity_directional', 'color_ambient', 'sh')}[layout]
    base = {'intensity_ambient': 0.45, 'intensity_directional': 0.6, 'color_ambient': (0.9, 0.8, 1.0),
            'color_directional': (1.0, 0.7, 0.85), 'direction': (0.3, 0.8, -0.45), 'sh': None}
    P = {}
    for n in NAMES:
        if n == 'sh':
            if not with_sh:
                P[n] = None
                continue
            val = rng.uniform(-0.3, 0.3, ((B,) if n in per else ()) + (9, 3))
        else:
            val = np.asarray(base[n], np.float64)
            if n in per:
                val = val * rng.uniform(0.8, 1.2, (B,) + val.shape)
        P[n] = val.astype(np.float32)
    return P


def upstream(shape, seed=0):
    """Upstream weights that differ per image."""
    rng = np.random.RandomState(3000 + seed)
    w = rng.uniform(-1, 1, shape).astype(np.float32)
    return w * (1.0 + 0.5 * np.arange(shape[0], dtype=np.float32)).reshape((-1,) + (1,) * (len(shape) - 1))


def all_cases():
    """(mesh, faces per image?, layout, sh?, fill_back, smooth): every mesh over every variant -- the cases over which the
    constants are measured and the kernels run."""
    for name in MESHES:
        for smooth in (False, True):
            for fill_back in (True, False):
                for per_batch in (False, True):
                    for layout in LAYOUTS:
                        for with_sh in (True, False):
                            yield name, per_batch, layout, with_sh, fill_back, smooth


# The noise seed of every mesh.  icosphere(3) has 1 280 faces and 642 vertices in three images under up to three directions:
# with most seeds one of those ~10^4 normals comes within 1e-4 of perpendicular to its direction (seed 0: 7.7e-5), which the
# tests' inputs must not (test_inputs_keep_away_from_the_relu_kink); seed 10 keeps all of them beyond 3.2e-4.
MESH_SEED = {'tetra': 0, 'ico1': 0, 'ico3': 10, 'odd': 0}


def case_inputs(name, per_batch, layout, with_sh, fill_back, smooth):
    v, f = mesh(name, MESH_SEED[name])
    faces = faces_per_image(f) if per_batch else f
    P = params(layout, with_sh)
    Nf = f.shape[0]
    F = 2 * Nf if fill_back else Nf
    g = upstream((B, F, 3, 3) if smooth else (B, F, 3))
    return v, faces, P, g
