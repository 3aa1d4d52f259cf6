"""Test-side restatement of the normal operators (include/nr_hip.h: nr_vertex_normals_*, nr_face_normals_*,
nr_corner_normals_*) in NumPy, written from the header's arithmetic:

  vertex_normals / face_normals / corner_normals (dt)   float32 in the kernels' operation order (normal sums in ascending
                                   (face, corner) order) or float64
  *_mag                            the magnitude every forward entry's rounding error is measured against
  adjoint64                        the adjoint in float64 with the magnitude of every entry of grad_vertices
  forward_k / backward_k           the number of roundings along the longest chain: the n of gamma_n in the bounds
  meshes()                         the small meshes the tests run on

The bounds.  |got - ref64| <= gamma_k * magnitude per entry, gamma_k = k u / (1 - k u), u = 2^-24; where the magnitude is 0
the entry must be equal (the inequality says so).  The vertices are float32 numbers, exact in float64, so an edge v0 - v1
carries one rounding relative to itself; from there on absolute values are propagated through every sum and difference:

  N_f, per component a1 b2 - a2 b1: 2 subtractions (the edges), 2 products and a subtraction, k = 5, against
      Nmag = |a1| |b2| + |a2| |b1|;
  m_v: that plus deg - 1 additions, against the sum of Nmag around the vertex;
  n = v / (sqrt(v . v) + eps): the dot product (3 products, 2 additions: 5 roundings, all terms positive), then the root,
      + eps and the division, which we count as the division's one and one more for root and eps together (the root halves
      the dot product's relative error): k = 6 relative to |n|; the error dv of v arrives through the Jacobian
      (1 / s) I - v v^T / (s^2 r), taken with absolute values:  nmag = vmag / s + |v| (|v| . vmag) / (s^2 r)  (>= |n|).
  forward_k: 5 + 6 for a face, 5 + (deg - 1) + 6 for a vertex of degree deg.

  Backward, the transposed chain.  Stage one: the corner difference front - back (1), the sum around the vertex (deg - 1) or
  over the corners (2), normalize's backward g / s - v k, k = (g . v) / (s^2 r): dot (5), s s r (2), division, product,
  g / s and the subtraction in parallel: 9 along the chain; v and r are recomputed in float32 and carry the forward's
  roundings (5 + deg - 1, and 4 for r).  Stage two: (g_m(v0) + g_m(v1)) + g_m(v2) (2), two cross products (2 each along a
  chain), -(ga + gb) (1), the sum around the vertex (deg - 1).  backward_k = 24 + 3 deg, deg the largest degree of the mesh.
  The magnitude takes normalize's backward with absolute values, with vmag in the place of |v| (v carries its own error) and
  the second term times kappa = (|v| . vmag) / r^2 >= 1, the condition of r: gmag / s + vmag (gmag . vmag) kappa / (s^2 r);
  the cross products with absolute values (vertex_ref._abs_cross) behind it.
"""
import numpy as np

import vertex_ref

f32 = np.float32
NORM_EPS = 1e-5
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


_idx = vertex_ref._idx
_cross = vertex_ref._cross
_abs_cross = vertex_ref._abs_cross
_dot = vertex_ref._dot


def _edges(v, ix):
    w = v[ix]  # [Nf,3,3]
    return w[:, 0] - w[:, 1], w[:, 2] - w[:, 1]


def _normalize(x, dt):
    s = np.sqrt(_dot(x, x)) + dt(NORM_EPS)
    return x / s[..., None]


def _normalize_mag(x, xmag):
    """nmag of the module docstring, float64."""
    r = np.sqrt((x * x).sum(-1))
    s = r + NORM_EPS
    with np.errstate(all='ignore'):
        second = np.where(r > 0, (np.abs(x) * xmag).sum(-1) / (s * s * r), 0.0)
    return xmag / s[..., None] + np.abs(x) * second[..., None]


def _sum_around(n, ix, Nv, dt):
    m = np.zeros((Nv, 3), dt)
    for e in range(3 * len(ix)):  # ascending (face, corner): the kernels' order
        m[ix[e // 3, e % 3]] += n[e // 3]
    return m


def degrees(faces_idx, Nv, B=1):
    """[B,Nv]: the number of (face, corner) pairs of every vertex."""
    idx = _idx(faces_idx, B)
    return np.stack([np.bincount(idx[b].reshape(-1), minlength=Nv) for b in range(B)])


def _forward(vertices, faces_idx, dt, what, smooth=False, fill_back=True):
    v = np.asarray(vertices, dt)
    B, Nv = v.shape[:2]
    idx = _idx(faces_idx, B)
    out = []
    with np.errstate(all='ignore'):
        for b in range(B):
            a, c = _edges(v[b], idx[b])
            N = _cross(a, c)
            nf = _normalize(N, dt)
            nv = _normalize(_sum_around(N, idx[b], Nv, dt), dt) if what == 'vertex' or (what == 'corner' and smooth) else None
            if what == 'face':
                out.append(nf)
            elif what == 'vertex':
                out.append(nv)
            else:
                front = nv[idx[b]] if smooth else np.repeat(nf[:, None, :], 3, axis=1)
                out.append(np.concatenate((front, -front[:, ::-1]), axis=0) if fill_back else front)
    return np.stack(out).astype(dt)


def vertex_normals(vertices, faces_idx, dt=np.float64):
    return _forward(vertices, faces_idx, dt, 'vertex')


def face_normals(vertices, faces_idx, dt=np.float64):
    return _forward(vertices, faces_idx, dt, 'face')


def corner_normals(vertices, faces_idx, smooth, fill_back, dt=np.float64):
    return _forward(vertices, faces_idx, dt, 'corner', smooth, fill_back)


def forward_mag(vertices, faces_idx):
    """(face magnitudes [B,Nf,3], vertex magnitudes [B,Nv,3]) of the forward bounds, float64."""
    v = np.asarray(vertices, np.float64)
    B, Nv = v.shape[:2]
    idx = _idx(faces_idx, B)
    fm, vm = [], []
    for b in range(B):
        a, c = _edges(v[b], idx[b])
        N, Nmag = _cross(a, c), _abs_cross(a, c)
        m, mmag = np.zeros((Nv, 3)), np.zeros((Nv, 3))
        for k in range(3):
            np.add.at(m, idx[b][:, k], N)
            np.add.at(mmag, idx[b][:, k], Nmag)
        fm.append(_normalize_mag(N, Nmag))
        vm.append(_normalize_mag(m, mmag))
    return np.stack(fm), np.stack(vm)


def corner_mag(vertices, faces_idx, smooth, fill_back):
    fm, vm = forward_mag(vertices, faces_idx)
    B = fm.shape[0]
    idx = _idx(faces_idx, B)
    out = []
    for b in range(B):
        front = vm[b][idx[b]] if smooth else np.repeat(fm[b][:, None, :], 3, axis=1)
        out.append(np.concatenate((front, front[:, ::-1]), axis=0) if fill_back else front)
    return np.stack(out)


def forward_k(faces_idx, Nv, what, B=1):
    """The n of gamma_n per face (scalar) or per vertex ([B,Nv,1])."""
    if what == 'face':
        return 5 + 6
    return (5 + np.maximum(degrees(faces_idx, Nv, B), 1) - 1 + 6)[..., None].astype(np.float64)


def corner_k(faces_idx, Nv, smooth, fill_back, B=1):
    if not smooth:
        return 5 + 6
    idx = _idx(faces_idx, B)
    k = forward_k(faces_idx, Nv, 'vertex', B)
    out = []
    for b in range(B):
        front = k[b][idx[b]]  # [Nf,3,1]
        out.append(np.concatenate((front, front[:, ::-1]), axis=0) if fill_back else front)
    return np.stack(out)


def backward_k(faces_idx, Nv, B=1):
    return 24 + 3 * int(degrees(faces_idx, Nv, B).max())


def _normalize_bwd(x, xmag, g, gmag):
    """normalize's backward at x from g, and its magnitude (module docstring)."""
    r = np.sqrt((x * x).sum(-1))
    s = r + NORM_EPS
    with np.errstate(all='ignore'):
        k = np.where(r > 0, (g * x).sum(-1) / (s * s * r), 0.0)
        kappa = np.where(r > 0, (np.abs(x) * xmag).sum(-1) / (r * r), 0.0)
        kmag = np.where(r > 0, (gmag * xmag).sum(-1) * kappa / (s * s * r), 0.0)  # (includes the |g . m| term)
    return g / s[..., None] - x * k[..., None], gmag / s[..., None] + xmag * kmag[..., None]


def adjoint64(vertices, faces_idx, g, what, smooth=False, fill_back=True):
    """(grad_vertices [B,Nv,3], its magnitude) in float64 from g: grad_normals [B,Nv,3] ('vertex'), [B,Nf,3] ('face') or
    grad_corner [B,F,3,3] ('corner')."""
    v = np.asarray(vertices, np.float64)
    g = np.asarray(g, np.float64)
    B, Nv = v.shape[:2]
    idx = _idx(faces_idx, B)
    Nf = idx.shape[1]
    gv, gv_mag = np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3))
    per_vertex = what == 'vertex' or (what == 'corner' and smooth)
    for b in range(B):
        ix = idx[b]
        a, c = _edges(v[b], ix)
        N, Nmag = _cross(a, c), _abs_cross(a, c)
        if what == 'corner':
            t = g[b, :Nf].copy()
            tmag = np.abs(t)
            if fill_back:
                t -= g[b, Nf:][:, ::-1]
                tmag += np.abs(g[b, Nf:][:, ::-1])
        if per_vertex:
            m, mmag = np.zeros((Nv, 3)), np.zeros((Nv, 3))
            for k in range(3):
                np.add.at(m, ix[:, k], N)
                np.add.at(mmag, ix[:, k], Nmag)
            if what == 'vertex':
                s, smag = g[b], np.abs(g[b])
            else:
                s, smag = np.zeros((Nv, 3)), np.zeros((Nv, 3))
                for k in range(3):
                    np.add.at(s, ix[:, k], t[:, k])
                    np.add.at(smag, ix[:, k], tmag[:, k])
            gm, gm_mag = _normalize_bwd(m, mmag, s, smag)
            gN, gN_mag = gm[ix].sum(1), gm_mag[ix].sum(1)
        else:
            s, smag = (g[b], np.abs(g[b])) if what == 'face' else (t.sum(1), tmag.sum(1))
            gN, gN_mag = _normalize_bwd(N, Nmag, s, smag)
        ga, gb = _cross(c, gN), _cross(gN, a)
        ga_mag, gb_mag = _abs_cross(c, gN_mag), _abs_cross(gN_mag, a)
        for k, (t_, tm) in enumerate(((ga, ga_mag), (-(ga + gb), ga_mag + gb_mag), (gb, gb_mag))):
            np.add.at(gv[b], ix[:, k], t_)
            np.add.at(gv_mag[b], ix[:, k], tm)
    return gv, gv_mag


def worst_ratio(got, ref, bound):
    """max over the entries of |got - ref| / bound, 0 / 0 = 0 and x / 0 = inf: <= 1 is the bound, with equality where it is 0."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    bound = np.broadcast_to(bound, d.shape)
    with np.errstate(all='ignore'):
        r = np.where(d == 0, 0.0, d / bound)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# meshes

def _grid(n):
    """An open n x n grid of vertices in the plane z = 0.1 x y, two triangles per cell."""
    xs = np.linspace(-0.8, 0.8, n)
    v = np.array([(x, y, 0.1 * x * y) for y in xs for x in xs], np.float64)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            p = j * n + i
            f += [(p, p + 1, p + n), (p + 1, p + n + 1, p + n)]
    return v, np.asarray(f, np.int32)


def _fan(n):
    """n triangles around vertex 0 (valence n): a long adjacency row."""
    ang = 2 * np.pi * np.arange(n) / n
    v = np.concatenate(([[0.0, 0.0, 0.3]], np.stack((np.cos(ang), np.sin(ang), 0.05 * np.cos(3 * ang)), axis=1)))
    f = np.asarray([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)], np.int32)
    return v, f


def meshes():
    """name -> (vertices [Nv,3] float64, faces [Nf,3] int32).  'degenerate': the last vertex has no face, the last face has a
    repeated vertex (zero area: its edge v0 - v1 is exactly 0)."""
    tri = (np.array([(0.1, 0.2, 0.3), (0.9, -0.1, 0.2), (0.3, 0.8, -0.4)]), np.asarray([(0, 1, 2)], np.int32))
    gv, gf = _grid(3)
    dv, df = _grid(3)
    dv = np.concatenate((dv, [[0.3, -0.2, 0.7]]))            # vertex 9: no face
    df = np.concatenate((df, [[4, 4, 8]])).astype(np.int32)  # a zero-area face on two vertices of the grid
    qv = np.array([(0.0, 0.0, 0.0), (1.0, 0.1, 0.0), (0.2, 0.9, 0.3), (0.8, 0.9, -0.2)])
    return {
        'triangle': tri,
        'grid3': (gv, gf),
        'fan12': _fan(12),
        'icosphere1': vertex_ref.icosphere(1),
        'icosphere3': vertex_ref.icosphere(3),
        'twin_faces': (qv, np.asarray([(0, 1, 2), (0, 1, 2), (1, 3, 2)], np.int32)),
        'degenerate': (dv, df),
    }


def batch(name, B, seed=0, per_image_topology=False):
    """(vertices [B,Nv,3] float32: the mesh jittered per image, faces [Nf,3] or -- per_image_topology -- [B,Nf,3] int32 with
    another face order and corner rotation per image)."""
    v, f = meshes()[name]
    rng = np.random.default_rng(4100 + seed)
    vb = (v[None] + rng.normal(scale=0.02, size=(B,) + v.shape)).astype(np.float32)
    if per_image_topology:
        keep = len(f) - 1 if name == 'degenerate' else len(f)   # (the zero-area face stays last)
        fs = []
        for _ in range(B):
            head = f[:keep][rng.permutation(keep)]
            head = np.stack([np.roll(row, rng.integers(3)) for row in head])
            fs.append(np.concatenate((head, f[keep:]), axis=0))
        f = np.stack(fs).astype(np.int32)
    return vb, f
