"""Restatement of neural_renderer_amd/isosurface.py (DESIGN "Isosurface extraction") in NumPy, independent of the product's code
and of its case table -- the yardstick of tests/test_isosurface.py and test_isosurface_gpu.py -- with the bounds of the
positions and of the gradients, the manifold checks and the fields.  u = 2^-24 in float32, 2^-53 in float64.

The definition.  values [D,H,W]; node (i,j,k) is n = (i H + j) W + k; inside iff value < iso ('below') or value > iso ('above'), a
node at iso is outside.  Cell (i,j,k) is cut into six tetrahedra, one per permutation pi of (0,1,2) in lexicographic order:
c0 = (i,j,k), c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = (i+1,j+1,k+1).  A vertex lies on every tetrahedron edge with one inside end;
e(p,q) is the vertex on the edge of the local corners p, q.  One inside corner p, the others q < r < s: e(p,q), e(p,r), e(p,s);
three inside and p outside: the same; two inside p < q, outside r < s: the quad e(p,r), e(p,s), e(q,s), e(q,r) as (0,1,2), (0,2,3).
A triangle whose normal -- here: of the edges' MIDPOINTS, exact half-integers, so no rounding takes part -- does not point from
the inside corners' centroid to the outside corners' has its last two entries exchanged.  Faces: cells ascending by n, the
permutations in order, the triangles as above.  Vertices: numbered by sorting their (a, b), a < b the nodes of the edge.
Positions: t = (iso - s_a) / (s_b - s_a), v = p_a + t (p_b - p_a); p per axis lo + (i + 1/2)(hi - lo) / D ('centers') or lo + i (hi -
lo) / (D - 1) ('corners'), computed in float64 and rounded ONCE to the dtype under test -- the rounded p, the values and iso are
the exact inputs of what follows.

Bounds, by counting roundings (each <= u relative; the second order is covered by the factor 1 + 64 u).
  t     two differences and a quotient: 3 u |t|
  v_c   the difference e_c = p_b - p_a (1), the product t e_c (t's 3, e's 1, its own 1: 5 u |t e_c|), the sum (u |v_c|, and
        |v_c| <= |p_a| + |t e_c|):   bound_c = u (6 |t e_c| + |p_a,c|)
  The restatement is itself float64 arithmetic: its own error, the same expression with 2^-53, is added.
Gradients of L = sum g . v, g [Nv,3].  With n = iso - s_a, d = s_b - s_a, G = g . e, M_G = sum_c |g_c e_c|:
  dL/ds_a = -(G / d)(1 - t),   dL/ds_b = -(G / d) t,   dL/dp_a = g (1 - t),   dL/dp_b = g t.
  autograd: grad_t = sum_c g_c e_c: e's rounding, a product, two additions: 4 u M_G.  grad_n = grad_t / d: d's rounding and the
  quotient: 6 u M_G / |d|.  grad_d = -grad_t ((n / d) / d): t's 3, d's 1 and a quotient, grad_t's 4 and a product: 10 u M_G |t| / |d|.
  s_a takes -grad_n - grad_d, one more addition on |grad_n| + |grad_d|: <= u (M_G / |d|)(7 + 11 |t|) <= C_S u A,  A = (M_G / |d|)(1 + |t|);
  s_b takes -grad_d: 10 u B <= C_S u B,  B = (M_G / |d|) |t|.   C_S = 11.
  p_a takes g - g t: t's 3 and the product (4 u |g t|), the addition (u (|g| + |g t|)): <= C_P u |g_c| (1 + |t|);  p_b takes g t:
  4 u |g_c t|.   C_P = 5.
  A node collects the terms of its K edges (14 at most) through torch's indexing backward, which adds in no fixed order:
  K - 1 additions, each within u of the sum of the terms' magnitudes.  An entry's bound is (K + C) u x the sum of its terms'
  magnitudes -- plus the restatement's own, with 2^-53.  A node on no crossing edge gets exactly 0."""
import itertools

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
C_S, C_P = 11.0, 5.0
SECOND = 1.0 + 64 * U

PERMUTATIONS = list(itertools.permutations((0, 1, 2)))  # lexicographic


def unit(dtype):
    return U if np.dtype(dtype) == np.float32 else U64


def inside_of(values, iso, inside):
    values = np.asarray(values)
    level = values.dtype.type(iso)
    return values > level if inside == 'above' else values < level


def extract(values, iso=0.0, inside='below'):
    """-> (edge_nodes [Nv,2] int64, faces [F,3] int64): a plain loop over cells and tetrahedra"""
    values = np.asarray(values)
    D, H, W = values.shape
    ins = inside_of(values, iso, inside)
    node = lambda c: (c[0] * H + c[1]) * W + c[2]
    triangles = []  # triples of (a, b)
    mixed = np.zeros((D - 1, H - 1, W - 1), bool)
    for di, dj, dk in itertools.product((0, 1), repeat=3):
        mixed |= ins[di:D - 1 + di, dj:H - 1 + dj, dk:W - 1 + dk] != ins[:D - 1, :H - 1, :W - 1]
    for i, j, k in np.argwhere(mixed):  # ascending n; a cell with eight equal corners has no face
        for perm in PERMUTATIONS:
            c = [np.array((i, j, k))]
            for axis in perm:
                c.append(c[-1] + np.eye(3, dtype=int)[axis])
            flags = [bool(ins[tuple(x)]) for x in c]
            inner = [p for p in range(4) if flags[p]]
            outer = [p for p in range(4) if not flags[p]]
            if len(inner) in (1, 3):
                p = inner[0] if len(inner) == 1 else outer[0]
                q, r, s = [x for x in range(4) if x != p]
                tris = [[(p, q), (p, r), (p, s)]]
            elif len(inner) == 2:
                (p, q), (r, s) = inner, outer
                quad = [(p, r), (p, s), (q, s), (q, r)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            else:
                continue
            towards = np.mean([c[p] for p in outer], 0) - np.mean([c[p] for p in inner], 0)
            for tri in tris:
                m = [(c[a] + c[b]) / 2.0 for a, b in tri]
                side = np.dot(np.cross(m[1] - m[0], m[2] - m[0]), towards)
                assert side != 0
                if side < 0:
                    tri = [tri[0], tri[2], tri[1]]
                triangles.append([tuple(sorted((node(c[a]), node(c[b])))) for a, b in tri])
    edges = sorted(set(e for tri in triangles for e in tri))
    number = {e: n for n, e in enumerate(edges)}
    faces = np.array([[number[e] for e in tri] for tri in triangles], np.int64).reshape(-1, 3)
    return np.array(edges, np.int64).reshape(-1, 2), faces


def crossing_edges(values, iso=0.0, inside='below'):
    """the sorted (a, b) of all grid edges of the 7 kinds with one inside end -- from the grid alone, not from the faces"""
    values = np.asarray(values)
    D, H, W = values.shape
    ins = inside_of(values, iso, inside)
    n = np.arange(D * H * W).reshape(D, H, W)
    out = []
    for di, dj, dk in list(itertools.product((0, 1), repeat=3))[1:]:
        lo, hi = (slice(0, D - di), slice(0, H - dj), slice(0, W - dk)), (slice(di, D), slice(dj, H), slice(dk, W))
        cross = ins[lo] != ins[hi]
        out.append(np.stack((n[lo][cross], n[hi][cross]), 1))
    out = np.concatenate(out)
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def case_histogram(values, iso=0.0, inside='below'):
    """[6,16]: how many tetrahedra of each permutation show each 4-bit inside mask (bit p: corner p) -- about the input"""
    values = np.asarray(values)
    D, H, W = values.shape
    ins = inside_of(values, iso, inside)
    hist = np.zeros((6, 16), np.int64)
    for t, perm in enumerate(PERMUTATIONS):
        off, mask = np.zeros(3, int), np.zeros((D - 1, H - 1, W - 1), np.int64)
        for p in range(4):
            mask |= ins[off[0]:D - 1 + off[0], off[1]:H - 1 + off[1], off[2]:W - 1 + off[2]].astype(np.int64) << p
            if p < 3:
                off[perm[p]] += 1
        hist[t] = np.bincount(mask.reshape(-1), minlength=16)
    return hist


def node_positions(shape, bounds, align, dtype):
    """[D H W,3]: the nodes' positions, float64 rounded once to `dtype` (then float64 again: exact inputs)"""
    pairs = [tuple(b) for b in bounds] if hasattr(bounds[0], '__len__') else [tuple(bounds)] * 3
    axes = []
    for (lo, hi), n in zip(pairs, shape):
        i = np.arange(n, dtype=np.float64)
        axes.append(lo + (i + 0.5) * ((hi - lo) / n) if align == 'centers' else lo + i * ((hi - lo) / (n - 1)))
    grid = np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3)
    return grid.astype(dtype).astype(np.float64)


def positions(values, edge_nodes, iso, node_pos, dtype):
    """-> (v [Nv,3] float64, bound [Nv,3]) for the dtype under test"""
    s = np.asarray(values, np.float64).reshape(-1)
    p = np.asarray(node_pos, np.float64).reshape(-1, 3)
    a, b = edge_nodes[:, 0], edge_nodes[:, 1]
    level = float(np.dtype(dtype).type(iso))
    t = (level - s[a]) / (s[b] - s[a])
    e = p[b] - p[a]
    v = p[a] + t[:, None] * e
    mag = 6 * np.abs(t[:, None] * e) + np.abs(p[a])
    return v, (unit(dtype) + U64) * SECOND * mag


def gradients(values, edge_nodes, iso, node_pos, g, dtype):
    """of L = sum g . v -> ((grad_values [N], bound), (grad_positions [N,3], bound))"""
    s = np.asarray(values, np.float64).reshape(-1)
    p = np.asarray(node_pos, np.float64).reshape(-1, 3)
    g = np.asarray(g, np.float64)
    a, b = edge_nodes[:, 0], edge_nodes[:, 1]
    level = float(np.dtype(dtype).type(iso))
    d = s[b] - s[a]
    t = (level - s[a]) / d
    e = p[b] - p[a]
    G, MG = (g * e).sum(1), np.abs(g * e).sum(1)
    N = s.shape[0]
    K = np.bincount(np.concatenate((a, b)), minlength=N).astype(np.float64)
    assert K.max(initial=0) <= 14
    gs, ms = np.zeros(N), np.zeros(N)
    np.add.at(gs, a, -(G / d) * (1 - t))
    np.add.at(gs, b, -(G / d) * t)
    np.add.at(ms, a, (MG / np.abs(d)) * (1 + np.abs(t)))
    np.add.at(ms, b, (MG / np.abs(d)) * np.abs(t))
    gp, mp = np.zeros((N, 3)), np.zeros((N, 3))
    np.add.at(gp, a, g * (1 - t)[:, None])
    np.add.at(gp, b, g * t[:, None])
    np.add.at(mp, a, np.abs(g) * (1 + np.abs(t))[:, None])
    np.add.at(mp, b, np.abs(g) * np.abs(t)[:, None])
    u = (unit(dtype) + U64) * SECOND
    return (gs, (K + C_S) * u * ms), (gp, (K[:, None] + C_P) * u * mp)


def ratio(err, bound):
    """the worst err / bound; an entry with bound 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# manifold checks

def mesh_report(faces, num_vertices):
    """-> dict: the largest count of a directed edge, how many undirected edges lie in 1 / 2 / more faces, the Euler
    characteristic V - E + F, whether every vertex is used; the boundary edges as vertex pairs"""
    faces = np.asarray(faces, np.int64)
    directed = np.concatenate((faces[:, (0, 1)], faces[:, (1, 2)], faces[:, (2, 0)]))
    _, counts = np.unique(directed, axis=0, return_counts=True)
    und, ucounts = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
    return dict(directed_max=int(counts.max(initial=0)), once=int((ucounts == 1).sum()), twice=int((ucounts == 2).sum()),
                more=int((ucounts > 2).sum()), euler=int(num_vertices - len(und) + len(faces)),
                all_used=bool(len(np.unique(faces)) == num_vertices), boundary=und[ucounts == 1])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------------
# fields

def sphere_field(G=12):
    """the sphere row: 770 vertices, 1 536 faces at iso = 0"""
    c = np.arange(G, dtype=np.float64) - (G - 1) / 2.0
    x, y, z = np.meshgrid(c + 0.013, c + 0.083, c - 0.018, indexing='ij')
    return (np.sqrt(x * x + y * y + z * z) - 3.72).astype(np.float32)


def lattice_field():
    """the lattice row: 26 nodes exactly at iso = 0; 229 vertices, 396 faces"""
    i, j, k = np.meshgrid(np.arange(6), np.arange(5), np.arange(7), indexing='ij')
    return (i + j + k - 7).astype(np.float32)


def torus_field(G=12):
    c = np.arange(G, dtype=np.float64) - (G - 1) / 2.0
    x, y, z = np.meshgrid(c + 0.021, c - 0.034, c + 0.057, indexing='ij')
    return (np.sqrt((np.sqrt(x * x + y * y) - 3.4) ** 2 + z * z) - 1.45).astype(np.float32)


def noise_field(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def smooth_noisy_field(shape=(64, 48, 80), seed=5):
    """a smooth field with low-amplitude noise: every tetrahedron case occurs (case_histogram)"""
    D, H, W = shape
    x, y, z = np.meshgrid(np.linspace(-1, 1, D), np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing='ij')
    f = np.sin(3.1 * x + 0.4) * np.cos(2.3 * y - 0.2) + 0.6 * np.sin(2.7 * z + 0.9 * x) - 0.1
    return (f + 0.05 * np.random.default_rng(seed).normal(size=shape)).astype(np.float32)


ROWS = {'sphere': (sphere_field, 770, 1536), 'lattice': (lattice_field, 229, 396)}
