"""The yardstick of mesh subdivision (neural_renderer_amd/subdivision.py): the test meshes, and a float64 restatement of
the definition that builds its own tables with dicts and sets -- independent of the product's vectorised NumPy --, applies
them in float64 with the unrounded float64 weights, takes gradients as the transposed product and returns, with every
value, the magnitude its float32 evaluation is measured against.

u = 2^-24.  A check is |got - ref| <= C u M for every entry, exact equality where M = 0 (mesh_loss_ref.worst_ratio).
  M = |S_L| ... |S_1| |x|: the entrywise absolute tables applied to |x|; for gradients the transposed chain on |g|.
  C = sum over the levels of (longest row of that level's table + 3); for the backward the transposed tables' rows.
The bound is derived, not measured.  A row of n entries, evaluated as acc = w_0 x_0, acc = fma(w_k, x_k, acc): every weight
is rounded to float32 once (n relative errors u, one per term), the product and each fma round once (n roundings, each of
a partial sum of magnitude <= the row's M): at most (n + 1) u M to first order against the float64 row, and (n + 3) u M
leaves room for the second-order terms and for an evaluation that rounds products and sums separately (the torch path).
The error a level leaves in its output passes through the next level's absolute table, i.e. into that level's M, so the
constants of the levels add."""
import functools

import numpy as np

import mesh_loss_ref as M

U = M.U
B = M.B
worst_ratio = M.worst_ratio


# ---------------------------------------------------------------------------------------------------------------------
# meshes: the smallest at which each rule, and the launch shape, can go wrong

def odd_topology():
    """mesh_loss_ref's 'odd' without its face (0, 3, 3) (a repeated index is an error here): an isolated vertex, a
    duplicated face (three edges in three faces), an edge in three faces, vertices with three or more sharp edges."""
    v, f = M.mesh('odd')
    keep = [k for k, tri in enumerate(f.tolist()) if len(set(tri)) == 3]
    assert len(keep) == len(f) - 1
    return v, f[keep]


def triangle():
    """A single triangle: every row is a crease row (its three vertices have two sharp edges each)."""
    return np.array([[0.1, 0.2, 0.3], [1.2, -0.1, 0.4], [0.3, 1.1, -0.2]]), np.asarray([(0, 1, 2)], np.int32)


def _ring(n, z):
    t = 2 * np.pi * np.arange(n) / n
    return np.stack((np.cos(t), np.sin(t), np.full(n, z)), axis=1)


def closed_fan(n=12):
    """n triangles around vertex 0, a second apex n + 1 closing the surface: two interior vertices of valence n."""
    v = np.concatenate(([[0.0, 0.0, 0.6]], _ring(n, 0.0), [[0.0, 0.0, -0.7]]), axis=0)
    f = []
    for i in range(n):
        a, b = 1 + i, 1 + (i + 1) % n
        f += [(0, a, b), (n + 1, b, a)]
    return v, np.asarray(f, np.int32)


def open_fan(n=7):
    """n triangles around vertex 0 that do not close: the centre lies on the boundary (valence n + 1, two sharp edges)."""
    t = np.pi * np.arange(n + 1) / n
    v = np.concatenate(([[0.0, 0.0, 0.3]], np.stack((np.cos(t), np.sin(t), 0.1 * t), axis=1)), axis=0)
    return v, np.asarray([(0, 1 + i, 2 + i) for i in range(n)], np.int32)


def twin():
    """Two identical faces: every edge lies in two faces whose opposite vertices coincide (o1 = o2)."""
    v, f = triangle()
    return v, np.concatenate((f, f), axis=0)


_MESHES = {'tetra': lambda: M.mesh('tetra'), 'ico1': lambda: M.mesh('ico1'), 'grid': lambda: M.mesh('grid'),
           'odd': odd_topology, 'blocks': lambda: M.mesh('blocks'), 'triangle': triangle, 'closed_fan': closed_fan,
           'open_fan': open_fan, 'twin': twin}
MESHES = tuple(_MESHES)
LEVEL3 = ('tetra', 'ico1')          # the meshes that also run three levels
CLOSED = ('tetra', 'ico1', 'blocks', 'closed_fan')     # closed manifolds: E = 3 F / 2
SCHEMES = ('loop', 'midpoint')


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f = _MESHES[name]()
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def inputs(name, channels=3, seed=0):
    """(x float32 [B,Nv,C], faces int32 [F,3]); treat as read-only.  Built as mesh_loss_ref.batch builds its vertices: image k
    scaled 1 + 0.2 k and shifted 0.3 k, each with its own Gaussian noise.  The channels are the positions, cut to C or
    extended by random attributes."""
    v, f = mesh(name)
    rng = np.random.default_rng(5200 + 17 * seed + channels)
    base = v[:, :channels] if channels <= 3 else np.concatenate((v, rng.normal(size=(len(v), channels - 3))), axis=1)
    x = np.stack([base * (1 + 0.2 * k) + 0.3 * k for k in range(B)]) + rng.normal(scale=0.03, size=(B,) + base.shape)
    return np.ascontiguousarray(x.astype(np.float32)), f


def upstream(shape, seed=0):
    """A gradient of mixed signs for an output of `shape`, float32."""
    return np.random.default_rng(6300 + seed).normal(size=shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the tables, with dicts and sets

def level(faces, num_vertices, scheme):
    """One level -> (children: list of triples, Nv', rows: list of {column: float64 weight})."""
    faces = [tuple(int(i) for i in tri) for tri in np.asarray(faces).tolist()]
    opposite = {}
    for a, b, c in faces:
        for p, q, o in ((a, b, c), (b, c, a), (c, a, b)):
            opposite.setdefault((min(p, q), max(p, q)), []).append(o)
    edges = sorted(opposite)
    vertex_of = {e: num_vertices + k for k, e in enumerate(edges)}
    mid = lambda p, q: vertex_of[(min(p, q), max(p, q))]
    children = []
    for a, b, c in faces:
        ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
        children += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    rows = [dict() for _ in range(num_vertices + len(edges))]

    def add(r, col, w):
        rows[r][col] = rows[r].get(col, 0.0) + w
    if scheme == 'midpoint':
        for v in range(num_vertices):
            add(v, v, 1.0)
        for (p, q) in edges:
            add(vertex_of[(p, q)], p, 0.5)
            add(vertex_of[(p, q)], q, 0.5)
        return children, len(rows), rows
    assert scheme == 'loop'
    nbrs = [set() for _ in range(num_vertices)]
    sharp_nbrs = [set() for _ in range(num_vertices)]
    for (p, q) in edges:
        nbrs[p].add(q)
        nbrs[q].add(p)
        if len(opposite[(p, q)]) != 2:
            sharp_nbrs[p].add(q)
            sharp_nbrs[q].add(p)
    for v in range(num_vertices):
        n, s = len(nbrs[v]), len(sharp_nbrs[v])
        if n == 0:
            add(v, v, 1.0)
        elif s == 0:
            beta = 3.0 / 16.0 if n == 3 else 3.0 / (8.0 * n)
            add(v, v, 1.0 - n * beta)
            for u in nbrs[v]:
                add(v, u, beta)
        elif s == 2:
            add(v, v, 0.75)
            for u in sharp_nbrs[v]:
                add(v, u, 0.125)
        else:
            add(v, v, 1.0)
    for (p, q) in edges:
        r, opp = vertex_of[(p, q)], opposite[(p, q)]
        if len(opp) != 2:
            add(r, p, 0.5)
            add(r, q, 0.5)
        else:
            add(r, p, 0.375)
            add(r, q, 0.375)
            add(r, opp[0], 0.125)
            add(r, opp[1], 0.125)
    return children, len(rows), rows


def csr(rows):
    """rows -> (offsets int32, cols int32 ascending within a row, weights float64)"""
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    cols = [c for r in rows for c in sorted(r)]
    w = [r[c] for r in rows for c in sorted(r)]
    return off, np.asarray(cols, np.int32), np.asarray(w, np.float64)


def transpose(rows, num_in):
    out = [dict() for _ in range(num_in)]
    for r, row in enumerate(rows):
        for c, w in row.items():
            out[c][r] = w
    return out


class Plan(object):
    """faces [4^L F, 3] int32, face_parent, num_vertices, and per level the rows (dicts) of the table."""

    def __init__(self, faces, num_vertices, levels, scheme):
        self.num_vertices_in = num_vertices
        self.rows, self.sizes = [], [num_vertices]
        f = [tuple(t) for t in np.asarray(faces).tolist()]
        for _ in range(levels):
            f, num_vertices, rows = level(f, num_vertices, scheme)
            self.rows.append(rows)
            self.sizes.append(num_vertices)
        self.faces = np.asarray(f, np.int32).reshape(-1, 3)
        self.num_vertices = num_vertices
        self.face_parent = np.arange(len(self.faces)) // 4 ** levels
        self.constant = sum(max(len(r) for r in rows) + 3 for rows in self.rows)
        self.constant_backward = sum(max(len(r) for r in transpose(rows, n)) + 3 for rows, n in zip(self.rows, self.sizes))

    def _coo(self, k):
        off, cols, w = csr(self.rows[k])
        return np.repeat(np.arange(len(off) - 1), np.diff(off)), cols.astype(np.int64), w

    def apply(self, x, absolute=False):
        """x [B,Nv,C] float64 -> [B,Nv',C]; absolute: |tables| on |x|."""
        x = np.abs(np.asarray(x, np.float64)) if absolute else np.asarray(x, np.float64)
        for k in range(len(self.rows)):
            r, c, w = self._coo(k)
            y = np.zeros((x.shape[0], self.sizes[k + 1], x.shape[2]))
            np.add.at(y, (slice(None), r), x[:, c] * (np.abs(w) if absolute else w)[None, :, None])
            x = y
        return x

    def apply_transposed(self, g, absolute=False):
        """g [B,Nv',C] float64 -> [B,Nv,C]: the transposed chain."""
        g = np.abs(np.asarray(g, np.float64)) if absolute else np.asarray(g, np.float64)
        for k in reversed(range(len(self.rows))):
            r, c, w = self._coo(k)
            y = np.zeros((g.shape[0], self.sizes[k], g.shape[2]))
            np.add.at(y, (slice(None), c), g[:, r] * (np.abs(w) if absolute else w)[None, :, None])
            g = y
        return g


@functools.lru_cache(maxsize=None)
def plan(name, levels=1, scheme='loop'):
    v, f = mesh(name)
    return Plan(f, len(v), levels, scheme)


class Result(object):
    """value [B,Nv',C] and its magnitude; grad [B,Nv,C] for the upstream g [B,Nv',C] and its magnitude; the two constants"""

    def __init__(self, value, value_mag, g, grad, grad_mag, constant, constant_backward):
        self.value, self.value_mag, self.g, self.grad, self.grad_mag = value, value_mag, g, grad, grad_mag
        self.constant, self.constant_backward = constant, constant_backward


@functools.lru_cache(maxsize=None)
def reference(name, levels=1, scheme='loop', channels=3, seed=0):
    """The restatement on inputs(name, channels, seed) with upstream(shape, seed), computed once and shared.  The images are
    independent: image k of the result is the result of image k alone."""
    x, _ = inputs(name, channels, seed)
    p = plan(name, levels, scheme)
    value = p.apply(x)
    g = upstream(value.shape, seed)
    return Result(value, p.apply(x, True), g, p.apply_transposed(g), p.apply_transposed(g, True), p.constant,
                  p.constant_backward)


# ---------------------------------------------------------------------------------------------------------------------
# batches of more than B images: the seeds' batches one behind the other

def _seeds(images):
    return range((images + B - 1) // B)


def inputs_wide(name, channels, images):
    """x float32 [images,Nv,C]: inputs(name, channels, seed) for seed = 0, 1, .. concatenated and cut to `images`."""
    return np.ascontiguousarray(np.concatenate([inputs(name, channels, k)[0] for k in _seeds(images)])[:images])


def reference_wide(name, levels, scheme, channels, images):
    """The restatement on inputs_wide: the seeds' references concatenated (the images are independent)."""
    refs = [reference(name, levels, scheme, channels, k) for k in _seeds(images)]
    cat = lambda field: np.concatenate([getattr(r, field) for r in refs])[:images]
    return Result(cat('value'), cat('value_mag'), cat('g'), cat('grad'), cat('grad_mag'), refs[0].constant,
                  refs[0].constant_backward)

