"""The yardstick of the edge-length and the cotangent Laplacian loss (neural_renderer_amd/mesh_losses.py): a float64
restatement of the two definitions on the meshes of tests/mesh_loss_ref.py, with tables built here from sets and dicts, gradients
from float64 autograd -- the cotangent weights detached: they are constants of the step, which is the definition -- and, with
every value, the magnitude its float32 evaluation is measured against: the float64 sum of the absolute values of every term of
the chain that leads to it.

u = 2^-24.  A check is |got - ref| <= C u M for every entry, exact equality where M = 0 (mesh_loss_ref.worst_ratio).
  Edge length, per edge d = x_v1 - x_v0, l = |d|, r = l - t:
    loss  M = sum_e [2 |r| (l + |t|) + r^2]   (t = 0 without a target tensor: sum_e 3 |d|^2)
    gradient entry (v, k)  M = 2 |g_b| sum_{u in N(v)} ((l + |t|) / l) |d_k|   (an edge with l = 0 adds nothing)
  Cotangent, per corner: Mc = |a| |b| / sqrt(|a x b|^2 + eps) -- the dot product cancels, so |cot| itself is the wrong scale
  (0 for a face with a repeated index); per vertex and component k
    MH_(v,k) = 1/2 sum_{(f,c) of v} [Mc_(c+2) |x_(c+1) - x_v|_k + Mc_(c+1) |x_(c+2) - x_v|_k]
    loss  M = sum_(v,k) 2 |H| MH + loss
    gradient entry (v, k)  M = |g_b| sum_{(f,c) of v} [Mc_(c+2) (MH_(c+1) + MH_v) + Mc_(c+1) (MH_(c+2) + MH_v)]_k
"""
import functools

import numpy as np
import torch

import mesh_loss_ref as R

U, UPSTREAM, B = R.U, R.UPSTREAM, R.B
KINDS = ('edge', 'cot')
TARGETS = ('zero', 'number', 'E', 'BE')     # the forms of edge_length_loss's target
EPS = 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the tables, with sets and dicts

def edge_tables(faces, num_vertices):
    """-> (edges: sorted list of (v0, v1) with v0 < v1; nbr_edge: per vertex, the edge number of each of its neighbours in
    ascending neighbour order)"""
    pairs = set()
    for tri in np.asarray(faces).tolist():
        for p in tri:
            for q in tri:
                if p < q:
                    pairs.add((p, q))
    edges = sorted(pairs)
    number = {e: i for i, e in enumerate(edges)}
    around = [[] for _ in range(num_vertices)]
    for p, q in edges:
        around[p].append(q)
        around[q].append(p)
    nbr_edge = [[number[(min(v, u), max(v, u))] for u in sorted(us)] for v, us in enumerate(around)]
    return edges, nbr_edge


def corner_entries(faces, num_vertices):
    """per vertex the list of 3 f + c of its (face, corner) pairs, ascending"""
    ent = {}
    for f, tri in enumerate(np.asarray(faces).tolist()):
        for c, v in enumerate(tri):
            ent.setdefault(v, []).append(3 * f + c)
    return [sorted(ent.get(v, [])) for v in range(num_vertices)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def copy_of(name, seed):
    """A differently-seeded noisy copy of the mesh behind R.inputs(name): float32 [B,Nv,3]"""
    base = R.icosphere(1)[0] if name == 'degenerate' else R.mesh(name)[0]
    return R.batch(base, 100 + seed, 0.03)


@functools.lru_cache(maxsize=None)
def target(name, seed, form):
    """The target of `form` for R.inputs(name, seed): 0.0; a number near the mean length; float32 [E] / [B,E] -- the edge
    lengths of copy_of (image 0 / every image).  Treat as read-only."""
    if form == 'zero':
        return 0.0
    v, f = R.inputs(name, seed)
    edges, _ = edge_tables(f, v.shape[1])
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if form == 'number':
        x = v.astype(np.float64)
        return float(np.round(np.sqrt(((x[:, e[:, 1]] - x[:, e[:, 0]]) ** 2).sum(2)).mean(), 3))
    x = copy_of(name, seed).astype(np.float64)
    lengths = np.sqrt(((x[:, e[:, 1]] - x[:, e[:, 0]]) ** 2).sum(2)).astype(np.float32)
    return np.ascontiguousarray(lengths[0] if form == 'E' else lengths)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement

def _grad(loss, x, g):
    if not loss.requires_grad:   # (no edge)
        return np.zeros(tuple(x.shape))
    return torch.autograd.grad((loss * torch.as_tensor(np.asarray(g, np.float64)[:x.shape[0]])).sum(), x)[0].numpy()


def edge_value(x, edges, t):
    """x: a float64 torch tensor [B,Nv,3]; t: a number, or an array [E] / [B,E] -> (loss [B], l [B,E], d [B,E,3])"""
    e = torch.as_tensor(np.asarray(edges, np.int64).reshape(-1, 2))
    d = x[:, e[:, 1]] - x[:, e[:, 0]]
    n = (d * d).sum(2)
    if isinstance(t, float) and t == 0.0:
        return n.sum(1), torch.sqrt(n.detach()), d
    pos = n > 0
    l = torch.where(pos, torch.sqrt(torch.where(pos, n, torch.ones_like(n))), torch.zeros_like(n))   # gradient 0 at l = 0
    r = l - torch.as_tensor(np.asarray(t, np.float64))
    return (r * r).sum(1), l, d


def edge_ref(vertices, faces, t=0.0, g=UPSTREAM):
    xn = np.asarray(vertices, np.float64)
    edges, _ = edge_tables(faces, xn.shape[1])
    if not edges:
        z = np.zeros(xn.shape[0])
        return R.Result(z, z.copy(), np.zeros_like(xn), np.zeros_like(xn))
    x = torch.tensor(xn, requires_grad=True)
    loss, l, d = edge_value(x, edges, t)
    grad = _grad(loss, x, g)
    l, d = l.detach().numpy(), np.abs(d.detach().numpy())
    tt = np.broadcast_to(np.abs(np.asarray(t, np.float64)), l.shape)
    r = l - tt
    if isinstance(t, float) and t == 0.0:
        loss_mag = 3 * (l * l).sum(1)
    else:
        loss_mag = (2 * np.abs(r) * (l + tt) + r * r).sum(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = np.where(l > 0, (l + tt) / l, 0.0)
    per_edge = k[:, :, None] * d                                         # [B,E,3]
    M = np.zeros_like(xn)
    for i, (p, q) in enumerate(edges):
        M[:, p] += per_edge[:, i]
        M[:, q] += per_edge[:, i]
    M *= 2 * np.abs(np.asarray(g, np.float64)[:xn.shape[0]])[:, None, None]
    return R.Result(loss.detach().numpy(), loss_mag, grad, M)


def cot_terms(x, faces, eps=EPS):
    """x float64 torch [B,Nv,3] -> (cot [B,F,3], Mc [B,F,3]) with zeros for a face with a repeated index"""
    idx = torch.as_tensor(np.asarray(faces, np.int64).reshape(-1, 3))
    ok = torch.as_tensor([len(set(tri)) == 3 for tri in np.asarray(faces).tolist()])
    p = x[:, idx]
    cot, mag = [], []
    for c in range(3):
        a, b = p[:, :, (c + 1) % 3] - p[:, :, c], p[:, :, (c + 2) % 3] - p[:, :, c]
        n = torch.cross(a, b, dim=2)
        s = torch.sqrt((n * n).sum(2) + eps)
        cot.append((a * b).sum(2) / s)
        mag.append(torch.sqrt((a * a).sum(2)) * torch.sqrt((b * b).sum(2)) / s)
    zero = torch.zeros_like(cot[0])
    return (torch.stack([torch.where(ok[None], t, zero) for t in cot], dim=2),
            torch.stack([torch.where(ok[None], t, zero) for t in mag], dim=2))


def cot_apply(phi, w, faces, entries, absolute=False):
    """L(phi) [B,Nv,3] with the weights w [B,F,3]: every vertex's (face, corner) entries one by one.  absolute: the sum of the
    absolute values of the terms instead."""
    tris = np.asarray(faces).tolist()
    rows = []
    for v, ent in enumerate(entries):
        h = torch.zeros_like(phi[:, v])
        for fc in ent:
            f, c = divmod(fc, 3)
            i1, i2 = tris[f][(c + 1) % 3], tris[f][(c + 2) % 3]
            w1, w2 = w[:, f, (c + 1) % 3, None], w[:, f, (c + 2) % 3, None]
            if absolute:
                h = h + w2 * (phi[:, i1] - phi[:, v]).abs() + w1 * (phi[:, i2] - phi[:, v]).abs()
            else:
                h = h + w2 * (phi[:, i1] - phi[:, v]) + w1 * (phi[:, i2] - phi[:, v])
        rows.append(0.5 * h)
    return torch.stack(rows, dim=1)


def cot_value(x, w, faces, entries):
    """the loss [B] for the weights w, which are NOT differentiated"""
    H = cot_apply(x, w.detach(), faces, entries)
    return (H * H).sum((1, 2)), H


def cot_ref(vertices, faces, g=UPSTREAM, eps=EPS):
    xn = np.asarray(vertices, np.float64)
    entries = corner_entries(faces, xn.shape[1])
    tris = np.asarray(faces).tolist()
    x = torch.tensor(xn, requires_grad=True)
    w, mc = cot_terms(x, faces, eps)
    loss, H = cot_value(x, w, faces, entries)
    grad = _grad(loss, x, g)
    with torch.no_grad():
        MH = cot_apply(x, mc, faces, entries, absolute=True)
        rows = []
        for v, ent in enumerate(entries):
            m = torch.zeros_like(MH[:, v])
            for fc in ent:
                f, c = divmod(fc, 3)
                i1, i2 = tris[f][(c + 1) % 3], tris[f][(c + 2) % 3]
                m = m + mc[:, f, (c + 2) % 3, None] * (MH[:, i1] + MH[:, v]) + mc[:, f, (c + 1) % 3, None] * (MH[:, i2] + MH[:, v])
            rows.append(m)
        M = torch.stack(rows, dim=1).numpy() * np.abs(np.asarray(g, np.float64)[:xn.shape[0]])[:, None, None]
        loss_mag = (2 * H.abs() * MH).sum((1, 2)) + loss
    return R.Result(loss.detach().numpy(), loss_mag.numpy(), grad, M)


@functools.lru_cache(maxsize=None)
def reference(kind, name, seed=0, form='zero'):
    """The restatement of `kind` ('edge' with the target `form` | 'cot') on R.inputs(name, seed), computed once and shared."""
    v, f = R.inputs(name, seed)
    return edge_ref(v, f, target(name, seed, form)) if kind == 'edge' else cot_ref(v, f)
