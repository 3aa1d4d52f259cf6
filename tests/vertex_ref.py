"""Test-side restatements of vertex colours and smooth shading (include/nr_hip.h: nr_forward_rasterize_corner,
nr_backward_corner_colors, nr_vertex_shade_forward / _backward) in NumPy, written from the header's arithmetic:

  corner_render / corner_adjoint   the rasterizer's corner mode from the maps a forward returned: float32 in the kernel's
                                   operation order, and the adjoint in float64 with the sum of |terms| of every entry
  shade32                          vertex shading in float32 in the kernels' operation order (normal sums in ascending
                                   (face, corner) order)
  shade64 / shade_adjoint64        the same function in float64 and its adjoint with per-entry term magnitudes
  icosphere                        a unit sphere mesh for the tests that need a well-conditioned closed surface
"""
import numpy as np

f32 = np.float32
NORM_EPS = 1e-5


class Light(object):
    def __init__(self, ia=0.5, id=0.5, ca=(1, 1, 1), cd=(1, 1, 1), direction=(0, 1, 0)):
        self.ia, self.id = float(ia), float(id)
        self.ca, self.cd, self.dir = (np.asarray(x, np.float64) for x in (ca, cd, direction))

    def kwargs(self):
        return dict(intensity_ambient=self.ia, intensity_directional=self.id, color_ambient=self.ca.tolist(),
                    color_directional=self.cd.tolist(), direction=self.dir.tolist())


# ---------------------------------------------------------------------------------------------------------------------
# rasterizer, corner mode

def _weights(faces, fi, wm, dm):
    """(b, f of the covered pixels, d [N,3] float32 = fmin(fmax(w * (zp / z), 0), 1))."""
    b, y, x = np.nonzero(fi >= 0)
    f = fi[b, y, x]
    z = faces[b, f][:, :, 2].astype(f32)
    with np.errstate(all='ignore'):
        d = np.fmin(np.fmax(wm[b, y, x].astype(f32) * (dm[b, y, x].astype(f32)[:, None] / z), f32(0)), f32(1))
    return (b, y, x), f, d


def corner_render(faces, fi, wm, dm, corner, background):
    """rgb_map [B,S,S,3] float32: (C0 d0 + C1 d1) + C2 d2, then * 1 + 0 * bg; uncovered pixels 0 * 0 + 1 * bg."""
    B, S = fi.shape[:2]
    bg = np.asarray(background, f32)
    bg = np.broadcast_to(bg if bg.ndim == 2 else bg[None], (B, 3))
    out = np.empty((B, S, S, 3), f32)
    out[:] = (f32(0) * f32(0) + f32(1) * bg)[:, None, None, :]
    (b, y, x), f, d = _weights(faces, fi, wm, dm)
    C = corner[b, f].astype(f32)  # [N,3(k),3(c)]
    with np.errstate(all='ignore'):
        rgb = (C[:, 0] * d[:, 0:1] + C[:, 1] * d[:, 1:2]) + C[:, 2] * d[:, 2:3]
        rgb = rgb * f32(1) + f32(0) * bg[b]
    out[b, y, x] = rgb
    return out


def corner_adjoint(faces, fi, wm, dm, g, F):
    """grad_corner [B,F,3,3] in float64 (the forward's float32 d_k, products and sums in double) and the sum of |terms|."""
    B = fi.shape[0]
    (b, y, x), f, d = _weights(faces, fi, wm, dm)
    terms = g[b, y, x].astype(np.float64)[:, None, :] * d.astype(np.float64)[:, :, None]  # [N,k,c]
    grad = np.zeros((B, F, 3, 3))
    mag = np.zeros((B, F, 3, 3))
    np.add.at(grad, (b, f), terms)
    np.add.at(mag, (b, f), np.abs(terms))
    return grad, mag


# ---------------------------------------------------------------------------------------------------------------------
# vertex shading

def _idx(faces_idx, B):
    idx = np.asarray(faces_idx, np.int64)
    if idx.ndim == 2:
        idx = idx[None]
    return np.broadcast_to(idx, (B,) + idx.shape[1:])


def _colors(colors, B):
    c = np.asarray(colors)
    if c.ndim == 2:
        c = c[None]
    return np.broadcast_to(c, (B,) + c.shape[1:])


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _light(nsum, L, dt):
    """The light colours seen by the faces and by their reversed copies from (sums of) unnormalised normals [...,3], in the
    operation order of the front-end's face_light; also n_hat . direction."""
    ca, cd, direction = (x.astype(dt) for x in (L.ca, L.cd, L.dir))
    ia, idir = dt(L.ia), dt(L.id)
    amb = ia * ca if L.ia != 0 else np.zeros(3, dt)
    if L.id == 0:
        a = np.broadcast_to(amb, nsum.shape).astype(dt)
        return a, a, np.zeros(nsum.shape[:-1], dt)
    s = np.sqrt(_dot(nsum, nsum)) + dt(NORM_EPS)
    nh = nsum / s[..., None]
    dot = _dot(nh, direction)
    front = amb + idir * (cd * np.fmax(dot, dt(0))[..., None])
    back = amb + idir * (cd * np.fmax(-dot, dt(0))[..., None])
    return front.astype(dt), back.astype(dt), dot


def _shade(vertices, faces_idx, colors, L, fill_back, smooth, dt):
    v = np.asarray(vertices, dt)
    B, Nv = v.shape[:2]
    idx = _idx(faces_idx, B)
    col = _colors(np.asarray(colors, dt), B)
    Nf = idx.shape[1]
    out = np.zeros((B, 2 * Nf if fill_back else Nf, 3, 3), dt)
    for b in range(B):
        w = v[b][idx[b]]  # [Nf,3,3]
        n = _cross(w[:, 0] - w[:, 1], w[:, 2] - w[:, 1])
        cf = col[b][idx[b]]
        if smooth:
            m = np.zeros((Nv, 3), dt)
            for e in range(3 * Nf):  # ascending (face, corner): the kernels' order
                m[idx[b, e // 3, e % 3]] += n[e // 3]
            lf, lb, _ = _light(m, L, dt)
            lf, lb = lf[idx[b]], lb[idx[b]]
        else:
            lf, lb, _ = _light(n, L, dt)
            lf, lb = lf[:, None, :], lb[:, None, :]
        out[b, :Nf] = cf * lf
        if fill_back:
            out[b, Nf:] = (cf * lb)[:, ::-1]
    return out


def shade32(vertices, faces_idx, colors, L, fill_back, smooth):
    with np.errstate(all='ignore'):
        return _shade(vertices, faces_idx, colors, L, fill_back, smooth, f32)


def shade64(vertices, faces_idx, colors, L, fill_back, smooth):
    return _shade(vertices, faces_idx, colors, L, fill_back, smooth, np.float64)


def face_light32(vertices, faces_idx, L):
    """(light of the faces, light of their reversed copies) [B,Nf,3] float32: nr_frontend_forward_light's colours."""
    v = np.asarray(vertices, f32)
    idx = _idx(faces_idx, v.shape[0])
    w = np.stack([v[b][idx[b]] for b in range(v.shape[0])])
    with np.errstate(all='ignore'):
        lf, lb, _ = _light(_cross(w[:, :, 0] - w[:, :, 1], w[:, :, 2] - w[:, :, 1]), L, f32)
    return lf, lb


def _abs_cross(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack((a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), axis=-1)


def _light_bwd(nsum, dot, glf, glb, glf_mag, glb_mag, L):
    """Gradient of the normal sums from the gradients of the two light colours, and its magnitude before cancellation."""
    if L.id == 0:
        return np.zeros_like(nsum), np.zeros_like(nsum)
    gcf, gcb = L.id * (glf @ L.cd), L.id * (glb @ L.cd)
    gdot = np.where(dot > 0, gcf, 0.0) - np.where(-dot > 0, gcb, 0.0)
    gdot_mag = np.where(dot > 0, abs(L.id) * (glf_mag @ np.abs(L.cd)), 0.0) + \
        np.where(-dot > 0, abs(L.id) * (glb_mag @ np.abs(L.cd)), 0.0)
    r = np.sqrt((nsum * nsum).sum(-1))
    s = r + NORM_EPS
    gnh = gdot[..., None] * L.dir
    with np.errstate(all='ignore'):
        k = np.where(r > 0, (gnh * nsum).sum(-1) / (s * s * r), 0.0)
        k_mag = np.where(r > 0, gdot_mag * np.abs(L.dir * nsum).sum(-1) / (s * s * r), 0.0)
    g = gnh / s[..., None] - nsum * k[..., None]
    mag = gdot_mag[..., None] * np.abs(L.dir) / s[..., None] + np.abs(nsum) * k_mag[..., None]
    return g, mag


def shade_adjoint64(vertices, faces_idx, colors, L, fill_back, smooth, g):
    """The adjoint of shade64 at g [B,F,3,3] in float64: (grad_colors, its sum of |terms|, grad_vertices, its magnitude).
    grad_colors has the colours' batch (summed over the images for shared colours).  The magnitudes propagate absolute values
    through every sum and difference, so a float32 evaluation of the same chain stays within a small multiple of u times them."""
    v = np.asarray(vertices, np.float64)
    g = np.asarray(g, np.float64)
    B, Nv = v.shape[:2]
    idx = _idx(faces_idx, B)
    colors = np.asarray(colors, np.float64)
    shared = colors.ndim == 2 or colors.shape[0] == 1
    col = _colors(colors, B)
    Nf = idx.shape[1]
    gcol, gcol_mag = np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3))
    gv, gv_mag = np.zeros((B, Nv, 3)), np.zeros((B, Nv, 3))
    for b in range(B):
        ix = idx[b]
        gF = g[b, :Nf]
        gB = g[b, Nf:][:, ::-1] if fill_back else np.zeros_like(gF)  # gB[f, k] belongs to vertex k of face f
        w = v[b][ix]
        v10, v12 = w[:, 0] - w[:, 1], w[:, 2] - w[:, 1]
        n = _cross(v10, v12)
        cf = col[b][ix]
        if smooth:
            m = np.zeros((Nv, 3))
            sF, sB, sFm, sBm = (np.zeros((Nv, 3)) for _ in range(4))
            for k in range(3):
                np.add.at(m, ix[:, k], n)
                np.add.at(sF, ix[:, k], gF[:, k])
                np.add.at(sB, ix[:, k], gB[:, k])
                np.add.at(sFm, ix[:, k], np.abs(gF[:, k]))
                np.add.at(sBm, ix[:, k], np.abs(gB[:, k]))
            lf, lb, dot = _light(m, L, np.float64)
            gcol[b] = sF * lf + sB * lb
            gcol_mag[b] = sFm * np.abs(lf) + sBm * np.abs(lb)
            gm, gm_mag = _light_bwd(m, dot, col[b] * sF, col[b] * sB, np.abs(col[b]) * sFm, np.abs(col[b]) * sBm, L)
            gn, gn_mag = gm[ix].sum(1), gm_mag[ix].sum(1)
        else:
            lf, lb, dot = _light(n, L, np.float64)
            for k in range(3):
                np.add.at(gcol[b], ix[:, k], gF[:, k] * lf + gB[:, k] * lb)
                np.add.at(gcol_mag[b], ix[:, k], np.abs(gF[:, k] * lf) + np.abs(gB[:, k] * lb))
            gn, gn_mag = _light_bwd(n, dot, (gF * cf).sum(1), (gB * cf).sum(1), np.abs(gF * cf).sum(1),
                                    np.abs(gB * cf).sum(1), L)
        ga, gb = _cross(v12, gn), _cross(gn, v10)
        ga_mag, gb_mag = _abs_cross(v12, gn_mag), _abs_cross(gn_mag, v10)
        for k, (t, tm) in enumerate(((ga, ga_mag), (-(ga + gb), ga_mag + gb_mag), (gb, gb_mag))):
            np.add.at(gv[b], ix[:, k], t)
            np.add.at(gv_mag[b], ix[:, k], tm)
    if shared:
        gcol, gcol_mag = gcol.sum(0, keepdims=True), gcol_mag.sum(0, keepdims=True)
        if colors.ndim == 2:
            gcol, gcol_mag = gcol[0], gcol_mag[0]
    return gcol, gcol_mag, gv, gv_mag


def icosphere(level):
    """(vertices [Nv,3] float64 on the unit sphere, faces [20 * 4^level, 3] int32, outward for the renderer's convention)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, np.float64), np.asarray(f, np.int32)
