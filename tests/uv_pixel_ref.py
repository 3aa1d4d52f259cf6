"""Test-side restatement of per-pixel UV images (include/nr_hip.h: nr_forward_rasterize_uv / nr_backward_uv_images) in
NumPy: the shading of covered pixels in float32 in the kernels' operation order, from the maps a forward returned, and the
adjoint in float64.  The bilinear lookup is uv_ref's (the bake's), evaluated at a pixel's barycentric point."""
import numpy as np

import uv_ref as U

f32 = np.float32


def reads(uv_tri, d, H, W):
    """The four bilinear reads at barycentric points d [N,3] (float32) of uv triangles uv_tri [N,3,2]: file-orientation
    pixel indices [N,4] and weights [N,4], in the kernels' order (uv_ref.texel_reads at arbitrary points)."""
    u = uv_tri[:, :, 0].astype(f32)
    v = uv_tri[:, :, 1].astype(f32)
    d = d.astype(f32)
    with np.errstate(all='ignore'):
        pos_x = ((u[:, 0] * d[:, 0] + u[:, 1] * d[:, 1]) + u[:, 2] * d[:, 2]) * f32(W - 1)
        pos_y = ((v[:, 0] * d[:, 0] + v[:, 1] * d[:, 1]) + v[:, 2] * d[:, 2]) * f32(H - 1)
        xi, yi, yi1 = U._f2i(pos_x), U._f2i(pos_y), U._f2i(pos_y + f32(1))
        wx1 = pos_x - xi.astype(f32)
        wx0 = f32(1) - wx1
        wy1 = pos_y - yi.astype(f32)
        wy0 = f32(1) - wy1
    last = H * W - 1

    def flat(row, col):
        p = np.clip(row * W + col, 0, last)
        r = p // W
        return (H - 1 - r) * W + (p - r * W)
    idx = np.stack((flat(yi, xi), flat(yi1, xi), flat(yi, xi + 1), flat(yi1, xi + 1)), axis=1)
    w = np.stack((wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1), axis=1).astype(f32)
    return idx, w


def cube_taps(w, zp, z, ts, eps, flip):
    """compute_taps (csrc/nr_device.h) per pixel: flat texel indices [N,8] (>= ts^3: weight 0, skipped) and weights."""
    tif = (w * f32(ts - 1)) * (zp[:, None] / z)
    tif = np.fmax(tif, f32(0))
    tif = np.fmin(tif.astype(np.float64), float(ts - 1) - eps).astype(f32)
    ti = U._f2i(tif)
    frac = tif - ti.astype(f32)
    isc = np.zeros((len(w), 8), np.int64)
    wt = np.zeros((len(w), 8), f32)
    for pn in range(8):
        ww = np.ones(len(w), f32)
        idx = []
        for k in range(3):
            if (pn >> k) & 1 == 0:
                ww = ww * (f32(1) - frac[:, k])
                idx.append(ti[:, k])
            else:
                ww = ww * frac[:, k]
                idx.append(ti[:, k] + 1)
        i0 = np.where(flip, idx[2], idx[0])
        i2 = np.where(flip, idx[0], idx[2])
        isc[:, pn] = (i0 * ts + idx[1]) * ts + i2
        wt[:, pn] = ww
    return isc, wt


def samples(faces, fi, wmap, dmap, layout, images, eps):
    """Per covered pixel (np.nonzero(fi >= 0) order): (b, f, c [N,3] float32 before the light factor, reads) with reads =
    list of (m, sel, bi, idx, w) of the pixels whose face has image m.  images: list of [Bi,H,W,3] float32 (Bi = 1: shared)."""
    Nf = layout.num_faces
    b, y, x = np.nonzero(fi >= 0)
    f = fi[b, y, x].astype(np.int64)
    flip = f >= Nf
    f0 = np.where(flip, f - Nf, f)
    w = wmap[b, y, x].astype(f32)
    zp = dmap[b, y, x].astype(f32)
    z = faces[b, f, :, 2].astype(f32)
    with np.errstate(all='ignore'):
        d = np.fmin(np.fmax(w * (zp[:, None] / z), f32(0)), f32(1))
    d[flip] = d[flip][:, ::-1]
    m_of = layout.face_image[f0]
    c = np.zeros((len(f), 3), f32)
    out = []
    for m, (H, W) in enumerate(layout.image_sizes):
        sel = np.nonzero(m_of == m)[0]
        if len(sel) == 0:
            continue
        idx, wt = reads(layout.faces_uv[f0[sel]], d[sel], H, W)
        img = np.asarray(images[m], f32)
        bi = b[sel] if img.shape[0] > 1 else np.zeros(len(sel), np.int64)
        flat = img.reshape(img.shape[0], -1, 3)
        acc = np.zeros((len(sel), 3), f32)
        for r in range(4):
            acc = acc + flat[bi, idx[:, r]] * wt[:, r, None]
        c[sel] = acc
        out.append((m, sel, bi, idx, wt))
    sel = np.nonzero((m_of < 0) | (m_of >= layout.num_images))[0]
    if len(sel):
        ts = layout.texture_size
        with np.errstate(all='ignore'):
            isc, wt = cube_taps(w[sel], zp[sel], z[sel], ts, eps, flip[sel])
        base = layout.base.reshape(Nf, -1, 3)
        acc = np.zeros((len(sel), 3), f32)
        for pn in range(8):
            ok = isc[:, pn] < ts ** 3
            tx = base[f0[sel], np.where(ok, isc[:, pn], 0)]
            acc = np.where(ok[:, None], acc + wt[:, pn, None] * tx, acc)
        c[sel] = acc
    return b, y, x, f, c, out


def render(faces, fi, wmap, dmap, light, layout, images, eps, background):
    """rgb_map [B,S,S,3] float32 as nr_forward_rasterize_uv computes it from the same maps."""
    B, S = fi.shape[:2]
    bg = np.broadcast_to(np.asarray(background, f32), (B, 3))
    rgb = np.broadcast_to(f32(0) * f32(0) + f32(1) * bg[:, None, None, :], (B, S, S, 3)).copy()
    b, y, x, f, c, _ = samples(faces, fi, wmap, dmap, layout, images, eps)
    rgb[b, y, x] = (c * light[b, f]) * f32(1) + f32(0) * bg[b]
    return rgb


def adjoint(faces, fi, wmap, dmap, light, layout, images, eps, grad_rgb):
    """float64 (grad_images list of [Bi,H,W,3], grad_light [B,F,3]) and the sums of |terms| of each entry."""
    B, F = light.shape[:2]
    b, y, x, f, c, out = samples(faces, fi, wmap, dmap, layout, images, eps)
    g = grad_rgb[b, y, x].astype(np.float64)
    gl, gl_mag = np.zeros((B, F, 3)), np.zeros((B, F, 3))
    t = g * c.astype(np.float64)
    np.add.at(gl, (b, f), t)
    np.add.at(gl_mag, (b, f), np.abs(t))
    gi = [np.zeros((np.asarray(im).shape[0], h * w, 3)) for im, (h, w) in zip(images, layout.image_sizes)]
    gi_mag = [np.zeros_like(a) for a in gi]
    for m, sel, bi, idx, wt in out:
        gk = g[sel] * light[b[sel], f[sel]].astype(np.float64)
        for r in range(4):
            t = gk * wt[:, r, None].astype(np.float64)
            np.add.at(gi[m], (bi, idx[:, r]), t)
            np.add.at(gi_mag[m], (bi, idx[:, r]), np.abs(t))
    shapes = [(a.shape[0], h, w, 3) for a, (h, w) in zip(gi, layout.image_sizes)]
    return ([a.reshape(s) for a, s in zip(gi, shapes)], [a.reshape(s) for a, s in zip(gi_mag, shapes)], gl, gl_mag)
