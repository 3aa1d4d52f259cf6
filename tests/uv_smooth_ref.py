"""Test-side restatement of smooth light on per-pixel UV images (include/nr_hip.h: nr_forward_rasterize_uv_smooth /
nr_backward_uv_images_smooth) in NumPy, from the maps a forward returned: the sample c and its reads are uv_pixel_ref.samples',
the corner weights e_k are vertex_ref._weights'.  The render is float32 in the header's operation order; the adjoint is
float64 with the sum of |terms| of every entry; render64 is the same function of (light, images) in float64 for finite
differences."""
import numpy as np

import uv_pixel_ref as P
import vertex_ref as V

f32 = np.float32


def scene(seed):
    """A fuzz scene as tests/test_uv_pixel_gpu.py builds them (the same generators, seeds of its own): random triangles, a
    random layout (1x1 images, degenerate uv triangles, faces without an image), fill_back on or off, shared or per-view
    images, B = 1..3, odd and non-power-of-two rasters -- and a light colour per corner, uniform in [0.2, 1.2]."""
    import helpers as H
    import uv_ref as U
    rng = np.random.default_rng(7300 + seed)
    B = int(rng.integers(1, 4))
    Nf = int(rng.integers(20, 120))
    fill_back = bool(seed % 2)
    S = int(rng.choice([37, 50, 64, 96]))
    sizes = [(1, 1) if rng.uniform() < 0.3 else (int(rng.integers(1, 40)), int(rng.integers(1, 60)))
             for _ in range(int(rng.integers(1, 4)))]
    ts = int(rng.choice([2, 3, 4]))
    uv, face_image, base = U.random_layout(rng, Nf, ts, sizes)
    faces = H.random_scene(rng, B, Nf, size=0.4)
    if fill_back:
        faces = np.ascontiguousarray(np.concatenate((faces, faces[:, :, ::-1]), axis=1))
    F = faces.shape[1]
    light = rng.uniform(0.2, 1.2, (B, F, 3, 3)).astype(np.float32)
    Bi = 1 if (seed // 2) % 2 == 0 else B
    images = [rng.uniform(0, 1, (Bi, h, w, 3)).astype(np.float32) for h, w in sizes]
    return dict(rng=rng, B=B, S=S, sizes=sizes, ts=ts, uv=uv, face_image=face_image, base=base, faces=faces, light=light,
                images=images, shared=Bi == 1 and B > 1)


def magnified_scene():
    """One-pixel images heavily magnified: a 1x1 and a 2x2 image on 40 large faces, two views of 128 x 128 -- thousands of
    pixels feed one image pixel and the nine light sums of one face."""
    import helpers as H
    import uv_ref as U
    rng = np.random.default_rng(7391)
    Nf = 40
    uv, _, base = U.random_layout(rng, Nf, 2, [(1, 1), (2, 2)])
    return dict(rng=rng, B=2, S=128, sizes=[(1, 1), (2, 2)], ts=2, uv=uv, face_image=(np.arange(Nf) % 2).astype(np.int32),
                base=base, faces=H.random_scene(rng, 2, Nf, spread=0.3, size=0.9), shared=True,
                light=rng.uniform(0.2, 1.2, (2, Nf, 3, 3)).astype(np.float32),
                images=[rng.uniform(0, 1, (1, 1, 1, 3)).astype(np.float32), rng.uniform(0, 1, (1, 2, 2, 3)).astype(np.float32)])


def np_images(sc):
    return [im[:1] if sc['shared'] else im for im in sc['images']]


def _pixels(faces, fi, wm, dm, layout, images, eps):
    """Per covered pixel, in np.nonzero(fi >= 0) order: (b, y, x, f, c float32 [N,3], e float32 [N,3], reads)."""
    b, y, x, f, c, reads = P.samples(faces, fi, wm, dm, layout, images, eps)
    (b2, y2, x2), f2, e = V._weights(faces, fi, wm, dm)
    assert np.array_equal(b, b2) and np.array_equal(y, y2) and np.array_equal(x, x2) and np.array_equal(f, f2)
    return b, y, x, f, c, e, reads


def pixel_light(light, b, f, e):
    """L [N,3] float32: (light[b,f,0] * e_0 + light[b,f,1] * e_1) + light[b,f,2] * e_2."""
    l = light[b, f].astype(f32)
    with np.errstate(all='ignore'):
        return (l[:, 0] * e[:, 0:1] + l[:, 1] * e[:, 1:2]) + l[:, 2] * e[:, 2:3]


def render(faces, fi, wm, dm, light, layout, images, eps, background):
    """rgb_map [B,S,S,3] float32 as nr_forward_rasterize_uv_smooth computes it from the same maps; light [B,F,3,3]."""
    B, S = fi.shape[:2]
    bg = np.broadcast_to(np.asarray(background, f32), (B, 3))
    rgb = np.broadcast_to(f32(0) * f32(0) + f32(1) * bg[:, None, None, :], (B, S, S, 3)).copy()
    b, y, x, f, c, e, _ = _pixels(faces, fi, wm, dm, layout, images, eps)
    with np.errstate(all='ignore'):
        rgb[b, y, x] = (c * pixel_light(light, b, f, e)) * f32(1) + f32(0) * bg[b]
    return rgb


def adjoint(faces, fi, wm, dm, light, layout, images, eps, grad_rgb):
    """float64 (grad_images list of [Bi,H,W,3], their sums of |terms|, grad_light [B,F,3,3], its sums of |terms|): the
    forward's float32 c, e_k and L, products and sums in double."""
    B, F = light.shape[:2]
    b, y, x, f, c, e, reads = _pixels(faces, fi, wm, dm, layout, images, eps)
    g = grad_rgb[b, y, x].astype(np.float64)
    t = (g * c.astype(np.float64))[:, None, :] * e.astype(np.float64)[:, :, None]  # [N,k,c]
    gl, gl_mag = np.zeros((B, F, 3, 3)), np.zeros((B, F, 3, 3))
    np.add.at(gl, (b, f), t)
    np.add.at(gl_mag, (b, f), np.abs(t))
    L = pixel_light(light, b, f, e).astype(np.float64)
    gi = [np.zeros((np.asarray(im).shape[0], h * w, 3)) for im, (h, w) in zip(images, layout.image_sizes)]
    gi_mag = [np.zeros_like(a) for a in gi]
    for m, sel, bi, idx, wt in reads:
        gk = g[sel] * L[sel]
        for r in range(4):
            t = gk * wt[:, r, None].astype(np.float64)
            np.add.at(gi[m], (bi, idx[:, r]), t)
            np.add.at(gi_mag[m], (bi, idx[:, r]), np.abs(t))
    shapes = [(a.shape[0], h, w, 3) for a, (h, w) in zip(gi, layout.image_sizes)]
    return ([a.reshape(s) for a, s in zip(gi, shapes)], [a.reshape(s) for a, s in zip(gi_mag, shapes)], gl, gl_mag)


def render64(faces, fi, wm, dm, light, layout, images, eps):
    """The covered pixels' colours [N,3] in float64 as a function of float64 `light` and `images`: the same reads, read
    weights and corner weights (the float32 values, exact in double), every product and sum in double.  Faces without an
    image keep their (constant) float32 base sample."""
    b, y, x, f, c, e, reads = _pixels(faces, fi, wm, dm, layout, [np.asarray(im, f32) for im in images], eps)
    c64 = c.astype(np.float64)
    for m, sel, bi, idx, wt in reads:
        flat = np.asarray(images[m], np.float64).reshape(np.asarray(images[m]).shape[0], -1, 3)
        acc = np.zeros((len(sel), 3))
        for r in range(4):
            acc = acc + flat[bi, idx[:, r]] * wt[:, r, None].astype(np.float64)
        c64[sel] = acc
    l = np.asarray(light, np.float64)[b, f]
    e = e.astype(np.float64)
    return (b, y, x), c64 * ((l[:, 0] * e[:, 0:1] + l[:, 1] * e[:, 1:2]) + l[:, 2] * e[:, 2:3])


# ---------------------------------------------------------------------------------------------------------------------
# meshes with lat/long uv coordinates for the renderer-level tests

def latlong_uv(vertices, faces_idx):
    """faces_uv [Nf,3,2] float32 of a mesh around the origin: u from the longitude, v from the latitude; a face that
    crosses the seam gets its small longitudes moved up by one turn and is then shifted back into [0, 1] as a whole (clipped:
    only its position in the image changes)."""
    v = np.asarray(vertices, np.float64)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    u = np.arctan2(n[:, 2], n[:, 0]) / (2 * np.pi) + 0.5
    t = np.arcsin(np.clip(n[:, 1], -1, 1)) / np.pi + 0.5
    fu, ft = u[faces_idx], t[faces_idx]
    seam = (fu.max(1) - fu.min(1)) > 0.5
    fu = np.where(seam[:, None] & (fu < 0.5), fu + 1, fu)
    fu = np.clip(fu - np.where(fu.max(1) > 1, fu.max(1) - 1, 0)[:, None], 0, 1)
    return np.stack((fu, ft), axis=2).astype(f32)


def latlong_sphere(n_lat=16, n_lon=32):
    """A unit UV sphere: (vertices [Nv,3] float32, faces [Nf,3] int32, faces_uv [Nf,3,2] float32), a vertex row per latitude
    and a duplicated seam column, so that no face crosses the seam."""
    v, uv = [], []
    for i in range(n_lat + 1):
        th = np.pi * i / n_lat
        for j in range(n_lon + 1):
            ph = 2 * np.pi * j / n_lon
            v.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
            uv.append((j / n_lon, 1 - i / n_lat))
    f = []
    for i in range(n_lat):
        for j in range(n_lon):
            a = i * (n_lon + 1) + j
            b, c, d = a + 1, a + n_lon + 1, a + n_lon + 2
            f += [(a, b, c), (b, d, c)]  # (wound as vertex_ref.icosphere: outward for the renderer)
    v, uv, f = np.asarray(v, f32), np.asarray(uv, f32), np.asarray(f, np.int32)
    return v, f, uv[f]


def checkerboard(h=64, w=128, cell=8):
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    board = (((rows // cell) + (cols // cell)) % 2).astype(f32)
    return np.stack((f32(0.1) + f32(0.8) * board, f32(0.2) + f32(0.6) * (1 - board), np.full_like(board, 0.5)), axis=2)


def image_layout(faces_uv, size, texture_size=2):
    """A UVLayout whose faces all sample one image of `size` = (H, W)."""
    import neural_renderer_amd as nr
    Nf = len(faces_uv)
    ts = texture_size
    return nr.UVLayout(faces_uv, np.zeros(Nf, np.int32), np.full((Nf, ts, ts, ts, 3), 0.5, f32), [tuple(size)])
