"""Test-side restatement of the learnable UV bake (include/nr_hip.h nr_bake_uv_textures) in NumPy: the forward in float32
in the kernel's operation order, the reads it takes, and its adjoint in float64."""
import numpy as np


def _f2i(x):
    """(int)x on the device: truncate, saturate, NaN -> 0."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0.0, np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64)


def texel_points(ts):
    """[ts^3, 3] float32 barycentric points of the texels (load_obj.py:98-106); texel (0,0,0) is the centroid (1/3 each)."""
    idx = np.arange(ts, dtype=np.int64)
    grid = (idx.astype(np.float64) / (ts - 1.)).astype(np.float32)
    d0, d1, d2 = [a.reshape(-1) for a in np.meshgrid(grid, grid, grid, indexing='ij')]
    with np.errstate(all='ignore'):
        total = (d0 + d1) + d2
        d = np.stack((d0 / total, d1 / total, d2 / total), axis=1)
    d[0] = np.float32(1) / np.float32(3)
    return d


def texel_reads(faces_uv, ts, H, W):
    """For every face and texel: file-orientation pixel indices [F,T,4] (int64) and weights [F,T,4] (float32) of the four
    bilinear reads, in the kernel's order (yi,xi), (yi1,xi), (yi,xi+1), (yi1,xi+1) of the bottom-row-first image."""
    d = texel_points(ts)
    u = faces_uv[:, None, :, 0].astype(np.float32)
    v = faces_uv[:, None, :, 1].astype(np.float32)
    with np.errstate(all='ignore'):
        pos_x = ((u[..., 0] * d[None, :, 0] + u[..., 1] * d[None, :, 1]) + u[..., 2] * d[None, :, 2]) * np.float32(W - 1)
        pos_y = ((v[..., 0] * d[None, :, 0] + v[..., 1] * d[None, :, 1]) + v[..., 2] * d[None, :, 2]) * np.float32(H - 1)
        xi, yi, yi1 = _f2i(pos_x), _f2i(pos_y), _f2i(pos_y + np.float32(1))
        wx1 = pos_x - xi.astype(np.float32)
        wx0 = np.float32(1) - wx1
        wy1 = pos_y - yi.astype(np.float32)
        wy0 = np.float32(1) - wy1
    last = H * W - 1

    def flat(row, col):
        p = np.clip(row * W + col, 0, last)
        r = p // W
        return (H - 1 - r) * W + (p - r * W)          # mirrored: the image is given top row first
    idx = np.stack((flat(yi, xi), flat(yi1, xi), flat(yi, xi + 1), flat(yi1, xi + 1)), axis=2)
    w = np.stack((wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1), axis=2).astype(np.float32)
    return idx, w


def bake(images, faces_uv, face_image, base, ts):
    """textures [F,ts,ts,ts,3] float32 from images (list of [H,W,3], top row first), exactly as k_bake_uv computes them."""
    F = faces_uv.shape[0]
    out = np.array(base, np.float32).reshape(F, -1, 3).copy()
    for m, image in enumerate(images):
        sel = np.nonzero(face_image == m)[0]
        if len(sel) == 0:
            continue
        H, W = image.shape[:2]
        idx, w = texel_reads(faces_uv[sel], ts, H, W)
        img = np.ascontiguousarray(image, np.float32).reshape(-1, 3)
        c = np.zeros(idx.shape[:2] + (3,), np.float32)
        for r in range(4):
            c = c + img[idx[..., r]] * w[..., r, None]
        out[sel] = c
    return out.reshape(F, ts, ts, ts, 3)


def bake_adjoint(grad_textures, faces_uv, face_image, image_sizes, ts):
    """float64 image gradients (list of [H,W,3]) and the sums of |terms| per pixel, from grad_textures [F,ts,ts,ts,3]."""
    F = faces_uv.shape[0]
    g = np.asarray(grad_textures, np.float64).reshape(F, -1, 3)
    grads, mags = [], []
    for m, (H, W) in enumerate(image_sizes):
        acc = np.zeros((H * W, 3))
        mag = np.zeros((H * W, 3))
        sel = np.nonzero(face_image == m)[0]
        if len(sel):
            idx, w = texel_reads(faces_uv[sel], ts, H, W)
            for r in range(4):
                t = g[sel] * w[..., r, None].astype(np.float64)
                np.add.at(acc, idx[..., r].reshape(-1), t.reshape(-1, 3))
                np.add.at(mag, idx[..., r].reshape(-1), np.abs(t).reshape(-1, 3))
        grads.append(acc.reshape(H, W, 3))
        mags.append(mag.reshape(H, W, 3))
    return grads, mags


def bake_f64(images, faces_uv, face_image, ts):
    """The forward as a linear map in float64 (weights from the float32 reads), zero on faces without an image."""
    F = faces_uv.shape[0]
    out = np.zeros((F, ts ** 3, 3))
    for m, image in enumerate(images):
        sel = np.nonzero(face_image == m)[0]
        if len(sel) == 0:
            continue
        H, W = image.shape[:2]
        idx, w = texel_reads(faces_uv[sel], ts, H, W)
        img = np.asarray(image, np.float64).reshape(-1, 3)
        out[sel] = sum(img[idx[..., r]] * w[..., r, None].astype(np.float64) for r in range(4))
    return out.reshape(F, ts, ts, ts, 3)


def random_layout(rng, num_faces, ts, sizes):
    """faces_uv with values outside [0,1], exactly 0 and 1 and degenerate triangles; face_image with some -1; base."""
    uv = rng.uniform(-0.3, 1.3, (num_faces, 3, 2)).astype(np.float32)
    pick = rng.uniform(size=uv.shape)
    uv[pick < 0.1] = 1.0
    uv[(pick >= 0.1) & (pick < 0.15)] = 0.0
    deg = rng.uniform(size=num_faces) < 0.1
    uv[deg, 1] = uv[deg, 0]
    uv[deg, 2] = uv[deg, 0]
    wrap = 1 < uv
    uv[wrap] = uv[wrap] % 1                        # as the loader does
    face_image = rng.integers(-1, len(sizes), num_faces).astype(np.int32)
    base = np.broadcast_to(rng.uniform(0, 1, (num_faces, 1, 1, 1, 3)).astype(np.float32),
                           (num_faces, ts, ts, ts, 3)).copy()
    return uv, face_image, base
