"""Float64 NumPy restatement of the projection camera (neural_renderer_amd/projection.py, include/nr_hip.h): the yardstick
of tests/test_projection*.py."""
import numpy as np


def _batched(p, B, shape):
    p = np.asarray(p, np.float64)
    if p.shape == shape:
        p = np.broadcast_to(p, (B,) + shape)
    assert p.shape == (B,) + shape, p.shape
    return p


def projection(vertices, K, R, t, dist_coeffs=None, orig_size=None):
    """vertices [B, Nv, 3] -> [B, Nv, 3] (NDC x, NDC y with y up, camera depth), all in float64."""
    w = np.asarray(vertices, np.float64)
    B = w.shape[0]
    K = _batched(K, B, (3, 3))
    R = _batched(R, B, (3, 3))
    t = np.asarray(t, np.float64)
    if t.ndim == 3:
        t = t[:, 0]
    t = _batched(t, B, (3,))
    c = np.einsum('bij,bnj->bni', R, w) + t[:, None, :]
    x = c[..., 0] / c[..., 2]
    y = c[..., 1] / c[..., 2]
    if dist_coeffs is not None:
        k1, k2, p1, p2, k3 = [a[:, None] for a in _batched(dist_coeffs, B, (5,)).T]
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        x, y = (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x),
                y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
    u = K[:, 0, 0, None] * x + K[:, 0, 1, None] * y + K[:, 0, 2, None]
    v = K[:, 1, 0, None] * x + K[:, 1, 1, None] * y + K[:, 1, 2, None]
    S = float(orig_size)
    return np.stack(((2 * u - S) / S, (S - 2 * v) / S, c[..., 2]), axis=2)


def rotation(axis_angle):
    """Rodrigues: axis-angle [3] -> rotation matrix [3, 3] (float64)."""
    a = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def camera(B, seed, per_image=True, distortion=True, orig_size=256.0):
    """A random but sensible camera for the unit-size teapot: K, R, t (float32), dist_coeffs or None.  The mesh sits
    at depth ~2.7 in front of it; the distortion stays within a few percent at the image corners."""
    rng = np.random.default_rng(seed)
    n = B if per_image else 1
    K = np.zeros((n, 3, 3), np.float32)
    K[:, 0, 0] = orig_size * rng.uniform(0.8, 1.0, n)
    K[:, 1, 1] = K[:, 0, 0] * rng.uniform(0.95, 1.05, n)
    K[:, 0, 1] = rng.uniform(-2, 2, n)
    K[:, 0, 2] = orig_size / 2 + rng.uniform(-8, 8, n)
    K[:, 1, 2] = orig_size / 2 + rng.uniform(-8, 8, n)
    K[:, 2, 2] = 1
    R = np.stack([rotation(rng.normal(scale=0.6, size=3)) for _ in range(n)]).astype(np.float32)
    t = np.concatenate([rng.uniform(-0.2, 0.2, (n, 2)), rng.uniform(2.5, 3.0, (n, 1))], axis=1).astype(np.float32)
    d = np.concatenate([rng.uniform(-0.1, 0.1, (n, 2)), rng.uniform(-0.01, 0.01, (n, 2)), rng.uniform(-0.05, 0.05, (n, 1))],
                       axis=1).astype(np.float32) if distortion else None
    if not per_image:
        K, R, t = K[0], R[0], t[0]
        d = d[0] if d is not None else None
    return K, R, t, d
