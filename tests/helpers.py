"""Shared test helpers: golden fixtures, teapot scene construction, comparison utilities."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'reference_fixtures.npz')

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def teapot(normalization=True):
    """(vertices [1292,3] f32, faces [2464,3] i32) of the reference's teapot.obj (tests/test_load_obj.py:36)."""
    from oracle import oracle as O
    g = golden()
    v = g['teapot_vertices_raw']
    return (O.normalize_vertices(v) if normalization else v.copy()), g['teapot_faces'].copy()


def to_minibatch(data, batch_size=4, target_num=2):
    """Reference tests/utils.py:7-14: batch of zeros with the payload in slot `target_num`."""
    ret = []
    for d in data:
        d2 = np.repeat(np.expand_dims(np.zeros_like(d), 0), batch_size, axis=0)
        d2[target_num] = d
        ret.append(d2)
    return ret


def bytescale(x):
    """scipy.misc.imsave byte scaling used to write test_rasterize{1,2}.png."""
    x = np.asarray(x, np.float64)
    return np.floor(np.clip((x - x.min()) * 255.0 / (x.max() - x.min()), 0, 255) + 0.5).astype(np.uint8)


def teapot_views(batch, image_size=256, elevation=30.0, distance=2.732, fill_back=True):
    """The headline scene: teapot seen from `batch` azimuths 360*i/batch, elevation 30,
    distance 2.732 (examples/example1.py:26-27), through look_at + perspective(30) + vertices_to_faces.
    Returns faces [B, F, 3, 3] float32 in the rasterizer's input convention and world-space faces."""
    from oracle import oracle as O
    v, f = teapot()
    if fill_back:
        f = np.concatenate((f, f[:, ::-1]), axis=0)
    out = []
    for i in range(batch):
        eye = O.get_points_from_angles(distance, elevation, 360.0 * i / batch)
        vv = O.perspective(O.look_at(v[None], eye), 30.)
        out.append(O.vertices_to_faces(vv, f[None])[0])
    return np.stack(out).astype(np.float32), f


def random_scene(rng, batch, num_faces, spread=0.6, size=0.25, zmin=1.0, zmax=3.0):
    """Random triangle soup in the rasterizer's input convention: x,y in NDC, z = positive depth."""
    c = rng.uniform(-spread, spread, (batch, num_faces, 1, 3)).astype(np.float32)
    d = rng.uniform(-size, size, (batch, num_faces, 3, 3)).astype(np.float32)
    faces = c + d
    faces[..., 2] = rng.uniform(zmin, zmax, (batch, num_faces, 3)).astype(np.float32)
    return np.ascontiguousarray(faces, np.float32)


def rel_err(a, b, floor=None):
    """max |a-b| / max(|b|, floor); floor defaults to 1e-3 * max|b| (sum-order noise is relative to the
    magnitude of the partial sums, not of a result that may have cancelled)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if floor is None:
        floor = 1e-3 * (np.abs(b).max() if b.size else 1.0) + 1e-30
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max()) if b.size else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# Entrywise bounds: every gradient entry against its own term magnitudes (oracle Rasterize.backward(magnitudes=True))
U = 2.0 ** -24   # float32 unit roundoff
UD = 2.0 ** -53  # float64 unit roundoff
# Per-term constants c1 of the two default-mode band kernels (first-order roundings counted in entrywise's docstring,
# plus one for the second-order products)
C1_ROW = 22
C1_FAST = 24
# Longest float partial sum a lane forms before its sum goes to double
M_ROW = 32   # k_bpm_row: a lane's even / odd segment terms, <= 8 at raster 256 and <= 32 at 1024, the largest raster it serves
M_FAST = 49  # k_bpm_fast: <= 3 pieces of 15 pixels in one float sum (a class-U super-piece), then a float tree over <= 16
             # pieces of a run of lanes (depth 4): 45 + 4
MODES = ('exact', 'row', 'fast', 'default', 'global', 'textures')


def gamma(n, u=U):
    """Higham's gamma_n = n u / (1 - n u): |fl(sum of n terms in any order) - sum| <= gamma_{n-1} * sum |terms|."""
    n = np.asarray(n, np.float64)
    return n * u / (1.0 - n * u)


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def entrywise_bound(ref_d, mags, mode, got=None):
    """Per-entry bound on |got - ref_d| for `mode`; see entrywise."""
    ref_d = np.asarray(ref_d, np.float64)
    big = np.abs(ref_d) if got is None else np.maximum(np.abs(ref_d), np.abs(np.asarray(got, np.float64)))
    ulp = _ulp(big)
    if mode == 'textures':
        a, n = mags['At'], mags['Nt']
        return ulp + gamma(n) * a
    a, m, n = mags['A'], mags['M'], mags['N']
    double_sums = 2 * UD * n * a
    if mode in ('exact', 'global'):
        b = ulp + double_sums
    elif mode == 'row':
        b = ulp + double_sums + C1_ROW * U * m + gamma(M_ROW) * a
    elif mode == 'fast':
        b = ulp + double_sums + C1_FAST * U * m + gamma(M_FAST) * a
    elif mode == 'default':
        b = ulp + double_sums + np.maximum(C1_ROW * U * m + gamma(M_ROW) * a, C1_FAST * U * m + gamma(M_FAST) * a)
    else:
        raise ValueError(mode)
    if 'A8' in mags:
        x8 = mags['M8'].copy()
        x8[..., 2] = mags['A8'][..., 2]
        b = b + gamma(mags['N8'] + 1) * (a + x8) + ulp
    return b


def entrywise(got, ref_d, mags, mode):
    """Every gradient entry against a bound built from its OWN terms, not from the largest gradient of the call (rel_err's floor).

    `ref_d` is the oracle's output with its float terms summed in double (Rasterize.backward(accumulate_double=True)), `mags`
    the dict of Rasterize.backward(magnitudes=True) on the same inputs: per grad_faces entry A = sum |term|, M = sum of the
    magnitudes entering each term before its colour difference cancels (nr_oracle.c, K6), N = number of terms; A8 / M8 / N8
    the same for K8's terms; At / Nt per grad_textures element (K7).  Returns (worst |got - ref_d| / bound, indices of the
    entries above their bound).  Entries where got, ref_d or the bound is not finite are skipped (the NaN pattern is
    asserted where the tests compare gradients).  u = 2^-24, u_d = 2^-53, gamma_n = n u / (1 - n u).

    grad_faces, by `mode` (K6's kernels: neural_renderer_amd/csrc/nr_k6_global.h, nr_k6_fast.h, nr_k6_row.h, parts of the
    translation unit nr_backward_pixel_map.hip; `file [anchor]` names a comment `// [anchor]` in that file):
      'exact' -- NR_FLAG_EXACT_GRADIENT on either band kernel (include/nr_hip.h:79-93: the reference's operations one by one,
          every sum in double): the terms are the oracle's bits, so only the two double sums differ, each by <= N u_d A
          (any order), and each side rounds its double to float once:  ulp(ref_d) + 2 u_d N A.
      'global' -- k_bpm_global (NR_FLAG_K6_GLOBAL, rasters whose band does not fit in LDS): the reference's terms
          (nr_k6_global.h [global-terms]) in per-lane double sums, stored without atomics: the exact mode's bound.
      'row' -- k_bpm_row, default mode.  Per term, against the oracle's float term (first order, S = sum_c (|I_c| + |ref_c| +
          2 kappa) |g_c| of the pixel, so that M = sum S / |dist|):
            diff: P formed in double and rounded once (u S), ref_c - K_c rounded (u S), four fused multiply-adds
                (nr_k6_row.h [row-visit], 4 u S) -> 6 u S; the oracle's sum_c (I_c - ref_c) g_c (nr_oracle.c, K6): a subtraction, a
                product and an add per channel (the first add onto 0 exact) -> 5 u S;
            dist: t = fma(sdir, d1, -sdir cross) is the reference's subtraction (same bits); |c| 2/S (2 u: the product
                and 2/S when S is no power of two), fma(|c| 2/S, |t|, eps) (u), eps in float (u) -> 4 u; the oracle's c t,
                x 2/S, +- eps -> 3 u;
            reciprocal: v_rcp_f32 <= 1 ulp = 2 u ([row-rcp]; phase A's recip_n with a Newton step, [row-recip-n], less); the
                oracle's division u.
          |term - term_ref| <= (6 + 5) u S / |dist| + (4 + 3 + 2 + 1) u |term| <= 21 u S / |dist|: C1_ROW = 22 with the
          second-order products.  A visit that one side skips (diff <= 0) and the other keeps has |diff| within those
          roundings of 0 and is covered the same way: M counts skipped visits too.  Sums: fma(dm, rcp, a) into a lane's
          float partial sums of <= M_ROW terms (gamma_M_ROW A), the rest in double (u_d N A per side), one rounding to float:
            ulp(ref_d) + 2 u_d N A + C1_ROW u M + gamma_M_ROW A.
      'fast' -- k_bpm_fast, default mode (NR_FLAG_K6_LEGACY, the scan path NR_FLAG_K6_SCAN, overflow images, rasters above
          k_bpm_row's): the colour difference from b - ref or c - ref, one product and three fused multiply-adds
          (nr_k6_fast.h [fast-diff], 5 u S; the oracle 5 u S); t = (d1 - cross) + k, two roundings of one sign ([fast-t]: 2 u against the
          reference's one, 3 u apart), c 2/S (2 u), fma (u), eps (u); the oracle 3 u; v_rcp_f32 without a Newton step
          ([fast-rcp]: 2 u), the oracle's division (u): (5 + 5) u S / |dist| + (3 + 4 + 3 + 2 + 1) u |term|
          <= 23 u S / |dist|: C1_FAST = 24.  (The general loop of class G forms t = d1 - cross in one
          rounding and c t + eps in two, a product and an addition: the same count.)  Float sums of <= M_FAST terms ([fast-rcp]
          and the run sums), double above:
            ulp(ref_d) + 2 u_d N A + C1_FAST u M + gamma_M_FAST A.
      'default' -- the default mode where either band kernel may serve an image (k_bpm_row hands overflow images to
          k_bpm_fast): the larger of the two.
    With K8 (depth; `mags` has A8): its terms are the reference's expressions (nr_backward_gather.hip and nr_face_gather.h [k8-terms] against
    nr_oracle.c K8), added in float in any order together with K6's rounded total (atomics, nr_face_gather.h [k8-atomics]), so the bound grows
    by gamma_{N8+1} (A + X8) + ulp, X8 = M8 for x, y (tmp_l cancels) and A8 for z.
    'textures' (grad_textures, K7): one product per term, the reference's (rasterize.py:780), float partial sums and
    atomics in any order:  ulp(ref) + gamma_Nt At.
    """
    got = np.asarray(got, np.float64)
    ref_d = np.asarray(ref_d, np.float64)
    bound = entrywise_bound(ref_d, mags, mode, got)
    ok = np.isfinite(got) & np.isfinite(ref_d) & np.isfinite(bound)
    ratio = np.zeros(got.shape, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio[ok] = np.abs(got[ok] - ref_d[ok]) / bound[ok]
    ratio[ok & (bound == 0) & (got != ref_d)] = np.inf
    ratio[ok & (bound == 0) & (got == ref_d)] = 0.0
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst, np.argwhere(ratio > 1)


def above_1e4(got, ref_d):
    """Number of entries more than 1e-4 off elementwise (relative to the entry itself; exact zeros of ref_d excluded)."""
    got = np.asarray(got, np.float64)
    ref_d = np.asarray(ref_d, np.float64)
    ok = np.isfinite(got) & np.isfinite(ref_d) & (ref_d != 0)
    return int((np.abs(got[ok] - ref_d[ok]) > 1e-4 * np.abs(ref_d[ok])).sum())


def grad_faces_bounds(ref_float, ref_d):
    """(noise, bound of the default mode, bound of the exact mode) for grad_faces in the parity metric (rel_err): the north
    star's 1e-4 (the exact mode with a depth gradient: 2e-5) of the reference's terms summed exactly (`ref_d`:
    accumulate_double=True), plus twice the reference's own float-summation noise on the scene -- `ref_float`, its serial float
    sums, against the same exact sum (test_fuzz_gpu.py::test_fuzz_unusual_parameters has the reasoning)."""
    okn = np.isfinite(ref_d) & np.isfinite(ref_float)
    noise = rel_err(ref_float[okn], ref_d[okn]) if okn.any() else 0.0
    return noise, 1e-4 + 2 * noise, 2e-5 + 2 * noise


def err_default(got, ref_d, ref_k6, ok):
    """The default mode's grad_faces error over the entries `ok`: against the larger of the total (`ref_d`) and its K6 part
    (`ref_k6`: the same call with a zero depth gradient), element by element, floor at 1e-3 of the larger maximum -- K6's
    sums and K8's can cancel (test_fuzz_gpu.py::test_fuzz_unusual_parameters)."""
    okk = ok & np.isfinite(ref_k6)
    if not okk.any():
        return 0.0
    mag = np.maximum(np.abs(ref_d[okk]), np.abs(ref_k6[okk]))
    den = np.maximum(mag, 1e-3 * mag.max())
    return float((np.abs(got[okk] - ref_d[okk]) / np.where(den > 0, den, 1.0)).max())


_display = None


def display_model():
    """tests/golden/display_model.npz: the textured ShapeNet model of the reference's tests/test_load_obj.py:51-59."""
    global _display
    if _display is None:
        _display = dict(np.load(os.path.join(os.path.dirname(GOLDEN), 'display_model.npz')))
    return _display


def write_display_model(dirpath):
    """Re-create model.obj / model.mtl / images/*.png from the fixture arrays (lossless: %.9g floats, PNG textures whose
    pixels are the JPEGs as decoded when the fixture was made).  Returns the .obj path."""
    from PIL import Image
    g = display_model()
    os.makedirs(os.path.join(dirpath, 'images'), exist_ok=True)
    with open(os.path.join(dirpath, 'model.mtl'), 'w') as f:
        for name, kd, tex in zip(g['materials'], g['kd'], g['map_kd']):
            f.write('newmtl %s\nKa 0.000000 0.000000 0.000000\nKd %.6f %.6f %.6f\n' % ((name,) + tuple(kd)))
            if tex:
                png = os.path.splitext(os.path.basename(str(tex)))[0] + '.png'
                Image.fromarray(g['image_' + os.path.basename(str(tex))]).save(os.path.join(dirpath, 'images', png))
                f.write('map_Kd ./images/%s\n' % png)
            f.write('\n')
    path = os.path.join(dirpath, 'model.obj')
    with open(path, 'w') as f:
        f.write('mtllib model.mtl\n')
        f.writelines('v %.9g %.9g %.9g\n' % tuple(v) for v in g['v'])
        f.writelines('vt %.9g %.9g\n' % tuple(t) for t in g['vt'])
        cur = -1
        for fv, ft, m in zip(g['faces_v'], g['faces_vt'], g['face_material']):
            if m != cur:
                cur = m
                f.write('usemtl %s\n' % g['materials'][m])
            if ft[0] < 0:
                f.write('f %d %d %d\n' % tuple(fv + 1))
            else:
                f.write('f %d/%d %d/%d %d/%d\n' % (fv[0] + 1, ft[0] + 1, fv[1] + 1, ft[1] + 1, fv[2] + 1, ft[2] + 1))
    return path
