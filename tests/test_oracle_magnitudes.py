"""The oracle's term magnitudes (Rasterize.backward(magnitudes=True), nr_oracle.c K6 / K7 / K8) and the entrywise check built
on them (helpers.entrywise).  CPU only.

A gradient entry is a sum of signed terms; the suite's rel_err holds it to a floor of 1e-3 of the largest gradient of the
call, so a small entry may lose or gain a term unseen.  The magnitudes give every entry a bound of its own; these tests check
that the magnitudes are right (a second restatement, oracle/numpy_naive.py, agrees; |sum| <= A <= M) and that the check
catches what rel_err lets through.
"""
import numpy as np
import pytest

import helpers as H
from oracle import numpy_naive as N
from oracle import oracle as O
from test_oracle_golden import CASE1, CASE2

K6_BOUND_DEFAULT = 1e-4  # tests/test_hip_parity.py: the suite's rel_err bounds of the two arithmetic modes
K6_BOUND_EXACT = 2e-6


def _scene(kind, rng, S):
    faces = H.random_scene(rng, 2, 30, spread=0.5, size=0.3)
    if kind == 'snapped':  # vertices on pixel centres: crossing points on pixel centres, |t| = 0 and 1 exactly
        xy = faces[..., :2]
        faces[..., :2] = (2 * np.round((xy * S + S - 1) / 2) + 1 - S) / S
    elif kind == 'clipped':  # faces past the image border on every side
        faces[..., :2] *= np.float32(2.2)
    return np.ascontiguousarray(faces, np.float32)


@pytest.mark.parametrize('kind', ['random', 'snapped', 'clipped'])
@pytest.mark.parametrize('eps', [0.0, 1e-10, 1e-3])
@pytest.mark.parametrize('rgb', [False, True], ids=['alpha', 'rgb_alpha'])
def test_magnitudes_match_the_numpy_restatement(kind, eps, rgb):
    """A (sum of |term|) and N (number of terms) of the C oracle equal the NumPy restatement's, entry by entry: A to 1e-12
    relative (the same float terms in another order), N exactly.  eps 0 makes dist exactly 0 on snapped scenes (infinite
    terms: the same entries must be infinite on both sides)."""
    S = 20
    rng = np.random.default_rng(900 + 10 * ['random', 'snapped', 'clipped'].index(kind) + 2 * [0.0, 1e-10, 1e-3].index(eps) + rgb)
    faces = _scene(kind, rng, S)
    bg = (0.3, 0.5, 0.2)
    textures = rng.uniform(0, 1, (2, 30, 2, 2, 2, 3)).astype(np.float32) if rgb else None
    fn = O.Rasterize(S, 0.1, 100, eps, bg, return_rgb=rgb, return_alpha=True)
    fn(faces, textures)
    g_rgb = rng.standard_normal((2, S, S, 3)).astype(np.float32) if rgb else None
    g_alpha = rng.standard_normal((2, S, S)).astype(np.float32)
    out = fn.backward(g_rgb, g_alpha, None, accumulate_double=True, magnitudes=True)
    ref, mags = out[0], out[-1]
    grad, a, n = N.backward_pixel_map(faces, fn.face_index_map, fn.rgb_map, fn.alpha_map, g_rgb, g_alpha, eps,
                                      magnitudes=True)
    assert (mags['N'] > 0).sum() > 50
    np.testing.assert_array_equal(mags['N'], n)
    fin = np.isfinite(a)
    np.testing.assert_array_equal(np.isfinite(mags['A']), fin)
    np.testing.assert_allclose(mags['A'][fin], a[fin], rtol=1e-12, atol=0)
    assert H.rel_err(grad[np.isfinite(grad)], ref[np.isfinite(grad)]) < 1e-6


def _check_invariants(ref_d, mags):
    """|sum of the terms| <= A <= M wherever finite (ref_d is the double sum rounded to float: half an ulp of slack)."""
    ref = np.asarray(ref_d, np.float64)
    for a, m in ((mags['A'], mags['M']), (mags.get('A8'), mags.get('M8'))):
        if a is not None:
            ok = np.isfinite(a) & np.isfinite(m)
            assert np.all(a[ok] <= m[ok])
    a = mags['A'] + mags.get('A8', 0)
    ok = np.isfinite(a) & np.isfinite(ref)
    assert np.all(np.abs(ref[ok]) <= a[ok] * (1 + 1e-12) + np.spacing(np.abs(ref[ok]).astype(np.float32)))
    assert np.all(mags['N'][mags['A'] == 0] == 0) and np.all(mags['A'][mags['N'] == 0] == 0)


@pytest.mark.parametrize('case', [CASE1, CASE2], ids=['case1', 'case2'])
def test_invariants_on_the_golden_gradient_cases(case):
    """The reference's grad_ref scenes (tests/test_oracle_golden.py): the golden pins keep their values (magnitudes=True
    changes no bit of the gradients) and |grad| <= A <= M."""
    vb, fb = H.to_minibatch((np.array(case['vertices'], np.float32), np.array([[0, 1, 2]], np.int32)))
    faces = O.vertices_to_faces(vb, fb)
    for rgb in (False, True):
        fn = O.Rasterize(64, 0.1, 100, 1e-4, (0, 0, 0), return_rgb=rgb, return_alpha=True, return_depth=True)
        textures = np.full((4, 1, 2, 2, 2, 3), 0.7, np.float32) if rgb else None
        fn(faces, textures)
        g_alpha = np.zeros((4, 64, 64), np.float32)
        g_alpha[:, case['pyi'], case['pxi']] = np.sign(fn.alpha_map[:, case['pyi'], case['pxi']] - case['target'])
        g_depth = np.random.default_rng(3).standard_normal((4, 64, 64)).astype(np.float32)
        g_rgb = np.random.default_rng(4).standard_normal((4, 64, 64, 3)).astype(np.float32) if rgb else None
        for acc in (False, True):
            plain = [x.copy() for x in fn.backward(g_rgb, g_alpha, g_depth, accumulate_double=acc)]
            out = fn.backward(g_rgb, g_alpha, g_depth, accumulate_double=acc, magnitudes=True)
            for x, y in zip(plain, out[:-1]):
                np.testing.assert_array_equal(x, y)
        _check_invariants(out[0], out[-1])
        if rgb:
            ok = out[-1]['Nt'] > 0
            assert np.all(np.abs(out[1].astype(np.float64)) <= out[-1]['At'] * (1 + 1e-6) + 1e-30) and ok.any()


@pytest.mark.parametrize('seed', range(4))
def test_invariants_on_random_scenes(seed):
    rng = np.random.default_rng(800 + seed)
    S = [16, 33, 64, 40][seed]
    faces = H.random_scene(rng, 2, 60, spread=0.7, size=0.3)
    textures = rng.uniform(-1, 2, (2, 60, 3, 3, 3, 3)).astype(np.float32)   # colours beyond [0, 1]: kappa > 1
    fn = O.Rasterize(S, 0.1, 100, [1e-3, 1e-4, 0.0, 1e-10][seed], (0.9, -0.4, 1.5), True, True, True)
    fn(faces, textures)
    g = [rng.standard_normal(s).astype(np.float32) for s in ((2, S, S, 3), (2, S, S), (2, S, S))]
    ref_d, ref_t, mags = fn.backward(*g, accumulate_double=True, magnitudes=True)
    _check_invariants(ref_d, mags)
    assert (mags['N8'] > 0).any() and np.all(mags['N8'][..., 2] == mags['N8'][..., 0])
    assert np.all(np.abs(ref_t.astype(np.float64)) <= mags['At'] * (1 + 1e-6) + 1e-30)
    # the oracle's own outputs are within their bounds in every mode (a check that rejects the reference is no check)
    for mode in H.MODES[:-1]:
        assert H.entrywise(ref_d, ref_d, mags, mode)[0] <= 1
    # and the reference's serial float sums too (what any float-summing kernel could return)
    ref_f = fn.backward(*g)[0]
    assert H.entrywise(ref_f, ref_d, mags, 'row')[0] <= 1


def _gap_scene():
    """Two clusters of faces, one in the top-left quadrant, one in the bottom-right, and a loss weighted by a mask: the
    gradient maps are 1e-5 of their scale outside the top-left quadrant.  The bottom-right faces' lines meet only
    down-weighted pixels, so their gradients are ~1e-5 of the largest one and their terms smaller still."""
    S = 48
    rng = np.random.default_rng(71)
    a = H.random_scene(rng, 1, 40, spread=0.25, size=0.2)
    a[..., :2] += np.float32(-0.5)
    b = H.random_scene(rng, 1, 40, spread=0.25, size=0.2)
    b[..., :2] += np.float32(0.5)
    faces = np.concatenate((a, b), 1)
    textures = rng.uniform(0, 1, (1, 80, 2, 2, 2, 3)).astype(np.float32)
    fn = O.Rasterize(S, 0.1, 100, 1e-3, (0.2, 0.4, 0.6), True, True, False)
    fn(faces, textures)
    w = np.full((S, S), 1e-5, np.float32)
    w[:S // 2, :S // 2] = 1
    g_rgb = (rng.normal(size=(1, S, S, 3)) * w[..., None]).astype(np.float32)
    g_alpha = (rng.normal(size=(1, S, S)) * w).astype(np.float32)
    return fn, g_rgb, g_alpha


@pytest.mark.parametrize('mode,pixel,rel_bound', [('row', (35, 37), K6_BOUND_DEFAULT), ('exact', (36, 12), K6_BOUND_EXACT)])
def test_entrywise_catches_a_removed_term_that_rel_err_accepts(mode, pixel, rel_bound):
    """The gap this check closes.  Entry (0, 52, 1, 0) of the scene is ~5e-6 of the largest gradient.  Removing the terms
    that one pixel contributes to it -- the oracle's own terms, obtained by zeroing that pixel's gradient -- moves it by
    less than rel_err's bound of the mode times the floor (1e-3 of the largest gradient), so the suite's metric accepts the
    result; the entrywise bound of the same mode rejects it, and it accepts the unperturbed oracle output."""
    fn, g_rgb, g_alpha = _gap_scene()
    ref_d, _, mags = fn.backward(g_rgb, g_alpha, None, accumulate_double=True, magnitudes=True)
    ref_d = ref_d.copy()
    entry = (0, 52, 1, 0)
    mx = float(np.abs(ref_d).max())
    assert 1e-6 < abs(float(ref_d[entry])) / mx < 3e-5
    y, x = pixel
    g2, a2 = g_rgb.copy(), g_alpha.copy()
    g2[0, y, x] = 0
    a2[0, y, x] = 0
    without = fn.backward(g2, a2, None, accumulate_double=True)[0]
    got = ref_d.copy()
    got[entry] = without[entry]                                # only this entry loses the pixel's terms
    assert got[entry] != ref_d[entry]
    assert H.rel_err(got, ref_d) <= rel_bound                  # the floor metric does not see it ...
    worst, bad = H.entrywise(got, ref_d, mags, mode)
    assert worst > 1 and [tuple(i) for i in bad] == [entry]    # ... the entrywise bound does, and only there
    assert H.entrywise(ref_d, ref_d, mags, mode)[0] <= 1


def test_entrywise_mode_bounds_are_ordered():
    """exact <= row <= fast per entry (fewer roundings, shorter float sums), 'default' the larger of row and fast, and
    grad_textures' bound grows with its number of terms."""
    fn, g_rgb, g_alpha = _gap_scene()
    ref_d, ref_t, mags = fn.backward(g_rgb, g_alpha, None, accumulate_double=True, magnitudes=True)
    b = {m: H.entrywise_bound(ref_d, mags, m) for m in ('exact', 'row', 'fast', 'default', 'global')}
    assert np.all(b['exact'] <= b['row']) and np.all(b['row'] <= b['fast'])
    np.testing.assert_allclose(b['default'], np.maximum(b['row'], b['fast']), rtol=1e-14, atol=0)
    np.testing.assert_array_equal(b['global'], b['exact'])
    bt = H.entrywise_bound(ref_t, mags, 'textures')
    assert np.all(bt >= H.gamma(mags['Nt']) * mags['At'])
    # a NaN entry is skipped, not reported
    got = ref_d.copy()
    got[0, 0, 0, 0] = np.nan
    assert H.entrywise(got, ref_d, mags, 'exact')[0] <= 1


def test_entry_points_of_oracle_version_4_keep_their_signatures():
    """oracle_backward_pixel_map / _textures / _depth_map keep the argument lists they had before the magnitudes (a caller
    built against them passes no magnitude buffers); the magnitudes come through the *_mags entry points.  Called with the
    old argument lists, they return the same bits as Rasterize.backward."""
    import ctypes
    rng = np.random.default_rng(12)
    S = 32
    faces = H.random_scene(rng, 2, 40)
    textures = rng.uniform(0, 1, (2, 40, 2, 2, 2, 3)).astype(np.float32)
    fn = O.Rasterize(S, 0.1, 100, 1e-3, (0.2, 0.4, 0.6), True, True, True)
    fn(faces, textures)
    g_rgb, g_alpha, g_depth = [rng.standard_normal(s).astype(np.float32) for s in ((2, S, S, 3), (2, S, S), (2, S, S))]
    ref_gf, ref_gt = [x.copy() for x in fn.backward(g_rgb, g_alpha, g_depth)]
    L = O.lib()
    f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    p = lambda a, t: a.ctypes.data_as(t)
    gf = np.zeros_like(fn.faces)
    gt = np.zeros_like(fn.textures)
    visits = ctypes.c_longlong(0)
    L.oracle_backward_pixel_map(p(fn.faces, f32p), p(fn.face_index_map, i32p), p(fn.rgb_map, f32p), p(fn.alpha_map, f32p),
                                p(g_rgb, f32p), p(g_alpha, f32p), p(gf, f32p), 2, 40, S, ctypes.c_double(1e-3), 1, 1,
                                ctypes.byref(visits), 0)
    L.oracle_backward_textures(p(fn.face_index_map, i32p), p(fn.sampling_weight_map, f32p), p(fn.sampling_index_map, i32p),
                               p(g_rgb, f32p), p(gt, f32p), 2, 40, S, 2, None)
    L.oracle_backward_depth_map(p(fn.faces, f32p), p(fn.depth_map, f32p), p(fn.face_index_map, i32p), p(fn.face_inv_map, f32p),
                                p(fn.weight_map, f32p), p(g_depth, f32p), p(gf, f32p), 2, 40, S, None)
    assert visits.value == fn.visits > 0
    np.testing.assert_array_equal(gf.view(np.int32), ref_gf.view(np.int32))
    np.testing.assert_array_equal(gt.view(np.int32), ref_gt.view(np.int32))
