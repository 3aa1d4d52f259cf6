"""Fuzz parity (GPU): random small scenes with unusual parameters -- raster sizes 1..64 (odd, tiny), near / far / eps values
far from the defaults (eps = 0 and eps below float32 resolution included), faces behind the camera, vertices snapped onto
pixel centres (ties, edges through centres), duplicated faces, per-image backgrounds, the batch-z flag -- through the C ABI
against the oracle: forward maps bit for bit (NaN == NaN), gradients NaN in the same places and within tolerance elsewhere,
staged and fused backward."""
import numpy as np
import pytest

import abi
import helpers as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (a soak run: NR_FUZZ_EXTRA_SEEDS="4 5 6 ..." adds seeds to the parameter, dense-scene and error-level tests below; the suite itself runs the fixed ones)
import os
EXTRA_SEEDS = [int(x) for x in os.environ.get('NR_FUZZ_EXTRA_SEEDS', '').split()]


@pytest.mark.parametrize('seed', [1, 2, 3, 6, 118] + EXTRA_SEEDS)  # (6: the scene at the metric's worst case, see the bound below;
# 118: a crossing point half an ulp below a pixel centre -- the out sweep's second pixel, which k_bpm_row's first version dropped)
def test_fuzz_unusual_parameters(seed):
    from test_hip_parity import report
    rng = np.random.default_rng(seed)
    failures = []
    worst, above = {}, {}
    for it in range(60):
        B = int(rng.integers(1, 4))
        F = int(rng.integers(1, 50))
        S = int(rng.choice([1, 2, 3, 5, 8, 16, 31, 32, 47, 64]))
        ts = int(rng.choice([2, 2, 3, 4]))
        eps = float(rng.choice([0.0, 1e-10, 1e-4, 1e-3, 0.1, 1.0]))
        near = float(rng.choice([1e-6, 0.1, 0.5, 1.7]))
        far = float(rng.choice([2.0, 10.1, 100, 1e10]))
        faces = H.random_scene(rng, B, F, spread=float(rng.choice([0.3, 0.8, 1.5])), size=float(rng.choice([0.05, 0.3, 1.2])),
                               zmin=float(rng.choice([-1.0, 0.05, 1.0])), zmax=3.0)
        if rng.uniform() < 0.5:   # snap some vertices onto pixel centres
            q = (np.round((faces[..., :2] * S + S - 1) / 2) * 2 + 1 - S) / S
            m = rng.uniform(size=faces[..., :2].shape) < 0.5
            faces[..., :2] = np.where(m, q, faces[..., :2]).astype(np.float32)
        if rng.uniform() < 0.3 and F > 1:   # reversed duplicates of the first half
            faces[:, F // 2:] = faces[:, : F - F // 2][:, :, ::-1]
        textures = rng.uniform(0, 1, (B, F, ts, ts, ts, 3)).astype(np.float32)
        bg = rng.uniform(0, 1, (B, 3)).astype(np.float32) if rng.uniform() < 0.5 else (0.2, 0.4, 0.6)
        flags = int(rng.integers(0, 2))
        fn = O.Rasterize(S, near, far, eps, bg, True, True, True, bool(flags))
        fn(faces, textures)
        fw = abi.forward(faces, textures, S, near, far, eps, bg, flags, True, True, True)
        msg = []
        if int((abi.host(fw['face_index_map']) != fn.face_index_map).sum()):
            msg.append('face_index_map')
        for k in ('weight_map', 'depth_map', 'rgb_map', 'alpha_map'):
            if not np.array_equal(abi.host(fw[k]), getattr(fn, k), equal_nan=True):
                msg.append(k)
        g = [rng.normal(size=x.shape).astype(np.float32) for x in (fn.rgb_map, fn.alpha_map, fn.depth_map)]
        if rng.uniform() < 0.3:
            g[0][rng.uniform(size=g[0].shape) < 0.5] = 0
        ref_gf, ref_gt, mags = fn.backward(*g, accumulate_double=True, magnitudes=True)
        # default K6 numerics (staged and fused entry points; the default mode runs k_bpm_row; 128: NR_FLAG_K6_LEGACY -- the same
        # terms on k_bpm_fast) within the north star's 1e-4 of the reference's terms summed exactly, PLUS twice the reference's
        # own float-summation noise on the scene (its serial float sums against the same exact sum) -- the allowance the float
        # comparison of tests/test_hip_parity.py::check_backward has.  Why not the plain 1e-4: the default mode is ~1 ulp per
        # term, and the metric's floor is 1e-3 of the largest gradient: a full ulp on the largest term of an entry that cancels
        # down to the floor reads as 2^-23 / 1e-3 = 1.2e-4.  k_bpm_row refines the reciprocals of the two pixels next to the
        # crossing point (a record's largest terms) with a Newton step, which took round 5's soak maximum (seed 6, scene 59:
        # 1.13e-4) to 7e-5 and kept 48 scenes x 60 below 1e-4 -- 100 more seeds then found 1.8e-4 in a scene built to cancel
        # (test_fuzz_default_k6_error_levels, seed 185; k_bpm_fast 1.5e-4), which neither a Newton step on every reciprocal nor
        # double sums in every lane move (LAB-NOTEBOOK, round 6): the terms themselves differ from the reference's by ~1 ulp
        # (another order of roundings).  On such entries the reference's own sums differ from run to run (float atomics) by more.
        # NR_FLAG_EXACT_GRADIENT: K6's terms are the reference's bit for bit and summed in double (2e-6 on K6 alone:
        # test_hip_parity.py); with a depth gradient K8's float partial sums come on top -- 2e-5 plus the same allowance.
        # (the bounds and the default mode's metric: helpers.grad_faces_bounds / helpers.err_default, shared with
        # test_backward_plans_gpu.py)
        ref_f, _ = fn.backward(*g)
        noise, b_default, b_exact = H.grad_faces_bounds(ref_f, ref_gf)
        # grad_faces = K6's sums + K8's (the depth gradient's), and the two can cancel: the default mode's ~1e-6 of a K6 sum of 8
        # is 4e-4 of a total that cancels to the metric's floor (seed 171, scene 47: 4.3e-4 by helpers.rel_err with the exact
        # mode at 0 and K6 alone at 1.6e-6).  The default-mode runs are therefore measured against the larger of the total and
        # its K6 part, element by element, with the floor at 1e-3 of the larger maximum; the exact mode keeps the plain metric.
        ref_k6 = fn.backward(g[0], g[1], np.zeros_like(g[2]), accumulate_double=True)[0]

        def err_default(a, ok):
            return H.err_default(a, ref_gf, ref_k6, ok)
        for name, run, bound in (('backward', abi.backward, b_default), ('backward_fused', abi.backward_fused, b_default),
                                 ('backward_legacy', lambda *a: abi.backward(*a, k6_flags=128), b_default),
                                 ('backward_fused_legacy', lambda *a: abi.backward_fused(*a, k6_flags=128), b_default),
                                 ('backward_exact', lambda *a: abi.backward(*a, k6_flags=2), b_exact),
                                 ('backward_fused_exact', lambda *a: abi.backward_fused(*a, k6_flags=2), b_exact)):
            gf, gt = run(fw, *g)
            gf, gt = abi.host(gf), abi.host(gt)
            if not np.array_equal(np.isnan(gf), np.isnan(ref_gf)) or not np.array_equal(np.isnan(gt), np.isnan(ref_gt)):
                msg.append(name + ': NaN pattern')
            ok = np.isfinite(ref_gf) & np.isfinite(gf)
            e_gf = (H.rel_err(gf[ok], ref_gf[ok]) if name.endswith('exact') else err_default(gf, ok)) if ok.any() else 0.0
            if e_gf > bound:
                msg.append('%s: grad_faces %.2e (bound %.2e, reference noise %.2e)' % (name, e_gf, bound, noise))
            ok = np.isfinite(ref_gt) & np.isfinite(gt)
            if ok.any() and H.rel_err(gt[ok], ref_gt[ok]) > 1e-4:
                msg.append('%s: grad_textures %.2e' % (name, H.rel_err(gt[ok], ref_gt[ok])))
            # every entry against its own term magnitudes (helpers.entrywise), in the mode of the kernel that ran
            mode = 'exact' if name.endswith('exact') else ('fast' if name.endswith('legacy') else 'default')
            w_f, bad_f = H.entrywise(gf, ref_gf, mags, mode)
            w_t, bad_t = H.entrywise(gt, ref_gt, mags, 'textures')
            worst[name] = max(worst.get(name, 0.0), w_f)
            worst[name + ' grad_textures'] = max(worst.get(name + ' grad_textures', 0.0), w_t)
            above[name] = above.get(name, 0) + H.above_1e4(gf, ref_gf)
            if w_f > 1 or w_t > 1:
                msg.append('%s: entrywise grad_faces %.3g at %s, grad_textures %.3g at %s' % (
                    name, w_f, [tuple(i) for i in bad_f[:3]], w_t, [tuple(i) for i in bad_t[:3]]))
        if msg:
            failures.append((it, dict(B=B, F=F, S=S, ts=ts, eps=eps, near=near, far=far, flags=flags), msg))
    report('fuzz_unusual_parameters', seed=seed, entrywise_worst=worst, above_1e4_elementwise=above)
    assert not failures, failures


@pytest.mark.parametrize('seed', [11, 12] + [1000 + x for x in EXTRA_SEEDS])
def test_fuzz_dense_scenes(seed):
    """Larger random scenes (up to 3000 faces, raster sizes up to 256 incl. non-powers of two, random output modes): several
    scan passes and line windows per band, accumulator-slot overflow, the large-face queue of the forward."""
    from test_hip_parity import report
    rng = np.random.default_rng(seed)
    failures = []
    worst, above = {}, {}
    for it in range(8):
        B = int(rng.integers(1, 3))
        F = int(rng.choice([200, 700, 1500, 3000]))
        S = int(rng.choice([64, 100, 128, 200, 256]))
        ts = int(rng.choice([2, 3]))
        eps = float(rng.choice([1e-4, 1e-3]))
        modes = [(True, True, True), (True, False, False), (False, True, False), (True, True, False)][int(rng.integers(0, 4))]
        faces = H.random_scene(rng, B, F, spread=float(rng.choice([0.4, 0.9])), size=float(rng.choice([0.03, 0.1, 0.4])))
        textures = rng.uniform(0, 1, (B, F, ts, ts, ts, 3)).astype(np.float32)
        rgb, alpha, depth = modes
        fn = O.Rasterize(S, 0.1, 100, eps, (0.2, 0.4, 0.6), rgb, alpha, depth)
        fn(faces, textures) if rgb else fn(faces)
        fw = abi.forward(faces, textures if rgb else None, S, 0.1, 100.0, eps, (0.2, 0.4, 0.6), 0, rgb, alpha, depth)
        msg = []
        if int((abi.host(fw['face_index_map']) != fn.face_index_map).sum()):
            msg.append('face_index_map')
        g_rgb = rng.normal(size=(B, S, S, 3)).astype(np.float32) if rgb else None
        g_alpha = rng.normal(size=(B, S, S)).astype(np.float32) if alpha else None
        g_depth = rng.normal(size=(B, S, S)).astype(np.float32) if depth else None
        ref = fn.backward(g_rgb, g_alpha, g_depth, accumulate_double=True, magnitudes=True)
        mags = ref[-1]
        for name, run, bound in (('backward', abi.backward, 1e-4), ('backward_fused', abi.backward_fused, 1e-4),
                                 ('backward_fused_exact', lambda *a: abi.backward_fused(*a, k6_flags=2), 1e-5)):
            gf, gt = run(fw, g_rgb, g_alpha, g_depth)
            e = H.rel_err(abi.host(gf), ref[0])
            if not e <= bound:
                msg.append('%s: grad_faces %.2e' % (name, e))
            if rgb:
                e = H.rel_err(abi.host(gt), ref[1])
                if not e <= 1e-4:
                    msg.append('%s: grad_textures %.2e' % (name, e))
            # every entry against its own term magnitudes (helpers.entrywise)
            w_f, bad_f = H.entrywise(abi.host(gf), ref[0], mags, 'exact' if name.endswith('exact') else 'default')
            w_t = H.entrywise(abi.host(gt), ref[1], mags, 'textures')[0] if rgb else 0.0
            worst[name] = max(worst.get(name, 0.0), w_f, w_t)
            above[name] = above.get(name, 0) + H.above_1e4(abi.host(gf), ref[0])
            if w_f > 1 or w_t > 1:
                msg.append('%s: entrywise grad_faces %.3g at %s, grad_textures %.3g' % (name, w_f, [tuple(i) for i in bad_f[:3]],
                                                                                        w_t))
        if msg:
            failures.append((it, dict(B=B, F=F, S=S, ts=ts, eps=eps, modes=modes), msg))
    report('fuzz_dense_scenes', seed=seed, entrywise_worst=worst, above_1e4_elementwise=above)
    assert not failures, failures


def _coverage_mismatches(faces, S):
    fn = O.Rasterize(S, 0.1, 100, 1e-3, (0, 0, 0), False, True, True)
    fn(faces)
    fw = abi.forward(faces, None, S, 0.1, 100.0, 1e-3, (0, 0, 0), 0, False, True, True)
    same_depth = np.array_equal(abi.host(fw['depth_map']), fn.depth_map, equal_nan=True)
    return int((abi.host(fw['face_index_map']) != fn.face_index_map).sum()) + (0 if same_depth else 1)


@pytest.mark.parametrize('seed', [21, 22])
def test_fuzz_micro_triangles_and_needles(seed):
    """Coverage parity where the reference's rounded inside test (rasterize.py:310-312) is least intuitive: triangles of a
    few ulps to 0.1 NDC around pixel centres, a vertex exactly on a centre, edges through a centre, collinear triples, and
    needles whose apex angle is 3e-9 .. 1e-3 rad aimed exactly at another pixel centre (the test accepts pixels far along a
    needle's axis; faces that thin are exempt from screen-box culling, face_bbox)."""
    rng = np.random.default_rng(seed)
    bad = []
    for it in range(40):
        S = int(rng.choice([8, 16, 32, 33, 64]))
        F = 256
        kind = rng.integers(0, 4, F)
        c = (2 * rng.integers(0, S, (F, 1, 2)) + 1 - S) / S
        base = rng.normal(size=(F, 3, 2)) * 10.0 ** rng.uniform(-9, -1, (F, 1, 1))
        base[kind == 1, 2] = (rng.normal(size=(F, 2)) * 10.0 ** rng.uniform(-3, 0.5, (F, 1)))[kind == 1]   # long third vertex
        base[kind == 2, 0] = 0                                   # a vertex exactly on the pixel centre
        base[kind == 3, 1] = -base[kind == 3, 0]                 # an edge through the centre
        faces = np.zeros((1, F, 3, 3), np.float32)
        faces[0, :, :, :2] = (c + base).astype(np.float32)
        faces[..., 2] = rng.uniform(1, 3, (1, F, 3)).astype(np.float32)
        if _coverage_mismatches(faces, S):
            bad.append(('micro', it, S))
        # needles: apex A near a pixel centre, axis through another centre, apex angle theta
        i0, i1 = rng.integers(0, S, (F, 2)), rng.integers(0, S, (F, 2))
        c0, c1 = (2 * i0 + 1 - S) / S, (2 * i1 + 1 - S) / S
        u = c1 - c0
        n = np.linalg.norm(u, axis=1, keepdims=True)
        u = u / np.where(n == 0, 1, n)
        th = 10.0 ** rng.uniform(-8.5, -3, F) * rng.choice([-1, 1], F)
        t1, t2 = 10.0 ** rng.uniform(-7, -0.5, (F, 1)), 10.0 ** rng.uniform(-7, -0.5, (F, 1))
        rot = np.stack((u[:, 0] * np.cos(th) - u[:, 1] * np.sin(th), u[:, 0] * np.sin(th) + u[:, 1] * np.cos(th)), axis=1)
        A = c0 + rng.normal(size=(F, 2)) * 10.0 ** rng.uniform(-9, -6, (F, 1)) * (rng.uniform(size=(F, 1)) < 0.5)
        faces[0, :, 0, :2], faces[0, :, 1, :2], faces[0, :, 2, :2] = A, A - u * t1, A - rot * t2
        f = faces[0]
        back = ((f[:, 2, 1] - f[:, 0, 1]) * (f[:, 1, 0] - f[:, 0, 0]) < (f[:, 1, 1] - f[:, 0, 1]) * (f[:, 2, 0] - f[:, 0, 0]))
        f[back] = f[back][:, ::-1]
        if _coverage_mismatches(faces, S):
            bad.append(('needle', it, S))
    assert not bad, bad


@pytest.mark.parametrize('seed', [31, 32, 112, 121, 185] + [100 + x for x in EXTRA_SEEDS])  # (112, 121: the bright scenes that caught round 5's sums
# around K = 0; 185: the soak's worst scene for the default mode, 1.8e-4 with the reference's own float sums 7e-4 off)
def test_fuzz_default_k6_error_levels(seed):
    """How far the default (tolerance-mode) K6 kernel gets from the exactly summed reference terms on scenes built to cancel:
    many overlapping faces of similar, bright colours (small `diff`, both signs), large and small `eps` (with a large eps every
    term of a sweep has the same size, so thousands of comparable terms cancel), alpha-only and colour-only modes, meshes seen
    edge-on.  The default kernel is ~1 ulp per term with double sums above a record, so its deviation in the parity metric
    (helpers.rel_err: |a - b| / max(|b|, 1e-3 max|b|)) stays at a few 1e-5 -- except on entries that cancel down to the metric's
    floor, where one ulp of a large term reads as 1.2e-4: the bound is the north star's 1e-4 plus twice the reference's own
    float-summation noise on the scene (which is what such entries measure).  The levels, and the reference's noise beside them,
    go to gpurun_out/parity_errors.jsonl (`worst` per scene family)."""
    from test_hip_parity import icosphere, project_mesh, report
    rng = np.random.default_rng(seed)
    worst = {}
    failures = []
    for it in range(14):
        family = ['soup', 'bright_soup', 'sphere', 'teapot', 'big_faces'][it % 5]
        S = int(rng.choice([96, 128, 200, 256]))
        eps = float(rng.choice([1e-4, 1e-3, 1e-2, 0.1]))
        B = 2
        if family in ('soup', 'bright_soup'):
            faces = H.random_scene(rng, B, int(rng.choice([800, 2500])), spread=0.7, size=float(rng.choice([0.08, 0.25])))
        elif family == 'big_faces':
            faces = H.random_scene(rng, B, 60, spread=0.5, size=1.2)
        elif family == 'sphere':
            v0, f0 = icosphere(3)
            faces = np.stack([project_mesh((v0 * (0.5 + 0.2 * rng.normal(size=(v0.shape[0], 1)))).astype(np.float32), f0,
                                           [float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)), -2.6])
                              for _ in range(B)])
        else:
            faces = H.teapot_views(64, S)[0][rng.integers(0, 64, B)]
        F = faces.shape[1]
        if family == 'bright_soup':  # nearly equal colours: `diff` is the small difference of large products
            textures = (0.9 + 0.1 * rng.uniform(size=(B, F, 2, 2, 2, 3))).astype(np.float32)
            bg = (0.95, 0.95, 0.95)
        else:
            textures = rng.uniform(0, 1, (B, F, 2, 2, 2, 3)).astype(np.float32)
            bg = (0.1, 0.2, 0.3)
        rgb, alpha = [(True, True), (True, False), (False, True)][int(rng.integers(0, 3))]
        fn = O.Rasterize(S, 0.1, 100, eps, bg, rgb, alpha, False)
        fn(faces, textures) if rgb else fn(faces)
        fw = abi.forward(faces, textures if rgb else None, S, 0.1, 100.0, eps, bg, 0, rgb, alpha, False)
        assert int((abi.host(fw['face_index_map']) != fn.face_index_map).sum()) == 0
        scale = float(rng.choice([1.0, 100.0]))
        g_rgb = (scale * rng.normal(size=(B, S, S, 3))).astype(np.float32) if rgb else None
        g_alpha = (scale * rng.normal(size=(B, S, S))).astype(np.float32) if alpha else None
        out = fn.backward(g_rgb, g_alpha, None, accumulate_double=True, magnitudes=True)
        ref, mags = out[0], out[-1]
        noise = H.rel_err(fn.backward(g_rgb, g_alpha, None)[0], ref)  # the reference's own serial float sums against the exact sum
        gf = abi.host(abi.backward_fused(fw, g_rgb, g_alpha, None)[0])                 # the default mode: k_bpm_row
        gp = abi.host(abi.backward_fused(fw, g_rgb, g_alpha, None, k6_flags=128)[0])   # k_bpm_fast (NR_FLAG_K6_LEGACY)
        ge = abi.host(abi.backward_fused(fw, g_rgb, g_alpha, None, k6_flags=2)[0])
        e_def, e_px, e_exact = H.rel_err(gf, ref), H.rel_err(gp, ref), H.rel_err(ge, ref)
        worst[family] = max(worst.get(family, 0.0), e_def)
        worst[family + ' (k_bpm_fast)'] = max(worst.get(family + ' (k_bpm_fast)', 0.0), e_px)
        worst[family + ' (reference float sums)'] = max(worst.get(family + ' (reference float sums)', 0.0), noise)
        # (the bound: the north star's 1e-4 plus twice the reference's own float-summation noise on the scene -- see
        # test_fuzz_unusual_parameters; the exact mode: K6 alone, 2e-6)
        bound = 1e-4 + 2 * noise
        if not e_def <= bound or not e_px <= bound or not e_exact <= 2e-6:
            failures.append((it, family, dict(S=S, eps=eps, rgb=rgb, alpha=alpha, F=F), e_def, e_px, e_exact, noise))
        # every entry against its own term magnitudes (helpers.entrywise): is the noise allowance above only cancellation?
        for run, got, mode in (('default', gf, 'default'), ('k_bpm_fast', gp, 'fast'), ('exact', ge, 'exact')):
            w, bad = H.entrywise(got, ref, mags, mode)
            key = '%s %s entrywise' % (family, run)
            worst[key] = max(worst.get(key, 0.0), w)
            key = '%s %s above_1e4_elementwise' % (family, run)
            worst[key] = worst.get(key, 0) + H.above_1e4(got, ref)
            if w > 1:
                failures.append((it, family, dict(S=S, eps=eps, rgb=rgb, alpha=alpha, F=F), run, 'entrywise %.3g' % w,
                                 [tuple(i) for i in bad[:3]]))
    report('fuzz_default_k6_error_levels', seed=seed, worst=worst)
    assert not failures, failures


def test_fuzz_band_kernels_against_each_other():
    """K6's two band kernels against each other, without the oracle, on 300 random scenes at rasters up to 1024 and down to 2
    (scripts/kernel_cross_soak.py): the exact modes agree in every bit of grad_faces, the default modes to 1e-4 of the largest
    gradient (measured over 18 000 scenes: 7e-7) -- a dropped or doubled pixel of either kernel reads as 1e-2."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env in (dict(N='200', SEED='5'), dict(N='100', SEED='6', SIZES='2 3 5 8 9 16 24')):
        out = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'kernel_cross_soak.py')], cwd=root, capture_output=True,
                             text=True, timeout=900, env=dict(os.environ, **env))
        assert out.returncode == 0, out.stderr[-2000:]
        last = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
        assert last['flagged'] == 0 and last['worst']['exact_bits'] <= 2, out.stdout[-2000:]
