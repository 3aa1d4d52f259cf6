"""`-m gpu`: every launch plan of the fused backward that the grid of tests/backward_plans.py reaches (CASES: one call per plan,
test_backward_plans.py keeps the table complete on the host), run through the C ABI against the oracle.

Per case: the forward maps bit for bit; the fused backward on outputs pre-filled with NaN (every zero is stored by somebody)
against the oracle's exactly summed terms under the suite's criteria -- grad_textures rel_err <= 1e-4 and every element within
its own bound (helpers.entrywise), grad_faces within test_fuzz_unusual_parameters' bound (helpers.grad_faces_bounds /
err_default) and every entry within its own bound in the mode that ran, NaN where the oracle has NaN; then the same call in the
serial order (NR_FLAG_SERIAL_BACKWARD): grad_textures bit for bit, grad_faces within SAME_TERMS.

Per-face light colours have no oracle of their own: grad_textures and grad_light are held to the lit-texture call of the same
scene through the chain rule of the host-side product, as tests/test_face_light_gpu.py does (GRAD_TOL), and to the oracle's
lit-texture gradients through the same chain rule (1e-4).

Each test first asserts, through the measurement build, that the call it is about to make takes the plan recorded with its
case in the table (`signature`).

Above texture size 13 K7 is the per-pixel scatter (k_backward_textures_atomic, csrc/nr_backward_gather.hip): hardware float
atomics onto global memory, one launch that both orders make identically.  A float sum of three or more atomically added
terms has no defined order -- on faces of hundreds of pixels two runs of ONE order differ in hundreds of elements --, so a
bit-for-bit comparison says something about the plan only where the sum is the same in any order: the scenes of these cases
have faces of about a pixel, and test_backward_plans.py asserts that no element of grad_textures receives more than two
terms (0 + a is exact, a + b commutes).  An unzeroed cube or a gather that ran twice still shows in every element."""
import numpy as np
import pytest

import abi
import backward_plans as P
import helpers as H
from neural_renderer_amd import _build
from oracle import oracle as O
from test_face_light_gpu import GRAD_TOL
from test_hip_parity import SAME_TERMS, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def profile_lib():
    _build.build_profile()  # (the measurement build, with the staleness check of tests/test_abi.py)
    return P.hook()

BG = (0.1, 0.2, 0.3)


def _chain(case, g_lit, textures):
    """gradients of the lit, duplicated cubes -> (gradient of the original cubes, gradient of the colours): the chain rule of
    oracle_textures' product, in double"""
    n = textures.shape[1]
    light = P.light_colors(case).astype(np.float64)
    g = np.asarray(g_lit, np.float64)
    t_all = np.concatenate((textures, textures.transpose((0, 1, 4, 3, 2, 5))), axis=1).astype(np.float64)
    gt = g[:, :n] * light[:, :n, None, None, None, :] + (g[:, n:] * light[:, n:, None, None, None, :]).transpose((0, 1, 4, 3, 2, 5))
    return gt, (g * t_all).sum(axis=(2, 3, 4))


def _close(a, b, tol):
    """test_face_light_gpu._close's metric: the largest difference over the largest component"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a[ok] - b[ok]).max() / max(np.abs(b[ok]).max(), 1e-30)) / tol if ok.any() else 0.0


@pytest.mark.parametrize('case', P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_plan_against_the_oracle(case):
    c = case['call']
    B, F, S, ts, eps, flags = c['B'], c['F'], c['S'], c['ts'], c['eps'], c['flags']
    rgb, alpha, depth = [bool(m) for m in c['modes']]
    faces, cubes = P.scene(case)
    textures = P.oracle_textures(case, cubes) if rgb else None
    g = P.upstream(case)

    fn = O.Rasterize(S, 0.1, 100.0, eps, BG, rgb, alpha, depth)
    fn(faces, textures) if rgb else fn(faces)
    fw = abi.forward_fused(faces, textures, S, 0.1, 100.0, eps, BG, 0, rgb, alpha, depth)
    np.testing.assert_array_equal(abi.host(fw['face_index_map']), fn.face_index_map)
    for k in ('weight_map', 'depth_map', 'rgb_map', 'alpha_map'):
        if getattr(fn, k) is not None and fw.get(k) is not None:
            assert np.array_equal(abi.host(fw[k]), getattr(fn, k), equal_nan=True), k

    # the plan of the call about to be made, from what is passed, against the signature recorded with the case
    made = P.call(fw['B'], fw['F'], fw['S'], fw['ts'] if rgb else 2, tuple(int(x is not None) for x in g), flags, fw['eps'],
                  int(c['lit'] and rgb), c['mis'], c['visible'], c['ws'])
    assert P.signature(made) == case['signature'], (made, P.named(P.signature(made)), P.named(case['signature']))
    sig = P.named(case['signature'])

    lit = dict(light=P.light_colors(case), textures=cubes, grad_light=True) if c['lit'] and rgb else None

    def run(extra_flags, face_light=lit):
        out = abi.backward_fused(fw, *g, k6_flags=flags | extra_flags, use_visible=bool(c['visible']), tex_offset=c['mis'],
                                 workspace_bytes=c['ws'] or None, face_light=face_light)
        return [abi.host(t) for t in out]

    out = run(0)
    gf, gt = out[0], out[1]
    ref = fn.backward(*g, accumulate_double=True, magnitudes=True)
    ref_gf, ref_gt, mags = ref[0], (ref[1] if rgb else None), ref[-1]
    noise, b_default, b_exact = H.grad_faces_bounds(fn.backward(*g)[0], ref_gf)
    ref_k6 = fn.backward(g[0], g[1], None if g[2] is None else np.zeros_like(g[2]), accumulate_double=True)[0]
    exact = bool(flags & P.EXACT)
    ratios = {}

    # grad_faces
    assert np.array_equal(np.isnan(gf), np.isnan(ref_gf)), 'grad_faces: NaN pattern'
    ok = np.isfinite(ref_gf) & np.isfinite(gf)
    e_gf = (H.rel_err(gf[ok], ref_gf[ok]) if exact else H.err_default(gf, ref_gf, ref_k6, ok)) if ok.any() else 0.0
    bound = b_exact if exact else b_default
    ratios['grad_faces'] = e_gf / bound
    ratios['grad_faces entrywise'], bad_f = H.entrywise(gf, ref_gf, mags, 'exact' if exact else 'default')
    # grad_textures
    if rgb and lit is None:
        assert np.array_equal(np.isnan(gt), np.isnan(ref_gt)), 'grad_textures: NaN pattern'
        ok = np.isfinite(ref_gt) & np.isfinite(gt)
        ratios['grad_textures'] = (H.rel_err(gt[ok], ref_gt[ok]) if ok.any() else 0.0) / 1e-4
        ratios['grad_textures entrywise'], bad_t = H.entrywise(gt, ref_gt, mags, 'textures')
    elif rgb:
        gl = out[2]
        plain = run(0, face_light=None)  # the lit-texture call of the same scene: the plan of the unlit call
        want_gt, want_gl = _chain(case, plain[1], cubes)
        o_gt, o_gl = _chain(case, ref_gt, cubes)
        assert np.array_equal(np.isnan(gt), np.isnan(want_gt.astype(np.float32))), 'grad_textures: NaN pattern'
        assert np.array_equal(np.isnan(gl), np.isnan(want_gl.astype(np.float32))), 'grad_light: NaN pattern'
        assert np.array_equal(np.isnan(plain[1]), np.isnan(ref_gt)), 'grad_textures of the lit-texture call: NaN pattern'
        ratios['grad_textures (lit-texture call)'] = _close(gt, want_gt, GRAD_TOL)
        ratios['grad_light (lit-texture call)'] = _close(gl, want_gl, GRAD_TOL)
        ok = np.isfinite(o_gt) & np.isfinite(gt)
        ratios['grad_textures'] = (H.rel_err(gt[ok], o_gt[ok]) if ok.any() else 0.0) / 1e-4
        ok = np.isfinite(o_gl) & np.isfinite(gl)
        ratios['grad_light'] = (H.rel_err(gl[ok], o_gl[ok]) if ok.any() else 0.0) / 1e-4
        assert np.array_equal(plain[0], gf, equal_nan=True) or H.rel_err(plain[0], gf) <= SAME_TERMS  # (the light does not enter grad_faces)

    # the serial order: the same kernel bodies on the same data, every step a launch of its own
    if not flags & P.SERIAL:
        serial = run(P.SERIAL)
        differing = int((~((serial[0] == gf) | (np.isnan(serial[0]) & np.isnan(gf)))).sum())
        okf = np.isfinite(serial[0]) & np.isfinite(gf)
        ratios['serial order grad_faces'] = (H.rel_err(gf[okf], serial[0][okf]) if okf.any() else 0.0) / SAME_TERMS
        assert np.array_equal(np.isnan(serial[0]), np.isnan(gf))
        tex_diff = 0
        if rgb:
            tex_diff = int((~((serial[1] == gt) | (np.isnan(serial[1]) & np.isnan(gt)))).sum())
        print('serial order: grad_faces entries differing %d of %d (%.3g of SAME_TERMS), grad_textures differing %d'
              % (differing, gf.size, ratios['serial order grad_faces'], tex_diff))
        ratios['serial order grad_textures differing'] = tex_diff
    # a depth-only call builds K8's lists in the workspace when it is large enough: the same call with a workspace of one byte
    # takes the plan without them (asserted through the hook) and sums the same terms
    if sig['depth_lists']:
        small = dict(made, ws=1)
        assert P.named(P.signature(small))['depth_lists'] == 0
        gf_small = [abi.host(t) for t in abi.backward_fused(fw, *g, k6_flags=flags, use_visible=True, workspace_bytes=1)][0]
        ratios['without lists grad_faces'] = H.rel_err(gf_small, gf) / SAME_TERMS
    print(P.case_id(case), {k: sig[k] for k in ('gather_first', 'gather_in_tail', 'tex_zeros', 'finish', 'face_zeros', 'big_overflow')},
          'noise %.2e' % noise, {k: float('%.3g' % v) for k, v in ratios.items()})
    report('backward_plans', case=P.case_id(case), ratios=ratios, noise=noise)
    over = {k: v for k, v in ratios.items() if (v > 0 if k.endswith('differing') else not v <= 1)}
    assert not over, (over, [tuple(i) for i in bad_f[:3]])
    # the scene reached the gradients at all
    finite = ref_gf[np.isfinite(ref_gf)]
    assert finite.size and np.abs(finite).max() > 0
