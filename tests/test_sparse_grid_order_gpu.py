"""`-m gpu`: the working-first order of the sparse launches over (list slots, image) -- k_line_setup and the gather part of
k_band_gather take (slot workgroup, image) = (id / B, id % B) from a 1-D id (image_fastest, nr_device.h); k_line_setup holds
four words per line across its ownership reads and derives the rest of the line's head again.  The same workgroups in another
order, the same records: what could break is a workgroup that never runs, runs twice or takes another image's slots, or a
record whose bits change.  The other launches over the lists (k_setup_gather, the stage calls' gathers) keep the order of
their 2-D grids and run here beside them.

Every scene runs the fused backward in the order its plan picks (gather-first up to 98 304 faces, the gather in the band
kernel's grid tail above) and with NR_FLAG_SERIAL_BACKWARD, in both arithmetic modes, on outputs pre-filled with NaN:

  grad_textures  bit for bit between the orders;
  grad_faces     bit for bit in the exact mode; in the default mode up to the order in which the double atomics add a face's
                 records -- the allowance of tests/test_sharding_gpu.py: at most two entries differ, 1e-6 in the parity metric;
  every result   against the oracle with the bounds of tests/test_hip_parity.py (check_backward) for the same mode.

Shapes: B in {1, 3, 7} (no multiple of the 8 XCDs), F in {33, 100, 1025} (one, a few and more than LS_FACES = 32 list
positions per workgroup; 1025: two compaction chunks), rasters 16 and 32; with three images or more one image's faces are
all back-facing (list length 0) and one image lists many more faces than the others, so that the number of working
workgroups differs from image to image; 97 images (just above the gate) with every fifth image empty; list lengths on both
sides of a workgroup's share (16 faces per gather workgroup, 32 per line-setup workgroup)."""
import numpy as np
import pytest

import abi
import helpers as H
import test_hip_parity as P

pytestmark = pytest.mark.gpu

SERIAL, EXACT, K6_SCAN = P.SERIAL, P.EXACT, P.K6_SCAN
GATE_FACES = 98304  # NR_SHARED_LAUNCH_MAX_FACES: calls above it leave the gather-first order
BG = (0.1, 0.2, 0.3)
EPS = 1e-3
MODES = (True, True, True)


def _front(faces, front):
    """faces with the winding that makes them front-facing (front) or back-facing: the rasterizer skips a face whose
    (p2y - p0y) (p1x - p0x) < (p1y - p0y) (p2x - p0x) (rasterize.py:119-120)."""
    f = faces.copy()
    d1, d2 = f[..., 1, :2] - f[..., 0, :2], f[..., 2, :2] - f[..., 0, :2]
    is_front = d2[..., 1] * d1[..., 0] > d1[..., 1] * d2[..., 0]
    swap = is_front != front
    f[swap] = f[swap][:, [0, 2, 1]]
    return f


def _mixed_scene(rng, B, F):
    """Image 0: every face front-facing (a long list); image 1 (B >= 3): every face back-facing (an empty list); the others:
    one face in sixteen front-facing."""
    faces = H.random_scene(rng, B, F, spread=0.8, size=0.2)
    keep = rng.uniform(size=(B, F)) < 0.0625
    out = np.where(keep[:, :, None, None], _front(faces, True), _front(faces, False))
    out[0] = _front(faces[0], True)
    if B >= 3:
        out[1] = _front(faces[1], False)
    return np.ascontiguousarray(out, np.float32)


def _grid_scene(rng, F, S, counts):
    """Per image exactly counts[b] faces that own a pixel: disjoint front-facing triangles around pixel centres three pixels
    apart, at random places in the face array; every other face back-facing."""
    B = len(counts)
    faces = _front(H.random_scene(rng, B, F, spread=0.8, size=0.2), False)
    centres = [(x, y) for y in range(2, S - 1, 3) for x in range(2, S - 1, 3)]
    assert max(counts) <= len(centres)
    tri = np.array([[-1.3, -1.1], [1.3, -1.1], [0.0, 1.3]])
    for b, n in enumerate(counts):
        where = rng.choice(F, size=n, replace=False)
        cells = rng.choice(len(centres), size=n, replace=False)
        for fn, ci in zip(where, cells):
            px = np.array(centres[ci], np.float64) + tri      # pixel coordinates: an integer is a pixel's centre
            faces[b, fn, :, :2] = (2.0 * px + 1.0 - S) / S    # p = (x S + S - 1) / 2
        faces[b, where] = _front(faces[b, where], True)
    return np.ascontiguousarray(faces, np.float32)


def _listed(fw):
    """faces that own a pixel, per image (the length of K6's visible-face list)"""
    fi = abi.host(fw['face_index_map'])
    return [int(np.unique(fi[b][fi[b] >= 0]).size) for b in range(fi.shape[0])]


class _Reference:
    """the oracle's gradients of one scene, computed once: the literal ones, the double-summed ones, the term magnitudes"""

    def __init__(self, faces, textures, S, grads):
        self.fn = P.oracle_forward(faces, textures, S, 0.1, 100, EPS, BG, *MODES)
        ref = self.fn.backward(*grads)
        self.gf, self.gt = ref[0].copy(), ref[1].copy()
        ref_dd = self.fn.backward(*grads, accumulate_double=True, magnitudes=True)
        self.gf_d, self.gt_d, self.mags = ref_dd[0].copy(), ref_dd[1].copy(), ref_dd[-1]
        self.noise = H.rel_err(self.gf, self.gf_d)
        self.noise_t = H.rel_err(self.gt, self.gt_d)

    def check(self, gf, gt, flags, what):
        """tests/test_hip_parity.py check_backward's assertions on one result (depth on: K8's float partial sums)"""
        assert not np.isnan(gf).any(), '%s: grad_faces has unwritten elements' % what
        bound = max(P.K6_BOUND_EXACT if flags & EXACT else P.K6_BOUND_DEFAULT, 1e-5)
        err_d, err_f = H.rel_err(gf, self.gf_d), H.rel_err(gf, self.gf)
        assert err_d <= bound, '%s: grad_faces vs double-summed oracle: %g (flags %d)' % (what, err_d, flags)
        assert err_f <= P.RTOL + 2 * self.noise, '%s: grad_faces rel err %g (noise %g)' % (what, err_f, self.noise)
        worst, bad = H.entrywise(gf, self.gf_d, self.mags, P.k6_mode(flags))
        assert worst <= 1, '%s: %d grad_faces entries beyond their bound, worst %.3g' % (what, len(bad), worst)
        if gt is not None:
            assert not np.isnan(gt).any(), '%s: grad_textures has unwritten elements' % what
            assert H.rel_err(gt, self.gt_d) <= P.RTOL, '%s: grad_textures vs double-summed oracle' % what
            assert H.rel_err(gt, self.gt) <= P.RTOL + 2 * self.noise_t, '%s: grad_textures' % what
            worst_t, bad_t = H.entrywise(gt, self.gt_d, self.mags, 'textures')
            assert worst_t <= 1, '%s: %d grad_textures elements beyond their bound, worst %.3g' % (what, len(bad_t), worst_t)


def _forward(faces, S, seed):
    rng = np.random.default_rng(seed)
    B, F = faces.shape[:2]
    textures = rng.uniform(0, 1, (B, F, 2, 2, 2, 3)).astype(np.float32)
    fw = abi.forward_fused(faces, textures, S, 0.1, 100.0, EPS, BG, 0, *MODES)
    grads = (rng.normal(size=(B, S, S, 3)).astype(np.float32), rng.normal(size=(B, S, S)).astype(np.float32),
             rng.normal(size=(B, S, S)).astype(np.float32))
    ref = _Reference(faces, textures, S, grads)
    P.check_forward(fw, ref.fn)
    return fw, grads, ref


def _both_orders(fw, grads, ref):
    for mode_flag, name in ((0, 'default'), (EXACT, 'exact')):
        gf_s, gt_s = [abi.host(t) for t in abi.backward_fused(fw, *grads, k6_flags=mode_flag | SERIAL)]
        gf_p, gt_p = [abi.host(t) for t in abi.backward_fused(fw, *grads, k6_flags=mode_flag)]
        ref.check(gf_s, gt_s, mode_flag, name + ', serial order')
        ref.check(gf_p, gt_p, mode_flag, name + ', planned order')
        differing, rel = int((gf_s != gf_p).sum()), H.rel_err(gf_p, gf_s)
        print('%s: B %d F %d S %d: grad_faces entries differing %d of %d, rel %.3g; grad_textures differing %d'
              % (name, fw['B'], fw['F'], fw['S'], differing, gf_s.size, rel, int((gt_s != gt_p).sum())))
        np.testing.assert_array_equal(gt_p, gt_s, err_msg='grad_textures, %s mode' % name)
        if mode_flag == EXACT:
            np.testing.assert_array_equal(gf_p, gf_s, err_msg='grad_faces, exact mode')
        else:
            assert differing <= 2 and rel <= 1e-6, (differing, rel)


def _stage_calls(fw, grads, ref):
    """nr_backward_pixel_map (line-setup path and NR_FLAG_K6_SCAN), nr_backward_textures and nr_backward_depth_map alone"""
    for flags in (0, K6_SCAN, EXACT, EXACT | K6_SCAN):
        gf, gt = [abi.host(t) for t in abi.backward(fw, *grads, k6_flags=flags)]
        ref.check(gf, gt, flags, 'stage calls, flags %d' % flags)


@pytest.mark.parametrize('S', [16, 32])
@pytest.mark.parametrize('F', [33, 100, 1025])
@pytest.mark.parametrize('B', [1, 3, 7])
def test_gather_first_order(B, F, S):
    assert B * F <= GATE_FACES
    faces = _mixed_scene(np.random.default_rng(7000 + 100 * B + F + S), B, F)
    fw, grads, ref = _forward(faces, S, 7001 + B + F + S)
    n = _listed(fw)
    print('listed faces per image:', n)
    if B >= 3:
        assert n[1] == 0, n
        if F >= 100:
            assert n[0] >= 2 * max(n[1:]), n
    _both_orders(fw, grads, ref)


def test_tail_order_every_fifth_image_empty():
    B, F, S = 97, 1025, 32
    assert B * F > GATE_FACES
    rng = np.random.default_rng(7100)
    faces = _mixed_scene(rng, B, F)
    faces[1] = _front(faces[1], True)  # (the mixed scene's empty image: here the empty ones are every fifth)
    faces[::5] = _front(faces[::5], False)
    fw, grads, ref = _forward(faces, S, 7101)
    n = _listed(fw)
    assert all(n[b] == 0 for b in range(0, B, 5)) and min(n[b] for b in range(B) if b % 5) > 0, n
    _both_orders(fw, grads, ref)
    _stage_calls(fw, grads, ref)


@pytest.mark.parametrize('B,F,S', [(3, 1025, 32), (7, 100, 16)])
def test_stage_calls_alone(B, F, S):
    faces = _mixed_scene(np.random.default_rng(7200 + B), B, F)
    fw, grads, ref = _forward(faces, S, 7201 + B)
    _stage_calls(fw, grads, ref)


@pytest.mark.parametrize('counts', [(0, 65), (15, 33), (16, 32), (17, 31)], ids=lambda c: '%d_%d' % c)
def test_list_lengths_around_a_workgroups_share(counts):
    F, S = 2100, 32
    faces = _grid_scene(np.random.default_rng(7300 + counts[0]), F, S, counts)
    fw, grads, ref = _forward(faces, S, 7301 + counts[0])
    assert tuple(_listed(fw)) == counts, _listed(fw)
    _both_orders(fw, grads, ref)
    _stage_calls(fw, grads, ref)
