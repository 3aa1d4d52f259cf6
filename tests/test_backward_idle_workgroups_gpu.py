"""`-m gpu`: the fused backward without its idle workgroups -- the overflow pass of k_bpm_fast inside k_backward_big's launch
(k_big_overflow: the last overflow workgroup to take a ticket finishes the overflowed images' faces), k_line_setup and the
gather part of k_band_gather on a quarter of the list slots with a loop (NR_SLOT_STRIDE), k_setup_gather's ids image-fastest
-- against the serial order (NR_FLAG_SERIAL_BACKWARD: every launch of its own, one workgroup per slot) and against the oracle.

  grad_textures  bit for bit against the serial order (the outputs are pre-filled with NaN: every zero is stored by somebody);
  grad_faces     bit for bit in the exact mode; in the default mode up to the order in which the double atomics add a face's
                 records: at most two entries differ, 1e-6 in the parity metric (tests/test_backward_tail_order_gpu.py);
  both           against the oracle's double-summed terms within the suite's bounds (tests/test_hip_parity.py: grad_faces 1e-4
                 in the default mode, 2e-6 -- 1e-5 with K8's float sums -- in the exact one; grad_textures 1e-4).

One oracle pass per scene, shared by the two arithmetic modes."""
import numpy as np
import pytest

import abi
import helpers as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SERIAL = 64  # _lib.NR_FLAG_SERIAL_BACKWARD
EXACT = 2    # _lib.NR_FLAG_EXACT_GRADIENT
GATE_FACES = 98304  # NR_SHARED_LAUNCH_MAX_FACES: up to it the gather-first order, above it the tail order
BOUND_DEFAULT, BOUND_EXACT, BOUND_K8, RTOL = 1e-4, 2e-6, 1e-5, 1e-4  # tests/test_hip_parity.py
BG = (0.1, 0.2, 0.3)


def _against_serial_and_oracle(faces, textures, S, seed):
    B, F = faces.shape[:2]
    fw = abi.forward_fused(faces, textures, S, 0.1, 100.0, 1e-3, BG, 0, True, True, True)
    rng = np.random.default_rng(seed)
    g_rgb = rng.normal(size=(B, S, S, 3)).astype(np.float32)
    g_alpha = rng.normal(size=(B, S, S)).astype(np.float32)
    g_depth = rng.normal(size=(B, S, S)).astype(np.float32)
    fn = O.Rasterize(S, 0.1, 100, 1e-3, BG, True, True, True)
    fn(faces, textures)
    assert int((abi.host(fw['face_index_map']) != fn.face_index_map).sum()) == 0
    ref = fn.backward(g_rgb, g_alpha, g_depth, accumulate_double=True)
    ref_gf, ref_gt = ref[0], ref[1]
    out = {}
    for mode_flag, name in ((0, 'default'), (EXACT, 'exact')):
        gf_s, gt_s = [abi.host(t) for t in abi.backward_fused(fw, g_rgb, g_alpha, g_depth, k6_flags=mode_flag | SERIAL)]
        gf_n, gt_n = [abi.host(t) for t in abi.backward_fused(fw, g_rgb, g_alpha, g_depth, k6_flags=mode_flag)]
        assert np.isfinite(gf_s).all() and np.isfinite(gf_n).all() and np.isfinite(gt_n).all()
        differing, rel = int((gf_s != gf_n).sum()), H.rel_err(gf_n, gf_s)
        bound = max(BOUND_EXACT if mode_flag else BOUND_DEFAULT, BOUND_K8)
        err_gf = H.rel_err(gf_n, ref_gf) if np.abs(ref_gf).max() > 0 else float(np.abs(gf_n).max())
        err_gt = H.rel_err(gt_n, ref_gt) if np.abs(ref_gt).max() > 0 else float(np.abs(gt_n).max())
        print('%s: B %d F %d S %d: grad_faces entries differing from the serial order %d of %d, rel %.3g; grad_textures differing '
              '%d; against the oracle: grad_faces %.3g (bound %.0e), grad_textures %.3g'
              % (name, B, F, S, differing, gf_s.size, rel, int((gt_s != gt_n).sum()), err_gf, bound, err_gt))
        np.testing.assert_array_equal(gt_n, gt_s, err_msg='grad_textures, %s mode' % name)
        if mode_flag == EXACT:
            np.testing.assert_array_equal(gf_n, gf_s, err_msg='grad_faces, exact mode')
        else:
            assert differing <= 2 and rel <= 1e-6, (differing, rel)
        assert err_gf <= bound, (name, err_gf)
        assert err_gt <= RTOL, (name, err_gt)
        out[name] = (gf_n, gt_n)
    return fw, out


def _line_records(fw, faces, S):
    """the records of each image: one per visible face, edge, axis and integer line inside the edge's extent (rasterize.py:567-569)"""
    fi = abi.host(fw['face_index_map'])
    records = []
    for b in range(faces.shape[0]):
        vis = np.unique(fi[b][fi[b] >= 0])
        p = (faces[b, vis, :, :2].astype(np.float64) * S + S - 1) / 2
        n = 0
        for e in range(3):
            for ax in range(2):
                lo = np.maximum(np.ceil(np.minimum(p[:, e, ax], p[:, (e + 1) % 3, ax])), 0)
                hi = np.minimum(np.floor(np.maximum(p[:, e, ax], p[:, (e + 1) % 3, ax])), S - 1)
                n += int(np.maximum(hi - lo + 1, 0).sum())
        records.append(n)
    return np.array(records)


def _overflow_scene(B, F, S, seed, large):
    """images `large` (a boolean mask) hold F faces that span most of the raster -- far more line records than the buffer's
    8 F + 32 S + 1.2 S sqrt(F) --, the others small faces that fit (the scene of tests/test_backward_tail_order_gpu.py)"""
    rng = np.random.default_rng(seed)
    big = H.random_scene(rng, B, F, spread=0.4, size=1.2)
    faces = H.random_scene(rng, B, F, spread=0.5, size=0.1)
    faces[large] = big[large]
    textures = rng.uniform(0, 1, (B, F, 2, 2, 2, 3)).astype(np.float32)
    return faces, textures


def _check_overflow(fw, faces, S, large):
    F = faces.shape[1]
    capacity = 8 * F + 32 * S + int(1.2 * S * np.sqrt(F))
    records = _line_records(fw, faces, S)
    print('line records: capacity %d, large images %s, small images %s'
          % (capacity, records[large].tolist()[:8], records[~large].tolist()[:8]))
    assert (records[large] > capacity).all() and (records[~large] < capacity).all()


def _mask(B, which):
    m = np.zeros(B, bool)
    m[list(which)] = True
    return m


def test_overflow_in_the_gather_first_order():
    """Images 0 and 3 of six are over the line buffer: the overflow workgroups in front of k_backward_big's walk their bands, the
    last one to take a ticket rounds their K6 sums onto grad_faces; the other four images are finished by k_backward_big's threads."""
    B, F, S = 6, 800, 64
    large = _mask(B, (0, 3))
    faces, textures = _overflow_scene(B, F, S, 1100, large)
    assert B * F <= GATE_FACES
    fw, _ = _against_serial_and_oracle(faces, textures, S, 1101)
    _check_overflow(fw, faces, S, large)


def test_overflow_in_the_tail_order():
    """The same scene with 124 images (99 200 faces, just above the gate): the band kernel with the gather in its tail, then the
    merged overflow pass."""
    B, F, S = 124, 800, 64
    large = _mask(B, (0, 3))
    faces, textures = _overflow_scene(B, F, S, 1110, large)
    assert B * F > GATE_FACES
    fw, _ = _against_serial_and_oracle(faces, textures, S, 1111)
    _check_overflow(fw, faces, S, large)


@pytest.mark.parametrize('every', [True, False], ids=['all', 'none'])
def test_every_image_over_the_buffer_and_none(every):
    """all: k_backward_big's threads finish nothing, the last ticket everything.  none: no ticket is taken."""
    B, F, S = 6, 800, 64
    large = np.full(B, every)
    faces, textures = _overflow_scene(B, F, S, 1120, large)
    fw, _ = _against_serial_and_oracle(faces, textures, S, 1121)
    _check_overflow(fw, faces, S, large)


def test_big_face_in_an_overflowed_image():
    """A sliver along the diagonal in front of every image's faces: a box of ~3 700 candidate pixels at 64 x 64 (above BIG_PX =
    2048) of which it owns a hundred, so the images keep their records.  In the two overflowed images it is listed, and the
    deferred finish adds its K6 sums with float atomics beside the K8 sums that one of k_backward_big's workgroups adds in the
    same launch."""
    B, F, S = 6, 800, 64
    large = _mask(B, (0, 3))
    faces, textures = _overflow_scene(B, F, S, 1130, large)
    sliver = np.array([[-0.95, -0.95, 0.5], [0.95, 0.9, 0.5], [0.9, 0.95, 0.5]], np.float32)
    faces[:, 0] = sliver[::-1] if _is_backside(sliver) else sliver
    p = (faces[0, 0, :, :2].astype(np.float64) * S + S - 1) / 2
    assert np.prod(np.floor(p.max(axis=0)) - np.ceil(p.min(axis=0)) + 1) > 2048  # its box of candidate pixels
    fw, out = _against_serial_and_oracle(faces, textures, S, 1131)
    _check_overflow(fw, faces, S, large)
    owned = (abi.host(fw['face_index_map']) == 0).sum(axis=(1, 2))
    print('pixels the sliver owns, per image:', owned.tolist())
    assert owned.min() > 0  # listed in every image, the overflowed ones among them
    gf, gt = out['default']
    assert (np.abs(gf[:, 0]).max(axis=(1, 2)) > 0).all() and (np.abs(gt[:, 0]).reshape(B, -1).max(axis=1) > 0).all()


def _tiles(B, F, S, seed, off_screen):
    """F small front-facing triangles per image around the centres of every second pixel in x and y: no two overlap and each
    owns its centre pixel, so every face is listed; image `off_screen` has all of them outside the raster: an empty list."""
    rng = np.random.default_rng(seed)
    per_row = S // 2
    assert F <= per_row * per_row
    k = np.arange(F)
    centre = np.stack([2 * (k % per_row) + 1, 2 * (k // per_row) + 1], axis=1)  # pixel units: a pixel's centre is its number
    ang = rng.uniform(0, 2 * np.pi, (B, F, 1)) + np.array([0.0, 2.0, 4.0]) * np.pi / 3  # counter-clockwise
    rad = rng.uniform(0.6, 0.9, (B, F, 1))
    px = centre[None, :, None, 0] + rad * np.cos(ang)
    py = centre[None, :, None, 1] + rad * np.sin(ang)
    faces = np.empty((B, F, 3, 3), np.float32)
    faces[..., 0] = (2 * px + 1 - S) / S
    faces[..., 1] = (2 * py + 1 - S) / S
    faces[..., 2] = rng.uniform(1, 3, (B, F, 1))
    if _is_backside(faces[0, 0]):
        faces = np.ascontiguousarray(faces[:, :, ::-1])
    faces[off_screen, :, :, 0] += 4.0
    textures = rng.uniform(0, 1, (B, F, 2, 2, 2, 3)).astype(np.float32)
    return np.ascontiguousarray(faces), textures


def _is_backside(face):
    """the rasterizer's orientation test: such a face is not drawn"""
    (x0, y0), (x1, y1), (x2, y2) = face[:, :2].astype(np.float64)
    return (y2 - y0) * (x1 - x0) < (y1 - y0) * (x2 - x0)


@pytest.mark.parametrize('B', [3, 400], ids=['line_setup_loops', 'tail_gather_loops'])
def test_strided_slots_with_full_and_empty_lists(B):
    """250 listed faces of 250 -- 8 line-setup slots and 16 gather slots, neither a multiple of the stride, on launches of a
    quarter of them: every workgroup loops -- and one image whose list is empty.  3 images take the gather-first order (the line
    setup inside k_setup_gather loops), 400 (100 000 faces) the tail order (the gather inside k_band_gather loops as well)."""
    F, S = 250, 32
    faces, textures = _tiles(B, F, S, 1140 + B, off_screen=1)
    assert (B * F > GATE_FACES) == (B == 400)
    fw, out = _against_serial_and_oracle(faces, textures, S, 1141 + B)
    vis = abi.host(fw['visible_faces']).astype(bool)
    assert vis[np.arange(B) != 1].all() and not vis[1].any()
    gf, gt = out['default']
    assert (np.abs(gf[0]).max(axis=(1, 2)) > 0).all() and not gf[1].any() and not gt[1].any()


@pytest.mark.parametrize('B', [16, 24, 12])
def test_small_batches_equal_their_slices(B):
    """Which workgroup, and which XCD, serves an image must not show in its results: a batch against its halves and quarters,
    in the way of tests/test_full_size_gpu.py::test_headline_batch_equals_its_shards (maps and grad_textures the same bits;
    grad_faces up to the order of the double atomics that add a face's records: 1e-6 in the parity metric)."""
    S = 64
    faces, _ = H.teapot_views(B, S)
    rng = np.random.default_rng(1150 + B)
    textures = rng.uniform(0, 1, (B, faces.shape[1], 2, 2, 2, 3)).astype(np.float32)
    g_rgb = rng.normal(size=(B, S, S, 3)).astype(np.float32)
    g_alpha = rng.normal(size=(B, S, S)).astype(np.float32)
    g_depth = rng.normal(size=(B, S, S)).astype(np.float32)

    def run(sl, flags):
        fw = abi.forward_fused(faces[sl], textures[sl], S, 0.1, 100.0, 1e-3, BG, 0, True, True, True, faces_z_ref=faces[0])
        gf, gt = abi.backward_fused(fw, g_rgb[sl], g_alpha[sl], g_depth[sl], k6_flags=flags)
        return abi.host(fw['rgb_map']), abi.host(fw['alpha_map']), abi.host(gt), abi.host(gf)

    for flags in (0, EXACT):
        full = run(slice(0, B), flags)
        for n in (2, 4):
            step = B // n
            parts = [run(slice(i * step, (i + 1) * step), flags) for i in range(n)]
            for k, name in enumerate(('rgb_map', 'alpha_map', 'grad_textures')):
                np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), full[k], err_msg='%s, %d slices' % (name, n))
            got = np.concatenate([p[3] for p in parts])
            e = H.rel_err(got, full[3])
            print('B %d flags %d slices %d: grad_faces rel %.3g, bit-equal %s' % (B, flags, n, e, np.array_equal(got, full[3])))
            assert e <= 1e-6, (flags, n, e)
