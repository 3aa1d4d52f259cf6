"""`-m gpu`: the fused backward's third launch order -- the K7 / K8 gather's workgroups behind k_bpm_row's in ONE grid
(k_band_gather; plan_backward: gather_in_tail, calls above 96 k faces with texture_size 2) -- against the serial order
(NR_FLAG_SERIAL_BACKWARD: line setup | band kernel | gather, each a launch of its own).  The same kernel bodies on the same
data; K6's rounded sums and K8's meet in one float addition per element either way:

  grad_textures  bit for bit (the outputs are pre-filled with NaN: every zero is stored by somebody);
  grad_faces     bit for bit in the exact mode; in the default mode up to the order in which the double atomics add a face's
                 records -- the allowance of tests/test_sharding_gpu.py: at most two entries differ, 1e-6 in the parity metric.

Shapes: the headline batch, 32 views (just above the gate of 96 k faces), 132 views at 128 x 128 (the largest teapot batch
under the order's upper bound, NR_TAIL_GATHER_MAX_FACES = 655 360 faces), a batch with a face above 2048 candidate pixels in every view (so that
k_backward_big walks faces, beside rounding K6's sums onto grad_faces) and a batch in which every third image's line records
overflow the line buffer (the overflow-only launch of k_bpm_fast behind the merged launch does work)."""
import numpy as np
import pytest

import abi
import helpers as H

pytestmark = pytest.mark.gpu

SERIAL = 64  # _lib.NR_FLAG_SERIAL_BACKWARD
EXACT = 2    # _lib.NR_FLAG_EXACT_GRADIENT
GATE_FACES = 98304  # NR_SHARED_LAUNCH_MAX_FACES: calls above it leave the gather-first order
MAX_FACES = 655360  # NR_TAIL_GATHER_MAX_FACES


def _both_orders(faces, textures, S, modes, seed, bg=(0.1, 0.2, 0.3)):
    rgb, alpha, depth = modes
    B, F = faces.shape[:2]
    assert GATE_FACES < B * F <= MAX_FACES, (B, F)
    fw = abi.forward_fused(faces, textures, S, 0.1, 100.0, 1e-3, bg, 0, rgb, alpha, depth)
    rng = np.random.default_rng(seed)
    g_rgb = rng.normal(size=(B, S, S, 3)).astype(np.float32) if rgb else None
    g_alpha = rng.normal(size=(B, S, S)).astype(np.float32) if alpha else None
    g_depth = rng.normal(size=(B, S, S)).astype(np.float32) if depth else None
    out = {}
    for mode_flag, name in ((0, 'default'), (EXACT, 'exact')):
        gf_s, gt_s = [abi.host(t) for t in abi.backward_fused(fw, g_rgb, g_alpha, g_depth, k6_flags=mode_flag | SERIAL)]
        gf_t, gt_t = [abi.host(t) for t in abi.backward_fused(fw, g_rgb, g_alpha, g_depth, k6_flags=mode_flag)]
        assert np.isfinite(gf_s).all() and np.isfinite(gf_t).all()
        assert np.abs(gf_s).max() > 0 and np.abs(gt_s).max() > 0
        differing, rel = int((gf_s != gf_t).sum()), H.rel_err(gf_t, gf_s)
        print('%s: B %d F %d S %d: grad_faces entries differing %d of %d, rel %.3g; grad_textures differing %d'
              % (name, B, F, S, differing, gf_s.size, rel, int((gt_s != gt_t).sum())))
        if differing:
            print('    images with differing grad_faces entries:', np.flatnonzero((gf_s != gf_t).reshape(B, -1).any(axis=1)).tolist())
        np.testing.assert_array_equal(gt_t, gt_s, err_msg='grad_textures, %s mode' % name)
        if mode_flag == EXACT:
            np.testing.assert_array_equal(gf_t, gf_s, err_msg='grad_faces, exact mode')
        else:
            assert differing <= 2 and rel <= 1e-6, (differing, rel)
        out[name] = (gf_t, gt_t)
    return fw, out


def _teapots(B, S, seed):
    faces, _ = H.teapot_views(B, S)
    rng = np.random.default_rng(seed)
    textures = rng.uniform(0, 1, (B, faces.shape[1], 2, 2, 2, 3)).astype(np.float32)
    return faces, textures


@pytest.mark.parametrize('B,S', [(64, 256), (32, 256), (132, 128)], ids=['headline', 'above_gate', 'upper_bound'])
def test_tail_order_equals_serial_order(B, S):
    faces, textures = _teapots(B, S, 900 + B)
    if B == 132:
        assert MAX_FACES - faces.shape[1] < B * faces.shape[1] <= MAX_FACES  # one more view would leave the order
    _both_orders(faces, textures, S, (True, True, True), seed=901 + B)


@pytest.mark.parametrize('modes', [(True, False, False), (True, True, False), (True, False, True)], ids=['rgb', 'rgb_alpha', 'rgb_depth'])
def test_tail_order_other_output_modes(modes):
    """The merged kernel's other instantiations: without alpha, without K8."""
    faces, textures = _teapots(32, 128, 930)
    _both_orders(faces, textures, 128, modes, seed=931)


def test_tail_order_with_faces_for_k_backward_big():
    """A backdrop triangle behind the teapot in every view: ~6 000 candidate pixels at 128 x 128 (above BIG_PX = 2048), most of
    them its own -- the face gather leaves it out, k_backward_big walks it and, in the tail order, also rounds K6's sums of
    every listed face onto grad_faces (FINISH_BIG)."""
    faces, textures = _teapots(32, 128, 940)
    faces = faces.copy()
    faces[:, 0] = np.array([[-0.9, -0.85, 50.0], [0.9, -0.85, 50.0], [0.0, 0.9, 50.0]], np.float32)
    fw, out = _both_orders(faces, textures, 128, (True, True, True), seed=941)
    owned = (abi.host(fw['face_index_map']) == 0).sum(axis=(1, 2))
    assert owned.min() > 2048, owned.min()
    gf, gt = out['default']
    assert np.abs(gt[:, 0]).max() > 0 and np.abs(gf[:, 0]).max() > 0  # the backdrop's own gradients arrived


def test_tail_order_with_images_over_the_line_buffer():
    """Every third image holds 800 faces that span most of a 64 x 64 raster: far more line records than the buffer's
    8 F + 32 S + 1.2 S sqrt(F); the other images fit.  k_bpm_row's workgroups leave such an image at once and the overflow-only
    launch of k_bpm_fast behind the merged launch serves it."""
    rng = np.random.default_rng(950)
    B, F, S = 126, 800, 64
    big = H.random_scene(rng, B, F, spread=0.4, size=1.2)
    faces = H.random_scene(rng, B, F, spread=0.5, size=0.1)
    faces[::3] = big[::3]
    textures = rng.uniform(0, 1, (B, F, 2, 2, 2, 3)).astype(np.float32)
    fw, _ = _both_orders(faces, textures, S, (True, True, True), seed=951)
    # the records of an image: one per visible face, edge, axis and integer line inside the edge's extent (rasterize.py:567-569)
    fi = abi.host(fw['face_index_map'])
    capacity = 8 * F + 32 * S + int(1.2 * S * np.sqrt(F))
    records = []
    for b in range(B):
        vis = np.unique(fi[b][fi[b] >= 0])
        p = (faces[b, vis, :, :2].astype(np.float64) * S + S - 1) / 2
        n = 0
        for e in range(3):
            for ax in range(2):
                lo = np.maximum(np.ceil(np.minimum(p[:, e, ax], p[:, (e + 1) % 3, ax])), 0)
                hi = np.minimum(np.floor(np.maximum(p[:, e, ax], p[:, (e + 1) % 3, ax])), S - 1)
                n += int(np.maximum(hi - lo + 1, 0).sum())
        records.append(n)
    records = np.array(records)
    print('line records: capacity %d, large images %d..%d, small images %d..%d'
          % (capacity, records[::3].min(), records[::3].max(), np.delete(records, np.s_[::3]).min(), np.delete(records, np.s_[::3]).max()))
    assert records[::3].min() > capacity and np.delete(records, np.s_[::3]).max() < capacity
