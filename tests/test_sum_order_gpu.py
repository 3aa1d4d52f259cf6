"""The ORDER of the fixed-order sums (DESIGN "Fixed-order sums and scans"; csrc/nr_reduce.h), pinned on two outputs that show
a double sum without a float32 rounding in between that would hide it: the IoU loss's `sums` (doubles) and the point-mesh
loss on values whose float32 result depends on the order of the double additions.  Other tests show that two runs agree and
that values lie within bounds of float64 restatements; neither would notice another fixed order.

The replay below is written from the words of that DESIGN section, in numpy float64:
  * a thread adds its own terms in the kernel's stated order;
  * the wave's butterfly: v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1, after which every lane holds the same bits;
  * the waves of a workgroup in wave order, starting from wave 0's value;
  * the workgroups of an image in block order, starting from 0.0.
Raw ABI calls through _lib.launch.

A property of the INPUTS (seeds and values chosen for it, asserted on the host in every test): the same terms added one after
the other in index order give other bits than the replay -- a different float64 for the IoU sums, a different float32 for the
point-mesh loss -- so a kernel that summed in that order, and a test that compared against it, would not pass here."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE, BLOCK = 64, 256
TW, TH = 64, 16  # nr_image_losses.hip's tile


def workgroup_sum(terms):
    """The sum of one float64 per thread, terms [BLOCK], in the contract's order: butterfly, then the waves from wave 0's."""
    v = np.asarray(terms, dtype=np.float64).reshape(BLOCK // WAVE, WAVE).copy()
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    assert (v.view(np.uint64) == v[:, :1].view(np.uint64)).all()  # every lane ends with the same bits
    s = v[0, 0]
    for w in range(1, BLOCK // WAVE):
        s = s + v[w, 0]
    return s


def sequential_sum(terms):
    """terms added to 0.0 one after the other in index order (float64)"""
    s = np.float64(0.0)
    for x in np.asarray(terms, dtype=np.float64).ravel():
        s = s + x
    return s


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(u) == b.view(u)).all())


# ----------------------------------------------------------------------------------------------------------------------
# IoU sums

def iou_terms(a, t):
    """per pixel in float64: p = a t (for I) and (a + t) - p (for U)"""
    da, dt = a.astype(np.float64), t.astype(np.float64)
    p = da * dt
    return p, (da + dt) - p


def iou_replay(alpha, target):
    """sums [B, 2] of nr_iou_loss_forward at levels = 1 (nr_image_losses.hip's head): tiles of 64 x 16 row-major, one
    workgroup each; thread (tid % 16, tid / 16) adds its four pixels left to right into I and U from 0.0, a pixel outside the
    image as a = t = 0, exactly 0; the workgroup's sum; the tiles in tile order from 0.0."""
    B, H, W = alpha.shape
    rows, cols = (H + TH - 1) // TH, (W + TW - 1) // TW
    pa = np.zeros((B, rows * TH, cols * TW), dtype=np.float32)
    pt = np.zeros_like(pa)
    pa[:, :H, :W] = alpha
    pt[:, :H, :W] = target
    out = np.zeros((B, 2), dtype=np.float64)
    for b in range(B):
        I, U = np.float64(0.0), np.float64(0.0)
        for r in range(rows):
            for c in range(cols):
                # [ty, tx, j]: thread tid = 16 ty + tx holds pixels 4 tx + j of row ty
                ta = pa[b, r * TH:(r + 1) * TH, c * TW:(c + 1) * TW].reshape(TH, 16, 4)
                tt = pt[b, r * TH:(r + 1) * TH, c * TW:(c + 1) * TW].reshape(TH, 16, 4)
                p, q = iou_terms(ta, tt)
                ti, tu = np.zeros((TH, 16)), np.zeros((TH, 16))
                for j in range(4):
                    ti = ti + p[:, :, j]
                    tu = tu + q[:, :, j]
                I = I + workgroup_sum(ti.ravel())
                U = U + workgroup_sum(tu.ravel())
        out[b] = I, U
    return out


@pytest.mark.parametrize('H,W', [(24, 80), (16, 64)])
def test_iou_sums_follow_the_order(H, W):
    """B = 2.  24 x 80: 2 x 2 tiles, the right column 16 pixels wide and the bottom row 8 rows high -- workgroups with empty
    threads and empty waves, several tiles per image.  16 x 64: one tile, exactly full.  `sums` equals the replay bit for
    bit; the terms in row-major pixel order from 0.0 give other bits in every entry (a property of this seed's inputs)."""
    import torch
    from neural_renderer_amd import _lib
    B = 2
    rng = np.random.default_rng(20261021)
    alpha = rng.random((B, H, W), dtype=np.float32)
    target = rng.random((B, H, W), dtype=np.float32)
    want = iou_replay(alpha, target)
    p, q = iou_terms(alpha, target)
    seq = np.array([[sequential_sum(p[b]), sequential_sum(q[b])] for b in range(B)])
    assert (seq != want).all(), 'the inputs do not tell the orders apart'
    a, t = torch.from_numpy(alpha).cuda(), torch.from_numpy(target).cuda()
    dev = a.device
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    sums = torch.empty((B, 2), dtype=torch.float64, device=dev)
    weights = (ctypes.c_double * 5)(1.0, 0.0, 0.0, 0.0, 0.0)
    _lib.launch('nr_iou_loss_forward', dev, a.data_ptr(), t.data_ptr(), 1, weights, loss.data_ptr(), sums.data_ptr(), B, H, W,
                1, 1e-6, workspace_bytes=_lib.workspace_bytes('nr_image_loss_workspace_bytes', B, H, W, 1))
    got = sums.cpu().numpy()
    print('I, U: kernel %r replay %r sequential %r' % (got.tolist(), want.tolist(), seq.tolist()))
    assert same_bits(got, want)


# ----------------------------------------------------------------------------------------------------------------------
# point-mesh loss

def signed_powers(rng, n, top=60):
    """n float32 values +-2^e, e in -20 .. top; the first half's negatives are shuffled into the second half, so the exact sum
    is small next to the terms and the float32 result shows which low bits the double additions lost on the way."""
    v = rng.choice([-1.0, 1.0], size=n) * np.exp2(rng.integers(-20, top + 1, size=n))
    h = n // 2
    v[h:2 * h] = -v[:h][rng.permutation(h)]
    return v.astype(np.float32)


def strided_replay(d):
    """nr_point_mesh.hip's k_loss for one image: thread t adds elements t, t + 256, .. in index order from 0.0, then the
    workgroup's sum"""
    terms = np.zeros(BLOCK, dtype=np.float64)
    for i, x in enumerate(d.astype(np.float64)):
        terms[i % BLOCK] = terms[i % BLOCK] + x
    return workgroup_sum(terms)


def weighted(sp, sf, wp, wf):
    """wp sum_p alone, wf sum_f alone, or wp sum_p + wf sum_f, in double, rounded once"""
    if sf is None:
        return np.float32(np.float64(wp) * sp)
    if sp is None:
        return np.float32(np.float64(wf) * sf)
    return np.float32(np.float64(wp) * sp + np.float64(wf) * sf)


@pytest.mark.parametrize('which', ['points', 'faces', 'both'])
@pytest.mark.parametrize('N', [1, 300])
def test_point_mesh_loss_follows_the_order(N, which):
    """B = 2, F = 70, arrays given directly.  `loss` equals the replay bit for bit.  The same terms in index order from 0.0
    give another float32 for every image (a property of this seed's values) -- except for N = 1 points only, a sum of one
    term, which has one order.  (The one point of N = 1 is at most 1, or it would hide the faces' sum behind it in 'both'.)"""
    import torch
    from neural_renderer_amd import _lib
    B, F, wp, wf = 2, 70, 0.75, 1.5
    rng = np.random.default_rng(6)
    df = np.stack([signed_powers(rng, F) for _ in range(B)])  # (both drawn in every case: the same values in all of them)
    dp = np.stack([signed_powers(rng, N, 60 if N > 1 else 0) for _ in range(B)])
    dp, df = (dp if which != 'faces' else None), (df if which != 'points' else None)
    want = np.array([weighted(None if dp is None else strided_replay(dp[b]), None if df is None else strided_replay(df[b]),
                              wp, wf) for b in range(B)], dtype=np.float32)
    seq = np.array([weighted(None if dp is None else sequential_sum(dp[b]), None if df is None else sequential_sum(df[b]),
                             wp, wf) for b in range(B)], dtype=np.float32)
    assert np.isfinite(want).all()
    if not (N == 1 and which == 'points'):
        assert (seq != want).all(), 'the inputs do not tell the orders apart'
    tp = None if dp is None else torch.from_numpy(dp).cuda()
    tf = None if df is None else torch.from_numpy(df).cuda()
    loss = torch.empty((B,), dtype=torch.float32, device='cuda')
    dev = loss.device
    _lib.launch('nr_point_mesh_loss', dev, _lib.ptr(tp), _lib.ptr(tf), loss.data_ptr(), B, N, F, wp, wf)
    got = loss.cpu().numpy()
    print('loss: kernel %r replay %r sequential %r' % (got.tolist(), want.tolist(), seq.tolist()))
    assert same_bits(got, want)
