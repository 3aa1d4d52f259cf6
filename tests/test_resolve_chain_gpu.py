"""The forward's resolve pass requests a covered pixel's loads in groups (nr_forward.hip: resolve_pixel, sum_taps, the static
taps of texture size 2).  Nothing of that may change a bit: every path of it against the staged pass and the CPU oracle, with
taps outside the cube, both settings of quirk Q1, both kinds of background, per-face light colours and unaligned cubes."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import abi
import helpers as H
import neural_renderer_amd as nr
from neural_renderer_amd import _lib

pytestmark = pytest.mark.gpu

FIX = _lib.NR_FLAG_FIX_TEXTURE_BATCH_Z
NR_E_SIZE = -2


def fused(faces, textures, S, eps, bg, flags=0, epoch=False, z_ref=None, light=None, tex_faces=0, raw=False):
    """nr_forward_rasterize_lit on device tensors (`textures` is taken as it is: its data pointer is the caller's business).
    epoch: a kept workspace in epoch mode, the way the operator calls (k_resolve_quads on aligned maps of an even raster)."""
    lib = _lib.load()
    f = abi.dev(faces, torch.float32)
    B, F = f.shape[:2]
    ts = int(textures.shape[2])
    zr = abi.dev(z_ref, torch.float32) if z_ref is not None else None
    bgt = abi.dev(np.asarray(bg, np.float32))
    lt = abi.dev(light, torch.float32) if light is not None else None
    lit = _lib.FaceLight(lt.data_ptr(), tex_faces, None, None) if lt is not None else None
    out = {'face_index_map': torch.full((B, S, S), 12345, dtype=torch.int32, device='cuda'),
           'weight_map': torch.full((B, S, S, 3), float('nan'), device='cuda'),
           'depth_map': torch.full((B, S, S), float('nan'), device='cuda'),
           'rgb_map': torch.full((B, S, S, 3), float('nan'), device='cuda'),
           'alpha_map': torch.full((B, S, S), float('nan'), device='cuda'),
           'visible_faces': torch.full((B, F), 77, dtype=torch.uint8, device='cuda')}
    wsb = lib.nr_forward_workspace_bytes(B, F, S)
    ws = torch.full((wsb,), 255, dtype=torch.uint8, device='cuda')
    if epoch:
        flags |= _lib.NR_FLAG_ZBUF_EPOCH | (254 << 8)
    code = lib.nr_forward_rasterize_lit(
        lit, f.data_ptr(), _lib.ptr(zr), textures.data_ptr(), out['face_index_map'].data_ptr(), out['weight_map'].data_ptr(),
        out['depth_map'].data_ptr(), out['rgb_map'].data_ptr(), out['alpha_map'].data_ptr(), out['visible_faces'].data_ptr(),
        bgt.data_ptr(), int(bgt.dim() == 2), B, F, S, ts, 0.1, 100.0, eps, flags, ws.data_ptr(), wsb,
        torch.cuda.current_stream().cuda_stream)
    if raw:
        return code
    _lib.check(code, 'nr_forward_rasterize_lit')
    torch.cuda.synchronize()
    return {k: abi.host(v) for k, v in out.items()}


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint8), b.view(np.uint32 if b.itemsize == 4 else np.uint8)), what


# ------------------------------------------------------------------------------------------------------------------------
# Taps outside the cube
def corner_scene(S, lo, hi):
    """A triangle with its vertices on the pixel centres (lo, lo), (hi, lo), (lo, hi) and depths (2, 2, 4), its reversed copy
    and a degenerate face.  At a vertex a perspective-corrected weight is exactly 1, so with texture size 2 and an eps that
    float32 does not resolve an index float reaches 1.0 and the upper taps of that axis fall outside the cube, with weight 0."""
    c = lambda p: (2.0 * p + 1 - S) / S
    tri = np.array([[c(lo), c(lo), 2], [c(hi), c(lo), 2], [c(lo), c(hi), 4]], np.float32)
    return np.stack([tri, tri[::-1].copy(), np.zeros((3, 3), np.float32)])[None]


def rebuilt_rgb(fn, textures, bg):
    """rgb from the oracle's two sampling maps in float32, in tap order, a tap outside the cube skipped."""
    fi, si, sw = fn.face_index_map, fn.sampling_index_map, fn.sampling_weight_map
    B, S = fi.shape[:2]
    T = textures.shape[2] ** 3
    tex = textures.reshape(B, -1, T, 3)
    bg = np.asarray(bg, np.float32)
    out = np.empty((B, S, S, 3), np.float32)
    out[...] = np.float32(0) * np.float32(0) + np.float32(1) * bg
    for b, y, x in zip(*np.nonzero(fi >= 0)):
        acc = np.zeros(3, np.float32)
        for pn in range(8):
            if si[b, y, x, pn] < T:
                acc = acc + sw[b, y, x, pn] * tex[b, fi[b, y, x], si[b, y, x, pn]]
        out[b, y, x] = acc * np.float32(1) + np.float32(0) * bg
    return out


# (raster, first and last vertex pixel, covered pixels, taps with index >= 8 at eps 0 and 1e-9 / at 1e-3: counted with
# oracle.Rasterize on the CPU)
CORNER_CASES = [(8, 1, 6, 21, 7, 0), (9, 1, 7, 28, 7, 0)]


@pytest.mark.parametrize('eps', [0.0, 1e-9, 1e-3])
@pytest.mark.parametrize('S,lo,hi,covered,outside,outside_eps', CORNER_CASES)
def test_taps_outside_the_cube(S, lo, hi, covered, outside, outside_eps, eps):
    faces = corner_scene(S, lo, hi)
    rng = np.random.default_rng(11)
    textures = rng.uniform(0.1, 1, (1, 3, 2, 2, 2, 3)).astype(np.float32)
    bg = (0.25, 0.5, 0.75)
    fn = O.Rasterize(S, 0.1, 100, eps, bg, True, True, True)
    fn(faces, textures)
    hit = fn.face_index_map >= 0
    assert int(hit.sum()) == covered
    assert int((fn.sampling_index_map[hit] >= 8).sum()) == (outside_eps if eps == 1e-3 else outside)
    owner = int(fn.face_index_map[hit][0])
    assert (fn.face_index_map[hit] == owner).all() and owner < 2  # (not the last face: a cube follows the owner's in memory)
    rebuilt = rebuilt_rgb(fn, textures, bg)
    poisoned = textures.copy()
    poisoned[0, owner + 1] = np.nan

    def runs(tex):
        t = abi.dev(tex, torch.float32)
        got = [fused(faces, t, S, eps, bg)['rgb_map']]                                           # k_resolve, per-call fill
        if S % 2 == 0:
            got.append(fused(faces, t, S, eps, bg, epoch=True)['rgb_map'])                       # k_resolve_quads
            rgb, _, _ = nr.Rasterize(S, 0.1, 100, eps, bg, True, True, True)(
                torch.tensor(faces, device='cuda'), t)                                          # the operator (epoch mode)
            got.append(rgb.cpu().numpy())
        got.append(abi.host(abi.forward(faces, tex, S, 0.1, 100.0, eps, bg, 0, True, True, True)['rgb_map']))  # staged: k_shade
        return got

    clean = runs(textures)
    for k, rgb in enumerate(clean):
        same_bits(rgb, fn.rgb_map, 'oracle, path %d' % k)
        same_bits(rgb, rebuilt, 'sampling maps, path %d' % k)
    for k, rgb in enumerate(runs(poisoned)):
        same_bits(rgb, clean[k], 'NaN cube behind the owner, path %d' % k)


# ------------------------------------------------------------------------------------------------------------------------
# Every path against the staged pass and the oracle
def scene3(ts, S):
    rng = np.random.default_rng(100 * ts + S)
    faces = H.random_scene(rng, 3, 24, spread=0.5, size=0.4)
    textures = rng.uniform(0, 1, (3, 24, ts, ts, ts, 3)).astype(np.float32)
    bgs = rng.uniform(0, 1, (3, 3)).astype(np.float32)
    return faces, textures, bgs


_oracle_cache = {}


def oracle3(ts, S, fix, per_image):
    key = (ts, S, fix, per_image)
    if key not in _oracle_cache:
        faces, textures, bgs = scene3(ts, S)
        fn = O.Rasterize(S, 0.1, 100, 1e-3, bgs if per_image else tuple(bgs[0]), True, True, True, fix)
        fn(faces, textures)
        _oracle_cache[key] = fn
    return _oracle_cache[key]


@pytest.mark.parametrize('S', [16, 15])
@pytest.mark.parametrize('ts', [1, 2, 3, 4])
def test_every_path_equals_the_staged_pass_and_the_oracle(ts, S):
    """Texture sizes 2 (static taps where the cubes allow), 3 and 4 (sum_taps); rasters 16 (k_resolve_quads in epoch mode) and
    15 (k_resolve); quirk Q1 both ways, on the batch's own first image and on `faces_z_ref` (images 1 and 2 of the batch as a
    call of their own); the background shared and per image.  Texture size 1 has no trilinear cell: the entry points refuse it
    (include/nr_hip.h, rasterize.py:78-90), which is all there is to check."""
    if ts == 1:
        faces, _, bgs = scene3(2, S)
        t1 = torch.zeros((3, 24, 1, 1, 1, 3), device='cuda')
        assert fused(faces, t1, S, 1e-3, bgs[0], raw=True) == NR_E_SIZE
        assert fused(faces, t1, S, 1e-3, bgs[0], epoch=True, raw=True) == NR_E_SIZE
        return
    faces, textures, bgs = scene3(ts, S)
    for fix in (False, True):
        for per_image in (False, True):
            fn = oracle3(ts, S, fix, per_image)
            assert (fn.face_index_map >= 0).any(axis=(1, 2)).all()
            flags = FIX if fix else 0
            for sub in (slice(0, 3), slice(1, 3)):  # the whole batch / two images with faces_z_ref
                z_ref = faces[:1] if sub.start else None
                bg = bgs[sub] if per_image else bgs[0]
                what = 'ts %d S %d fix %d per-image bg %d z_ref %d' % (ts, S, fix, per_image, sub.start)
                staged = abi.forward(faces[sub], textures[sub], S, 0.1, 100.0, 1e-3, bg, flags, True, True, True,
                                     want_sampling=True, faces_z_ref=z_ref)
                same_bits(abi.host(staged['rgb_map']), fn.rgb_map[sub], 'staged rgb, ' + what)
                same_bits(abi.host(staged['sampling_index_map']), fn.sampling_index_map[sub], 'sampling_index_map, ' + what)
                same_bits(abi.host(staged['sampling_weight_map']), fn.sampling_weight_map[sub], 'sampling_weight_map, ' + what)
                t = abi.dev(textures[sub], torch.float32)
                for epoch in (False, True):
                    fw = fused(faces[sub], t, S, 1e-3, bg, flags, epoch, z_ref)
                    same_bits(fw['rgb_map'], fn.rgb_map[sub], 'fused rgb, epoch %d, ' % epoch + what)
                    same_bits(fw['face_index_map'], fn.face_index_map[sub], 'face_index_map, ' + what)
                    same_bits(fw['depth_map'], fn.depth_map[sub], 'depth_map, ' + what)
                    same_bits(fw['weight_map'], fn.weight_map[sub], 'weight_map, ' + what)
                    same_bits(fw['alpha_map'], fn.alpha_map[sub], 'alpha_map, ' + what)


@pytest.mark.parametrize('S', [16, 15])
@pytest.mark.parametrize('ts', [2, 3])
def test_per_face_light_with_a_reversed_copy(ts, S):
    """nr_forward_rasterize_lit: the cubes of the original faces, read transposed by the reversed copies (which own pixels
    here), times one light colour per face.  The oracle samples the duplicated, transposed cubes (renderer.py:79); the light
    factor is one float32 product on top of its sample."""
    rng = np.random.default_rng(7 * ts + S)
    B, Nf = 2, 12
    front = H.random_scene(rng, B, Nf, spread=0.5, size=0.4)
    faces = np.concatenate([front, front[:, :, ::-1]], axis=1).copy()
    textures = rng.uniform(0.1, 1, (B, Nf, ts, ts, ts, 3)).astype(np.float32)
    light = rng.uniform(0.2, 1, (B, 2 * Nf, 3)).astype(np.float32)
    bg = (0.2, 0.4, 0.6)
    fn = O.Rasterize(S, 0.1, 100, 1e-3, bg, True, True, True, True)
    fn(faces, np.concatenate([textures, textures.transpose(0, 1, 4, 3, 2, 5)], axis=1))
    hit = fn.face_index_map >= 0
    assert (fn.face_index_map[hit] >= Nf).any() and (fn.face_index_map[hit] < Nf).any()
    want = fn.rgb_map.copy()
    b_of = np.nonzero(hit)[0]
    want[hit] = (fn.rgb_map[hit] * light[b_of, fn.face_index_map[hit]]) * np.float32(1) + np.float32(0) * np.asarray(bg, np.float32)
    t = abi.dev(textures, torch.float32)
    for epoch in (False, True):
        fw = fused(faces, t, S, 1e-3, bg, FIX, epoch, light=light, tex_faces=Nf)
        same_bits(fw['face_index_map'], fn.face_index_map, 'face_index_map')
        same_bits(fw['rgb_map'], want, 'lit rgb, epoch %d' % epoch)


def test_unaligned_cubes():
    """Texture size 2 with `textures` 4 bytes past a 16-byte boundary: the 16-byte loads of the static-tap path cannot read
    them, the pass takes the tap loads, and the bits are those of the aligned call."""
    faces, textures, bgs = scene3(2, 16)
    aligned = abi.dev(textures, torch.float32)
    flat = torch.empty(aligned.numel() + 1, device='cuda')
    shifted = flat[1:].view(aligned.shape)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for epoch in (True, False):
        a = fused(faces, aligned, 16, 1e-3, bgs[0], 0, epoch)
        b = fused(faces, shifted, 16, 1e-3, bgs[0], 0, epoch)
        for k in a:
            same_bits(a[k], b[k], '%s, epoch %d' % (k, epoch))
    same_bits(a['rgb_map'], oracle3(2, 16, False, False).rgb_map, 'oracle')

