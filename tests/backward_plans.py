"""The fused backward's launch plans as data (no test in here): which plan a call takes, read without a launch through the
measurement build's nr_profile_backward_plan (include/nr_hip_profile.h -- the planning function the launch path runs, no copy of
its rules), a bounded grid of calls that straddles the thresholds of that function (all but two: see GRID), and CASES: for every distinct plan of the
grid its cheapest call with a scene to run it on (tests/golden/backward_plan_cases.json, written by
scripts/make_backward_plan_cases.py and committed: a changed rule shows as a failing comparison in test_backward_plans.py,
not as a silently different table).

A call is a dict: B, F, S, ts, modes = (grad_rgb, grad_alpha, grad_depth given), flags, eps, lit (per-face light colours on
F / 2 original cubes with their gradient asked for -- the Renderer's fill_back layout), mis (grad_textures one float off the
16-byte grid), visible (the forward's per-face flags are passed), ws (workspace bytes; 0: what the library asks for)."""
import ctypes
import itertools
import json
import os

import numpy as np

from neural_renderer_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_PATH = os.path.join(HERE, 'golden', 'backward_plan_cases.json')
SECONDS_PATH = os.path.join(HERE, 'golden', 'backward_plan_oracle_seconds.json')

EXACT, SERIAL = _lib.NR_FLAG_EXACT_GRADIENT, _lib.NR_FLAG_SERIAL_BACKWARD
BIG_PX = 2048  # nr_face_gather.h: candidate sets above this are k_backward_big's

# include/nr_hip_profile.h, in the hook's order: the discrete fields (the signature), then the sizes the thresholds compare
FIELDS = ('k6', 'kernel', 'use_records', 'overflow_pass', 'row_chunked', 'threads', 'bands', 'face_zeros', 'gather_first',
          'gather_in_tail', 'setup_alone', 'setup_in_gather', 'tex_zeros', 'light_fill', 'gather', 'listed', 'static_taps', 'lanes',
          'depth_in_gather', 'big', 'big_overflow', 'finish', 'depth', 'fill_faces', 'depth_lists')
SIZES = ('tex_bytes', 'gather_lds', 'fast_lds', 'row_lds', 'fill_max', 'W_fast', 'W_row', 'W', 'n_bands', 'setup_lds')
assert len(FIELDS) + len(SIZES) == _lib.NR_PLAN_FIELDS
# the enumerations of nr_device.h
FACE_ZEROS_NONE, FACE_ZEROS_UNLISTED, FACE_ZEROS_ALL = 0, 1, 2
TEX_ZEROS_NONE, TEX_ZEROS_BAND, TEX_ZEROS_SETUP, TEX_ZEROS_FILL, TEX_ZEROS_BAND_UNLISTED = 0, 1, 2, 3, 4
FINISH_NONE, FINISH_KERNEL, FINISH_GATHER, FINISH_BIG, FINISH_ADD = 0, 1, 2, 3, 4
GATHER_NONE, GATHER_FACE, GATHER_ATOMIC = 0, 1, 2
KERNEL_FAST, KERNEL_ROW, KERNEL_GLOBAL = 0, 1, 2

ALL_MODES = ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))

# The grid: every combination of these, within grid_calls' bounds.  Texture sizes on both sides of 2 | 5 | 8 | 13 and of the 40 KB
# of gather LDS (5, 8, 12 above; 6, 9 below); batch x faces on both sides of 98 304 (2049 x 48, 14 000 x 8 above); rasters on both
# sides of 400, 512 and 1024, and 1366 for the far side of the 32 768 bytes of line-setup LDS (1366 bands: 32 784); fill_max on
# both sides (330 cubes of texture size 8 beside a band kernel of one image of 8 x 8).  48: the smallest raster with room for
# a face above BIG_PX.
# NOT in the grid, because S >= 8 and B F S^2 <= MAX_WORK allow no more than 625 000 faces: a call above 655 360 faces (the
# largest here has 112 000; such a call takes the plan of a serial-order call: neither early order) -- and 2^15 faces on a
# raster above 512 (8.6e9).  Those two thresholds are straddled by test_backward_plans.py's host-only pairs alone.
GRID = dict(B=(1, 2, 3, 16, 64, 2049, 14000), F=(2, 8, 48, 330), S=(8, 16, 33, 48, 64, 400, 401, 512, 513, 600, 1024, 1056, 1366),
            ts=(2, 3, 5, 6, 8, 9, 12, 13, 14), modes=ALL_MODES, flags=(0, EXACT, SERIAL), eps=(1e-3, 0.0, 1e-10), lit=(0, 1),
            mis=(0, 1), visible=(1, 0))
MAX_WORK = 4e7  # B F S^2 of a grid call

_hook = None
_out = (ctypes.c_int64 * _lib.NR_PLAN_FIELDS)()


def hook():
    """nr_profile_backward_plan of the measurement build -- or of the library NR_HIP_LIB names, when that one has it (a
    development variant built with NR_PROFILE_HOOK=1: a changed threshold must fail test_backward_plans.py)."""
    global _hook
    if _hook is None:
        name = 'nr_profile_backward_plan'
        lib = None
        if os.environ.get('NR_HIP_LIB'):
            cand = ctypes.CDLL(os.environ['NR_HIP_LIB'])
            if hasattr(cand, name):
                lib = cand
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = _lib.PROFILE_SIGNATURES[name]
        if lib is None:
            lib = _lib.load_profile()
        _hook = getattr(lib, name)
    return _hook


def call(B, F, S, ts=2, modes=(1, 1, 1), flags=0, eps=1e-3, lit=0, mis=0, visible=1, ws=0):
    return dict(B=B, F=F, S=S, ts=ts, modes=tuple(modes), flags=flags, eps=eps, lit=lit, mis=mis, visible=visible, ws=ws)


def _raw(c):
    m = c['modes']
    return hook()(c['B'], c['F'], c['S'], c['ts'], m[0], m[1], m[2], c['eps'], c['flags'], c['F'] // 2 if c['lit'] else 0,
                  1 if c['lit'] else 0, (4 if c['mis'] else 0) if m[0] else -1, c['visible'], c['ws'], _out)


def plan(c):
    """Every field of the call's plan by name; raises on a call that plan_backward refuses."""
    e = _raw(c)
    if e:
        raise ValueError('plan_backward refuses %r: %d' % (c, e))
    return dict(zip(FIELDS + SIZES, _out))


def signature(c):
    """The plan's discrete fields (FIELDS), or None for a call that plan_backward refuses."""
    return None if _raw(c) else tuple(_out[:len(FIELDS)])


def named(sig):
    return dict(zip(FIELDS, sig))


def cost(c):
    return c['B'] * c['F'] * c['S'] ** 2 + 3 * c['B'] * c['F'] * c['ts'] ** 3


def grid_calls():
    """The calls of GRID: B F S^2 <= MAX_WORK; light colours and a misaligned grad_textures only where there is a texture
    gradient, one texture size without; per-face light needs an even F; visible_faces left out only where the plan can depend on it
    (a depth-only call)."""
    g = GRID
    for B, F, S in itertools.product(g['B'], g['F'], g['S']):
        if B * F * S * S > MAX_WORK:
            continue
        for ts, modes, flags, eps, lit, mis, visible in itertools.product(g['ts'], g['modes'], g['flags'], g['eps'], g['lit'],
                                                                          g['mis'], g['visible']):
            if not modes[0] and (lit or mis or ts != 2):
                continue
            if lit and F % 2:
                continue
            if not visible and modes != (0, 0, 1):
                continue
            yield call(B, F, S, ts, modes, flags, eps, lit, mis, visible)


def grid_signatures():
    """signature -> cheapest grid call, over the whole grid (a few seconds of host time)."""
    best = {}
    for c in grid_calls():
        s = signature(c)
        if s is None:
            continue
        k = cost(c)
        if s not in best or k < best[s][0]:
            best[s] = (k, c)
    return {s: c for s, (k, c) in best.items()}


def _load_cases():
    with open(CASES_PATH) as f:
        cases = json.load(f)
    for c in cases:
        c['call']['modes'] = tuple(c['call']['modes'])
        c['signature'] = tuple(c.get('signature', ()))  # (a table without them fails the tests' comparisons)
    return cases


# [{'call': call, 'signature': the plan's discrete fields when the table was written, 'scene': {'seed', 'spread', 'size',
# 'backdrop', 'overflow'}}], one per signature of the grid
CASES = _load_cases()


def case_id(case):
    c = case['call']
    return 'B%d-F%d-S%d-ts%d-m%d%d%d-f%d-e%g%s%s%s%s%s' % (
        c['B'], c['F'], c['S'], c['ts'], c['modes'][0], c['modes'][1], c['modes'][2], c['flags'], c['eps'], '-lit' if c['lit'] else '',
        '-mis' if c['mis'] else '', '' if c['visible'] else '-novis', '-backdrop' if case['scene']['backdrop'] else '',
        '-overflow' if case['scene']['overflow'] else '')


# ------------------------------------------------------------------------------------------------------------------------
# scenes

BACKDROP = np.array([[-1.2, -1.1, 50.0], [1.2, -1.1, 50.0], [0.0, 1.2, 50.0]], np.float32)


def scene(case):
    """(faces [B, F, 3, 3], textures [B, F, ts^3, 3] or None) of a case: helpers.random_scene by the recipe; `overflow`: every
    third image takes faces that span most of the raster (their line records exceed the line buffer); `backdrop`: face 0 of
    every image is one large triangle behind the others.  With per-face light colours the second half of the faces is the first
    half reversed (fill_back) and the textures are the F / 2 original cubes."""
    import helpers as H
    c, s = case['call'], case['scene']
    B, F, ts = c['B'], c['F'], c['ts']
    rng = np.random.default_rng(s['seed'])
    n = F // 2 if c['lit'] else F
    faces = H.random_scene(rng, B, n, spread=s['spread'], size=s['size'])
    if s['overflow']:
        faces[::3] = H.random_scene(rng, B, n, spread=0.4, size=1.2)[::3]
    if s['backdrop']:
        faces[:, 0] = BACKDROP
    if c['lit']:
        faces = np.ascontiguousarray(np.concatenate((faces, faces[:, :, ::-1]), axis=1))
    textures = rng.uniform(0, 1, (B, n, ts, ts, ts, 3)).astype(np.float32) if c['modes'][0] else None
    return faces, textures


def light_colors(case):
    """[B, F, 3] light colours of a case with per-face light"""
    c = case['call']
    return np.random.default_rng(case['scene']['seed'] + 77).uniform(0.2, 1.5, (c['B'], c['F'], 3)).astype(np.float32)


def oracle_textures(case, textures):
    """The textures the oracle (and the lit-texture call) takes: the cubes themselves, or -- per-face light colours -- the cubes
    duplicated for the reversed faces (axes 0 and 2 exchanged, renderer.py:79) and multiplied by the colours (lighting.py:50-51)."""
    if not case['call']['lit']:
        return textures
    t_all = np.concatenate((textures, textures.transpose((0, 1, 4, 3, 2, 5))), axis=1)
    return np.ascontiguousarray((t_all * light_colors(case)[:, :, None, None, None, :]).astype(np.float32))


ATOMIC_TERMS = 2  # a float sum of up to two atomically added terms onto a zero is the same in any order


def terms_per_texel(case):
    """The largest number of terms that one element of grad_textures receives (the oracle's K7 count, Nt).  Cases whose K7 is
    the per-pixel scatter with float atomics keep it at ATOMIC_TERMS or below: the GPU test compares grad_textures bit for bit
    between two launch orders, and a float sum of three or more atomically added terms has no defined order (two runs of ONE
    order differ), while 0 + a is exact and a + b commutes."""
    from oracle import oracle as O
    c = case['call']
    faces, cubes = scene(case)
    fn = O.Rasterize(c['S'], 0.1, 100.0, c['eps'], (0.1, 0.2, 0.3), True, bool(c['modes'][1]), bool(c['modes'][2]))
    fn(faces, oracle_textures(case, cubes))
    return int(fn.backward(*upstream(case), magnitudes=True)[-1]['Nt'].max())


def oracle_seconds(cases):
    """{case id: seconds} of the oracle's work on each case -- the forward and the three backward runs that the GPU test makes
    of it -- behind one untimed warm-up (the library's first call starts its threads); a case above a second is timed twice
    and the shorter time counts."""
    import time
    from oracle import oracle as O

    def once(case):
        c = case['call']
        faces, cubes = scene(case)
        rgb, alpha, depth = [bool(m) for m in c['modes']]
        g = upstream(case)
        t0 = time.perf_counter()
        fn = O.Rasterize(c['S'], 0.1, 100.0, c['eps'], (0.1, 0.2, 0.3), rgb, alpha, depth)
        fn(faces, oracle_textures(case, cubes)) if rgb else fn(faces)
        fn.backward(*g, accumulate_double=True, magnitudes=True)
        fn.backward(*g)
        fn.backward(g[0], g[1], None if g[2] is None else np.zeros_like(g[2]), accumulate_double=True)
        return time.perf_counter() - t0, fn
    out, fns = {}, {}
    for m in ALL_MODES:
        once(dict(call=call(1, 2, 8, 2, m), scene=dict(seed=0, spread=0.6, size=0.25, backdrop=False, overflow=False)))
    for case in cases:
        t, fn = once(case)
        if t > 1.0:
            t = min(t, once(case)[0])
        out[case_id(case)], fns[case_id(case)] = round(t, 3), fn
    return out, fns


def write_oracle_seconds(seconds):
    slow = sorted(seconds.items(), key=lambda kv: -kv[1])[:5]
    with open(SECONDS_PATH, 'w') as f:
        json.dump(dict(total=round(sum(seconds.values()), 1), slowest=dict(slow), cases=len(seconds)), f, indent=1, sort_keys=True)
        f.write('\n')


def upstream(case):
    c = case['call']
    B, S = c['B'], c['S']
    rng = np.random.default_rng(case['scene']['seed'] + 1000003)
    m = c['modes']
    return (rng.normal(size=(B, S, S, 3)).astype(np.float32) if m[0] else None,
            rng.normal(size=(B, S, S)).astype(np.float32) if m[1] else None,
            rng.normal(size=(B, S, S)).astype(np.float32) if m[2] else None)


def line_records(faces, face_index_map, S):
    """Per image the line records of its visible faces, counted as tests/test_backward_tail_order_gpu.py does: one per visible
    face, edge, axis and integer line inside the edge's extent."""
    out = []
    for b in range(faces.shape[0]):
        fi = face_index_map[b]
        vis = np.unique(fi[fi >= 0])
        p = (faces[b, vis, :, :2].astype(np.float64) * S + S - 1) / 2
        n = 0
        for e in range(3):
            for ax in range(2):
                lo = np.maximum(np.ceil(np.minimum(p[:, e, ax], p[:, (e + 1) % 3, ax])), 0)
                hi = np.minimum(np.floor(np.maximum(p[:, e, ax], p[:, (e + 1) % 3, ax])), S - 1)
                n += int(np.maximum(hi - lo + 1, 0).sum())
        out.append(n)
    return np.array(out)


def line_capacity(F, S):
    return 8 * F + 32 * S + int(1.2 * S * np.sqrt(F))


def scene_facts(case, faces, face_index_map):
    """What test_backward_plans.py asserts of a case's scene, from the oracle's forward: (covered pixels, uncovered pixels,
    listed faces, unlisted faces, backdrop holds, overflow holds)."""
    c, s = case['call'], case['scene']
    B, F, S = c['B'], c['F'], c['S']
    fi = face_index_map
    covered = int((fi >= 0).sum())
    owners = np.unique((fi + np.arange(B)[:, None, None] * F)[fi >= 0])
    backdrop = overflow = True
    if s['backdrop']:
        # the candidate set is the face's pixel box clipped to the raster (face_candidates, nr_device.h)
        p = (BACKDROP[:, :2].astype(np.float64) * S + S - 1) / 2
        lo, hi = np.clip(np.ceil(p.min(axis=0)), 0, S - 1), np.clip(np.floor(p.max(axis=0)), 0, S - 1)
        box = int((hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1))
        own = (fi == 0).sum(axis=(1, 2))
        backdrop = box > BIG_PX and int(own.min()) > box // 2
    if s['overflow']:
        rec, cap = line_records(faces, fi, S), line_capacity(F, S)
        rest = np.delete(rec, np.s_[::3])
        overflow = bool(rec[::3].min() > cap and (rest.size == 0 or rest.max() < cap))
    return covered, B * S * S - covered, len(owners), B * F - len(owners), backdrop, overflow
