"""The fused backward's launch plans, on the host (no device): plan_backward (csrc/nr_backward.hip) decides every launch of a call
before the first one goes out, as a pure function of the call, and turns on thresholds that a suite's shapes must be chosen to
straddle.  Read through the measurement build's nr_profile_backward_plan (the planning function of the launch path itself):

  * the committed table of cases (backward_plans.CASES, run on the GPU by test_backward_plans_gpu.py) holds exactly the plans
    that the grid of calls reaches -- none missing, none stale;
  * the plan's invariants, as BackwardPlan's comments state them, over the whole grid;
  * every threshold separates a pair of calls that differ only across it;
  * every case's scene has what its plan needs to go wrong visibly (oracle's forward).
"""
import json

import numpy as np
import pytest

import backward_plans as P
from neural_renderer_amd import _build
from oracle import oracle as O

T = 4928  # the teapot's faces with fill_back


@pytest.fixture(scope='module', autouse=True)
def profile_lib():
    _build.build_profile()
    return P.hook()


@pytest.fixture(scope='module')
def grid():
    """[(call, every field of its plan)] over the whole grid"""
    out = []
    for c in P.grid_calls():
        if P.signature(c) is not None:
            out.append((c, P.plan(c)))
    return out


def test_cases_cover_the_grid_both_ways(grid):
    of_grid = {tuple(p[k] for k in P.FIELDS) for _, p in grid}
    of_cases = {P.signature(c['call']) for c in P.CASES}
    missing, stale = of_grid - of_cases, of_cases - of_grid
    print('%d grid calls, %d signatures, %d cases' % (len(grid), len(of_grid), len(P.CASES)))
    assert not missing, 'plans of the grid without a case (scripts/make_backward_plan_cases.py): %s' % [P.named(s) for s in sorted(missing)[:3]]
    assert not stale, 'cases whose plan the grid does not reach: %s' % [P.named(s) for s in sorted(stale)[:3]]
    assert len(P.CASES) == len(of_cases), 'two cases of one signature'
    # ... case by case: the signature recorded when the table was written is the one the call takes now
    drifted = [P.case_id(c) for c in P.CASES if c['signature'] != P.signature(c['call'])]
    assert not drifted, drifted[:5]
    # each case is a grid call, and none costs more than the issue's budget for a sub-second oracle run
    calls = {json.dumps(c, sort_keys=True) for c, _ in grid}
    for case in P.CASES:
        assert json.dumps(case['call'], sort_keys=True) in calls, case
        assert P.cost(case['call']) <= 2e7, case


def test_required_scene_options_are_placed():
    """`backdrop` in a case of every (big, finish, big_overflow, depth_in_gather) with big set; `overflow` in one of every such
    combination with big_overflow and in one signature whose overflow pass is a launch of its own."""
    combos, with_backdrop, with_overflow, own_pass = set(), set(), set(), False
    for case in P.CASES:
        n = P.named(P.signature(case['call']))
        cb = (n['big'], n['finish'], n['big_overflow'], n['depth_in_gather'])
        if n['big']:
            combos.add(cb)
            if case['scene']['backdrop']:
                assert case['call']['S'] >= 48
                with_backdrop.add(cb)
            if case['scene']['overflow']:
                with_overflow.add(cb)
        if case['scene']['overflow'] and n['overflow_pass'] and not n['big_overflow']:
            own_pass = True
    assert combos and with_backdrop == combos, combos - with_backdrop
    assert {cb for cb in combos if cb[2]} <= with_overflow
    assert own_pass


def test_plan_invariants_over_the_grid(grid):
    bad = []
    for c, p in grid:
        def check(ok, what):
            if not ok:
                bad.append((what, c, {k: p[k] for k in P.FIELDS}))
        rgb, alpha, depth = c['modes']
        k7, early = p['gather'] != P.GATHER_NONE, p['gather_first'] or p['gather_in_tail']
        aligned = not c['mis']
        check(p['k6'] == int(bool(rgb or alpha)) and k7 == bool(rgb), 'stages')
        check(not (p['gather_first'] and p['gather_in_tail']), 'both early orders')
        if p['bands'] and p['use_records']:
            check(p['setup_alone'] + p['setup_in_gather'] == 1, 'line setup: one launch')
        else:
            check(not p['setup_alone'] and not p['setup_in_gather'], 'line setup without records')
        check(not p['setup_in_gather'] or p['gather_first'], 'setup_in_gather outside the gather-first order')
        # exactly one owner zeroes each cube of grad_textures
        if k7:
            stores_all = p['gather'] == P.GATHER_FACE and not p['listed'] and not c['lit']
            check((p['tex_zeros'] == P.TEX_ZEROS_NONE) == stores_all, 'tex_zeros: nobody / the gather itself')
            check(p['gather'] == (P.GATHER_FACE if c['ts'] <= 13 else P.GATHER_ATOMIC), 'gather')
        else:
            check(p['tex_zeros'] == P.TEX_ZEROS_NONE and not p['light_fill'], 'tex_zeros without K7')
        check(p['tex_zeros'] != P.TEX_ZEROS_SETUP or p['setup_in_gather'], 'TEX_ZEROS_SETUP')
        check(p['tex_zeros'] != P.TEX_ZEROS_SETUP or (aligned and not c['lit']), 'TEX_ZEROS_SETUP: alignment, light')
        check(p['tex_zeros'] != P.TEX_ZEROS_BAND_UNLISTED or p['gather_in_tail'], 'TEX_ZEROS_BAND_UNLISTED')
        check(p['tex_zeros'] != P.TEX_ZEROS_BAND or not early, 'TEX_ZEROS_BAND beside an early gather')
        check(not p['gather_in_tail'] or p['tex_zeros'] in (P.TEX_ZEROS_BAND_UNLISTED, P.TEX_ZEROS_FILL), 'tail order: zeros')
        if p['tex_zeros'] in (P.TEX_ZEROS_BAND, P.TEX_ZEROS_BAND_UNLISTED):
            check(aligned and p['tex_bytes'] % 16 == 0 and p['tex_bytes'] <= p['fill_max'] and p['bands'], 'band fill')
        check(p['light_fill'] == int(bool(c['lit'] and k7)), 'light_fill')
        # grad_faces has exactly one finisher
        check((p['finish'] == P.FINISH_NONE) == (not p['bands']), 'finish none')
        check((p['finish'] in (P.FINISH_BIG, P.FINISH_ADD)) == bool(early), 'finish early')
        if early:
            check(p['finish'] == (P.FINISH_BIG if c['ts'] <= 8 else P.FINISH_ADD), 'finish: big / add')
            check(p['finish'] != P.FINISH_BIG or p['big'], 'FINISH_BIG without k_backward_big')
        check(p['finish'] != P.FINISH_GATHER or (p['gather'] == P.GATHER_FACE and p['listed']), 'FINISH_GATHER')
        want_zeros = P.FACE_ZEROS_ALL if early else (P.FACE_ZEROS_UNLISTED if p['finish'] == P.FINISH_GATHER else P.FACE_ZEROS_NONE)
        check(p['face_zeros'] == want_zeros, 'face_zeros')
        check(not p['listed'] or p['bands'], 'lists without the band pipeline')
        # K8
        check(p['depth_in_gather'] + p['depth'] == int(bool(depth)), 'depth')
        check(not p['depth_in_gather'] or (k7 and p['big']), 'depth_in_gather without its gather')
        # the merged overflow pass
        if p['big_overflow']:
            check(p['finish'] == P.FINISH_BIG and p['static_taps'] and not c['lit'] and p['overflow_pass'] and p['threads'] == 256,
                  'big_overflow')
        if c['flags'] & P.SERIAL:
            check(not early and not p['big_overflow'], 'serial order')
        check(p['fill_faces'] == int(not p['k6']), 'fill_faces')
        check(not p['depth_lists'] or (p['fill_faces'] and depth and c['visible']), 'depth_lists')
        check(p['big'] == int(k7 and c['ts'] <= 8), 'big')
        check(p['static_taps'] == int(k7 and c['ts'] == 2 and c['eps'] > 2.0 ** -25), 'static_taps')
    assert not bad, (len(bad), bad[:3])


EPS_LOW, EPS_HIGH = 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20)  # float(1 - eps) == 1 (ties to even) | < 1
# (what the threshold is, the call below it, the call above it, the fields that must differ)
THRESHOLDS = [
    ('98 304 faces: gather-first | tail order', P.call(2048, 48, 8), P.call(2049, 48, 8), ('gather_first', 'gather_in_tail', 'tex_zeros')),
    ('655 360 faces: tail | serial order', P.call(2048, 320, 8), P.call(2049, 320, 8), ('gather_in_tail', 'finish', 'face_zeros')),
    ('texture size 2 | 3: static taps', P.call(2, 48, 64, 2), P.call(2, 48, 64, 3), ('static_taps',)),
    ('texture size 5 | 6: lanes per face', P.call(2, 48, 64, 5), P.call(2, 48, 64, 6), ('lanes',)),
    ('texture size 8 | 9: k_backward_big', P.call(2, 48, 64, 8), P.call(2, 48, 64, 9), ('big', 'lanes', 'finish', 'depth_in_gather')),
    ('texture size 13 | 14: face gather | atomics', P.call(2, 48, 64, 13), P.call(2, 48, 64, 14), ('gather', 'listed', 'gather_first')),
    ('40 960 bytes of gather LDS, 16 lanes (texture size 4: 24 576 | 5: 48 000)', P.call(2, 48, 64, 4), P.call(2, 48, 64, 5),
     ('setup_in_gather', 'setup_alone', 'tex_zeros')),
    ('40 960 bytes of gather LDS, 256 lanes (texture size 11: 31 944 | 12: 41 472)', P.call(2, 48, 64, 11), P.call(2, 48, 64, 12),
     ('setup_in_gather', 'setup_alone', 'tex_zeros')),
    ('32 768 bytes of line-setup LDS (1365 | 1366 bands)', P.call(1, 8, 1365, 3), P.call(1, 8, 1366, 3),
     ('setup_in_gather', 'setup_alone', 'tex_zeros')),
    ('grad_textures on | off the 16-byte grid, gather-first', P.call(2, 48, 64, 3), P.call(2, 48, 64, 3, mis=1), ('tex_zeros',)),
    ('grad_textures on | off the 16-byte grid, band fill', P.call(2, 48, 64, 3, flags=P.SERIAL), P.call(2, 48, 64, 3, flags=P.SERIAL, mis=1),
     ('tex_zeros',)),
    ('tex_bytes % 16 (1296 | 648 bytes)', P.call(1, 4, 8, 3, flags=P.SERIAL), P.call(1, 2, 8, 3, flags=P.SERIAL), ('tex_zeros',)),
    ('fill_max (1 MiB here: 170 | 172 cubes of 6144 bytes)', P.call(1, 170, 8, 8, flags=P.SERIAL), P.call(1, 172, 8, 8, flags=P.SERIAL),
     ('tex_zeros',)),
    ('eps 2^-25: static taps', P.call(2, 48, 64, 2, eps=EPS_HIGH), P.call(2, 48, 64, 2, eps=EPS_LOW), ('static_taps', 'depth_in_gather')),
    ('raster 512 | 513: the tail order (whole lines either way)', P.call(4, 32768, 512), P.call(4, 32768, 513), ('gather_in_tail',)),
    ('2^15 faces: chunked lines', P.call(1, 32767, 513), P.call(1, 32768, 513), ('row_chunked',)),
    ('raster 400 | 401: band workgroup, merged overflow pass', P.call(2, 48, 400), P.call(2, 48, 401), ('threads', 'big_overflow')),
    ('raster 1024 | 1056: k_bpm_row | k_bpm_fast', P.call(1, 8, 1024), P.call(1, 8, 1056), ('kernel', 'overflow_pass')),
]


@pytest.mark.parametrize('what,below,above,fields', THRESHOLDS, ids=[t[0].split(':')[0].split('(')[0].strip().replace(' ', '_') for t in THRESHOLDS])
def test_threshold_separates_a_pair(what, below, above, fields):
    a, b = P.plan(below), P.plan(above)
    same = [k for k in fields if a[k] == b[k]]
    assert not same, '%s: %s the same on both sides (%r)' % (what, same, {k: a[k] for k in same})


def test_threshold_pair_sizes():
    """The sizes the pairs above are built on: if a size moves, its pair no longer straddles the threshold it names."""
    assert P.plan(P.call(2, 48, 64, 4))['gather_lds'] == 24576 and P.plan(P.call(2, 48, 64, 5))['gather_lds'] == 48000
    assert P.plan(P.call(2, 48, 64, 11))['gather_lds'] == 31944 and P.plan(P.call(2, 48, 64, 12))['gather_lds'] == 41472
    assert P.plan(P.call(1, 8, 1365, 3))['setup_lds'] == 32760 and P.plan(P.call(1, 8, 1366, 3))['setup_lds'] == 32784
    lo, hi = P.plan(P.call(1, 170, 8, 8, flags=P.SERIAL)), P.plan(P.call(1, 172, 8, 8, flags=P.SERIAL))
    assert lo['tex_bytes'] <= lo['fill_max'] == hi['fill_max'] < hi['tex_bytes'] and hi['tex_bytes'] % 16 == 0
    assert P.plan(P.call(1, 2, 8, 3, flags=P.SERIAL))['tex_bytes'] % 16 == 8


def test_tail_order_tests_run_the_order_they_name():
    """tests/test_backward_tail_order_gpu.py: its mirrors of the two face gates, and the plans of its shapes."""
    import test_backward_tail_order_gpu as tail
    F = 48
    assert tail.GATE_FACES % F == 0 and tail.MAX_FACES % 320 == 0
    at, above = P.plan(P.call(tail.GATE_FACES // F, F, 8)), P.plan(P.call(tail.GATE_FACES // F + 1, F, 8))
    assert at['gather_first'] and not at['gather_in_tail'] and not above['gather_first'] and above['gather_in_tail']
    at, above = P.plan(P.call(tail.MAX_FACES // 320, 320, 8)), P.plan(P.call(tail.MAX_FACES // 320 + 1, 320, 8))
    assert at['gather_in_tail'] and not above['gather_in_tail'] and not above['gather_first']
    shapes = [(64, T, 256, (1, 1, 1)), (32, T, 256, (1, 1, 1)), (132, T, 128, (1, 1, 1)), (32, T, 128, (1, 0, 0)), (32, T, 128, (1, 1, 0)),
              (32, T, 128, (1, 0, 1)), (32, T, 128, (1, 1, 1)), (126, 800, 64, (1, 1, 1))]
    for B, F, S, modes in shapes:
        p = P.plan(P.call(B, F, S, 2, modes))
        want = dict(gather_first=0, gather_in_tail=1, tex_zeros=P.TEX_ZEROS_BAND_UNLISTED, finish=P.FINISH_BIG, face_zeros=P.FACE_ZEROS_ALL,
                    big_overflow=1, kernel=P.KERNEL_ROW, static_taps=1, depth_in_gather=modes[2], depth=0, setup_alone=1)
        assert {k: p[k] for k in want} == want, (B, F, S, modes)
        for flags in (P.SERIAL, P.EXACT, P.EXACT | P.SERIAL):
            p = P.plan(P.call(B, F, S, 2, modes, flags=flags))
            want = dict(gather_first=0, gather_in_tail=0, tex_zeros=P.TEX_ZEROS_BAND, finish=P.FINISH_GATHER,
                        face_zeros=P.FACE_ZEROS_UNLISTED, big_overflow=0, kernel=P.KERNEL_ROW, setup_alone=1)
            assert {k: p[k] for k in want} == want, (B, F, S, modes, flags)


def test_case_scenes_and_oracle_seconds():
    """Every case's scene through the oracle's forward: covered and uncovered pixels, listed and unlisted faces, the backdrop
    above BIG_PX candidate pixels and the images over the line buffer where the table says so; where K7 is the per-pixel scatter
    with float atomics, no element of grad_textures with more than two terms (backward_plans.terms_per_texel) and some with
    one.  The oracle's time per case -- forward and the three backward runs the GPU test makes of it, behind a warm-up -- is
    printed and held to the limit; the figures of the run that wrote the table stand beside it
    (tests/golden/backward_plan_oracle_seconds.json, written by scripts/make_backward_plan_cases.py, and here if it is missing)."""
    import os
    seconds, fns = P.oracle_seconds(P.CASES)
    bad = []
    for case in P.CASES:
        c = case['call']
        faces, _ = P.scene(case)
        cov, unc, lst, unl, backdrop, overflow = P.scene_facts(case, faces, fns[P.case_id(case)].face_index_map)
        # (per-pixel float atomics: one or two terms per texel, or the bit-for-bit comparison of two orders is ill-posed)
        atomic = P.named(P.signature(c))['gather'] == P.GATHER_ATOMIC
        terms = P.terms_per_texel(case) if atomic else None
        if not (cov and unc and lst and unl and backdrop and overflow) or (atomic and not 1 <= terms <= P.ATOMIC_TERMS):
            bad.append((P.case_id(case), cov, unc, lst, unl, backdrop, overflow, terms))
    slow = sorted(seconds.items(), key=lambda kv: -kv[1])[:5]
    print('oracle seconds per case: total %.1f, slowest %s' % (sum(seconds.values()), slow))
    if not os.path.exists(P.SECONDS_PATH):
        P.write_oracle_seconds(seconds)
    assert not bad, bad
    assert slow[0][1] <= 2.0, slow  # (no case may be why a GPU test needs more than a few seconds)
