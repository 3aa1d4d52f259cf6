"""Writes tests/golden/backward_plan_cases.json (and backward_plan_oracle_seconds.json beside it): for every distinct launch plan (tests/backward_plans.py: signature) that the
grid of fused-backward calls reaches, the cheapest grid call that takes it and a scene to run it on.  Host only: the plans come
from the measurement build's nr_profile_backward_plan, the scenes are checked with the oracle's forward.

    python scripts/make_backward_plan_cases.py

Scenes: helpers.random_scene by the first (spread, size, seed) that leaves covered and uncovered pixels and listed and unlisted
faces.  `backdrop` (a face above BIG_PX candidate pixels: k_backward_big walks it) goes to one signature of every distinct
(big, finish, big_overflow, depth_in_gather) with big set, `overflow` (every third image over the line buffer) to one of every
such combination with big_overflow and to one signature with an overflow pass of its own; where the cheapest call of a
signature is too small for its option the cheapest grid call that is large enough takes its place.

Plans whose K7 is the per-pixel scatter with float atomics (texture size above 13) get faces of about a pixel (size 3 / S), and
the first seed at which no texel of grad_textures receives more than two terms (backward_plans.terms_per_texel): the test
compares grad_textures bit for bit between two launch orders, a float sum of three or more atomically added terms has no
defined order, and up to two terms onto the zero fill give one result in any order (0 + a is exact, a + b commutes)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

TABLE = os.path.join(ROOT, 'tests', 'golden', 'backward_plan_cases.json')
if not os.path.exists(TABLE):  # (backward_plans loads the table when it is imported)
    with open(TABLE, 'w') as f:
        f.write('[]\n')
import backward_plans as P  # noqa: E402
from oracle import oracle as O  # noqa: E402

RECIPES = [(0.6, 0.25), (0.8, 0.12), (0.9, 0.05), (1.5, 0.3), (0.3, 0.6)]
SEEDS = range(12)


def facts(case):
    faces, _ = P.scene(case)
    c = case['call']
    fn = O.Rasterize(c['S'], 0.1, 100.0, c['eps'], (0, 0, 0), False, True, False)
    fn(faces)
    return P.scene_facts(case, faces, fn.face_index_map)


def find_scene(c, backdrop=False, overflow=False):
    atomic = P.named(P.signature(c))['gather'] == P.GATHER_ATOMIC
    recipes, seeds = ([(0.6, 3.0 / c['S'])], range(400)) if atomic else (RECIPES, SEEDS)
    for spread, size in recipes:
        for seed in seeds:
            case = dict(call=c, scene=dict(seed=seed, spread=spread, size=size, backdrop=backdrop, overflow=overflow))
            cov, unc, lst, unl, bd, ov = facts(case)
            if cov and unc and lst and unl and bd and ov and (not atomic or P.terms_per_texel(case) <= P.ATOMIC_TERMS):
                return case
    return None


def main():
    by_sig = {}  # signature -> {(B, F, S): cheapest call of that shape}
    for c in P.grid_calls():
        s = P.signature(c)
        if s is None:
            continue
        shapes = by_sig.setdefault(s, {})
        k = (c['B'], c['F'], c['S'])
        if k not in shapes or P.cost(c) < P.cost(shapes[k]):
            shapes[k] = c
    ordered = {s: sorted(v.values(), key=P.cost) for s, v in by_sig.items()}
    sigs = sorted(ordered, key=lambda s: (P.cost(ordered[s][0]), s))
    print('%d signatures' % len(sigs))
    cases = {}

    def place(group, what, fits, **opt):
        """the option on the first signature of `group` (cheapest first) that has a grid call with a scene for it"""
        for s in group:
            if s in cases:
                continue
            for c in ordered[s]:
                if P.cost(c) > 2e7 or not fits(c):
                    continue
                case = find_scene(c, **opt)
                if case:
                    cases[s] = case
                    print('%s -> %s' % (what, P.case_id(case)))
                    return
        raise SystemExit('no grid call takes %s' % what)

    combo = lambda s: tuple(P.named(s)[k] for k in ('big', 'finish', 'big_overflow', 'depth_in_gather'))
    for cb in sorted({combo(s) for s in sigs if P.named(s)['big']}):
        group = [s for s in sigs if combo(s) == cb]
        place(group, 'backdrop %r' % (cb,), lambda c: c['S'] >= 48, backdrop=True)
        if cb[2]:
            place(group, 'overflow %r' % (cb,), lambda c: c['F'] >= 48 and c['B'] >= 3, overflow=True)
    place([s for s in sigs if P.named(s)['overflow_pass'] and not P.named(s)['big_overflow']], 'overflow, a pass of its own',
          lambda c: c['F'] >= 48 and c['B'] >= 3, overflow=True)
    for s in sigs:
        if s not in cases:
            cases[s] = find_scene(ordered[s][0])
            if cases[s] is None:
                raise SystemExit('no scene for %r' % (ordered[s][0],))
    out = [dict(cases[s], signature=list(s)) for s in sigs]
    with open(P.CASES_PATH, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(c, sort_keys=True) for c in out) + '\n]\n')
    print('wrote %d cases, largest cost %.3g' % (len(out), max(P.cost(c['call']) for c in out)))
    # the oracle's time per case when the table was written (test_backward_plans.py prints its own and holds them to the limit)
    seconds, _ = P.oracle_seconds(out)
    P.write_oracle_seconds(seconds)
    print('oracle seconds: total %.1f, slowest %.2f' % (sum(seconds.values()), max(seconds.values())))


if __name__ == '__main__':
    main()
