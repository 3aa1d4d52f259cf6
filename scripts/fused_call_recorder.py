"""Which launch plans of the fused backward does the suite reach?  A pytest plugin that writes down every call of
nr_backward_rasterize[_lit] that a test makes in its own process -- as nr_profile_backward_plan describes a call
(include/nr_hip_profile.h), with the test's id -- and a replay that counts the plans of the recorded calls.

    PYTHONPATH=scripts python -m pytest tests -m gpu -p fused_call_recorder --fused-calls calls.jsonl
    python scripts/fused_call_recorder.py calls.jsonl [more.jsonl ...]

The replay prints how many distinct plans (tests/backward_plans.py: signature) the tests other than
tests/test_backward_plans_gpu.py reach, and how many of the table's plans (backward_plans.CASES) are among them.  Calls made by
child processes (bench.py, the examples run as scripts) are not seen."""
import json
import os
import sys


def pytest_addoption(parser):
    parser.addoption('--fused-calls', default=None, help='append the fused backward calls of this run to this file (JSON lines)')


def pytest_configure(config):
    path = config.getoption('--fused-calls')
    if not path:
        return
    from neural_renderer_amd import _lib
    lib = _lib.load()
    out = open(path, 'a')
    seen = set()

    def wrap(name, has_lit):
        fn = getattr(lib, name)

        def record(*a):
            lit, r = (a[0], a[1:]) if has_lit else (None, a)
            # r: faces z_ref face_index weight depth rgb alpha g_rgb g_alpha g_depth grad_faces grad_textures B F S ts eps flags
            #    visible_faces workspace workspace_bytes stream
            tex_faces = grad_light = 0
            if lit is not None and r[7] and r[11]:
                lit = getattr(lit, 'contents', lit)
                tex_faces, grad_light = int(lit.texture_faces), int(bool(lit.grad_light))
            d = dict(B=r[12], F=r[13], S=r[14], ts=r[15], rgb=int(bool(r[7])), alpha=int(bool(r[8])), depth=int(bool(r[9])), eps=r[16],
                     flags=r[17], tex_faces=tex_faces, grad_light=grad_light, low=(int(r[11]) & 15) if r[11] else -1,
                     visible=int(bool(r[18])), ws=int(r[20]))
            test = os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]
            key = (json.dumps(d, sort_keys=True), test.split('[')[0])
            if key not in seen:
                seen.add(key)
                out.write(json.dumps(dict(test=test, call=d)) + '\n')
                out.flush()
            return fn(*a)
        setattr(lib, name, record)
    wrap('nr_backward_rasterize', False)
    wrap('nr_backward_rasterize_lit', True)


def replay(paths):
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    import backward_plans as P
    hook, out = P.hook(), (ctypes.c_int64 * len(P.FIELDS + P.SIZES))()
    earlier, refused, records = set(), 0, 0
    for path in paths:
        for line in open(path):
            r = json.loads(line)
            if 'test_backward_plans_gpu' in r['test']:
                continue
            d = r['call']
            records += 1
            if hook(d['B'], d['F'], d['S'], d['ts'] or 2, d['rgb'], d['alpha'], d['depth'], d['eps'], d['flags'], d['tex_faces'],
                    d['grad_light'], d['low'], d['visible'], d['ws'], out):
                refused += 1
                continue
            earlier.add(tuple(out[:len(P.FIELDS)]))
    table = {c['signature'] for c in P.CASES}
    print('%d recorded calls of the other tests (%d refused by the plan), %d distinct plans; of the table\'s %d plans they reach %d, %d are new'
          % (records, refused, len(earlier), len(table), len(table & earlier), len(table - earlier)))


if __name__ == '__main__':
    replay(sys.argv[1:])
