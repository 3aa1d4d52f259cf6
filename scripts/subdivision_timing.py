"""Mesh subdivision, forward + backward of plan(vertices): the HIP kernel against this module's plain-torch path.

    python scripts/subdivision_timing.py            # one JSON line per (workload, implementation), then the ratios

Workloads, 64 images each, Loop: the teapot (1 292 vertices) at levels 1 and 2, and icosphere(3) at level 2 (642 -> 10 242
vertices).  A step is plan(vertices, implementation) followed by the backward of its sum with a fixed upstream gradient,
the plan already built; both implementations run on the SAME tensors.  After a warm-up the two are timed in alternating
rounds of `--steps` steps, each round between two host clock readings that end in a device synchronise, and the median
round is reported.  The one-off host cost of building a plan (tables, transposes, upload) is timed on a fresh index tensor.
One process; the first error ends it.  `--only N` runs workload N alone, for a kernel trace of one size.  Informational: no
threshold.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (('teapot', 1), ('teapot', 2), ('icosphere3', 2))
IMPLEMENTATIONS = ('hip', 'torch')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=50, help='steps per timed round')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--only', type=int, default=None, help='run workload number N alone (a kernel trace of one size)')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    if not torch.cuda.is_available():
        raise SystemExit('subdivision_timing: needs a GPU (a CPU run says nothing about the kernel)')
    dev = torch.device('cuda', 0)
    for mesh, levels in (WORKLOADS if args.only is None else WORKLOADS[args.only:args.only + 1]):
        if mesh == 'teapot':
            v, f = bench.load_teapot()
        else:
            v, f = (t.numpy() for t in nr.icosphere(3))
        rng = np.random.default_rng(7)
        x = (v[None] + rng.normal(scale=0.01, size=(args.batch,) + v.shape)).astype(np.float32)
        vertices = torch.tensor(x, device=dev, requires_grad=True)
        faces = torch.tensor(f, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = nr.subdivision(faces, v.shape[0], levels, 'loop')
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        upstream = torch.tensor(rng.normal(size=(args.batch, plan.num_vertices, 3)).astype(np.float32), device=dev)

        def step(implementation):
            vertices.grad = None
            y = plan(vertices, implementation=implementation)
            y.backward(upstream)
            return y

        def timed_round(implementation):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(implementation)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3
        out = {}
        for impl in IMPLEMENTATIONS:           # warm-up: code objects, the allocator, the torch path's row index
            for _ in range(10):
                out[impl] = step(impl).detach().clone(), vertices.grad.clone()
        rounds = {impl: [] for impl in IMPLEMENTATIONS}
        for _ in range(args.rounds):           # alternating, so that a busy host spoils both alike
            for impl in IMPLEMENTATIONS:
                rounds[impl].append(timed_round(impl))
        diff = float((out['hip'][0] - out['torch'][0]).abs().max()), float((out['hip'][1] - out['torch'][1]).abs().max())
        entries = sum(l.forward.num_entries for l in plan._levels)
        for impl in IMPLEMENTATIONS:
            r = rounds[impl]
            print(json.dumps({'mesh': mesh, 'levels': levels, 'B': args.batch, 'vertices_in': int(v.shape[0]),
                              'vertices_out': plan.num_vertices, 'faces_out': int(plan.faces.shape[0]), 'entries': entries,
                              'implementation': impl, 'fwd_bwd_ms_median': round(statistics.median(r), 4),
                              'fwd_bwd_ms_min': round(min(r), 4), 'fwd_bwd_ms_max': round(max(r), 4),
                              'steps': args.steps, 'rounds': args.rounds, 'plan_build_ms': round(build_ms, 2)}), flush=True)
        h, t = statistics.median(rounds['hip']), statistics.median(rounds['torch'])
        print(json.dumps({'mesh': mesh, 'levels': levels, 'hip_ms': round(h, 4), 'torch_ms': round(t, 4),
                          'torch_over_hip': round(t / h, 2), 'max_abs_diff_value': diff[0], 'max_abs_diff_grad': diff[1],
                          'plan_build_ms': round(build_ms, 2)}), flush=True)


if __name__ == '__main__':
    main()
