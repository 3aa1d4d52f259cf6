"""Normals, forward + backward: the HIP kernels against this module's plain-torch path.

    python scripts/normals_timing.py            # one JSON line per (workload, row, implementation), then the ratios

Workloads, 64 images each: the teapot (1 292 vertices, 2 464 faces) and icosphere(5) (10 242 vertices, 20 480 faces).  Rows:
corner_normals flat and smooth with fill_back (a step is the call followed by the backward with a fixed upstream gradient),
and Renderer.render_normals at 256 x 256, smooth, world space (a step is the render and the backward of its sum with a
fixed upstream image; the torch row is the same composition with corner_normals(implementation='torch')).  Both
implementations run on the SAME tensors.  After a warm-up the two are timed in alternating rounds, each round between two
host clock readings that end in a device synchronise, and the median round is reported.  A round is as many steps as fill
`--round-ms` (a pilot round of `--steps` steps sets the count per row and implementation; never fewer than `--steps`), so
that a row of 0.2 ms steps is not a measurement of the clock.  One process; the first error ends it.  `--only N` runs
workload N alone.  Informational: no threshold.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ('teapot', 'icosphere5')
ROWS = ('corner_flat', 'corner_smooth', 'render_normals')
IMPLEMENTATIONS = ('hip', 'torch')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20, help='steps of the pilot round, and the least per timed round')
    ap.add_argument('--round-ms', type=float, default=300.0, help='a timed round runs about this long')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--image-size', type=int, default=256)
    ap.add_argument('--only', type=int, default=None, help='run workload number N alone')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    if not torch.cuda.is_available():
        raise SystemExit('normals_timing: needs a GPU (a CPU run says nothing about the kernels)')
    dev = torch.device('cuda', 0)
    B = args.batch
    for mesh in (WORKLOADS if args.only is None else WORKLOADS[args.only:args.only + 1]):
        if mesh == 'teapot':
            v, f = bench.load_teapot()
        else:
            v, f = (t.numpy() for t in nr.icosphere(5, 0.6))
        rng = np.random.default_rng(7)
        x = (v[None] + rng.normal(scale=0.002, size=(B,) + v.shape)).astype(np.float32)
        vertices = torch.tensor(x, device=dev, requires_grad=True)
        faces = torch.tensor(f, device=dev)[None].expand(B, -1, -1).contiguous()
        renderer = nr.Renderer()
        renderer.image_size = args.image_size
        renderer.shading = 'smooth'
        renderer.eye = torch.tensor([nr.get_points_from_angles(2.732, 30.0, 360.0 * i / B) for i in range(B)],
                                    dtype=torch.float32, device=dev)
        up_corner = torch.tensor(rng.normal(size=(B, 2 * f.shape[0], 3, 3)).astype(np.float32), device=dev)
        up_image = torch.tensor(rng.normal(size=(B, 3, args.image_size, args.image_size)).astype(np.float32), device=dev)

        def step(row, implementation):
            vertices.grad = None
            if row == 'render_normals':
                if implementation == 'hip':
                    y = renderer.render_normals(vertices, faces)
                else:
                    corner = nr.corner_normals(vertices, faces, smooth=True, fill_back=True, implementation='torch')
                    projected, _ = renderer._frontend(vertices, faces)
                    y = nr.rasterize_rgbad(projected, corner, renderer.image_size, renderer.anti_aliasing, renderer.near,
                                           renderer.far, renderer.rasterizer_eps, [0, 0, 0], True, False, False)['rgb']
                y.backward(up_image)
            else:
                y = nr.corner_normals(vertices, faces, smooth=row == 'corner_smooth', fill_back=True,
                                      implementation=implementation).colors
                y.backward(up_corner)
            return y

        def timed_round(row, implementation, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(row, implementation)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3
        for row in ROWS:
            out = {}
            for impl in IMPLEMENTATIONS:           # warm-up: code objects, the allocator, the adjacency table
                for _ in range(5):
                    out[impl] = step(row, impl).detach().clone(), vertices.grad.clone()
            steps = {impl: max(args.steps, int(args.round_ms / timed_round(row, impl, args.steps)) + 1) for impl in IMPLEMENTATIONS}
            rounds = {impl: [] for impl in IMPLEMENTATIONS}
            for _ in range(args.rounds):           # alternating, so that a busy host spoils both alike
                for impl in IMPLEMENTATIONS:
                    rounds[impl].append(timed_round(row, impl, steps[impl]))
            diff = float((out['hip'][0] - out['torch'][0]).abs().max()), float((out['hip'][1] - out['torch'][1]).abs().max())
            for impl in IMPLEMENTATIONS:
                r = rounds[impl]
                print(json.dumps({'mesh': mesh, 'row': row, 'B': B, 'vertices': int(v.shape[0]), 'faces': int(f.shape[0]),
                                  'implementation': impl, 'fwd_bwd_ms_median': round(statistics.median(r), 4),
                                  'fwd_bwd_ms_min': round(min(r), 4), 'fwd_bwd_ms_max': round(max(r), 4),
                                  'steps': steps[impl], 'rounds': args.rounds}), flush=True)
            h, t = statistics.median(rounds['hip']), statistics.median(rounds['torch'])
            print(json.dumps({'mesh': mesh, 'row': row, 'hip_ms': round(h, 4), 'torch_ms': round(t, 4),
                              'torch_over_hip': round(t / h, 2), 'max_abs_diff_value': diff[0],
                              'max_abs_diff_grad': diff[1]}), flush=True)


if __name__ == '__main__':
    main()
