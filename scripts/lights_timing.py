"""light_colors forward + backward: the HIP kernels against the plain-torch path.

    python scripts/lights_timing.py            # one JSON line per (mesh, shading, implementation), then the ratios

Meshes: 64 x the teapot (1 292 vertices, 2 464 faces) and 64 x an icosphere of 10 242 vertices (20 480 faces), the vertices
jittered per image.  The light: a lamp shared by the batch and nine SH coefficients per image, everything learnable.  A step is
(light_colors(vertices, faces, lights) * w).sum().backward() with the adjacency table already cached: gradients to the vertices
and to all six parameters.  Every timed step runs in a child process of its own under `timeout`, and the first one that fails
ends the run.  Informational: no threshold.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

MESHES = ('teapot', 'icosphere')
SHADINGS = ('flat', 'smooth')
IMPLEMENTATIONS = ('hip', 'torch')
STEP_TIMEOUT = 120  # seconds per child


def one(mesh, shading, implementation, batch, steps):
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    from example_lights import icosphere
    dev = torch.device('cuda', 0)
    v, f = bench.load_teapot() if mesh == 'teapot' else icosphere(5)
    rng = np.random.default_rng(5)
    x = (v[None] + rng.normal(scale=0.01, size=(batch,) + v.shape)).astype(np.float32)
    vertices = torch.tensor(x, device=dev, requires_grad=True)
    faces = torch.tensor(f, device=dev)
    sh = torch.tensor(rng.uniform(-0.3, 0.3, (batch, 9, 3)).astype(np.float32))
    lights = nr.Lights(0.4, 0.6, direction=(0.3, 0.8, -0.45), sh=sh, learnable=nr.lights.NAMES).to(dev)
    smooth = shading == 'smooth'
    w = torch.tensor(rng.normal(size=(batch, 2 * len(f)) + ((3, 3) if smooth else (3,))).astype(np.float32), device=dev)

    def step():
        vertices.grad = None
        lights.zero_grad()
        out = nr.light_colors(vertices, faces, lights, smooth=smooth, implementation=implementation)
        (out * w).sum().backward()
        return out
    t0 = time.perf_counter()
    first = step()
    torch.cuda.synchronize()
    table_ms = (time.perf_counter() - t0) * 1e3   # the first call: the adjacency table and its upload
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    stop.record()
    torch.cuda.synchronize()
    print(json.dumps({'mesh': mesh, 'B': batch, 'vertices': int(v.shape[0]), 'faces': int(f.shape[0]), 'shading': shading,
                      'implementation': implementation, 'fwd_bwd_ms': round(ms, 4),
                      'fwd_bwd_ms_events': round(start.elapsed_time(stop) / steps, 4), 'first_call_ms': round(table_ms, 2),
                      'light_mean': float(first.detach().mean()), 'grad_abs_sum': float(vertices.grad.abs().sum()),
                      'sh_grad_abs_sum': float(lights.sh.grad.abs().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--one', nargs=3, metavar=('MESH', 'SHADING', 'IMPLEMENTATION'), help='(a child: time one step)')
    args = ap.parse_args()
    if args.one:
        one(args.one[0], args.one[1], args.one[2], args.batch, args.steps)
        return
    results = {}
    for mesh in MESHES:
        for shading in SHADINGS:
            for impl in IMPLEMENTATIONS:
                cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), '--batch', str(args.batch),
                       '--steps', str(args.steps), '--one', mesh, shading, impl]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
                sys.stdout.write(p.stdout)
                sys.stdout.flush()
                if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started
                    print('%s %s %s ended with status %d: stopping' % (mesh, shading, impl, p.returncode), flush=True)
                    sys.exit(p.returncode)
                results[mesh, shading, impl] = json.loads(p.stdout.strip().splitlines()[-1])
    for mesh in MESHES:
        for shading in SHADINGS:
            h, t = results[mesh, shading, 'hip'], results[mesh, shading, 'torch']
            print(json.dumps({'mesh': mesh, 'shading': shading, 'hip_ms': h['fwd_bwd_ms'], 'torch_ms': t['fwd_bwd_ms'],
                              'torch_over_hip': round(t['fwd_bwd_ms'] / h['fwd_bwd_ms'], 2)}), flush=True)


if __name__ == '__main__':
    main()
