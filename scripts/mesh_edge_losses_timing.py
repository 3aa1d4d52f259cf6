"""edge_length_loss / cotangent_laplacian_loss forward + backward: the HIP kernels against the plain-torch path.

    python scripts/mesh_edge_losses_timing.py            # one JSON line per (mesh, loss, implementation), then the ratios

Meshes: 64 x the teapot (1 292 vertices, 2 464 faces) and 64 x an icosphere of 10 242 vertices (20 480 faces), the
vertices jittered per image.  A step is loss(vertices, faces).sum().backward() with the tables already cached.  Every timed
step runs in a child process of its own under `timeout`, and the first one that fails ends the run.  Informational: no
threshold.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MESHES = ('teapot', 'icosphere')
LOSSES = ('edge_squared', 'edge_rest', 'cotangent')   # the edge loss without a target (no square root) and with rest lengths [E]
IMPLEMENTATIONS = ('hip', 'torch')
STEP_TIMEOUT = 120  # seconds per child


def icosphere(level):
    import numpy as np
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def one(mesh, loss, implementation, batch, steps):
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    dev = torch.device('cuda', 0)
    v, f = bench.load_teapot() if mesh == 'teapot' else icosphere(5)
    rng = np.random.default_rng(5)
    x = (v[None] + rng.normal(scale=0.01, size=(batch,) + v.shape)).astype(np.float32)
    vertices = torch.tensor(x, device=dev, requires_grad=True)
    faces = torch.tensor(f, device=dev)
    if loss == 'cotangent':
        fn = nr.cotangent_laplacian_loss
    else:   # rest lengths: the unjittered mesh's own
        rest = 0.0 if loss == 'edge_squared' else nr.edge_lengths(torch.tensor(v, device=dev), faces)

        def fn(x, f, implementation):
            return nr.edge_length_loss(x, f, target=rest, implementation=implementation)

    def step():
        vertices.grad = None
        out = fn(vertices, faces, implementation=implementation)
        out.sum().backward()
        return out
    t0 = time.perf_counter()
    first = step()
    torch.cuda.synchronize()
    tables_ms = (time.perf_counter() - t0) * 1e3   # the first call: the host tables and their upload
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
    print(json.dumps({'mesh': mesh, 'B': batch, 'vertices': int(v.shape[0]), 'faces': int(f.shape[0]), 'loss': loss,
                      'implementation': implementation, 'fwd_bwd_ms': round(ms, 4),
                      'fwd_bwd_ms_events': round(start.elapsed_time(stop) / steps, 4), 'first_call_ms': round(tables_ms, 2),
                      'loss0': float(first.detach()[0]), 'grad_abs_sum': float(vertices.grad.abs().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--one', nargs=3, metavar=('MESH', 'LOSS', 'IMPLEMENTATION'), help='(a child: time one step)')
    args = ap.parse_args()
    if args.one:
        one(args.one[0], args.one[1], args.one[2], args.batch, args.steps)
        return
    results = {}
    for mesh in MESHES:
        for loss in LOSSES:
            for impl in IMPLEMENTATIONS:
                cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), '--batch', str(args.batch),
                       '--steps', str(args.steps), '--one', mesh, loss, impl]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
                sys.stdout.write(p.stdout)
                sys.stdout.flush()
                if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started
                    print('%s %s %s ended with status %d: stopping' % (mesh, loss, impl, p.returncode), flush=True)
                    sys.exit(p.returncode)
                results[mesh, loss, impl] = json.loads(p.stdout.strip().splitlines()[-1])
    for mesh in MESHES:
        for loss in LOSSES:
            h, t = results[mesh, loss, 'hip'], results[mesh, loss, 'torch']
            print(json.dumps({'mesh': mesh, 'loss': loss, 'hip_ms': h['fwd_bwd_ms'], 'torch_ms': t['fwd_bwd_ms'],
                              'torch_over_hip': round(t['fwd_bwd_ms'] / h['fwd_bwd_ms'], 2)}), flush=True)


if __name__ == '__main__':
    main()
