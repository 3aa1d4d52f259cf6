"""Soft silhouettes, forward + backward: the HIP kernels against soft_silhouettes_torch, with the hard silhouette as a bystander.

    python scripts/soft_silhouettes_timing.py            # one JSON line per row

Workloads: 64 teapot views (2 464 faces, no fill_back copies) at 256 x 256 and at 64 x 64 with sigma in (1e-5, 1e-4, 1e-3),
and one icosphere(5) (20 480 faces) at 256 x 256 with sigma 1e-4.  A step is soft_silhouettes on the projected faces followed
by the backward with a fixed upstream gradient.  The plain-torch path holds every (pixel, face) pair of the call in some
forty float32 temporaries for its backward -- 64 views at 256 x 256 would need terabytes --, so it runs on `--torch-batch`
views (default 1) and its time is reported per image next to the HIP time per image; the icosphere has no torch row (160 GB
for one image).  Bystander rows, whole pipeline from the vertices: Renderer.render_silhouettes + backward and
Renderer.render_soft_silhouettes + backward on the same 64 views.  After a warm-up each row is timed in rounds between two host
clock readings that end in a device synchronise; the median round is reported.  A round is as many steps as fill
`--round-ms` (never fewer than `--steps`; the torch rows: `--torch-steps` per round).  One process; the first error ends it.
Informational: no threshold.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMAS = (1e-5, 1e-4, 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--torch-batch', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5, help='steps of the pilot round, and the least per timed round')
    ap.add_argument('--torch-steps', type=int, default=2)
    ap.add_argument('--round-ms', type=float, default=200.0, help='a timed round runs about this long')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    if not torch.cuda.is_available():
        raise SystemExit('soft_silhouettes_timing: needs a GPU (a CPU run says nothing about the kernels)')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)

    def timed(step, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def measure(step, fixed_steps=None):
        for _ in range(2):
            step()
        steps = fixed_steps or max(args.steps, int(args.round_ms / timed(step, args.steps)) + 1)
        r = [timed(step, steps) for _ in range(args.rounds if fixed_steps is None else 3)]
        return statistics.median(r), min(r), max(r), steps

    for mesh, S, sigmas in (('teapot', 256, SIGMAS), ('teapot', 64, SIGMAS), ('icosphere5', 256, (1e-4,))):
        B = args.batch if mesh == 'teapot' else 1
        if mesh == 'teapot':
            v, f = bench.load_teapot()
        else:
            v, f = (t.numpy() for t in nr.icosphere(5, 0.6))
        vertices = torch.tensor(np.broadcast_to(v[None], (B,) + v.shape).astype(np.float32), device=dev, requires_grad=True)
        faces = torch.tensor(f, device=dev)[None].expand(B, -1, -1).contiguous()
        renderer = nr.Renderer()
        renderer.image_size = S
        renderer.eye = torch.tensor([nr.get_points_from_angles(2.732, 30.0, 360.0 * i / B) for i in range(B)],
                                    dtype=torch.float32, device=dev)
        with torch.no_grad():
            projected = renderer._frontend(vertices, faces)[0][:, :f.shape[0]].contiguous()
        up = torch.tensor(rng.normal(size=(B, S, S)).astype(np.float32), device=dev)
        base = {'mesh': mesh, 'faces': int(f.shape[0]), 'image_size': S}

        for sigma in sigmas:
            leaf = projected.clone().requires_grad_(True)

            def hip_step():
                leaf.grad = None
                nr.soft_silhouettes(leaf, S, sigma, renderer.near, renderer.far, implementation='hip').backward(up)
            med, lo, hi, steps = measure(hip_step)
            row = dict(base, row='soft_silhouettes', sigma=sigma, implementation='hip', B=B, fwd_bwd_ms_median=round(med, 4),
                       fwd_bwd_ms_min=round(lo, 4), fwd_bwd_ms_max=round(hi, 4), ms_per_image=round(med / B, 5), steps=steps)
            print(json.dumps(row), flush=True)
            if mesh != 'teapot' or args.no_torch:
                continue
            Bt = min(args.torch_batch, B)
            small = projected[:Bt].clone().requires_grad_(True)

            def torch_step():
                small.grad = None
                nr.soft_silhouettes(small, S, sigma, renderer.near, renderer.far, implementation='torch').backward(up[:Bt])
            tmed, tlo, thi, tsteps = measure(torch_step, args.torch_steps)
            hip_small = projected[:Bt].clone().requires_grad_(True)
            nr.soft_silhouettes(hip_small, S, sigma, renderer.near, renderer.far, implementation='hip').backward(up[:Bt])
            print(json.dumps(dict(base, row='soft_silhouettes', sigma=sigma, implementation='torch', B=Bt,
                                  fwd_bwd_ms_median=round(tmed, 4), fwd_bwd_ms_min=round(tlo, 4), fwd_bwd_ms_max=round(thi, 4),
                                  ms_per_image=round(tmed / Bt, 5), steps=tsteps,
                                  torch_over_hip_per_image=round((tmed / Bt) / (med / B), 1),
                                  max_abs_diff_grad=float((hip_small.grad - small.grad).abs().max()))), flush=True)
            del small, hip_small
            torch.cuda.empty_cache()

        if mesh != 'teapot':
            continue

        def hard_step():
            vertices.grad = None
            renderer.render_silhouettes(vertices, faces).backward(up)

        def soft_step():
            vertices.grad = None
            renderer.render_soft_silhouettes(vertices, faces).backward(up)
        for name, step in (('render_silhouettes', hard_step), ('render_soft_silhouettes', soft_step)):
            med, lo, hi, steps = measure(step)
            print(json.dumps(dict(base, row=name, sigma=renderer.soft_sigma if 'soft' in name else None, implementation='hip', B=B,
                                  fwd_bwd_ms_median=round(med, 4), fwd_bwd_ms_min=round(lo, 4), fwd_bwd_ms_max=round(hi, 4),
                                  ms_per_image=round(med / B, 5), steps=steps)), flush=True)


if __name__ == '__main__':
    main()
