"""Soft colour rendering, forward + backward: the HIP kernels against soft_render_torch, with soft_silhouettes and render as
bystanders.

    python scripts/soft_render_timing.py            # one JSON line per row
    python scripts/soft_render_timing.py --corners  # ... and the corner-colour rows

Workloads: 64 teapot views (2 464 faces, no fill_back copies) at 256 x 256 and at 64 x 64 with sigma in (1e-5, 1e-4, 1e-3),
gamma 1e-2, one random colour per face and image.  A step is soft_render on the projected faces followed by the backward with
a fixed upstream gradient.  The plain-torch path holds every (pixel, face) pair of the call in dozens of float32 temporaries
for its backward, so it runs on `--torch-batch` views (default 1) and its time is reported per image next to the HIP time per
image, with the largest differences of that view's rgba and gradients.  Bystander rows: soft_silhouettes + backward on the same
projected faces, and, whole pipeline from the vertices, Renderer.render (texture cubes, size 2) + backward and
Renderer.render_soft + backward on the same 64 views.  After a warm-up each row is timed in rounds between two host clock
readings that end in a device synchronise; the median round is reported.  A round is as many steps as fill `--round-ms` (never
fewer than `--steps`; the torch rows: `--torch-steps` per round).  One process; the first error ends it.  Informational: no
threshold.

`--corners` adds, after each flat row and measured the same way, the row of the same call with corner colours [B,F,3,3]
(`soft_render_corners`: the nr_soft_corners_* kernels, `corners_over_flat` its time over the flat row's; the two forwards
alone, `soft_render_forward` and `soft_render_corners_forward`, under no_grad; the torch path with
corner colours on the same `--torch-batch` views), Renderer.render_soft(per_pixel=True) with a VertexColors beside render_soft,
and one more workload: a single icosphere(5) (20 480 faces) at 256 x 256, sigma 1e-4, flat and corner colours.
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
GAMMA = 1e-2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--torch-batch', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5, help='steps of the pilot round, and the least per timed round')
    ap.add_argument('--torch-steps', type=int, default=2)
    ap.add_argument('--round-ms', type=float, default=200.0, help='a timed round runs about this long')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--corners', action='store_true', help='add the corner-colour rows and the icosphere(5) workload')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    if not torch.cuda.is_available():
        raise SystemExit('soft_render_timing: needs a GPU (a CPU run says nothing about the kernels)')
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

    def row(base, name, implementation, B, m, **more):
        med, lo, hi, steps = m
        print(json.dumps(dict(base, row=name, implementation=implementation, B=B, fwd_bwd_ms_median=round(med, 4),
                              fwd_bwd_ms_min=round(lo, 4), fwd_bwd_ms_max=round(hi, 4), ms_per_image=round(med / B, 5),
                              steps=steps, **more)), flush=True)

    B = args.batch
    v, f = bench.load_teapot()
    F = int(f.shape[0])
    for S in (256, 64):
        vertices = torch.tensor(np.broadcast_to(v[None], (B,) + v.shape).astype(np.float32), device=dev, requires_grad=True)
        faces = torch.tensor(f, device=dev)[None].expand(B, -1, -1).contiguous()
        renderer = nr.Renderer()
        renderer.image_size = S
        renderer.soft_gamma = GAMMA
        renderer.eye = torch.tensor([nr.get_points_from_angles(2.732, 30.0, 360.0 * i / B) for i in range(B)],
                                    dtype=torch.float32, device=dev)
        with torch.no_grad():
            projected = renderer._frontend(vertices, faces)[0][:, :F].contiguous()
        colors = torch.tensor(rng.uniform(0, 1, (B, F, 3)).astype(np.float32), device=dev)
        corner_colors = torch.tensor(rng.uniform(0, 1, (B, F, 3, 3)).astype(np.float32), device=dev) if args.corners else None
        up = torch.tensor(rng.normal(size=(B, 4, S, S)).astype(np.float32), device=dev)
        base = {'mesh': 'teapot', 'faces': F, 'image_size': S, 'gamma': GAMMA}

        for sigma in SIGMAS:
            leaf, cleaf = projected.clone().requires_grad_(True), colors.clone().requires_grad_(True)

            def hip_step():
                leaf.grad = cleaf.grad = None
                nr.soft_render(leaf, cleaf, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip').backward(up)
            m = measure(hip_step)
            row(base, 'soft_render', 'hip', B, m, sigma=sigma)
            if args.corners:
                kleaf = corner_colors.clone().requires_grad_(True)

                def corner_step():
                    leaf.grad = kleaf.grad = None
                    nr.soft_render(leaf, kleaf, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip').backward(up)
                mc = measure(corner_step)
                row(base, 'soft_render_corners', 'hip', B, mc, sigma=sigma, corners_over_flat=round(mc[0] / m[0], 3))

                def forward_step(c):   # the forward alone (set-up + forward kernel), nothing kept for a backward
                    def step():
                        with torch.no_grad():
                            nr.soft_render(leaf, c, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip')
                    return step
                mf, mk = measure(forward_step(cleaf)), measure(forward_step(kleaf))
                row(base, 'soft_render_forward', 'hip', B, mf, sigma=sigma)
                row(base, 'soft_render_corners_forward', 'hip', B, mk, sigma=sigma, corners_over_flat=round(mk[0] / mf[0], 3))

            def sil_step():
                leaf.grad = None
                nr.soft_silhouettes(leaf, S, sigma, renderer.near, renderer.far, implementation='hip').backward(up[:, 3])
            row(base, 'soft_silhouettes', 'hip', B, measure(sil_step), sigma=sigma)
            if args.no_torch:
                continue
            Bt = min(args.torch_batch, B)
            small, csmall = projected[:Bt].clone().requires_grad_(True), colors[:Bt].clone().requires_grad_(True)
            out_t = [None]

            def torch_step():
                small.grad = csmall.grad = None
                out_t[0] = nr.soft_render(small, csmall, S, sigma, GAMMA, renderer.near, renderer.far, implementation='torch')
                out_t[0].backward(up[:Bt])
            mt = measure(torch_step, args.torch_steps)
            hs, hc = projected[:Bt].clone().requires_grad_(True), colors[:Bt].clone().requires_grad_(True)
            out_h = nr.soft_render(hs, hc, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip')
            out_h.backward(up[:Bt])
            row(base, 'soft_render', 'torch', Bt, mt, sigma=sigma,
                torch_over_hip_per_image=round((mt[0] / Bt) / (m[0] / B), 1),
                max_abs_diff_rgba=float((out_h.detach() - out_t[0].detach()).abs().max()),
                max_abs_diff_grad_faces=float((hs.grad - small.grad).abs().max()),
                max_abs_diff_grad_colors=float((hc.grad - csmall.grad).abs().max()))
            del small, csmall, hs, hc, out_h
            out_t[0] = None
            torch.cuda.empty_cache()
            if args.corners:
                small, ksmall = projected[:Bt].clone().requires_grad_(True), corner_colors[:Bt].clone().requires_grad_(True)

                def torch_corner_step():
                    small.grad = ksmall.grad = None
                    out_t[0] = nr.soft_render(small, ksmall, S, sigma, GAMMA, renderer.near, renderer.far, implementation='torch')
                    out_t[0].backward(up[:Bt])
                mt = measure(torch_corner_step, args.torch_steps)
                hs, hc = projected[:Bt].clone().requires_grad_(True), corner_colors[:Bt].clone().requires_grad_(True)
                out_h = nr.soft_render(hs, hc, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip')
                out_h.backward(up[:Bt])
                row(base, 'soft_render_corners', 'torch', Bt, mt, sigma=sigma,
                    torch_over_hip_per_image=round((mt[0] / Bt) / (mc[0] / B), 1),
                    max_abs_diff_rgba=float((out_h.detach() - out_t[0].detach()).abs().max()),
                    max_abs_diff_grad_faces=float((hs.grad - small.grad).abs().max()),
                    max_abs_diff_grad_colors=float((hc.grad - ksmall.grad).abs().max()))
                del small, ksmall, hs, hc, out_h
                out_t[0] = None
                torch.cuda.empty_cache()

        cubes = colors[:, :, None, None, None, :].expand(B, F, 2, 2, 2, 3).contiguous().requires_grad_(True)
        cleaf = colors.clone().requires_grad_(True)

        def hard_step():
            vertices.grad = cubes.grad = None
            renderer.render(vertices, faces, cubes).backward(up[:, :3])

        def soft_step():
            vertices.grad = cleaf.grad = None
            renderer.render_soft(vertices, faces, cleaf).backward(up)
        row(base, 'render', 'hip', B, measure(hard_step))
        row(base, 'render_soft', 'hip', B, measure(soft_step), sigma=renderer.soft_sigma)
        if args.corners:
            vcol = torch.tensor(rng.uniform(0, 1, (int(v.shape[0]), 3)).astype(np.float32), device=dev, requires_grad=True)

            def per_pixel_step():
                vertices.grad = vcol.grad = None
                renderer.render_soft(vertices, faces, nr.VertexColors(vcol), per_pixel=True).backward(up)
            row(base, 'render_soft_per_pixel', 'hip', B, measure(per_pixel_step), sigma=renderer.soft_sigma)

    if args.corners:   # many small faces: one icosphere(5) at 256 x 256
        S, sigma = 256, 1e-4
        sv, sf = nr.icosphere(5, 0.8)
        F = int(sf.shape[0])
        renderer = nr.Renderer()
        renderer.image_size = S
        renderer.eye = nr.get_points_from_angles(2.732, 30.0, 40.0)
        with torch.no_grad():
            projected = renderer._frontend(sv[None].to(dev), sf[None].to(dev))[0][:, :F].contiguous()
        up = torch.tensor(rng.normal(size=(1, 4, S, S)).astype(np.float32), device=dev)
        base = {'mesh': 'icosphere(5)', 'faces': F, 'image_size': S, 'gamma': GAMMA}
        leaf = projected.clone().requires_grad_(True)
        times = {}
        for name, shape in (('soft_render', (1, F, 3)), ('soft_render_corners', (1, F, 3, 3))):
            cleaf = torch.tensor(rng.uniform(0, 1, shape).astype(np.float32), device=dev, requires_grad=True)

            def sphere_step():
                leaf.grad = cleaf.grad = None
                nr.soft_render(leaf, cleaf, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip').backward(up)
            times[name] = measure(sphere_step)
            more = {'corners_over_flat': round(times[name][0] / times['soft_render'][0], 3)} if name != 'soft_render' else {}
            row(base, name, 'hip', 1, times[name], sigma=sigma, **more)


if __name__ == '__main__':
    main()
