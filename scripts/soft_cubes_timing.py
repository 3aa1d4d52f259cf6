"""Soft colour rendering with texture cubes sampled at the pixel, forward + backward: the nr_soft_cubes_* kernels against the
corner-colour kernels on the same geometry, against soft_render_cubes_torch, and the whole pipeline against Renderer.render
with the same cubes.

    python scripts/soft_cubes_timing.py            # one JSON line per row

Workloads: 64 teapot views (2 464 faces, no fill_back copies) at 256 x 256 and at 64 x 64 with sigma in (1e-5, 1e-4, 1e-3),
gamma 1e-2, random cubes [1, F, ts, ts, ts, 3] shared by the batch with ts in (2, 4, 8) and one random light colour per face
and image.  A step is soft_render_cubes on the projected faces followed by the backward with a fixed upstream gradient; the
gradient is asked of the faces, the light and the cubes (`soft_render_cubes`), and of the faces and the light alone
(`soft_render_cubes_no_texture_grad`: the same kernels without the cube sums -- the difference is what those cost).
`soft_render_corners` is soft_render with corner colours on the same projected faces, in the same process:
`cubes_over_corners` is the cube row's time over it.  The plain-torch path runs on `--torch-batch` views (default 1) and is
reported per image next to the HIP time per image, with the largest differences of that view's outputs.  Whole pipeline from
the vertices (ts = 4): Renderer.render_soft(TextureCubes, per_pixel=True) + backward and Renderer.render + backward with the
same cubes.  After a warm-up each row is timed in rounds between two host clock readings that end in a device synchronise;
the median round is reported.  One process; the first error ends it.  Informational: no threshold.
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
SIZES = (2, 4, 8)
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
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import neural_renderer_amd as nr
    if not torch.cuda.is_available():
        raise SystemExit('soft_cubes_timing: needs a GPU (a CPU run says nothing about the kernels)')
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
    cubes = {ts: torch.tensor(rng.uniform(0, 1, (1, F, ts, ts, ts, 3)).astype(np.float32), device=dev) for ts in SIZES}
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
        light = torch.tensor(rng.uniform(0.5, 1.5, (B, F, 3)).astype(np.float32), device=dev)
        corner_colors = torch.tensor(rng.uniform(0, 1, (B, F, 3, 3)).astype(np.float32), device=dev)
        up = torch.tensor(rng.normal(size=(B, 4, S, S)).astype(np.float32), device=dev)
        base = {'mesh': 'teapot', 'faces': F, 'image_size': S, 'gamma': GAMMA}

        for sigma in SIGMAS:
            leaf, lleaf, kleaf = (t.clone().requires_grad_(True) for t in (projected, light, corner_colors))

            def corner_step():
                leaf.grad = kleaf.grad = None
                nr.soft_render(leaf, kleaf, S, sigma, GAMMA, renderer.near, renderer.far, implementation='hip').backward(up)
            mc = measure(corner_step)
            row(base, 'soft_render_corners', 'hip', B, mc, sigma=sigma)
            for ts in SIZES:
                tleaf, fixed = cubes[ts].clone().requires_grad_(True), cubes[ts].clone()

                def cube_step(tex):
                    def step():
                        leaf.grad = lleaf.grad = tleaf.grad = None
                        nr.soft_render_cubes(leaf, tex, lleaf, S, sigma, GAMMA, renderer.near, renderer.far,
                                             implementation='hip').backward(up)
                    return step
                m = measure(cube_step(tleaf))
                row(base, 'soft_render_cubes', 'hip', B, m, sigma=sigma, ts=ts, cubes_over_corners=round(m[0] / mc[0], 3))
                mn = measure(cube_step(fixed))
                row(base, 'soft_render_cubes_no_texture_grad', 'hip', B, mn, sigma=sigma, ts=ts,
                    cubes_over_corners=round(mn[0] / mc[0], 3))
                if args.no_torch:
                    continue
                Bt = min(args.torch_batch, B)
                out = {}

                def one(implementation):
                    fs, ls, tx = projected[:Bt].clone().requires_grad_(True), light[:Bt].clone().requires_grad_(True), \
                        cubes[ts].clone().requires_grad_(True)

                    def step():
                        fs.grad = ls.grad = tx.grad = None
                        out[implementation] = nr.soft_render_cubes(fs, tx, ls, S, sigma, GAMMA, renderer.near, renderer.far,
                                                                   implementation=implementation)
                        out[implementation].backward(up[:Bt])
                    return step, (fs, ls, tx)
                t_step, t_leaves = one('torch')
                mt = measure(t_step, args.torch_steps)
                # the HIP path on the same views, for the per-image ratio and the differences
                h_step, h_leaves = one('hip')
                mh1 = measure(h_step)
                row(base, 'soft_render_cubes', 'torch', Bt, mt, sigma=sigma, ts=ts,
                    torch_over_hip_per_image=round((mt[0] / Bt) / (m[0] / B), 1),
                    torch_over_hip_same_views=round(mt[0] / mh1[0], 1),
                    max_abs_diff_rgba=float((out['hip'].detach() - out['torch'].detach()).abs().max()),
                    max_abs_diff_grad_faces=float((h_leaves[0].grad - t_leaves[0].grad).abs().max()),
                    max_abs_diff_grad_light=float((h_leaves[1].grad - t_leaves[1].grad).abs().max()),
                    max_abs_diff_grad_textures=float((h_leaves[2].grad - t_leaves[2].grad).abs().max()))
                del t_leaves, h_leaves
                out.clear()
                torch.cuda.empty_cache()

        tleaf = cubes[4].clone().requires_grad_(True)

        def hard_step():
            vertices.grad = tleaf.grad = None
            renderer.render(vertices, faces, tleaf).backward(up[:, :3])

        def soft_step():
            vertices.grad = tleaf.grad = None
            renderer.render_soft(vertices, faces, nr.TextureCubes(tleaf), per_pixel=True).backward(up)
        mh = measure(hard_step)
        row(base, 'render_cubes', 'hip', B, mh, ts=4)
        ms = measure(soft_step)
        row(base, 'render_soft_texture_cubes', 'hip', B, ms, ts=4, sigma=renderer.soft_sigma, soft_over_hard=round(ms[0] / mh[0], 3))


if __name__ == '__main__':
    main()
