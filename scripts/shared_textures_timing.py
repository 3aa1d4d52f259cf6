"""Renderer.render forward + backward of ONE mesh seen from 64 views, with the texture cubes expanded to the batch or shared
by it (textures [1,Nf,ts,ts,ts,3]; include/nr_hip.h: NR_FLAG_SHARED_TEXTURES, nr_backward_textures_shared):

    python scripts/shared_textures_timing.py            # one JSON line per scene

Scenes: the teapot at texture_size 4 and 8, and config 4's mesh shape (an icosphere of 5 120 faces, fill_back -> 10 240) at
texture_size 4; 256 x 256, no anti-aliasing, vertices AND the [Nf,ts,ts,ts,3] texture parameter receiving gradients.
Variants: `expand` -- parameter[None].expand(B, ...) into lit, duplicated textures (Renderer.face_light = False);
`face_light_expand` -- the same expanded cubes with per-face light colours (face_light = True); `shared` -- parameter[None].
Reports ms per render + backward, ms per render, the peak torch memory of a step, and the largest difference of the
parameter's and the vertices' gradient from the `face_light_expand` variant.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import bench
import neural_renderer_amd as nr

VARIANTS = os.environ.get('ST_VARIANTS', 'expand,face_light_expand,shared').split(',')  # (development: one variant for a trace)


def timeit(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def scene(name, vertices, faces, ts, B, image_size):
    dev = vertices.device
    out = {'scene': name, 'B': B, 'faces': int(faces.shape[0]), 'ts': ts, 'image_size': image_size}
    param0 = torch.rand((faces.shape[0], ts, ts, ts, 3), device=dev)
    fb = faces[None].expand(B, *faces.shape).contiguous()
    keep = {}
    for variant in VARIANTS:
        r = nr.Renderer()
        r.image_size = image_size
        r.anti_aliasing = False
        r.face_light = variant != 'expand'
        r.eye = torch.tensor([nr.get_points_from_angles(2.732, 30., 360.0 * i / B) for i in range(B)], dtype=torch.float32,
                             device=dev)
        v = vertices.clone().requires_grad_(True)
        p = param0.clone().requires_grad_(True)

        def step():
            v.grad = None
            p.grad = None
            t = p[None] if variant == 'shared' else p[None].expand(B, *p.shape)
            img = r.render(v[None].expand(B, *v.shape), fb, t)
            img.square().sum().backward()
            return img

        def fwd():
            with torch.no_grad():
                return r.render(v[None].expand(B, *v.shape), fb, p[None] if variant == 'shared' else p[None].expand(B, *p.shape))

        step()
        assert r.last_frontend == 'fused'
        keep[variant] = (v.grad.cpu(), p.grad.cpu())  # (off the device: not part of the peak below)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        out[variant] = {'fwd_bwd_ms': round(timeit(step), 3), 'fwd_ms': round(timeit(fwd), 3), 'peak_MB': round(peak / 1e6, 1)}
        del v, p
    if 'face_light_expand' in keep:
        ref = keep['face_light_expand']
        out['max_rel_diff'] = {k: {'grad_vertices': rel(g[0], ref[0]), 'grad_textures': rel(g[1], ref[1])}
                               for k, g in keep.items() if k != 'face_light_expand'}
    print(json.dumps(out), flush=True)


def main():
    dev = torch.device('cuda', 0)
    B = 64
    v, f = bench.load_teapot()
    v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    for ts in (4, 8):
        scene('teapot, %d views, ts%d' % (B, ts), v, f, ts, B, 256)
    from test_hip_parity import icosphere
    v0, f0 = icosphere(4)
    scene('C4 mesh shape (%d faces), %d views, ts4' % (f0.shape[0], B), torch.from_numpy((0.6 * v0).astype(np.float32)).to(dev),
          torch.from_numpy(f0.astype(np.int32)).to(dev), 4, B, 256)


if __name__ == '__main__':
    main()
