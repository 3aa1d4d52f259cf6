"""Vertex colours (neural_renderer_amd/vertex_colors.py) against the texture_size 2 cube path, HIP-event ms per
Renderer.render + backward (256 x 256, anti-aliasing off, fill_back on; gradients to the vertices and to the colours /
textures):

    python scripts/vertex_color_timing.py            # one JSON line per shape

Shapes: 'headline' -- 64 views of the teapot (2 464 faces, 4 928 with fill_back), one mesh seen from 64 azimuths; 'config4' --
config 4's per-GPU shape, 64 distinct meshes of 5 120 faces (10 240 with fill_back; a latitude / longitude sphere with
per-mesh vertex noise).  Modes: 'vertex_flat' / 'vertex_smooth' (VertexColors [B,Nv,3], Renderer.shading) and 'cube_ts2'
(textures [B,Nf,2,2,2,3] with face_light = True) on the same geometry.  The kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of this script (VC_STEPS sets the timed steps per mode).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import neural_renderer_amd as nr

B, S = 64, 256
STEPS = int(os.environ.get('VC_STEPS', '20'))


def event_ms(fn, n=STEPS):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


def sphere(n_lat, n_lon):
    th = np.pi * np.arange(n_lat + 1) / n_lat
    ph = 2 * np.pi * np.arange(n_lon + 1) / n_lon
    T, P = np.meshgrid(th, ph, indexing='ij')
    v = np.stack((np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)), -1).reshape(-1, 3).astype(np.float32) * 0.6
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a = i * (n_lon + 1) + j
            b, c, d = a + 1, a + n_lon + 1, a + n_lon + 2
            faces += [(a, c, b), (b, c, d)]
    return v, np.array(faces, np.int32)


def shapes(dev):
    import helpers
    v, f = helpers.teapot()
    yield 'headline', torch.tensor(v, device=dev)[None].expand(B, -1, -1).contiguous(), f
    rng = np.random.default_rng(0)
    v, f = sphere(64, 40)
    yield 'config4', torch.tensor(np.stack([v * (1 + 0.05 * rng.normal(size=(v.shape[0], 1))).astype(np.float32)
                                            for _ in range(B)]), device=dev), f


def main():
    dev = torch.device('cuda', 0)
    for name, vertices, f in shapes(dev):
        vertices.requires_grad_(True)
        Nv, Nf = vertices.shape[1], f.shape[0]
        faces = torch.tensor(f, device=dev)[None].expand(B, -1, -1).contiguous()
        r = nr.Renderer()
        r.image_size = S
        r.anti_aliasing = False
        r.eye = torch.tensor(np.stack([nr.get_points_from_angles(2.732, 30., 360.0 * i / B) for i in range(B)]),
                             dtype=torch.float32, device=dev)
        colors = torch.rand((B, Nv, 3), device=dev, requires_grad=True)
        cubes = torch.rand((B, Nf, 2, 2, 2, 3), device=dev, requires_grad=True)
        out = {'shape': name, 'views': B, 'faces': Nf, 'vertices': Nv, 'image_size': S}

        def step(textures, shading, face_light):
            def run():
                vertices.grad = colors.grad = cubes.grad = None
                r.shading, r.face_light = shading, face_light
                r.render(vertices, faces, textures()).square().sum().backward()
            return run
        out['vertex_flat_ms'] = round(event_ms(step(lambda: nr.VertexColors(colors), 'flat', None)), 4)
        out['vertex_smooth_ms'] = round(event_ms(step(lambda: nr.VertexColors(colors), 'smooth', None)), 4)
        out['cube_ts2_ms'] = round(event_ms(step(lambda: cubes, 'flat', True)), 4)
        assert r.last_frontend == 'fused'
        r.shading = 'flat'
        with torch.no_grad():
            covered = int((r.render_silhouettes(vertices, faces) > 0).sum())
        out['covered_pixels'] = covered
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
