"""Smooth light on per-pixel UV images (Renderer.shading = 'smooth' with a UVImages) on config 4's per-GPU shape:

    python scripts/uv_smooth_timing.py            # one JSON line per case

The scene of scripts/uv_texture_timing.py: 64 meshes x 10 240 faces (a latitude / longitude sphere with per-mesh vertex
noise), 256 x 256, anti-aliasing off, fill_back off, one 1024 x 1024 image per mesh ('per_mesh') or one shared by the 64
('shared').  Reports ms per Renderer.render forward + backward with gradients to the images for shading 'flat'
('render_fwd_bwd_flat_ms': the same measurement as uv_texture_timing.py's render_fwd_bwd_per_pixel_ms) and 'smooth', and
vertex_light forward + backward on its own (gradients to the vertices).  The smooth render's excess over the flat one splits
into the vertex_light launches and the rasterizer's share; `smooth_with_vertex_grad` also sends the light's gradient back to
the vertices (what a geometry fit pays).

The backward's pixel stage alone, through the C ABI on the maps of one forward: nr_backward_uv_images_smooth against the
two-pass alternative it replaces -- nr_backward_uv_images (flat, one colour per face) plus nr_backward_corner_colors on the
same maps ('bwd_smooth_ms' / 'bwd_flat_ms' / 'bwd_corner_ms').  A `rocprofv3 --kernel-trace --stats` run of this script, in
a run of its own, gives the kernel times.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import neural_renderer_amd as nr
from neural_renderer_amd import _lib

B, TS, RES = 64, 4, 1024
N_LAT, N_LON = 64, 80   # 2 * 64 * 80 = 10 240 triangles
STEPS = int(os.environ.get('UV_STEPS', '10'))


def timeit(fn, n=STEPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def sphere():
    th = np.pi * np.arange(N_LAT + 1) / N_LAT
    ph = 2 * np.pi * np.arange(N_LON + 1) / N_LON
    T, P = np.meshgrid(th, ph, indexing='ij')
    v = np.stack((np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)), -1).reshape(-1, 3).astype(np.float32) * 0.6
    uv = np.stack((P / (2 * np.pi), 1 - T / np.pi), -1).reshape(-1, 2).astype(np.float32)
    faces = []
    for i in range(N_LAT):
        for j in range(N_LON):
            a = i * (N_LON + 1) + j
            b, c, d = a + 1, a + N_LON + 1, a + N_LON + 2
            faces += [(a, c, b), (b, c, d)]
    faces = np.array(faces, np.int32)
    return v, faces, uv[faces]


def main():
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    v, f, faces_uv = sphere()
    F = f.shape[0]
    layout = nr.UVLayout(faces_uv, np.zeros(F, np.int32), np.full((F, TS, TS, TS, 3), 0.5, np.float32), [(RES, RES)])
    vertices = torch.tensor(np.stack([v * (1 + 0.05 * rng.normal(size=(v.shape[0], 1))).astype(np.float32)
                                      for _ in range(B)]), device=dev)
    faces = torch.tensor(f, device=dev)[None].expand(B, -1, -1).contiguous()
    r = nr.Renderer()
    r.image_size = 256
    r.anti_aliasing = False
    r.fill_back = False
    r.eye = torch.tensor(np.stack([nr.get_points_from_angles(2.732, 30., 360.0 * i / B) for i in range(B)]),
                         dtype=torch.float32, device=dev)
    lib = _lib.load()
    S, P = r.image_size, RES * RES
    light_args = (r.light_intensity_ambient, r.light_intensity_directional, r.light_color_ambient,
                  r.light_color_directional, r.light_direction)
    vg = vertices.clone().requires_grad_(True)

    def light_fwd_bwd():
        vg.grad = None
        nr.vertex_light(vg, faces, *light_args, fill_back=False, smooth=True).square().sum().backward()
    vertex_light_ms = round(timeit(light_fwd_bwd), 3)
    for case in ('per_mesh', 'shared'):
        Bi = B if case == 'per_mesh' else 1
        image = torch.rand((Bi, RES, RES, 3), device=dev, requires_grad=True)
        shared = image[0] if Bi == 1 else image
        out = {'case': case, 'meshes': B, 'faces': F, 'image': [RES, RES], 'images': Bi, 'raster': S,
               'vertex_light_fwd_bwd_ms': vertex_light_ms}

        def render(shading, verts):
            def step():
                image.grad = None
                verts.grad = None
                r.shading = shading
                r.render(verts, faces, nr.UVImages(layout, [shared])).square().sum().backward()
            return step
        out['render_fwd_bwd_flat_ms'] = round(timeit(render('flat', vertices)), 3)
        out['render_fwd_bwd_smooth_ms'] = round(timeit(render('smooth', vertices)), 3)
        out['render_fwd_bwd_flat_2_ms'] = round(timeit(render('flat', vertices)), 3)      # (again: the spread of one process)
        out['render_fwd_bwd_smooth_with_vertex_grad_ms'] = round(timeit(render('smooth', vg)), 3)
        out['render_fwd_bwd_flat_with_vertex_grad_ms'] = round(timeit(render('flat', vg)), 3)
        assert r.last_frontend == 'fused'

        # the backward's pixel stage alone, on the maps of one forward
        with torch.no_grad():
            r.shading = 'smooth'
            pf = r._frontend(vertices, faces, fused=True)[0].contiguous()
            light9 = nr.vertex_light(vertices, faces, *light_args, fill_back=False, smooth=True).contiguous()
        fn = nr.Rasterize(S, r.near, r.far, r.rasterizer_eps, r.background_color, return_rgb=True)
        fn(pf, nr.UVImages(layout, [shared.detach()]), light9)
        light3 = light9[:, :, 0].contiguous()
        g = torch.rand((B, S, S, 3), device=dev)
        packed = shared.detach().reshape(Bi, P, 3).contiguous()
        st = layout._tensors(dev)
        uvs = _lib.UVImagesStruct(packed.data_ptr(), st['table'].data_ptr(), st['faces_uv'].data_ptr(),
                                  st['face_image'].data_ptr(), st['base'].data_ptr(), TS, 1, P, Bi)
        gi = torch.empty((Bi, P, 3), device=dev)
        gl9, gl3, gc = torch.empty_like(light9), torch.empty_like(light3), torch.empty_like(light9)
        stream = torch.cuda.current_stream(dev).cuda_stream
        maps = (fn.faces.data_ptr(), fn.face_index_map.data_ptr(), fn.weight_map.data_ptr(), fn.depth_map.data_ptr())
        wsb = max(lib.nr_backward_uv_images_smooth_workspace_bytes(B, F, P, Bi), lib.nr_backward_corner_colors_workspace_bytes(B, F))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def bwd_smooth():
            _lib.check(lib.nr_backward_uv_images_smooth(_lib.CornerLight(light9.data_ptr(), F, gl9.data_ptr()), uvs, *maps,
                                                        g.data_ptr(), gi.data_ptr(), B, F, S, r.rasterizer_eps,
                                                        ws.data_ptr(), wsb, stream), 'smooth')

        def bwd_flat():
            _lib.check(lib.nr_backward_uv_images(_lib.FaceLight(light3.data_ptr(), F, None, gl3.data_ptr()), uvs, *maps,
                                                 g.data_ptr(), gi.data_ptr(), B, F, S, r.rasterizer_eps, ws.data_ptr(),
                                                 wsb, stream), 'flat')

        def bwd_corner():
            _lib.check(lib.nr_backward_corner_colors(*maps, g.data_ptr(), None, gc.data_ptr(), B, F, S, ws.data_ptr(), wsb,
                                                     stream), 'corner')
        out['bwd_smooth_ms'] = round(timeit(bwd_smooth), 3)
        out['bwd_flat_ms'] = round(timeit(bwd_flat), 3)
        out['bwd_corner_ms'] = round(timeit(bwd_corner), 3)
        out['covered_pixels'] = int((fn.face_index_map >= 0).sum())
        print(json.dumps(out), flush=True)
        del image, gi, packed, ws
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
