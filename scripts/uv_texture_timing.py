"""Learnable UV texture images (neural_renderer_amd/uv_textures.py) on config 4's per-GPU shape:

    python scripts/uv_texture_timing.py            # one JSON line per case

64 meshes x 10 240 faces (a latitude / longitude sphere, uv = (longitude, latitude), per-mesh vertex noise), ts 4, one
1024 x 1024 image per mesh ('per_mesh') or one image shared by the 64 ('shared').  Reports ms per call of the forward bake,
the backward bake and the map build, and Renderer.render forward + backward (256 x 256, anti-aliasing off, fill_back off so
that the rasterizer sees the 10 240 faces) with the bake in front (gradients to the images) and without it (gradients to
[64,F,4,4,4,3] textures directly).  Also prints the algorithmic bytes of the two bake kernels (forward: texels x 12 written
+ each image read once; backward: grad_textures read once + the map read once + the image gradients written): divide by
the kernel times of a `rocprofv3 --kernel-trace --stats` run of this script for their share of HBM bandwidth.

Per-pixel sampling (UVImages, include/nr_hip.h nr_forward_rasterize_uv / nr_backward_uv_images) of the same images on the
same views: Renderer.render forward + backward ('render_fwd_bwd_per_pixel_ms') and the algorithmic bytes of its backward's
kernels -- k_uv_pixel_backward reads face_index_map everywhere, weights, depth and the upstream gradient at the covered
pixels (each image pixel's double sum read-modify-written at least once is counted with k_uv_round); the zero fill writes
the double sums once, k_uv_round reads them once and writes the float gradients.  The forward's image reads ride in the
resolve pass (4 reads per covered pixel, mostly from L2).
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
    lib = nr._lib.load()
    texels = B * F * TS ** 3
    P = RES * RES
    for case in ('per_mesh', 'shared'):
        Bi = B if case == 'per_mesh' else 1
        image = torch.rand((Bi, RES, RES, 3), device=dev, requires_grad=True)
        out = {'case': case, 'meshes': B, 'faces': F, 'ts': TS, 'image': [RES, RES], 'images': Bi}

        def bake_fwd():
            with torch.no_grad():
                return nr.bake_uv_textures([image], layout)
        textures = bake_fwd()
        layout._device.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row_ptr, entry_texel, entry_weight = layout.inverse_map(dev)
        torch.cuda.synchronize()
        out['map_build_first_ms'] = round((time.perf_counter() - t0) * 1e3, 3)

        def map_build():
            layout._device[dev].pop('row_ptr')
            layout.inverse_map(dev)
        out['map_build_ms'] = round(timeit(map_build, 3), 3)
        row_ptr, entry_texel, entry_weight = layout.inverse_map(dev)
        g = torch.rand_like(textures)
        grad_images = torch.empty((Bi, P, 3), device=dev)

        def bake_bwd():
            nr._lib.check(lib.nr_bake_uv_textures_backward(g.data_ptr(), row_ptr.data_ptr(), entry_texel.data_ptr(),
                                                           entry_weight.data_ptr(), grad_images.data_ptr(), Bi, F, TS, P,
                                                           torch.cuda.current_stream(dev).cuda_stream), 'bwd')
        out['bake_fwd_ms'] = round(timeit(bake_fwd), 3)
        out['bake_bwd_ms'] = round(timeit(bake_bwd), 3)
        n_entries = int(row_ptr[-1])
        out['bytes_fwd'] = Bi * F * TS ** 3 * 12 + Bi * P * 12
        out['bytes_bwd'] = Bi * F * TS ** 3 * 12 + (P + 1) * 4 + n_entries * 8 + Bi * P * 12
        out['map_entries'] = n_entries
        out['texels'] = Bi * F * TS ** 3

        def render_with_bake():
            image.grad = None
            t = nr.bake_uv_textures([image], layout)
            if Bi == 1:
                t = t[0:1].expand(B, -1, -1, -1, -1, -1)
            r.render(vertices, faces, t).square().sum().backward()
        direct = torch.rand((B, F, TS, TS, TS, 3), device=dev, requires_grad=True)

        def render_direct():
            direct.grad = None
            r.render(vertices, faces, direct).square().sum().backward()
        shared = image[0] if Bi == 1 else image

        def render_per_pixel():
            image.grad = None
            r.render(vertices, faces, nr.UVImages(layout, [shared])).square().sum().backward()
        out['render_fwd_bwd_with_bake_ms'] = round(timeit(render_with_bake), 3)
        out['render_fwd_bwd_without_bake_ms'] = round(timeit(render_direct), 3)
        out['render_fwd_bwd_per_pixel_ms'] = round(timeit(render_per_pixel), 3)
        with torch.no_grad():
            covered = int((r.render_silhouettes(vertices, faces) > 0).sum())
        S = r.image_size
        out['covered_pixels'] = covered
        out['bytes_uv_pixel_bwd'] = B * S * S * 4 + covered * (12 + 4 + 12)
        out['bytes_uv_fill'] = (Bi * P * 3 + B * F * 3) * 8
        out['bytes_uv_round'] = (Bi * P * 3 + B * F * 3) * (8 + 4)
        out['texels_per_step'] = texels
        print(json.dumps(out), flush=True)
        del image, textures, g, grad_images, direct
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
