"""
Smooth light on a UV-textured mesh (not in the reference): a coarse latitude / longitude sphere with a checkerboard image,
sampled per pixel, drawn with the light computed per face ('flat') and at the vertices ('smooth') side by side.

    python examples/example_uv_smooth.py
"""
import argparse
import os

import numpy as np
import torch

import neural_renderer
from example_io import save_image


def sphere(n_lat, n_lon):
    """vertices [Nv,3], faces [Nf,3] and the uv triangle of every face [Nf,3,2]: u is the longitude, v the latitude."""
    theta, phi = np.meshgrid(np.pi * np.arange(n_lat + 1) / n_lat, 2 * np.pi * np.arange(n_lon + 1) / n_lon, indexing='ij')
    vertices = np.stack((np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)), -1).reshape(-1, 3)
    uv = np.stack((phi / (2 * np.pi), 1 - theta / np.pi), -1).reshape(-1, 2)
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a = i * (n_lon + 1) + j
            b, c, d = a + 1, a + n_lon + 1, a + n_lon + 2
            faces += [(a, b, c), (b, d, c)]
    faces = np.array(faces, np.int32)
    return vertices.astype(np.float32), faces, uv.astype(np.float32)[faces]


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('-o', '--filename_output', type=str, default='./examples/data/example_uv_smooth.png')
    parser.add_argument('-g', '--gpu', type=int, default=0)
    parser.add_argument('--n_lat', type=int, default=8)
    parser.add_argument('--n_lon', type=int, default=16)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)

    vertices, faces, faces_uv = sphere(args.n_lat, args.n_lon)
    rows, cols = np.meshgrid(np.arange(64), np.arange(128), indexing='ij')
    board = (((rows // 8) + (cols // 8)) % 2).astype(np.float32)
    image = np.stack((0.1 + 0.8 * board, 0.2 + 0.6 * (1 - board), np.full_like(board, 0.5)), axis=2)

    # every face samples image 0; `base` would colour faces without an image
    num_faces = len(faces)
    layout = neural_renderer.UVLayout(faces_uv, np.zeros(num_faces, np.int32),
                                      np.full((num_faces, 2, 2, 2, 3), 0.5, np.float32), [image.shape[:2]])
    textures = neural_renderer.UVImages(layout, [torch.from_numpy(image).to(device)])
    vertices = torch.from_numpy(vertices).to(device)[None]
    faces = torch.from_numpy(faces).to(device)[None]

    renderer = neural_renderer.Renderer()
    renderer.image_size = 256
    renderer.eye = neural_renderer.get_points_from_angles(2.732, 20, 30)
    renderer.light_direction = [0.3, 0.8, -0.52]
    images = []
    with torch.no_grad():
        for shading in ('flat', 'smooth'):
            renderer.shading = shading   # 'smooth': light from area-weighted vertex normals, interpolated at every pixel
            images.append(renderer.render(vertices, faces, textures)[0].permute(1, 2, 0).cpu().numpy())
    os.makedirs(os.path.dirname(os.path.abspath(args.filename_output)), exist_ok=True)
    save_image(np.concatenate(images, axis=1), args.filename_output)
    print('wrote', args.filename_output)


if __name__ == '__main__':
    run()
