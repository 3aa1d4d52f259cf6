"""
Learning texture cubes through the soft colour image (not in the reference's examples).

An icosphere whose faces carry the library's native texture cubes [F, ts, ts, ts, 3] -- a colour pattern that varies inside
every face -- is rendered from a few views; grey cubes of the same size are then fitted to those views.
render_soft(vertices, faces, TextureCubes(t), per_pixel=True) samples a face's cube at every pixel with the rasterizer's
trilinear lookup, and its exact gradient reaches the texels through coverage and depth order alike.

    python examples/example_soft_cubes.py [steps]
"""
import os
import sys

import numpy as np
import torch

import neural_renderer
from example_io import save_image


def run(steps=100, image_size=64, views=4, texture_size=4, filename_output='./examples/data/example_soft_cubes.png'):
    device = torch.device('cuda', 0)
    vertices, faces = neural_renderer.icosphere(2, 0.8)
    num_faces, ts = int(faces.shape[0]), texture_size
    # the truth: a face's colour runs from red at its first corner over green at the second to blue at the third
    i, j, k = np.meshgrid(np.arange(ts), np.arange(ts), np.arange(ts), indexing='ij')
    ramp = np.stack((i, j, k), axis=3).astype(np.float32) / (ts - 1)
    truth = torch.from_numpy(np.broadcast_to(0.1 + 0.8 * ramp.clip(0, 1), (1, num_faces, ts, ts, ts, 3)).copy()).to(device)
    vertices = vertices.to(device)[None].expand(views, -1, -1).contiguous()
    faces = faces.to(device)[None].expand(views, -1, -1).contiguous()

    renderer = neural_renderer.Renderer()
    renderer.image_size = image_size
    renderer.eye = torch.tensor([neural_renderer.get_points_from_angles(2.732, 20.0, 360.0 * v / views) for v in range(views)],
                                dtype=torch.float32, device=device)
    renderer.soft_sigma = 1e-4
    renderer.soft_gamma = 1e-2
    with torch.no_grad():
        target = renderer.render_soft(vertices, faces, neural_renderer.TextureCubes(truth), per_pixel=True)

    textures = torch.full_like(truth, 0.5).requires_grad_(True)   # one set of cubes shared by the views
    optimizer = torch.optim.Adam([textures], lr=5e-2)
    for step in range(steps):
        optimizer.zero_grad()
        image = renderer.render_soft(vertices, faces, neural_renderer.TextureCubes(textures), per_pixel=True)
        loss = neural_renderer.squared_error_loss(image, target).sum()
        loss.backward()
        optimizer.step()
        if step == 0 or step == steps - 1 or step % 10 == 0:
            print('soft cubes step %3d loss %.5f' % (step, float(loss.detach())))
    with torch.no_grad():
        print('mean texel error %.3f -> %.3f' % (float((0.5 - truth).abs().mean()), float((textures - truth).abs().mean())))
        shown = renderer.render_soft(vertices, faces, neural_renderer.TextureCubes(textures), per_pixel=True)[0, :3]
    os.makedirs(os.path.dirname(os.path.abspath(filename_output)), exist_ok=True)
    save_image(np.concatenate((target[0, :3].permute(1, 2, 0).cpu().numpy(), shown.permute(1, 2, 0).cpu().numpy()), axis=1),
               filename_output)
    print('wrote', filename_output)


if __name__ == '__main__':
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
