"""
Learning a UV texture image through the soft colour image (not in the reference's examples).

A latitude / longitude sphere (the mesh of example_uv_smooth.py) with a checkerboard image is rendered from a few views; a
grey image of the same size is then fitted to those views.  render_soft(per_pixel=True) samples the UVTextures' image at every
pixel with the bake's bilinear lookup, and its exact gradient reaches the image pixels through coverage and depth order alike.

    python examples/example_soft_uv.py [steps]
"""
import os
import sys

import numpy as np
import torch

import neural_renderer
from example_io import save_image
from example_uv_smooth import sphere


def run(steps=100, image_size=64, views=4, filename_output='./examples/data/example_soft_uv.png'):
    device = torch.device('cuda', 0)
    vertices, faces, faces_uv = sphere(8, 16)
    rows, cols = np.meshgrid(np.arange(16), np.arange(32), indexing='ij')
    board = (((rows // 4) + (cols // 4)) % 2).astype(np.float32)
    truth = np.stack((0.1 + 0.8 * board, 0.2 + 0.6 * (1 - board), np.full_like(board, 0.5)), axis=2)
    num_faces = len(faces)
    layout = neural_renderer.UVLayout(faces_uv, np.zeros(num_faces, np.int32), np.full((num_faces, 2, 2, 2, 3), 0.5, np.float32),
                                      [truth.shape[:2]], images=[truth])
    vertices = torch.from_numpy(0.8 * vertices).to(device)[None].expand(views, -1, -1).contiguous()
    faces = torch.from_numpy(faces).to(device)[None].expand(views, -1, -1).contiguous()

    renderer = neural_renderer.Renderer()
    renderer.image_size = image_size
    renderer.eye = torch.tensor([neural_renderer.get_points_from_angles(2.732, 20.0, 360.0 * i / views) for i in range(views)],
                                dtype=torch.float32, device=device)
    renderer.soft_sigma = 1e-4
    renderer.soft_gamma = 1e-2
    target_textures = neural_renderer.UVTextures(layout).to(device)
    with torch.no_grad():
        target = renderer.render_soft(vertices, faces, target_textures.uv_images(), per_pixel=True)

    textures = neural_renderer.UVTextures(layout).to(device)
    with torch.no_grad():
        textures.images[0].fill_(0.5)
    optimizer = torch.optim.Adam(textures.parameters(), lr=5e-2)
    for i in range(steps):
        optimizer.zero_grad()
        image = renderer.render_soft(vertices, faces, textures.uv_images(), per_pixel=True)
        loss = neural_renderer.squared_error_loss(image, target).sum()
        loss.backward()
        optimizer.step()
        if i == 0 or i == steps - 1 or i % 10 == 0:
            print('soft uv step %3d loss %.5f' % (i, float(loss.detach())))
    with torch.no_grad():
        learned = textures.images[0].detach().clamp(0, 1).cpu().numpy()
        print('mean image error %.3f -> %.3f' % (float(np.abs(0.5 - truth).mean()), float(np.abs(learned - truth).mean())))
        shown = renderer.render_soft(vertices, faces, textures.uv_images(), per_pixel=True)[0, :3]
    os.makedirs(os.path.dirname(os.path.abspath(filename_output)), exist_ok=True)
    save_image(np.concatenate((target[0, :3].permute(1, 2, 0).cpu().numpy(), shown.permute(1, 2, 0).cpu().numpy()), axis=1),
               filename_output)
    print('wrote', filename_output)


if __name__ == '__main__':
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
