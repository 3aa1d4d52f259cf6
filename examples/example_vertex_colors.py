"""
Vertex colours and smooth shading (not in the reference): fit per-vertex colours of the teapot to views of a coloured
teapot, then draw it flat- and smooth-shaded side by side.

    python examples/make_data.py && python examples/example_vertex_colors.py
"""
import argparse

import numpy as np
import torch

import neural_renderer
from example_io import save_image


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('-i', '--filename_input', type=str, default='./examples/data/teapot.obj')
    parser.add_argument('-o', '--filename_output', type=str, default='./examples/data/example_vertex_colors.png')
    parser.add_argument('-g', '--gpu', type=int, default=0)
    parser.add_argument('--steps', type=int, default=150)
    parser.add_argument('--views', type=int, default=8)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)

    vertices, faces = neural_renderer.load_obj(args.filename_input)
    B = args.views
    vertices = torch.from_numpy(vertices).to(device)[None].expand(B, -1, -1).contiguous()
    faces = torch.from_numpy(faces).to(device)[None].expand(B, -1, -1).contiguous()

    renderer = neural_renderer.Renderer()
    renderer.image_size = 128
    renderer.shading = 'smooth'   # light from area-weighted vertex normals, interpolated over each triangle
    renderer.eye = torch.tensor(np.stack([neural_renderer.get_points_from_angles(2.732, 30, 360.0 * i / B) for i in range(B)]),
                                dtype=torch.float32, device=device)

    # the target: a colour field that is linear in the position
    truth = (0.5 + 0.4 * vertices[0] @ torch.tensor([[0.9, -0.3, 0.2], [0.1, 0.8, -0.5], [-0.4, 0.3, 0.7]], device=device))
    truth = truth.clamp(0, 1)
    with torch.no_grad():
        target = renderer.render(vertices, faces, neural_renderer.VertexColors(truth))

    colors = torch.full_like(truth, 0.5).requires_grad_(True)   # [num_vertices, RGB], shared by the views
    optimizer = torch.optim.Adam([colors], lr=0.03)
    for step in range(args.steps):
        optimizer.zero_grad()
        loss = ((renderer.render(vertices, faces, neural_renderer.VertexColors(colors)) - target) ** 2).mean()
        loss.backward()
        optimizer.step()
        if step % 25 == 0 or step == args.steps - 1:
            print('step %3d  loss %.3e' % (step, float(loss.detach())))

    # the fitted teapot, flat and smooth, from the first view
    renderer.image_size = 256
    renderer.eye = renderer.eye[0]
    images = []
    with torch.no_grad():
        for shading in ('flat', 'smooth'):
            renderer.shading = shading
            image = renderer.render(vertices[:1], faces[:1], neural_renderer.VertexColors(colors.detach()))
            images.append(image[0].permute(1, 2, 0).cpu().numpy())
    save_image(np.concatenate(images, axis=1), args.filename_output)
    print('wrote', args.filename_output)


if __name__ == '__main__':
    run()
