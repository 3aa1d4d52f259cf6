"""
Fitting two coloured, overlapping spheres to an image with the soft colour image (not in the reference's examples).

A red sphere stands in front of a smaller blue one and hides it.  In the target the blue sphere is the one in front.  The
rasterizer's approximate gradient knows nothing about occlusion: through render the vertices of the hidden sphere get a
gradient of exactly zero, and no z gets any.  render_soft aggregates the faces' colours by coverage and depth and has the
exact gradient of that definition, which reaches the hidden faces -- z included -- and the vertex colours.

    python examples/example_soft_render.py [steps]
"""
import sys

import torch

import neural_renderer


def scene(device):
    """-> vertices [1,Nv,3], faces [1,F,3], the number of vertices and faces of the front sphere"""
    v0, f0 = neural_renderer.icosphere(2, 0.6)
    v1, f1 = neural_renderer.icosphere(2, 0.35)
    v1 = v1 + torch.tensor([0.0, 0.0, 1.0])   # behind the first, seen from (0, 0, -2.732)
    return torch.cat((v0, v1))[None].to(device), torch.cat((f0, f1 + v0.shape[0]))[None].to(device), v0.shape[0], f0.shape[0]


def run(steps=100, image_size=64):
    device = torch.device('cuda', 0)
    vertices, faces, nv, nf = scene(device)
    colors = torch.zeros(vertices.shape[1], 3, device=device)
    colors[:nv, 0] = 1.0   # the front sphere red,
    colors[nv:, 2] = 1.0   # the hidden one blue
    renderer = neural_renderer.Renderer()
    renderer.image_size = image_size
    renderer.eye = [0.0, 0.0, -2.732]
    renderer.soft_sigma = 1e-3
    renderer.soft_gamma = 1e-2   # in units of (far - z) / (far - near): the two spheres are 0.01 apart
    with torch.no_grad():
        moved = vertices.clone()
        moved[:, nv:, 2] -= 1.8   # the blue sphere in front, its colours a little lighter
        target_colors = colors.clone()
        target_colors[nv:, 1] = 0.4
        target = renderer.render_soft(moved, faces, neural_renderer.VertexColors(target_colors))[:, :3]

    # the rasterizer: nothing for the hidden sphere
    hard = vertices.clone().requires_grad_(True)
    cubes = colors[faces[0].long()].mean(1)[None, :, None, None, None, :].expand(1, faces.shape[1], 2, 2, 2, 3).contiguous()
    neural_renderer.squared_error_loss(renderer.render(hard, faces, cubes), target).sum().backward()
    print('render: gradient of the hidden sphere\'s vertices exactly zero at step 0: %s' % (not bool(hard.grad[:, nv:].any())))

    soft = vertices.clone().requires_grad_(True)
    vertex_colors = colors.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([soft, vertex_colors], lr=5e-3)
    for i in range(steps):
        optimizer.zero_grad()
        image = renderer.render_soft(soft, faces, neural_renderer.VertexColors(vertex_colors))[:, :3]
        loss = neural_renderer.squared_error_loss(image, target).sum()
        loss.backward()
        if i == 0:
            print('render_soft: the hidden sphere\'s z gradient is non-zero at step 0: %s' % bool(soft.grad[:, nv:, 2].any()))
        optimizer.step()
        if i == 0 or i == steps - 1 or i % 10 == 0:
            print('soft step %3d loss %.5f' % (i, float(loss.detach())))
    with torch.no_grad():
        dz = (soft - vertices)[0, :, 2]
    print('mean z moved: front sphere %+.3f, hidden sphere %+.3f' % (float(dz[:nv].mean()), float(dz[nv:].mean())))


if __name__ == '__main__':
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
