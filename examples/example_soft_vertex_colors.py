"""
Fitting vertex colours and vertices through the soft colour image with colours interpolated per pixel (not in the
reference's examples).

The target is a sphere whose colour varies smoothly over its surface, under smooth (Gouraud) light, a little larger than the
grey sphere the fit starts from.  render_soft(per_pixel=True) hands soft_render the very corner colours render() would
rasterize -- vertex colours lit at the vertices -- and interpolates them perspective-correctly at every pixel; its exact
gradient reaches the vertex colours, and the vertices through coverage, depth AND colour.

    python examples/example_soft_vertex_colors.py [steps]
"""
import sys

import torch

import neural_renderer


def run(steps=100, image_size=64):
    device = torch.device('cuda', 0)
    vertices, faces = neural_renderer.icosphere(2, 0.7)
    vertices, faces = vertices[None].to(device), faces[None].to(device)
    renderer = neural_renderer.Renderer()
    renderer.image_size = image_size
    renderer.eye = neural_renderer.get_points_from_angles(2.732, 20, 30)
    renderer.shading = 'smooth'
    renderer.soft_sigma = 1e-3
    renderer.soft_gamma = 1e-2
    with torch.no_grad():
        target_colors = 0.5 + 0.5 * vertices[0] / 0.7          # a colour that follows the position on the sphere
        target = renderer.render_soft(1.15 * vertices, faces, neural_renderer.VertexColors(target_colors), per_pixel=True)

    fit = vertices.clone().requires_grad_(True)
    colors = torch.full_like(vertices[0], 0.5).requires_grad_(True)
    optimizer = torch.optim.Adam([fit, colors], lr=1e-2)
    for i in range(steps):
        optimizer.zero_grad()
        image = renderer.render_soft(fit, faces, neural_renderer.VertexColors(colors), per_pixel=True)
        loss = neural_renderer.squared_error_loss(image, target).sum()
        loss.backward()
        optimizer.step()
        if i == 0 or i == steps - 1 or i % 10 == 0:
            print('soft step %3d loss %.5f' % (i, float(loss.detach())))
    with torch.no_grad():
        print('mean colour error %.3f -> %.3f, mean radius 0.700 -> %.3f (target 0.805)'
              % (float((0.5 - target_colors).abs().mean()), float((colors - target_colors).abs().mean()),
                 float(fit[0].norm(dim=1).mean())))


if __name__ == '__main__':
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
