"""
Fitting a sphere to a silhouette it does not touch, with the soft silhouette (not in the reference's examples).

The target is the silhouette of the same sphere moved so far sideways -- and as far upwards -- that the two do not overlap
and share no pixel row and no pixel column.  The rasterizer's approximate gradient exists only where an edge, swept along its
row or its column, reaches a pixel whose colour differs; here no such pixel carries a loss gradient: through
render_silhouettes the vertex gradient is exactly zero and the fit cannot start.  render_soft_silhouettes gives every face
a coverage that decays with its screen-space distance and the exact gradient of that definition, which reaches the faces
from the target's pixels.

    python examples/example_soft_silhouette.py [steps]
"""
import sys

import torch

import neural_renderer


def run(steps=100, image_size=64, shift=0.9, radius=0.35):
    device = torch.device('cuda', 0)
    vertices, faces = neural_renderer.icosphere(2, radius)
    vertices, faces = vertices[None].to(device), faces[None].to(device)
    renderer = neural_renderer.Renderer()
    renderer.image_size = image_size
    renderer.eye = [0.0, 0.0, -2.732]
    renderer.soft_sigma = 3e-2   # wide enough for the two silhouettes to see each other
    with torch.no_grad():
        moved = vertices.clone()
        moved[:, :, :2] += shift
        target = renderer.render_silhouettes(moved, faces)
        start = renderer.render_silhouettes(vertices, faces)
    print('pixels shared by the start and the target silhouette: %d' % int((start * target > 0).sum()))

    # the hard silhouette: no gradient at all
    hard = vertices.clone().requires_grad_(True)
    neural_renderer.silhouette_iou_loss(renderer.render_silhouettes(hard, faces), target).sum().backward()
    print('hard silhouette: vertex gradient exactly zero at step 0: %s' % (not bool(hard.grad.any())))

    soft = vertices.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([soft], lr=1e-2)
    for i in range(steps):
        optimizer.zero_grad()
        iou = neural_renderer.silhouette_iou_loss(renderer.render_soft_silhouettes(soft, faces), target).sum()
        loss = iou + 0.01 * neural_renderer.laplacian_loss(soft, faces).sum()
        loss.backward()
        optimizer.step()
        if i == 0 or i == steps - 1 or i % 10 == 0:
            print('soft step %3d loss %.5f' % (i, float(loss.detach())))
    with torch.no_grad():
        moved_by = (soft - vertices)[0, :, :2].mean(0)
    print('mean x, y moved by %.3f, %.3f of %.3f' % (float(moved_by[0]), float(moved_by[1]), shift))


if __name__ == '__main__':
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
