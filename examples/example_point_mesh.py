"""
A fit in 3-D against the surface itself: a sphere is pulled onto a fixed point cloud by the point-to-mesh distance (not in
the reference's examples).

The target is a cloud on a dented ellipsoid, made once.  Every step scores the mesh against it with `point_mesh_distance` --
for every point of the cloud the nearest triangle, for every triangle the nearest point, no sampling of the surface and so no
sampling noise -- and the Laplacian and the flatness prior keep the surface smooth where the points leave it free.  Eager
steps; nothing is captured into a HIP graph.
"""
import argparse
import os

import torch

import neural_renderer


def target_cloud(num_points, device, seed=0):
    """points on an ellipsoid with a dent: [num_points, 3]"""
    generator = torch.Generator().manual_seed(seed)
    d = torch.randn((num_points, 3), generator=generator)
    d = d / d.norm(dim=1, keepdim=True)
    radius = 1.0 - 0.35 * torch.exp(-8.0 * (d - torch.tensor([0.0, 0.0, 1.0])).pow(2).sum(1))
    return (d * radius[:, None] * torch.tensor([0.9, 0.6, 0.5])).to(device)


def fit(target, steps, level=3, weight_laplacian=0.1, weight_flatness=1e-3, lr=5e-3, every=10, on_step=None):
    """-> (vertices [Nv,3], faces, the loss of every step)"""
    sphere, faces = neural_renderer.icosphere(level, 0.5, device=target.device)
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=lr)
    losses = []
    for i in range(steps):
        optimizer.zero_grad()
        distance = neural_renderer.point_mesh_distance(target, vertices, faces)
        laplacian = neural_renderer.laplacian_loss(vertices, faces)
        flatness = neural_renderer.flatness_loss(vertices, faces)
        loss = distance + weight_laplacian * laplacian + weight_flatness * flatness
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  (point-mesh %.6f, laplacian %.5f, flatness %.4f)'
                  % (i, losses[-1], float(distance.detach()), float(laplacian.detach()), float(flatness.detach())), flush=True)
        if on_step is not None:
            on_step(i, losses[-1])
    return vertices.detach(), faces, losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=300)
    parser.add_argument('-oo', '--filename_output', type=str, default='./examples/data/example_point_mesh_result.obj')
    parser.add_argument('-n', '--num_points', type=int, default=4096)
    parser.add_argument('-g', '--gpu', type=int, default=0)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)
    vertices, faces, losses = fit(target_cloud(args.num_points, device), args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.filename_output)), exist_ok=True)
    neural_renderer.save_obj(args.filename_output, vertices.cpu().numpy(), faces.cpu().numpy())
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))


if __name__ == '__main__':
    run()
