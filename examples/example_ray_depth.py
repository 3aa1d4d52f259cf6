"""
A fit against a range scan along the sensor's lines of sight: a sphere is pulled onto a synthetic scan by the difference of
the distances along its rays (not in the reference's examples).

The scan is a few hundred rays from three sensor positions, in directions that lie on no pixel grid, with the distance each
of them measured to a dented ellipsoid, made once.  Every step casts the same rays at the mesh with `ray_mesh_intersect` and
scores (t - t_scan)^2 on the rays that hit: a surface in front of the scanned one and a surface behind it are told apart,
which the unordered `point_mesh_distance` of the scanned points cannot do.  The Laplacian keeps the surface smooth where no
ray lands.  Eager steps; nothing is captured into a HIP graph.
"""
import argparse
import os

import torch

import neural_renderer


def range_scan(num_rays, device, seed=0):
    """-> (origins [R,3], directions [R,3] unit, t_scan [R]): rays from three sensors towards a dented ellipsoid, those that hit"""
    generator = torch.Generator().manual_seed(seed)
    sensors = torch.tensor([[0.0, 0.3, -3.0], [2.6, 0.8, 1.5], [-2.4, -1.0, 1.8]])
    origins = sensors[torch.randint(0, 3, (num_rays,), generator=generator)]
    aim = 0.45 * torch.randn((num_rays, 3), generator=generator)
    directions = aim - origins
    directions = directions / directions.norm(dim=1, keepdim=True)
    target, faces = neural_renderer.icosphere(4, 1.0)
    d = target / target.norm(dim=1, keepdim=True)
    radius = 1.0 - 0.35 * torch.exp(-8.0 * (d - torch.tensor([0.0, 0.0, -1.0])).pow(2).sum(1))
    target = d * radius[:, None] * torch.tensor([0.9, 0.6, 0.5])
    origins, directions, target, faces = (x.to(device) for x in (origins, directions, target, faces))
    with torch.no_grad():
        t_scan, ids, _ = neural_renderer.ray_mesh_intersect(origins, directions, target, faces)
    hit = ids >= 0
    return origins[hit], directions[hit], t_scan[hit]


def fit(scan, steps, level=3, weight_laplacian=0.1, lr=5e-3, every=10):
    """-> (vertices [Nv,3], faces, the loss of every step)"""
    origins, directions, t_scan = scan
    sphere, faces = neural_renderer.icosphere(level, 0.5, device=origins.device)
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=lr)
    losses = []
    for i in range(steps):
        optimizer.zero_grad()
        t, ids, _ = neural_renderer.ray_mesh_intersect(origins, directions, vertices, faces)
        hit = ids >= 0
        along = ((t - t_scan)[hit] ** 2).mean()
        laplacian = neural_renderer.laplacian_loss(vertices, faces)
        loss = along + weight_laplacian * laplacian
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  (along the rays %.6f on %d of %d rays, laplacian %.5f)'
                  % (i, losses[-1], float(along.detach()), int(hit.sum()), int(hit.numel()), float(laplacian.detach())), flush=True)
    return vertices.detach(), faces, losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=300)
    parser.add_argument('-oo', '--filename_output', type=str, default='./examples/data/example_ray_depth_result.obj')
    parser.add_argument('-n', '--num_rays', type=int, default=600)
    parser.add_argument('-g', '--gpu', type=int, default=0)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)
    vertices, faces, losses = fit(range_scan(args.num_rays, device), args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.filename_output)), exist_ok=True)
    neural_renderer.save_obj(args.filename_output, vertices.cpu().numpy(), faces.cpu().numpy())
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))


if __name__ == '__main__':
    run()
