"""
A fit whose unknown is a grid of signed distances (DMTet / MeshSDF style; not in the reference's examples): a 24^3 grid that
starts as a sphere is fitted to the teapot's vertices as a point cloud.

Every step extracts the zero set of the grid with `extract_isosurface` (marching tetrahedra; the topology may change from
step to step), places the vertices with `IsoSurface.vertices` -- differentiable in the grid values --, scores the mesh with
`point_mesh_distance` plus a small `laplacian_loss`, and Adam moves the grid values.  Every new `faces` tensor makes the mesh
operators rebuild their host tables, which are cached on the index tensor (3-100 ms per topology): a fit like this one pays that
in every step.  Eager steps; the extraction reads its counts back, so nothing here can be captured into a HIP graph.
"""
import argparse
import os

import torch

import neural_renderer


def sphere_grid(size, radius, bounds, device):
    """the signed distance to a sphere at the nodes of `voxel_centers`: [size, size, size]"""
    centres = neural_renderer.voxel_centers(size, bounds, device=device)
    return (centres.norm(dim=1) - radius).reshape(size, size, size)


def fit(target, steps, size=24, bounds=(-1.1, 1.1), weight_laplacian=0.02, lr=5e-3, every=1, on_step=None):
    """-> (vertices [Nv,3], faces, the loss of every step)"""
    values = torch.nn.Parameter(sphere_grid(size, 0.6, bounds, target.device))
    optimizer = torch.optim.Adam([values], lr=lr)
    losses = []
    for i in range(steps):
        optimizer.zero_grad()
        surface = neural_renderer.extract_isosurface(values)
        vertices = surface.vertices(values, bounds)
        distance = neural_renderer.point_mesh_distance(target, vertices, surface.faces)
        laplacian = neural_renderer.laplacian_loss(vertices, surface.faces)
        loss = distance + weight_laplacian * laplacian
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  faces %d  (point-mesh %.6f, laplacian %.5f)'
                  % (i, losses[-1], surface.num_faces, float(distance.detach()), float(laplacian.detach())), flush=True)
        if on_step is not None:
            on_step(i, losses[-1])
    with torch.no_grad():
        surface = neural_renderer.extract_isosurface(values)
        return surface.vertices(values, bounds), surface.faces, losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=200)
    parser.add_argument('-io', '--filename_obj', type=str, default='./examples/data/teapot.obj')
    parser.add_argument('-oo', '--filename_output', type=str, default='./examples/data/example_isosurface_fit_result.obj')
    parser.add_argument('-s', '--grid_size', type=int, default=24)
    parser.add_argument('-g', '--gpu', type=int, default=0, help='-1: the CPU (the plain-torch paths)')
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu) if args.gpu >= 0 else torch.device('cpu')
    vertices_obj, _ = neural_renderer.load_obj(args.filename_obj)
    vertices, faces, losses = fit(torch.from_numpy(vertices_obj).to(device), args.steps, args.grid_size)
    os.makedirs(os.path.dirname(os.path.abspath(args.filename_output)), exist_ok=True)
    neural_renderer.save_obj(args.filename_output, vertices.cpu().numpy(), faces.cpu().numpy())
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))


if __name__ == '__main__':
    run()
