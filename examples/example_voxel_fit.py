"""
A fit in 3-D against an occupancy grid: a sphere is pulled onto the voxels of a displaced, scaled ellipsoid through the
generalized winding number (not in the reference's examples).

The target is the hard voxel grid of an ellipsoid, made once with `voxelize`.  The winding number of a CLOSED mesh is 1
inside and 0 outside wherever the vertices are, so `voxelize(hard=False)` of the sphere has no gradient to fit with (it has
one on open and self-intersecting meshes).  The soft occupancy of a step is therefore sigmoid(-signed_distance / voxel size)
at the voxel centres: the winding number gives the sign, the point-to-mesh distance the gradient.  The two grids are
compared by their squared error, and the Laplacian prior keeps the surface smooth.  The voxel IoU of the hard grids, the
metric of single-image reconstruction, is printed before and after.  Eager steps; nothing is captured into a HIP graph.
"""
import argparse

import torch

import neural_renderer


def target_grid(grid_size, device):
    """the hard voxel grid [G,G,G] of an ellipsoid with half axes (0.7, 0.5, 0.4) centred at (0.1, -0.05, 0.1)"""
    sphere, faces = neural_renderer.icosphere(3, 1.0, device=device)
    ellipsoid = sphere * torch.tensor([0.7, 0.5, 0.4], device=device) + torch.tensor([0.1, -0.05, 0.1], device=device)
    return neural_renderer.voxelize(ellipsoid, faces, grid_size)


def fit(target, steps, level=2, weight_laplacian=0.05, lr=1e-2, every=10):
    """-> (vertices [Nv,3], faces, the voxel IoU before and after)"""
    grid_size = int(target.shape[0])
    sphere, faces = neural_renderer.icosphere(level, 0.4, device=target.device)
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=lr)
    centers = neural_renderer.voxel_centers(grid_size, device=target.device)
    voxel = 2.0 / grid_size
    before = float(neural_renderer.voxel_iou(neural_renderer.voxelize(vertices.detach(), faces, grid_size), target))
    for i in range(steps):
        optimizer.zero_grad()
        occupancy = torch.sigmoid(-neural_renderer.signed_distance(centers, vertices, faces) / voxel)
        error = (occupancy - target.reshape(-1)).pow(2).mean()
        laplacian = neural_renderer.laplacian_loss(vertices, faces)
        loss = error + weight_laplacian * laplacian
        loss.backward()
        optimizer.step()
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  (squared error %.6f, laplacian %.5f)'
                  % (i, float(loss.detach()), float(error.detach()), float(laplacian.detach())), flush=True)
    after = float(neural_renderer.voxel_iou(neural_renderer.voxelize(vertices.detach(), faces, grid_size), target))
    return vertices.detach(), faces, before, after


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=200)
    parser.add_argument('-s', '--grid_size', type=int, default=32, help='voxels per axis (a small value makes a quick run)')
    parser.add_argument('-oo', '--filename_output', type=str, default=None, help='write the fitted mesh to this .obj')
    parser.add_argument('-g', '--gpu', type=int, default=0)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)
    vertices, faces, before, after = fit(target_grid(args.grid_size, device), args.steps)
    if args.filename_output:
        neural_renderer.save_obj(args.filename_output, vertices.cpu().numpy(), faces.cpu().numpy())
    print('voxel IoU %.4f -> %.4f' % (before, after))


if __name__ == '__main__':
    run()
