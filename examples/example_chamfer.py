"""
A fit in 3-D, without a renderer: a subdivided sphere is pulled onto points sampled from the teapot (not in the
reference's examples).

The target is a point cloud drawn once from the teapot's surface.  In every step new points are drawn on the current mesh
(`sample_surface_points`: differentiable in the vertices) and scored against the target by the chamfer distance; the
Laplacian and the flatness prior keep the surface smooth where the points leave it free.  The learnable vertices are those
of `icosphere(2)`; the mesh that is sampled is their Loop subdivision, so a smooth surface moves with few parameters.
"""
import argparse

import torch

import neural_renderer


def fit(vertices_obj, faces_obj, steps, num_points=4096, levels=1, weight_laplacian=0.1, weight_flatness=1e-3, lr=1e-2,
        seed=0, every=10, on_step=None):
    """-> (coarse vertices [Nv,3], fine faces, the loss of every step)"""
    device = vertices_obj.device
    generator = torch.Generator(device=device).manual_seed(seed)
    with torch.no_grad():
        target, _ = neural_renderer.sample_surface_points(vertices_obj, faces_obj, num_points, generator)
    sphere, faces = neural_renderer.icosphere(2, 0.5, device=device)
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=lr)
    losses = []
    fine_faces = neural_renderer.subdivision(faces, vertices.shape[0], levels).faces
    for i in range(steps):
        optimizer.zero_grad()
        fine, fine_faces = neural_renderer.subdivide(vertices, faces, levels)
        points, _ = neural_renderer.sample_surface_points(fine, fine_faces, num_points, generator)
        chamfer = neural_renderer.chamfer_distance(points, target)
        laplacian = neural_renderer.laplacian_loss(fine, fine_faces)
        flatness = neural_renderer.flatness_loss(fine, fine_faces)
        loss = chamfer + weight_laplacian * laplacian + weight_flatness * flatness
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  (chamfer %.6f, laplacian %.5f, flatness %.4f)'
                  % (i, losses[-1], float(chamfer.detach()), float(laplacian.detach()), float(flatness.detach())), flush=True)
        if on_step is not None:
            on_step(i, losses[-1])
    return vertices.detach(), fine_faces, losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=300)
    parser.add_argument('-io', '--filename_obj', type=str, default='./examples/data/teapot.obj')
    parser.add_argument('-oo', '--filename_output', type=str, default='./examples/data/example_chamfer_result.obj')
    parser.add_argument('-n', '--num_points', type=int, default=4096)
    parser.add_argument('-g', '--gpu', type=int, default=0)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)
    vertices_obj, faces_obj = neural_renderer.load_obj(args.filename_obj)
    vertices, fine_faces, losses = fit(torch.from_numpy(vertices_obj).to(device), torch.from_numpy(faces_obj).to(device),
                                       args.steps, args.num_points)
    with torch.no_grad():
        fine, _ = neural_renderer.subdivide(vertices, neural_renderer.icosphere(2, 0.5, device=device)[1], 1)
    neural_renderer.save_obj(args.filename_output, fine.cpu().numpy(), fine_faces.cpu().numpy())
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))


if __name__ == '__main__':
    run()
