"""
A fit in 3-D with the two priors that keep the triangulation itself in shape (not in the reference's examples): a sphere is
pulled onto a fixed point cloud by the point-to-mesh distance, once with the edge-length loss and once without it.

The point-to-mesh distance constrains where the surface is, not how its triangles are spread over it: left alone, the fit
stretches the triangles near the dent of the target and squeezes others into slivers.  `edge_length_loss` with the sphere's own
edge lengths as rest lengths -- `edge_lengths(sphere, faces)`, scaled -- holds every edge near its share, and
`cotangent_laplacian_loss` penalises bending without sliding the vertices along the surface, as the uniform Laplacian would on
an irregular triangulation.  The script prints the ratio of the longest to the shortest edge of both results.  Eager steps;
nothing is captured into a HIP graph.
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


def edge_ratio(vertices, faces):
    """longest / shortest edge of a mesh"""
    lengths = neural_renderer.edge_lengths(vertices.detach(), faces)
    return float(lengths.max() / lengths.min())


def fit(target, steps, level=3, weight_edge=0.05, weight_cotangent=0.02, lr=5e-3, every=10, on_step=None):
    """-> (vertices [Nv,3], faces, the loss of every step); weight_edge = 0 leaves the edge term out"""
    sphere, faces = neural_renderer.icosphere(level, 0.5, device=target.device)
    # rest lengths: the template's own, scaled by the ratio of the target's extent to the template's
    scale = float(target.norm(dim=1).mean() / sphere.norm(dim=1).mean())
    rest = neural_renderer.edge_lengths(sphere, faces).detach() * scale
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=lr)
    losses = []
    for i in range(steps):
        optimizer.zero_grad()
        distance = neural_renderer.point_mesh_distance(target, vertices, faces)
        cotangent = neural_renderer.cotangent_laplacian_loss(vertices, faces)
        edge = neural_renderer.edge_length_loss(vertices, faces, target=rest)
        loss = distance + weight_cotangent * cotangent
        if weight_edge:
            loss = loss + weight_edge * edge
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        terms = (float(distance.detach()), float(edge.detach()), float(cotangent.detach()))
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  (point-mesh %.6f, edge length %.5f, cotangent laplacian %.5f)' % ((i, losses[-1]) + terms),
                  flush=True)
        if on_step is not None:
            on_step(i, losses[-1], terms)
    return vertices.detach(), faces, losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=300)
    parser.add_argument('-oo', '--filename_output', type=str, default='./examples/data/example_edge_regularizers_result.obj')
    parser.add_argument('-n', '--num_points', type=int, default=4096)
    parser.add_argument('-g', '--gpu', type=int, default=0)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)
    target = target_cloud(args.num_points, device)
    print('with the edge-length term:')
    vertices, faces, losses = fit(target, args.steps)
    print('without it:')
    free, _, free_losses = fit(target, args.steps, weight_edge=0.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.filename_output)), exist_ok=True)
    neural_renderer.save_obj(args.filename_output, vertices.cpu().numpy(), faces.cpu().numpy())
    print('loss %.6f -> %.6f with the edge term, %.6f -> %.6f without' % (losses[0], losses[-1], free_losses[0], free_losses[-1]))
    print('longest / shortest edge: %.3f with the edge term, %.3f without' % (edge_ratio(vertices, faces), edge_ratio(free, faces)))


if __name__ == '__main__':
    run()
