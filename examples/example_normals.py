"""
A fit on normal maps (not in the reference's examples): the vertices of a sphere are fitted to the normal maps and
silhouettes of a deformed sphere seen from a handful of views.

The target is rendered once from a squashed, bulged `icosphere(2)`: `Renderer.render_normals` with smooth shading gives, per
view, the camera-space normal at every pixel, the silhouette and nothing else -- what a normal estimator delivers for a
photograph.  The fit starts from the undeformed sphere; its loss is the squared error of the normal maps inside the target's
silhouette (`squared_error_loss(normals, target, mask)`), the silhouette IoU, and the Laplacian and flatness priors.
"""
import argparse

import torch

import neural_renderer


def deform(vertices):
    """The target shape: the sphere squashed along y, with a bulge towards +x."""
    x, y, z = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    bulge = 1.0 + 0.35 * torch.exp(-((x - 0.5) ** 2 + y ** 2 + z ** 2) / 0.08)
    return torch.stack((x * bulge, 0.7 * y, z * (1.0 + 0.2 * y)), dim=1)


def fit(steps, views=4, image_size=64, weight_iou=1.0, weight_laplacian=2.0, weight_flatness=5e-3, lr=5e-3, every=10,
        device='cuda', on_step=None):
    """-> (fitted vertices [Nv,3], faces [Nf,3], the loss of every step)"""
    sphere, faces = neural_renderer.icosphere(2, 0.5, device=device)
    faces_b = faces[None].expand(views, -1, -1).contiguous()
    renderer = neural_renderer.Renderer()
    renderer.image_size = image_size
    renderer.shading = 'smooth'
    renderer.eye = torch.tensor([neural_renderer.get_points_from_angles(2.732, 20.0, 360.0 * i / views + 15.0)
                                 for i in range(views)], dtype=torch.float32, device=device)

    def render(vertices):
        out = renderer.render_normals(vertices[None].expand(views, -1, -1), faces_b, space='camera', return_dict=True)
        return out['normals'], out['alpha']
    with torch.no_grad():
        target, target_alpha = render(deform(sphere))
        mask = (target_alpha > 0.5).float()
    vertices = torch.nn.Parameter(sphere.clone())
    optimizer = torch.optim.Adam([vertices], lr=lr)
    losses = []
    for i in range(steps):
        optimizer.zero_grad()
        normals, alpha = render(vertices)
        error = neural_renderer.squared_error_loss(normals, target, mask).mean() / mask.mean() / image_size ** 2
        iou = neural_renderer.silhouette_iou_loss(alpha, target_alpha).mean()
        laplacian = neural_renderer.laplacian_loss(vertices, faces)
        flatness = neural_renderer.flatness_loss(vertices, faces)
        loss = error + weight_iou * iou + weight_laplacian * laplacian + weight_flatness * flatness
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if i % every == 0 or i == steps - 1:
            print('step %4d  loss %.6f  (normals %.6f, iou %.6f, laplacian %.5f, flatness %.4f)'
                  % (i, losses[-1], float(error.detach()), float(iou.detach()), float(laplacian.detach()),
                     float(flatness.detach())), flush=True)
        if on_step is not None:
            on_step(i, losses[-1])
    return vertices.detach(), faces, losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('steps', type=int, nargs='?', default=200)
    parser.add_argument('-oo', '--filename_output', type=str, default=None)
    parser.add_argument('-g', '--gpu', type=int, default=0)
    args = parser.parse_args()
    vertices, faces, losses = fit(args.steps, device=torch.device('cuda', args.gpu))
    if args.filename_output:
        neural_renderer.save_obj(args.filename_output, vertices.cpu().numpy(), faces.cpu().numpy())
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))


if __name__ == '__main__':
    run()
