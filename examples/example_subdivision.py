"""
Coarse to fine: fitting a sphere to a silhouette, refining the mesh twice on the way (not in the reference's examples).

The rasterizer's approximate gradient moves a vertex only through the pixels next to its edges: a coarse mesh converges
fast but cannot hold detail, a fine one folds unless the priors are weighted heavily.  So the fit starts from
`icosphere(1)` -- 42 vertices --, and after each third of the steps the mesh is replaced by its Loop subdivision (162, then
642 vertices) and the fit continues.  The vertices are a new parameter after a refinement, so the optimiser is built anew.

The objective is the multi-scale silhouette IoU plus the Laplacian and the flatness prior, as in example_silhouette_iou.py.
"""
import argparse

import numpy as np
import torch
import torch.nn as nn
import tqdm

import neural_renderer
from example_io import make_gif, read_image


class Model(nn.Module):
    def __init__(self, filename_ref, weight_laplacian=0.03, weight_flatness=1e-4, levels=4, radius=0.5):
        super(Model, self).__init__()
        vertices, faces = neural_renderer.icosphere(1, radius)
        self.vertices = nn.Parameter(vertices[None, :, :])
        self.register_buffer('faces', faces[None, :, :])
        ref = read_image(filename_ref)
        if ref.ndim == 3:
            ref = ref.max(-1)
        self.register_buffer('image_ref', torch.from_numpy((ref > 0.5).astype(np.float32)))
        self.renderer = neural_renderer.Renderer()
        self.weight_laplacian, self.weight_flatness, self.levels = weight_laplacian, weight_flatness, levels

    @property
    def num_vertices(self):
        return self.vertices.shape[1]

    def refine(self, scheme='loop'):
        """Replace the mesh by its subdivision.  The old parameter, and any optimiser state for it, is void afterwards."""
        with torch.no_grad():
            vertices, faces = neural_renderer.subdivide(self.vertices, self.faces, 1, scheme)
        self.vertices = nn.Parameter(vertices.contiguous())
        self.faces = faces.contiguous()

    def forward(self):
        self.renderer.eye = neural_renderer.get_points_from_angles(2.732, 0, 90)
        image = self.renderer.render_silhouettes(self.vertices, self.faces)
        iou = neural_renderer.silhouette_iou_loss(image, self.image_ref, levels=self.levels).sum()
        laplacian = neural_renderer.laplacian_loss(self.vertices, self.faces).sum()
        flatness = neural_renderer.flatness_loss(self.vertices, self.faces).sum()
        return iou + self.weight_laplacian * laplacian + self.weight_flatness * flatness, (iou, laplacian, flatness)


def fit(model, steps, refine_at, lr=0.01, on_step=None):
    """`steps` Adam steps, the mesh refined in front of every step listed in `refine_at`; -> the loss of every step."""
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    losses = []
    for i in range(steps):
        if i in refine_at:
            model.refine()
            optimizer = torch.optim.Adam(model.parameters(), lr=lr)   # new parameters: a new optimiser
        optimizer.zero_grad()
        loss, terms = model()
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if on_step is not None:
            on_step(i, loss, terms)
    return losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('-ir', '--filename_ref', type=str, default='./examples/data/example2_ref.png')
    parser.add_argument('-oo', '--filename_output_optimization', type=str,
                        default='./examples/data/example_subdivision_optimization.gif')
    parser.add_argument('-g', '--gpu', type=int, default=0)
    parser.add_argument('--steps', type=int, default=300)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)

    model = Model(args.filename_ref).to(device)
    frames = []
    loop = tqdm.tqdm(total=args.steps)

    def on_step(i, loss, terms):
        loop.update(1)
        loop.set_description('Optimizing %d vertices' % model.num_vertices)
        with torch.no_grad():
            frames.append(model.renderer.render_silhouettes(model.vertices, model.faces).cpu().numpy()[0])
    with neural_renderer.graph.backward_on_caller_thread():   # (see example2.py)
        losses = fit(model, args.steps, (args.steps // 3, 2 * args.steps // 3), on_step=on_step)
    loop.close()
    print('loss %.4f -> %.4f, %d vertices' % (losses[0], losses[-1], model.num_vertices))
    make_gif(frames, args.filename_output_optimization)


if __name__ == '__main__':
    run()
