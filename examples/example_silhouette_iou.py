"""
Example 2 with the paper's objective: optimizing vertices against a silhouette with the multi-scale IoU loss plus the Laplacian
and the flatness prior (not in the reference's examples; Neural 3D Mesh Renderer, section 5).

The IoU is taken on an image pyramid of four levels: the rasterizer's approximate gradient moves a vertex only when a pixel
within its sweep changes, and the coarse levels carry a signal across the distance that the fine level cannot see.
"""
import argparse

import numpy as np
import torch
import torch.nn as nn
import tqdm

import neural_renderer
from example_io import make_gif, read_image


class Model(nn.Module):
    def __init__(self, filename_obj, filename_ref, weight_laplacian=0.03, weight_flatness=1e-5, levels=4):
        super(Model, self).__init__()
        vertices, faces = neural_renderer.load_obj(filename_obj)
        self.vertices = nn.Parameter(torch.from_numpy(vertices[None, :, :]))
        self.register_buffer('faces', torch.from_numpy(faces[None, :, :]))
        texture_size = 2
        self.register_buffer('textures', torch.ones((1, self.faces.shape[1], texture_size, texture_size, texture_size,
                                                     3), dtype=torch.float32))
        ref = read_image(filename_ref)
        if ref.ndim == 3:
            ref = ref.max(-1)
        self.register_buffer('image_ref', torch.from_numpy((ref > 0.5).astype(np.float32)))
        self.renderer = neural_renderer.Renderer()
        self.weight_laplacian, self.weight_flatness, self.levels = weight_laplacian, weight_flatness, levels

    def forward(self):
        self.renderer.eye = neural_renderer.get_points_from_angles(2.732, 0, 90)
        image = self.renderer.render_silhouettes(self.vertices, self.faces)
        # one loss per image of the batch (here: one); the reference silhouette [H,W] is shared by the batch
        iou = neural_renderer.silhouette_iou_loss(image, self.image_ref, levels=self.levels).sum()
        laplacian = neural_renderer.laplacian_loss(self.vertices, self.faces).sum()
        flatness = neural_renderer.flatness_loss(self.vertices, self.faces).sum()
        return iou + self.weight_laplacian * laplacian + self.weight_flatness * flatness, (iou, laplacian, flatness)


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('-io', '--filename_obj', type=str, default='./examples/data/teapot.obj')
    parser.add_argument('-ir', '--filename_ref', type=str, default='./examples/data/example2_ref.png')
    parser.add_argument('-oo', '--filename_output_optimization', type=str,
                        default='./examples/data/example_silhouette_iou_optimization.gif')
    parser.add_argument('-or', '--filename_output_result', type=str, default='./examples/data/example_silhouette_iou_result.gif')
    parser.add_argument('-g', '--gpu', type=int, default=0)
    parser.add_argument('--steps', type=int, default=300)
    parser.add_argument('--levels', type=int, default=4)
    parser.add_argument('--weight_laplacian', type=float, default=0.03)
    parser.add_argument('--weight_flatness', type=float, default=1e-5)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)

    model = Model(args.filename_obj, args.filename_ref, args.weight_laplacian, args.weight_flatness, args.levels).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    frames = []
    with neural_renderer.graph.backward_on_caller_thread():   # (see example2.py)
        loop = tqdm.tqdm(range(args.steps))
        for i in loop:
            loop.set_description('Optimizing')
            optimizer.zero_grad()
            loss, terms = model()
            loss.backward()
            optimizer.step()
            with torch.no_grad():
                images = model.renderer.render_silhouettes(model.vertices, model.faces)
            frames.append(images.cpu().numpy()[0])
        print('final loss %.4f (iou %.4f, laplacian %.4f, flatness %.4f)' % ((float(loss.detach()),) + tuple(float(t.detach()) for t in terms)))
        make_gif(frames, args.filename_output_optimization)

    frames = []
    for azimuth in tqdm.tqdm(range(0, 360, 4), desc='Drawing'):
        model.renderer.eye = neural_renderer.get_points_from_angles(2.732, 0, azimuth)
        with torch.no_grad():
            images = model.renderer.render(model.vertices, model.faces, model.textures)
        frames.append(images.cpu().numpy()[0].transpose((1, 2, 0)))
    make_gif(frames, args.filename_output_result)


if __name__ == '__main__':
    run()
