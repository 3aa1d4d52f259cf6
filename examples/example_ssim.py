"""
Fitting vertex colours to a target picture under a squared error paired with SSIM (not in the reference's examples).

The target is a picture of a sphere with a striped colour pattern under smooth (Gouraud) light; the fit starts from a grey
sphere of the same shape and learns one colour per vertex.  The objective is the usual photometric pair

    (1 - lambda) * squared error per pixel + lambda * (1 - SSIM),

`squared_error_loss` for the colours themselves and `ssim_loss` for their structure: the squared error alone averages over
what it cannot resolve, the structural term rewards the stripes' contrast.  Both run as HIP kernels in both directions.

    python examples/example_ssim.py [steps]
"""
import sys

import torch
import torch.nn as nn

import neural_renderer


class Model(nn.Module):
    def __init__(self, image_size=64, weight=0.2):
        super(Model, self).__init__()
        vertices, faces = neural_renderer.icosphere(3, 0.8)
        self.register_buffer('vertices', vertices[None])
        self.register_buffer('faces', faces[None])
        # stripes along the vertical axis, each channel with a phase of its own
        phase = vertices[:, 1:2] * 12 + torch.tensor([0.0, 2.0, 4.0])
        self.register_buffer('target_colors', 0.5 + 0.4 * torch.sin(phase))
        self.colors = nn.Parameter(torch.full_like(vertices, 0.5))
        self.weight = weight
        renderer = neural_renderer.Renderer()
        renderer.image_size = image_size
        renderer.eye = neural_renderer.get_points_from_angles(2.732, 20, 30)
        renderer.shading = 'smooth'
        self.renderer = renderer
        self.target = None

    def render(self, colors):
        return self.renderer.render(self.vertices, self.faces, neural_renderer.VertexColors(colors))

    def forward(self):
        if self.target is None:
            with torch.no_grad():
                self.target = self.render(self.target_colors).clone()
        image = self.render(self.colors)
        pixels = image.shape[1] * image.shape[2] * image.shape[3]
        error = neural_renderer.squared_error_loss(image, self.target).sum() / pixels
        structure = neural_renderer.ssim_loss(image, self.target).sum()
        return (1 - self.weight) * error + self.weight * structure, (error, structure)


def run(steps=200):
    model = Model().cuda()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.05)
    for i in range(steps):
        optimizer.zero_grad()
        loss, (error, structure) = model()
        loss.backward()
        optimizer.step()
        if i == 0 or i == steps - 1 or i % 20 == 0:
            print('step %3d loss %.5f (squared error %.5f, 1 - SSIM %.4f)'
                  % (i, float(loss.detach()), float(error.detach()), float(structure.detach())))
    with torch.no_grad():
        print('SSIM of the fit with the target: %.4f'
              % float(neural_renderer.ssim_index(model.render(model.colors), model.target).mean()))


if __name__ == '__main__':
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
