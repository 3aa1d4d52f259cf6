"""
Learnable lights (not in the reference): recover the light of a set of images -- nine spherical-harmonics coefficients per
image and the direction of one lamp shared by all of them -- from renders of a vertex-coloured icosphere, smooth-shaded.

    python examples/example_lights.py
"""
import argparse
import os

import numpy as np
import torch

import neural_renderer
from example_io import save_image


def icosphere(level):
    """vertices [Nv,3] on the unit sphere and faces [20 * 4^level, 3], outward for the renderer's convention."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


class Scene(object):
    """B views of an icosphere with fixed vertex colours; the targets are rendered with a hidden light."""

    def __init__(self, device, views=4, level=2, image_size=64, seed=0):
        rng = np.random.RandomState(seed)
        v, f = icosphere(level)
        self.vertices = torch.from_numpy(v).to(device)[None].expand(views, -1, -1).contiguous()
        self.faces = torch.from_numpy(f).to(device)[None].expand(views, -1, -1).contiguous()
        self.colors = neural_renderer.VertexColors(torch.from_numpy((0.6 + 0.4 * v).clip(0, 1).astype(np.float32)).to(device))
        self.renderer = neural_renderer.Renderer()
        self.renderer.image_size = image_size
        self.renderer.shading = 'smooth'
        self.renderer.eye = torch.tensor(np.stack([neural_renderer.get_points_from_angles(2.732, 20, 360.0 * i / views)
                                                   for i in range(views)]), dtype=torch.float32, device=device)
        # the hidden light: one lamp for all views, SH coefficients per view (a dominant constant term, weaker bands 1 and 2)
        sh = rng.uniform(-0.15, 0.15, (views, 9, 3)) * np.array([1.0] + [0.7] * 3 + [0.4] * 5)[None, :, None]
        sh[:, 0] += 0.8
        self.truth = neural_renderer.Lights(intensity_ambient=0.0, intensity_directional=0.6, direction=(0.5, 0.7, -0.5),
                                            sh=torch.tensor(sh, dtype=torch.float32)).to(device)
        with torch.no_grad():
            self.target = self.render(self.truth)
        # the start: a lamp from above, a flat grey environment
        start = torch.zeros((views, 9, 3))
        start[:, 0] = 0.5
        self.lights = neural_renderer.Lights(intensity_ambient=0.0, intensity_directional=0.6, direction=(0.0, 1.0, 0.0), sh=start,
                                             learnable=('sh', 'direction')).to(device)

    def render(self, lights):
        self.renderer.lights = lights
        return self.renderer.render(self.vertices, self.faces, self.colors)

    def loss(self):
        return ((self.render(self.lights) - self.target) ** 2).mean()


def fit(scene, steps, lr=0.03, log=None):
    """Adam on the scene's learnable light; returns the loss of every step."""
    optimizer = torch.optim.Adam(scene.lights.parameters(), lr=lr)
    losses = []
    for step in range(steps):
        optimizer.zero_grad()
        loss = scene.loss()
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if log and (step % 50 == 0 or step == steps - 1):
            log('step %3d  loss %.3e' % (step, losses[-1]))
    return losses


def run():
    parser = argparse.ArgumentParser()
    parser.add_argument('-o', '--filename_output', type=str, default='./examples/data/example_lights.png')
    parser.add_argument('-g', '--gpu', type=int, default=0)
    parser.add_argument('--steps', type=int, default=300)
    parser.add_argument('--views', type=int, default=4)
    args = parser.parse_args()
    device = torch.device('cuda', args.gpu)

    scene = Scene(device, views=args.views)
    fit(scene, args.steps, log=print)
    d, t = scene.lights.direction.detach(), scene.truth.direction
    print('lamp direction %s (hidden: %s), cosine %.4f' % (np.round(d.cpu().numpy(), 3), t.cpu().numpy(),
                                                          float(torch.nn.functional.cosine_similarity(d, t, dim=0))))
    print('largest SH coefficient error %.3f' % float((scene.lights.sh.detach() - scene.truth.sh).abs().max()))
    with torch.no_grad():
        fitted = scene.render(scene.lights)
    rows = [torch.cat(list(x), dim=2).permute(1, 2, 0).clamp(0, 1).cpu().numpy() for x in (scene.target, fitted)]
    os.makedirs(os.path.dirname(os.path.abspath(args.filename_output)), exist_ok=True)
    save_image(np.concatenate(rows, axis=0), args.filename_output)
    print('wrote', args.filename_output)


if __name__ == '__main__':
    run()
