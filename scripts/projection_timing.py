"""Renderer.render forward + backward with camera_mode = 'projection' (development helper): 64 teapot views at 256^2 with a
learnable per-image pose R, t -- the fused HIP front-end against the module-by-module torch front-end, next to the fused
look_at front-end with a learnable per-image eye.  The projection cameras are the look_at cameras restated
(R = diag(1,-1,1) R_lookat(eye), t = -R eye, f = S / (2 tan 30deg)), so all rows draw the same images."""
import os, sys, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
import neural_renderer_amd as nr
from neural_renderer_amd import frontend
from neural_renderer_amd._util import normalize
dev = torch.device('cuda', 0)
v, f = bench.load_teapot()
B, S = 64, 256
vertices = torch.from_numpy(v).to(dev)[None].repeat(B, 1, 1).requires_grad_(True)
faces = torch.from_numpy(f).to(dev)[None].repeat(B, 1, 1)
textures = torch.ones((B, f.shape[0], 2, 2, 2, 3), device=dev, requires_grad=True)
eyes = torch.tensor([nr.get_points_from_angles(2.732, 30., 360.0 * i / B) for i in range(B)], dtype=torch.float32)
z = normalize(-eyes)
x = normalize(torch.cross(torch.tensor([[0., 1., 0.]]).expand(B, 3), z, dim=1))
y = normalize(torch.cross(z, x, dim=1))
R0 = torch.stack((x, -y, z), dim=1)
t0 = -torch.matmul(R0, eyes[:, :, None])[:, :, 0]
tan = np.tan(np.float32(30) / np.float32(180) * np.float32(3.1416), dtype=np.float32)
fl = float(np.float32(S) / (np.float32(2) * tan))
K = torch.tensor([[fl, 0, S / 2], [0, fl, S / 2], [0, 0, 1]], device=dev)
R = R0.to(dev).requires_grad_(True)
t = t0.to(dev).requires_grad_(True)
eye = eyes.to(dev).requires_grad_(True)


def timed(fn, n=10):
    for _ in range(3): fn()
    torch.cuda.synchronize(); t_0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t_0) / n * 1e3


_fusable = frontend.fusable
for mode, fused in (('look_at', True), ('projection', True), ('projection', False)):
    frontend.fusable = _fusable if fused else (lambda *a: False)   # False: module-by-module torch front-end
    r = nr.Renderer()
    r.image_size, r.anti_aliasing = S, False
    if mode == 'projection':
        r.camera_mode, r.K, r.R, r.t, r.orig_size = 'projection', K, R, t, S
    else:
        r.eye = eye
    params = (vertices, textures, R, t, eye)

    def rgb():
        for p in params: p.grad = None
        img = r.render(vertices, faces, textures); img.square().sum().backward()

    def sil():
        for p in params: p.grad = None
        img = r.render_silhouettes(vertices, faces); img.square().sum().backward()

    ms_rgb, ms_sil = timed(rgb), timed(sil)
    assert r.last_frontend == ('fused' if fused else 'torch')
    print(json.dumps({'camera_mode': mode, 'fused_frontend': fused, 'render_fwd_bwd_ms': round(ms_rgb, 3),
                      'silhouettes_fwd_bwd_ms': round(ms_sil, 3)}))
frontend.fusable = _fusable
