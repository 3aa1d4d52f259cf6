"""winding_number and voxelize: the HIP kernels against (a) this module's plain-torch path and (b) a stand-alone chunked-broadcast
torch spelling kept here -- what a user could write without the module, and the yardstick.

    python scripts/winding_timing.py                     # one JSON line per row and implementation
    python scripts/winding_timing.py --rows 0 2 --skip torch

Rows: 64 teapots (2 464 faces) x 1 024 and x 4 096 points, one icosphere of 20 480 faces x 10 242 points, and the 32^3 voxel
centres (one shared cloud) against 64 teapots and against one icosphere(3).  Columns: forward alone, forward + backward to
the vertices, forward + backward to the points (a cloud per image only).  Every figure is device events around enough
repetitions to last at least 0.2 s, after a warm-up of the same length, in one process; a call that alone lasts more than a
second is timed once, and above 3e9 pairs the torch columns are forward only (marked).  The nr_point_mesh_points_to_faces
sweep on the same shapes is reported beside the forward: the same structure, the range the new kernel should be in.
Informational: no threshold.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (mesh, batch, points or None for the voxel centres of a 32^3 grid)
WORKLOADS = (('teapot', 64, 1024), ('teapot', 64, 4096), ('icosphere5', 1, 10242), ('teapot', 64, None), ('icosphere3', 1, None))
GRID = 32
MIN_SECONDS = 0.2
CHUNK_ELEMENTS = 1 << 26
FORWARD_ONLY_ABOVE = 3e9


def timed(step):
    """(ms per call of step(), calls): device events over at least MIN_SECONDS after a warm-up as long; one call above a second
    is its own measurement"""
    import torch
    n, ms = 1, 0.0
    while True:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            step()
        stop.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(stop)
        if n == 1 and ms >= 1e3:
            return ms, 1
        if ms >= MIN_SECONDS * 1e3:
            break
        n = max(n + 1, int(n * min(10.0, 1.3 * MIN_SECONDS * 1e3 / max(ms, 1e-3))))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        step()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n, n


def workload(mesh, batch, num_points):
    """-> (points [B,N,3], or [N,3] for the voxel centres; vertices [B,Nv,3]; faces) on the device"""
    import torch
    import bench
    import neural_renderer_amd as nr
    dev = torch.device('cuda', 0)
    if mesh == 'teapot':
        v, f = bench.load_teapot()
        v, f = torch.tensor(v, device=dev), torch.tensor(f, device=dev)
    else:
        v, f = nr.icosphere(int(mesh[-1]), 0.8, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    vb = (v[None] + 0.01 * torch.randn((batch,) + tuple(v.shape), generator=gen, device=dev)).contiguous()
    if num_points is None:
        return nr.voxel_centers(GRID, device=dev), vb, f
    return (2 * torch.rand((batch, num_points, 3), generator=gen, device=dev) - 1).contiguous(), vb, f


def standalone_chunks(points, vertices, faces):
    """The winding number as a user would spell it in torch: broadcast [B,n,F,3] differences in chunks of points; yields
    (n0, w [B,n]) per chunk so that a backward can run chunk by chunk"""
    import torch
    f = faces.long()
    if points.dim() == 2:
        points = points[None]
    B, N, F = vertices.shape[0], points.shape[1], f.shape[0]
    step = max(1, CHUNK_ELEMENTS // (B * F * 12))
    for n0 in range(0, N, step):
        v0, v1, v2 = vertices[:, None, f[:, 0]], vertices[:, None, f[:, 1]], vertices[:, None, f[:, 2]]  # (a graph per chunk)
        p = points[:, n0:n0 + step, None, :]
        a, b, c = v0 - p, v1 - p, v2 - p
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        yield n0, (2.0 * torch.atan2(num, den)).sum(-1) / (4.0 * math.pi)


def rows(args):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import _lib, winding
    for k, (mesh, batch, num_points) in enumerate(WORKLOADS):
        if args.rows and k not in args.rows:
            continue
        points, vertices, faces = workload(mesh, batch, num_points)
        shared = points.dim() == 2
        N, F = int(points.shape[-2]), int(faces.shape[0])
        pairs = float(batch) * N * F
        base = {'mesh': mesh, 'B': batch, 'points': N, 'faces': F, 'shared_points': shared,
                'split_bytes': [_lib.workspace_bytes('nr_winding_workspace_bytes', batch, N, F, which, winding._SPLIT) for which in (0, 1, 2)]}
        upstream = torch.rand((batch, N), device=points.device, generator=torch.Generator(device=points.device).manual_seed(5)) - 0.5

        def module(implementation):
            def forward(p, v):
                return nr.winding_number(p, v, faces, implementation)

            def step(p, v):
                (forward(p, v) * upstream).sum().backward()
            return forward, step

        def standalone():
            def forward(p, v):
                return torch.cat([w for _, w in standalone_chunks(p, v, faces)], 1)

            def step(p, v):
                for n0, w in standalone_chunks(p, v, faces):
                    (w * upstream[:, n0:n0 + w.shape[1]]).sum().backward()
            return forward, step

        for name, (forward, step) in (('hip', module('hip')), ('torch', module('torch')), ('standalone_torch', standalone())):
            if name in args.skip:
                continue
            out = dict(base, implementation=name)

            def fwd():
                with torch.no_grad():
                    forward(points, vertices)
            out['forward_ms'], calls = timed(fwd)
            out['calls'] = [calls]
            if name != 'hip' and pairs > FORWARD_ONLY_ABOVE:
                out['note'] = 'forward only above %.0e pairs' % FORWARD_ONLY_ABOVE
            else:
                v = vertices.detach().clone().requires_grad_(True)

                def to_vertices():
                    v.grad = None
                    step(points, v)
                out['forward_backward_vertices_ms'], calls = timed(to_vertices)
                out['calls'].append(calls)
                if not shared:
                    p = points.detach().clone().requires_grad_(True)

                    def to_points():
                        p.grad = None
                        step(p, vertices)
                    out['forward_backward_points_ms'], calls = timed(to_points)
                    out['calls'].append(calls)
            print(json.dumps({key: (round(val, 4) if isinstance(val, float) else val) for key, val in out.items()}), flush=True)

        def sweep():
            with torch.no_grad():
                nr.closest_surface_points(points, vertices, faces, 'hip')
        ms, calls = timed(sweep)
        print(json.dumps(dict(base, implementation='point_mesh_points_to_faces', forward_ms=round(ms, 4), calls=[calls])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', nargs='*', type=int, default=[], help='indices into WORKLOADS (all when empty)')
    ap.add_argument('--skip', nargs='*', default=[], help='implementations to leave out: hip, torch, standalone_torch')
    rows(ap.parse_args())


if __name__ == '__main__':
    main()
