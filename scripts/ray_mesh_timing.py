"""ray_mesh_intersect: the HIP kernels against (a) this module's plain-torch path and (b) the point-to-mesh sweep
(`closest_surface_points`, nr_point_mesh_points_to_faces) of the same shape, the nearest thing the package had.

    python scripts/ray_mesh_timing.py                     # one JSON line per row
    python scripts/ray_mesh_timing.py --skip torch        # without the plain-torch path (seconds per call on the large rows)
    python scripts/ray_mesh_timing.py --build-variants    # (no GPU needed) csrc/nr_ray_mesh.hip alone, other -D values
    python scripts/ray_mesh_timing.py --variants          # the variants' two sweeps through the C ABI on torch tensors

Rows, those of scripts/winding_timing.py: 64 teapots (2 464 faces) x 1 024 and x 4 096 rays, one icosphere of 20 480 faces x
10 242 rays, and `camera_rays` at 64 x 64^2 on the teapot (one origin per image).  Two rays in three are aimed at the surface
from a sphere around it, the third has a random direction.  Columns: forward alone (first hit; any hit for the HIP path as
well), and forward + backward to the vertices of sum (t on the hits).  Every figure is device events around enough
repetitions to last at least 0.2 s, after a warm-up of the same length, in one process.  Informational: no threshold.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (('teapot', 64, 1024), ('teapot', 64, 4096), ('icosphere5', 1, 10242), ('teapot', 64, 'camera64'))
# tag -> -D values of csrc/nr_ray_mesh.hip
VARIANTS = {'q1': ['NR_RAY_Q=1'], 'q2': [], 'q4': ['NR_RAY_Q=4'], 'q2_t128': ['NR_RAY_T=128'], 'q2_t1024': ['NR_RAY_T=1024'],
            'q2_nosplit': ['NR_RAY_SPLIT_BELOW=0']}
MIN_SECONDS = 0.2


def variant_path(tag):
    return os.path.join(ROOT, 'build_dev', 'libnr_ray_mesh_%s.so' % tag)


def build_variants():
    import subprocess
    from neural_renderer_amd import _build
    os.makedirs(os.path.join(ROOT, 'build_dev'), exist_ok=True)
    for tag, defines in VARIANTS.items():
        cmd = [_build.hipcc()] + _build.HIPCC_FLAGS + ['-D%s' % d for d in defines] + \
            [os.path.join(_build.HERE, 'csrc', 'nr_ray_mesh.hip'), '-o', variant_path(tag)]
        print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)


def timed(step):
    """ms per call of step(): device events over at least MIN_SECONDS, after a warm-up as long"""
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


def workload(mesh, batch, rays):
    """-> (origins, directions [B,R,3] fixed -- origins [B,3] for the camera --, vertices [B,Nv,3] learnable, faces) on the device"""
    import torch
    import bench
    import neural_renderer_amd as nr
    dev = torch.device('cuda', 0)
    if mesh == 'teapot':
        v, f = bench.load_teapot()
        v, f = torch.tensor(v, device=dev), torch.tensor(f, device=dev)
    else:
        v, f = nr.icosphere(5, 0.5, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    vb = v[None] + 0.01 * torch.randn((batch,) + tuple(v.shape), generator=gen, device=dev)
    if rays == 'camera64':
        renderer = nr.Renderer()
        renderer.image_size = 64
        renderer.eye = torch.tensor([nr.get_points_from_angles(2.732, 30.0, 360.0 * i / batch) for i in range(batch)], device=dev)
        origins, directions = nr.camera_rays(renderer, batch, vb)
        return origins.contiguous(), directions.contiguous(), vb.contiguous().requires_grad_(True), f
    with torch.no_grad():
        aim, _ = nr.sample_surface_points(vb, f, rays, gen)
        origins = torch.randn((batch, rays, 3), generator=gen, device=dev)
        origins = 3.0 * origins / origins.norm(dim=2, keepdim=True)
        free = torch.randn((batch, rays, 3), generator=gen, device=dev)
        third = (torch.arange(rays, device=dev) % 3 == 2)[None, :, None]
        directions = torch.where(third, free, aim - origins)
    return origins.contiguous(), directions.contiguous(), vb.contiguous().requires_grad_(True), f


def rows(args):
    import torch
    import neural_renderer_amd as nr
    for mesh, batch, rays in WORKLOADS:
        origins, directions, vertices, faces = workload(mesh, batch, rays)
        R = int(directions.shape[1])
        with torch.no_grad():
            t, ids, _ = nr.ray_mesh_intersect(origins, directions, vertices, faces)
            o_full = origins[:, None].expand(-1, R, -1) if origins.dim() == 2 else origins
            points = torch.where((ids >= 0)[..., None], o_full + torch.nan_to_num(t, posinf=0.0)[..., None] * directions, o_full)
            points = points.contiguous()
        share = float((ids >= 0).float().mean())

        def first(implementation):
            return nr.ray_mesh_intersect(origins, directions, vertices, faces, implementation=implementation)

        def loss_of(out):
            t, ids = out[0], out[1]
            return torch.where(ids >= 0, t, torch.zeros_like(t)).sum()

        cases = [('hip', lambda: first('hip'), loss_of), ('torch', lambda: first('torch'), loss_of),
                 ('point_mesh_sweep', lambda: nr.closest_surface_points(points, vertices, faces, 'hip'), lambda out: out[0].sum())]
        for name, fn, loss in cases:
            if name in args.skip:
                continue

            def forward():
                with torch.no_grad():
                    fn()

            def both():
                vertices.grad = None
                loss(fn()).backward()
            both()  # (the first backward of a process sets up autograd's device thread: not part of any figure)
            fwd, n1 = timed(forward)
            fb, n2 = timed(both)
            row = {'mesh': mesh, 'B': batch, 'rays': R, 'faces': int(faces.shape[0]), 'hit_share': round(share, 3),
                   'implementation': name, 'forward_ms': round(fwd, 4), 'forward_backward_ms': round(fb, 4), 'calls': [n1, n2]}
            if name == 'hip':
                def occluded():
                    nr.ray_mesh_occluded(origins, directions, vertices, faces, implementation='hip')
                row['any_hit_ms'] = round(timed(occluded)[0], 4)
            print(json.dumps(row), flush=True)


def variants():
    """The two sweeps of every variant library through the C ABI, per workload: ms per call"""
    import torch
    from neural_renderer_amd import _lib
    from neural_renderer_amd.vertex_colors import _adjacency
    names = [n for n in _lib.SIGNATURES if n.startswith('nr_ray_mesh_')]
    for mesh, batch, rays in WORKLOADS:
        origins, directions, vertices, faces = workload(mesh, batch, rays)
        v = vertices.detach()
        B, R, Nv = int(v.shape[0]), int(directions.shape[1]), int(v.shape[1])
        o = (origins[:, None].expand(-1, R, -1) if origins.dim() == 2 else origins).contiguous()
        idx = _adjacency(faces, Nv)[0]
        F = int(idx.shape[1])
        dev = v.device
        stream = _lib.stream_ptr(dev)
        for tag in VARIANTS:
            if not os.path.exists(variant_path(tag)):
                print(json.dumps({'variant': tag, 'missing': variant_path(tag)}), flush=True)
                continue
            lib = ctypes.CDLL(variant_path(tag))
            for n in names:
                getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.SIGNATURES[n]
            t = torch.empty((B, R), device=dev)
            ids = torch.empty((B, R), dtype=torch.int32, device=dev)
            w = torch.empty((B, R, 3), device=dev)
            occ = torch.empty((B, R), dtype=torch.bool, device=dev)
            nbytes = max(lib.nr_ray_mesh_workspace_bytes(B, R, F, 0, 0), lib.nr_ray_mesh_workspace_bytes(B, R, F, 1, 0))
            ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)

            def first_hit():
                rc = lib.nr_ray_mesh_first_hit(o.data_ptr(), directions.data_ptr(), v.data_ptr(), idx.data_ptr(), t.data_ptr(),
                                               ids.data_ptr(), w.data_ptr(), B, R, Nv, F, 1, 0.0, float('inf'), 0, 0, ws.data_ptr(),
                                               nbytes, stream)
                assert rc == 0, rc

            def any_hit():
                rc = lib.nr_ray_mesh_any_hit(o.data_ptr(), directions.data_ptr(), v.data_ptr(), idx.data_ptr(), occ.data_ptr(), B, R,
                                             Nv, F, 1, 0.0, float('inf'), 0, 0, ws.data_ptr(), nbytes, stream)
                assert rc == 0, rc
            print(json.dumps({'variant': tag, 'defines': VARIANTS[tag], 'mesh': mesh, 'B': B, 'rays': R, 'faces': F,
                              'first_hit_ms': round(timed(first_hit)[0], 4), 'any_hit_ms': round(timed(any_hit)[0], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--build-variants', action='store_true')
    ap.add_argument('--variants', action='store_true')
    ap.add_argument('--skip', nargs='*', default=[], help="implementations to leave out: hip, torch, point_mesh_sweep")
    args = ap.parse_args()
    if args.build_variants:
        build_variants()
    elif args.variants:
        variants()
    else:
        rows(args)


if __name__ == '__main__':
    main()
