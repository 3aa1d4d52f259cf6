"""point_mesh_distance: the HIP kernels against (a) this module's plain-torch path and (b) the way the job was done before it,
`sample_surface_points` with as many samples as scan points followed by `chamfer_distance`.

    python scripts/point_mesh_timing.py                     # one JSON line per row
    python scripts/point_mesh_timing.py --build-variants    # (no GPU needed) csrc/nr_point_mesh.hip alone, other -D values
    python scripts/point_mesh_timing.py --variants          # the variants through the C ABI on torch tensors

Rows: 64 teapots (2 464 faces) x 1 024 and x 4 096 points, and one icosphere of 20 480 faces x 10 242 points; each direction
and both; forward alone and forward + backward (points fixed, vertices learnable).  Every figure is device events around
enough repetitions to last at least 0.2 s, after a warm-up of the same length, in one process.  Informational: no threshold.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (('teapot', 64, 1024), ('teapot', 64, 4096), ('icosphere', 1, 10242))
DIRECTIONS = ('points_to_mesh', 'mesh_to_points', 'both')
# tag -> -D values of csrc/nr_point_mesh.hip
VARIANTS = {'q1': ['NR_PM_Q=1'], 'q2': [], 'q4': ['NR_PM_Q=4'], 'q8': ['NR_PM_Q=8'], 'q2_t128': ['NR_PM_T=128'],
            'q2_t1024': ['NR_PM_T=1024'], 'q2_nosplit': ['NR_PM_SPLIT_BELOW=0'], 'q2_split1024': ['NR_PM_SPLIT_BELOW=1024']}
MIN_SECONDS = 0.2


def variant_path(tag):
    return os.path.join(ROOT, 'build_dev', 'libnr_point_mesh_%s.so' % tag)


def build_variants():
    import subprocess
    from neural_renderer_amd import _build
    os.makedirs(os.path.join(ROOT, 'build_dev'), exist_ok=True)
    for tag, defines in VARIANTS.items():
        cmd = [_build.hipcc()] + _build.HIPCC_FLAGS + ['-D%s' % d for d in defines] + \
            [os.path.join(_build.HERE, 'csrc', 'nr_point_mesh.hip'), '-o', variant_path(tag)]
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


def workload(mesh, batch, num_points):
    """-> (points [B,N,3] fixed, vertices [B,Nv,3] learnable, faces) on the device: the scan is the mesh's own surface, jittered"""
    import numpy as np
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
    with torch.no_grad():
        points, _ = nr.sample_surface_points(vb, f, num_points, gen)
        points = points + 0.02 * torch.randn(points.shape, generator=gen, device=dev)
    return points.contiguous(), vb.contiguous().requires_grad_(True), f


def rows(args):
    import torch
    import neural_renderer_amd as nr
    for mesh, batch, num_points in WORKLOADS:
        points, vertices, faces = workload(mesh, batch, num_points)
        gen = torch.Generator(device=points.device).manual_seed(4)
        chamfer_of = {'points_to_mesh': 'y_to_x', 'mesh_to_points': 'x_to_y', 'both': 'both'}
        for direction in DIRECTIONS:
            def hip():
                return nr.point_mesh_distance(points, vertices, faces, direction, implementation='hip')

            def eager():
                return nr.point_mesh_distance(points, vertices, faces, direction, implementation='torch')

            def sampled():  # (b): sample the surface with as many samples as scan points, then the chamfer distance
                samples, _ = nr.sample_surface_points(vertices, faces, num_points, gen)
                return nr.chamfer_distance(samples, points, chamfer_of[direction])

            for name, fn in (('hip', hip), ('torch', eager), ('sampled_chamfer', sampled)):
                if name in args.skip:
                    continue

                def forward():
                    with torch.no_grad():
                        fn()

                def both():
                    vertices.grad = None
                    fn().sum().backward()
                fwd, n1 = timed(forward)
                fb, n2 = timed(both)
                print(json.dumps({'mesh': mesh, 'B': batch, 'points': num_points, 'faces': int(faces.shape[0]),
                                  'direction': direction, 'implementation': name, 'forward_ms': round(fwd, 4),
                                  'forward_backward_ms': round(fb, 4), 'calls': [n1, n2]}), flush=True)


def variants():
    """The sweeps and the two backward kernels of every variant library through the C ABI, per workload: ms per call"""
    import torch
    from neural_renderer_amd import _lib
    from neural_renderer_amd.point_mesh import _sorted_by
    from neural_renderer_amd.vertex_colors import _adjacency
    names = [n for n in _lib.SIGNATURES if n.startswith('nr_point_mesh_')]
    for mesh, batch, num_points in WORKLOADS:
        points, vertices, faces = workload(mesh, batch, num_points)
        v = vertices.detach()
        B, N, Nv = int(v.shape[0]), int(points.shape[1]), int(v.shape[1])
        idx, adj_off, adj_ent, _ = _adjacency(faces, Nv)
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
            out = {}
            for flag, rows_n, fn in ((0, N, lib.nr_point_mesh_points_to_faces), (1, F, lib.nr_point_mesh_faces_to_points)):
                d = torch.empty((B, rows_n), device=dev)
                ids = torch.empty((B, rows_n), dtype=torch.int32, device=dev)
                w = torch.empty((B, rows_n, 3), device=dev)
                nbytes = lib.nr_point_mesh_workspace_bytes(B, N, F, flag, 0)
                ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)

                def sweep():
                    rc = fn(points.data_ptr(), v.data_ptr(), idx.data_ptr(), d.data_ptr(), ids.data_ptr(), w.data_ptr(), B, N, Nv, F,
                            1, 0, ws.data_ptr(), nbytes, stream)
                    assert rc == 0, rc
                out[flag] = (d, ids, w, timed(sweep)[0])
            (dp, fid, wp, ms_p), (df, pid, wf, ms_f) = out[0], out[1]
            gp, gf = torch.ones_like(dp), torch.ones_like(df)
            order_p, off_f = _sorted_by(fid, F)
            order_f, off_p = _sorted_by(pid, N)
            grad_p, grad_v = torch.empty_like(points), torch.empty_like(v)

            def backward_points():
                rc = lib.nr_point_mesh_backward_points(points.data_ptr(), v.data_ptr(), idx.data_ptr(), fid.data_ptr(), wp.data_ptr(),
                                                       gp.data_ptr(), pid.data_ptr(), wf.data_ptr(), gf.data_ptr(), order_f.data_ptr(),
                                                       off_p.data_ptr(), grad_p.data_ptr(), B, N, Nv, F, stream)
                assert rc == 0, rc

            def backward_vertices():
                rc = lib.nr_point_mesh_backward_vertices(points.data_ptr(), v.data_ptr(), idx.data_ptr(), adj_off.data_ptr(),
                                                         adj_ent.data_ptr(), fid.data_ptr(), wp.data_ptr(), gp.data_ptr(),
                                                         order_p.data_ptr(), off_f.data_ptr(), pid.data_ptr(), wf.data_ptr(),
                                                         gf.data_ptr(), grad_v.data_ptr(), B, N, Nv, F, 1, stream)
                assert rc == 0, rc
            print(json.dumps({'variant': tag, 'defines': VARIANTS[tag], 'mesh': mesh, 'B': B, 'points': N, 'faces': F,
                              'points_to_faces_ms': round(ms_p, 4), 'faces_to_points_ms': round(ms_f, 4),
                              'backward_points_ms': round(timed(backward_points)[0], 4),
                              'backward_vertices_ms': round(timed(backward_vertices)[0], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--build-variants', action='store_true')
    ap.add_argument('--variants', action='store_true')
    ap.add_argument('--skip', nargs='*', default=[], help="implementations to leave out: hip, torch, sampled_chamfer")
    args = ap.parse_args()
    if args.build_variants:
        build_variants()
    elif args.variants:
        variants()
    else:
        rows(args)


if __name__ == '__main__':
    main()
