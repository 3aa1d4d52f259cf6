"""extract_isosurface: the HIP kernels against this module's plain-torch path, and against a plain copy of the value array.

    python scripts/isosurface_timing.py                  # one JSON line per row
    python scripts/isosurface_timing.py --skip torch     # without the plain-torch path

Rows: the signed distance to a sphere (radius 0.6 in [-1, 1]^3) at 64^3, 128^3 and 256^3, and a batch of 64 spheres of different
radii at 32^3.  Columns: `extract_isosurface` in HIP (count, scans, the readback, the allocations, emit), the kernels alone
(count + scans + emit through the C ABI into buffers made once: no readback), the module's torch path, `marching_tetrahedra` +
backward of the vertices' sum to the values, and `values.clone()`, the plain copy that reads and writes the array once -- the
memory bound the kernels are compared with (the count reads the values once and writes 6 bytes per node, the emit reads
those).  Every figure is device events around enough repetitions to last at least 0.2 s, after a warm-up of the same length,
in one process.  Informational: no threshold.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ((1, 64), (1, 128), (1, 256), (64, 32))
MIN_SECONDS = 0.2


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


def workload(batch, size):
    """values [B,G,G,G] (or [G,G,G]) on the device"""
    import torch
    import neural_renderer_amd as nr
    dev = torch.device('cuda', 0)
    distance = nr.voxel_centers(size, (-1.0, 1.0), device=dev).norm(dim=1).reshape(size, size, size)
    if batch == 1:
        return (distance - 0.6).contiguous()
    radii = torch.linspace(0.3, 0.9, batch, device=dev)
    return (distance[None] - radii[:, None, None, None]).contiguous()


def kernels_alone(values):
    """count + scans + emit through the C ABI into buffers made once"""
    import torch
    from neural_renderer_amd import _lib
    v = values if values.dim() == 4 else values[None]
    B, D, H, W = (int(s) for s in v.shape)
    dev = v.device
    ws_bytes = _lib.workspace_bytes('nr_isosurface_workspace_bytes', B, D, H, W, 0)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    totals = torch.empty((B, 3), dtype=torch.int32, device=dev)

    def count():
        _lib.launch('nr_isosurface_count', dev, v.data_ptr(), totals.data_ptr(), B, D, H, W, 0.0, 0, 0, ws.data_ptr(), ws_bytes)
    count()
    t = totals.cpu()
    nv, nf = int(t[:, 0].sum()), int(t[:, 1].sum())
    edge_nodes = torch.empty((nv, 2), dtype=torch.int32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)

    def emit():
        _lib.launch('nr_isosurface_emit', dev, edge_nodes.data_ptr(), faces.data_ptr(), nv, nf, B, D, H, W, 0, ws.data_ptr(), ws_bytes)
    return count, emit


def rows(args):
    import torch
    import neural_renderer_amd as nr
    for batch, size in WORKLOADS:
        values = workload(batch, size)
        out = nr.extract_isosurface(values, implementation='hip')
        surfaces = out if isinstance(out, list) else [out]
        row = {'B': batch, 'grid': size, 'vertices': sum(s.num_vertices for s in surfaces), 'faces': sum(s.num_faces for s in surfaces)}
        row['copy_ms'] = round(timed(lambda: values.clone())[0], 4)
        count, emit = kernels_alone(values)
        row['count_ms'], row['emit_ms'] = round(timed(count)[0], 4), round(timed(emit)[0], 4)
        row['kernels_over_copy'] = round((row['count_ms'] + row['emit_ms']) / row['copy_ms'], 2)
        row['hip_ms'] = round(timed(lambda: nr.extract_isosurface(values, implementation='hip'))[0], 4)
        row['hip_over_copy'] = round(row['hip_ms'] / row['copy_ms'], 2)
        if 'torch' not in args.skip:
            row['torch_ms'] = round(timed(lambda: nr.extract_isosurface(values, implementation='torch'))[0], 4)
        leaf = values.clone().requires_grad_(True)

        def both():
            leaf.grad = None
            meshes = nr.marching_tetrahedra(leaf, implementation='hip')
            meshes = meshes if isinstance(meshes, list) else [meshes]
            sum(v.sum() for v, _ in meshes).backward()
        both()  # (the first backward of a process sets up autograd's device thread: not part of any figure)
        row['marching_tetrahedra_backward_ms'] = round(timed(both)[0], 4)
        print(json.dumps(row), flush=True)
        del values, leaf, out, surfaces
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip', nargs='*', default=[], help='implementations to leave out: torch')
    rows(ap.parse_args())


if __name__ == '__main__':
    main()
