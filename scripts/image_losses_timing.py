"""silhouette_iou_loss / squared_error_loss forward + backward: the HIP kernels against the same losses spelled out with torch
operations in this script (what a user writes without the feature; NOT the package's own torch path), and a whole fitting
step through Renderer.render_rgbad against render + render_silhouettes.

    python scripts/image_losses_timing.py            # one JSON line per row

Loss rows: B x 256 x 256 for B in (64, 1) and levels in (1, 4); `iou`, `se` (C = 3) and `both`; a step is
loss.sum().backward() on a leaf image.  Render rows: 64 teapot views at 256 x 256, a step is the render (rgb + alpha), both
losses and the backward to the vertices.  The two variants of a row alternate inside one child process: warm-up, then
`repeats` rounds of `steps` steps each, timed with device events; a row reports the median round and the spread (min, max)
of each variant.  Behind the timings, in children of their own: kernels per step from torch's profiler for the rows at B =
64 and 4 levels (`not measured` when the profiler gives none).  Every
row runs in a child process of its own under `timeout`, and the first one that fails ends the run.  Informational: no
threshold.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_TIMEOUT = 150  # seconds per child
LOSS_ROWS = [(what, batch, levels) for batch in (64, 1) for levels in (1, 4) for what in ('iou', 'se', 'both')]
RENDER_ROWS = [('render', 64, 1), ('render', 64, 4)]


# the losses as a user spells them with torch operations
def iou_spelled(alpha, target, levels, eps=1e-6):
    import torch.nn.functional as F
    a, t, loss = alpha[:, None], target[:, None], 0
    for l in range(levels):
        if l:
            a, t = F.avg_pool2d(a, 2), F.avg_pool2d(t, 2)
        inter = (a * t).sum((1, 2, 3))
        union = (a + t - a * t).sum((1, 2, 3))
        loss = loss + (1 - inter / (union + eps))
    return loss


def se_spelled(images, target, levels):
    import torch.nn.functional as F
    d, loss = images - target, 0
    for l in range(levels):
        if l:
            d = F.avg_pool2d(d, 2)
        loss = loss + (d * d).sum((1, 2, 3))
    return loss


def timed(variants, steps, repeats, warmup=5):
    """variants: name -> step function.  -> name -> sorted list of ms per step, one per round; the variants alternate."""
    import torch
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    rounds = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(steps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            rounds[n].append(start.elapsed_time(stop) / steps)
    return {n: sorted(v) for n, v in rounds.items()}


def launches(fn):
    """kernels per step, from torch's profiler; None when it reports none"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n // 3 if n else None
    except Exception as exc:  # the measurement is optional
        print('# profiler: %s' % exc, file=sys.stderr)
        return None


def report(row, variants, steps, repeats, count):
    """one JSON line: the timings of the row's variants, or (count) their launches per step"""
    out = dict(row)
    if count:
        out['row'] += '_launches'
        for n, fn in variants.items():
            k = launches(fn)
            out[n + '_launches'] = k if k is not None else 'not measured'
    else:
        for n, v in timed(variants, steps, repeats).items():
            out[n + '_ms'] = round(v[len(v) // 2], 4)
            out[n + '_ms_min_max'] = [round(v[0], 4), round(v[-1], 4)]
        names = list(variants)
        out['%s_over_%s' % (names[1], names[0])] = round(out[names[1] + '_ms'] / out[names[0] + '_ms'], 2)
    print(json.dumps(out), flush=True)


def loss_row(what, batch, levels, steps, repeats, count):
    import torch
    import neural_renderer_amd as nr
    dev = torch.device('cuda', 0)
    S = 256
    gen = torch.Generator(device='cpu').manual_seed(3)
    alpha = torch.rand((batch, S, S), generator=gen).to(dev).requires_grad_(True)
    target = (torch.rand((batch, S, S), generator=gen) > 0.5).float().to(dev)
    image = torch.rand((batch, 3, S, S), generator=gen).to(dev).requires_grad_(True)
    image_target = torch.rand((batch, 3, S, S), generator=gen).to(dev)

    def step(iou, se):
        def run():
            alpha.grad = image.grad = None
            loss = 0
            if what in ('iou', 'both'):
                loss = loss + iou(alpha, target).sum()
            if what in ('se', 'both'):
                loss = loss + se(image, image_target).sum()
            loss.backward()
        return run
    variants = {'hip': step(lambda a, t: nr.silhouette_iou_loss(a, t, levels=levels, implementation='hip'),
                            lambda x, t: nr.squared_error_loss(x, t, levels=levels, implementation='hip')),
                'torch': step(lambda a, t: iou_spelled(a, t, levels), lambda x, t: se_spelled(x, t, levels))}
    report({'row': 'loss', 'loss': what, 'B': batch, 'size': S, 'levels': levels}, variants, steps, repeats, count)


def render_row(batch, levels, steps, repeats, count):
    import torch
    import bench
    import neural_renderer_amd as nr
    dev = torch.device('cuda', 0)
    v, f = bench.load_teapot()
    vertices = torch.tensor(v[None], device=dev).expand(batch, -1, -1).contiguous().requires_grad_(True)
    faces = torch.tensor(f, device=dev)[None].expand(batch, -1, -1).contiguous()
    textures = torch.ones((batch, f.shape[0], 2, 2, 2, 3), device=dev)
    r = nr.Renderer()
    r.eye = torch.tensor([nr.get_points_from_angles(2.732, 30., 360.0 * i / batch) for i in range(batch)], device=dev)
    with torch.no_grad():
        out = r.render_rgbad(vertices * 1.05, faces, textures, return_depth=False)
        rgb_target, alpha_target = out['rgb'].clone(), out['alpha'].clone()

    def one_pass():
        vertices.grad = None
        out = r.render_rgbad(vertices, faces, textures, return_depth=False)
        loss = nr.silhouette_iou_loss(out['alpha'], alpha_target, levels=levels).sum() + \
            nr.squared_error_loss(out['rgb'], rgb_target, levels=levels).sum()
        loss.backward()

    def two_passes():
        vertices.grad = None
        rgb, alpha = r.render(vertices, faces, textures), r.render_silhouettes(vertices, faces)
        loss = iou_spelled(alpha, alpha_target, levels).sum() + se_spelled(rgb, rgb_target, levels).sum()
        loss.backward()
    variants = {'render_rgbad_hip_losses': one_pass, 'two_renders_torch_losses': two_passes}
    report({'row': 'render', 'B': batch, 'size': 256, 'levels': levels, 'faces': int(f.shape[0])}, variants, steps, repeats,
           count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--count', action='store_true', help='(a child: count the launches instead of timing)')
    ap.add_argument('--one', nargs=3, metavar=('WHAT', 'BATCH', 'LEVELS'), help='(a child: one row)')
    args = ap.parse_args()
    if args.one:
        what, batch, levels = args.one[0], int(args.one[1]), int(args.one[2])
        if what == 'render':
            render_row(batch, levels, args.steps, args.repeats, args.count)
        else:
            loss_row(what, batch, levels, args.steps, args.repeats, args.count)
        return
    rows = LOSS_ROWS + RENDER_ROWS
    # every timing first; the launch counts (the profiler) last, for the rows at 4 levels
    for count, (what, batch, levels) in [(False, r) for r in rows] + [(True, r) for r in rows if r[1] == 64 and r[2] == 4]:
        cmd = ['timeout', '-k', '10', str(ROW_TIMEOUT), sys.executable, os.path.abspath(__file__), '--steps', str(args.steps),
               '--repeats', str(args.repeats), '--one', what, str(batch), str(levels)] + (['--count'] if count else [])
        p = subprocess.run(cmd)
        if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started
            print('%s B = %d levels = %d ended with status %d: stopping' % (what, batch, levels, p.returncode), flush=True)
            sys.exit(p.returncode)


if __name__ == '__main__':
    main()
