"""ssim_loss forward + backward: the HIP kernels against the module's own torch path (ssim_loss_torch: the windowed sums
tap by tap, autograd) and against SSIM as a user spells it without the feature (five grouped conv2d with the 2-D window,
autograd; in this script) in the same run, with and without a mask.

    python scripts/ssim_timing.py            # one JSON line per row

Rows: B x 3 x S x S for (B, S) in (64, 256), (64, 64), (1, 1024), window 11, padding 'same', reduction 'mean'; a step is
loss.sum().backward() on a leaf image.  The three variants of a row alternate inside one child process: warm-up, then
`repeats` rounds of `steps` steps each, timed with device events; a row reports the median round and the spread (min, max)
of each variant, and the peak device memory of one step of each above what the inputs hold (torch's allocator statistics:
for 'hip' that is the three maps the forward keeps for the backward, the gradient and the workspace).  Every row runs in a
child process of its own under `timeout`, and the first one that fails ends the run.  Informational: no threshold.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_TIMEOUT = 150  # seconds per child
ROWS = [(batch, size, masked) for batch, size in ((64, 256), (64, 64), (1, 1024)) for masked in (0, 1)]


def ssim_spelled(x, t, m, n=11, sigma=1.5, c1=0.01 ** 2, c2=0.03 ** 2):
    """what a user writes: five grouped conv2d with the 2-D Gaussian window, zero padding, the masked mean per image"""
    import torch
    import torch.nn.functional as F
    C = x.shape[1]
    w = torch.exp(-(torch.arange(n, dtype=torch.float32, device=x.device) - n // 2) ** 2 / (2 * sigma * sigma))
    w = w / w.sum()
    w2 = (w[:, None] * w[None, :]).expand(C, 1, n, n).contiguous()
    G = lambda z: F.conv2d(z, w2, padding=n // 2, groups=C)
    mux, muy = G(x), G(t)
    sxx, syy, sxy = G(x * x) - mux * mux, G(t * t) - muy * muy, G(x * t) - mux * muy
    S = ((2 * mux * muy + c1) * (2 * sxy + c2)) / ((mux * mux + muy * muy + c1) * (sxx + syy + c2))
    if m is None:
        return (1 - S).mean((1, 2, 3))
    return (m[:, None] * (1 - S)).sum((1, 2, 3)) / (C * m.sum((1, 2)))


def timed(variants, steps, repeats, warmup=3):
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


def peak_megabytes(fn):
    """the peak of torch's allocator during one step, above what is allocated before it"""
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def row(batch, size, masked, steps, repeats):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import image_losses
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device='cpu').manual_seed(3)
    image = torch.rand((batch, 3, size, size), generator=gen).to(dev).requires_grad_(True)
    target = torch.rand((batch, 3, size, size), generator=gen).to(dev)
    mask = (torch.rand((batch, size, size), generator=gen) > 0.3).float().to(dev) if masked else None

    def step(fn):
        def run():
            image.grad = None
            fn(image, target, mask).sum().backward()
        return run
    variants = {'hip': step(lambda x, t, m: nr.ssim_loss(x, t, m, implementation='hip')),
                'torch': step(lambda x, t, m: image_losses.ssim_loss_torch(x, t, m)),
                'conv2d': step(ssim_spelled)}
    out = {'row': 'ssim', 'B': batch, 'C': 3, 'size': size, 'window': 11, 'mask': bool(masked)}
    for n, v in timed(variants, steps, repeats).items():
        out[n + '_ms'] = round(v[len(v) // 2], 4)
        out[n + '_ms_min_max'] = [round(v[0], 4), round(v[-1], 4)]
    out['torch_over_hip'] = round(out['torch_ms'] / out['hip_ms'], 2)
    out['conv2d_over_hip'] = round(out['conv2d_ms'] / out['hip_ms'], 2)
    for n, fn in variants.items():
        out[n + '_peak_MB'] = peak_megabytes(fn)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--one', nargs=3, metavar=('BATCH', 'SIZE', 'MASKED'), help='(a child: one row)')
    args = ap.parse_args()
    if args.one:
        row(int(args.one[0]), int(args.one[1]), int(args.one[2]), args.steps, args.repeats)
        return
    for batch, size, masked in ROWS:
        cmd = ['timeout', '-k', '10', str(ROW_TIMEOUT), sys.executable, os.path.abspath(__file__), '--steps', str(args.steps),
               '--repeats', str(args.repeats), '--one', str(batch), str(size), str(masked)]
        p = subprocess.run(cmd)
        if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started
            print('B = %d size = %d mask = %d ended with status %d: stopping' % (batch, size, masked, p.returncode), flush=True)
            sys.exit(p.returncode)


if __name__ == '__main__':
    main()
