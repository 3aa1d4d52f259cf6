"""Ray casting on the GPU (csrc/nr_ray_mesh.hip through neural_renderer_amd/ray_mesh.py): every shape that crosses a wave, a tile
and a split with a remainder against the float64 restatement of tests/ray_ref.py within its derived bounds -- t, ids, weights and
the three gradients --, the exact lattice for three splits, collapsed faces and non-finite input on the device, the bit-level
properties (two runs, an image alone or in a batch, split or not, layouts and streams), the two implementations' ids, whether
the vertex gradient repeats, the rasterizer cross-check, a short fit and the example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_ref as R
from test_ray_mesh import (CROSS_EYES, SHAPES, analysis, case, check_any_hit, check_case, check_collapsed, check_lattice,
                           check_miss_rows, check_non_finite, check_visibility, cross_check_renderer, cross_check_scenes, host,
                           tensors)

pytestmark = pytest.mark.gpu


def run_all(o, d, v, f, implementation='hip'):
    """Every output of the two searches: (t, ids, weights, occluded)"""
    import neural_renderer_amd as nr
    return nr.ray_mesh_intersect(o, d, v, f, implementation=implementation) + \
        (nr.ray_mesh_occluded(o, d, v, f, implementation=implementation),)


def same_bits(a, b):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), k


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_kernels_against_the_float64_restatement(k):
    check_case(k, device='cuda', implementation='hip', what='hip %s' % (SHAPES[k],))


def test_miss_rows_give_exact_zeros_on_the_device():
    check_miss_rows('cuda', 'hip')


def test_lattice_is_exact_on_the_device(monkeypatch):
    from neural_renderer_amd import ray_mesh
    for split in (0, 1, 3):
        monkeypatch.setattr(ray_mesh, '_SPLIT', split)
        check_lattice('cuda', 'hip')


def test_collapsed_faces_on_the_device():
    check_collapsed('cuda', 'hip')


def test_non_finite_input_on_the_device():
    check_non_finite('cuda', 'hip')


def test_any_hit_equals_first_hit_on_the_device(monkeypatch):
    from neural_renderer_amd import ray_mesh
    for split in (0, 1, 3):
        monkeypatch.setattr(ray_mesh, '_SPLIT', split)
        check_any_hit('cuda', 'hip')


def test_vertex_visibility_on_the_device():
    import torch
    assert torch.equal(check_visibility('cuda', 'hip').cpu(), check_visibility('cpu', 'torch'))


def test_two_runs_and_an_image_alone_have_the_same_bits():
    for k in (2, 3):
        o, d, v, f = tensors(*case(k), device='cuda')
        first = run_all(o, d, v, f)
        same_bits(first, run_all(o, d, v, f))
        b = v.shape[0] - 1
        alone = run_all(o if o.dim() == 2 else o[b:b + 1], d if d.dim() == 2 else d[b:b + 1], v[b:b + 1], f)
        same_bits([x[b:b + 1] for x in first], alone)


def test_split_and_unsplit_agree_to_the_bit(monkeypatch):
    from neural_renderer_amd import _lib, ray_mesh
    lib = _lib.load()
    for k in (5, 3, 2):
        B, N, F, _ = SHAPES[k]
        o, d, v, f = tensors(*case(k), device='cuda')
        monkeypatch.setattr(ray_mesh, '_SPLIT', 1)
        assert lib.nr_ray_mesh_workspace_bytes(B, N, F, 0, 1) == 0 and lib.nr_ray_mesh_workspace_bytes(B, N, F, 1, 1) == 0
        unsplit = run_all(o, d, v, f)
        for split in (0, 2, 3, 1000):
            monkeypatch.setattr(ray_mesh, '_SPLIT', split)
            same_bits(unsplit, run_all(o, d, v, f))
    assert lib.nr_ray_mesh_workspace_bytes(1, 70, 5000, 0, 0) > 0      # (1, 70, 5000) splits its faces by itself
    assert lib.nr_ray_mesh_workspace_bytes(2, 1027, 515, 1, 3) > 0


def test_layouts_and_a_side_stream_have_the_dense_call_s_bits():
    import torch
    o, d, v, f = tensors(*case(2), device='cuda')
    dense = run_all(o, d, v, f)
    assert int((dense[1] >= 0).sum()) > 0 and bool(dense[3].any())

    def offset(x, k):
        flat = torch.zeros(x.numel() + k, dtype=x.dtype, device=x.device)
        flat[k:] = x.reshape(-1)
        return flat[k:].view(x.shape)

    def strided(x):
        wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=x.dtype, device=x.device)
        wide[..., ::2] = x
        return wide[..., ::2]

    def permuted(x):
        return x.permute(*reversed(range(x.dim()))).contiguous().permute(*reversed(range(x.dim())))

    for name, change in (('offset4', lambda x: offset(x, 1)), ('offset8', lambda x: offset(x, 2)),
                         ('offset12', lambda x: offset(x, 3)), ('strided', strided), ('permuted', permuted)):
        assert not (change(o).is_contiguous() and change(o).data_ptr() % 16 == 0), name
        same_bits(dense, run_all(change(o), change(d), change(v), change(f)))
    same_bits(dense, run_all(o, d, v, f.long()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run_all(o, d, v, f)
    torch.cuda.current_stream().wait_stream(side)
    same_bits(dense, on_side)


def test_hip_and_torch_agree_on_the_ids_of_every_ray_that_is_kept():
    for k in (1, 2, 3, 5):
        o, d, v, f = tensors(*case(k), device='cuda')
        hip, eager = run_all(o, d, v, f), run_all(o, d, v, f, 'torch')
        keep = ~analysis(k)[1]
        assert np.array_equal(host(hip[1])[keep], host(eager[1])[keep]) and np.array_equal(host(hip[3])[keep], host(eager[3])[keep])


def test_the_vertex_gradient_repeats():
    """The gradients go through torch's indexing backward (index_put_ with accumulate).  Measured on the MI355X: the vertex
    gradient of two backward runs repeated bit for bit on every shape here, so it is asserted (README "Ray casting")."""
    import torch
    import neural_renderer_amd as nr
    for k in (2, 3, 5):
        o, d, v, f = tensors(*case(k), device='cuda', grad=True)
        g = torch.tensor(np.random.default_rng(5).uniform(-1, 1, SHAPES[k][:2]).astype(np.float32), device='cuda')
        runs = []
        for _ in range(2):
            t = nr.ray_mesh_intersect(o, d, v, f, implementation='hip')[0]
            runs.append(torch.autograd.grad(t, [o, d, v], g))
        repeated = [torch.equal(a, b) for a, b in zip(*runs)]
        print('shape %s: gradients repeated bit for bit (origins, directions, vertices): %s' % (SHAPES[k], repeated))
        assert all(repeated), (SHAPES[k], repeated)


def test_dispatch(monkeypatch):
    import torch
    import neural_renderer_amd as nr
    from neural_renderer_amd import _lib, ray_mesh
    o, d, v, f = tensors(*case(1), device='cuda')
    with pytest.raises(ValueError) as err:
        nr.ray_mesh_intersect(o.double(), d.double(), v.double(), f, implementation='hip')
    assert ray_mesh._NEEDS in str(err.value)
    calls = []
    launch = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: (calls.append(name), launch(name, *a, **k))[1])
    nr.ray_mesh_intersect(o, d, v, f)
    nr.ray_mesh_occluded(o, d, v, f)
    nr.vertex_visibility(v, f, torch.tensor((0.0, 0.0, 3.0), device='cuda'))
    assert calls == ['nr_ray_mesh_first_hit', 'nr_ray_mesh_any_hit', 'nr_ray_mesh_any_hit']

    def no_launch(*a, **k):
        raise AssertionError('a kernel was launched')

    monkeypatch.setattr(_lib, 'launch', no_launch)
    assert nr.ray_mesh_intersect(o.double(), d.double(), v.double(), f)[0].dtype == torch.float64   # float64: plain torch
    nr.ray_mesh_intersect(o, d, v, f, implementation='torch')


def test_rays_through_the_pixel_centres_return_the_rasterizer_s_depth_map():
    """Two unrelated kernels and two formulas held against each other: ray_mesh_intersect along camera_rays against
    Renderer.render_depth at 32 x 32 from three eyes, on icosphere(2) and the teapot.  The cap and the bound were established
    on the CPU (test_ray_mesh.test_float64_rays_agree_with_the_oracle_rasterizer_within_the_cap)."""
    import torch
    import neural_renderer_amd as nr
    S, B = 32, len(CROSS_EYES)
    renderer = cross_check_renderer(S)
    renderer.eye = renderer.eye.cuda()
    like = torch.zeros(1, device='cuda')
    origins, directions = nr.camera_rays(renderer, B, like)
    rot = host(nr.camera_rotation(renderer, B, like.double()))
    tangent = math.tan(np.float32(30.0) / np.float32(180.0) * np.float32(3.1416))
    for name, v, f in cross_check_scenes():
        vertices = torch.tensor(np.repeat(v[None], B, 0), device='cuda')
        faces = torch.tensor(f, device='cuda')
        depth = renderer.render_depth(vertices, faces[None].expand(B, -1, -1))
        t, ids, w = nr.ray_mesh_intersect(origins, directions, vertices, faces, near=renderer.near, far=renderer.far,
                                          implementation='hip')
        assert tuple(depth.shape) == (B, S, S) and tuple(t.shape) == (B, S * S)
        o64, d64 = host(origins)[:, None], host(directions)
        b_t = R.pair_values(o64, d64, host(vertices), f, host(ids))[2]
        share, worst = R.check_depth_maps(host(depth), host(t), host(ids), b_t, o64, d64, host(vertices), f, CROSS_EYES, rot, tangent, S,
                                          renderer.far, what='render_depth against ray_mesh_intersect, %s' % name)
        assert worst <= 1.0 and int((ids >= 0).sum()) > 50


def test_a_short_fit_along_the_rays_descends():
    import torch
    import neural_renderer_amd as nr
    rng = np.random.default_rng(21)
    directions = rng.normal(size=(300, 3))
    directions = torch.tensor(directions / np.linalg.norm(directions, axis=1, keepdims=True), dtype=torch.float32, device='cuda')
    origins = -3.0 * directions
    target, faces = nr.icosphere(2, 0.8, device='cuda')
    target = target * torch.tensor((1.0, 0.7, 0.5), device='cuda')
    with torch.no_grad():
        t_scan, ids_scan, _ = nr.ray_mesh_intersect(origins, directions, target, faces)
    assert bool((ids_scan >= 0).all())
    sphere, faces = nr.icosphere(2, 0.5, device='cuda')
    vertices = torch.nn.Parameter(sphere)
    optimizer = torch.optim.Adam([vertices], lr=1e-2)
    losses = []
    for _ in range(11):
        optimizer.zero_grad()
        t, ids, _ = nr.ray_mesh_intersect(origins, directions, vertices, faces)
        hit = ids >= 0
        loss = ((t - t_scan)[hit] ** 2).mean() + 0.1 * nr.laplacian_loss(vertices, faces)
        loss.backward()
        assert torch.isfinite(vertices.grad).all() and float(vertices.grad.abs().sum()) > 0
        optimizer.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


def test_example_ray_depth_runs(tmp_path):
    """examples/example_ray_depth.py as a child process with 20 steps: it exits 0 and its last printed loss is below its first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    out = str(tmp_path / 'example_ray_depth_test.obj')
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_ray_depth.py'), '20', '-oo', out], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('step')]
    assert len(losses) >= 2 and losses[-1] < losses[0]
