"""Isosurface extraction on the GPU (csrc/nr_isosurface.hip through neural_renderer_amd/isosurface.py): the kernels' integers
against the NumPy restatement on the fixed rows, against the default run length with small runs (several workgroups, a partly
filled last one, a run of several rounds, more than one pass of both scans), against the torch path on a field that shows
every case, the bit-level properties (batch, repeat, layouts, streams), positions and gradients end to end within the derived
bounds, the round trip through `voxelize`, and the example."""
import os
import subprocess
import sys

import pytest

import isosurface_ref as R
from test_isosurface import FIELDS, check_batch, check_integers, check_positions_and_gradients, round_trip

pytestmark = pytest.mark.gpu


def extract(values, implementation='hip', **kw):
    import neural_renderer_amd as nr
    return nr.extract_isosurface(values, implementation=implementation, **kw)


def same(a, b):
    import torch
    assert a.faces.dtype == b.faces.dtype and a.edge_nodes.dtype == b.edge_nodes.dtype
    assert a.faces.shape == b.faces.shape and a.edge_nodes.shape == b.edge_nodes.shape
    assert torch.equal(a.edge_nodes, b.edge_nodes) and torch.equal(a.faces, b.faces)


@pytest.mark.parametrize('inside', ('below', 'above'))
@pytest.mark.parametrize('name', sorted(FIELDS))
def test_kernels_equal_the_restatement(name, inside):
    check_integers(name, 'cuda', 'hip', inside=inside)


@pytest.mark.parametrize('run', (8, 96, 300, 4096))
def test_run_length_does_not_matter(monkeypatch, run):
    """(40,9,7) = 2520 nodes.  run 96: 27 workgroups, the last one partly filled; 300: two rounds, the second partly filled;
    8: 315 workgroups, two passes of the scan of their totals; 4096: one workgroup, ten rounds"""
    import torch
    from neural_renderer_amd import isosurface
    values = torch.tensor(R.noise_field((40, 9, 7), 21)).cuda()
    batch = torch.stack((values, -values.flip(0), torch.ones_like(values)))
    monkeypatch.setattr(isosurface, '_RUN', 0)
    want, want_batch = extract(values), extract(batch)
    assert want.num_faces > 0
    monkeypatch.setattr(isosurface, '_RUN', run)
    same(extract(values), want)
    for got, ref in zip(extract(batch), want_batch):
        same(got, ref)
    same(want, extract(values, 'torch'))


def test_many_images_take_several_passes_of_the_image_scan():
    """300 images: the scan over the images' totals walks more than one pass; each image equals the torch path's"""
    import torch
    batch = torch.tensor(R.noise_field((300, 2, 3, 2), 22)).cuda()
    got, want = extract(batch), extract(batch, 'torch')
    assert len(got) == 300 and sum(s.num_faces for s in got) > 300
    for a, b in zip(got, want):
        same(a, b)


def test_kernels_equal_the_torch_path_on_every_case():
    """(64,48,80), smooth with low-amplitude noise: all 14 non-trivial masks of each of the six permutations occur -- asserted on
    the input, by the restatement's histogram"""
    import torch
    field = R.smooth_noisy_field()
    assert (R.case_histogram(field)[:, 1:15] > 0).all()
    values = torch.tensor(field).cuda()
    for inside in ('below', 'above'):
        got, want = extract(values, inside=inside), extract(values, 'torch', inside=inside)
        assert got.num_faces > 100000
        same(got, want)


def test_batch_equals_single_calls_on_the_device():
    check_batch('cuda', 'hip')


def test_two_runs_give_the_same_bits():
    import torch
    values = torch.tensor(R.smooth_noisy_field((33, 20, 27), 7)).cuda()
    same(extract(values), extract(values))


def test_layouts():
    """a permuted view and a slice that starts off the 16-byte grid give what their dense copies give (_lib.dense)"""
    import torch
    base = torch.tensor(R.noise_field((7, 6, 5), 23)).cuda()
    permuted = base.permute(2, 0, 1)
    assert not permuted.is_contiguous()
    same(extract(permuted), extract(permuted.contiguous()))
    flat = torch.tensor(R.noise_field((5 * 6 * 7 + 3,), 24)).cuda()
    offset = flat[3:].view(5, 6, 7)
    assert offset.data_ptr() % 16 != 0
    same(extract(offset), extract(offset.clone()))
    same(extract(offset), extract(offset, 'torch'))


def test_side_stream():
    import torch
    values = torch.tensor(R.smooth_noisy_field((33, 20, 27), 7)).cuda()
    want = extract(values)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = extract(values)
    stream.synchronize()
    same(got, want)


def test_non_finite_values_raise_on_the_device():
    import torch
    values = torch.tensor(R.noise_field((5, 6, 7), 4)).cuda()
    for bad in (float('nan'), float('-inf')):
        broken = values.clone()
        broken[4, 5, 6] = bad
        with pytest.raises(ValueError, match='extract_isosurface: values must be finite'):
            extract(broken)
        with pytest.raises(ValueError, match='extract_isosurface: values must be finite'):
            extract(torch.stack((values, broken)))


@pytest.mark.parametrize('mode', ('centers', 'corners', 'positions'))
@pytest.mark.parametrize('name', ('sphere', 'noise567'))
def test_marching_tetrahedra_end_to_end(name, mode):
    import torch
    check_positions_and_gradients(name, torch.float32, 'cuda', 'hip', mode)


def test_round_trip_through_voxelize():
    round_trip('cuda', 'hip')


def test_example_isosurface_fit_runs(tmp_path):
    """examples/example_isosurface_fit.py as a child process with 8 steps: it exits 0 and its last printed loss is below its first"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = os.path.join(root, 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import make_data
    make_data.main()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ex, os.environ.get('PYTHONPATH', '')]))
    out = str(tmp_path / 'example_isosurface_fit_test.obj')
    run = subprocess.run([sys.executable, os.path.join(ex, 'example_isosurface_fit.py'), '8', '-oo', out], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    losses = [float(line.split('loss')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('step')]
    faces = [int(line.split('faces')[1].split()[0]) for line in run.stdout.splitlines() if line.startswith('step')]
    assert len(losses) == 8 and losses[-1] < losses[0] and min(faces) > 0
