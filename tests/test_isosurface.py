"""Isosurface extraction on the CPU (neural_renderer_amd/isosurface.py's torch path) against the NumPy restatement of
tests/isosurface_ref.py: the integers entry for entry on the fixed rows, both `inside` modes, the manifold checks, the package's
orientation convention, positions and gradients within the derived bounds in float32 and float64, batches, argument errors,
and the case table of csrc/nr_marching_tets.h against the module's."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import isosurface_ref as R
import neural_renderer_amd as nr
from neural_renderer_amd import isosurface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    'sphere': R.sphere_field, 'lattice': R.lattice_field, 'torus': R.torus_field,
    'noise657': lambda: R.noise_field((6, 5, 7), 1), 'noise222': lambda: R.noise_field((2, 2, 2), 2),
    'noise293': lambda: R.noise_field((2, 9, 3), 3), 'noise567': lambda: R.noise_field((5, 6, 7), 4),
}
BOUNDS = ((-1.0, 1.0), (-0.5, 0.75), (0.25, 2.0))
WINDING_SUM = 1e-5  # the summation error allowed to a winding number on a closed mesh


@functools.lru_cache(maxsize=None)
def field(name):
    f = FIELDS[name]()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name, inside='below'):
    """(edge_nodes, faces) of the restatement, computed once and left unchanged"""
    en, fa = R.extract(field(name), 0.0, inside)
    en.setflags(write=False)
    fa.setflags(write=False)
    return en, fa


def host(t):
    return t.detach().cpu().numpy()


def check_integers(name, device, implementation, dtype=torch.float32, inside='below'):
    en, fa = reference(name, inside)
    s = nr.extract_isosurface(torch.tensor(field(name)).to(device=device, dtype=dtype), 0.0, inside, implementation=implementation)
    assert s.faces.dtype == torch.int32 and s.edge_nodes.dtype == torch.int32
    assert s.faces.shape == (len(fa), 3) and s.edge_nodes.shape == (len(en), 2)
    assert (s.num_vertices, s.num_faces, s.grid_shape, s.iso, s.inside) == (len(en), len(fa), field(name).shape, 0.0, inside)
    assert np.array_equal(host(s.edge_nodes), en) and np.array_equal(host(s.faces), fa), name
    if name in R.ROWS and inside == 'below':   # the fixed rows' counts
        assert (len(en), len(fa)) == R.ROWS[name][1:]
    return s


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
@pytest.mark.parametrize('name', sorted(FIELDS))
def test_torch_path_equals_the_restatement(name, dtype):
    check_integers(name, 'cpu', None, dtype)


def test_restatement_uses_every_crossing_edge():
    for name in FIELDS:
        en, fa = reference(name)
        assert np.array_equal(en, R.crossing_edges(field(name))), name
        assert R.mesh_report(fa, len(en))['all_used'], name


def canonical(faces):
    """every triangle rotated to start at its smallest entry, the rows sorted"""
    f = np.asarray(faces)
    k = f.argmin(1)
    f = np.stack([f[np.arange(len(f)), (k + c) % 3] for c in range(3)], 1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


@pytest.mark.parametrize('name', ('sphere', 'torus', 'noise567'))
def test_both_inside_modes(name):
    """'above' against the restatement; -f below IS f above; f above has f below's vertices and the reversed triangles"""
    f = torch.tensor(field(name))
    assert (f != 0).all()
    above = check_integers(name, 'cpu', None, inside='above')
    negated = nr.extract_isosurface(-f, 0.0, 'below')
    assert torch.equal(negated.faces, above.faces) and torch.equal(negated.edge_nodes, above.edge_nodes)
    below = nr.extract_isosurface(f, 0.0, 'below')
    assert torch.equal(below.edge_nodes, above.edge_nodes)
    assert np.array_equal(canonical(host(below.faces)), canonical(host(above.faces)[:, ::-1]))
    assert torch.equal(below.vertices(f), above.vertices(f))


def test_constant_field_gives_empty_outputs():
    for values in (torch.ones(3, 4, 5), torch.full((2, 3, 4, 5), -2.0)):
        out = nr.extract_isosurface(values)
        for s in (out if isinstance(out, list) else [out]):
            assert s.faces.shape == (0, 3) and s.faces.dtype == torch.int32
            assert s.edge_nodes.shape == (0, 2) and s.edge_nodes.dtype == torch.int32
            v = s.vertices(values if values.dim() == 3 else values[0])
            assert v.shape == (0, 3) and v.dtype == torch.float32
    v, f = nr.marching_tetrahedra(torch.ones(3, 4, 5, dtype=torch.float64))
    assert v.shape == (0, 3) and v.dtype == torch.float64 and f.shape == (0, 3)


def check_closed(faces, vertices, euler):
    rep = R.mesh_report(faces, len(vertices))
    assert rep['directed_max'] == 1              # every directed edge at most once
    assert rep['once'] == 0 and rep['more'] == 0 and rep['twice'] * 2 == 3 * len(faces)   # every undirected edge exactly twice
    assert rep['euler'] == euler and rep['all_used']
    assert R.signed_volume(vertices, faces) > 0


@pytest.mark.parametrize('name,euler', (('sphere', 2), ('torus', 0)))
def test_manifold(name, euler):
    f = torch.tensor(field(name))
    v, faces = nr.marching_tetrahedra(f, bounds=(-6.0, 6.0))
    check_closed(host(faces), host(v), euler)


def test_open_surfaces_end_on_the_grid_boundary():
    """an edge in one face has both vertices on the grid's boundary (lattice and noise); none is in more than two"""
    for name in ('lattice', 'noise657', 'noise293'):
        en, fa = reference(name)
        D, H, W = field(name).shape
        rep = R.mesh_report(fa, len(en))
        assert rep['directed_max'] == 1 and rep['more'] == 0
        n = en[rep['boundary']]                                   # [E,2 vertices,2 nodes]
        i, j, k = n // (H * W), n // W % H, n % W
        on_face = [(c == 0).all((1, 2)) | (c == m - 1).all((1, 2)) for c, m in ((i, D), (j, H), (k, W))]
        assert (on_face[0] | on_face[1] | on_face[2]).all(), name


def test_orientation_is_the_package_convention():
    """the winding number of the sphere's centre is 1: on a closed outward mesh it is 1 up to summation error"""
    v, faces = nr.marching_tetrahedra(torch.tensor(field('sphere')), bounds=(-6.0, 6.0))
    w = nr.winding_number(torch.tensor([[-0.013, -0.083, 0.018]]), v, faces)
    print('winding number at the centre', float(w))
    assert abs(float(w) - 1.0) <= WINDING_SUM


def positions_case(name, dtype, device, implementation, mode):
    """-> (vertices, edge_nodes, values, positions or None, the restatement's node positions)"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    f = field(name)
    values = torch.tensor(f).to(device=device, dtype=dtype).requires_grad_(True)
    if mode == 'positions':
        rng = np.random.default_rng(11)
        grid = R.node_positions(f.shape, (-1, 1), 'corners', npdt) + rng.uniform(-0.04, 0.04, (f.size, 3))
        grid = grid.astype(npdt)
        positions = torch.from_numpy(grid.reshape(f.shape + (3,))).to(device).requires_grad_(True)
        v, faces = nr.marching_tetrahedra(values, positions=positions, implementation=implementation)
        return v, faces, values, positions, grid.astype(np.float64)
    v, faces = nr.marching_tetrahedra(values, bounds=BOUNDS, align=mode, implementation=implementation)
    return v, faces, values, None, R.node_positions(f.shape, BOUNDS, mode, npdt)


def check_positions_and_gradients(name, dtype, device, implementation, mode):
    npdt = np.float32 if dtype == torch.float32 else np.float64
    en, fa = reference(name)
    v, faces, values, positions, grid = positions_case(name, dtype, device, implementation, mode)
    assert np.array_equal(host(faces), fa) and v.dtype == dtype and v.shape == (len(en), 3)
    want, bound = R.positions(field(name), en, 0.0, grid, npdt)
    r_v = R.ratio(np.abs(host(v).astype(np.float64) - want), bound)
    g = np.random.default_rng(3).normal(size=want.shape).astype(npdt)
    (v * torch.from_numpy(g).to(device)).sum().backward()
    (gs, bs), (gp, bp) = R.gradients(field(name), en, 0.0, grid, g, npdt)
    r_s = R.ratio(np.abs(host(values.grad).astype(np.float64).reshape(-1) - gs), bs)
    r_p = 0.0
    if positions is not None:
        r_p = R.ratio(np.abs(host(positions.grad).astype(np.float64).reshape(-1, 3) - gp), bp)
    print('%s %s %s %s: ratios to the bounds: positions %.4f, grad values %.4f, grad positions %.4f'
          % (name, dtype, device, mode, r_v, r_s, r_p))
    assert r_v <= 1.0 and r_s <= 1.0 and r_p <= 1.0
    return r_v, r_s, r_p


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
@pytest.mark.parametrize('mode', ('centers', 'corners', 'positions'))
@pytest.mark.parametrize('name', ('sphere', 'noise567'))
def test_positions_and_gradients_within_the_bounds(name, mode, dtype):
    check_positions_and_gradients(name, dtype, 'cpu', None, mode)


def test_voxel_centers_are_the_nodes_of_align_centers():
    G = 12
    f = torch.tensor(field('sphere'))
    s = nr.extract_isosurface(f)
    centres = nr.voxel_centers(G, BOUNDS)
    a, b = s.edge_nodes[:, 0].long(), s.edge_nodes[:, 1].long()
    pa, pb = isosurface._node_positions('test', s.grid_shape, BOUNDS, 'centers', f, (a, b))
    assert torch.equal(pa, centres[a]) and torch.equal(pb, centres[b])
    sa, sb = f.reshape(-1)[a], f.reshape(-1)[b]
    assert torch.equal(s.vertices(f, BOUNDS), centres[a] + ((0.0 - sa) / (sb - sa))[:, None] * (centres[b] - centres[a]))


def test_second_derivative_runs():
    values = torch.tensor(field('sphere')).double().requires_grad_(True)
    v, _ = nr.marching_tetrahedra(values)
    g1, = torch.autograd.grad(v.sum(), values, create_graph=True)
    g2, = torch.autograd.grad((g1 * g1).sum(), values)
    assert torch.isfinite(g2).all() and float(g2.abs().max()) > 0


def test_vertices_on_rescaled_values():
    f = torch.tensor(field('sphere'))
    en, _ = reference('sphere')
    s = nr.extract_isosurface(f)
    want, bound = R.positions(field('sphere'), en, 0.0, R.node_positions(f.shape, BOUNDS, 'centers', np.float32), np.float32)
    r = R.ratio(np.abs(host(s.vertices(2 * f, BOUNDS)).astype(np.float64) - want), bound)
    print('rescaled values: ratio %.4f' % r)
    assert r <= 1.0


def check_batch(device, implementation):
    fields = [torch.tensor(field('noise567')), torch.full((5, 6, 7), 3.0), torch.from_numpy(R.noise_field((5, 6, 7), 9))]
    batch = torch.stack(fields).to(device)
    for images in (batch, batch[:1]):
        out = nr.extract_isosurface(images, implementation=implementation)
        assert isinstance(out, list) and len(out) == images.shape[0]
        for b, s in enumerate(out):
            one = nr.extract_isosurface(images[b], implementation=implementation)
            assert torch.equal(s.faces, one.faces) and torch.equal(s.edge_nodes, one.edge_nodes)
            assert s.faces.dtype == torch.int32 and s.faces.shape == (one.num_faces, 3)
        pairs = nr.marching_tetrahedra(images, bounds=BOUNDS, implementation=implementation)
        for b, (v, faces) in enumerate(pairs):
            v1, f1 = nr.marching_tetrahedra(images[b], bounds=BOUNDS, implementation=implementation)
            assert torch.equal(v, v1) and torch.equal(faces, f1)
    assert out[0].num_faces > 0
    out = nr.extract_isosurface(batch, implementation=implementation)
    assert out[1].num_faces == 0 and out[1].num_vertices == 0 and out[2].num_faces > 0
    if out[0].num_faces and out[2].num_faces:   # views of shared allocations
        assert out[0].faces.untyped_storage().data_ptr() == out[2].faces.untyped_storage().data_ptr()
    positions = torch.rand(3, 5, 6, 7, 3, device=device)
    for b, (v, faces) in enumerate(nr.marching_tetrahedra(batch, positions=positions, implementation=implementation)):
        assert torch.equal(v, nr.marching_tetrahedra(batch[b], positions=positions[b], implementation=implementation)[0])


def test_batch_equals_single_calls():
    check_batch('cpu', None)


def test_argument_errors():
    f = torch.tensor(field('noise567'))
    for bad in (torch.zeros(5, 6), torch.zeros(1, 2, 3, 4, 5), torch.zeros(3, 4, 5, dtype=torch.int32), [[[0.0]]]):
        with pytest.raises(ValueError, match=r'extract_isosurface: values must be a float tensor \[D, H, W\] or \[batch size, D, H, W\]'):
            nr.extract_isosurface(bad)
    with pytest.raises(ValueError, match='extract_isosurface: D, H and W must be 2 at least'):
        nr.extract_isosurface(torch.zeros(1, 4, 5))
    with pytest.raises(ValueError, match='marching_tetrahedra: D, H and W must be 2 at least'):
        nr.marching_tetrahedra(torch.zeros(2, 4, 1, 5))
    with pytest.raises(ValueError, match="extract_isosurface: inside must be 'below' or 'above'"):
        nr.extract_isosurface(f, inside='under')
    with pytest.raises(ValueError, match='extract_isosurface: iso must be a number'):
        nr.extract_isosurface(f, iso='0')
    with pytest.raises(ValueError, match="marching_tetrahedra: align must be 'centers' or 'corners'"):
        nr.marching_tetrahedra(f, align='middle')
    with pytest.raises(ValueError, match='marching_tetrahedra: bounds must be a pair'):
        nr.marching_tetrahedra(f, bounds=(1.0, -1.0))
    with pytest.raises(ValueError, match='marching_tetrahedra: positions must be a float tensor of the shape of values'):
        nr.marching_tetrahedra(f, positions=torch.zeros(5, 6, 7))
    s = nr.extract_isosurface(f)
    with pytest.raises(ValueError, match=r'IsoSurface.vertices: positions must be a float tensor of shape \(5, 6, 7, 3\)'):
        s.vertices(f, positions=torch.zeros(5, 6, 7, 2))
    with pytest.raises(ValueError, match='IsoSurface.vertices: values must be a float tensor of the grid shape'):
        s.vertices(f[:4])
    with pytest.raises(ValueError, match="IsoSurface.vertices: align must be"):
        s.vertices(f, align='x')
    with pytest.raises(ValueError, match='IsoSurface.vertices: bounds must be a pair'):
        s.vertices(f, bounds=((0, 1), (0, 1)))
    for bad in (float('nan'), float('inf')):
        g = f.clone()
        g[2, 3, 4] = bad
        with pytest.raises(ValueError, match='extract_isosurface: values must be finite'):
            nr.extract_isosurface(g)
    with pytest.raises(ValueError, match="extract_isosurface: implementation must be None, 'torch' or 'hip'"):
        nr.extract_isosurface(f, implementation='cuda')
    for name, call in (('extract_isosurface', nr.extract_isosurface), ('marching_tetrahedra', nr.marching_tetrahedra)):
        with pytest.raises(ValueError) as e:
            call(f, implementation='hip')
        assert str(e.value) == name + ': ' + isosurface._NEEDS
    assert '65535' in isosurface._NEEDS and '2^31' in isosurface._NEEDS


def test_no_new_autograd_function():
    assert not [n for n, o in vars(isosurface).items() if isinstance(o, type) and issubclass(o, torch.autograd.Function)]


def header_tables():
    src = open(os.path.join(ROOT, 'neural_renderer_amd', 'csrc', 'nr_marching_tets.h')).read()
    out = {}
    for name in ('TET_CORNERS', 'TET_TRIANGLES', 'TET_TABLE'):
        body = re.search(r'constexpr unsigned char %s[\[\]0-9]*\s*=\s*\{(.*?)\};' % name, src, re.S).group(1)
        out[name] = [int(x) for x in re.findall(r'\d+', body)]
    return out


def test_header_table_is_the_modules_table():
    t = header_tables()
    assert t['TET_CORNERS'] == [c for row in isosurface._CORNERS for c in row]
    assert t['TET_TRIANGLES'] == list(isosurface._COUNT)
    assert t['TET_TABLE'] == [x for perm in isosurface._TABLE for row in perm for x in row]
    assert [list(p) for p in isosurface._PERMUTATIONS] == [list(p) for p in R.PERMUTATIONS]


def test_smooth_noisy_field_shows_every_case():
    """the field of the GPU comparison at (64,48,80): all 14 non-trivial masks of each of the six permutations occur"""
    hist = R.case_histogram(R.smooth_noisy_field())
    assert (hist[:, 1:15] > 0).all(), hist


def round_trip(device, implementation):
    """voxelize(hard=False) of icosphere(2) at 16^3, extracted at 0.5 with the same bounds: closed, Euler characteristic 2, and
    every vertex has a winding number within m of 0.5, m the largest |w_a - w_b| / 2 over the crossing edges of the grid.
    The mesh is closed, so w is 0 or 1 at every point and m is 1 / 2, each up to the summation error of a winding number:
    measured on the torch paths m = 0.5000001 and w in [-1.2e-7, 1.0000002], 1.2e-7 outside.  WINDING_SUM, the allowance
    test_orientation_is_the_package_convention makes for that error, is therefore added on both sides."""
    G, bounds = 16, (-0.8, 0.8)
    sphere, faces = nr.icosphere(2, 0.5, device=device)
    grid = nr.voxelize(sphere, faces, G, bounds, hard=False)
    surface = nr.extract_isosurface(grid, 0.5, 'above', implementation=implementation)
    vertices = surface.vertices(grid, bounds)
    check_closed(host(surface.faces), host(vertices), 2)
    w = grid.reshape(-1)
    a, b = surface.edge_nodes[:, 0].long(), surface.edge_nodes[:, 1].long()
    m = float((w[a] - w[b]).abs().max()) / 2
    at = nr.winding_number(vertices, sphere, faces)
    print('round trip: %d vertices, m %.6f, winding numbers in [%.6f, %.6f]' % (len(vertices), m, float(at.min()), float(at.max())))
    assert float(at.min()) >= 0.5 - m - WINDING_SUM and float(at.max()) <= 0.5 + m + WINDING_SUM


def test_round_trip_through_voxelize_on_the_torch_paths():
    round_trip('cpu', None)
