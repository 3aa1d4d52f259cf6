"""Mesh subdivision without a GPU (neural_renderer_amd/subdivision.py): the product's vectorised tables against the
restatement's dict-built ones (tests/subdivision_ref.py), the counts, hand pins, the plain-torch implementation entry by
entry within the derived bound, the sphere template, every argument error, the C ABI's argument checks and
Mesh.subdivide."""
import importlib

import numpy as np
import pytest
import torch

import neural_renderer
import neural_renderer_amd as nr
import subdivision_ref as R
import vertex_ref
from neural_renderer_amd import _lib

S = importlib.import_module('neural_renderer_amd.subdivision')   # (the package attribute of that name is the function)


def images_per_thread():
    """IMAGES of csrc/nr_subdivision.hip: a call of more images spans several groups on the grid's y, the last possibly
    partial.  The GPU tests size their batches from it."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(S.__file__)), 'csrc', 'nr_subdivision.hip')).read()
    return int(re.search(r'constexpr int IMAGES = (\d+)', src).group(1))


def apply_and_grad(plan, x, g, dtype=torch.float32, device='cpu', implementation=None):
    """(plan(x), the gradient of sum(plan(x) g) in x) as numpy"""
    xt = torch.tensor(x, dtype=dtype, device=device, requires_grad=True)
    y = plan(xt, implementation=implementation)
    grad, = torch.autograd.grad((y * torch.tensor(g, dtype=dtype, device=device)).sum(), xt)
    return y.detach().cpu().numpy(), grad.cpu().numpy()


def check_against_restatement(got, grad, ref, images=slice(None), factor=1, what=''):
    """Every entry of the value and of the gradient within factor * C u M of the restatement; prints before it asserts."""
    rv = R.worst_ratio(got, ref.value[images], ref.value_mag[images])
    rg = R.worst_ratio(grad, ref.grad[images], ref.grad_mag[images])
    print('%s: value at %.3f of u M (C = %d), gradient at %.3f (C = %d)' % (what, rv, ref.constant, rg, ref.constant_backward))
    assert rv <= factor * ref.constant and rg <= factor * ref.constant_backward, what


def test_images_per_thread_is_readable():
    assert 1 <= images_per_thread() <= 16


def test_public_names():
    assert nr.subdivision is S.subdivision and nr.subdivide is S.subdivide and nr.icosphere is S.icosphere
    assert nr.Subdivision is S.Subdivision and neural_renderer.subdivide is S.subdivide
    assert all(n in nr.__all__ for n in ('Subdivision', 'subdivision', 'subdivide', 'icosphere'))


@pytest.mark.parametrize('levels', [1, 2])
@pytest.mark.parametrize('scheme', R.SCHEMES)
@pytest.mark.parametrize('name', R.MESHES)
def test_tables_equal_the_restatement(name, scheme, levels):
    v, f = R.mesh(name)
    ref = R.plan(name, levels, scheme)
    plan = nr.subdivision(torch.tensor(f), len(v), levels, scheme)
    assert (plan.levels, plan.scheme, plan.num_vertices_in, plan.num_vertices) == (levels, scheme, len(v), ref.num_vertices)
    assert plan.faces.dtype == torch.int32 and np.array_equal(plan.faces.numpy(), ref.faces)
    assert plan.face_parent.dtype == torch.int64 and np.array_equal(plan.face_parent.numpy(), ref.face_parent)
    assert plan.faces.shape[0] == 4 ** levels * len(f)
    nf, nv = len(f), len(v)
    for k, lev in enumerate(plan._levels):
        off, cols, w = R.csr(ref.rows[k])
        t = lev.forward
        assert t.offsets.dtype == t.cols.dtype == torch.int32 and t.weights.dtype == torch.float32
        assert np.array_equal(t.offsets.numpy(), off) and np.array_equal(t.cols.numpy(), cols)
        assert np.array_equal(t.weights.numpy(), w.astype(np.float32))
        sums = np.add.reduceat(t.weights.numpy().astype(np.float64), off[:-1])
        assert np.abs(sums - 1).max() <= 2.0 ** -23                      # every row sums to 1
        toff, tcols, tw = R.csr(R.transpose(ref.rows[k], ref.sizes[k]))
        b = lev.backward
        assert np.array_equal(b.offsets.numpy(), toff) and np.array_equal(b.cols.numpy(), tcols)
        assert np.array_equal(b.weights.numpy(), tw.astype(np.float32))
        assert (t.num_in, t.num_out, b.num_in, b.num_out) == (ref.sizes[k], ref.sizes[k + 1], ref.sizes[k + 1], ref.sizes[k])
        # Nv' = Nv + E, F' = 4 F; E = 3 F / 2 on a closed manifold
        if k == 0:
            edges = {(min(p, q), max(p, q)) for tri in f.tolist() for p, q in zip(tri, tri[1:] + tri[:1])}
            assert ref.sizes[1] == nv + len(edges)
        if name in R.CLOSED:
            assert ref.sizes[k + 1] - ref.sizes[k] == 3 * nf // 2
        nf *= 4


@pytest.mark.parametrize('name', ['tetra', 'ico1', 'grid'])
def test_euler_characteristic_is_preserved(name):
    v, f = R.mesh(name)
    def chi(nv, faces):
        edges = {(min(p, q), max(p, q)) for tri in faces.tolist() for p, q in zip(tri, tri[1:] + tri[:1])}
        return nv - len(edges) + len(faces)
    want = chi(len(v), f)
    assert want == (1 if name == 'grid' else 2)
    for scheme in R.SCHEMES:
        for levels in (1, 2):
            plan = nr.subdivision(torch.tensor(f), len(v), levels, scheme)
            assert chi(plan.num_vertices, plan.faces.numpy()) == want


def test_tetrahedron_by_hand():
    """Loop, one level: an old vertex is 7/16 v + 3/16 (the other three); the vertex on edge ab is 3/8 (a + b) + 1/8 (c + d)."""
    v, f = R.mesh('tetra')
    out, faces = nr.subdivide(torch.tensor(v), torch.tensor(f), 1, 'loop')
    assert out.dtype == torch.float64 and out.shape == (10, 3) and faces.shape == (16, 3)
    out = out.numpy()
    for a in range(4):
        others = [u for u in range(4) if u != a]
        assert np.allclose(out[a], 7 / 16 * v[a] + 3 / 16 * v[others].sum(0), rtol=0, atol=1e-15)
    edges = sorted((p, q) for p in range(4) for q in range(p + 1, 4))
    for e, (p, q) in enumerate(edges):
        c, d = [u for u in range(4) if u not in (p, q)]
        assert np.allclose(out[4 + e], 3 / 8 * (v[p] + v[q]) + 1 / 8 * (v[c] + v[d]), rtol=0, atol=1e-15)


@pytest.mark.parametrize('name', ['ico1', 'grid', 'odd'])
def test_midpoint_children_lie_in_their_parent(name):
    """float64: the four children of a face are coplanar with it and keep its normal direction (a quarter of its area each)."""
    x, f = R.inputs(name)
    v = x[0].astype(np.float64)
    out, faces = nr.subdivide(torch.tensor(v), torch.tensor(f), 1, 'midpoint')
    out, faces = out.numpy(), faces.numpy()
    normal = lambda p, t: np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    n_parent, n_child = normal(v, f), normal(out, faces)
    scale = np.abs(n_parent).max()
    assert np.abs(n_child - np.repeat(n_parent, 4, axis=0) / 4).max() <= 1e-13 * scale
    offset = ((out[faces[:, 0]] - np.repeat(v[f[:, 0]], 4, axis=0)) * np.repeat(n_parent, 4, axis=0)).sum(1)
    assert np.abs(offset).max() <= 1e-13 * scale


@pytest.mark.parametrize('levels', [0, 1, 2, 3])
@pytest.mark.parametrize('scheme', R.SCHEMES)
@pytest.mark.parametrize('name', R.MESHES)
def test_torch_implementation_against_the_restatement(name, scheme, levels):
    v, f = R.mesh(name)
    plan = nr.subdivision(torch.tensor(f), len(v), levels, scheme)
    for channels in (1, 3, 5):
        x, _ = R.inputs(name, channels)
        ref = R.reference(name, levels, scheme, channels)
        got, grad = apply_and_grad(plan, x, ref.g, implementation='torch')
        assert got.shape == ref.value.shape and got.dtype == np.float32
        check_against_restatement(got, grad, ref, what='%s %s L%d C%d' % (name, scheme, levels, channels))
        if levels == 0:
            assert np.array_equal(got, x)
    # without a batch axis
    x, _ = R.inputs(name, 3)
    ref = R.reference(name, levels, scheme, 3)
    got, grad = apply_and_grad(plan, x[1], ref.g[1], implementation='torch')
    assert got.shape == ref.value.shape[1:]
    check_against_restatement(got[None], grad[None], ref, images=slice(1, 2), what='%s %s L%d [Nv,C]' % (name, scheme, levels))


def test_other_dtypes_and_wide_data_take_the_torch_path():
    v, f = R.mesh('ico1')
    plan = nr.subdivision(torch.tensor(f), len(v), 1)
    x64 = torch.tensor(R.inputs('ico1')[0], dtype=torch.float64)
    ref = R.reference('ico1', 1, 'loop', 3)
    assert np.abs(plan(x64).numpy() - ref.value).max() <= 1e-6          # (float32 weights in float64 arithmetic)
    wide = torch.rand(42, 20)
    assert plan(wide).shape == (162, 20)
    with pytest.raises(ValueError, match='HIP kernel'):
        plan(wide, implementation='hip')


def test_subdivide_layouts_and_cache():
    x, f = R.inputs('ico1')
    faces = torch.tensor(f)
    out, new_faces = nr.subdivide(torch.tensor(x), faces, 1)
    assert out.shape == (3, 162, 3) and new_faces.shape == (320, 3) and new_faces.dtype == torch.int32
    batched = faces[None].expand(3, -1, -1)
    out_b, faces_b = nr.subdivide(torch.tensor(x), batched, 1)
    assert faces_b.shape == (3, 320, 3) and faces_b.stride(0) == 0 and torch.equal(faces_b[2], new_faces)
    assert torch.equal(out_b, out)
    # levels = 0 returns the inputs unchanged
    xt = torch.tensor(x)
    same, same_faces = nr.subdivide(xt, batched, 0)
    assert same is xt and same_faces is batched
    flat = xt[0]
    same, same_faces = nr.subdivide(flat, faces, 0)                 # ... also without a batch axis
    assert same is flat and same_faces is faces and nr.subdivision(faces, 42, 0)(flat) is flat
    # one plan per (index tensor, num_vertices, levels, scheme); an in-place edit of the indices builds a new one
    plan = nr.subdivision(faces, 42, 1)
    assert nr.subdivision(faces, 42, 1) is plan and nr.subdivision(faces, 42, 1, 'midpoint') is not plan
    assert nr.subdivision(faces, 42, 2) is not plan and nr.subdivision(faces, 43, 1) is not plan
    assert nr.subdivision(faces[None].expand(2, -1, -1), 42, 1).faces.shape == (320, 3)
    faces[0] = faces[0].flip(0)
    assert nr.subdivision(faces, 42, 1) is not plan


@pytest.mark.parametrize('level', [0, 1, 2, 3])
def test_icosphere(level):
    radius = 1.7
    v, f = nr.icosphere(level, radius)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.shape == (10 * 4 ** level + 2, 3) and f.shape == (20 * 4 ** level, 3)
    v64, f = v.numpy().astype(np.float64), f.numpy()
    assert np.abs(np.linalg.norm(v64, axis=1) / radius - 1).max() <= 2.0 ** -23
    want, want_f = vertex_ref.icosphere(level)
    key = lambda p: p[np.lexsort(np.round(p, 4).T[::-1])]
    assert np.abs(key(v64 / radius) - key(want)).max() <= 1e-6              # the same vertex SET (the numbering differs)
    if level == 0:
        assert np.array_equal(f, want_f) and np.abs(v64 / radius - want).max() <= 1e-6
    # every face points outward for the renderer's convention: the side vertex_ref's faces point to
    side = lambda p, t: np.sign((np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]) * p[t].mean(1)).sum(1))
    assert len(set(side(want, want_f).tolist())) == 1 and (side(v64, f) == side(want, want_f)[0]).all()
    assert len({tuple(sorted(t)) for t in f.tolist()}) == len(f)
    unit, _ = nr.icosphere(level)
    assert np.abs(np.linalg.norm(unit.numpy().astype(np.float64), axis=1) - 1).max() <= 2.0 ** -23


def test_argument_errors():
    v, f = R.mesh('ico1')
    x, faces = torch.tensor(R.inputs('ico1')[0]), torch.tensor(f)
    with pytest.raises(ValueError, match='levels'):
        nr.subdivision(faces, 42, -1)
    with pytest.raises(ValueError, match='levels'):
        nr.subdivide(x, faces, -2)
    with pytest.raises(ValueError, match='scheme'):
        nr.subdivision(faces, 42, 1, 'catmull-clark')
    with pytest.raises(ValueError, match='implementation'):
        nr.subdivide(x, faces, 1, 'loop', 'triton')
    with pytest.raises(ValueError, match='implementation'):
        nr.subdivision(faces, 42, 1)(x, implementation='cuda')
    with pytest.raises(ValueError, match='int32'):            # 80 * 4^13 faces
        nr.subdivision(faces, 42, 13)
    with pytest.raises(ValueError, match='int32'):
        nr.subdivision(faces, 2 ** 31, 1)
    with pytest.raises(ValueError, match='int32'):
        nr.icosphere(14)
    with pytest.raises(IndexError):
        nr.subdivision(torch.tensor(f), 41, 1)
    with pytest.raises(IndexError):
        nr.subdivide(x, torch.tensor(f) - 1, 1)
    odd = torch.tensor(R.M.mesh('odd')[1])                    # with its face (0, 3, 3): number 81
    with pytest.raises(ValueError, match=r'face 81 \(0, 3, 3\) repeats'):
        nr.subdivision(odd, 44, 1)
    two = torch.stack((faces, faces.flip(0)))
    with pytest.raises(ValueError, match='one topology per call'):
        nr.subdivision(two, 42, 1)
    for bad in (faces.float(), faces[:, :2], faces[0], f):    # dtype, shapes, not a tensor
        with pytest.raises(ValueError):
            nr.subdivision(bad, 42, 1)
    plan = nr.subdivision(faces, 42, 1)
    for bad in (x[:, :41], x.long(), x[None], x.numpy()):
        with pytest.raises(ValueError):
            plan(bad)
    with pytest.raises(ValueError):
        nr.subdivide(x[:2], faces[None].expand(3, -1, -1), 1)
    # the HIP kernel takes float32 CUDA tensors only
    for bad in (x, x.double()):
        with pytest.raises(ValueError, match='HIP kernel'):
            plan(bad, implementation='hip')


def test_abi_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    NULL, SIZE = -1, -2
    ok = (1, 1, 1, 1, 1)      # pointers (never dereferenced: no launch happens)
    assert lib.nr_stencil_apply(*ok, 1, 4, 10, 17, 24, None) == SIZE          # channels
    assert lib.nr_stencil_apply(*ok, 1, 4, 10, 0, 24, None) == SIZE
    assert lib.nr_stencil_apply(*ok, 65536, 4, 10, 3, 24, None) == SIZE       # batch size
    for sizes in ((0, 4, 10, 3, 24), (1, 0, 10, 3, 24), (1, 4, 0, 3, 24), (1, 4, 10, 3, 0), (1, 4, -1, 3, 24),
                  (1, 2 ** 31 - 1, 10, 3, 24), (1, 4, 2 ** 30, 16, 24)):
        assert lib.nr_stencil_apply(*ok, *sizes, None) == SIZE, sizes
    for k in range(5):
        ptrs = [1] * 5
        ptrs[k] = None
        assert lib.nr_stencil_apply(*ptrs, 1, 4, 10, 3, 24, None) == NULL


def test_mesh_subdivide(tmp_path):
    v, f = R.mesh('ico1')
    path = tmp_path / 'ico.obj'
    with open(str(path), 'w') as fh:
        for p in v:
            fh.write('v %r %r %r\n' % tuple(float(c) for c in p))
        for t in f:
            fh.write('f %d %d %d\n' % tuple(int(i) + 1 for i in t))
    mesh = nr.Mesh(str(path), texture_size=2, normalization=False)
    mesh.set_lr(0.5, 2.0)
    old_v, old_t = mesh.vertices.detach().clone(), mesh.textures.detach().clone()
    plan = mesh.subdivide()
    assert isinstance(mesh.vertices, torch.nn.Parameter) and isinstance(mesh.textures, torch.nn.Parameter)
    assert mesh.vertices.shape == (162, 3) and mesh.faces.shape == (320, 3) and mesh.textures.shape == (320, 2, 2, 2, 3)
    assert (mesh.num_vertices, mesh.num_faces) == (162, 320) and mesh.faces.dtype == torch.int32
    assert torch.equal(mesh.textures.detach(), old_t[plan.face_parent]) and torch.equal(plan.face_parent, torch.arange(320) // 4)
    assert torch.equal(mesh.vertices.detach(), plan(old_v)) and torch.equal(mesh.faces, plan.faces)
    assert mesh.vertices.lr == 0.5 and mesh.textures.lr == 2.0
    assert set(dict(mesh.named_parameters())) == {'vertices', 'textures'} and 'faces' in dict(mesh.named_buffers())
    assert 'new optimiser' in nr.Mesh.subdivide.__doc__ and 'not resampled' in nr.Mesh.subdivide.__doc__
    lap = mesh.laplacian_loss()
    lap.backward()
    assert bool(torch.isfinite(lap)) and mesh.vertices.grad.shape == (162, 3)
    vb, fb, tb = mesh.get_batch(2)
    assert vb.shape == (2, 162, 3) and fb.shape == (2, 320, 3) and tb.shape == (2, 320, 2, 2, 2, 3)
    mesh.subdivide(2, 'midpoint')
    assert (mesh.num_vertices, mesh.num_faces) == (2562, 5120) and mesh.textures.shape[0] == 5120
    assert mesh.subdivide(0).levels == 0 and mesh.num_faces == 5120
