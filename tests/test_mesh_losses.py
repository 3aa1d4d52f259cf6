"""Mesh losses without a GPU (neural_renderer_amd/mesh_losses.py): the host tables against a set-and-dict construction, their
cache, the plain-torch paths against the float64 restatement of tests/mesh_loss_ref.py, the restatement itself against
finite differences, the flat and the quad-less limits, argument errors and the C ABI's error codes."""
import numpy as np
import pytest
import torch

import mesh_loss_ref as R
from neural_renderer_amd import mesh_losses as ML

# The four constants C of the checks |got - ref| <= C u M (tests/mesh_loss_ref.py): 4 x the worst ratio the float32 torch
# path shows against the float64 restatement over R.all_cases() -- the five meshes, the odd topology and the multi-block
# mesh (six seeds of each noisy one) and the degenerate mesh --, rounded up to a power of two.  The float32 torch path must
# stay within C / 4 (test_float32_torch_paths_stay_within_a_quarter); the factor 4 is for a kernel that orders the same
# operations differently.
#                  measured worst float32 ratio
C_LAP_GRAD = 8     # 1.078  (odd topology, seed 2)
C_FLAT_GRAD = 4    # 0.546  (the tetrahedron; the noisy meshes stay below 0.21)
C_LAP_LOSS = 2     # 0.379  (the tetrahedron)
C_FLAT_LOSS = 16   # 3.801  (the degenerate mesh: a vertex on the line of its opposite edge leaves c = b - t a as rounding noise,
#                            which 1 / sqrt(eps) = 1000 amplifies into cos, and the loss's magnitude sum (|cos| + 1)^2 does not
#                            know of it; without that mesh the worst is 0.923, the tetrahedron, and below 0.05 on the noisy meshes)
CONSTANTS = {('laplacian', 'loss'): C_LAP_LOSS, ('laplacian', 'grad'): C_LAP_GRAD,
             ('flatness', 'loss'): C_FLAT_LOSS, ('flatness', 'grad'): C_FLAT_GRAD}
TORCH_FN = {'laplacian': ML.laplacian_loss_torch, 'flatness': ML.flatness_loss_torch}


def loss_and_grad(fn, vertices, faces, dtype, device='cpu', **kw):
    """(loss [B], grad [B,Nv,3]) as numpy for the upstream R.UPSTREAM"""
    x = torch.tensor(vertices, dtype=dtype, device=device, requires_grad=True)
    loss = fn(x, torch.tensor(faces, device=device), **kw)
    g = torch.tensor(R.UPSTREAM[:x.shape[0]], dtype=dtype, device=device)
    grad, = torch.autograd.grad((loss * g).sum(), x)
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


def ratios(kind, name, seed, loss, grad):
    ref = R.reference(kind, name, seed)
    return R.worst_ratio(loss, ref.loss, ref.loss_mag), R.worst_ratio(grad, ref.grad, ref.grad_mag)


# ---------------------------------------------------------------------------------------------------------------------
# tables

@pytest.mark.parametrize('name', R.MESHES + R.ODD + R.DEGENERATE)
def test_tables_match_the_set_and_dict_construction(name):
    v, f = R.inputs(name)
    Nv = v.shape[1]
    nbrs, quads, inc = R.tables(f, Nv)
    if name in R.EXPECTED:
        assert (Nv, len(f), len(quads)) == R.EXPECTED[name]
    nbr_offsets, nbr, q, inc_offsets, ient = ML.build_tables(f, Nv)
    for a in (nbr_offsets, nbr, q, inc_offsets, ient):
        assert a.dtype == np.int32
    off, ent = R.csr(nbrs)
    assert np.array_equal(nbr_offsets, off) and np.array_equal(nbr, ent)
    assert q.shape == (len(quads), 4) and np.array_equal(q, np.asarray(quads, np.int32).reshape(-1, 4))
    off, ent = R.csr(inc)
    assert np.array_equal(inc_offsets, off) and np.array_equal(ient, ent)


def test_odd_topology_is_what_it_says():
    v, f = R.inputs('odd')
    nbrs, quads, _ = R.tables(f, v.shape[1])
    n0 = 42
    assert nbrs[n0] == [] and 3 in nbrs[0] and 0 in nbrs[3]         # the isolated vertex; the face (0, 3, 3)
    edges = {(q[0], q[1]) for q in quads}
    assert (0, 3) not in edges                                       # ... which makes no quad
    a, b, c = (int(i) for i in f[7])                                 # the duplicated face: its edges lie in three faces
    for p, q in ((a, b), (b, c), (c, a)):
        assert (min(p, q), max(p, q)) not in edges
    assert (min(f[5, 0], f[5, 1]), max(f[5, 0], f[5, 1])) not in edges   # the edge with a third face
    assert len(quads) == 120 - 4


def test_table_cache():
    _, f = R.inputs('ico1')
    faces = torch.tensor(f)
    t = ML._tables(faces, 42)
    assert ML._tables(faces, 42) is t                                 # a second call
    assert ML._tables(faces, 43) is not t                             # another vertex count
    view = ML._tables(faces[None], 42)
    assert ML._tables(faces[None], 42) is view                        # a view built anew: found on the tensor it views
    exp = ML._tables(faces[None].expand(3, -1, -1), 42)
    assert ML._tables(faces[None].expand(3, -1, -1), 42) is exp       # .expand
    for other in (view, exp):
        assert torch.equal(other.quads, t.quads) and torch.equal(other.nbr, t.nbr) and torch.equal(other.inc, t.inc)
    faces[0, 0] = faces[0, 0]                                         # an in-place edit: the version counter moves
    assert ML._tables(faces, 42) is not t
    assert ML._tables(faces[None].expand(3, -1, -1), 42) is not exp


def _adjacency_tensors(hit):
    return hit[:3]


def _plan_tensors(plan):
    return [plan.faces] + [t for level in plan._levels for t in (level.forward.offsets, level.forward.cols, level.forward.weights)]


@pytest.mark.parametrize('which', ['adjacency', 'subdivision'])
def test_table_cache_of_the_other_index_tables(which):
    """test_table_cache's assertions on the other users of _util.cached_on_index"""
    import neural_renderer_amd as nr
    from neural_renderer_amd import vertex_colors as VC
    get, tensors = {'adjacency': (VC._adjacency, _adjacency_tensors), 'subdivision': (nr.subdivision, _plan_tensors)}[which]
    _, f = R.inputs('ico1')
    faces = torch.tensor(f)
    t = get(faces, 42)
    assert get(faces, 42) is t                                        # a second call
    assert get(faces, 43) is not t                                    # another vertex count
    view = get(faces[None], 42)
    assert get(faces[None], 42) is view                               # a view built anew: found on the tensor it views
    exp = get(faces[None].expand(3, -1, -1), 42)
    assert get(faces[None].expand(3, -1, -1), 42) is exp              # .expand
    for other in (view, exp):
        assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(tensors(other), tensors(t)))
    if which == 'subdivision':
        assert get(faces, 42, levels=2) is not t and get(faces, 42, scheme='midpoint') is not t   # the rest of its key
    faces[0, 0] = faces[0, 0]                                         # an in-place edit: the version counter moves
    assert get(faces, 42) is not t
    assert get(faces[None].expand(3, -1, -1), 42) is not exp


# ---------------------------------------------------------------------------------------------------------------------
# the torch paths against the restatement

@pytest.mark.parametrize('kind', ['laplacian', 'flatness'])
def test_float64_torch_paths_equal_the_restatement(kind):
    for name in R.MESHES + R.ODD:
        v, f = R.inputs(name)
        ref = R.reference(kind, name, 0)
        loss, grad = loss_and_grad(TORCH_FN[kind], v, f, torch.float64)
        assert np.abs(loss - ref.loss).max() <= 1e-12 * np.abs(ref.loss).max(), name
        assert np.abs(grad - ref.grad).max() <= 1e-12 * np.abs(ref.grad).max(), name


@pytest.mark.parametrize('kind', ['laplacian', 'flatness'])
def test_float32_torch_paths_stay_within_a_quarter(kind):
    worst = [0.0, 0.0]
    for name, seed in R.all_cases():
        v, f = R.inputs(name, seed)
        rl, rg = ratios(kind, name, seed, *loss_and_grad(TORCH_FN[kind], v, f, torch.float32))
        worst = [max(worst[0], rl), max(worst[1], rg)]
    print('%s, float32 torch path: worst ratio loss %.3f, gradient %.3f' % (kind, worst[0], worst[1]))
    assert worst[0] <= CONSTANTS[kind, 'loss'] / 4 and worst[1] <= CONSTANTS[kind, 'grad'] / 4


def test_restatement_against_finite_differences():
    """Central differences of the float64 restatement on the tetrahedron (step 1e-6: truncation ~ h^2 |f'''|, rounding ~
    1e-16 |f| / h, both below 1e-8 of the largest entry here) against its autograd."""
    v, f = R.inputs('tetra')
    x = v.astype(np.float64)
    nbrs, quads, _ = R.tables(f, 4)
    values = {'laplacian': lambda t: R.laplacian_value(t, nbrs)[0], 'flatness': lambda t: R.flatness_value(t, quads)}
    h = 1e-6
    for kind, value in values.items():
        ref = R.reference(kind, 'tetra', 0)
        fd = np.zeros_like(x)
        for b in range(x.shape[0]):
            for i in range(4):
                for c in range(3):
                    xp, xm = x.copy(), x.copy()
                    xp[b, i, c] += h
                    xm[b, i, c] -= h
                    d = (value(torch.tensor(xp)) - value(torch.tensor(xm))).numpy() / (2 * h)
                    fd[b, i, c] = (d * R.UPSTREAM).sum()
        assert np.abs(fd - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max(), kind
        assert np.abs(ref.grad).max() > 0.1    # (an irregular tetrahedron: the regular one is a stationary point)


def test_flat_grid_and_no_quads():
    v, f = R.inputs('grid_flat')
    for dtype in (torch.float32, torch.float64):
        loss, grad = loss_and_grad(ML.flatness_loss_torch, v, f, dtype)
        assert (loss >= 0).all() and (loss <= 176 * 4e-6).all()
    # a single triangle and an open fan's boundary: no edge lies in two faces
    tri = torch.tensor([[0, 1, 2]])
    x = torch.tensor(v[:, :3].copy(), requires_grad=True)
    loss = ML.flatness_loss(x, tri)
    assert loss.shape == (3,) and not loss.any()
    grad, = torch.autograd.grad(loss.sum(), x)
    assert grad.shape == x.shape and not grad.any()
    assert ML.build_tables(tri.numpy(), 3)[2].shape == (0, 4)
    ref = R.flatness_ref(v[:, :3], tri.numpy())
    assert not ref.loss.any() and not ref.grad.any()


def test_shapes_and_mesh_methods(tmp_path):
    import neural_renderer_amd as nr
    import neural_renderer
    assert nr.laplacian_loss is ML.laplacian_loss and nr.flatness_loss is ML.flatness_loss
    assert neural_renderer.laplacian_loss is ML.laplacian_loss and neural_renderer.flatness_loss is ML.flatness_loss
    assert 'laplacian_loss' in nr.__all__ and 'flatness_loss' in nr.__all__
    v, f = R.inputs('ico1')
    faces = torch.tensor(f)
    for fn in (nr.laplacian_loss, nr.flatness_loss):
        batch = fn(torch.tensor(v), faces)
        single = fn(torch.tensor(v[1]), faces)
        assert batch.shape == (3,) and single.dim() == 0
        assert torch.equal(fn(torch.tensor(v[1:2]), faces)[0], single)
        assert torch.equal(fn(torch.tensor(v), faces[None].expand(3, -1, -1)), batch)     # [B,Nf,3] with equal images
        assert torch.equal(fn(torch.tensor(v), faces, implementation='torch'), batch)
    path = tmp_path / 'ico.obj'
    with open(str(path), 'w') as fh:
        for p in v[0]:
            fh.write('v %r %r %r\n' % tuple(float(c) for c in p))
        for t in f:
            fh.write('f %d %d %d\n' % tuple(int(i) + 1 for i in t))
    mesh = nr.Mesh(str(path), normalization=False)
    lap, flat = mesh.laplacian_loss(), mesh.flatness_loss()
    assert lap.dim() == 0 and flat.dim() == 0 and lap.requires_grad and flat.requires_grad
    assert torch.equal(lap.detach(), nr.laplacian_loss(mesh.vertices.detach(), mesh.faces))
    assert torch.equal(flat.detach(), nr.flatness_loss(mesh.vertices.detach(), mesh.faces, eps=1e-6))
    (lap + flat).backward()
    assert mesh.vertices.grad is not None and mesh.vertices.grad.abs().sum() > 0


def test_argument_errors():
    v, f = R.inputs('ico1')
    x, faces = torch.tensor(v), torch.tensor(f)
    for fn in (ML.laplacian_loss, ML.flatness_loss, ML.laplacian_loss_torch, ML.flatness_loss_torch):
        for bad in (x[..., :2], x[None], x.long(), v):                       # shapes, dtype, not a tensor
            with pytest.raises(ValueError):
                fn(bad, faces)
        for bad in (faces[:, :2], faces.float(), faces[None].expand(2, -1, -1), f):   # ... of the faces; another batch size
            with pytest.raises(ValueError):
                fn(x, bad)
        other = torch.stack((faces, faces, faces.flip(0)))                   # differing topologies
        with pytest.raises(ValueError):
            fn(x, other)
        with pytest.raises(IndexError):
            fn(x, faces + 1)
        with pytest.raises(IndexError):
            fn(x, faces - 1)
        with pytest.raises(ValueError):
            fn(x.to('meta'), faces)                                          # two devices
    for fn in (ML.laplacian_loss, ML.flatness_loss):
        with pytest.raises(ValueError):
            fn(x, faces, implementation='cuda')
        with pytest.raises(ValueError):
            fn(x, faces, implementation='hip')                               # CPU tensors do not fit the kernels
        with pytest.raises(ValueError):
            fn(x.double(), faces, implementation='hip')


def test_new_entry_points_return_error_codes_without_a_gpu():
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    # host only
    assert lib.nr_mesh_loss_workspace_bytes(3, 648) == 3 * 3 * 8
    assert lib.nr_mesh_loss_workspace_bytes(64, 10242) == 64 * 41 * 8
    assert lib.nr_mesh_loss_workspace_bytes(2, 0) == 2 * 8           # no quads: one (unused) slot per image
    assert lib.nr_mesh_loss_workspace_bytes(0, 10) == 0 and lib.nr_mesh_loss_workspace_bytes(65536, 10) == 0
    assert lib.nr_mesh_loss_workspace_bytes(1, -1) == 0
    # NULL pointers (NR_E_NULL = -1), sizes (-2), workspace (-3): all before any launch
    assert lib.nr_laplacian_forward(None, None, None, None, None, 1, 4, 12, None, 0, None) == -1
    assert lib.nr_laplacian_forward(1, 1, None, None, 1, 1, 4, 12, 1, 64, None) == -1      # neighbours announced, no list
    assert lib.nr_laplacian_forward(1, 1, 1, None, 1, 0, 4, 12, 1, 64, None) == -2
    assert lib.nr_laplacian_forward(1, 1, 1, None, 1, 65536, 4, 12, 1, 1 << 30, None) == -2
    assert lib.nr_laplacian_forward(1, 1, 1, None, 1, 1, 0, 12, 1, 64, None) == -2
    assert lib.nr_laplacian_forward(1, 1, 1, None, 1, 1, 4, -1, 1, 64, None) == -2
    assert lib.nr_laplacian_forward(1, 1, 1, None, 1, 2, 300, 12, None, 0, None) == -3
    assert lib.nr_laplacian_forward(1, 1, 1, None, 1, 2, 300, 12, 1, 2 * 2 * 8 - 1, None) == -3
    assert lib.nr_laplacian_backward(None, None, None, None, None, 1, 4, 12, None) == -1
    assert lib.nr_laplacian_backward(1, 1, 1, 1, None, 1, 4, 12, None) == -1
    assert lib.nr_laplacian_backward(1, 1, 1, 1, 1, 1, 0, 12, None) == -2
    assert lib.nr_flatness_forward(None, None, None, 1, 4, 6, 1e-6, None, 0, None) == -1
    assert lib.nr_flatness_forward(1, None, 1, 1, 4, 6, 1e-6, 1, 64, None) == -1            # quads announced, no list
    assert lib.nr_flatness_forward(1, 1, 1, 1, 4, -1, 1e-6, 1, 64, None) == -2
    assert lib.nr_flatness_forward(1, 1, 1, 0, 4, 6, 1e-6, 1, 64, None) == -2
    assert lib.nr_flatness_forward(1, 1, 1, 1, 4, 6, 1e-6, None, 0, None) == -3
    assert lib.nr_flatness_forward(1, None, 1, 1, 4, 0, 1e-6, None, 0, None) == -3          # no quads: still a workspace
    assert lib.nr_flatness_backward(None, None, None, None, None, None, 1, 4, 6, 1e-6, None) == -1
    assert lib.nr_flatness_backward(1, 1, 1, None, 1, 1, 1, 4, 6, 1e-6, None) == -1
    assert lib.nr_flatness_backward(1, 1, 1, 1, 1, None, 1, 4, 6, 1e-6, None) == -1
    assert lib.nr_flatness_backward(1, 1, 1, 1, 1, 1, 1, 0, 6, 1e-6, None) == -2
