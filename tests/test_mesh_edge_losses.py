"""The edge-length and the cotangent Laplacian loss without a GPU (neural_renderer_amd/mesh_losses.py): the host tables against
a set-and-dict construction, their cache, the plain-torch paths against the float64 restatement of tests/mesh_edge_ref.py, the
restatement itself against finite differences, the exact cases, shapes, argument errors and the C ABI's error codes."""
import numpy as np
import pytest
import torch

import mesh_edge_ref as E
import mesh_loss_ref as R
from neural_renderer_amd import mesh_losses as ML

# The constants C of the checks |got - ref| <= C u M (tests/mesh_edge_ref.py), one per (loss, output): 4 x the worst ratio the
# float32 torch path shows on the CPU against the float64 restatement over R.all_cases() -- the five meshes, the odd topology
# and the multi-block mesh (six seeds of each noisy one) and the degenerate mesh; the edge loss with every target form of
# E.TARGETS --, rounded up to a power of two.  The float32 torch path must stay within C / 4
# (test_float32_torch_paths_stay_within_a_quarter); the factor 4 is for a kernel that does the same operations in another order.
#                      measured worst float32 ratio
C_EDGE_LOSS = 4        # 0.860  (ico1, target 0; 0.367 on the degenerate mesh)
C_EDGE_GRAD = 16       # 2.432  (the multi-block mesh, seed 5, target 0; 2.244 on the degenerate mesh)
C_COT_LOSS = 2 ** 18   # 36050.7  (the degenerate mesh ALONE: without it 0.457, grid_flat -- see C_COT_LOSS_REGULAR)
C_COT_GRAD = 2 ** 14   # 2068.99  (the degenerate mesh ALONE: without it 1.290, the grid, seed 4 -- see C_COT_GRAD_REGULAR)
# The degenerate mesh has a face whose third vertex lies on the line of the opposite edge up to the rounding of its float32
# coordinates: |a x b|^2 ~ 1e-15 is itself rounding noise of the cross product's cancelling differences, next to eps = 1e-12,
# so the float32 square root's argument is off by ~1e-4 of itself, and the cotangent's magnitude |a| |b| / sqrt(|a x b|^2 + eps)
# knows of the dot product's cancellation, not of the cross product's.  Every other mesh is held to the constants without it:
C_COT_LOSS_REGULAR = 2
C_COT_GRAD_REGULAR = 8
CONSTANTS = {('edge', 'loss'): C_EDGE_LOSS, ('edge', 'grad'): C_EDGE_GRAD, ('cot', 'loss'): C_COT_LOSS, ('cot', 'grad'): C_COT_GRAD}
REGULAR = dict(CONSTANTS)
REGULAR.update({('cot', 'loss'): C_COT_LOSS_REGULAR, ('cot', 'grad'): C_COT_GRAD_REGULAR})


def constants(name):
    """the constants that hold for the mesh `name`"""
    return CONSTANTS if name in R.DEGENERATE else REGULAR


def forms_of(kind):
    return E.TARGETS if kind == 'edge' else ('zero',)


def call(fn, kind, x, faces, name, seed, form, **kw):
    """fn(x, faces, [target of `form` on x's device and in its dtype]) for inputs(name, seed)"""
    if kind == 'cot':
        return fn(x, faces, **kw)
    t = E.target(name, seed, form)
    if isinstance(t, np.ndarray):
        t = torch.tensor(t, dtype=x.dtype, device=x.device)
    return fn(x, faces, target=t, **kw)


def loss_and_grad(fn, kind, name, seed, form, dtype, device='cpu', **kw):
    """(loss [B], grad [B,Nv,3]) as numpy for the upstream R.UPSTREAM"""
    v, f = R.inputs(name, seed)
    x = torch.tensor(v, dtype=dtype, device=device, requires_grad=True)
    loss = call(fn, kind, x, torch.tensor(f, device=device), name, seed, form, **kw)
    g = torch.tensor(R.UPSTREAM[:x.shape[0]], dtype=dtype, device=device)
    grad, = torch.autograd.grad((loss * g).sum(), x)
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


def ratios(kind, name, seed, form, loss, grad):
    ref = E.reference(kind, name, seed, form)
    return R.worst_ratio(loss, ref.loss, ref.loss_mag), R.worst_ratio(grad, ref.grad, ref.grad_mag)


TORCH_FN = {'edge': ML.edge_length_loss_torch, 'cot': ML.cotangent_laplacian_loss_torch}


# ---------------------------------------------------------------------------------------------------------------------
# tables

@pytest.mark.parametrize('name', R.MESHES + R.ODD + R.DEGENERATE)
def test_edge_tables_match_the_set_and_dict_construction(name):
    v, f = R.inputs(name)
    Nv = v.shape[1]
    edges, nbr_edge = E.edge_tables(f, Nv)
    nbr_offsets, nbr = ML.build_tables(f, Nv)[:2]
    got_edges, got_nbr_edge = ML.build_edge_tables(nbr_offsets, nbr)
    assert got_edges.dtype == np.int32 and got_nbr_edge.dtype == np.int32
    assert got_edges.shape == (len(edges), 2) and np.array_equal(got_edges, np.asarray(edges, np.int32).reshape(-1, 2))
    assert np.array_equal(got_nbr_edge, R.csr(nbr_edge)[1]) and got_nbr_edge.shape == nbr.shape
    # every entry of nbr names the edge of its own two ends
    owner = np.repeat(np.arange(Nv), np.diff(nbr_offsets))
    assert np.array_equal(np.sort(np.stack((owner, nbr), 1), axis=1), got_edges[got_nbr_edge])
    public = ML.mesh_edges(torch.tensor(f), Nv)
    assert public.dtype == torch.int64 and np.array_equal(public.numpy(), got_edges)
    if name in R.EXPECTED:   # a closed or open manifold: E = V + F - chi, and the listed quads are its interior edges
        nv, nf, quads = R.EXPECTED[name]
        boundary = {'grid': 32, 'grid_flat': 32}.get(name, 0)
        assert len(edges) == quads + boundary == nv + nf - (1 if boundary else 2)


def test_odd_topology_edges():
    """the duplicated face, the edge in three faces and the repeated index each count once / add nothing but the pair (0, 3)"""
    v, f = R.inputs('odd')
    edges = [tuple(e) for e in ML.mesh_edges(torch.tensor(f), v.shape[1]).tolist()]
    plain = [tuple(e) for e in ML.mesh_edges(torch.tensor(R.inputs('ico1')[1]), 42).tolist()]
    a, b = int(f[5, 0]), int(f[5, 1])
    extra = {(0, 3), (min(a, 43), max(a, 43)), (min(b, 43), max(b, 43))}
    assert len(edges) == len(set(edges)) and set(edges) == set(plain) | extra and len(edges) == 120 + 3
    assert not any(42 in e for e in edges)                               # the isolated vertex
    assert ML.mesh_edges(torch.tensor([[0, 1, 2]]), 3).tolist() == [[0, 1], [0, 2], [1, 2]]      # a single triangle: E = 3
    assert ML.mesh_edges(torch.tensor([[1, 1, 1]]), 3).shape == (0, 2)


def test_edge_table_cache():
    """tests/test_mesh_losses.py test_table_cache's assertions on the edge tables"""
    _, f = R.inputs('ico1')
    faces = torch.tensor(f)
    t = ML._edge_tables(faces, 42)
    assert ML._edge_tables(faces, 42) is t                                 # a second call
    assert t.mesh is ML._tables(faces, 42)                                  # built from the cached neighbour tables
    assert ML._edge_tables(faces, 43) is not t                             # another vertex count
    view = ML._edge_tables(faces[None], 42)
    assert ML._edge_tables(faces[None], 42) is view                        # a view built anew: found on the tensor it views
    exp = ML._edge_tables(faces[None].expand(3, -1, -1), 42)
    assert ML._edge_tables(faces[None].expand(3, -1, -1), 42) is exp       # .expand
    for other in (view, exp):
        assert torch.equal(other.edges, t.edges) and torch.equal(other.nbr_edge, t.nbr_edge)
    faces[0, 0] = faces[0, 0]                                              # an in-place edit: the version counter moves
    assert ML._edge_tables(faces, 42) is not t
    assert ML._edge_tables(faces[None].expand(3, -1, -1), 42) is not exp


def test_corner_entries_match_the_adjacency_table():
    """the restatement's (face, corner) lists against the table the kernels gather through"""
    from neural_renderer_amd import vertex_colors as VC
    for name in R.MESHES + R.ODD:
        v, f = R.inputs(name)
        off, ent = VC.build_adjacency(f[None], v.shape[1])
        want_off, want_ent = R.csr(E.corner_entries(f, v.shape[1]))
        assert np.array_equal(off[0], want_off) and np.array_equal(ent[0], want_ent)


# ---------------------------------------------------------------------------------------------------------------------
# the torch paths against the restatement

@pytest.mark.parametrize('kind', E.KINDS)
def test_float64_torch_paths_equal_the_restatement(kind):
    for name in R.MESHES + R.ODD + R.DEGENERATE:
        for form in forms_of(kind):
            ref = E.reference(kind, name, 0, form)
            loss, grad = loss_and_grad(TORCH_FN[kind], kind, name, 0, form, torch.float64)
            assert np.abs(loss - ref.loss).max() <= 1e-12 * np.abs(ref.loss).max(), (name, form)
            assert np.abs(grad - ref.grad).max() <= 1e-12 * np.abs(ref.grad).max(), (name, form)
            assert np.isfinite(ref.loss).all() and np.isfinite(ref.grad).all()


@pytest.mark.parametrize('kind', E.KINDS)
def test_float32_torch_paths_stay_within_a_quarter(kind):
    worst = {True: [0.0, 0.0], False: [0.0, 0.0]}
    for name, seed in R.all_cases():
        for form in forms_of(kind):
            rl, rg = ratios(kind, name, seed, form, *loss_and_grad(TORCH_FN[kind], kind, name, seed, form, torch.float32))
            w = worst[name in R.DEGENERATE]
            w[0], w[1] = max(w[0], rl), max(w[1], rg)
            assert rl <= constants(name)[kind, 'loss'] / 4 and rg <= constants(name)[kind, 'grad'] / 4, (name, seed, form, rl, rg)
    print('%s, float32 torch path: worst ratio loss %.3f, gradient %.3f; on the degenerate mesh %.3f, %.3f'
          % (kind, worst[False][0], worst[False][1], worst[True][0], worst[True][1]))


def test_restatement_against_finite_differences():
    """Central differences of the float64 restatement on the tetrahedron (step 1e-6, as in tests/test_mesh_losses.py) against
    its autograd.  The cotangent weights are held at their unperturbed values: that is the definition."""
    v, f = R.inputs('tetra')
    x = v.astype(np.float64)
    edges, _ = E.edge_tables(f, 4)
    entries = E.corner_entries(f, 4)
    w = E.cot_terms(torch.tensor(x), f)[0]
    number = E.target('tetra', 0, 'number')
    assert number > 0.5
    values = {('edge', 'zero'): lambda t: E.edge_value(t, edges, 0.0)[0],
              ('edge', 'number'): lambda t: E.edge_value(t, edges, number)[0],
              ('edge', 'BE'): lambda t: E.edge_value(t, edges, E.target('tetra', 0, 'BE'))[0],
              ('cot', 'zero'): lambda t: E.cot_value(t, w, f, entries)[0]}
    h = 1e-6
    for (kind, form), value in values.items():
        ref = E.reference(kind, 'tetra', 0, form)
        fd = np.zeros_like(x)
        for b in range(x.shape[0]):
            for i in range(4):
                for c in range(3):
                    xp, xm = x.copy(), x.copy()
                    xp[b, i, c] += h
                    xm[b, i, c] -= h
                    d = (value(torch.tensor(xp)) - value(torch.tensor(xm))).numpy() / (2 * h)
                    fd[b, i, c] = (d * R.UPSTREAM).sum()
        assert np.abs(fd - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max(), (kind, form)
        assert np.abs(ref.grad).max() > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# exact cases

def test_rest_lengths_give_exactly_zero():
    v, f = R.inputs('ico2', 1)
    faces = torch.tensor(f)
    for x in (torch.tensor(v, requires_grad=True), torch.tensor(v[1], requires_grad=True)):
        rest = ML.edge_lengths(x.detach(), faces)
        assert rest.shape == x.shape[:-2] + (480,) and not rest.requires_grad
        loss = ML.edge_length_loss(x, faces, target=rest)
        grad, = torch.autograd.grad(loss.sum(), x)
        assert not loss.any() and not grad.any()
    lengths = ML.edge_lengths(torch.tensor(v, requires_grad=True), faces)
    assert lengths.requires_grad                                          # differentiable by autograd
    e = ML.mesh_edges(faces, 162)
    want = (torch.tensor(v)[:, e[:, 1]] - torch.tensor(v)[:, e[:, 0]]).norm(dim=2)
    assert torch.allclose(lengths.detach(), want, rtol=1e-6, atol=0)


def test_zero_length_edge_has_a_finite_loss_and_no_gradient():
    """one triangle with two coincident vertices and a positive target: the zero-length edge adds t^2 and exactly nothing to
    the gradient -- what is left is the gradient of the other two edges"""
    faces = torch.tensor([[0, 1, 2]])
    for dtype in (torch.float32, torch.float64):
        x = torch.tensor([[0.5, 0.25, 0.0], [0.5, 0.25, 0.0], [1.5, 0.25, 0.0]], dtype=dtype, requires_grad=True)
        target = torch.tensor([0.75, 1.0, 1.0], dtype=dtype)             # edges (0,1), (0,2), (1,2): the other two at rest
        loss = ML.edge_length_loss(x, faces, target=target)
        grad, = torch.autograd.grad(loss, x)
        assert float(loss.detach()) == 0.75 ** 2 and not grad.any()
        loss = ML.edge_length_loss(x, faces, target=0.75)
        grad, = torch.autograd.grad(loss, x)
        assert float(loss.detach()) == 0.75 ** 2 + 2 * 0.25 ** 2
        assert torch.equal(grad, torch.tensor([[-0.5, 0, 0], [-0.5, 0, 0], [1.0, 0, 0]], dtype=dtype))
    v, f = R.inputs('degenerate')
    ref = E.reference('edge', 'degenerate', 0, 'BE')
    assert np.isfinite(ref.loss).all() and np.isfinite(ref.grad).all()


def test_flat_grid_has_no_curvature():
    """On the flat regular grid H = 0 at the interior vertices up to rounding (grid_flat against its M); the z components,
    whose M is 0, exactly."""
    v, f = R.inputs('grid_flat')
    x64 = torch.tensor(v.astype(np.float64))
    entries = E.corner_entries(f, 81)
    H = E.cot_apply(x64, E.cot_terms(x64, f)[0], f, entries).numpy().reshape(3, 9, 9, 3)
    assert np.abs(H[:, 1:-1, 1:-1]).max() <= 1e-12 and np.abs(H).max() > 0.1      # (the boundary is not flat: it has an edge)
    for dtype in (torch.float32, torch.float64):
        loss, grad = loss_and_grad(TORCH_FN['cot'], 'cot', 'grid_flat', 0, 'zero', dtype)
        rl, rg = ratios('cot', 'grid_flat', 0, 'zero', loss, grad)
        assert rl <= C_COT_LOSS_REGULAR / 4 and rg <= C_COT_GRAD_REGULAR / 4
        assert not grad[:, :, 2].any()


def test_single_triangle_and_repeated_index():
    x = torch.tensor(R.inputs('ico1')[0][:, :4].copy(), requires_grad=True)
    tri = torch.tensor([[0, 1, 2]])
    for fn in (ML.edge_length_loss, ML.cotangent_laplacian_loss):
        one = fn(x, tri)
        grad, = torch.autograd.grad(one.sum(), x)
        assert one.shape == (3,) and (one > 0).all() and grad[:, :3].abs().sum() > 0 and not grad[:, 3].any()
        # a face with a repeated index contributes nothing to the cotangent loss, and only its pair to the edges
        both = fn(x, torch.tensor([[0, 1, 2], [3, 3, 3]]))
        assert torch.equal(both, one)
    assert torch.equal(ML.cotangent_laplacian_loss(x, torch.tensor([[0, 1, 2], [0, 3, 3]])), ML.cotangent_laplacian_loss(x, tri))
    with_pair = ML.edge_length_loss(x, torch.tensor([[0, 1, 2], [0, 3, 3]]))
    d = (x[:, 3] - x[:, 0]).detach()
    assert torch.allclose(with_pair, ML.edge_length_loss(x, tri) + (d * d).sum(1), rtol=1e-6, atol=0)
    # a duplicated face counts twice in the cotangent operator (H doubles: four times the loss), once in the edges
    twice = torch.tensor([[0, 1, 2], [0, 1, 2]])
    assert torch.allclose(ML.cotangent_laplacian_loss(x, twice), 4 * ML.cotangent_laplacian_loss(x, tri), rtol=1e-6, atol=0)
    assert torch.equal(ML.edge_length_loss(x, twice), ML.edge_length_loss(x, tri))
    only = ML.edge_length_loss(x, torch.tensor([[3, 3, 3]]))               # no edge at all
    assert only.shape == (3,) and not only.any()
    ref = E.edge_ref(x.detach().numpy(), [[3, 3, 3]])
    assert not ref.loss.any() and not ref.grad.any()


# ---------------------------------------------------------------------------------------------------------------------
# shapes, methods, errors

def test_shapes_and_mesh_methods(tmp_path):
    import neural_renderer_amd as nr
    import neural_renderer
    for n in ('edge_length_loss', 'cotangent_laplacian_loss', 'mesh_edges', 'edge_lengths'):
        assert getattr(nr, n) is getattr(ML, n) and getattr(neural_renderer, n) is getattr(ML, n) and n in nr.__all__
    v, f = R.inputs('ico1')
    faces = torch.tensor(f)
    rest = nr.edge_lengths(torch.tensor(E.copy_of('ico1', 0)), faces)
    assert rest.shape == (3, 120)
    for fn, kw in ((nr.edge_length_loss, {}), (nr.edge_length_loss, {'target': 0.3}), (nr.edge_length_loss, {'target': rest[0]}),
                   (nr.cotangent_laplacian_loss, {})):
        batch = fn(torch.tensor(v), faces, **kw)
        single = fn(torch.tensor(v[1]), faces, **kw)
        assert batch.shape == (3,) and single.dim() == 0
        assert torch.equal(fn(torch.tensor(v[1:2]), faces, **kw)[0], single)
        assert torch.equal(fn(torch.tensor(v), faces[None].expand(3, -1, -1), **kw), batch)     # [B,Nf,3] with equal images
        assert torch.equal(fn(torch.tensor(v), faces, implementation='torch', **kw), batch)
    per_image = nr.edge_length_loss(torch.tensor(v), faces, target=rest)
    for k in range(3):
        assert torch.equal(nr.edge_length_loss(torch.tensor(v[k]), faces, target=rest[k]), per_image[k])
    # a learnable target: the torch path differentiates it
    t = rest[0].clone().requires_grad_(True)
    nr.edge_length_loss(torch.tensor(v), faces, target=t).sum().backward()
    assert t.grad is not None and t.grad.abs().sum() > 0
    path = tmp_path / 'ico.obj'
    with open(str(path), 'w') as fh:
        for p in v[0]:
            fh.write('v %r %r %r\n' % tuple(float(c) for c in p))
        for tri in f:
            fh.write('f %d %d %d\n' % tuple(int(i) + 1 for i in tri))
    mesh = nr.Mesh(str(path), normalization=False)
    edge, rigid, cot = mesh.edge_length_loss(), mesh.edge_length_loss(target=rest[0]), mesh.cotangent_laplacian_loss()
    assert all(t.dim() == 0 and t.requires_grad for t in (edge, rigid, cot))
    assert torch.equal(edge.detach(), nr.edge_length_loss(mesh.vertices.detach(), mesh.faces))
    assert torch.equal(rigid.detach(), nr.edge_length_loss(mesh.vertices.detach(), mesh.faces, target=rest[0]))
    assert torch.equal(cot.detach(), nr.cotangent_laplacian_loss(mesh.vertices.detach(), mesh.faces, eps=1e-12))
    (edge + rigid + cot).backward()
    assert mesh.vertices.grad is not None and mesh.vertices.grad.abs().sum() > 0


def test_argument_errors():
    v, f = R.inputs('ico1')
    x, faces = torch.tensor(v), torch.tensor(f)
    for fn in (ML.edge_length_loss, ML.cotangent_laplacian_loss, ML.edge_length_loss_torch, ML.cotangent_laplacian_loss_torch,
               ML.edge_lengths):
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
    for fn in (ML.edge_length_loss, ML.cotangent_laplacian_loss):
        with pytest.raises(ValueError):
            fn(x, faces, implementation='cuda')
        with pytest.raises(ValueError):
            fn(x, faces, implementation='hip')                               # CPU tensors do not fit the kernels
        with pytest.raises(ValueError):
            fn(x.double(), faces, implementation='hip')
    for fn in (ML.edge_length_loss, ML.edge_length_loss_torch):
        for bad in (-0.5, float('inf'), float('nan'), True, '1', None):      # the target as a number
            with pytest.raises(ValueError):
                fn(x, faces, target=bad)
        for bad in (torch.zeros(119), torch.zeros(3, 119), torch.zeros(2, 120), torch.zeros(1, 120), torch.zeros(3, 120, 1),
                    torch.zeros(120, dtype=torch.int64), torch.zeros(120, device='meta')):
            with pytest.raises(ValueError):
                fn(x, faces, target=bad)
    with pytest.raises(ValueError):
        ML.cotangent_laplacian_loss(x, faces, eps='small')
    for bad in (0, -1, 4.5, True):
        with pytest.raises(ValueError):
            ML.mesh_edges(faces, bad)
    with pytest.raises(IndexError):
        ML.mesh_edges(faces, 41)
    with pytest.raises(ValueError):
        ML.mesh_edges(faces.float(), 42)


def test_new_entry_points_return_error_codes_without_a_gpu():
    from neural_renderer_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert lib.nr_version() == 600
    # NULL pointers (NR_E_NULL = -1), sizes (-2), workspace (-3): all before any launch
    fwd, bwd, weights, apply = lib.nr_edge_length_forward, lib.nr_edge_length_backward, lib.nr_cot_weights, lib.nr_cot_apply
    assert fwd(None, None, None, None, 1, 4, 6, 0, 0.0, None, 0, None) == -1
    assert fwd(1, None, None, 1, 1, 4, 6, 0, 0.0, 1, 64, None) == -1                 # edges announced, no list
    assert fwd(1, 1, None, 1, 0, 4, 6, 0, 0.0, 1, 64, None) == -2
    assert fwd(1, 1, None, 1, 65536, 4, 6, 0, 0.0, 1, 1 << 30, None) == -2
    assert fwd(1, 1, None, 1, 1, 0, 6, 0, 0.0, 1, 64, None) == -2
    assert fwd(1, 1, None, 1, 1, 4, -1, 0, 0.0, 1, 64, None) == -2
    assert fwd(1, 1, None, 1, 1, 4, 6, 0, -0.5, 1, 64, None) == -2                   # a negative / non-finite target number
    assert fwd(1, 1, None, 1, 1, 4, 6, 0, float('nan'), 1, 64, None) == -2
    assert fwd(1, 1, None, 1, 1, 4, 6, 0, float('inf'), 1, 64, None) == -2
    assert fwd(1, 1, None, 1, 1, 4, 6, 0, 0.0, None, 0, None) == -3
    assert fwd(1, 1, None, 1, 2, 4, 300, 0, 0.0, 1, 2 * 2 * 8 - 1, None) == -3
    assert fwd(1, None, None, 1, 1, 4, 0, 0, 0.0, None, 0, None) == -3               # no edges: still a workspace
    assert bwd(None, None, None, None, None, None, None, 1, 4, 12, 6, 0, 0.0, None) == -1
    assert bwd(1, 1, None, 1, None, 1, 1, 1, 4, 12, 6, 0, 0.0, None) == -1           # neighbours announced, no list
    assert bwd(1, 1, 1, None, 1, 1, 1, 1, 4, 12, 6, 0, 0.0, None) == -1              # a target tensor without nbr_edge
    assert bwd(1, 1, 1, 1, None, 1, None, 1, 4, 12, 6, 0, 0.0, None) == -1
    assert bwd(1, 1, 1, 1, None, 1, 1, 1, 0, 12, 6, 0, 0.0, None) == -2
    assert bwd(1, 1, 1, 1, None, 1, 1, 1, 4, -1, 6, 0, 0.0, None) == -2
    assert bwd(1, 1, 1, 1, None, 1, 1, 1, 4, 12, 6, 0, -1.0, None) == -2
    assert bwd(1, 1, 1, 1, 1, 1, 1, 1, 4, 12, 0, 0, 0.0, None) == -2                 # neighbours and a target, no edge
    assert weights(None, None, None, 1, 4, 4, 1e-12, None) == -1
    assert weights(1, 1, None, 1, 4, 4, 1e-12, None) == -1
    assert weights(1, 1, 1, 0, 4, 4, 1e-12, None) == -2
    assert weights(1, 1, 1, 1, 4, 0, 1e-12, None) == -2
    assert weights(1, 1, 1, 65536, 4, 4, 1e-12, None) == -2
    assert apply(None, None, None, None, None, None, None, None, 1, 4, 4, None, 0, None) == -1
    assert apply(1, 1, 1, 1, None, None, 1, 1, 1, 4, 4, 1, 64, None) == -1
    assert apply(1, 1, 1, 1, 1, None, None, None, 1, 4, 4, 1, 64, None) == -1        # neither an output nor a loss
    assert apply(1, 1, 1, 1, 1, None, 1, 1, 1, 0, 4, 1, 64, None) == -2
    assert apply(1, 1, 1, 1, 1, None, 1, 1, 1, 4, 0, 1, 64, None) == -2
    assert apply(1, 1, 1, 1, 1, None, 1, 1, 1, 4, 4, None, 0, None) == -3            # a loss needs the workspace
    assert apply(1, 1, 1, 1, 1, None, None, 1, 2, 300, 4, 1, 2 * 2 * 8 - 1, None) == -3
