"""Mesh subdivision on the GPU (include/nr_hip.h nr_stencil_apply; neural_renderer_amd/subdivision.py): the HIP path in both
directions entry by entry against the float64 restatement of tests/subdivision_ref.py within its derived bound, bit-for-bit
repetition, the batch against its slices, identity rows, the torch path, the autograd wiring through a render, graph
capture and the example."""
import numpy as np
import pytest

import subdivision_ref as R
from test_subdivision import apply_and_grad, check_against_restatement, images_per_thread

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 5, 16)
# The kernel walks a row once for IMAGES images (csrc/nr_subdivision.hip), groups of IMAGES images on the grid's y: a batch
# of more images runs several groups, and one that is no multiple of IMAGES ends in a partial group whose unused slots read
# the last image and store nothing.  WIDE: two full groups and a partial one; GROUP_EDGES: exactly one group, one image more.
IMAGES = images_per_thread()
WIDE = 2 * IMAGES + 1
GROUP_EDGES = (IMAGES, IMAGES + 1)


def _plan(name, levels, scheme):
    import torch
    import neural_renderer_amd as nr
    v, f = R.mesh(name)
    return nr.subdivision(torch.tensor(f, device='cuda'), len(v), levels, scheme)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('scheme', R.SCHEMES)
@pytest.mark.parametrize('name', R.MESHES)
def test_hip_against_the_float64_restatement(name, scheme):
    """Forward and backward, levels 1 to 3 (3 on tetra and ico1), C in (1, 3, 5, 16), B = 3, B = 1 and no batch axis; and the
    torch path on the same tensors within twice the bound (each path is within the bound of the restatement)."""
    for levels in (1, 2, 3):
        if levels == 3 and name not in R.LEVEL3:
            continue
        plan = _plan(name, levels, scheme)
        for channels in CHANNELS:
            x, _ = R.inputs(name, channels)
            ref = R.reference(name, levels, scheme, channels)
            what = '%s %s L%d C%d' % (name, scheme, levels, channels)
            got, grad = apply_and_grad(plan, x, ref.g, device='cuda', implementation='hip')
            assert got.shape == ref.value.shape and got.dtype == np.float32
            check_against_restatement(got, grad, ref, what=what + ' B3')
            auto, auto_grad = apply_and_grad(plan, x, ref.g, device='cuda')          # implementation=None takes the kernel
            assert np.array_equal(auto, got) and np.array_equal(auto_grad, grad)
            t_got, t_grad = apply_and_grad(plan, x, ref.g, device='cuda', implementation='torch')
            check_against_restatement(t_got, t_grad, ref, what=what + ' torch')
            assert R.worst_ratio(got, t_got, ref.value_mag) <= 2 * ref.constant
            assert R.worst_ratio(grad, t_grad, ref.grad_mag) <= 2 * ref.constant_backward
            one, one_grad = apply_and_grad(plan, x[2:], ref.g[2:], device='cuda', implementation='hip')
            check_against_restatement(one, one_grad, ref, images=slice(2, 3), what=what + ' B1')
            flat, flat_grad = apply_and_grad(plan, x[1], ref.g[1], device='cuda', implementation='hip')
            assert flat.shape == ref.value.shape[1:]
            check_against_restatement(flat[None], flat_grad[None], ref, images=slice(1, 2), what=what + ' [Nv,C]')
            # batches that span several groups of images and end in a partial one
            for images in (WIDE,) + (GROUP_EDGES if channels == 3 else ()):
                xw, refw = R.inputs_wide(name, channels, images), R.reference_wide(name, levels, scheme, channels, images)
                wide, wide_grad = apply_and_grad(plan, xw, refw.g, device='cuda', implementation='hip')
                assert wide.shape == refw.value.shape == (images,) + ref.value.shape[1:]
                check_against_restatement(wide, wide_grad, refw, what=what + ' B%d' % images)
                # the first images are the batch of B = 3 above: the same bits, whatever group shape they ran in
                assert np.array_equal(wide[:3].view(np.int32), got.view(np.int32))
                assert np.array_equal(wide_grad[:3].view(np.int32), grad.view(np.int32))


@pytest.mark.parametrize('name,scheme,levels', [('blocks', 'loop', 2), ('odd', 'loop', 2), ('grid', 'midpoint', 1)])
def test_bit_reproducibility(name, scheme, levels):
    """Two runs give the same bits, forward and backward; image k alone gives the bits it has inside the batch."""
    import torch
    plan = _plan(name, levels, scheme)
    for channels in (3, 16):
        x = torch.tensor(R.inputs(name, channels)[0], device='cuda')
        g = torch.tensor(R.reference(name, levels, scheme, channels).g, device='cuda')

        def run(x, g):
            x = x.clone().requires_grad_(True)
            y = plan(x, implementation='hip')
            return y.detach(), torch.autograd.grad((y * g).sum(), x)[0]
        y0, g0 = run(x, g)
        y1, g1 = run(x, g)
        assert torch.equal(_bits(y0), _bits(y1)) and torch.equal(_bits(g0), _bits(g1))
        for k in range(x.shape[0]):
            yk, gk = run(x[k:k + 1], g[k:k + 1])
            assert torch.equal(_bits(yk[0]), _bits(y0[k])) and torch.equal(_bits(gk[0]), _bits(g0[k]))
            yk, gk = run(x[k], g[k])
            assert torch.equal(_bits(yk), _bits(y0[k])) and torch.equal(_bits(gk), _bits(g0[k]))
        # a batch over several groups of images with a partial last one: every image alone -- the first, second and last
        # group's among them -- and every group alone give the bits they have inside the batch
        xw = torch.tensor(R.inputs_wide(name, channels, WIDE), device='cuda')
        gw = torch.tensor(R.reference_wide(name, levels, scheme, channels, WIDE).g, device='cuda')
        yw0, gw0 = run(xw, gw)
        yw1, gw1 = run(xw, gw)
        assert torch.equal(_bits(yw0), _bits(yw1)) and torch.equal(_bits(gw0), _bits(gw1))
        assert torch.equal(_bits(yw0[:3]), _bits(y0)) and torch.equal(_bits(gw0[:3]), _bits(g0))
        for k in range(WIDE):
            yk, gk = run(xw[k:k + 1], gw[k:k + 1])
            assert torch.equal(_bits(yk[0]), _bits(yw0[k])) and torch.equal(_bits(gk[0]), _bits(gw0[k])), k
        for k in range(0, WIDE, IMAGES):
            yk, gk = run(xw[k:k + IMAGES], gw[k:k + IMAGES])
            assert torch.equal(_bits(yk), _bits(yw0[k:k + IMAGES])) and torch.equal(_bits(gk), _bits(gw0[k:k + IMAGES])), k
        # a shifted window: images that sat in slots 1 .. of their groups now sit in slots 0 ..
        yk, gk = run(xw[1:IMAGES + 2], gw[1:IMAGES + 2])
        assert torch.equal(_bits(yk), _bits(yw0[1:IMAGES + 2])) and torch.equal(_bits(gk), _bits(gw0[1:IMAGES + 2]))


@pytest.mark.parametrize('name,scheme', [('grid', 'midpoint'), ('odd', 'midpoint'), ('odd', 'loop')])
def test_identity_rows_copy_their_input(name, scheme):
    """Rows {v: 1} -- every old vertex of the midpoint scheme; Loop's corners: the vertices of 'odd' whose number of sharp
    edges is neither 0 nor 2, and its isolated vertex -- return their input bit for bit (w_0 * x_0 with w_0 = 1: no fma in
    front of it), a negative zero included."""
    import torch
    rows = R.plan(name, 1, scheme).rows[0]
    ident = [(r, next(iter(row))) for r, row in enumerate(rows) if len(row) == 1]
    assert ident and all(rows[r][c] == 1.0 for r, c in ident)
    nv = len(R.mesh(name)[0])
    if scheme == 'midpoint':
        assert [r for r, _ in ident] == list(range(nv))
    x = torch.tensor(R.inputs(name, 5)[0], device='cuda')
    x[0, ident[0][1], 0] = -0.0
    y = _plan(name, 1, scheme)(x, implementation='hip')
    r, c = (torch.tensor(t, device='cuda') for t in zip(*ident))
    assert torch.equal(_bits(y[:, r]), _bits(x[:, c]))


def test_identity_rows_across_groups_of_images():
    """The midpoint scheme's old vertices in a batch over several groups of images, the last one partial: image b of the
    output holds image b of the input bit for bit, so no group reads or stores another group's image."""
    import torch
    nv = len(R.mesh('blocks')[0])
    x = torch.tensor(R.inputs_wide('blocks', 3, WIDE), device='cuda')
    y = _plan('blocks', 1, 'midpoint')(x, implementation='hip')
    assert y.shape[0] == WIDE and torch.equal(_bits(y[:, :nv]), _bits(x))
    assert len({bytes(x[b].cpu().numpy().tobytes()) for b in range(WIDE)}) == WIDE      # (the images all differ)


def test_second_derivative_raises():
    """The operator is once-differentiable: differentiating its backward raises instead of returning a wrong zero."""
    import torch
    x = torch.tensor(R.inputs('ico1')[0], device='cuda', requires_grad=True)
    y = _plan('ico1', 1, 'loop')(x, implementation='hip')
    g, = torch.autograd.grad((y * y).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        g.sum().backward()


def test_chain_through_the_renderer():
    """render_silhouettes of subdivide(vertices, faces, 1, 'loop') back-propagates to the control vertices: that gradient
    equals the restatement's transposed product of the gradient taken at the fine vertices of the SAME render, within the
    backward bound.  This pins the autograd wiring, not the rasterizer."""
    import torch
    import neural_renderer_amd as nr
    x, f = R.inputs('ico1')
    control = torch.tensor(x[:2], device='cuda', requires_grad=True)
    faces = torch.tensor(f, device='cuda')[None].expand(2, -1, -1)
    fine, fine_faces = nr.subdivide(control, faces, 1, 'loop', implementation='hip')
    assert fine.shape == (2, 162, 3) and fine_faces.shape == (2, 320, 3) and fine.requires_grad
    fine.retain_grad()
    r = nr.Renderer()
    r.image_size = 32
    r.eye = nr.get_points_from_angles(2.732, 20, 40)
    target = torch.zeros((2, 32, 32), device='cuda')
    target[:, 8:24, 6:20] = 1
    ((r.render_silhouettes(fine, fine_faces) - target) ** 2).sum().backward()
    g = fine.grad.cpu().numpy().astype(np.float64)
    assert np.abs(g).sum() > 0
    p = R.plan('ico1', 1, 'loop')
    ratio = R.worst_ratio(control.grad.cpu().numpy(), p.apply_transposed(g), p.apply_transposed(g, True))
    print('chain through the renderer: control gradient at %.3f of u M (C = %d)' % (ratio, p.constant_backward))
    assert ratio <= p.constant_backward


def test_graph_capture_equals_eager():
    """A step -- plan(vertices) and its gradient -- captured with neural_renderer_amd.graph.capture replays bit-equal to
    eager after the inputs change.  The plan is built on the host, before the capture."""
    import torch
    import neural_renderer_amd as nr
    name, levels = 'blocks', 2
    x = R.inputs(name, 3)[0]
    vertices = torch.tensor(x, device='cuda', requires_grad=True)
    faces = torch.tensor(R.mesh(name)[1], device='cuda')
    plan = nr.subdivision(faces, vertices.shape[1], levels)                 # builds the tables eagerly
    w = torch.tensor(R.reference(name, levels, 'loop', 3).g, device='cuda')
    out = torch.zeros((3, plan.num_vertices, 3), device='cuda')

    def step():
        y = nr.subdivision(faces, vertices.shape[1], levels)(vertices)
        out.copy_(y)
        return torch.autograd.grad((y * w).sum(), [vertices])
    grads = [None]

    def captured():
        grads[0] = step()
    replay = nr.graph.capture(captured)
    with torch.no_grad():
        vertices.copy_(torch.tensor(R.inputs(name, 3, seed=1)[0]))
        w.copy_(torch.tensor(R.upstream(tuple(w.shape), seed=1)))
    replay()
    torch.cuda.synchronize()
    got_out, got = out.clone(), grads[0][0].clone()
    eager = step()
    assert torch.equal(_bits(got_out), _bits(out)) and torch.equal(_bits(got), _bits(eager[0]))
    assert float(got.abs().sum()) > 0


def test_unknown_topology_raises_while_capturing(monkeypatch):
    """The plan is built on the host, which a capture cannot do: an index tensor that subdivision has not seen raises there
    (as mesh_losses._tables does).  The capture state is simulated; nothing is captured."""
    import importlib
    import torch
    import neural_renderer_amd as nr
    S = importlib.import_module('neural_renderer_amd.subdivision')
    x, f = R.inputs('ico1')
    vertices, faces = torch.tensor(x, device='cuda'), torch.tensor(f, device='cuda')
    seen = torch.tensor(f, device='cuda')
    want, _ = nr.subdivide(vertices, seen)
    checked = torch.tensor(f, device='cuda')
    nr.laplacian_loss(vertices, checked)             # its indices are range-checked, its plan is not built
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='before the capture'):
        nr.subdivide(vertices, faces)
    with pytest.raises(RuntimeError, match='not built yet'):
        S.subdivision(checked, 42, 1)
    with pytest.raises(RuntimeError, match='not built yet'):
        S.subdivision(seen, 42, 2)                   # another number of levels is another plan
    assert torch.equal(nr.subdivide(vertices, seen)[0], want)      # a known one goes through


def test_example_subdivision_first_steps():
    """examples/example_subdivision.py: the coarse-to-fine silhouette fit from icosphere(1); its first steps with the first
    refinement run, every loss is finite, the mesh has 162 vertices afterwards and the loss has gone down."""
    import os
    import sys
    import torch
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import make_data
    make_data.main()
    import example_subdivision
    model = example_subdivision.Model(os.path.join(ex, 'data', 'example2_ref.png')).cuda()
    assert model.num_vertices == 42
    counts = []
    losses = example_subdivision.fit(model, 36, (24,), on_step=lambda i, loss, terms: counts.append(model.num_vertices))
    assert counts == [42] * 24 + [162] * 12 and model.faces.shape == (1, 320, 3)
    assert all(np.isfinite(losses)) and bool(torch.isfinite(model.vertices).all())
    print('example_subdivision: loss %.4f -> %.4f (at the refinement %.4f -> %.4f)' % (losses[0], losses[-1], losses[23], losses[24]))
    assert losses[-1] < losses[0]
