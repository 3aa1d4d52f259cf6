"""Layout, alignment and stream invariance of every HIP-backed operator ("Tensor boundary").

The kernels are pinned to the oracle and to float64 restatements elsewhere, on fresh contiguous tensors on the default
stream.  Here the SAME call is made twice -- on contiguous, 16-byte aligned copies and on other layouts of the same values
(or on a side stream) -- and the results are compared.  The layouts (`lay`):

    offset4 / offset8 / offset12   a contiguous .view into a flat buffer 1, 2 or 3 elements longer: 4, 8 or 12 bytes off the
                                   16-byte grid on which the kernels read maps, cubes and workspaces as float4
    strided                        every second element of a buffer of twice the width
    permuted                       stored in the reversed axis order and permuted back (R: the transpose of its transpose)
    expanded                       stride 0 on the batch axis (only tensors whose images are all equal)
    int64                          index tensors as int64, 8 bytes off the grid

Upstream gradients arrive in the same layouts (`grad_as`) and as the stride-0 gradient of `out.sum().backward()`.

What "equal" means, per result (the kernel comment each choice rests on):
  bits    torch.equal.  Every forward output, and every gradient of an operator that the project states to be order-free:
          the image epilogue (nr_image.hip), batched cube gradients at ts = 2 ("24 register accumulators per lane, group
          reduction, one 96-byte store per face ... no atomics", nr_backward_gather.hip), the mesh losses ("no float or
          double atomics in either direction", nr_mesh_losses.hip), subdivision ("No atomics, every output element is
          stored", nr_subdivision.hip), the UV bake (its inverse map is a gather), lights ("no atomics, the same bits in
          every run", nr_lights.hip), vertex_shade ("no atomics in either direction", nr_vertex_colors.hip) and Adam
          (elementwise).
  ints    torch.equal after upstream gradients that are small integers: vertices_to_faces' scatter uses float atomics in
          arrival order (nr_geometry.hip), and sums of small integers are exact in float32 in any order.
  order   H.rel_err(a, b) <= SAME_TERMS, the suite's criterion for two runs of one call (test_hip_parity.py): grad_faces
          (K6's double atomics arrive in no fixed order) and what is summed by unordered atomics behind it -- the shared
          cubes' gradient, larger cubes' (LDS doubles added in arrival order), the face light's, the per-pixel UV images'
          and the corner colours' (double atomics per run of lanes: nr_backward_gather.hip, nr_uv_pixel.hip,
          nr_vertex_colors.hip) -- and the Renderer's eye and camera gradients, double sums of the front-end over that
          grad_faces.  A layout error is wrong by whole entries.
  close   max |a - b| <= GRAD_TOL max |b|, the suite's criterion for the vertex gradient of two Renderer paths
          (test_face_light_gpu.GRAD_TOL = 1e-5; test_shared_textures_gpu.py, "grad_vertices"): the Renderer's vertex
          gradient.  The front-end scatters it with float atomics in arrival order behind non-integer factors
          (nr_frontend.hip), so two runs differ by up to 2 gamma(n - 1) of an entry's sum of magnitudes -- n <= 12 addends
          on the icosphere, 1.3e-6 of that sum -- and an entry that cancels can be much smaller than its sum of magnitudes,
          which is why rel_err's entry-by-entry view does not fit here (25 repetitions of these cases on an MI355X: up to
          1.7e-5 entry by entry, below 1.4e-7 of the largest entry).  The entrywise statement for these sums is made where
          their magnitudes are known: `entry`.
  entry   the front-end called directly: its vertex and camera gradients multiply by non-integers in front of float
          atomics (nr_frontend.hip), so every layout's result is held to the bound the contiguous call is held to --
          frontend_ref.worst_ratio against the float64 restatement with test_frontend_ref.CONSTANTS (<= 1).

Measured on an MI355X: every `order` comparison of the rasterizer cases came out bit-equal at these sizes; the Renderer's
camera gradients too; `entry` stayed below 0.04 of its bound in every layout.

Every contiguous result is checked to be non-trivial first (some pixels covered, some not; every compared gradient with a
non-zero sum of magnitudes), so two wrong but equal results cannot pass."""
import numpy as np
import pytest
import torch

import helpers as H
import abi
import uv_ref
import frontend_ref as F
from test_frontend_ref import CONSTANTS, reference, run_module
from test_hip_parity import SAME_TERMS
from test_face_light_gpu import GRAD_TOL

pytestmark = pytest.mark.gpu

FLOAT_LAYOUTS = ('offset4', 'offset8', 'offset12', 'strided', 'permuted')
GRAD_LAYOUTS = FLOAT_LAYOUTS + ('stride0',)


# ---------------------------------------------------------------------------------------------------------------------
# layouts

def lay(x, name):
    """The values of x in the named layout, differentiable in x.  None stays None; a layout that does not apply to x (an
    integer layout on floats, `expanded` on images that differ) returns x."""
    if x is None or name in ('plain', 'contiguous'):
        return x
    if name == 'int64' and x.is_floating_point():
        return x
    if name == 'int64' or name.startswith('offset'):
        if name == 'int64':
            x, k = x.long(), 1       # 8 bytes off the grid
        else:
            k = int(name[6:]) // 4   # elements of a 4-byte type: 4, 8 or 12 bytes off the grid
        flat = torch.cat((x.new_zeros(k), x.reshape(-1)))
        v = flat[k:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == (k * x.element_size()) % 16
        return v
    if name == 'strided':
        v = torch.stack((x, torch.zeros_like(x)), dim=-1)[..., 0]
        assert x.numel() < 2 or not v.is_contiguous()
        return v
    if name == 'permuted':
        if x.dim() < 2:
            return lay(x, 'strided')
        back = tuple(reversed(range(x.dim())))
        return x.permute(*back).contiguous().permute(*back)
    if name == 'expanded':
        if x.dim() < 2 or x.shape[0] < 2 or not bool((x == x[0:1]).all()):
            return x
        v = x[0:1].expand(x.shape)
        assert v.stride(0) == 0
        return v
    raise ValueError(name)


class _GradLayout(torch.autograd.Function):
    """Identity whose backward hands the gradient on in a named layout: what the operator in front of it receives."""

    @staticmethod
    def forward(ctx, x, name):
        ctx.name = name
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if ctx.name == 'stride0':
            assert all(s == 0 for s in g.stride()) or g.numel() == 1, 'out.sum().backward() gives a stride-0 gradient'
            return g, None
        if ctx.name in ('contiguous', 'ones'):
            g = g.clone(memory_format=torch.contiguous_format)
            assert g.data_ptr() % 16 == 0
            return g, None
        return lay(g, ctx.name), None


def grad_as(y, name):
    return None if y is None else _GradLayout.apply(y, name)


def _cuda(a, grad=False):
    a = np.ascontiguousarray(a)
    return torch.tensor(a, device='cuda', requires_grad=bool(grad) and a.dtype.kind == 'f')


def _host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# a case: named inputs, a call, and how its gradients compare

class Case(object):
    """inputs: name -> float32 array (a leaf that takes a gradient unless named in `fixed`) or integer array.
    call(t, L, G) -> dict of outputs: t the leaves by name, L(x) an input in the run's layout, G(y) an output whose gradient
    arrives in the run's layout.  kinds: gradient name -> 'bits' | 'order' | 'close' (default `kind`).  integer: upstream
    gradients are small integers.  covered(outs) -> a 0/1 map that must hold both values, or None."""

    def __init__(self, inputs, call, kind='bits', kinds=None, fixed=(), integer=False, covered=None, layouts=FLOAT_LAYOUTS,
                 grad_layouts=GRAD_LAYOUTS):
        self.inputs, self.call, self.kind, self.kinds, self.fixed = inputs, call, kind, kinds or {}, fixed
        self.integer, self.covered, self.layouts, self.grad_layouts = integer, covered, layouts, grad_layouts
        self.upstream = {}
        self.worst = {}   # kind -> the largest error seen by an 'order' / 'close' comparison

    def leaves(self):
        return {n: _cuda(a, n not in self.fixed) for n, a in self.inputs.items()}

    def _weights(self, key, out):
        w = self.upstream.get(key)
        if w is None:
            rng = np.random.default_rng(len(self.upstream) + 1)
            a = rng.integers(-3, 4, tuple(out.shape)) if self.integer else rng.normal(size=tuple(out.shape))
            w = self.upstream[key] = _cuda(a.astype(np.float32))
        return w

    def run(self, layout='plain', grad_layout='contiguous', leaves=None, only=None):
        """-> (outputs, gradients by input name).  `only`: the outputs that take an upstream gradient (default: all)."""
        t = leaves if leaves is not None else self.leaves()
        outs = self.call(t, lambda x: lay(x, layout), lambda y: grad_as(y, grad_layout))
        loss = 0
        for key, o in outs.items():
            if o is None or not o.requires_grad or (only is not None and key not in only):
                continue
            loss = loss + (o.sum() if grad_layout in ('stride0', 'ones') else (o * self._weights(key, o)).sum())
        names = [n for n, x in t.items() if x.requires_grad]
        grads = torch.autograd.grad(loss, [t[n] for n in names], allow_unused=True) if names else ()
        return ({k: (None if o is None else o.detach()) for k, o in outs.items()},
                {n: g for n, g in zip(names, grads) if g is not None})

    def _is_expanded(self, name, layout):
        a = self.inputs[name]
        return layout == 'expanded' and a.ndim >= 2 and a.shape[0] >= 2 and bool((a == a[0:1]).all())

    def compare(self, got, ref, what, layout=None):
        (o1, g1), (o0, g0) = got, ref
        assert sorted(o1) == sorted(o0) and sorted(g1) == sorted(g0), what
        for k in o0:
            if o0[k] is not None:
                assert o1[k].shape == o0[k].shape and torch.equal(o1[k], o0[k]), '%s: output %s' % (what, k)
        for n in g0:
            assert g1[n].shape == g0[n].shape, (what, n)
            a, b = g1[n], g0[n]
            if self._is_expanded(n, layout):   # one row behind all images: its gradient is the images' sum, the rest zeros
                assert float(a[1:].abs().sum()) == 0, (what, n)
                a, b = a[0], b.sum(0)
            kind = self.kinds.get(n, self.kind)
            if kind == 'bits':
                assert torch.equal(a, b), '%s: gradient of %s' % (what, n)
            elif kind == 'order':
                err = H.rel_err(_host(a), _host(b))
                self.worst[kind] = max(self.worst.get(kind, 0.0), err)
                assert err <= SAME_TERMS, '%s: gradient of %s, rel_err %.3g' % (what, n, err)
            else:
                err = float((a - b).abs().max()) / float(b.abs().max())
                self.worst[kind] = max(self.worst.get(kind, 0.0), err)
                assert err <= GRAD_TOL, '%s: gradient of %s, max |a - b| / max |b| %.3g' % (what, n, err)

    def nontrivial(self, ref, what, need=None):
        outs, grads = ref
        if self.covered is not None:
            c = self.covered(outs)
            assert bool((c > 0).any()) and bool((c == 0).any()), '%s: some pixels covered and some not' % what
        need = [n for n, x in self.inputs.items() if x.dtype.kind == 'f' and n not in self.fixed] if need is None else need
        for n in need:
            assert n in grads and float(grads[n].abs().sum()) > 0 and bool(torch.isfinite(grads[n]).all()), (what, n)


def check_layouts(case, what, subsets=(None,), need=None):
    """Every layout of the inputs and every layout of the upstream gradients against the contiguous call."""
    for only in subsets:
        ref = case.run(only=only)
        case.nontrivial(ref, what, need if only is None else [])
        assert only is None or any(float(g.abs().sum()) > 0 for g in ref[1].values()), (what, only)
        for name in case.layouts:
            case.compare(case.run(layout=name, only=only), ref, '%s, inputs %s, gradients of %s' % (what, name, only), name)
        for name in case.grad_layouts:
            if name == 'stride0':
                continue
            case.compare(case.run(grad_layout=name, only=only), ref, '%s, upstream %s of %s' % (what, name, only))
        if only is None:   # everything at once: inputs and upstream gradients 4 bytes off
            case.compare(case.run('offset4', 'offset4'), ref, what + ', inputs and upstream offset4')
    if 'stride0' in case.grad_layouts:
        ones = case.run(grad_layout='ones')
        case.compare(case.run(grad_layout='stride0'), ones, what + ', the stride-0 gradient of sum()')
    if case.worst:
        print('%s: worst %s' % (what, ', '.join('%s %.3g (bound %.3g)' % (k, v, SAME_TERMS if k == 'order' else GRAD_TOL)
                                                for k, v in sorted(case.worst.items()))))


# ---------------------------------------------------------------------------------------------------------------------
# the rasterizer

B, NF = 2, 61   # 61 * 9 % 4 = 1: a slice of the faces' rows is off the grid for real


def _raster_case(S, ts, shared, lit, source='cubes', smooth=False):
    """nr.Rasterize called directly on a random scene, rgb + alpha + depth."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(1000 + 8 * S + ts)
    inputs = {'faces': H.random_scene(rng, B, NF, size=0.4)}
    kinds = {'faces': 'order'}
    layout = None
    if source == 'cubes':
        inputs['textures'] = rng.uniform(0, 1, (1 if shared else B, NF, ts, ts, ts, 3)).astype(np.float32)
        if shared or ts != 2:
            # one cube for all images: double atomics per (image, face) pair; ts > 2: a face's lanes add into LDS doubles in
            # arrival order before the store.  Per-image cubes of ts = 2 are summed in registers in a fixed order: bits
            kinds['textures'] = 'order'
        if lit:
            inputs['light'] = rng.uniform(0.2, 1.2, (B, NF, 3)).astype(np.float32)
            kinds['light'] = 'order'
    elif source == 'corner':
        inputs['colors'] = rng.uniform(0, 1, (B, NF, 3, 3)).astype(np.float32)
        kinds['colors'] = 'order'
    else:   # per-pixel UV images, 15 + 63 = 78 pixels: the packing's second image starts off the grid
        sizes = [(3, 5), (7, 9)]
        uv, face_image, base = uv_ref.random_layout(rng, NF, ts, sizes)
        layout = nr.UVLayout(uv, face_image, base, sizes)
        inputs['light'] = rng.uniform(0.2, 1.2, (B, NF, 3, 3) if smooth else (B, NF, 3)).astype(np.float32)
        inputs['image0'] = rng.uniform(0, 1, (B, 3, 3, 5)).astype(np.float32)   # [Bi,3,H,W], handed over permuted
        inputs['image1'] = rng.uniform(0, 1, (B, 3, 7, 9)).astype(np.float32)
        kinds.update(light='order', image0='order', image1='order')

    def call(t, L, G):
        fn = nr.Rasterize(S, 0.1, 100, 1e-3, (0.2, 0.3, 0.4), True, True, True)
        if source == 'cubes':
            rgb, alpha, depth = fn(L(t['faces']), L(t['textures']), L(t.get('light')))
        elif source == 'corner':
            rgb, alpha, depth = fn(L(t['faces']), nr.CornerColors(L(t['colors'])))
        else:
            images = [L(t['image0']).permute(0, 2, 3, 1), L(t['image1']).permute(0, 2, 3, 1)]
            rgb, alpha, depth = fn(L(t['faces']), nr.UVImages(layout, images), L(t['light']))
        return {'rgb': G(rgb), 'alpha': G(alpha), 'depth': G(depth), 'face_index_map': fn.face_index_map}
    return Case(inputs, call, kinds=kinds, covered=lambda o: o['alpha'])


@pytest.mark.parametrize('S,ts', [(32, 2), (32, 3), (30, 2), (30, 3)], ids=['quad_float4cube', 'quad_cube3', 'scalar_float4cube',
                                                                              'scalar_cube3'])
def test_rasterize_called_directly(S, ts):
    """S = 32 reads the upstream maps as float4, S = 30 one by one; ts = 2 reads a cube as six float4, ts = 3 takes the
    general path.  Cubes per image and shared [1, ...], with and without face_light; the three upstream gradients together
    and one at a time."""
    for shared in (False, True):
        for lit in (False, True):
            case = _raster_case(S, ts, shared, lit)
            check_layouts(case, 'Rasterize S=%d ts=%d shared=%d lit=%d' % (S, ts, shared, lit),
                          subsets=(None, ('rgb',), ('alpha',), ('depth',)))
    # cubes [B, ...] that are an expanded view of one set
    case = _raster_case(S, ts, False, True)
    case.inputs['textures'][1] = case.inputs['textures'][0]
    case.layouts, case.grad_layouts = ('expanded',), ()
    check_layouts(case, 'Rasterize S=%d ts=%d, expanded cubes' % (S, ts))


@pytest.mark.parametrize('S', [32, 30])
def test_rasterize_function_protocol(S):
    """forward_gpu / backward_gpu, the chainer.Function protocol: no autograd in between, the gradients handed to
    backward_gpu are the caller's own tensors."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(50 + S)
    faces = H.random_scene(rng, B, NF, size=0.4)
    tex = rng.uniform(0, 1, (B, NF, 2, 2, 2, 3)).astype(np.float32)
    grads = [rng.normal(size=shape).astype(np.float32) for shape in ((B, S, S, 3), (B, S, S), (B, S, S))]

    def run(name):
        fn = nr.Rasterize(S, 0.1, 100, 1e-3, (0.2, 0.3, 0.4), True, True, True)
        inputs = (lay(_cuda(faces), name), lay(_cuda(tex), name))
        outs = fn.forward_gpu(inputs)
        return tuple(outs) + tuple(fn.backward_gpu(inputs, tuple(lay(_cuda(g), name) for g in grads)))
    ref = run('plain')
    assert bool((ref[1] == 1).any()) and bool((ref[1] == 0).any())
    assert all(float(g.abs().sum()) > 0 for g in ref[3:])
    for name in FLOAT_LAYOUTS:
        rgb, alpha, depth, gf, gt = run(name)
        for a, b in zip((rgb, alpha, depth, gt), ref[:3] + ref[4:]):
            assert torch.equal(a, b), name
        assert H.rel_err(_host(gf), _host(ref[3])) <= SAME_TERMS, name


@pytest.mark.parametrize('source', ['corner', 'uv', 'uv_smooth'])
def test_rasterize_other_shading_sources(source):
    """CornerColors [B,F,3,3], and UVImages sampled per pixel with a light colour per face (plain) and per corner (smooth);
    the images arrive as [Bi,3,H,W].permute(0,2,3,1) in every layout."""
    for S in (32, 30):
        case = _raster_case(S, 2, False, True, source='corner' if source == 'corner' else 'uv', smooth=source == 'uv_smooth')
        check_layouts(case, 'Rasterize %s S=%d' % (source, S), subsets=(None, ('rgb',)))


@pytest.mark.parametrize('aa', [False, True], ids=['no_aa', 'aa'])
def test_rasterize_rgbad(aa):
    """The public wrapper: the epilogue (transpose, flip, 2x2 mean) behind the rasterizer, raster 32 (quad) and 30 (scalar)."""
    import neural_renderer_amd as nr
    for S in (32, 30):
        for lit in (False, True):
            rng = np.random.default_rng(40 + S)
            inputs = {'faces': H.random_scene(rng, B, NF, size=0.4),
                      'textures': rng.uniform(0, 1, (B, NF, 2, 2, 2, 3)).astype(np.float32)}
            if lit:
                inputs['light'] = rng.uniform(0.2, 1.2, (B, NF, 3)).astype(np.float32)

            def call(t, L, G):
                out = nr.rasterize_rgbad(L(t['faces']), L(t['textures']), S // 2 if aa else S, aa, 0.1, 100, 1e-3,
                                         (0.2, 0.3, 0.4), face_light=L(t.get('light')))
                return {k: G(out[k]) for k in ('rgb', 'alpha', 'depth')}
            case = Case(inputs, call, kinds={'faces': 'order', 'light': 'order'}, covered=lambda o: (o['alpha'] == 1).float())
            check_layouts(case, 'rasterize_rgbad S=%d aa=%d lit=%d' % (S, aa, lit), subsets=(None, ('alpha',)))


# ---------------------------------------------------------------------------------------------------------------------
# the Renderer and the front-end

def _sphere(level=1, scale=0.8):
    import neural_renderer_amd as nr
    v, f = nr.icosphere(level)
    return (v.numpy() * scale).astype(np.float32), f.numpy().astype(np.int32)


def _renderer_case(mode, method, ts=2):
    import neural_renderer_amd as nr
    import projection_ref
    rng = np.random.default_rng(7)
    v, f = _sphere()
    inputs = {'vertices': (v[None] + rng.normal(scale=0.02, size=(B,) + v.shape)).astype(np.float32),
              'faces': np.repeat(f[None], B, axis=0),
              'textures': rng.uniform(0, 1, (B, f.shape[0], ts, ts, ts, 3)).astype(np.float32)}
    size = 16
    if mode == 'projection':
        K, R, t, d = projection_ref.camera(B, seed=32, per_image=True, distortion=True, orig_size=256.0)
        inputs.update(K=K, Rt=np.ascontiguousarray(R.transpose(0, 2, 1)), t=t, dist=d)
    else:
        inputs['eye'] = np.asarray([nr.get_points_from_angles(2.732, 20.0 + 10 * i, 40.0 * i) for i in range(B)], np.float32)
        if mode == 'look':   # looking along (0.1, -0.2, 1) at the origin
            inputs['eye'] = np.asarray([[-0.27 + 0.1 * i, 0.5 + 0.05 * i, -2.6] for i in range(B)], np.float32)

    def call(t, L, G):
        r = nr.Renderer()
        r.image_size, r.camera_mode = size, mode
        r.light_direction, r.light_color_ambient, r.light_intensity_ambient = [0.3, 0.8, -0.5], [1.0, 0.9, 0.8], 0.4
        if mode == 'projection':
            # (R as the transpose of a stored R^T: the layout a pose network's output has)
            r.K, r.R, r.t, r.dist_coeffs, r.orig_size = L(t['K']), L(t['Rt']).transpose(1, 2), L(t['t']), L(t['dist']), 256
        else:
            r.eye = L(t['eye'])
            if mode == 'look':
                r.camera_direction = [0.1, -0.2, 1.0]
        vertices, faces, textures = L(t['vertices']), L(t['faces']), L(t['textures'])
        if method == 'render':
            out = {'rgb': G(r.render(vertices, faces, textures))}
        elif method == 'render_silhouettes':
            out = {'alpha': G(r.render_silhouettes(vertices, faces))}
        elif method == 'render_depth':
            out = {'depth': G(r.render_depth(vertices, faces))}
        else:
            out = {k: G(x) for k, x in r.render_rgbad(vertices, faces, textures).items()}
        assert r.last_frontend == 'fused'
        return out

    def covered(o):
        if 'alpha' in o:
            return (o['alpha'] == 1).float()
        if 'depth' in o:
            return (o['depth'] < 100).float()
        return (o['rgb'].abs().sum(1) > 0).float()   # (the background is black)
    fixed = ('dist',) + (('textures',) if method in ('render_silhouettes', 'render_depth') else ())
    kind = dict({n: 'order' for n in ('eye', 'K', 'Rt', 't')}, vertices='close')
    return Case(inputs, call, kinds=kind, fixed=fixed, covered=covered, layouts=FLOAT_LAYOUTS + ('int64', 'expanded'))


@pytest.mark.parametrize('method', ['render', 'render_silhouettes', 'render_depth', 'render_rgbad'])
@pytest.mark.parametrize('mode', ['look_at', 'look', 'projection'])
def test_renderer(mode, method):
    """icosphere(1), 42 vertices and 80 faces, through the fused front-end: layouts of the vertices, of the index tensor (int32,
    int64, [None].expand), of the cubes, of a tensor-valued eye and of K, R (as a transposed R^T), t and dist_coeffs."""
    case = _renderer_case(mode, method)
    need = ['vertices'] + ([] if method in ('render_silhouettes', 'render_depth') else ['textures'])
    need += ['K', 'Rt', 't'] if mode == 'projection' else ['eye']
    check_layouts(case, 'Renderer.%s %s' % (method, mode), need=need)


@pytest.mark.parametrize('cname,variant,ts', [('look_at_30', 'textures', 2), ('look', 'colors', 0),
                                               ('projection_per_image_dist', 'textures', 3),
                                               ('projection_t_b13_dist', 'colors', 0)])
def test_front_end_called_directly(cname, variant, ts):
    """frontend.project_and_light / project_and_light_colors on the fan (a vertex of valence 65): what is stored -- faces,
    lit textures, light colours, grad_textures -- has the contiguous call's bits in every layout; grad_vertices and the
    camera gradients, summed by float atomics behind non-integer factors, stay within the entrywise bound of the float64
    restatement that the contiguous call is held to (test_frontend_entrywise_gpu.py)."""
    from neural_renderer_amd import frontend
    case = ('fan', cname, variant, ts, True, True, 'host')
    inp = F.case_inputs(case)
    fw, adj = reference(case)
    state = {}

    def fused(r, v, f, t, colors):
        L, G = (lambda x: lay(x, state['layout'])), (lambda y: grad_as(y, state['grad']))
        for n in ('eye', 'K', 't', 'dist_coeffs'):
            if torch.is_tensor(getattr(r, n, None)):
                setattr(r, n, L(getattr(r, n)))
        if torch.is_tensor(r.R):
            r.R = L(r.R.transpose(-1, -2)).transpose(-1, -2) if state['layout'] == 'permuted' else L(r.R)
        v, f, t = L(v), L(f), L(t)
        assert frontend.fusable(r, v, f, t) and (not colors or frontend.light_fusable(r))
        faces, second = frontend.project_and_light_colors(r, v, f) if colors else frontend.project_and_light(r, v, f, t)
        return G(faces), G(second)

    def run(layout, grad):
        state.update(layout=layout, grad=grad)
        return run_module(inp, fused, torch.float32, 'cuda')
    outs0, grads0 = run('plain', 'contiguous')
    assert all(np.abs(g).sum() > 0 for g in grads0.values()) and sorted(grads0) == sorted(adj)
    runs = [(name, 'contiguous') for name in FLOAT_LAYOUTS + ('int64',)] + [('plain', name) for name in FLOAT_LAYOUTS]
    worst = 0.0
    for layout, grad in runs + [('offset4', 'offset4')]:
        outs, grads = run(layout, grad)
        for key in outs0:
            assert outs[key].tobytes() == outs0[key].tobytes(), (layout, grad, key)
        for key, got in grads.items():
            if key == 'textures':
                assert got.tobytes() == grads0[key].tobytes(), (layout, grad, key)
                continue
            ref, M, n = adj[key]
            ratio = F.worst_ratio(got, ref, M, n, CONSTANTS[key])
            worst = max(worst, ratio)
            assert ratio <= 1, (layout, grad, key, ratio)
    print('front-end %s %s: worst fraction of the entrywise bound over the layouts %.3f' % (cname, variant, worst))


# ---------------------------------------------------------------------------------------------------------------------
# vertices_to_faces, lights, vertex colours

def _v2f_case():
    import neural_renderer_amd as nr
    rng = np.random.default_rng(3)
    v, f = _sphere()
    inputs = {'vertices': rng.normal(size=(B,) + v.shape).astype(np.float32), 'faces': np.repeat(f[None], B, axis=0)}
    return Case(inputs, lambda t, L, G: {'faces': G(nr.vertices_to_faces(L(t['vertices']), L(t['faces'])))}, integer=True,
                layouts=FLOAT_LAYOUTS + ('int64', 'expanded'))


def test_vertices_to_faces():
    """The gather is exact; the scatter adds float atomics in arrival order, so the upstream gradients are small integers:
    every partial sum is exact and the bits do not depend on the order."""
    check_layouts(_v2f_case(), 'vertices_to_faces')


def _lights_case(smooth, per_image=True):
    import neural_renderer_amd as nr
    rng = np.random.default_rng(11)
    v, f = _sphere()
    n = (B,) if per_image else ()
    inputs = {'vertices': (v[None] + rng.normal(scale=0.05, size=(B,) + v.shape)).astype(np.float32),
              'faces': np.repeat(f[None], B, axis=0),
              'intensity_ambient': rng.uniform(0.2, 0.6, n).astype(np.float32),
              'intensity_directional': rng.uniform(0.3, 0.8, n).astype(np.float32),
              'color_ambient': rng.uniform(0.5, 1.0, n + (3,)).astype(np.float32),
              'color_directional': rng.uniform(0.5, 1.0, n + (3,)).astype(np.float32),
              'direction': rng.normal(size=n + (3,)).astype(np.float32),
              'sh': rng.normal(scale=0.2, size=n + (9, 3)).astype(np.float32)}

    lights = nr.Lights(sh=torch.zeros(9, 3)).cuda()   # (built once: the call itself uploads nothing)

    def call(t, L, G):
        for name in nr.lights.NAMES:
            setattr(lights, name, L(t[name]))
        return {'light': G(nr.light_colors(L(t['vertices']), L(t['faces']), lights, fill_back=True, smooth=smooth,
                                           implementation='hip'))}
    return Case(inputs, call, layouts=FLOAT_LAYOUTS + ('int64', 'expanded'))


@pytest.mark.parametrize('smooth', [False, True], ids=['flat', 'smooth'])
def test_light_colors(smooth):
    """nr.light_colors with SH coefficients: the six parameters one per image and shared, in every layout (0-dim and [B]
    intensities included)."""
    for per_image in (True, False):
        check_layouts(_lights_case(smooth, per_image), 'light_colors smooth=%d per_image=%d' % (smooth, per_image))


def _shade_case(smooth, batched_colors):
    import neural_renderer_amd as nr
    rng = np.random.default_rng(13)
    v, f = _sphere()
    inputs = {'vertices': (v[None] + rng.normal(scale=0.05, size=(B,) + v.shape)).astype(np.float32),
              'faces': np.repeat(f[None], B, axis=0),
              'colors': rng.uniform(0, 1, ((B,) if batched_colors else ()) + (v.shape[0], 3)).astype(np.float32)}

    def call(t, L, G):
        cc = nr.vertex_shade(L(t['vertices']), L(t['faces']), L(t['colors']), 0.4, 0.6, (1.0, 0.9, 0.8), (0.7, 1.0, 0.6),
                             (0.3, 0.8, -0.5), fill_back=True, smooth=smooth, implementation='hip')
        return {'corner': G(cc.colors)}
    return Case(inputs, call, layouts=FLOAT_LAYOUTS + ('int64', 'expanded'))


@pytest.mark.parametrize('smooth', [False, True], ids=['flat', 'smooth'])
def test_vertex_shade(smooth):
    """nr.vertex_shade with colours [Nv,3] and [B,Nv,3]."""
    for batched in (False, True):
        check_layouts(_shade_case(smooth, batched), 'vertex_shade smooth=%d colours per image=%d' % (smooth, batched))


def test_renderer_vertex_colors_and_lights():
    """The Renderer's remaining dispatches, once each: VertexColors with smooth shading, and `lights` with shared cubes."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(17)
    v, f = _sphere()
    base = {'vertices': (v[None] + rng.normal(scale=0.02, size=(B,) + v.shape)).astype(np.float32),
            'faces': np.repeat(f[None], B, axis=0),
            'eye': np.asarray([nr.get_points_from_angles(2.732, 20.0 + 10 * i, 40.0 * i) for i in range(B)], np.float32)}

    def renderer(t, L):
        r = nr.Renderer()
        r.image_size, r.eye = 16, L(t['eye'])
        return r

    def call_vc(t, L, G):
        r = renderer(t, L)
        r.shading = 'smooth'
        return {'rgb': G(r.render(L(t['vertices']), L(t['faces']), nr.VertexColors(L(t['colors']))))}

    def call_lights(t, L, G):
        r = renderer(t, L)
        r.lights = nr.Lights().cuda()
        r.lights.sh = L(t['sh'])
        return {'rgb': G(r.render(L(t['vertices']), L(t['faces']), L(t['textures'])))}
    order = dict({n: 'order' for n in ('eye', 'colors', 'textures', 'sh')}, vertices='close')
    covered = lambda o: (o['rgb'].abs().sum(1) > 0).float()
    check_layouts(Case(dict(base, colors=rng.uniform(0.2, 1, (v.shape[0], 3)).astype(np.float32)), call_vc, kinds=order,
                       covered=covered, layouts=FLOAT_LAYOUTS + ('int64',)), 'Renderer.render VertexColors smooth')
    check_layouts(Case(dict(base, textures=rng.uniform(0.2, 1, (1, f.shape[0], 2, 2, 2, 3)).astype(np.float32),
                            sh=rng.normal(scale=0.2, size=(9, 3)).astype(np.float32)), call_lights, kinds=order,
                       covered=covered, layouts=FLOAT_LAYOUTS + ('int64',)), 'Renderer.render lights, shared cubes')


# ---------------------------------------------------------------------------------------------------------------------
# UV bake, mesh losses, subdivision

def _bake_case(ts):
    import neural_renderer_amd as nr
    rng = np.random.default_rng(19 + ts)
    sizes = [(3, 5), (7, 9)]   # 15 + 63 pixels: neither image's rows nor the packing's second image sit on the grid
    uv, face_image, base = uv_ref.random_layout(rng, NF, ts, sizes)
    layout = nr.UVLayout(uv, face_image, base, sizes)
    inputs = {'image0': rng.uniform(0, 1, (B, 3, 3, 5)).astype(np.float32),
              'image1': rng.uniform(0, 1, (3, 7, 9)).astype(np.float32)}

    def call(t, L, G):
        images = [L(t['image0']).permute(0, 2, 3, 1), L(t['image1']).permute(1, 2, 0)]   # batched and shared
        return {'textures': G(nr.bake_uv_textures(images, layout))}
    return Case(inputs, call)


@pytest.mark.parametrize('ts', [2, 3])
def test_bake_uv_textures(ts):
    """Images [Bi,3,H,W].permute(0,2,3,1) and a shared [3,H,W].permute(1,2,0).  Both gradients are the inverse map's gather,
    the shared image's summed over the batch by torch from one and the same packing: bits."""
    check_layouts(_bake_case(ts), 'bake_uv_textures ts=%d' % ts)


def _mesh_loss_case(which, squeeze=False):
    import neural_renderer_amd as nr
    rng = np.random.default_rng(23)
    v, f = _sphere()
    vb = (v[None] + rng.normal(scale=0.05, size=(B,) + v.shape)).astype(np.float32)
    inputs = {'vertices': vb[0] if squeeze else vb, 'faces': f if squeeze else np.repeat(f[None], B, axis=0)}
    fn = nr.laplacian_loss if which == 'laplacian' else nr.flatness_loss
    return Case(inputs, lambda t, L, G: {'loss': G(fn(L(t['vertices']), L(t['faces']), implementation='hip'))},
                layouts=FLOAT_LAYOUTS + ('int64', 'expanded'))


@pytest.mark.parametrize('which', ['laplacian', 'flatness'])
def test_mesh_losses(which):
    """Vertices [B,Nv,3] and [Nv,3]; grad_loss in every layout and as the expanded gradient of loss.sum()."""
    check_layouts(_mesh_loss_case(which), which + '_loss')
    check_layouts(_mesh_loss_case(which, squeeze=True), which + '_loss, one mesh')


@pytest.mark.parametrize('C', [3, 5])
@pytest.mark.parametrize('levels', [1, 2])
def test_subdivide(levels, C):
    """nr.subdivide on the icosahedron (a Subdivision plan's __call__ underneath), Loop and midpoint."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(29)
    _, f = _sphere(0)
    for scheme in ('loop', 'midpoint'):
        inputs = {'x': rng.normal(size=(B, 12, C)).astype(np.float32), 'faces': np.repeat(f[None], B, axis=0)}

        def call(t, L, G):
            out, faces = nr.subdivide(L(t['x']), L(t['faces']), levels=levels, scheme=scheme, implementation='hip')
            assert faces.shape == (B, 20 * 4 ** levels, 3)
            return {'x': G(out), 'faces': faces.contiguous()}
        check_layouts(Case(inputs, call, layouts=FLOAT_LAYOUTS + ('int64', 'expanded')),
                      'subdivide %s levels=%d C=%d' % (scheme, levels, C))


# ---------------------------------------------------------------------------------------------------------------------
# Adam

ADAM_SIZES = (1, 255, 257, 1027)   # under, at and over one block of 256, and several blocks


def _adam(kind, steps=5):
    """Five steps of nr.Adam on parameters that are offset4 views of one flat buffer.  kind: how the gradients arrive."""
    import neural_renderer_amd as nr
    from oracle import oracle as O
    rng = np.random.default_rng(31)
    p0 = [rng.normal(size=n).astype(np.float32) for n in ADAM_SIZES]
    total = sum(ADAM_SIZES)
    flat = torch.zeros(total + 1, device='cuda')
    assert flat.data_ptr() % 16 == 0
    params, at = [], 1
    for p in p0:
        view = flat[at:at + p.size]
        view.copy_(torch.tensor(p))
        params.append(view.requires_grad_())
        at += p.size
    assert all(p.is_contiguous() for p in params) and params[0].data_ptr() % 16 == 4
    assert {p.data_ptr() % 16 for p in params} != {0}
    params[1].lr = 0.25
    opt = nr.Adam(params, alpha=0.01, beta1=0.5)
    ref = [p.copy() for p in p0]
    oracle = O.Adam(alpha=0.01, beta1=0.5)
    for _ in range(steps):
        if kind == 'sum':
            grads = [np.ones_like(p) for p in p0]
            # (autograd.grad hands the expanded scalar over as it is; .backward() would let AccumulateGrad copy it)
            for p, g in zip(params, torch.autograd.grad(sum(p.sum() for p in params), params)):
                assert g.stride() == (0,) or g.numel() == 1
                p.grad = g
        else:
            grads = [rng.normal(size=p.shape).astype(np.float32) for p in p0]
            for g in grads:
                g[rng.uniform(size=g.shape) < 0.4] = 0
            if kind == 'bucket':
                bucket = torch.zeros(total + 1, device='cuda')
                at = 1
                for p, g in zip(params, grads):
                    p.grad = bucket[at:at + g.size]
                    p.grad.copy_(torch.tensor(g))
                    at += g.size
                assert params[0].grad.data_ptr() % 16 == 4
            else:
                for p, g in zip(params, grads):
                    p.grad = lay(torch.tensor(g, device='cuda'), 'strided')
                    assert p.grad.numel() < 2 or not p.grad.is_contiguous()
        opt.step()
        oracle.update(ref, grads, lr_mult=[1.0, 0.25, 1.0, 1.0])
    assert float(flat[0]) == 0   # nothing in front of the first parameter was touched
    return [_host(p) for p in params], ref


@pytest.mark.parametrize('kind', ['bucket', 'strided', 'sum'])
def test_adam_on_views_of_a_flat_buffer(kind):
    """k_adam_update reads and writes one float per thread (csrc/nr_optim.hip), so parameters and gradients 4 bytes off the
    grid go to it as they are: bit for bit O.Adam, as test_optimizer.py asks of aligned ones."""
    got, ref = _adam(kind)
    for a, b in zip(got, ref):
        assert np.abs(a - b).max() == 0 and np.abs(b).sum() > 0


def test_adam_non_contiguous_parameter_takes_the_torch_path():
    import neural_renderer_amd as nr
    from oracle import oracle as O
    rng = np.random.default_rng(37)
    p0 = rng.normal(size=(257,)).astype(np.float32)
    wide = torch.zeros(257, 2, device='cuda')
    wide[:, 0] = torch.tensor(p0)
    p = wide[:, 0].requires_grad_()
    assert not p.is_contiguous()
    opt = nr.Adam([p], alpha=0.01, beta1=0.5)
    ref, oracle = [p0.copy()], O.Adam(alpha=0.01, beta1=0.5)
    for _ in range(5):
        g = rng.normal(size=p0.shape).astype(np.float32)
        g[rng.uniform(size=g.shape) < 0.4] = 0
        p.grad = torch.tensor(g, device='cuda')
        opt.step()
        oracle.update(ref, [g])
    np.testing.assert_allclose(_host(p), ref[0], rtol=1e-6, atol=1e-7)   # test_optimizer.py's tolerance for the torch path
    assert float(wide[:, 1].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the kept forward workspace through the operator

def _cycle_scenes(S):
    """The four scenes of test_hip_parity.test_kept_workspace_epochs_equal_the_filling_forward, B = 2, F = 60, and their
    per-call-fill maps from the C ABI (flags = 0)."""
    rng = np.random.default_rng(77)
    scenes = []
    for k in range(4):
        f = H.random_scene(rng, 2, 60, size=0.2 + 0.2 * k)
        f[:, 0, :, :2] *= 6.0   # a face with a large screen box: goes through the queues
        scenes.append(f)
    tex = rng.uniform(0, 1, (2, 60, 2, 2, 2, 3)).astype(np.float32)
    ref = [abi.forward_fused(f, tex, S, 0.1, 100.0, 1e-3, (0.2, 0.3, 0.4), 0, True, True, True) for f in scenes]
    ref = [tuple(r[k].clone() for k in ('rgb_map', 'alpha_map', 'depth_map')) for r in ref]
    return [_cuda(f) for f in scenes], _cuda(tex), ref


def _rasterize_module():
    import importlib
    return importlib.import_module('neural_renderer_amd.rasterize')   # (the package attribute of that name is the function)


def _entries(S, stream=None):
    R = _rasterize_module()
    return [e for k, e in R._ZBUF_CACHE.items() if k[2:5] == (2, 60, S) and (stream is None or k[1] == stream)]


def test_workspace_cache_cycle_through_the_operator():
    """The Python bookkeeping of the kept z-buffer (rasterize._forward_workspace) over more than one cycle of 255 epochs:
    every call's maps equal the per-call-fill maps bit for bit, the counter wraps through -1 back to 254, a second shape
    keeps its own counter, the 17th key evicts the first (which is then refilled), and a side stream has its own entry."""
    import neural_renderer_amd as nr
    R = _rasterize_module()
    scenes, tex, ref = _cycle_scenes(32)
    scenes48, _, ref48 = _cycle_scenes(48)
    nr.clear_workspace_cache()
    fn = nr.Rasterize(32, 0.1, 100, 1e-3, (0.2, 0.3, 0.4), True, True, True)
    fn48 = nr.Rasterize(48, 0.1, 100, 1e-3, (0.2, 0.3, 0.4), True, True, True)

    def same(got, want, what):
        for name, a, b in zip(('rgb', 'alpha', 'depth'), got, want):
            assert torch.equal(a, b), '%s: %s' % (what, name)
    assert bool((ref[0][1] == 1).any()) and bool((ref[0][1] == 0).any())
    calls48 = 0
    for call in range(300):
        same(fn(scenes[call % 4], tex), ref[call % 4], 'call %d' % call)
        ent, = _entries(32)
        # the counter holds the NEXT epoch: 254 after the fill, 253 after the first call, ..., -1 after the 255th (epoch 0),
        # and the 256th call refills
        assert ent[1] == 253 - call % 255, (call, ent[1])
        if call % 7 == 6:
            same(fn48(scenes48[calls48 % 4], tex), ref48[calls48 % 4], 'S=48 call %d' % calls48)
            calls48 += 1
            ent48, = _entries(48)
            assert ent48[1] == 253 - (calls48 - 1) % 255 and ent48[0] is not ent[0]
    assert call == 299 and _entries(32)[0][1] == 253 - 299 % 255 == 209 and calls48 == 42
    # 17 distinct keys (rasterize._forward_workspace keeps 16): the least recently used goes first
    same(fn48(scenes48[0], tex), ref48[0], 'S=48 again')
    first = _entries(32)[0]
    others = [nr.Rasterize(S, 0.1, 100, 1e-3, (0, 0, 0), False, True, False) for S in range(9, 9 + 2 * 15, 2)]
    assert len(R._ZBUF_CACHE) == 2
    same(fn(scenes[0], tex), ref[0], 'S=32 before the other keys')   # S = 48 is now the oldest, S = 32 the second oldest
    for o in others[:14]:
        o(scenes[1])
    assert len(R._ZBUF_CACHE) == 16 and _entries(32) and _entries(48)
    others[14](scenes[1])     # the 17th key: S = 48 goes
    assert len(R._ZBUF_CACHE) == 16 and not _entries(48) and _entries(32)[0] is first
    fn48(scenes48[1], tex)    # the 18th: S = 32 goes
    assert len(R._ZBUF_CACHE) == 16 and not _entries(32)
    same(fn(scenes[1], tex), ref[1], 'S=32 after its eviction')
    ent, = _entries(32)
    assert ent is not first and ent[1] == 253   # a new entry, filled, one epoch handed out
    same(fn(scenes[2], tex), ref[2], 'S=32, second call after its eviction')
    # a side stream: its own key, the default stream's bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for call in range(20):
            same(fn(scenes[call % 4], tex), ref[call % 4], 'side stream call %d' % call)
    side.synchronize()
    mine = _entries(32, stream=int(side.cuda_stream))
    assert len(mine) == 1 and mine[0] is not ent and mine[0][1] == 253 - 19 and len(_entries(32)) == 2
    nr.clear_workspace_cache()


# ---------------------------------------------------------------------------------------------------------------------
# streams

def _producer():
    """A few milliseconds of dependent work on the current stream."""
    x = torch.ones(1 << 26, device='cuda')
    for _ in range(48):
        x = x * 1.0001 + 1e-3
    return x


def _on_side_stream(case, what):
    """The case's forward and backward on a side stream whose inputs are still being written when the operator is enqueued:
    zeros first (valid, degenerate data for a read that does not wait), the values behind a producer of >= 1 ms."""
    staged = case.leaves()
    # (the reference run on the staged tensors also leaves the index tensor's range verdict and host-built tables behind,
    # cached on the tensor object: the run on the stream then reads nothing back, and no launch waits for the host)
    ref = case.run(leaves=staged)
    case.nontrivial(ref, what)
    bufs = {n: (torch.zeros_like(x).requires_grad_(x.requires_grad) if x.is_floating_point() else x) for n, x in staged.items()}
    side = torch.cuda.Stream()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        start.record()
        keep = _producer()
        stop.record()
        with torch.no_grad():
            for n in bufs:
                if bufs[n] is not staged[n]:
                    bufs[n].copy_(staged[n])
        got = case.run(leaves=bufs)
        pending = not stop.query()
    side.synchronize()
    ms = start.elapsed_time(stop)
    print('%s: producer %.2f ms, still running after forward and backward were enqueued: %s' % (what, ms, pending))
    assert ms >= 1.0, 'the producer took %.2f ms: the operator may have been enqueued after its inputs were ready' % ms
    del keep
    case.compare(got, ref, what + ' on a side stream')


STREAM_CASES = {
    'rasterizer': lambda: _raster_case(32, 2, False, True),
    'front_end': lambda: _renderer_case('projection', 'render_rgbad'),
    'lights': lambda: _lights_case(True),
    'vertex_colours': lambda: _shade_case(True, True),
    'uv_bake': lambda: _bake_case(2),
    'uv_per_pixel': lambda: _raster_case(32, 2, False, True, source='uv', smooth=True),
    'laplacian_loss': lambda: _mesh_loss_case('laplacian'),
    'flatness_loss': lambda: _mesh_loss_case('flatness'),
    'vertices_to_faces': _v2f_case,
}


@pytest.mark.parametrize('family', sorted(STREAM_CASES))
def test_side_stream(family):
    _on_side_stream(STREAM_CASES[family](), family)


def test_side_stream_subdivision():
    import neural_renderer_amd as nr
    rng = np.random.default_rng(41)
    _, f = _sphere(0)
    inputs = {'x': rng.normal(size=(B, 12, 3)).astype(np.float32)}
    plan = nr.subdivision(_cuda(f), 12, levels=2)   # (the plan is built on the host from the indices: ahead of the stream)
    _on_side_stream(Case(inputs, lambda t, L, G: {'x': G(plan(L(t['x']), implementation='hip'))}), 'Subdivision.__call__')


def test_uv_inverse_map_built_on_one_stream_and_read_on_another():
    """UVLayout.inverse_map is built by a kernel on the stream of the first backward and kept on the layout.  Here that
    first backward runs on a side stream behind a producer, and the default stream asks for the same layout's gradient at
    once, without any synchronisation of the caller's: it has to wait for the build (uv_textures.py records an event), and
    both calls give the gradient of a layout whose map was built in order.  (The tables start as zeros, so a read that did
    not wait would see empty rows -- a zero gradient, not stale indices.)"""
    ref = _bake_case(2).run()
    case = _bake_case(2)             # the same layout as another object: nothing of it is on the device yet
    case.nontrivial(ref, 'bake_uv_textures')
    staged = case.leaves()
    with torch.no_grad():            # a forward alone uploads the layout's host tables and does not build the inverse map
        warm = case.call(staged, lambda x: x, lambda y: y)
    case._weights('textures', warm['textures'])
    side = torch.cuda.Stream()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        start.record()
        keep = _producer()
        stop.record()
        first = case.run(leaves=staged)
    second = case.run(leaves=staged)
    pending = not stop.query()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop)
    print('inverse map: producer %.2f ms, still running after both calls were enqueued: %s' % (ms, pending))
    assert ms >= 1.0
    del keep
    case.compare(first, ref, 'the call that builds the inverse map, on a side stream')
    case.compare(second, ref, 'the call on the default stream right behind it')


def test_side_stream_adam():
    """nr.Adam on a side stream behind a producer: parameters and gradients are written there, and stepped at once."""
    import neural_renderer_amd as nr
    rng = np.random.default_rng(43)
    p0 = rng.normal(size=(1027,)).astype(np.float32)
    g0 = rng.normal(size=(1027,)).astype(np.float32)

    def step(p, g):
        p.grad = g
        nr.Adam([p], alpha=0.01, beta1=0.5).step()
    ref = _cuda(p0, True)
    step(ref, _cuda(g0))
    assert not torch.equal(ref.detach(), _cuda(p0))
    sp, sg = _cuda(p0), _cuda(g0)
    p, g = torch.zeros(1027, device='cuda', requires_grad=True), torch.zeros(1027, device='cuda')
    side = torch.cuda.Stream()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        start.record()
        keep = _producer()
        stop.record()
        with torch.no_grad():
            p.copy_(sp)
            g.copy_(sg)
        step(p, g)
    side.synchronize()
    assert start.elapsed_time(stop) >= 1.0
    del keep
    assert torch.equal(p.detach(), ref.detach())
