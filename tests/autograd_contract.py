"""The autograd contract of every torch.autograd.Function of the package: the registry of calls (ROWS) and the helpers that
tests/test_autograd_contract_gpu.py (the properties P1 .. P7 on the device) and tests/test_autograd_contract.py (completeness,
the static form of P7, and _WindingTorch on the CPU) run over it.

The values of these operators are held elsewhere: float64 restatements with counted bounds, the oracle, layouts, streams.
Here one call is made in more than one way THROUGH AUTOGRAD -- a second backward over a retained graph, .grad accumulation,
every subset of inputs that ask for a gradient and of outputs that receive one, two forwards before one backward, one image's
upstream gradient zeroed, a second derivative -- and the results are compared with the plain call's.  No tolerance is added:
the comparison kinds are those of tests/test_layout_invariance_gpu.py (its docstring: bits | ints | order | close), through
that file's Case.compare, and every row names the existing GPU test that holds its plain call to a restatement (`pinned`)
or brings the family's own check function (`check`), so that an equality here carries that verdict over to the variant.

A row: name; the Function classes whose nodes its call records; build() -> a fresh layout-invariance Case (named inputs, the
call, the kinds); `shared`: the inputs without a batch axis of the row's B images (index tensors of one topology, cubes or
images shared by the batch); `vary`: the input in which the two forwards of P5 differ (None: only their upstream gradients
differ) -- the eye, the cloud, the target, or the scene beside shared cubes; `upstream`: output name -> the upstream gradient
of the pinned test where that is a fixed array.  Every case has B >= 2 images that differ, and upstream gradients that
differ per image.

The _FrontEnd rows run under Renderer.render_rgbad, as the layout file's test_renderer does, with that test's kinds (vertices
`close`, cameras `order`); the `entry` kind belongs to the front-end called directly through test_frontend_ref.run_module,
which builds its own leaves and has no place for a second backward or a second forward, so it is not used here.

What a forward leaves on ctx besides saved_tensors is listed per class in CTX, by attribute name; `Row.ctx` is the union over
the row's classes.  P1 clones the tensors found there (inside tuples and on the attributes of the objects kept there: the
residual record's fields, a UVLayout's tables, a subdivision level's) and compares their bits after a backward."""
import importlib
import importlib.machinery
import pkgutil
import types
import weakref

import numpy as np
import torch

import test_layout_invariance_gpu as LI
from test_layout_invariance_gpu import Case

# ---------------------------------------------------------------------------------------------------------------------
# the classes

# the node that refuses a second derivative (neural_renderer_amd/_util.py): part of the mechanism under test, no operator
MECHANISM = ('_SecondDerivative',)

# class -> what its forward leaves on ctx besides saved_tensors (attribute names; the plain numbers and flags beside them --
# meta, dims, params, sizes, eps, weights, ... -- hold no tensor)
CTX = {
    '_RasterizeFunction': ('z_ref', 'visible', 'cfg', 'source'), '_GraphedRasterizeFunction': ('entry',), '_ImageEpilogue': (),
    '_FrontEnd': ('params',), '_VerticesToFaces': (), '_LightColors': ('setup',), '_VertexShade': ('setup',),
    '_BakeUV': ('layout',), '_VertexNormals': ('setup',), '_FaceNormals': ('setup',), '_CornerNormals': ('setup',),
    '_ApplyLevel': ('level',), '_LaplacianLoss': ('tables',), '_FlatnessLoss': ('tables',),
    '_EdgeLengthLoss': ('tables', 'target'), '_CotangentLaplacianLoss': ('adj',), '_IoULoss': (), '_SquaredError': (),
    '_SSIMLoss': (), '_SoftSilhouettes': ('args',), '_SoftRender': ('args',), '_SoftRenderUV': ('uv', 'args'),
    '_SoftRenderCubes': ('args',), '_PointMesh': ('tables',), '_LossSum': (), '_Winding': ('tables',), '_WindingTorch': (),
}


def package_functions():
    """name -> class of every torch.autograd.Function subclass defined in neural_renderer_amd (MECHANISM left out)."""
    import neural_renderer_amd as nr
    found = {}
    for info in pkgutil.iter_modules(nr.__path__):
        spec = info.module_finder.find_spec('neural_renderer_amd.' + info.name)
        if not isinstance(spec.loader, importlib.machinery.SourceFileLoader):   # (the built libraries lie beside the modules)
            continue
        module = importlib.import_module('neural_renderer_amd.' + info.name)
        for obj in vars(module).values():
            if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj.__module__ == module.__name__ \
                    and obj.__name__ not in MECHANISM:
                found[obj.__name__] = obj
    return found


# ---------------------------------------------------------------------------------------------------------------------
# rows

class Row(object):
    def __init__(self, name, classes, build, pinned, check=None, shared=(), vary=None, upstream=None, gpu=True, raster=False):
        self.name, self.classes, self.build, self.pinned, self.check = name, tuple(classes), build, pinned, check
        self.shared, self.vary, self.upstream, self.gpu, self.raster = tuple(shared), vary, upstream, gpu, raster

    @property
    def ctx(self):
        return tuple(sorted({a for c in self.classes for a in CTX[c]}))

    def case(self, inputs=None):
        """A fresh Case (its own table of upstream gradients and of worst errors); `inputs` replaces the arrays."""
        case = self.build()
        if inputs is not None:
            case.inputs = inputs
        for key, g in (self.upstream() if self.upstream else {}).items():
            case.upstream[key] = LI._cuda(np.asarray(g, np.float32))
        return case

    def __repr__(self):
        return self.name


def _flip(a):
    """The images of a batch in the reverse order: another valid scene / eye / cloud / target for every image but the middle
    one of an odd batch (the rows with B = 3 keep that one -- its two forwards then differ by the upstream gradient only)."""
    return np.ascontiguousarray(a[::-1])


def _raster(S, ts, shared, lit, source='cubes', smooth=False):
    return lambda: LI._raster_case(S, ts, shared, lit, source=source, smooth=smooth)


def _check_cubes_against_the_oracle():
    """The rasterizer family's check function (the oracle's forward and backward, entry by entry) on the scene of the row
    raster_cubes."""
    from test_hip_parity import check_backward
    inputs = LI._raster_case(32, 2, False, False).inputs
    check_backward(inputs['faces'], inputs['textures'], 32, 1e-3, (True, True, True), 5, ts_bg=(0.2, 0.3, 0.4))


def _rgbad(aa):
    def build():
        import neural_renderer_amd as nr
        S = 32
        rng = np.random.default_rng(40 + S)   # test_layout_invariance_gpu.test_rasterize_rgbad's scene, with face_light
        inputs = {'faces': LI.H.random_scene(rng, LI.B, LI.NF, size=0.4),
                  'textures': rng.uniform(0, 1, (LI.B, LI.NF, 2, 2, 2, 3)).astype(np.float32),
                  'light': rng.uniform(0.2, 1.2, (LI.B, LI.NF, 3)).astype(np.float32)}

        def call(t, L, G):
            out = nr.rasterize_rgbad(L(t['faces']), L(t['textures']), S // 2 if aa else S, aa, 0.1, 100, 1e-3, (0.2, 0.3, 0.4),
                                     face_light=L(t['light']))
            return {k: G(out[k]) for k in ('rgb', 'alpha', 'depth')}
        return Case(inputs, call, kinds={'faces': 'order', 'light': 'order'}, covered=lambda o: (o['alpha'] == 1).float())
    return build


def _normals(op):
    def build():
        import normals_ref
        from test_normals_gpu import _ops
        v, f = normals_ref.batch('icosphere1', 3)
        fn = _ops(((True, True),))[{'vertex': 'vertex', 'face': 'face', 'corner': 'corner-smooth-fill_back'}[op]]
        return Case({'vertices': v, 'faces': f}, lambda t, L, G: {'normals': G(fn(L(t['vertices']), L(t['faces'])))})
    return build


def _subdivide():
    import neural_renderer_amd as nr
    rng = np.random.default_rng(29)   # test_layout_invariance_gpu.test_subdivide: two Loop levels of the icosahedron, C = 3
    _, f = LI._sphere(0)
    inputs = {'x': rng.normal(size=(LI.B, 12, 3)).astype(np.float32), 'faces': np.repeat(f[None], LI.B, axis=0)}

    def call(t, L, G):
        out, faces = nr.subdivide(L(t['x']), L(t['faces']), levels=2, scheme='loop', implementation='hip')
        return {'x': G(out), 'faces': faces.contiguous()}
    return Case(inputs, call)


def _edge(kind, form):
    def build():
        import mesh_edge_ref as E
        import mesh_loss_ref as R
        from test_mesh_edge_losses_gpu import _fn
        seed = 1 if kind == 'edge' else 0
        v, f = R.inputs('blocks', seed)   # 648 vertices: three blocks of 256 per image, the last one partly filled
        inputs, fixed = {'vertices': v, 'faces': f}, ()
        target = E.target('blocks', seed, form) if kind == 'edge' else None
        if isinstance(target, np.ndarray):
            inputs['target'], fixed = target, ('target',)

        def call(t, L, G):
            kw = {} if kind == 'cot' else {'target': L(t['target']) if 'target' in t else target}
            return {'loss': G(_fn(kind)(L(t['vertices']), L(t['faces']), implementation='hip', **kw))}
        return Case(inputs, call, fixed=fixed)
    return build


def _mesh_upstream():
    import mesh_loss_ref as R
    return {'loss': R.UPSTREAM}


IOU_CASE = (40, 72, 3, 'soft', False, 3)          # image_loss_ref.BIG: six workgroups per image, partly filled
SE_CASE = (40, 72, 3, 3, False, 'per', 3)
SSIM_CASE = (40, 72, 7, 'same', 0, 'noise', False, 'per', 'sum', 3)


def _iou():
    import image_loss_ref as R
    from neural_renderer_amd import image_losses as IL
    assert IOU_CASE in R.iou_cases()
    alpha, target, weights = R.iou_inputs(IOU_CASE)
    return Case({'alpha': alpha, 'target': target}, lambda t, L, G: {'loss': G(IL.silhouette_iou_loss(
        L(t['alpha']), L(t['target']), levels=len(weights), level_weights=weights, eps=R.EPS, implementation='hip'))},
        fixed=('target',))


def _se():
    import image_loss_ref as R
    from neural_renderer_amd import image_losses as IL
    assert SE_CASE in R.se_cases()
    x, target, mask, weights = R.se_inputs(SE_CASE)
    return Case({'images': x, 'target': target, 'mask': mask}, lambda t, L, G: {'loss': G(IL.squared_error_loss(
        L(t['images']), L(t['target']), L(t['mask']), levels=len(weights), level_weights=weights, implementation='hip'))},
        fixed=('target', 'mask'))


def _ssim():
    import ssim_ref as R
    from neural_renderer_amd import image_losses as IL
    assert SSIM_CASE in R.cases()
    x, target, mask = R.inputs(SSIM_CASE)
    return Case({'images': x, 'target': target, 'mask': mask}, lambda t, L, G: {'loss': G(IL.ssim_loss(
        L(t['images']), L(t['target']), L(t['mask']), window_size=SSIM_CASE[2], padding=SSIM_CASE[3], reduction=SSIM_CASE[8],
        implementation='hip'))}, fixed=('target', 'mask'))


def _image_upstream():
    import image_loss_ref as R
    return {'loss': R.UPSTREAM}


# in the CASES of all four soft colour files (soft cubes: with ts = 2); 80 faces that reach every pixel
SOFT = ('ico1', 3, 16, 1.0, 1e-1)


def _soft_silhouettes():
    import neural_renderer_amd as nr
    from test_soft_silhouettes_gpu import _reference
    faces, _, _ = _reference('ico1', 3, 16, 1.0)
    return Case({'faces': faces},
                lambda t, L, G: {'alpha': G(nr.soft_silhouettes(L(t['faces']), 16, 1.0, implementation='hip'))})


def _soft_render(corners):
    def build():
        import neural_renderer_amd as nr
        import test_soft_corners_gpu
        import test_soft_render_gpu
        G0 = test_soft_corners_gpu if corners else test_soft_render_gpu
        faces, colors, _ = G0.reference(*SOFT)
        return Case({'faces': faces, 'colors': colors}, lambda t, L, G: {'rgba': G(nr.soft_render(
            L(t['faces']), L(t['colors']), SOFT[2], SOFT[3], SOFT[4], background_color=G0.BG, implementation='hip'))})
    return build


def _soft_cubes():
    import neural_renderer_amd as nr
    import test_soft_cubes_gpu as G0
    faces, textures, light, _ = G0.reference(*(SOFT + (2,)))   # B = 3: the cubes are shared by the batch
    return Case({'faces': faces, 'textures': textures, 'light': light}, lambda t, L, G: {'rgba': G(nr.soft_render_cubes(
        L(t['faces']), L(t['textures']), L(t['light']), SOFT[2], SOFT[3], SOFT[4], background_color=G0.BG, texture_eps=1e-3,
        implementation='hip'))})


def _soft_uv():
    import neural_renderer_amd as nr
    import test_soft_uv_gpu as G0
    faces, args, images, light, _ = G0.reference(*SOFT)        # B = 3: the four images are shared by the batch
    layout = nr.UVLayout(*args)
    inputs = dict({'faces': faces, 'light': light}, **{'image%d' % k: im for k, im in enumerate(images)})

    def call(t, L, G):
        uv = nr.UVImages(layout, [L(t['image%d' % k]) for k in range(len(images))])
        return {'rgba': G(nr.soft_render_uv(L(t['faces']), uv, L(t['light']), SOFT[2], SOFT[3], SOFT[4],
                                            background_color=G0.BG, implementation='hip'))}
    return Case(inputs, call)


def _soft_upstream(module, *more):
    """The pinned test's upstream gradient: the restatement's .g, 0 on its masked pixels."""
    def get():
        return {'rgba': importlib.import_module(module).reference(*(SOFT + more))[-1].g}
    return get


def _point_mesh_both():
    """_PointMesh.apply with both directions in one node (the public functions ask for one each; point_mesh_distance('both')
    hides the two distances behind _LossSum): the distances, both differentiable."""
    from neural_renderer_amd import point_mesh as PM
    from test_point_mesh import case
    points, vertices, faces = case(2)   # (3, 257, 65): more than a tile of points, a face count that is no multiple of a wave

    def call(t, L, G):
        p, v, f, _, hip = PM._inputs('closest_surface_points', L(t['points']), L(t['vertices']), L(t['faces']), 'hip')
        out = PM._PointMesh.apply(p, v, f, True, True, PM._SPLIT)
        return {'dist2_points': G(out[0]), 'dist2_faces': G(out[3]), 'face_ids': out[1], 'point_ids': out[4]}
    return Case({'points': points, 'vertices': vertices, 'faces': faces}, call)


def _check_point_mesh_both():
    """The family's check function on the same arrays, and the node with both directions against the two public calls."""
    import neural_renderer_amd as nr
    from test_point_mesh import case, check_case
    points, vertices, faces = case(2)
    check_case(points, vertices, faces, device='cuda', implementation='hip', what='autograd contract, point_mesh_both')
    c = _point_mesh_both()
    t = c.leaves()
    outs = c.call(t, lambda x: x, lambda y: y)
    ds = nr.closest_surface_points(t['points'], t['vertices'], t['faces'], 'hip')
    dc = nr.closest_cloud_points(t['points'], t['vertices'], t['faces'], 'hip')
    assert torch.equal(outs['dist2_points'], ds[0]) and torch.equal(outs['dist2_faces'], dc[0])
    assert torch.equal(outs['face_ids'].long(), ds[1]) and torch.equal(outs['point_ids'].long(), dc[1])


def _point_mesh_loss():
    import neural_renderer_amd as nr
    from test_point_mesh import case
    points, vertices, faces = case(1)   # (2, 63, 255)
    return Case({'points': points, 'vertices': vertices, 'faces': faces}, lambda t, L, G: {'loss': G(nr.point_mesh_distance(
        L(t['points']), L(t['vertices']), L(t['faces']), 'both', 'mean', 'hip'))})


def winding_arrays():
    from test_winding import case
    # (3, 513, 515): a batched cloud, more points than a workgroup's, more faces than two tiles, both with a rest
    return case(4)


def _winding():
    import neural_renderer_amd as nr
    points, vertices, faces = winding_arrays()
    return Case({'points': points, 'vertices': vertices, 'faces': faces}, lambda t, L, G: {'w': G(nr.winding_number(
        L(t['points']), L(t['vertices']), L(t['faces']), 'hip'))})


_RASTER = ('_RasterizeFunction',)
_RENDER = ('_FrontEnd', '_RasterizeFunction', '_ImageEpilogue')
_LAYOUT = 'tests/test_layout_invariance_gpu.py::'

ROWS = [
    # the rasterizer called directly, rgb + alpha + depth, one row per shading source (the scenes of the layout file; its
    # kinds: grad_faces `order`, per-image cubes of ts = 2 `bits`, what double atomics sum `order`)
    Row('raster_cubes', _RASTER, _raster(32, 2, False, False), 'tests/test_hip_parity.py::test_texture_size_paths',
        check=_check_cubes_against_the_oracle, vary=('faces', _flip), raster=True),
    Row('raster_cubes_shared', _RASTER, _raster(30, 2, True, False),
        'tests/test_shared_textures_gpu.py::test_shared_cubes_equal_the_expanded_call', shared=('textures',),
        vary=('faces', _flip), raster=True),
    Row('raster_cubes_face_light', _RASTER, _raster(30, 2, False, True),
        'tests/test_face_light_gpu.py::test_face_light_against_the_oracle', vary=('faces', _flip), raster=True),
    Row('raster_uv_flat', _RASTER, _raster(32, 2, False, True, 'uv', False), 'tests/test_uv_pixel_gpu.py::test_adjoint',
        vary=('faces', _flip), raster=True),
    Row('raster_uv_smooth', _RASTER, _raster(30, 2, False, True, 'uv', True), 'tests/test_uv_smooth_gpu.py::test_adjoint',
        vary=('faces', _flip), raster=True),
    Row('raster_corner_colors', _RASTER, _raster(30, 2, False, True, 'corner'),
        'tests/test_vertex_colors_gpu.py::test_adjoint', vary=('faces', _flip), raster=True),
    # the public wrapper: the epilogue behind the rasterizer
    Row('rgbad_aa', _RASTER + ('_ImageEpilogue',), _rgbad(True),
        'tests/test_hip_parity.py::test_public_api_rasterize_rgbad_matches_oracle', vary=('faces', _flip)),
    Row('rgbad_no_aa', _RASTER + ('_ImageEpilogue',), _rgbad(False),
        'tests/test_hip_parity.py::test_public_api_rasterize_rgbad_matches_oracle', vary=('faces', _flip)),
    # the fused front-end under Renderer.render_rgbad, one row per camera mode (vertices `close`, cameras `order`)
    Row('frontend_look_at', _RENDER, lambda: LI._renderer_case('look_at', 'render_rgbad'),
        'tests/test_frontend_entrywise_gpu.py::test_kernels_against_the_restatement', vary=('eye', _flip)),
    Row('frontend_look', _RENDER, lambda: LI._renderer_case('look', 'render_rgbad'),
        'tests/test_frontend_entrywise_gpu.py::test_kernels_against_the_restatement', vary=('eye', _flip)),
    Row('frontend_projection', _RENDER, lambda: LI._renderer_case('projection', 'render_rgbad'),
        'tests/test_frontend_entrywise_gpu.py::test_kernels_against_the_restatement', vary=('t', _flip)),
    Row('vertices_to_faces', ('_VerticesToFaces',), LI._v2f_case,
        'tests/test_hip_parity.py::test_vertices_to_faces_gather_and_atomic_scatter'),
    Row('light_colors', ('_LightColors',), lambda: LI._lights_case(True),
        'tests/test_lights_gpu.py::test_kernels_against_the_restatement', vary=('direction', _flip)),
    Row('vertex_shade', ('_VertexShade',), lambda: LI._shade_case(True, True),
        'tests/test_vertex_colors_gpu.py::test_backward_against_adjoint_and_finite_differences', vary=('colors', _flip)),
    Row('bake_uv', ('_BakeUV',), lambda: LI._bake_case(2), 'tests/test_uv_textures_gpu.py::test_fuzz_forward_and_adjoint',
        shared=('image1',)),
    Row('vertex_normals', ('_VertexNormals',), _normals('vertex'),
        'tests/test_normals_gpu.py::test_forward_and_backward_within_the_derived_bounds[icosphere1-B3]', shared=('faces',)),
    Row('face_normals', ('_FaceNormals',), _normals('face'),
        'tests/test_normals_gpu.py::test_forward_and_backward_within_the_derived_bounds[icosphere1-B3]', shared=('faces',)),
    Row('corner_normals', ('_CornerNormals',), _normals('corner'),
        'tests/test_normals_gpu.py::test_forward_and_backward_within_the_derived_bounds[icosphere1-B3]', shared=('faces',)),
    Row('subdivide', ('_ApplyLevel',), _subdivide, 'tests/test_subdivision_gpu.py::test_hip_against_the_float64_restatement'),
    Row('laplacian_loss', ('_LaplacianLoss',), lambda: LI._mesh_loss_case('laplacian'),
        'tests/test_mesh_losses_gpu.py::test_against_the_float64_restatement'),
    Row('flatness_loss', ('_FlatnessLoss',), lambda: LI._mesh_loss_case('flatness'),
        'tests/test_mesh_losses_gpu.py::test_against_the_float64_restatement'),
    Row('edge_length_number', ('_EdgeLengthLoss',), _edge('edge', 'number'),
        'tests/test_mesh_edge_losses_gpu.py::test_every_target_form[blocks-number]', shared=('faces',),
        upstream=_mesh_upstream),
    Row('edge_length_per_image_target', ('_EdgeLengthLoss',), _edge('edge', 'BE'),
        'tests/test_mesh_edge_losses_gpu.py::test_every_target_form[blocks-BE]', shared=('faces',), vary=('target', _flip),
        upstream=_mesh_upstream),
    Row('cotangent_laplacian', ('_CotangentLaplacianLoss',), _edge('cot', 'zero'),
        'tests/test_mesh_edge_losses_gpu.py::test_against_the_float64_restatement[cot-blocks]', shared=('faces',),
        upstream=_mesh_upstream),
    Row('iou_loss', ('_IoULoss',), _iou, 'tests/test_image_losses_gpu.py::test_against_the_float64_restatement[iou]',
        vary=('target', _flip), upstream=_image_upstream),
    Row('squared_error', ('_SquaredError',), _se, 'tests/test_image_losses_gpu.py::test_against_the_float64_restatement[se]',
        vary=('target', _flip), upstream=_image_upstream),
    Row('ssim_loss', ('_SSIMLoss',), _ssim, 'tests/test_ssim_gpu.py::test_against_the_float64_restatement',
        vary=('target', _flip), upstream=_image_upstream),
    Row('soft_silhouettes', ('_SoftSilhouettes',), _soft_silhouettes,
        'tests/test_soft_silhouettes_gpu.py::test_forward_and_gradient_within_the_derived_bounds[ico1-B3-S16-sigma1]',
        vary=('faces', _flip), upstream=lambda: {'alpha': importlib.import_module('test_soft_silhouettes_gpu')._reference(
            'ico1', 3, 16, 1.0)[1]}),
    Row('soft_render', ('_SoftRender',), _soft_render(False),
        'tests/test_soft_render_gpu.py::test_forward_and_gradients_within_the_derived_bounds[ico1-B3-S16-sigma1-gamma0.1]',
        vary=('faces', _flip), upstream=_soft_upstream('test_soft_render_gpu')),
    Row('soft_render_corner_colors', ('_SoftRender',), _soft_render(True),
        'tests/test_soft_corners_gpu.py::test_forward_and_gradients_within_the_derived_bounds[ico1-B3-S16-sigma1-gamma0.1]',
        vary=('faces', _flip), upstream=_soft_upstream('test_soft_corners_gpu')),
    Row('soft_render_uv', ('_SoftRenderUV',), _soft_uv,
        'tests/test_soft_uv_gpu.py::test_forward_and_gradients_within_the_derived_bounds[ico1-B3-S16-sigma1-gamma0.1]',
        shared=('image0', 'image1', 'image2', 'image3'), vary=('faces', _flip), upstream=_soft_upstream('test_soft_uv_gpu')),
    Row('soft_render_cubes', ('_SoftRenderCubes',), _soft_cubes,
        'tests/test_soft_cubes_gpu.py::test_forward_and_gradients_within_the_derived_bounds[ico1-B3-S16-sigma1-gamma0.1-ts2]',
        shared=('textures',), vary=('faces', _flip), upstream=_soft_upstream('test_soft_cubes_gpu', 2)),
    Row('point_mesh_both', ('_PointMesh',), _point_mesh_both,
        'tests/test_point_mesh_gpu.py::test_kernels_against_the_float64_restatement[2]', check=_check_point_mesh_both,
        shared=('faces',), vary=('points', _flip)),
    Row('point_mesh_loss', ('_PointMesh', '_LossSum'), _point_mesh_loss,
        'tests/test_point_mesh_gpu.py::test_loss_against_the_float64_restatement[mean-both]', shared=('faces',),
        vary=('points', _flip)),
    Row('winding_number', ('_Winding',), _winding,
        'tests/test_winding_gpu.py::test_kernels_against_the_float64_restatement[4]', shared=('faces',),
        vary=('points', _flip)),
    # not run on the device by the contract's file: the replayed operator is documented to raise when a second forward comes
    # before the backward, and nothing there captures a graph (tests/test_hip_parity.py::test_graph_replay_equals_the_eager_
    # operator holds it); the plain-torch winding path runs on the CPU in tests/test_autograd_contract.py
    Row('graphed_rasterize', ('_GraphedRasterizeFunction',), None,
        'tests/test_hip_parity.py::test_graph_replay_equals_the_eager_operator', gpu=False),
    Row('winding_torch', ('_WindingTorch',), None, 'tests/test_winding.py::test_torch_path_against_the_float64_restatement',
        gpu=False),
]

GPU_ROWS = [r for r in ROWS if r.gpu]


# ---------------------------------------------------------------------------------------------------------------------
# helpers

def ident(x):
    return x


def bits(t):
    """t's bits as integers: equality that holds for NaN payloads and tells -0.0 from 0.0 (a residual may be an uninitialised
    map of which only the covered pixels are stored)."""
    t = t.detach()
    if t.is_floating_point():
        t = t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t.clone()


def tensors_in(obj, depth=2):
    """The tensors in obj: a tensor, a tuple / list / dict of them, or the attributes of an object (one level: a residual
    record, a UVLayout, a subdivision level)."""
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, (tuple, list)):
        return [t for x in obj for t in tensors_in(x, depth)]
    if isinstance(obj, dict):
        return [t for x in obj.values() for t in tensors_in(x, depth)]
    plain = (type, types.FunctionType, types.MethodType, weakref.ref)
    if depth > 0 and hasattr(obj, '__dict__') and not isinstance(obj, plain):
        return [t for x in vars(obj).values() for t in tensors_in(x, depth - 1)]
    return []


def package_nodes(outputs):
    """The backward nodes of the package's Functions reachable from `outputs` (tensors)."""
    names = {c + 'Backward' for c in CTX}
    seen, todo, found = set(), [o.grad_fn for o in outputs if o is not None and o.grad_fn is not None], []
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if type(node).__name__ in names:
            found.append(node)
        todo.extend(n for n, _ in node.next_functions)
    return found


def residuals(row, outputs):
    """[(what, tensor)]: every saved tensor and every tensor under the row's ctx attributes, of every package node."""
    out = []
    for node in package_nodes(outputs):
        name = type(node).__name__
        out += [('%s.saved_tensors[%d]' % (name, i), t) for i, t in enumerate(node.saved_tensors) if t is not None]
        for attr in row.ctx:
            out += [('%s.%s[%d]' % (name, attr, i), t) for i, t in enumerate(tensors_in(getattr(node, attr, None)))]
    return out


def diff_outputs(outs):
    return [(k, o) for k, o in outs.items() if torch.is_tensor(o) and o.is_floating_point() and o.requires_grad]


def loss_of(case, outs, only=None, explicit_zeros=False, zero_image=None, second=False):
    """sum_k (out_k * w_k).sum() over the differentiable outputs.  only: the outputs that receive a gradient -- the others are
    left out, or (explicit_zeros) take part with a gradient of exact zeros; zero_image: that image's upstream gradient is
    exact zeros; second: the other set of upstream gradients (P5's second forward: the images' in reverse order)."""
    total = None
    for k, o in diff_outputs(outs):
        w = case._weights(k, o)
        if second:
            w = w.flip(0)
        if only is not None and k not in only:
            if not explicit_zeros:
                continue
            w = torch.zeros_like(w)
        if zero_image is not None:
            w = w.clone()
            w[zero_image] = 0
        term = (o * w).sum()
        total = term if total is None else total + term
    return total


def leaves_of(case, want=None):
    """The case's leaves; want: the names that ask for a gradient (default: every float input that is not fixed)."""
    t = case.leaves()
    if want is not None:
        for n, x in t.items():
            if x.requires_grad and n not in want:
                x.requires_grad_(False)
    return t


def names_of(t):
    return [n for n, x in t.items() if x.requires_grad]


def forward(case, t):
    return case.call(t, ident, ident)


def gradients(case, want=None, **loss_kw):
    """One plain call -> (outputs detached, gradients by input name)."""
    t = leaves_of(case, want)
    outs = forward(case, t)
    names = names_of(t)
    grads = torch.autograd.grad(loss_of(case, outs, **loss_kw), [t[n] for n in names], allow_unused=True) if names else ()
    return ({k: (o.detach() if torch.is_tensor(o) else o) for k, o in outs.items()},
            {n: g for n, g in zip(names, grads) if g is not None})


def same(case, name, got, ref, what):
    """got against ref by the kind of the gradient `name` (Case.compare: bits | order | close, the worst error kept)."""
    assert got is not None and ref is not None, '%s: gradient of %s is missing' % (what, name)
    case.compare(({}, {name: got}), ({}, {name: ref}), what)


def same_outputs(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), '%s: output %s' % (what, k)


def report(case, what):
    kinds = sorted({case.kinds.get(n, case.kind) for n, a in case.inputs.items()
                    if a.dtype.kind == 'f' and n not in case.fixed})
    worst = ', '.join('%s %.3g (bound %.3g)' % (k, v, LI.SAME_TERMS if k == 'order' else LI.GRAD_TOL)
                      for k, v in sorted(case.worst.items()))
    print('%s: kinds %s%s; worst %s' % (what, '+'.join(kinds), ' (integer upstream)' if case.integer else '', worst or '-'))
