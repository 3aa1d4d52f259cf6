"""ctypes binding of libnr_hip.so (include/nr_hip.h).  The product path has NO fallback: if the HIP
library is missing or an entry point fails, this raises."""
import ctypes
import os

import torch

from . import _build

_CONTIGUOUS = torch.contiguous_format

_c = ctypes
_vp, _i32, _f64, _sz = _c.c_void_p, _c.c_int32, _c.c_double, _c.c_size_t


class Camera(_c.Structure):
    """struct nr_camera (include/nr_hip.h)."""
    _fields_ = [('mode', _i32), ('perspective', _i32), ('target', _c.c_float * 3), ('up', _c.c_float * 3),
                ('width', _c.c_float)]


class Light(_c.Structure):
    """struct nr_light (include/nr_hip.h)."""
    _fields_ = [('intensity_ambient', _c.c_float), ('intensity_directional', _c.c_float),
                ('color_ambient', _c.c_float * 3), ('color_directional', _c.c_float * 3), ('direction', _c.c_float * 3)]


class FaceLight(_c.Structure):
    """struct nr_face_light (include/nr_hip.h): per-face light colours for the _lit entry points."""
    _fields_ = [('light', _vp), ('texture_faces', _i32), ('textures', _vp), ('grad_light', _vp)]


class CornerLight(_c.Structure):
    """struct nr_corner_light (include/nr_hip.h): a light colour per corner for the _uv_smooth entry points."""
    _fields_ = [('light', _vp), ('texture_faces', _i32), ('grad_light', _vp)]


class Projection(_c.Structure):
    """struct nr_projection (include/nr_hip.h): device pointers of K, R, t, dist_coeffs (or None) and their layouts."""
    _fields_ = [('K', _vp), ('R', _vp), ('t', _vp), ('dist_coeffs', _vp), ('K_per_batch', _i32), ('R_per_batch', _i32),
                ('t_per_batch', _i32), ('dist_per_batch', _i32), ('orig_size', _c.c_float)]


class UVImagesStruct(_c.Structure):
    """struct nr_uv_images (include/nr_hip.h): a UV layout's device tables and its packed images."""
    _fields_ = [('images', _vp), ('image_table', _vp), ('faces_uv', _vp), ('face_image', _vp), ('base', _vp),
                ('texture_size', _i32), ('num_images', _i32), ('num_pixels', _i32), ('image_batch', _i32)]


class Lights(_c.Structure):
    """struct nr_lights (include/nr_hip.h): device pointers of the six light parameters (sh or None) and their layouts."""
    _fields_ = [('intensity_ambient', _vp), ('intensity_directional', _vp), ('color_ambient', _vp),
                ('color_directional', _vp), ('direction', _vp), ('sh', _vp), ('per_image', _i32)]


class LightsGrad(_c.Structure):
    """struct nr_lights_grad (include/nr_hip.h): where each parameter's gradient goes (None = not needed)."""
    _fields_ = [('intensity_ambient', _vp), ('intensity_directional', _vp), ('color_ambient', _vp),
                ('color_directional', _vp), ('direction', _vp), ('sh', _vp)]


_cam_p, _light_p, _fl_p, _proj_p = _c.POINTER(Camera), _c.POINTER(Light), _c.POINTER(FaceLight), _c.POINTER(Projection)
_uv_p, _cl_p = _c.POINTER(UVImagesStruct), _c.POINTER(CornerLight)
_lights_p, _lights_grad_p = _c.POINTER(Lights), _c.POINTER(LightsGrad)

# name -> (restype, argtypes); mirrors include/nr_hip.h one to one
SIGNATURES = {
    'nr_version': (_c.c_int, []),
    'nr_error_string': (_c.c_char_p, [_c.c_int]),
    'nr_forward_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'nr_backward_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32, _i32]),
    'nr_forward_face_index_map': (_c.c_int, [_vp] * 6 + [_i32, _i32, _i32, _f64, _f64, _vp, _sz, _vp]),
    'nr_forward_texture_sampling': (_c.c_int, [_vp] * 10 + [_i32, _vp, _i32, _i32, _i32, _i32, _f64, _i32, _vp]),
    'nr_backward_pixel_map': (_c.c_int, [_vp] * 7 + [_i32, _i32, _i32, _f64, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    'nr_backward_textures': (_c.c_int, [_vp] * 9 + [_i32, _i32, _i32, _i32, _f64, _i32, _vp]),
    'nr_backward_depth_map': (_c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    'nr_forward_rasterize': (_c.c_int, [_vp] * 10 + [_i32] * 5 + [_f64] * 3 + [_i32, _vp, _sz, _vp]),
    'nr_vertices_to_faces': (_c.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    'nr_vertices_to_faces_backward': (_c.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    'nr_backward_rasterize': (_c.c_int, [_vp] * 12 + [_i32] * 4 + [_f64, _i32, _vp, _vp, _sz, _vp]),
    'nr_image_epilogue': (_c.c_int, [_vp] * 6 + [_i32] * 3 + [_vp]),
    'nr_image_epilogue_backward': (_c.c_int, [_vp] * 6 + [_i32] * 3 + [_vp]),
    'nr_load_textures': (_c.c_int, [_vp] * 4 + [_i32] * 4 + [_vp]),
    'nr_create_texture_image': (_c.c_int, [_vp] * 3 + [_i32] * 5 + [_vp]),
    'nr_bake_uv_textures': (_c.c_int, [_vp] * 6 + [_i32] * 5 + [_vp]),
    'nr_uv_texture_map_workspace_bytes': (_sz, [_i32] * 4),
    'nr_uv_texture_map': (_c.c_int, [_vp] * 6 + [_i32] * 4 + [_vp, _sz, _vp]),
    'nr_bake_uv_textures_backward': (_c.c_int, [_vp] * 5 + [_i32] * 4 + [_vp]),
    'nr_forward_rasterize_uv': (_c.c_int, [_fl_p, _uv_p] + [_vp] * 8 + [_i32] * 4 + [_f64] * 3 + [_i32, _vp, _sz, _vp]),
    'nr_backward_uv_images_workspace_bytes': (_sz, [_i32] * 4),
    'nr_backward_uv_images': (_c.c_int, [_fl_p, _uv_p] + [_vp] * 6 + [_i32] * 3 + [_f64, _vp, _sz, _vp]),
    'nr_forward_rasterize_uv_smooth': (_c.c_int, [_cl_p, _uv_p] + [_vp] * 8 + [_i32] * 4 + [_f64] * 3 + [_i32, _vp, _sz, _vp]),
    'nr_backward_uv_images_smooth_workspace_bytes': (_sz, [_i32] * 4),
    'nr_backward_uv_images_smooth': (_c.c_int, [_cl_p, _uv_p] + [_vp] * 6 + [_i32] * 3 + [_f64, _vp, _sz, _vp]),
    'nr_forward_rasterize_corner': (_c.c_int, [_vp] * 9 + [_i32] * 4 + [_f64] * 2 + [_i32, _vp, _sz, _vp]),
    'nr_backward_corner_colors_workspace_bytes': (_sz, [_i32] * 2),
    'nr_backward_corner_colors': (_c.c_int, [_vp] * 7 + [_i32] * 3 + [_vp, _sz, _vp]),
    'nr_vertex_shade_workspace_bytes': (_sz, [_i32] * 2),
    'nr_vertex_shade_forward': (_c.c_int, [_vp] * 6 + [_i32] * 7 + [_light_p, _vp, _sz, _vp]),
    'nr_vertex_shade_backward': (_c.c_int, [_vp] * 8 + [_i32] * 7 + [_light_p, _vp, _sz, _vp]),
    'nr_normals_workspace_bytes': (_sz, [_i32] * 3),
    'nr_vertex_normals_forward': (_c.c_int, [_vp] * 5 + [_i32] * 4 + [_vp]),
    'nr_vertex_normals_backward': (_c.c_int, [_vp] * 6 + [_i32] * 4 + [_vp, _sz, _vp]),
    'nr_face_normals_forward': (_c.c_int, [_vp] * 3 + [_i32] * 4 + [_vp]),
    'nr_face_normals_backward': (_c.c_int, [_vp] * 6 + [_i32] * 4 + [_vp, _sz, _vp]),
    'nr_corner_normals_forward': (_c.c_int, [_vp] * 5 + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_corner_normals_backward': (_c.c_int, [_vp] * 6 + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_soft_silhouette_workspace_bytes': (_sz, [_i32] * 3),
    'nr_soft_silhouette_forward': (_c.c_int, [_vp] * 3 + [_i32] * 3 + [_f64] * 3 + [_vp, _sz, _vp]),
    'nr_soft_silhouette_backward': (_c.c_int, [_vp] * 4 + [_i32] * 3 + [_f64] * 3 + [_vp, _sz, _vp]),
    'nr_soft_render_workspace_bytes': (_sz, [_i32] * 3),
    'nr_soft_render_forward': (_c.c_int, [_vp] * 5 + [_i32] * 4 + [_f64] * 8 + [_vp, _sz, _vp]),
    'nr_soft_render_backward': (_c.c_int, [_vp] * 8 + [_i32] * 4 + [_f64] * 8 + [_vp, _sz, _vp]),
    'nr_soft_corners_workspace_bytes': (_sz, [_i32] * 3),
    'nr_soft_corners_forward': (_c.c_int, [_vp] * 5 + [_i32] * 4 + [_f64] * 8 + [_vp, _sz, _vp]),
    'nr_soft_corners_backward': (_c.c_int, [_vp] * 8 + [_i32] * 4 + [_f64] * 8 + [_vp, _sz, _vp]),
    'nr_soft_uv_workspace_bytes': (_sz, [_uv_p] + [_i32] * 3),
    'nr_soft_uv_forward': (_c.c_int, [_uv_p] + [_vp] * 5 + [_i32] * 4 + [_f64] * 8 + [_vp, _sz, _vp]),
    'nr_soft_uv_backward': (_c.c_int, [_uv_p] + [_vp] * 9 + [_i32] * 4 + [_f64] * 8 + [_vp, _sz, _vp]),
    'nr_soft_cubes_workspace_bytes': (_sz, [_i32] * 5),
    'nr_soft_cubes_forward': (_c.c_int, [_vp] * 6 + [_i32] * 6 + [_f64] * 9 + [_vp, _sz, _vp]),
    'nr_soft_cubes_backward': (_c.c_int, [_vp] * 10 + [_i32] * 6 + [_f64] * 9 + [_vp, _sz, _vp]),
    'nr_mesh_loss_workspace_bytes': (_sz, [_i32] * 2),
    'nr_laplacian_forward': (_c.c_int, [_vp] * 5 + [_i32] * 3 + [_vp, _sz, _vp]),
    'nr_laplacian_backward': (_c.c_int, [_vp] * 5 + [_i32] * 3 + [_vp]),
    'nr_flatness_forward': (_c.c_int, [_vp] * 3 + [_i32] * 3 + [_f64, _vp, _sz, _vp]),
    'nr_flatness_backward': (_c.c_int, [_vp] * 6 + [_i32] * 3 + [_f64, _vp]),
    'nr_edge_length_forward': (_c.c_int, [_vp] * 4 + [_i32] * 4 + [_f64, _vp, _sz, _vp]),
    'nr_edge_length_backward': (_c.c_int, [_vp] * 7 + [_i32] * 5 + [_f64, _vp]),
    'nr_cot_weights': (_c.c_int, [_vp] * 3 + [_i32] * 3 + [_f64, _vp]),
    'nr_cot_apply': (_c.c_int, [_vp] * 8 + [_i32] * 3 + [_vp, _sz, _vp]),
    'nr_point_mesh_workspace_bytes': (_sz, [_i32] * 5),
    'nr_point_mesh_points_to_faces': (_c.c_int, [_vp] * 6 + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_point_mesh_faces_to_points': (_c.c_int, [_vp] * 6 + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_point_mesh_loss': (_c.c_int, [_vp] * 3 + [_i32] * 3 + [_f64] * 2 + [_vp]),
    'nr_point_mesh_backward_points': (_c.c_int, [_vp] * 12 + [_i32] * 4 + [_vp]),
    'nr_point_mesh_backward_vertices': (_c.c_int, [_vp] * 14 + [_i32] * 5 + [_vp]),
    'nr_winding_workspace_bytes': (_sz, [_i32] * 5),
    'nr_winding_forward': (_c.c_int, [_vp] * 4 + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_winding_backward_points': (_c.c_int, [_vp] * 5 + [_i32] * 5 + [_vp, _sz, _vp]),
    'nr_winding_backward_vertices': (_c.c_int, [_vp] * 7 + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_ray_mesh_workspace_bytes': (_sz, [_i32] * 5),
    'nr_ray_mesh_first_hit': (_c.c_int, [_vp] * 7 + [_i32] * 5 + [_f64] * 2 + [_i32] * 2 + [_vp, _sz, _vp]),
    'nr_ray_mesh_any_hit': (_c.c_int, [_vp] * 5 + [_i32] * 5 + [_f64] * 2 + [_i32] * 2 + [_vp, _sz, _vp]),
    'nr_isosurface_workspace_bytes': (_sz, [_i32] * 5),
    'nr_isosurface_count': (_c.c_int, [_vp] * 2 + [_i32] * 4 + [_f64] + [_i32] * 2 + [_vp, _sz, _vp]),
    'nr_isosurface_emit': (_c.c_int, [_vp] * 2 + [_sz] * 2 + [_i32] * 5 + [_vp, _sz, _vp]),
    'nr_light_colors_workspace_bytes': (_sz, [_i32] * 4),
    'nr_light_colors_forward': (_c.c_int, [_vp] * 4 + [_lights_p, _vp] + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_light_colors_backward': (_c.c_int, [_vp] * 4 + [_lights_p, _vp, _vp, _lights_grad_p] + [_i32] * 6 + [_vp, _sz, _vp]),
    'nr_image_loss_workspace_bytes': (_sz, [_i32] * 4),
    'nr_iou_loss_forward': (_c.c_int, [_vp, _vp, _i32, _vp, _vp, _vp] + [_i32] * 4 + [_f64, _vp, _sz, _vp]),
    'nr_iou_loss_backward': (_c.c_int, [_vp, _i32] + [_vp] * 4 + [_i32] * 4 + [_f64, _vp]),
    'nr_squared_error_forward': (_c.c_int, [_vp] * 3 + [_i32] * 2 + [_vp] * 2 + [_i32] * 5 + [_vp, _sz, _vp]),
    'nr_squared_error_backward': (_c.c_int, [_vp] * 3 + [_i32] * 2 + [_vp] * 3 + [_i32] * 5 + [_vp]),
    'nr_ssim_workspace_bytes': (_sz, [_i32] * 5),
    'nr_ssim_loss_forward': (_c.c_int, [_vp] * 3 + [_i32] * 2 + [_vp] * 5 + [_i32] * 7 + [_f64] * 2 + [_vp, _sz, _vp]),
    'nr_ssim_loss_backward': (_c.c_int, [_vp] * 3 + [_i32] * 2 + [_vp] * 5 + [_i32] * 6 + [_vp]),
    'nr_stencil_apply': (_c.c_int, [_vp] * 5 + [_i32] * 5 + [_vp]),
    'nr_adam_update': (_c.c_int, [_vp] * 4 + [_sz] + [_c.c_float] * 4 + [_vp]),
    'nr_frontend_workspace_bytes': (_sz, [_i32]),
    'nr_frontend_forward': (_c.c_int, [_vp] * 6 + [_i32] * 7 + [_cam_p, _light_p, _vp]),
    'nr_frontend_backward': (_c.c_int, [_vp] * 9 + [_i32] * 7 + [_cam_p, _light_p, _vp, _sz, _vp]),
    'nr_forward_rasterize_lit': (_c.c_int, [_fl_p] + [_vp] * 10 + [_i32] * 5 + [_f64] * 3 + [_i32, _vp, _sz, _vp]),
    'nr_backward_rasterize_lit': (_c.c_int, [_fl_p] + [_vp] * 12 + [_i32] * 4 + [_f64, _i32, _vp, _vp, _sz, _vp]),
    'nr_backward_textures_shared_workspace_bytes': (_sz, [_i32] * 3),
    'nr_backward_textures_shared': (_c.c_int, [_fl_p] + [_vp] * 8 + [_i32] * 4 + [_f64, _i32, _vp, _sz, _vp]),
    'nr_frontend_forward_light': (_c.c_int, [_vp] * 5 + [_i32] * 6 + [_cam_p, _light_p, _vp]),
    'nr_frontend_backward_light': (_c.c_int, [_vp] * 7 + [_i32] * 6 + [_cam_p, _light_p, _vp, _sz, _vp]),
    'nr_frontend_projection_workspace_bytes': (_sz, [_i32]),
    'nr_frontend_forward_projection': (_c.c_int, [_vp] * 6 + [_i32] * 6 + [_proj_p, _light_p, _vp]),
    'nr_frontend_backward_projection': (_c.c_int, [_vp] * 11 + [_i32] * 6 + [_proj_p, _light_p, _vp, _sz, _vp]),
}

NR_VERSION = 600  # include/nr_hip.h; load() refuses a library of another version (a stale build)
NR_FLAG_FIX_TEXTURE_BATCH_Z = 1
NR_FLAG_EXACT_GRADIENT = 2
NR_FLAG_K6_GLOBAL = 4
NR_FLAG_K6_SCAN = 8
NR_FLAG_ZBUF_EPOCH = 16  # + epoch number << 8 (include/nr_hip.h)
NR_FLAG_SPARSE_WEIGHT_MAP = 32
NR_FLAG_SERIAL_BACKWARD = 64
NR_FLAG_K6_LEGACY = 128
NR_FLAG_SHARED_TEXTURES = 131072  # one set of cubes for the batch (forward; nr_backward_textures_shared)
NR_FLAG_K6_PX = 65536  # (accepted and ignored since 0.6.0; bits 8..15 of a forward's flags carry the epoch number)
NR_E_INDEX = -6
NR_CAMERA_LOOK_AT = 1
NR_CAMERA_LOOK = 2
NR_CAMERA_PROJECTION = 3

_lib = None


class NRError(RuntimeError):
    pass


def load():
    """Load (never build implicitly at import on a GPU box: the .so ships in-tree; build() exists for that)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get('NR_HIP_LIB') or _build.LIB_PATH  # NR_HIP_LIB: a variant build (development timing runs)
    if not os.path.exists(path):
        raise NRError('%s not found: build it with `python -m neural_renderer_amd._build` '
                      '(or __graft_entry__.build()); there is no CPU/eager fallback.' % path)
    lib = _c.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.nr_version() != NR_VERSION and not os.environ.get('NR_HIP_LIB'):  # (a development variant: the caller's business)
        raise NRError('%s is version %d, this package binds version %d: rebuild it (python -m neural_renderer_amd._build)'
                      % (path, lib.nr_version(), NR_VERSION))
    _lib = lib
    return lib


# the measurement build's extra exports (include/nr_hip_profile.h)
PROFILE_SIGNATURES = {
    'nr_profile_band_kernel': (_c.c_int, [_i32]),
    'nr_profile_band_kernel_ms': (_c.c_float, []),
    'nr_profile_band_kernel_which': (_c.c_int, []),
    'nr_profile_k6_choice': (_c.c_int, [_i32, _i32, _i32, _i32, _i32, _c.c_double, _i32]),
    'nr_profile_backward_plan': (_c.c_int, [_i32] * 7 + [_f64] + [_i32] * 5 + [_sz, _c.POINTER(_c.c_int64)]),
}
NR_PLAN_FIELDS = 35  # include/nr_hip_profile.h
_profile_lib = None


def load_profile():
    """libnr_hip_prof.so -- the product's sources with the band-kernel timing hook compiled in -- for measurements only
    (bench.py's roofline, the hook's test).  The product path never loads it."""
    global _profile_lib
    if _profile_lib is None:
        path = _build.PROFILE_LIB_PATH
        if not os.path.exists(path):
            raise NRError('%s not found: build it with neural_renderer_amd._build.build_profile()' % path)
        lib = _c.CDLL(path)
        for name, (res, args) in list(SIGNATURES.items()) + list(PROFILE_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.nr_version() != NR_VERSION:
            raise NRError('%s is version %d, this package binds version %d: rebuild it' % (path, lib.nr_version(), NR_VERSION))
        _profile_lib = lib
    return _profile_lib


def check(code, what):
    if code != 0:
        msg = load().nr_error_string(code)
        text = '%s failed (%d): %s' % (what, code, msg.decode() if msg else '?')
        if code == NR_E_INDEX:
            raise IndexError(text)
        raise NRError(text)


def ptr(t):
    """data_ptr of a tensor or None."""
    return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device):
    """hipStream_t of torch's current stream on `device` (the raw query: no Stream object per call)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(device.index)
    return torch.cuda.current_stream(device).cuda_stream


class _NoGuard(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on_device(device):
    """Context that makes `device` the current HIP device for the launches -- nothing at all when it already is (one process
    per GPU: always), torch.cuda.device otherwise."""
    return _NO_GUARD if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def workspace_bytes(name, *sizes):
    """What the host-only size query `name` (an nr_*_workspace_bytes entry) answers for `sizes`."""
    return getattr(load(), name)(*sizes)


def launch(name, device, *args, workspace_bytes=None):
    """Call entry point `name` for tensors on `device`: makes `device` current for the call (no guard when it already is), passes
    torch's current stream on it as the last argument, raises through check().  The entry is looked up on the loaded library
    at every call (tests and tools replace its attributes).  workspace_bytes None: the entry has no workspace parameters.
    An int (0 allowed): a fresh uint8 workspace of max(bytes, 1) on `device`, allocated inside the guard and alive until
    the call returns, passed as (pointer, bytes) in front of the stream -- include/nr_hip.h's trailing convention."""
    with on_device(device):
        fn = getattr(load(), name)
        if workspace_bytes is None:
            check(fn(*args, stream_ptr(device)), name)
        else:
            ws = torch.empty((max(workspace_bytes, 1),), dtype=torch.uint8, device=device)
            check(fn(*args, ws.data_ptr(), workspace_bytes, stream_ptr(device)), name)


def dense(t):
    """The tensor boundary: `t` itself when it is contiguous and starts on a 16-byte boundary -- what
    include/nr_hip.h asks of every buffer, because the kernels move maps, textures and workspaces as 16-byte words --, else a
    contiguous copy that does (torch's allocators align fresh storage to 64 bytes and more).  None stays None.  A view that
    is contiguous but starts 4, 8 or 12 bytes off the grid (a slice of a flat parameter vector, a gradient-bucket view)
    is returned unchanged by .contiguous(): hence the clone."""
    if t is None:
        return None
    if not t.is_contiguous():
        t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=_CONTIGUOUS)
