"""Fused geometry + lighting front-end of `Renderer.render*` (reference neural_renderer/renderer.py:35-107).

`project_and_light(renderer, vertices, faces, textures)` produces what the reference computes with
fill_back -> vertices_to_faces -> lighting -> look_at / look -> perspective -> vertices_to_faces, i.e. the rasterizer's
inputs `faces [B, F, 3, 3]` and lit `textures [B, F, ts, ts, ts, 3]`, with ONE HIP kernel per direction
(`nr_frontend_forward` / `nr_frontend_backward`, csrc/nr_frontend.hip) instead of ~60 + ~100 small torch launches.
Gradients reach `vertices`, `textures` and a learnable camera position `eye` (example4).

camera_mode = 'projection' (projection.py: intrinsics K, pose R | t, lens distortion) runs in the same kernels through
`nr_frontend_forward_projection` / `_backward_projection`; gradients reach `vertices`, `textures`, `K`, `R` and `t`
(not `dist_coeffs`: a learnable one keeps the torch path).  The camera arrays stay on the device -- the host never reads
them -- so a call stays asynchronous and can be captured into a graph.

`fusable(...)` decides whether a call fits the kernel's parameter space (CUDA float32 tensors, look_at / look camera,
numeric viewing angle, or the projection camera; one light for the whole batch); everything else -- CPU tensors,
tensor-valued angles, per-image light colours -- keeps the module-by-module torch path of renderer.py, which mirrors the
reference line by line.
"""
import numpy as np
import torch

from . import _lib, _util


def _vec3(value):
    """Host float32 [3] from a list / tuple / ndarray, or None if `value` is not that (tensor, per-batch array, ...)."""
    if torch.is_tensor(value):
        return None
    try:
        arr = np.asarray(value, dtype=np.float32)
    except (TypeError, ValueError):
        return None
    return arr if arr.shape == (3,) else None


def _is_number(value):
    return isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool)


def _projection_layout(value, batch_size, shape, squeeze_t=False):
    """True / False = one camera parameter per image / shared, or None when `value` is not a float32 CUDA tensor or an
    array-like of shape `shape` or [B] + shape (t also [B, 1, 3])."""
    if torch.is_tensor(value):
        if not (value.is_cuda and value.dtype == torch.float32):
            return None
        got = tuple(value.shape)
    else:
        try:
            got = np.asarray(value, dtype=np.float32).shape
        except (TypeError, ValueError, RuntimeError):  # (RuntimeError: a list of CUDA tensors)
            return None
    if got == shape:
        return False
    if got == (batch_size,) + shape or (squeeze_t and got == (batch_size, 1) + shape):
        return True
    return None


def _projection_fusable(renderer, batch_size):
    if any(_projection_layout(getattr(renderer, n), batch_size, s, n == 't') is None
           for n, s in (('K', (3, 3)), ('R', (3, 3)), ('t', (3,)))):
        return False
    d = renderer.dist_coeffs
    if d is not None and ((torch.is_tensor(d) and d.requires_grad) or _projection_layout(d, batch_size, (5,)) is None):
        return False  # (a learnable dist_coeffs: the torch path gives its gradient)
    size = renderer.orig_size
    return _is_number(size) and 0 < float(size) < float('inf')


def light_fusable(renderer):
    """The light parameters are host numbers / 3-vectors, as the fused kernels take them (nr_light)."""
    if not (_is_number(renderer.light_intensity_ambient) and _is_number(renderer.light_intensity_directional)):
        return False
    return all(_vec3(v) is not None for v in (renderer.light_color_ambient, renderer.light_color_directional,
                                              renderer.light_direction))


def fusable(renderer, vertices, faces, textures):
    if not (torch.is_tensor(vertices) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 3
            and vertices.shape[2] == 3):
        return False
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dim() == 3 and faces.shape[2] == 3
            and faces.shape[0] == vertices.shape[0] and not faces.is_floating_point()):
        return False
    if vertices.shape[0] > 65535:
        return False
    if textures is not None:
        if not (torch.is_tensor(textures) and textures.is_cuda and textures.dtype == torch.float32 and textures.dim() == 6
                and tuple(textures.shape[:2]) == tuple(faces.shape[:2]) and textures.shape[5] == 3
                and textures.shape[2] == textures.shape[3] == textures.shape[4]):
            return False
        if not light_fusable(renderer):
            return False
    if renderer.camera_mode == 'projection':
        return _projection_fusable(renderer, vertices.shape[0])
    if renderer.camera_mode == 'look':
        if _vec3(renderer.camera_direction) is None:
            return False
    elif renderer.camera_mode != 'look_at':
        return False
    if renderer.perspective and not _is_number(renderer.viewing_angle):
        return False
    eye = renderer.eye
    if torch.is_tensor(eye):
        if eye.dtype != torch.float32 or tuple(eye.shape) not in ((3,), (vertices.shape[0], 3)):
            return False
    else:
        arr = np.asarray(eye, dtype=np.float32)
        if arr.shape not in ((3,), (vertices.shape[0], 3)):
            return False
    return True


_STRUCT_CACHE = {}


def _cached(kind, key, make):
    """Camera / light structs per distinct parameter set: a fixed-shape optimisation loop (example 2, B = 1) is bound by
    host time, and rebuilding two ctypes structs through NumPy costs more than the kernel they parameterise."""
    k = (kind,) + key
    v = _STRUCT_CACHE.get(k)
    if v is None:
        if len(_STRUCT_CACHE) > 128:
            _STRUCT_CACHE.clear()
        v = _STRUCT_CACHE[k] = make()
    return v


def _hashable(v):
    return tuple(np.asarray(v, dtype=np.float64).reshape(-1).tolist())


def _camera_struct(renderer):
    key = (renderer.camera_mode, bool(renderer.perspective),
           float(renderer.viewing_angle) if renderer.perspective else 0.0,
           _hashable(renderer.camera_direction) if renderer.camera_mode == 'look' else ())
    return _cached('camera', key, lambda: _make_camera_struct(renderer))


def _make_camera_struct(renderer):
    cam = _lib.Camera()
    if renderer.camera_mode == 'look_at':
        cam.mode = _lib.NR_CAMERA_LOOK_AT
        target = np.zeros(3, np.float32)  # `at` default, look_at.py:13-14 (Renderer never passes another one)
    else:
        cam.mode = _lib.NR_CAMERA_LOOK
        target = _vec3(renderer.camera_direction)
    cam.perspective = 1 if renderer.perspective else 0
    for k in range(3):
        cam.target[k] = float(target[k])
        cam.up[k] = (0.0, 1.0, 0.0)[k]  # look_at.py:17-18, look.py:16-17
    # perspective.py:10-13 in float32: angle / 180 * 3.1416, tan
    angle = np.float32(renderer.viewing_angle) / np.float32(180.) * np.float32(3.1416) if renderer.perspective \
        else np.float32(0)
    cam.width = float(np.tan(angle, dtype=np.float32))
    return cam


def _light_struct(renderer):
    key = (float(renderer.light_intensity_ambient), float(renderer.light_intensity_directional),
           _hashable(renderer.light_color_ambient), _hashable(renderer.light_color_directional),
           _hashable(renderer.light_direction))
    return _cached('light', key, lambda: _make_light_struct(renderer))


def _make_light_struct(renderer):
    light = _lib.Light()
    light.intensity_ambient = float(renderer.light_intensity_ambient)
    light.intensity_directional = float(renderer.light_intensity_directional)
    for name, src in (('color_ambient', renderer.light_color_ambient),
                      ('color_directional', renderer.light_color_directional), ('direction', renderer.light_direction)):
        v = _vec3(src)
        for k in range(3):
            getattr(light, name)[k] = float(v[k])
    return light


@_util.once_differentiable
class _FrontEnd(torch.autograd.Function):
    """forward(ctx, vertices, textures | None, faces_idx, setup, *camera)
    -> (faces [B,F,3,3], lit textures [B,F,ts,ts,ts,3] | None), or with `colors` (the front-end for the rasterizer's
    `face_light` mode, include/nr_hip.h: nr_frontend_forward_light; textures None, their gradient comes straight out of the
    rasterizer) -> (faces, light colours [B,F,3]).
    setup = (nr_camera struct | orig_size, dist | None, light | None, fill_back, colors).  camera = (eye [3] | [B,3],) with
    the nr_camera struct (look_at / look), or the projection camera's (K, R [3,3] | [B,3,3], t [3] | [B,3]) with orig_size
    and dist [5] | [B,5] | None; all float32 device tensors.  (The camera tensors come last so that a look_at call passes
    autograd no unused arguments: a fixed-shape loop at B = 1 is bound by host time.)"""

    @staticmethod
    def forward(ctx, vertices, textures, faces_idx, setup, *camera):
        cam, dist, light, fill_back, colors = setup
        dev = vertices.device
        v = _lib.dense(vertices.detach())
        idx = _lib.dense(faces_idx.detach().to(torch.int32))
        tex = _lib.dense(textures.detach()) if textures is not None else None
        camera = tuple(_lib.dense(x.detach()) for x in camera)
        d = _lib.dense(dist.detach()) if dist is not None else None
        B, Nv = v.shape[:2]
        Nf = idx.shape[1]
        F = Nf * 2 if fill_back else Nf
        ts = int(tex.shape[2]) if tex is not None else 0
        faces_out = torch.empty((B, F, 3, 3), dtype=torch.float32, device=dev)
        tex_out = torch.empty((B, F, ts, ts, ts, 3), dtype=torch.float32, device=dev) if tex is not None else None
        light_out = torch.empty((B, F, 3), dtype=torch.float32, device=dev) if colors else None
        proj = _projection_struct(*camera, d, cam) if len(camera) == 3 else None
        if proj is not None:
            fn, args = 'nr_frontend_forward_projection', (_lib.ptr(tex), faces_out.data_ptr(), _lib.ptr(tex_out),
                                                          _lib.ptr(light_out), B, Nv, Nf, ts, 1, int(fill_back), proj)
        else:
            e = camera[0]
            if colors:
                fn, args = 'nr_frontend_forward_light', (e.data_ptr(), faces_out.data_ptr(), light_out.data_ptr(), B, Nv,
                                                         Nf, 1, int(e.dim() == 2), int(fill_back), cam)
            else:
                fn, args = 'nr_frontend_forward', (_lib.ptr(tex), e.data_ptr(), faces_out.data_ptr(), _lib.ptr(tex_out),
                                                   B, Nv, Nf, ts, 1, int(e.dim() == 2), int(fill_back), cam)
        _lib.launch(fn, dev, v.data_ptr(), idx.data_ptr(), *args, light)
        ctx.save_for_backward(v, idx, tex, d, *camera)
        ctx.params = (cam, light, proj, bool(fill_back), bool(colors), B, Nv, Nf, ts)
        ctx.set_materialize_grads(False)
        return faces_out, (light_out if colors else tex_out)

    @staticmethod
    def backward(ctx, g_faces, g_second):
        v, idx, tex, _, *camera = ctx.saved_tensors
        cam, light, proj, fill_back, colors, B, Nv, Nf, ts = ctx.params
        dev = v.device
        need = ctx.needs_input_grad
        need_cam = True in need[4:]
        need_tex = need[1] and tex is not None and g_second is not None
        need_v = need[0] or need_cam  # the camera sums come out of the vertex pass
        if not (need_v or need_tex):
            return (None,) * len(need)
        F = Nf * 2 if fill_back else Nf
        if g_faces is None:
            g_faces = torch.zeros((B, F, 3, 3), dtype=torch.float32, device=dev)
        g_faces = _lib.dense(g_faces)
        g_second = _lib.dense(g_second)
        g_tex_out = g_second if tex is not None else None
        g_light = g_second if colors else None
        grad_v = torch.empty((B, Nv, 3), dtype=torch.float32, device=dev) if need_v else None
        grad_tex = torch.empty_like(tex) if need_tex else None
        grad_cam = tuple(torch.empty_like(x) if n else None for x, n in zip(camera, need[4:]))
        ws_bytes = 0
        if need_cam:
            ws_bytes = _lib.workspace_bytes('nr_frontend_projection_workspace_bytes' if proj is not None else
                                            'nr_frontend_workspace_bytes', B)
        if proj is not None:
            fn, args = 'nr_frontend_backward_projection', (
                _lib.ptr(tex), g_faces.data_ptr(), _lib.ptr(g_tex_out), _lib.ptr(g_light), _lib.ptr(grad_v), _lib.ptr(grad_tex),
                *(_lib.ptr(g) for g in grad_cam), B, Nv, Nf, ts, 1, int(fill_back), proj)
        else:
            e = camera[0]
            if colors:
                fn, args = 'nr_frontend_backward_light', (e.data_ptr(), g_faces.data_ptr(), _lib.ptr(g_light),
                                                          grad_v.data_ptr(), _lib.ptr(grad_cam[0]), B, Nv, Nf, 1,
                                                          int(e.dim() == 2), int(fill_back), cam)
            else:
                fn, args = 'nr_frontend_backward', (_lib.ptr(tex), e.data_ptr(), g_faces.data_ptr(), _lib.ptr(g_tex_out),
                                                    _lib.ptr(grad_v), _lib.ptr(grad_tex), _lib.ptr(grad_cam[0]), B, Nv, Nf,
                                                    ts, 1, int(e.dim() == 2), int(fill_back), cam)
        _lib.launch(fn, dev, v.data_ptr(), idx.data_ptr(), *args, light, workspace_bytes=ws_bytes)
        return ((grad_v if need[0] else None), grad_tex, None, None) + grad_cam


def _projection_struct(K, R, t, d, orig_size):
    """struct nr_projection for contiguous float32 device tensors (its pointers change with every call: not cached)."""
    p = _lib.Projection()
    p.K, p.R, p.t = K.data_ptr(), R.data_ptr(), t.data_ptr()
    p.dist_coeffs = _lib.ptr(d)
    p.K_per_batch, p.R_per_batch, p.t_per_batch = int(K.dim() == 3), int(R.dim() == 3), int(t.dim() == 2)
    p.dist_per_batch = int(d is not None and d.dim() == 2)
    p.orig_size = float(orig_size)
    return p


_EYE_CACHE = {}


def _eye_tensor(eye, device):
    """`eye` (or a projection camera parameter) as a float32 device tensor; array-likes are converted once and cached."""
    if torch.is_tensor(eye):
        return eye.to(device=device)
    arr = np.ascontiguousarray(eye, dtype=np.float32)
    key = (str(device), arr.shape, arr.tobytes())
    t = _EYE_CACHE.get(key)
    if t is None:
        if len(_EYE_CACHE) > 64:
            _EYE_CACHE.clear()
        t = _EYE_CACHE[key] = torch.as_tensor(arr, device=device)
    return t


def _project(renderer, vertices, faces, textures, colors):
    _util.check_face_indices(faces, vertices.shape[1], vertices.device)
    dev = vertices.device
    light = _light_struct(renderer) if (textures is not None or colors) else None
    if renderer.camera_mode == 'projection':
        K, R, t = (_eye_tensor(getattr(renderer, n), dev) for n in ('K', 'R', 't'))
        if t.dim() == 3:  # [B, 1, 3]
            t = t.reshape(t.shape[0], 3)
        d = _eye_tensor(renderer.dist_coeffs, dev) if renderer.dist_coeffs is not None else None
        setup = (float(renderer.orig_size), d, light, bool(renderer.fill_back), colors)
        return _FrontEnd.apply(vertices, textures, faces, setup, K, R, t)
    setup = (_camera_struct(renderer), None, light, bool(renderer.fill_back), colors)
    return _FrontEnd.apply(vertices, textures, faces, setup, _eye_tensor(renderer.eye, dev))


def project_and_light(renderer, vertices, faces, textures=None):
    """-> (faces [B,F,3,3], lit textures | None) for the rasterizer; call only when fusable(...)."""
    return _project(renderer, vertices, faces, textures, False)


def project_and_light_colors(renderer, vertices, faces):
    """-> (faces [B,F,3,3], light colours [B,F,3]) for the rasterizer's face_light mode; call only when fusable(...)."""
    return _project(renderer, vertices, faces, None, True)
