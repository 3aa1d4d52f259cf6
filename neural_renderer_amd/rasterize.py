"""Rasterizer operator: the reference's `neural_renderer/rasterize.py` API on PyTorch-ROCm tensors,
backed by the hand-written HIP kernels of libnr_hip.so (include/nr_hip.h) through ctypes.

Mirrors (reference file:line):
  Rasterize(image_size, near, far, eps, background_color, return_rgb, return_alpha, return_depth)
      rasterize.py:19-64 (constructor), :467-513 (forward_gpu), :849-889 (backward_gpu)
  rasterize_rgbad / rasterize / rasterize_silhouettes / rasterize_depth      rasterize.py:900-1060
  use_unsafe_rasterizer                                                        rasterize.py:1063-1065
  module defaults                                                              rasterize.py:7-16

There is no CPU path (the reference has none either: rasterize.py:893-897) and no eager fallback.
"""
import collections
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib, _util
from ._lib import on_device as _on_device, stream_ptr as _stream_ptr
from .uv_textures import UVImages, pack_images, unpack_image_gradients
from .vertex_colors import CornerColors

DEFAULT_IMAGE_SIZE = 256
DEFAULT_ANTI_ALIASING = True
DEFAULT_NEAR = 0.1
DEFAULT_FAR = 100
DEFAULT_EPS = 1e-4
DEFAULT_BACKGROUND_COLOR = (0, 0, 0)
USE_UNSAFE_IMPLEMENTATION = False

if 'NEURAL_RENDERER_UNSAFE' in os.environ and int(os.environ['NEURAL_RENDERER_UNSAFE']):
    USE_UNSAFE_IMPLEMENTATION = True

# the reference samples textures with the face depth of batch element 0
# (rasterize.py:389).  Default = reference-literal; NR_FIX_TEXTURE_BATCH_Z=1 (or the `fix_batch_z`
# attribute of a Rasterize instance) uses the pixel's own batch element.
FIX_TEXTURE_BATCH_Z = bool(int(os.environ.get('NR_FIX_TEXTURE_BATCH_Z', '0')))

# K6 (backward_pixel_map) numerics.  Default: float terms through fused multiply-adds and the hardware reciprocal, ~1 ulp per
# term; the tests bound the deviation from the reference's terms summed exactly by the north star's 1e-4 (plus twice the reference's
# own float-summation noise on entries that cancel down to the metric's floor: include/nr_hip.h).  NR_EXACT_GRADIENT=1
# (read once, here) or the `exact_gradient` attribute of a Rasterize instance: every term with the reference's own arithmetic,
# sums in double (bound 2e-6).  Measured levels and costs of both: profiles/*_parity_summary.md.
# Reproducibility: both modes return the same grad_faces bit for bit from call to call, and for a batch and its shards (one band
# kernel, k_bpm_row, whose per-record sums do not depend on the launch; profiles/r06_same_terms.txt).
EXACT_GRADIENT = bool(int(os.environ.get('NR_EXACT_GRADIENT', '0')))
# (measuring aid, read once: NR_SERIAL_BACKWARD=1 makes the fused backward launch K6's line setup, its band kernel and the gather one
# after the other instead of the first and the last in one grid -- include/nr_hip.h NR_FLAG_SERIAL_BACKWARD; same values)
_BACKWARD_ORDER_FLAG = _lib.NR_FLAG_SERIAL_BACKWARD if int(os.environ.get('NR_SERIAL_BACKWARD', '0')) else 0
# (measuring aid, read once: NR_K6_LEGACY=1 keeps K6's default mode on the piece-per-lane band kernel -- NR_FLAG_K6_LEGACY)
_BACKWARD_ORDER_FLAG |= _lib.NR_FLAG_K6_LEGACY if int(os.environ.get('NR_K6_LEGACY', '0')) else 0


_BG_CACHE = {}


def _background_tensor(bg, device):
    """Device copy of a host background colour, cached (a pageable H2D copy per call would serialise the stream)."""
    # (the fast key only for tuples of plain Python numbers: a 0-d tensor or array element hashes by identity and may change in
    # place; floats are keyed by their repr so that -0.0 and 0.0 stay apart)
    fast = type(bg) is tuple and all(type(x) in (int, float) for x in bg)
    if fast:
        key = (device.index, tuple(repr(x) for x in bg))
        t = _BG_CACHE.get(key)
        if t is not None:
            return t
    arr = np.asarray(bg, dtype=np.float32)
    key2 = (device.index, arr.shape, arr.tobytes())
    t = _BG_CACHE.get(key2)
    if t is None:
        if len(_BG_CACHE) > 64:
            _BG_CACHE.clear()
        t = _BG_CACHE[key2] = torch.as_tensor(arr, device=device)
    if fast:
        _BG_CACHE[key] = t
    return t


# Graph replay (not in the reference): for fixed shapes the forward and the backward of the operator are each captured once
# in a HIP graph and replayed from then on -- at small batches the ~12 launches of a step take longer to ISSUE than to run
# (BASELINE config 2, 16 views: 0.27 ms eager, 0.18 ms replayed).  Off by default; `use_graph_replay(True)`, the
# NR_GRAPH_REPLAY=1 environment variable (read once, here) or the `graph_replay` attribute of a Rasterize / Renderer
# instance switch it on.  Semantics stay those of the eager operator: inputs are copied into the graphs' fixed buffers and
# results are returned as copies, so callers may keep them; what replay cannot offer is two forwards of the same shapes in
# flight before the first one's backward (the residual maps live in the fixed buffers) -- that raises.  Measured (config 2):
# 0.25 ms eager -> 0.21 ms with replay; a step captured as a whole by the caller (neural_renderer_amd.graph.capture: no
# copies, loss and optimizer inside) 0.17 ms -- prefer that where the whole step is fixed.  (Round 3's crash of a whole-step
# capture after this mode had run is gone: neural_renderer_amd.graph.capture.)  `clear_graph_replay_cache()` drops the graphs.
GRAPH_REPLAY = bool(int(os.environ.get('NR_GRAPH_REPLAY', '0')))


def use_graph_replay(flag):
    global GRAPH_REPLAY
    GRAPH_REPLAY = bool(flag)


# The forward's scratch (z-buffer + queues), kept per (device, stream, sizes) and reused with a falling epoch number
# (include/nr_hip.h: NR_FLAG_ZBUF_EPOCH) so that the library neither fills the z-buffer before a call nor cleans it afterwards.
# Least-recently-used entries go first; the cache holds at most _ZBUF_CACHE_BYTES (a workspace larger than half of that is
# not kept at all: such a call takes the per-call fill); `clear_workspace_cache()` releases everything.
_ZBUF_CACHE = collections.OrderedDict()
_ZBUF_CACHE_BYTES = int(os.environ.get('NR_WORKSPACE_CACHE_MB', '1024')) << 20
_ZBUF_LOCK = threading.Lock()


def clear_workspace_cache():
    """Release the kept forward workspaces (8 bytes per raster pixel each; see _forward_workspace)."""
    with _ZBUF_LOCK:
        _ZBUF_CACHE.clear()


def _forward_workspace(lib, dev, stream, B, F, S):
    """(workspace tensor, flags) for one forward call.  A kept workspace is refilled with 0xff every 255 calls.  While
    a HIP graph is being captured the epoch would be frozen into the graph, so capture takes a throw-away workspace and the
    filling path."""
    ws_bytes = lib.nr_forward_workspace_bytes(B, F, S)
    if ws_bytes == 0:
        raise ValueError('unsupported sizes B=%d F=%d S=%d' % (B, F, S))
    if F >= (1 << 24) or 2 * ws_bytes > _ZBUF_CACHE_BYTES or torch.cuda.is_current_stream_capturing():
        return torch.empty((ws_bytes,), dtype=torch.uint8, device=dev), 0
    # (the calling THREAD is part of the key: the epochs of a workspace must reach the stream in the order they were handed out
    # -- a call launched later with the larger epoch of an earlier hand-out would lose every atomic minimum against the words of
    # the call in front of it -- and within one host thread hand-out order is launch order; two threads rendering the same shapes
    # on one stream each keep their own workspace)
    key = (dev.index, int(stream), B, F, S, threading.get_ident())
    with _ZBUF_LOCK:
        ent = _ZBUF_CACHE.get(key)
        if ent is None:
            total = sum(e[0].numel() for e in _ZBUF_CACHE.values()) + ws_bytes
            while _ZBUF_CACHE and (total > _ZBUF_CACHE_BYTES or len(_ZBUF_CACHE) >= 16):
                total -= _ZBUF_CACHE.popitem(last=False)[1][0].numel()
            ent = _ZBUF_CACHE[key] = [torch.empty((ws_bytes,), dtype=torch.uint8, device=dev), -1]
        else:
            _ZBUF_CACHE.move_to_end(key)
        if ent[1] < 0:
            ent[0].fill_(255)
            ent[1] = 254
        epoch = ent[1]
        ent[1] -= 1
    return ent[0], _lib.NR_FLAG_ZBUF_EPOCH | (epoch << 8)


class _Config(object):
    """What a Rasterize instance is configured with, frozen for one call (the autograd node keeps it)."""
    __slots__ = ('image_size', 'near', 'far', 'eps', 'background_color', 'return_rgb', 'return_alpha', 'return_depth',
                 'fix_batch_z', 'exact_gradient', 'faces_z_ref', 'owner')

    def __init__(self, fn):
        self.image_size = int(fn.image_size)
        self.near, self.far, self.eps = float(fn.near), float(fn.far), float(fn.eps)
        self.background_color = fn.background_color if fn.background_color is not None else DEFAULT_BACKGROUND_COLOR
        self.return_rgb, self.return_alpha, self.return_depth = bool(fn.return_rgb), bool(fn.return_alpha), bool(fn.return_depth)
        self.fix_batch_z, self.exact_gradient = bool(fn.fix_batch_z), bool(fn.exact_gradient)
        self.faces_z_ref = fn.faces_z_ref
        self.owner = weakref.ref(fn)


class _Residuals(object):
    """Everything one forward leaves behind for its backward (the reference keeps the same on `self`, rasterize.py:39-58).
    `source` is the call's shading source; textures / light / packed / corner are what that source keeps (the rest None)."""
    __slots__ = ('B', 'F', 'S', 'ts', 'Nf', 'flags', 'faces', 'z_ref', 'face_index_map', 'weight_map', 'depth_map',
                 'rgb_map', 'alpha_map', 'visible', 'source', 'textures', 'light', 'packed', 'corner', 'shared')

    def __init__(self):
        self.textures = self.light = None  # cubes [B,Nf,ts,ts,ts,3]; per-face light colours [B,F,3]
        self.shared = False                # the cubes are [1,Nf,ts,ts,ts,3], one set for all B > 1 images
        self.packed = None                 # per-pixel UV images: their packing [Bi,P,3]
        self.corner = None                 # corner colours [B,F,3,3]


def _base_flags(cfg):
    """The flags both directions of a call share (the forward adds its workspace's and the sparse weight map's)."""
    flags = (_lib.NR_FLAG_FIX_TEXTURE_BATCH_Z if cfg.fix_batch_z else 0) | _BACKWARD_ORDER_FLAG
    if cfg.exact_gradient:
        flags |= _lib.NR_FLAG_EXACT_GRADIENT
    return flags


def _alloc_maps(r, cfg, dev):
    """The output and residual maps of a call of r's sizes."""
    B, F, S = r.B, r.F, r.S
    need_wd = cfg.return_rgb or cfg.return_depth
    i32, f32 = torch.int32, torch.float32
    r.face_index_map = torch.empty((B, S, S), dtype=i32, device=dev)
    r.weight_map = torch.empty((B, S, S, 3), dtype=f32, device=dev) if need_wd else None
    r.depth_map = torch.empty((B, S, S), dtype=f32, device=dev) if need_wd else None
    r.rgb_map = torch.empty((B, S, S, 3), dtype=f32, device=dev) if cfg.return_rgb else None
    r.alpha_map = torch.empty((B, S, S), dtype=f32, device=dev) if cfg.return_alpha else None
    # per-face "owns a pixel" flags: a residual the backward starts from (K6's lists; the depth-only gather skips the
    # faces without a pixel)
    r.visible = torch.empty((B, F), dtype=torch.uint8, device=dev)


def _launch_forward(lib, cfg, r, background, bg_per_batch, flags, workspace, stream):
    """The forward's one C-ABI call (visibility + shading, rasterize.py:499-502) into r's maps: the source's entry point around
    the arguments every source shares.  The eager operator and graph replay both launch through here."""
    ptr = _lib.ptr
    maps = (r.face_index_map.data_ptr(), ptr(r.weight_map), ptr(r.depth_map), ptr(r.rgb_map), ptr(r.alpha_map),
            r.visible.data_ptr(), ptr(background), bg_per_batch, r.B, r.F, r.S)
    r.source.forward(lib, cfg, r, maps, (flags, workspace.data_ptr(), workspace.numel(), stream))


def _launch_backward(lib, cfg, r, lit, grad_textures, g_rgb, g_alpha, g_depth, grad_faces, workspace, ws_bytes, stream):
    """K6 -> K7 -> K8 (rasterize.py:881-883) behind one C-ABI call, from r's maps.  A gradient that is None is zeros: its terms
    are skipped.  `lit` / `grad_textures`: the texture stage of the cubes (None: grad_faces alone, K6 + K8)."""
    ptr = _lib.ptr
    _lib.check(lib.nr_backward_rasterize_lit(
        lit, r.faces.data_ptr(), ptr(r.z_ref), r.face_index_map.data_ptr(), ptr(r.weight_map), ptr(r.depth_map),
        ptr(r.rgb_map) if g_rgb is not None else None, ptr(r.alpha_map) if g_alpha is not None else None, ptr(g_rgb),
        ptr(g_alpha), ptr(g_depth), grad_faces.data_ptr(), ptr(grad_textures), r.B, r.F, r.S, r.ts, cfg.eps, r.flags,
        ptr(r.visible), workspace.data_ptr(), ws_bytes, stream), 'nr_backward_rasterize')


class _Cubes(object):
    """Shading source: texture cubes [B,Nf,ts,ts,ts,3] as in the reference (None when no rgb is drawn), alone or with per-face
    light colours [B,F,3] (F = Nf or 2 Nf; include/nr_hip.h: nr_face_light).  Inputs of the autograd node: (textures, light).
    Cubes [1,Nf,ts,ts,ts,3] beside B > 1 images (not in the reference) are ONE set shared by the batch: the forward reads the
    single copy (NR_FLAG_SHARED_TEXTURES), the backward returns its gradient summed over the images, [1,Nf,...]
    (nr_backward_textures_shared behind the rasterizer's own backward, which then runs without its texture stage).

    A shading source is everything the operator does differently for one kind of `textures`; _source_of picks it, and the
    operator asks it for: `check` (the input checks -> Nf, ts), `keep` (the residuals of the inputs), `saved` / `restore`
    (which of them go through save_for_backward), `forward` (the C call) and `backward` (the rasterizer's backward plus the
    source's colour gradient -> one gradient per input)."""
    def check(self, cfg, faces, B, F, inputs):
        textures, light = inputs
        Nf = F
        if not cfg.return_rgb:
            return Nf, 0
        if textures is None:
            raise ValueError('textures are required when return_rgb is set')
        if light is not None:
            if light.dim() == 4 and tuple(light.shape) == (B, F, 3, 3):
                raise ValueError('face_light [batch size, num of faces, 3, 3] (a light colour per corner) goes with UVImages '
                                 'only: texture cubes take one colour per face, [batch size, num of faces, 3]')
            if light.dtype != torch.float32 or tuple(light.shape) != (B, F, 3):
                raise ValueError('face_light must be float32 [batch size, num of faces, 3], got %s %s'
                                 % (light.dtype, tuple(light.shape)))
            if textures.dim() == 6 and textures.shape[1] * 2 == F:
                Nf = F // 2  # fill_back: face Nf + f is the reversed copy of face f
        sh = textures.shape
        if (textures.dtype != torch.float32 or textures.dim() != 6 or sh[0] not in (1, B) or sh[1] != Nf or sh[2] < 2 or
                sh[2] != sh[3] or sh[3] != sh[4] or sh[5] != 3):
            raise ValueError('textures must be float32 [batch size (or 1: shared by the batch), num of faces, ts, ts, ts, 3] '
                             'with ts >= 2, got %s %s' % (textures.dtype, tuple(sh)))  # rasterize.py:78-90
        if sh[0] != B and sh[2] > 13:
            raise ValueError('textures shared by the batch need ts <= 13, got %d: expand them to the batch size' % sh[2])
        return Nf, int(sh[2])

    def keep(self, r, inputs):
        textures, light = inputs
        r.shared = textures is not None and textures.shape[0] != r.B
        r.textures = _lib.dense(textures.detach()) if textures is not None else None  # rasterize.py:473
        r.light = _lib.dense(light.detach()) if light is not None else None

    def saved(self, r):
        return (r.textures if r.light is not None else None), r.light  # (the backward reads the cubes only with light)

    def restore(self, r, saved):
        r.textures, r.light = saved

    def forward(self, lib, cfg, r, maps, tail):
        # weight_map is a residual only (the backward reads it at covered pixels): the eager operator does not store the zeros
        # of uncovered pixels (NR_FLAG_SPARSE_WEIGHT_MAP; `Rasterize.weight_map` fills them in when somebody reads the attribute)
        lit = _lib.FaceLight(r.light.data_ptr(), r.Nf, None, None) if r.light is not None else None
        if r.shared:
            tail = (tail[0] | _lib.NR_FLAG_SHARED_TEXTURES,) + tuple(tail[1:])
        _lib.check(lib.nr_forward_rasterize_lit(lit, r.faces.data_ptr(), _lib.ptr(r.z_ref), _lib.ptr(r.textures), *maps, r.ts,
                                                cfg.near, cfg.far, cfg.eps, *tail), 'nr_forward_rasterize')

    def _backward_shared(self, lib, cfg, r, want, call):
        """One set of cubes for the batch: grad_faces from the rasterizer's backward without its texture stage (K6 + K8 do not
        read the cubes), then the gather over (image, face) pairs that sums the cubes' gradient over the images."""
        _launch_backward(lib, cfg, r, None, None, *call)
        g_rgb, stream = call[0], call[-1]
        if g_rgb is None or not (want[0] or (r.light is not None and want[1])):
            return None, None
        B, F, ts = r.B, r.F, r.ts
        f32, dev = torch.float32, r.faces.device
        grad_textures = torch.empty((1, r.Nf, ts, ts, ts, 3), dtype=f32, device=dev)
        grad_light = lit = None
        if r.light is not None:
            grad_light = torch.empty((B, F, 3), dtype=f32, device=dev) if want[1] else None
            lit = _lib.FaceLight(r.light.data_ptr(), r.Nf, r.textures.data_ptr(), _lib.ptr(grad_light))
        ws_bytes = lib.nr_backward_textures_shared_workspace_bytes(B, r.Nf, ts)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        _lib.check(lib.nr_backward_textures_shared(
            lit, r.faces.data_ptr(), _lib.ptr(r.z_ref), r.face_index_map.data_ptr(), r.weight_map.data_ptr(),
            r.depth_map.data_ptr(), g_rgb.data_ptr(), _lib.ptr(r.visible), grad_textures.data_ptr(), B, F, r.S, ts, cfg.eps,
            r.flags, ws.data_ptr(), ws_bytes, stream), 'nr_backward_textures_shared')
        return grad_textures, grad_light

    def backward(self, lib, cfg, r, want, call):
        if r.shared:
            return self._backward_shared(lib, cfg, r, want, call)
        grad_textures = grad_light = lit = None
        if call[0] is not None:  # a gradient of rgb_map: the texture stage (K7) runs inside the rasterizer's backward
            B, F, ts = r.B, r.F, r.ts
            f32, dev = torch.float32, r.faces.device
            if r.light is not None:
                if want[0] or want[1]:
                    # one gather produces both (the colours' gradient is a by-product of the texel sums)
                    grad_textures = torch.empty((B, r.Nf, ts, ts, ts, 3), dtype=f32, device=dev)
                    if want[1]:
                        grad_light = torch.empty((B, F, 3), dtype=f32, device=dev)
                lit = _lib.FaceLight(r.light.data_ptr(), r.Nf, r.textures.data_ptr(), _lib.ptr(grad_light))
            elif want[0]:
                grad_textures = torch.empty((B, F, ts, ts, ts, 3), dtype=f32, device=dev)
        _launch_backward(lib, cfg, r, lit, grad_textures, *call)
        return grad_textures, grad_light


class _UVSource(object):
    """Shading source: a UVImages with per-face light colours [B,F,3] -- the images sampled at every covered pixel
    (include/nr_hip.h: nr_forward_rasterize_uv / nr_backward_uv_images) -- or with a light colour per corner [B,F,3,3],
    interpolated at the pixel (nr_forward_rasterize_uv_smooth / nr_backward_uv_images_smooth): light.dim() picks the entry
    points, and the light's gradient has the light's shape.  Inputs of the autograd node: (light, *images).
    grad_faces comes from the rasterizer's own backward (K6 + K8, no texture stage), the images' and the colours' gradients
    from nr_backward_uv_images.  Always eager: the operator's graph-replay mode does not apply (a whole step can still be
    captured with neural_renderer_amd.graph)."""
    name = 'UVImages'

    def __init__(self, uv):
        self.uv = uv

    def check(self, cfg, faces, B, F, inputs):
        uv, light = self.uv, inputs[0]
        Nf = uv.layout.num_faces
        if (light.dtype != torch.float32 or tuple(light.shape) not in ((B, F, 3), (B, F, 3, 3)) or not light.is_cuda):
            raise ValueError('face_light must be float32 [batch size, num of faces, 3] (a colour per face) or [batch size, '
                             'num of faces, 3, 3] (a colour per corner) on the GPU, got %s %s'
                             % (light.dtype, tuple(light.shape)))
        if F not in (Nf, 2 * Nf):
            raise ValueError('UVImages: the layout has %d faces, the call %d (the layout\'s, or twice that with fill_back)'
                             % (Nf, F))
        if uv.image_batch not in (1, B):
            raise ValueError('UVImages: batched images must have the batch size of the faces (%d), got %d'
                             % (B, uv.image_batch))
        if uv.device != faces.device or light.device != faces.device:
            raise ValueError('UVImages: images, face_light and faces must be on one device')
        return Nf, uv.layout.texture_size

    def keep(self, r, inputs):
        r.light = _lib.dense(inputs[0].detach())
        r.packed = pack_images(inputs[1:], self.uv.batch).detach()

    def saved(self, r):
        return r.light, r.packed

    def restore(self, r, saved):
        r.light, r.packed = saved

    def _struct(self, r):
        """struct nr_uv_images of the layout's device tables (uploaded once per device) and the call's packing."""
        layout = self.uv.layout
        st = layout._tensors(r.faces.device)
        return _lib.UVImagesStruct(r.packed.data_ptr(), st['table'].data_ptr(), st['faces_uv'].data_ptr(),
                                   st['face_image'].data_ptr(), st['base'].data_ptr(), layout.texture_size, layout.num_images,
                                   layout.num_pixels, int(r.packed.shape[0]))

    def forward(self, lib, cfg, r, maps, tail):
        if r.light.dim() == 4:
            _lib.check(lib.nr_forward_rasterize_uv_smooth(_lib.CornerLight(r.light.data_ptr(), r.Nf, None), self._struct(r),
                                                          r.faces.data_ptr(), *maps, cfg.near, cfg.far, cfg.eps, *tail),
                       'nr_forward_rasterize_uv_smooth')
            return
        _lib.check(lib.nr_forward_rasterize_uv(_lib.FaceLight(r.light.data_ptr(), r.Nf, None, None), self._struct(r),
                                               r.faces.data_ptr(), *maps, cfg.near, cfg.far, cfg.eps, *tail),
                   'nr_forward_rasterize_uv')

    def backward(self, lib, cfg, r, want, call):
        _launch_backward(lib, cfg, r, None, None, *call)
        g_rgb, stream = call[0], call[-1]
        grads = [None] * len(want)
        want_images = True in want[1:]
        if g_rgb is None or not (want[0] or want_images):
            return tuple(grads)
        uv, B, F = self.uv, r.B, r.F
        f32, dev, ptr = torch.float32, r.faces.device, _lib.ptr
        Bi, P = int(r.packed.shape[0]), uv.layout.num_pixels
        grad_packed = torch.empty((Bi, P, 3), dtype=f32, device=dev) if want_images else None
        grads[0] = torch.empty_like(r.light) if want[0] else None
        if r.light.dim() == 4:
            name, lit = 'nr_backward_uv_images_smooth', _lib.CornerLight(r.light.data_ptr(), r.Nf, ptr(grads[0]))
        else:
            name, lit = 'nr_backward_uv_images', _lib.FaceLight(r.light.data_ptr(), r.Nf, None, ptr(grads[0]))
        ws_bytes = getattr(lib, name + '_workspace_bytes')(B, F, P, Bi)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        _lib.check(getattr(lib, name)(
            lit, self._struct(r), r.faces.data_ptr(), r.face_index_map.data_ptr(), r.weight_map.data_ptr(),
            r.depth_map.data_ptr(), g_rgb.data_ptr(), ptr(grad_packed), B, F, r.S, cfg.eps, ws.data_ptr(), ws_bytes, stream),
            name)
        if want_images:
            for m, (g, im) in enumerate(zip(unpack_image_gradients(uv.layout, grad_packed), uv.images), 1):
                if want[m]:  # an image shared by the batch: one row when every image is shared, else the rows summed
                    grads[m] = g if im.dim() == 4 else (g[0] if uv.batch is None else g.sum(0))
        return tuple(grads)


class _CornerSource(object):
    """Shading source: corner colours [B,F,3,3], three lit colours per face interpolated at every covered pixel
    (include/nr_hip.h: nr_forward_rasterize_corner / nr_backward_corner_colors).  Input of the autograd node: (colors,).
    grad_faces comes from the rasterizer's own backward (K6 + K8, no texture stage).  Always eager, like _UVSource."""
    name = 'CornerColors'

    def check(self, cfg, faces, B, F, inputs):
        cc = inputs[0]
        if not cc.is_cuda or cc.device != faces.device:
            raise ValueError('CornerColors: colors and faces must be on one GPU (%s, %s)' % (cc.device, faces.device))
        if int(cc.shape[0]) != B:
            raise ValueError('CornerColors: batch size %d, the faces have %d' % (cc.shape[0], B))
        if int(cc.shape[1]) != F:
            raise ValueError('CornerColors: %d faces, the call has %d (with fill_back the reversed copies carry their own '
                             'colours: twice the mesh\'s faces)' % (cc.shape[1], F))
        return F, 0

    def keep(self, r, inputs):
        r.corner = _lib.dense(inputs[0].detach())

    def saved(self, r):
        return r.corner,

    def restore(self, r, saved):
        r.corner, = saved

    def forward(self, lib, cfg, r, maps, tail):
        _lib.check(lib.nr_forward_rasterize_corner(r.corner.data_ptr(), r.faces.data_ptr(), *maps, cfg.near, cfg.far, *tail),
                   'nr_forward_rasterize_corner')

    def backward(self, lib, cfg, r, want, call):
        _launch_backward(lib, cfg, r, None, None, *call)
        g_rgb, stream = call[0], call[-1]
        if g_rgb is None or not want[0]:
            return None,
        grad_colors = torch.empty_like(r.corner)
        ws_bytes = lib.nr_backward_corner_colors_workspace_bytes(r.B, r.F)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=r.faces.device)
        _lib.check(lib.nr_backward_corner_colors(
            r.faces.data_ptr(), r.face_index_map.data_ptr(), r.weight_map.data_ptr(), r.depth_map.data_ptr(),
            g_rgb.data_ptr(), _lib.ptr(r.visible), grad_colors.data_ptr(), r.B, r.F, r.S, ws.data_ptr(), ws_bytes, stream),
            'nr_backward_corner_colors')
        return grad_colors,


_CUBES, _CORNER = _Cubes(), _CornerSource()


def _no_protocol(name):
    raise NotImplementedError('forward_gpu / backward_gpu do not take %s: call the Rasterize instance itself, which records '
                              'the autograd graph' % name)


def _source_of(textures, face_light, protocol=False):
    """(shading source, the differentiable inputs it takes after `faces`) of a call -- the one place that looks at what
    `textures` is.  `protocol`: the call comes through forward_gpu / backward_gpu, which take cubes only."""
    if not isinstance(textures, (UVImages, CornerColors)):
        return _CUBES, (textures, face_light)
    if protocol:
        _no_protocol(type(textures).__name__)
    if isinstance(textures, UVImages):  # (not in the reference) images sampled per pixel: per-face light colours required
        if face_light is None:
            raise ValueError('UVImages need face_light: light colours per face [batch size, num of faces, 3] or per corner '
                             '[batch size, num of faces, 3, 3]')
        return _UVSource(textures), (face_light,) + tuple(textures.images)
    if face_light is not None:  # (not in the reference) three lit colours per face: no light, no cubes
        raise ValueError('CornerColors are already lit: face_light does not apply')
    return _CORNER, (textures.colors,)


def _forward_impl(cfg, faces, src, inputs):
    """forward_gpu (rasterize.py:467-513): visibility + shading behind one C-ABI call, for the shading source `src` and its
    `inputs` (_source_of).  Returns the residuals."""
    lib = _lib.load()
    # type / shape checks of rasterize.py:66-90 (the source's: + the face_light, UVImages and CornerColors extensions)
    if not faces.is_cuda:
        raise NotImplementedError('neural_renderer_amd has no CPU rasterizer (neither has the reference: '
                                  'rasterize.py:893-897)')
    if faces.dtype != torch.float32 or faces.dim() != 4 or tuple(faces.shape[2:]) != (3, 3):
        raise ValueError('faces must be float32 [batch size, num of faces, 3, 3], got %s %s'
                         % (faces.dtype, tuple(faces.shape)))
    B, F = int(faces.shape[0]), int(faces.shape[1])
    Nf, ts = src.check(cfg, faces, B, F, inputs)
    dev = faces.device
    S = cfg.image_size
    r = _Residuals()
    r.B, r.F, r.S, r.ts, r.Nf, r.source = B, F, S, ts, Nf, src
    r.faces = _lib.dense(faces.detach())  # rasterize.py:470
    src.keep(r, inputs)
    with _on_device(dev):
        stream = _stream_ptr(dev)
        _alloc_maps(r, cfg, dev)
        workspace, ws_flags = _forward_workspace(lib, dev, stream, B, F, S)
        background = None
        bg_per_batch = 0
        if cfg.return_rgb:
            bg = cfg.background_color
            if torch.is_tensor(bg):
                background = _lib.dense(bg.detach().to(device=dev, dtype=torch.float32))
            else:
                background = _background_tensor(bg, dev)
            if tuple(background.shape) == (B, 3):
                bg_per_batch = 1  # rasterize.py:464-465
            elif tuple(background.shape) != (3,):
                raise ValueError('background_color must have shape (3,) or (batch size, 3)')
        r.flags = _base_flags(cfg)
        # batch element 0 of the GLOBAL batch when this call holds a shard of it (include/nr_hip.h)
        z_ref = cfg.faces_z_ref
        if z_ref is not None:
            z_ref = _lib.dense(z_ref.detach().to(device=dev, dtype=torch.float32))
            if tuple(z_ref.shape) != (F, 3, 3):
                raise ValueError('faces_z_ref must have shape (num of faces, 3, 3), got %s' % (tuple(z_ref.shape),))
        r.z_ref = z_ref
        _launch_forward(lib, cfg, r, background, bg_per_batch, r.flags | ws_flags | _lib.NR_FLAG_SPARSE_WEIGHT_MAP, workspace,
                        stream)
    return r


_BWD_WS_BYTES = {}


def _backward_impl(cfg, r, g_rgb, g_alpha, g_depth, want):
    """backward_gpu (rasterize.py:849-889).  `None` gradients are zeros (:858-878); a zero gradient adds exactly 0 to every
    `diff_grad`, so the corresponding term is skipped instead of being multiplied out.  Returns (grad_faces, one gradient or
    None per input of the call's shading source); `want` says which of those inputs ask for one."""
    lib = _lib.load()
    B, F, S = r.B, r.F, r.S
    use_rgb = cfg.return_rgb and g_rgb is not None
    use_alpha = cfg.return_alpha and g_alpha is not None
    use_depth = cfg.return_depth and g_depth is not None
    if not (use_rgb or use_alpha or use_depth):
        return None, (None,) * len(want)
    dev = r.faces.device
    with _on_device(dev):
        stream = _stream_ptr(dev)
        g_rgb = _lib.dense(g_rgb) if use_rgb else None
        g_alpha = _lib.dense(g_alpha) if use_alpha else None
        g_depth = _lib.dense(g_depth) if use_depth else None
        grad_faces = torch.empty_like(r.faces)  # stored by the library (zeros when neither rgb nor alpha)
        key = (B, F, S, use_rgb, use_alpha)
        ws_bytes = _BWD_WS_BYTES.get(key)
        if ws_bytes is None:
            if len(_BWD_WS_BYTES) > 256:
                _BWD_WS_BYTES.clear()
            ws_bytes = _BWD_WS_BYTES[key] = lib.nr_backward_workspace_bytes(B, F, S, int(use_rgb), int(use_alpha))
        workspace = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        grads = r.source.backward(lib, cfg, r, want, (g_rgb, g_alpha, g_depth, grad_faces, workspace, ws_bytes, stream))
    owner = cfg.owner()
    if owner is not None:  # rasterize.py:41-51: the gradient buffers stay readable on the instance
        owner.grad_rgb_map, owner.grad_alpha_map, owner.grad_depth_map = g_rgb, g_alpha, g_depth
        # (aliases, not the returned tensors themselves: a second reference to a returned gradient makes autograd's
        # AccumulateGrad clone it instead of adopting it -- two device copies, 41 MB per step at the headline size)
        owner.grad_faces = grad_faces.detach()
        owner.grad_textures = grads[0].detach() if (r.source is _CUBES and grads[0] is not None) else None
    return grad_faces, grads


@_util.once_differentiable
class _RasterizeFunction(torch.autograd.Function):
    """forward(ctx, faces, cfg, source, *inputs) -> (rgb_map [B,S,S,3] | None, alpha_map [B,S,S] | None,
    depth_map [B,S,S] | None, face_index_map); backward(ctx, g_rgb, g_alpha, g_depth, _) -> (grad_faces, None, None, one
    gradient per input).  `source`, `inputs`: the call's shading source and its differentiable inputs (_source_of)."""

    @staticmethod
    def forward(ctx, faces, cfg, src, *inputs):
        r = _forward_impl(cfg, faces, src, inputs)
        owner = cfg.owner()
        if owner is not None:
            owner._keep(r)
        ctx.cfg, ctx.source = cfg, src
        # (the node must not hold its own OUTPUTS except through save_for_backward: output -> grad_fn -> node -> output is a
        # cycle through C++ that nothing collects -- every step's maps would stay allocated)
        ctx.meta = (r.B, r.F, r.S, r.ts, r.Nf, r.flags, r.shared)
        ctx.z_ref, ctx.visible = r.z_ref, r.visible
        ctx.set_materialize_grads(False)  # an unused output arrives as `None` in backward and its terms are skipped
        # residuals (the reference keeps them on `self`, rasterize.py:39-58); outputs and inputs among them go through
        # save_for_backward so that in-place edits by the caller are detected
        ctx.save_for_backward(r.faces, r.face_index_map, r.weight_map, r.depth_map, r.rgb_map, r.alpha_map, *src.saved(r))
        ctx.mark_non_differentiable(r.face_index_map)
        return (r.rgb_map if cfg.return_rgb else None, r.alpha_map if cfg.return_alpha else None,
                r.depth_map if cfg.return_depth else None, r.face_index_map)

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth, _g_fi):
        r = _Residuals()
        r.B, r.F, r.S, r.ts, r.Nf, r.flags, r.shared = ctx.meta
        r.z_ref, r.visible, r.source = ctx.z_ref, ctx.visible, ctx.source
        # (unpacking checks the version counters of the saved tensors: an in-place edit since the forward raises)
        saved = ctx.saved_tensors
        r.faces, r.face_index_map, r.weight_map, r.depth_map, r.rgb_map, r.alpha_map = saved[:6]
        r.source.restore(r, saved[6:])
        gf, grads = _backward_impl(ctx.cfg, r, g_rgb, g_alpha, g_depth, ctx.needs_input_grad[3:])
        return (gf, None, None) + grads


def _capture(fn, dev):
    """Warm `fn` up on a side stream, then capture it (see neural_renderer_amd.graph.capture)."""
    from .graph import capture
    return capture(fn, dev, warmup=2)


class _GraphEntry(object):
    """Fixed buffers + captured graphs of one (device, sizes, configuration) of the operator."""

    def __init__(self, lib, dev, cfg, B, F, S, ts, bg, bg_per_batch):
        self.lib, self.dev, self.cfg = lib, dev, cfg
        f32 = dict(dtype=torch.float32, device=dev)
        # the residuals every replay writes and every backward reads: the eager operator's, in buffers that stay.  The
        # z-buffer is filled by every call (a replayed epoch number would stand still) and weight_map is written densely:
        # `Rasterize.weight_map` hands it out as it is
        r = self.r = _Residuals()
        r.B, r.F, r.S, r.ts, r.Nf, r.source, r.z_ref = B, F, S, ts, F, _CUBES, None
        r.faces = torch.zeros((B, F, 3, 3), **f32)
        r.textures = torch.zeros((B, F, ts, ts, ts, 3), **f32) if cfg.return_rgb else None
        _alloc_maps(r, cfg, dev)
        r.flags = _base_flags(cfg)
        self.background = bg.clone() if bg is not None else None
        self.bg_per_batch = bg_per_batch
        ws_bytes = lib.nr_forward_workspace_bytes(B, F, S)
        if ws_bytes == 0:
            raise ValueError('unsupported sizes B=%d F=%d S=%d' % (B, F, S))
        self.fwd_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        self.generation = 0
        self.pending = None  # generation of the forward whose residuals the buffers hold and whose backward may still come
        self.bwd = {}        # (use_rgb, use_alpha, use_depth, want grad_textures) -> (graph, buffers)
        self.eager_bwd = {}  # the same for combinations the forward did not foresee: (launcher, buffers)
        with torch.cuda.device(dev):
            self.fwd = _capture(self._forward, dev)

    def _forward(self):
        _launch_forward(self.lib, self.cfg, self.r, self.background, self.bg_per_batch, self.r.flags, self.fwd_ws,
                        _stream_ptr(self.dev))

    def _backward_buffers(self, use_rgb, use_alpha, use_depth, want_gt):
        B, F, S, ts = self.r.B, self.r.F, self.r.S, self.r.ts
        f32 = dict(dtype=torch.float32, device=self.dev)
        buf = {'g_rgb': torch.zeros((B, S, S, 3), **f32) if use_rgb else None,
               'g_alpha': torch.zeros((B, S, S), **f32) if use_alpha else None,
               'g_depth': torch.zeros((B, S, S), **f32) if use_depth else None,
               'grad_faces': torch.empty((B, F, 3, 3), **f32),
               'grad_textures': torch.empty((B, F, ts, ts, ts, 3), **f32) if want_gt else None}
        ws_bytes = self.lib.nr_backward_workspace_bytes(B, F, S, int(use_rgb), int(use_alpha))
        buf['ws'] = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=self.dev)

        def run():
            _launch_backward(self.lib, self.cfg, self.r, None, buf['grad_textures'], buf['g_rgb'], buf['g_alpha'],
                             buf['g_depth'], buf['grad_faces'], buf['ws'], ws_bytes, _stream_ptr(self.dev))
        return run, buf

    def prepare_backward(self, key):
        """Capture the backward for one combination of present gradients -- on the CALLER's thread, from the forward: autograd
        runs `backward` on its own device thread, and a graph captured there left the process in a state in which a later
        capture on the main thread crashed (ROCm 7.2 / torch 2.10)."""
        if key not in self.bwd:
            run, buf = self._backward_buffers(*key)
            with torch.cuda.device(self.dev):
                self.bwd[key] = (_capture(run, self.dev), buf)

    def backward_runner(self, key):
        """(callable, buffers): the captured graph when the forward prepared this combination, else plain launches."""
        ent = self.bwd.get(key)
        if ent is None:
            ent = self.eager_bwd.get(key)
            if ent is None:
                ent = self.eager_bwd[key] = self._backward_buffers(*key)
        return ent


_GRAPH_CACHE = {}


def clear_graph_replay_cache():
    """Drop the operator's captured graphs and their fixed buffers (a later call in replay mode captures again)."""
    _GRAPH_CACHE.clear()


@_util.once_differentiable
class _GraphedRasterizeFunction(torch.autograd.Function):
    """The operator replayed from captured graphs (see GRAPH_REPLAY): same results as _RasterizeFunction."""

    @staticmethod
    def forward(ctx, faces, textures, entry):
        cfg, r = entry.cfg, entry.r
        r.faces.copy_(faces.detach())
        if r.textures is not None:
            r.textures.copy_(textures.detach())
        entry.fwd()
        entry.generation += 1
        entry.pending = entry.generation
        ctx.entry, ctx.generation = entry, entry.generation
        ctx.set_materialize_grads(False)
        fi = r.face_index_map.clone()
        ctx.mark_non_differentiable(fi)
        return (r.rgb_map.clone() if cfg.return_rgb else None, r.alpha_map.clone() if cfg.return_alpha else None,
                r.depth_map.clone() if cfg.return_depth else None, fi)

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth, _g_fi):
        entry, cfg = ctx.entry, ctx.entry.cfg
        if entry.generation != ctx.generation:
            raise RuntimeError('graph replay: a later forward of the same shapes has replaced the residual maps of this call; '
                               'run backward before the next forward of these shapes, or switch graph replay off')
        use_rgb = cfg.return_rgb and g_rgb is not None
        use_alpha = cfg.return_alpha and g_alpha is not None
        use_depth = cfg.return_depth and g_depth is not None
        if not (use_rgb or use_alpha or use_depth):
            return None, None, None
        want_gt = bool(use_rgb and ctx.needs_input_grad[1])
        graph, buf = entry.backward_runner((use_rgb, use_alpha, use_depth, want_gt))
        for name, g in (('g_rgb', g_rgb if use_rgb else None), ('g_alpha', g_alpha if use_alpha else None),
                        ('g_depth', g_depth if use_depth else None)):
            if g is not None:
                buf[name].copy_(g)
        graph()
        return buf['grad_faces'].clone(), (buf['grad_textures'].clone() if want_gt else None), None


def _graph_entry(faces, src, inputs, cfg):
    """The cached graphs for this call's device / sizes / configuration, or None when the call is not eligible (replay knows
    batched cubes without face_light only -- one set of cubes shared by the batch runs eagerly --; CPU tensors raise in the eager operator; tensor-valued backgrounds or z references that
    change between calls are handled by value)."""
    if src is not _CUBES or inputs[1] is not None:
        return None
    textures = inputs[0]
    if not faces.is_cuda or faces.dtype != torch.float32 or faces.dim() != 4 or torch.cuda.is_current_stream_capturing():
        return None
    dev = faces.device
    B, F = int(faces.shape[0]), int(faces.shape[1])
    S = cfg.image_size
    ts = 0
    bg, bg_per_batch, bg_key = None, 0, None
    if cfg.return_rgb:
        if textures is None or textures.dim() != 6 or textures.dtype != torch.float32 or tuple(textures.shape[:2]) != (B, F):
            return None
        ts = int(textures.shape[2])
        b = cfg.background_color
        if torch.is_tensor(b):
            return None  # a device-side background may change between calls: eager path
        arr = np.asarray(b, dtype=np.float32)
        if arr.shape == (B, 3):
            bg_per_batch = 1
        elif arr.shape != (3,):
            return None
        bg, bg_key = _background_tensor(b, dev), arr.tobytes()
    if cfg.faces_z_ref is not None:
        return None  # sharded batches hand a reference view over per call: eager path
    key = (dev.index, B, F, S, ts, cfg.return_rgb, cfg.return_alpha, cfg.return_depth, cfg.near, cfg.far, cfg.eps, bg_key,
           bg_per_batch, cfg.fix_batch_z, cfg.exact_gradient)
    entry = _GRAPH_CACHE.get(key)
    if entry is None:
        if len(_GRAPH_CACHE) >= 8:
            _GRAPH_CACHE.pop(next(iter(_GRAPH_CACHE)))
        entry = _GRAPH_CACHE[key] = _GraphEntry(_lib.load(), dev, cfg, B, F, S, ts, bg, bg_per_batch)
    return entry


@_util.once_differentiable
class _ImageEpilogue(torch.autograd.Function):
    """rgb_map [B,S,S,3] -> [B,3,is,is], alpha / depth maps [B,S,S] -> [B,is,is]: NHWC -> NCHW, vertical flip and (with
    anti-aliasing) the 2x2 mean of rasterize.py:953-969, forward and backward each as one kernel (csrc/nr_image.hip)."""

    @staticmethod
    def forward(ctx, rgb_map, alpha_map, depth_map, anti_aliasing):
        maps = [_lib.dense(m.detach()) if m is not None else None for m in (rgb_map, alpha_map, depth_map)]
        ref = next(m for m in maps if m is not None)
        dev = ref.device
        B, S = ref.shape[0], ref.shape[1]
        if anti_aliasing and S % 2:
            raise ValueError('anti-aliasing needs an even raster size, got %d' % S)
        size = S // 2 if anti_aliasing else S
        outs = [None if maps[0] is None else torch.empty((B, 3, size, size), dtype=torch.float32, device=dev),
                None if maps[1] is None else torch.empty((B, size, size), dtype=torch.float32, device=dev),
                None if maps[2] is None else torch.empty((B, size, size), dtype=torch.float32, device=dev)]
        _lib.launch('nr_image_epilogue', dev, _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.ptr(maps[2]), _lib.ptr(outs[0]),
                    _lib.ptr(outs[1]), _lib.ptr(outs[2]), B, S, int(anti_aliasing))
        ctx.dims = (B, S, bool(anti_aliasing))
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth):
        B, S, aa = ctx.dims
        grads = [_lib.dense(g) for g in (g_rgb, g_alpha, g_depth)]
        ref = next((g for g in grads if g is not None), None)
        if ref is None:
            return None, None, None, None
        dev = ref.device
        # an output without gradient keeps `None`, so that the rasterizer's backward skips its terms altogether
        outs = [None if grads[0] is None else torch.empty((B, S, S, 3), dtype=torch.float32, device=dev),
                None if grads[1] is None else torch.empty((B, S, S), dtype=torch.float32, device=dev),
                None if grads[2] is None else torch.empty((B, S, S), dtype=torch.float32, device=dev)]
        _lib.launch('nr_image_epilogue_backward', dev, _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]),
                    _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), B, S, int(aa))
        return outs[0], outs[1], outs[2], None


class Rasterize(object):
    """Same constructor and call convention as the reference's `Rasterize` chainer.Function
    (rasterize.py:19-64): `Rasterize(...)(faces[, textures]) -> (rgb, alpha, depth)` in the internal
    layout (rgb [B,S,S,3], alpha/depth [B,S,S], row 0 = bottom), `None` for outputs not requested.
    The intermediate maps of the last call stay on the instance like in the reference (:54-58).

    Two ways in, as on a chainer.Function:
      fn(faces, textures)                          the differentiable call (torch.autograd.Function underneath)
      fn.forward_gpu((faces, textures)), fn.backward_gpu(inputs, grad_outputs)
                                                   the Function protocol itself (rasterize.py:467, :849), no autograd graph:
                                                   what Chainer calls on the reference.  Same kernels, same results; at small
                                                   batches the direct calls save torch's autograd hand-over to its device
                                                   thread, which costs more host time than the launches."""

    def __init__(self, image_size, near, far, eps, background_color, return_rgb=False, return_alpha=False,
                 return_depth=False):
        if not any((return_rgb, return_alpha, return_depth)):
            # nothing to draw (rasterize.py:25-27 raises a bare Exception)
            raise Exception('nothing to draw: none of return_rgb / return_alpha / return_depth is set')
        self.image_size = image_size
        self.near = near
        self.far = far
        self.eps = eps
        self.background_color = background_color
        self.return_rgb = return_rgb
        self.return_alpha = return_alpha
        self.return_depth = return_depth
        self.fix_batch_z = FIX_TEXTURE_BATCH_Z
        self.exact_gradient = EXACT_GRADIENT
        self.graph_replay = GRAPH_REPLAY  # replay the operator from captured HIP graphs (fixed shapes; see GRAPH_REPLAY)
        # [F,3,3] faces of the global batch element 0 when this call renders a shard of a larger batch (SURVEY Q1:
        # the reference samples textures with batch element 0's depths); None = element 0 of this call
        self.faces_z_ref = None
        # buffers of the last call, as on the reference's Function (rasterize.py:39-64).  The reference also keeps
        # face_inv_map and the two sampling maps; the kernels here recompute them instead of storing them, so
        # those three are properties that run the per-stage entry point with the optional pointers when somebody reads them.
        self.faces = self.textures = None
        self.grad_rgb_map = self.grad_alpha_map = self.grad_depth_map = None
        self.rgb_map = self.alpha_map = self.depth_map = None
        self.grad_faces = self.grad_textures = None
        self.face_index_map = None
        self.batch_size = self.num_faces = self.texture_size = None
        self._res = None    # residuals of the last forward (forward_gpu / backward_gpu protocol, lazy maps)
        self._lazy = {}

    # ---- the buffers of the last call (rasterize.py:39-58)
    def _keep(self, r):
        self._res = r
        self._lazy = {}
        self.faces, self.textures = r.faces, r.textures
        self.face_index_map, self.depth_map = r.face_index_map, r.depth_map
        self.rgb_map, self.alpha_map = r.rgb_map, r.alpha_map
        self.batch_size, self.num_faces = r.B, r.F
        self.texture_size = r.ts if self.return_rgb else None

    def _lazy_maps(self, which):
        """face_inv_map [B,S,S,3,3] (rasterize.py:57) or the sampling maps [B,S,S,8] (:47-48) of the last call: not kept by
        the kernels (they recompute them), so reading one runs the per-stage entry point with the optional output pointers."""
        if which in self._lazy:
            return self._lazy[which]
        r = self._res
        if r is None:
            return None
        lib = _lib.load()
        dev = r.faces.device
        B, F, S, ts = r.B, r.F, r.S, r.ts
        f32 = torch.float32
        with _on_device(dev):
            stream = _stream_ptr(dev)
            if which == 'face_inv_map':
                out = torch.empty((B, S, S, 3, 3), dtype=f32, device=dev)
                ws_bytes = lib.nr_forward_workspace_bytes(B, F, S)
                ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
                fi = torch.empty_like(r.face_index_map)
                wm = torch.empty((B, S, S, 3), dtype=f32, device=dev)
                dm = torch.empty((B, S, S), dtype=f32, device=dev)
                _lib.check(lib.nr_forward_face_index_map(r.faces.data_ptr(), fi.data_ptr(), wm.data_ptr(), dm.data_ptr(),
                                                         out.data_ptr(), None, B, F, S, float(self.near), float(self.far),
                                                         ws.data_ptr(), ws_bytes, stream), 'nr_forward_face_index_map')
                self._lazy['face_inv_map'] = out
            else:
                if r.textures is None or r.light is not None or r.shared:
                    # no texture sampling in this call (or per-face light colours: no reference counterpart; or one set of
                    # cubes for the batch: the staged pass strides the cubes by the batch)
                    return None
                si = torch.empty((B, S, S, 8), dtype=torch.int32, device=dev)
                sw = torch.empty((B, S, S, 8), dtype=f32, device=dev)
                rgb = torch.empty((B, S, S, 3), dtype=f32, device=dev)
                bg = self.background_color if self.background_color is not None else DEFAULT_BACKGROUND_COLOR
                bg = _lib.dense(bg.detach().to(device=dev, dtype=f32)) if torch.is_tensor(bg) else _background_tensor(bg, dev)
                wm = _lib.dense(self.weight_map)  # (the attribute may have been assigned by the caller)
                _lib.check(lib.nr_forward_texture_sampling(
                    r.faces.data_ptr(), _lib.ptr(r.z_ref), r.textures.data_ptr(), r.face_index_map.data_ptr(),
                    wm.data_ptr(), r.depth_map.data_ptr(), rgb.data_ptr(), si.data_ptr(), sw.data_ptr(), bg.data_ptr(),
                    int(tuple(bg.shape) == (B, 3)), None, B, F, S, ts, float(self.eps), r.flags, stream),
                    'nr_forward_texture_sampling')
                self._lazy['sampling_index_map'], self._lazy['sampling_weight_map'] = si, sw
        return self._lazy[which]

    def _get_weight_map(self):
        """weight_map [B,S,S,3] of the last call (rasterize.py:43): the forward stores the weights of covered pixels only; the
        zeros of the others (:479) are filled in here, once, when the attribute is read."""
        if 'weight_map' not in self._lazy:
            r = self._res
            if r is None or r.weight_map is None:
                return None
            self._lazy['weight_map'] = torch.where((r.face_index_map >= 0).unsqueeze(-1), r.weight_map,
                                                   torch.zeros((), dtype=r.weight_map.dtype, device=r.weight_map.device))
        return self._lazy['weight_map']

    def _set_weight_map(self, value):
        self._lazy['weight_map'] = value

    weight_map = property(_get_weight_map, _set_weight_map)
    face_inv_map = property(lambda self: self._lazy_maps('face_inv_map'))
    sampling_index_map = property(lambda self: self._lazy_maps('sampling_index_map'))
    sampling_weight_map = property(lambda self: self._lazy_maps('sampling_weight_map'))

    # ---- the chainer.Function protocol of the reference (rasterize.py:467-513, :849-889)
    def forward_gpu(self, inputs, face_light=None):
        """inputs = (faces,) or (faces, textures) -> (rgb_map, alpha_map, depth_map), `None` for outputs not requested.  Keeps
        the maps on the instance for backward_gpu.  No autograd graph is recorded."""
        faces = inputs[0]
        textures = inputs[1] if len(inputs) > 1 and self.return_rgb else None
        r = _forward_impl(_Config(self), faces, *_source_of(textures, face_light if self.return_rgb else None, protocol=True))
        self._keep(r)
        return (r.rgb_map if self.return_rgb else None, r.alpha_map if self.return_alpha else None,
                r.depth_map if self.return_depth else None)

    forward = forward_gpu

    def backward_gpu(self, inputs, grad_outputs):
        """grad_outputs = (grad_rgb_map, grad_alpha_map, grad_depth_map), `None` = zeros (rasterize.py:858-878) ->
        (grad_faces,) or (grad_faces, grad_textures) like :886-889; with face_light also grad_light (third).  `inputs` is
        accepted for the protocol's sake: the residuals of the last forward_gpu are what is used."""
        r = self._res
        _source_of(inputs[1] if len(inputs) > 1 else None, None, protocol=True)
        if r is None:
            raise RuntimeError('backward_gpu before forward_gpu')
        if r.source is not _CUBES:  # (the last forward was the instance's own call)
            _no_protocol(r.source.name)
        g_rgb, g_alpha, g_depth = (tuple(grad_outputs) + (None, None, None))[:3]
        gf, (gt, gl) = _backward_impl(_Config(self), r, g_rgb, g_alpha, g_depth, (self.return_rgb, r.light is not None))
        if gf is None:  # no gradient at all: zeros (:851-853)
            gf = torch.zeros_like(r.faces)
        if not self.return_rgb or len(inputs) < 2:
            return (gf,)
        if gt is None:
            gt = torch.zeros_like(r.textures)
        return (gf, gt) if r.light is None else (gf, gt, gl)

    backward = backward_gpu

    def __call__(self, faces, textures=None, face_light=None):
        """`face_light` (not in the reference; include/nr_hip.h nr_face_light): [B,F,3] colours that multiply the sampled
        colour of each face; `textures` are then the cubes of the original faces ([B,F,...], or [B,F/2,...] when the second
        half of `faces` are fill_back's reversed copies).  Cubes with a batch of 1 beside B > 1 faces (not in the reference) are
        one set shared by the batch: no expanded copy, and their gradient comes back summed over the images, [1,...]; the
        call runs eagerly, and the sampling maps read as None.  `textures` may be a UVImages (not in the reference): the images are
        sampled at every covered pixel; `face_light` is then required, `faces` has the layout's faces (or twice as many with
        fill_back), and the call runs eagerly whatever graph_replay says."""
        cfg = _Config(self)
        if not self.return_rgb:
            textures = face_light = None
        src, inputs = _source_of(textures, face_light)
        if self.graph_replay:
            entry = _graph_entry(faces, src, inputs, cfg)
            if entry is not None:
                if torch.is_grad_enabled() and (faces.requires_grad or (textures is not None and textures.requires_grad)):
                    # the usual case: every requested output receives a gradient
                    entry.prepare_backward((bool(self.return_rgb), bool(self.return_alpha), bool(self.return_depth),
                                            bool(self.return_rgb and textures is not None and textures.requires_grad)))
                rgb, alpha, depth, fi = _GraphedRasterizeFunction.apply(faces, textures, entry)
                self._res, self._lazy = None, {}
                r = entry.r
                self.faces, self.textures, self.weight_map = r.faces, r.textures, r.weight_map  # (dense there)
                self.depth_map = depth if depth is not None else r.depth_map
                self.rgb_map, self.alpha_map, self.face_index_map = rgb, alpha, fi
                self.batch_size, self.num_faces = r.B, r.F
                self.texture_size = r.ts if self.return_rgb else None
                return rgb, alpha, depth
        rgb, alpha, depth, _ = _RasterizeFunction.apply(faces, cfg, src, *inputs)
        return rgb, alpha, depth


def rasterize_rgbad(
        faces,
        textures=None,
        image_size=DEFAULT_IMAGE_SIZE,
        anti_aliasing=DEFAULT_ANTI_ALIASING,
        near=DEFAULT_NEAR,
        far=DEFAULT_FAR,
        eps=DEFAULT_EPS,
        background_color=DEFAULT_BACKGROUND_COLOR,
        return_rgb=True,
        return_alpha=True,
        return_depth=True,
        faces_z_ref=None,
        graph_replay=None,
        face_light=None,
):
    """RGB, alpha and depth images from faces (and textures for RGB) -- reference rasterize.py:900-977.

    Returns a dict with 'rgb' [B, 3, image_size, image_size], 'alpha' and 'depth' [B, image_size, image_size]
    (None when not requested).  `faces_z_ref` (not in the reference): see Rasterize.faces_z_ref; `face_light` (not in the
    reference): see Rasterize.__call__; `textures` may be a UVImages (not in the reference), with `face_light`, or a
    CornerColors (not in the reference; vertex_colors.py), without."""
    inputs = [faces] if textures is None else [faces, textures, face_light]
    size = image_size * 2 if anti_aliasing else image_size  # 2x super-sampling, :945-951
    fn = Rasterize(size, near, far, eps, background_color, return_rgb, return_alpha, return_depth)
    fn.faces_z_ref = faces_z_ref
    if graph_replay is not None:
        fn.graph_replay = bool(graph_replay)
    rgb, alpha, depth = fn(*inputs)
    # transpose & vertical flip (:953-960) and 0.5x down-sampling (:962-969): one HIP kernel per direction
    rgb, alpha, depth = _ImageEpilogue.apply(rgb, alpha, depth, bool(anti_aliasing))
    return {
        'rgb': rgb if return_rgb else None,
        'alpha': alpha if return_alpha else None,
        'depth': depth if return_depth else None,
    }


def rasterize(
        faces,
        textures,
        image_size=DEFAULT_IMAGE_SIZE,
        anti_aliasing=DEFAULT_ANTI_ALIASING,
        near=DEFAULT_NEAR,
        far=DEFAULT_FAR,
        eps=DEFAULT_EPS,
        background_color=DEFAULT_BACKGROUND_COLOR,
        faces_z_ref=None,
        graph_replay=None,
        face_light=None,
):
    """RGB images [B, 3, image_size, image_size] -- reference rasterize.py:980-1008."""
    return rasterize_rgbad(
        faces, textures, image_size, anti_aliasing, near, far, eps, background_color, True, False, False,
        faces_z_ref=faces_z_ref, graph_replay=graph_replay, face_light=face_light)['rgb']


def rasterize_silhouettes(
        faces,
        image_size=DEFAULT_IMAGE_SIZE,
        anti_aliasing=DEFAULT_ANTI_ALIASING,
        near=DEFAULT_NEAR,
        far=DEFAULT_FAR,
        eps=DEFAULT_EPS,
        graph_replay=None,
):
    """Alpha channels [B, image_size, image_size] -- reference rasterize.py:1011-1034."""
    return rasterize_rgbad(faces, None, image_size, anti_aliasing, near, far, eps, None, False, True, False,
                           graph_replay=graph_replay)['alpha']


def rasterize_depth(
        faces,
        image_size=DEFAULT_IMAGE_SIZE,
        anti_aliasing=DEFAULT_ANTI_ALIASING,
        near=DEFAULT_NEAR,
        far=DEFAULT_FAR,
        eps=DEFAULT_EPS,
        graph_replay=None,
):
    """Depth images [B, image_size, image_size] -- reference rasterize.py:1037-1060."""
    return rasterize_rgbad(faces, None, image_size, anti_aliasing, near, far, eps, None, False, False, True,
                           graph_replay=graph_replay)['depth']


def use_unsafe_rasterizer(flag):
    """Kept for API compatibility (rasterize.py:1063-1065, env NEURAL_RENDERER_UNSAFE :15-16).  The reference's "unsafe"
    kernel (K3, :102-236) is a per-face scan conversion with a per-pixel spin lock: same coverage and face indices as
    the safe path, an order-dependent tie rule and weights that differ at the 1e-4 level.  The face-parallel
    rasterizer here already is O(sum of screen boxes) -- what K3 buys the reference -- and deterministic, so both settings
    run it and give bit-identical outputs (tests/test_hip_parity.py::test_unsafe_rasterizer_flag_is_equivalent)."""
    global USE_UNSAFE_IMPLEMENTATION
    USE_UNSAFE_IMPLEMENTATION = flag
