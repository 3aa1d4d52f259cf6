"""Learnable UV texture images (not in the reference): the texture bake of load_obj(load_texture=True) as a differentiable step.

`UVLayout.from_obj` reads a mesh's uv triangles, materials and texture images (the parsing of load_textures, no GPU);
`bake_uv_textures(images, layout)` turns the images into the [Bi,F,ts,ts,ts,3] textures Renderer.render samples, and its
backward hands the texture gradient back to the image pixels; `UVImages(layout, images)` hands Renderer.render the images
themselves, sampled at every covered pixel (include/nr_hip.h: nr_forward_rasterize_uv); `UVTextures` holds one learnable
image per textured material and writes the result back out as OBJ / MTL / PNG in the mesh's own uv layout.

Both directions are HIP kernels (csrc/nr_texture_io.hip, include/nr_hip.h: nr_bake_uv_textures[_backward]); the inverse
map the backward walks (nr_uv_texture_map) is built on the device on the first backward and cached on the layout.
Texel (0,0,0) differs from load_obj on purpose: there the reference divides 0 by 0, here it is the lookup at the uv centroid.
"""
import os

import numpy as np
import torch

from . import _lib, _util
from .load_obj import parse_textures, read_texture_image


class UVLayout(object):
    """How a mesh's F faces sample its M texture images: faces_uv [F,3,2] float32 (values above 1 wrapped, as load_obj),
    face_image [F] int32 (index of the image a face samples, or -1), base [F,ts,ts,ts,3] float32 (the texels of faces
    without an image: their Kd colour or 0.5), image_sizes [(H_m, W_m)].  `images` holds the images read from the files
    ([H,W,3] float32 in [0,1], top row first), `materials` the material name of every face, `colors` the Kd colours and
    `image_materials` the material of each image (what save_obj writes)."""

    def __init__(self, faces_uv, face_image, base, image_sizes, images=None, materials=None, colors=None,
                 image_materials=None):
        faces_uv = np.ascontiguousarray(faces_uv, np.float32)
        face_image = np.ascontiguousarray(face_image, np.int32)
        base = np.ascontiguousarray(base, np.float32)
        num_faces = faces_uv.shape[0]
        if faces_uv.shape != (num_faces, 3, 2) or face_image.shape != (num_faces,) or base.ndim != 5 or \
                base.shape[0] != num_faces or base.shape[4] != 3 or not base.shape[1] == base.shape[2] == base.shape[3]:
            raise ValueError('UVLayout: faces_uv [F,3,2], face_image [F] and base [F,ts,ts,ts,3] expected')
        if base.shape[1] < 2:
            raise ValueError('UVLayout: texture_size must be at least 2')
        self.image_sizes = [(int(h), int(w)) for h, w in image_sizes]
        if any(h < 1 or w < 1 for h, w in self.image_sizes):
            raise ValueError('UVLayout: image sizes must be positive')
        if ((face_image < -1) | (face_image >= len(self.image_sizes))).any():
            raise ValueError('UVLayout: face_image must be -1 or the index of an image')
        self.faces_uv = faces_uv
        self.face_image = face_image
        self.base = base
        self.images = images
        self.materials = materials
        self.colors = colors
        self.image_materials = image_materials
        offsets = np.cumsum([0] + [h * w for h, w in self.image_sizes])
        self.num_pixels = int(offsets[-1])
        if self.num_pixels >= 2 ** 31 - 1:
            raise ValueError('UVLayout: too many image pixels')
        self.image_table = np.array([(offsets[m], h, w) for m, (h, w) in enumerate(self.image_sizes)],
                                    np.int32).reshape(-1, 3)
        self._device = {}  # device -> tensors of the layout (+ the inverse map once built)

    @property
    def num_faces(self):
        return self.faces_uv.shape[0]

    @property
    def num_images(self):
        return len(self.image_sizes)

    @property
    def texture_size(self):
        return self.base.shape[1]

    @classmethod
    def from_obj(cls, filename_obj, texture_size=4):
        """The layout of an OBJ file with an MTL library (the last `mtllib`, as load_obj): one image per material with a
        `map_Kd`, in the MTL's order.  Host only: no GPU needed."""
        filename_mtl = None
        with open(filename_obj) as f:
            for line in f:
                if line.startswith('mtllib'):
                    filename_mtl = os.path.join(os.path.dirname(filename_obj), line.split()[1])
        if filename_mtl is None:
            raise ValueError('%s names no mtllib' % filename_obj)
        faces_uv, materials, colors, texture_filenames, base = parse_textures(filename_obj, filename_mtl, texture_size)
        face_image = np.full(faces_uv.shape[0], -1, np.int32)
        images, image_materials = [], []
        for m, (name, filename_texture) in enumerate(texture_filenames.items()):
            face_image[materials == name] = m
            images.append(read_texture_image(filename_obj, filename_texture))
            image_materials.append(name)
        return cls(faces_uv, face_image, base, [im.shape[:2] for im in images], images, materials, colors, image_materials)

    def _tensors(self, device):
        state = self._device.get(device)
        if state is None:
            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a)).to(device)
            state = dict(faces_uv=up(self.faces_uv), face_image=up(self.face_image),
                         base=up(self.base.reshape(self.num_faces, -1, 3)), table=up(self.image_table))
            self._device[device] = state
        return state

    def inverse_map(self, device):
        """(row_ptr [P+1], entry_texel, entry_weight) on `device`: built by nr_uv_texture_map on first use, then cached.
        The build is one launch on the stream that is current at that moment; a later call on ANOTHER stream waits for it
        (an event, dropped once it has passed), so that the tables are never read ahead of the kernel that writes them.
        (Inside a graph capture nothing is waited for: a capture needs an eager call in front of it anyway.)"""
        state = self._tensors(device)
        if 'row_ptr' not in state:
            lib = _lib.load()
            F, ts, M, P = self.num_faces, self.texture_size, self.num_images, self.num_pixels
            n = 4 * F * ts ** 3
            with torch.cuda.device(device):
                wsb = lib.nr_uv_texture_map_workspace_bytes(F, ts, M, P)
                if wsb == 0:
                    raise _lib.NRError('nr_uv_texture_map_workspace_bytes: layout out of range (F=%d ts=%d P=%d)' % (F, ts, P))
                stream = torch.cuda.current_stream(device)
                ws = torch.empty(wsb, dtype=torch.uint8, device=device)
                # (zeros, once per layout: whatever reads the tables out of order finds empty rows, not stale indices)
                row_ptr = torch.zeros(P + 1, dtype=torch.int32, device=device)
                entry_texel = torch.zeros(n, dtype=torch.int32, device=device)
                entry_weight = torch.zeros(n, dtype=torch.float32, device=device)
                _lib.check(lib.nr_uv_texture_map(state['table'].data_ptr(), state['faces_uv'].data_ptr(),
                                                 state['face_image'].data_ptr(), row_ptr.data_ptr(), entry_texel.data_ptr(),
                                                 entry_weight.data_ptr(), F, ts, M, P, ws.data_ptr(), wsb,
                                                 stream.cuda_stream), 'nr_uv_texture_map')
                built = torch.cuda.Event()
                built.record(stream)
            state.update(row_ptr=row_ptr, entry_texel=entry_texel, entry_weight=entry_weight, workspace=ws,
                         built=(built, stream.cuda_stream))
        elif state.get('built') is not None and not torch.cuda.is_current_stream_capturing():
            built, on = state['built']
            if built.query():
                state['built'] = None
            else:
                stream = torch.cuda.current_stream(device)
                if stream.cuda_stream != on:
                    stream.wait_event(built)
        return state['row_ptr'], state['entry_texel'], state['entry_weight']


def check_images(images, layout, who):
    """The images of a layout as bake_uv_textures and UVImages take them: a list of float32 CUDA tensors on one device, top
    row first, image m [H_m,W_m,3] (shared by the batch) or [Bi,H_m,W_m,3].  Returns (list, Bi or None when none is
    batched); raises ValueError."""
    if not isinstance(layout, UVLayout):
        raise ValueError('%s: layout must be a UVLayout' % who)
    if torch.is_tensor(images):
        images = [images]
    images = list(images)
    if len(images) != layout.num_images or layout.num_images == 0:
        raise ValueError('%s: the layout has %d images, %d given' % (who, layout.num_images, len(images)))
    batch = None
    for m, (im, (h, w)) in enumerate(zip(images, layout.image_sizes)):  # shapes first: checkable without a GPU
        if not torch.is_tensor(im) or im.dim() not in (3, 4) or tuple(im.shape[-3:]) != (h, w, 3):
            raise ValueError('%s: image %d must be a tensor [%d,%d,3] or [Bi,%d,%d,3], got %s'
                             % (who, m, h, w, h, w, tuple(im.shape) if torch.is_tensor(im) else type(im).__name__))
        if im.dim() == 4:
            if im.shape[0] < 1 or (batch is not None and im.shape[0] != batch):
                raise ValueError('%s: batched images must share one batch size' % who)
            batch = im.shape[0]
    for m, im in enumerate(images):
        if not im.is_cuda or im.dtype != torch.float32:
            raise ValueError('%s: image %d must be a float32 CUDA tensor' % (who, m))
        if im.device != images[0].device:
            raise ValueError('%s: all images must be on one device' % who)
    return images, batch


def pack_images(images, batch):
    """[Bi,P,3] contiguous (Bi = batch or 1): the images one after another, the unbatched ones repeated for every element
    when others are batched -- the packing the kernels read (include/nr_hip.h: images [Bi,P,3])."""
    Bi = batch or 1
    flat = [(im if im.dim() == 4 else im[None].expand(Bi, -1, -1, -1)).reshape(Bi, -1, 3) for im in images]
    return _lib.dense(flat[0] if len(flat) == 1 else torch.cat(flat, 1))


def unpack_image_gradients(layout, grad_packed):
    """A gradient of pack_images' packing [Bi,P,3] as one view [Bi,H_m,W_m,3] per image of the layout."""
    Bi = grad_packed.shape[0]
    return [grad_packed[:, off:off + h * w].view(Bi, h, w, 3) for off, h, w in layout.image_table.tolist()]


@_util.once_differentiable
class _BakeUV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layout, *images):
        device = images[0].device
        Bi = images[0].shape[0]
        packed = pack_images(images, Bi)
        state = layout._tensors(device)
        F, ts = layout.num_faces, layout.texture_size
        textures = torch.empty((Bi, F, ts, ts, ts, 3), dtype=torch.float32, device=device)
        _lib.launch('nr_bake_uv_textures', device, packed.data_ptr(), state['table'].data_ptr(), state['faces_uv'].data_ptr(),
                    state['face_image'].data_ptr(), state['base'].data_ptr(), textures.data_ptr(), Bi, F, ts,
                    layout.num_images, layout.num_pixels)
        ctx.layout = layout
        ctx.batch = Bi
        ctx.device = device
        return textures

    @staticmethod
    def backward(ctx, grad_textures):
        layout, Bi, device = ctx.layout, ctx.batch, ctx.device
        row_ptr, entry_texel, entry_weight = layout.inverse_map(device)
        grad_textures = _lib.dense(grad_textures)
        P = layout.num_pixels
        grad_packed = torch.empty((Bi, P, 3), dtype=torch.float32, device=device)
        _lib.launch('nr_bake_uv_textures_backward', device, grad_textures.data_ptr(), row_ptr.data_ptr(), entry_texel.data_ptr(),
                    entry_weight.data_ptr(), grad_packed.data_ptr(), Bi, layout.num_faces, layout.texture_size, P)
        return (None,) + tuple(unpack_image_gradients(layout, grad_packed))


def bake_uv_textures(images, layout):
    """textures [Bi,F,ts,ts,ts,3] from the layout's M images (a list of float32 CUDA tensors in file orientation, top row
    first, each [H_m,W_m,3] or [Bi,H_m,W_m,3]; unbatched ones are shared by the batch).  Differentiable in the images.
    Equal to load_obj(load_texture=True)'s bake of the same images bit for bit, except at texel (0,0,0) (the uv centroid
    here, NaN there).  For one image shared by a batch of B renders, use bake_uv_textures(...)[0:1].expand(B, ...)."""
    images, batch = check_images(images, layout, 'bake_uv_textures')
    batch = batch or 1
    images = [im if im.dim() == 4 else im[None].expand(batch, -1, -1, -1) for im in images]
    return _BakeUV.apply(layout, *images)


class UVImages(object):
    """A UV layout's images for per-pixel sampling: Renderer.render(vertices, faces, UVImages(layout, images)) and
    rasterize(faces, UVImages(...), ..., face_light=...) sample the images at every covered pixel with the bake's bilinear
    lookup (include/nr_hip.h: nr_forward_rasterize_uv) instead of baking them into texture cubes first.  `images` as
    bake_uv_textures takes them: a list of float32 CUDA tensors, top row first, [H_m,W_m,3] shared by the batch or
    [B,H_m,W_m,3] per render.  Gradients reach every image tensor; faces_uv and base (the colour of faces without an
    image, sampled as a cube) receive none.  Holds references, no copies: build one per step, or keep one whose tensors
    are updated in place."""

    def __init__(self, layout, images):
        self.images, self.batch = check_images(images, layout, 'UVImages')
        self.layout = layout

    @property
    def image_batch(self):
        """1 when every image is shared by the batch, else the batch size of the batched images."""
        return self.batch or 1

    @property
    def device(self):
        return self.images[0].device


class UVTextures(torch.nn.Module):
    """One learnable image per textured material of a UVLayout (initialised from the files), baked for Renderer.render."""

    def __init__(self, layout):
        super(UVTextures, self).__init__()
        if layout.images is None:
            raise ValueError('UVTextures: the layout carries no images (use UVLayout.from_obj)')
        self.layout = layout
        self.images = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(np.array(im, np.float32)))
                                              for im in layout.images])

    def forward(self, batch_size=1):
        """textures [batch_size,F,ts,ts,ts,3]: the bake of the images, shared by the batch."""
        textures = bake_uv_textures(list(self.images), self.layout)
        return textures[0:1].expand(batch_size, -1, -1, -1, -1, -1)

    def uv_images(self):
        """The images as a UVImages (shared by the batch): Renderer.render samples them per pixel."""
        return UVImages(self.layout, list(self.images))

    def save_obj(self, filename, vertices, faces):
        """Writes `filename` (one `vt` per face corner, `usemtl` runs), `<stem>.mtl` (Kd and map_Kd) and the learned images
        as 8-bit PNGs `<stem>_<m>.png` (clamped to [0,1], top row first), so that load_obj(load_texture=True) reads them
        back: its textures equal the bake of the images rounded to 8 bits (texel (0,0,0) aside)."""
        from PIL import Image
        layout = self.layout
        vertices = _numpy(vertices)
        faces = _numpy(faces)
        if vertices.ndim != 2 or faces.ndim != 2 or faces.shape != (layout.num_faces, 3):
            raise ValueError('save_obj: vertices [V,3] and faces [F,3] of the layout expected')
        stem = filename[:-4] if filename.endswith('.obj') else filename
        base = os.path.basename(stem)
        materials = layout.materials if layout.materials is not None else \
            np.array(['image_%d' % m if m >= 0 else '' for m in layout.face_image])
        names = {}   # material -> name written (the reference's unnamed material '' gets one)
        for name in materials:
            if name not in names:
                names[name] = name if name else 'default_material'
        colors = layout.colors or {}
        image_of = dict(zip(layout.image_materials or ['image_%d' % m for m in range(layout.num_images)],
                            range(layout.num_images)))
        with open(stem + '.mtl', 'w') as f:
            for name, out_name in names.items():
                kd = colors.get(name, np.float32([0.5, 0.5, 0.5]))
                f.write('newmtl %s\nKd %.9g %.9g %.9g\n' % ((out_name,) + tuple(np.float32(kd).tolist())))
                if name in image_of:
                    m = image_of[name]
                    png = '%s_%d.png' % (base, m)
                    image = self.images[m].detach()
                    image = image.reshape(image.shape[-3:]).cpu().numpy()
                    Image.fromarray(quantize(image)).save(os.path.join(os.path.dirname(stem) or '.', png))
                    f.write('map_Kd %s\n' % png)
                f.write('\n')
        out = ['mtllib %s.mtl\n' % base]
        out += ['v %.9g %.9g %.9g\n' % tuple(v) for v in vertices.tolist()]
        out += ['vt %.9g %.9g\n' % tuple(t) for t in layout.faces_uv.reshape(-1, 2).tolist()]
        current = None
        for i, (a, b, c) in enumerate(faces.tolist()):
            if materials[i] != current:
                current = materials[i]
                out.append('usemtl %s\n' % names[current])
            out.append('f %d/%d %d/%d %d/%d\n' % (a + 1, 3 * i + 1, b + 1, 3 * i + 2, c + 1, 3 * i + 3))
        with open(filename, 'w') as f:
            f.writelines(out)


def quantize(image):
    """[H,W,3] float in [0,1] -> uint8: clamp, scale by 255, round half up (what save_obj writes)."""
    return np.floor(np.clip(np.asarray(image, np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def _numpy(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a)
