"""Renderer facade -- reference neural_renderer/renderer.py:8-107 (same attributes, defaults and methods).

On CUDA tensors with the usual parameter types the chain in front of the rasterizer (fill_back, lighting, look_at / look,
perspective, vertices_to_faces) runs as one fused HIP kernel per direction (frontend.py); any other input keeps the
module-by-module path below, which mirrors the reference line by line.  camera_mode = 'projection' (a calibrated camera:
K, R, t, dist_coeffs, orig_size; projection.py) is not in the reference."""
import math
import os
import sys

import torch

from . import frontend
from .lighting import lighting
from .lights import light_colors
from .look import look
from .look_at import look_at
from .normals import camera_rotation, corner_normals
from .perspective import perspective
from .projection import projection
from .rasterize import rasterize, rasterize_depth, rasterize_rgbad, rasterize_silhouettes
from .soft_render import TextureCubes, soft_render, soft_render_cubes, soft_render_uv
from .soft_silhouette import soft_silhouettes
from .uv_textures import UVImages
from .vertex_colors import CornerColors, VertexColors, vertex_light, vertex_shade
from .vertices_to_faces import vertices_to_faces

# Renderer.face_light default (see the attribute): NR_FACE_LIGHT = 0 | 1 | auto
FACE_LIGHT = {'0': False, '1': True}.get(os.environ.get('NR_FACE_LIGHT', 'auto'))


def check_projection(renderer):
    """camera_mode = 'projection' needs K, R, t and orig_size."""
    missing = [n for n in ('K', 'R', 't', 'orig_size') if getattr(renderer, n) is None]
    if missing:
        raise ValueError("camera_mode 'projection' needs Renderer.%s" % ', '.join(missing))


class Renderer(object):
    def __init__(self):
        # rendering
        self.image_size = 256
        self.anti_aliasing = True
        self.background_color = [0, 0, 0]
        self.fill_back = True

        # camera
        self.perspective = True
        self.viewing_angle = 30
        self.eye = [0, 0, -(1. / math.tan(math.radians(self.viewing_angle)) + 1)]
        self.camera_mode = 'look_at'
        self.camera_direction = [0, 0, 1]
        self.near = 0.1
        self.far = 100
        # not in the reference: camera_mode = 'projection' -- a calibrated camera (projection.py): intrinsics K, pose R | t
        # (world -> camera), OpenCV dist_coeffs (None = no distortion) and the size of the image K refers to.  Lists,
        # arrays or (learnable) tensors, shared by the batch or one per image, like `eye`.  The mode ignores `perspective`
        # and `viewing_angle`.
        self.K = None
        self.R = None
        self.t = None
        self.dist_coeffs = None
        self.orig_size = None

        # light
        self.light_intensity_ambient = 0.5
        self.light_intensity_directional = 0.5
        self.light_color_ambient = [1, 1, 1]  # white
        self.light_color_directional = [1, 1, 1]  # white
        self.light_direction = [0, 1, 0]  # up-to-down

        # rasterization
        self.rasterizer_eps = 1e-3

        # not in the reference: which implementation of the chain in front of the rasterizer the calls took -- 'fused'
        # (one HIP kernel per direction, frontend.py) or 'torch' (module by module).  A benchmark asserts on this so that it
        # cannot fall onto the ~160-launch path unnoticed.
        self.last_frontend = None
        self.frontend_calls = {'fused': 0, 'torch': 0}
        # [F,3,3] faces of the global batch element 0 when this renderer draws a shard of a larger batch
        self.faces_z_ref = None
        # not in the reference: replay the rasterizer from captured HIP graphs (fixed shapes; None = the module default,
        # neural_renderer_amd.use_graph_replay / NR_GRAPH_REPLAY; see rasterize.py)
        self.graph_replay = None
        # not in the reference: render() hands the rasterizer the ORIGINAL textures plus one light colour per face instead of
        # lit, fill_back-duplicated textures (include/nr_hip.h: nr_face_light).  Same images up to the rounding
        # order of the light product (measured 3e-7 of the largest colour, tests/test_face_light_gpu.py), a fraction of the
        # memory traffic on textured meshes (scripts/face_light_timing.py: config 4's shape 2.20 -> 1.12 ms per render +
        # backward at texture_size 4, 16.3 -> 1.85 ms at 8; neutral at 2).  True / False, or None = when it pays
        # (texture_size >= 3).  Needs the fused front-end and no graph replay; otherwise, and with False,
        # the lit-texture path runs.  Default: NR_FACE_LIGHT (auto).
        self.face_light = FACE_LIGHT
        # not in the reference: where render() computes the light -- 'flat': one colour per face (lighting.py), 'smooth': at
        # the vertices, from the area-weighted normals of their faces, interpolated over the triangle (Gouraud shading).
        # 'smooth' takes vertex colours (render(vertices, faces, VertexColors(c)), vertex_colors.py) or UV images (UVImages,
        # uv_textures.py); texture cubes are lit per face only.  render_silhouettes and render_depth ignore the attribute.
        self.shading = 'flat'
        # not in the reference: a Lights (lights.py) -- the light as tensors, shared or one per image, possibly learnable,
        # with nine spherical-harmonics coefficients next to the lamp.  None: the host attributes `light_*` above, every path
        # exactly as without the attribute.  With a Lights render() ignores `light_*` and takes its light from light_colors
        # (see _render_lights); render_silhouettes and render_depth ignore the attribute.
        self.lights = None
        # not in the reference: the sigma of render_soft_silhouettes (soft_silhouette.py), in squared NDC units
        self.soft_sigma = 1e-4
        # not in the reference: render_soft's sharpness of the depth order and the background's place in it (soft_render.py)
        self.soft_gamma = 1e-4
        self.soft_eps = 1e-3

    def _project(self, vertices, faces):
        """camera + perspective + gather (renderer.py:40-51, :60-71, :92-103)."""
        if self.camera_mode == 'projection':
            check_projection(self)
            vertices = projection(vertices, self.K, self.R, self.t, self.dist_coeffs, self.orig_size)
            return vertices_to_faces(vertices, faces)
        if self.camera_mode == 'look_at':
            vertices = look_at(vertices, self.eye)
        elif self.camera_mode == 'look':
            vertices = look(vertices, self.eye, self.camera_direction)
        if self.perspective:
            vertices = perspective(vertices, angle=self.viewing_angle)
        return vertices_to_faces(vertices, faces)

    def _frontend_torch(self, vertices, faces, textures=None, light_colors=False):
        """Everything in front of the rasterizer, module by module as in the reference (renderer.py:37-51, :77-103).  With
        `light_colors` (not in the reference) the second result is lighting()'s colour of every face, [B,F,3]."""
        if self.fill_back:  # renderer.py:37-38, :77-79
            faces = torch.cat((faces, torch.flip(faces, dims=[2])), dim=1).detach()
            if textures is not None:
                textures = torch.cat((textures, textures.permute(0, 1, 4, 3, 2, 5)), dim=1)
        if light_colors:  # the light of a white texel
            textures = torch.ones(tuple(faces.shape[:2]) + (1, 1, 1, 3), dtype=torch.float32, device=vertices.device)
        if textures is not None:  # lighting in world space (renderer.py:82-90)
            faces_lighting = vertices_to_faces(vertices, faces)
            textures = lighting(
                faces_lighting,
                textures,
                self.light_intensity_ambient,
                self.light_intensity_directional,
                self.light_color_ambient,
                self.light_color_directional,
                self.light_direction)
        if light_colors:
            textures = textures.reshape(textures.shape[0], -1, 3)
        return self._project(vertices, faces), textures

    def _frontend(self, vertices, faces, textures=None, light_colors=False, fused=None):
        """-> (faces [B,F,3,3], what the rasterizer takes second: lit textures, with `light_colors` the per-face light colours
        [B,F,3] for its face_light, else None): the fused HIP front-end when the call fits it (`fused`: the caller's answer
        where it had to ask already), else torch.  Every render* comes through here, once, and only here are `last_frontend`
        and `frontend_calls` written."""
        if fused is None:
            fused = frontend.fusable(self, vertices, faces, textures) and (not light_colors or frontend.light_fusable(self))
        self.last_frontend = 'fused' if fused else 'torch'
        self.frontend_calls[self.last_frontend] += 1
        if not fused:
            return self._frontend_torch(vertices, faces, textures, light_colors)
        if light_colors:
            return frontend.project_and_light_colors(self, vertices, faces)
        return frontend.project_and_light(self, vertices, faces, textures)

    def render_silhouettes(self, vertices, faces):
        faces, _ = self._frontend(vertices, faces)
        # NB: near / far / rasterizer_eps are NOT forwarded here (renderer.py:52)
        return rasterize_silhouettes(faces, self.image_size, self.anti_aliasing, graph_replay=self.graph_replay)

    def render_depth(self, vertices, faces):
        faces, _ = self._frontend(vertices, faces)
        return rasterize_depth(faces, self.image_size, self.anti_aliasing, graph_replay=self.graph_replay)  # renderer.py:72 (Q2)

    def render_soft_silhouettes(self, vertices, faces, sigma=None):
        """Not in the reference: the soft silhouette [B,S,S] of soft_silhouette.py, whose exact gradient reaches a face from
        pixels it does not cover.  `sigma` (None: `soft_sigma`) sets the width of the transition.  The geometry is the
        front-end's, without the fill_back copies (a duplicated face would count twice; orientation plays no role); `near`
        and `far` select the faces; `anti_aliasing`, the lights and `shading` are ignored."""
        nf = faces.shape[1]
        faces, _ = self._frontend(vertices, faces)
        return soft_silhouettes(faces[:, :nf], self.image_size, self.soft_sigma if sigma is None else sigma, self.near, self.far)

    def _soft_face_colors(self, vertices, faces, colors):
        """render_soft's colour of every face before the light, [B|1,F,3]: a face-colour tensor as it is, the mean of a
        VertexColors' three vertex colours, the mean of a texture cube.  Plain torch, differentiable."""
        if isinstance(colors, VertexColors):
            B = vertices.shape[0]
            if colors.num_vertices != vertices.shape[1]:
                raise ValueError('VertexColors: %d colours for %d vertices' % (colors.num_vertices, vertices.shape[1]))
            if colors.color_batch not in (1, B):
                raise ValueError('VertexColors: batched colours must have the batch size of the vertices (%d), got %d'
                                 % (B, colors.color_batch))
            idx, vc = faces.long(), colors.colors
            if vc.dim() == 2:
                return (vc[idx] if idx.dim() == 3 else vc[idx][None]).mean(2)
            if idx.dim() == 2:
                idx = idx[None].expand(B, -1, -1)
            return vc[torch.arange(B, device=idx.device)[:, None, None], idx].mean(2)
        if torch.is_tensor(colors) and colors.is_floating_point():
            if colors.dim() == 6 and colors.shape[5] == 3:
                return colors.mean((2, 3, 4))
            if colors.dim() == 3 and colors.shape[2] == 3:
                return colors
            if colors.dim() == 2 and colors.shape[1] == 3:
                return colors[None]
        raise ValueError('render_soft: colors must be face colours [B|1,F,3] or [F,3], a VertexColors or texture cubes '
                         '[B|1,F,ts,ts,ts,3]')

    def _soft_corner_colors(self, vertices, faces, colors):
        """render_soft(per_pixel=True): -> (projected faces [B,F',3,3], lit corner colours [B|1,F',3,3]), F' the front-end's
        face count.  A VertexColors goes through render()'s own preparation (_render_vertex_colors, or _render_lights with
        `lights`); a tensor is multiplied by the light, per face ('flat') or per corner ('smooth')."""
        if self.shading not in ('flat', 'smooth'):
            raise ValueError("Renderer.shading must be 'flat' or 'smooth', got %r" % (self.shading,))
        if isinstance(colors, VertexColors):
            if self.lights is not None:
                projected, corner, _ = self._render_lights(vertices, faces, colors)
            else:
                projected, corner, _ = self._render_vertex_colors(vertices, faces, colors)
            return projected, corner.colors
        nf = faces.shape[1]
        if not (torch.is_tensor(colors) and colors.is_floating_point()):
            raise ValueError('render_soft: colors must be a float tensor or a VertexColors')
        if colors.dim() == 6:
            raise ValueError('render_soft: per_pixel=True takes a VertexColors, corner colours [B|1,F,3,3] / [F,3,3] or face '
                             'colours [B|1,F,3] / [F,3]; texture cubes are not sampled per pixel (wrap them in a '
                             'TextureCubes)')
        shape = tuple(colors.shape)
        if colors.dim() == 4 and shape[1:] == (nf, 3, 3):
            corner = colors
        elif colors.dim() == 3 and shape[1:] == (nf, 3):          # (with three faces [3,3,3] reads as face colours)
            corner = colors[:, :, None, :].expand(-1, -1, 3, -1)
        elif colors.dim() == 3 and shape == (nf, 3, 3):
            corner = colors[None]
        elif colors.dim() == 2 and shape == (nf, 3):
            corner = colors[None, :, None, :].expand(-1, -1, 3, -1)
        else:
            raise ValueError('render_soft: per_pixel=True takes a VertexColors, corner colours [B|1,F,3,3] / [F,3,3] or face '
                             'colours [B|1,F,3] / [F,3] (F = %d), got %s' % (nf, shape))
        smooth = self.shading == 'smooth'
        if self.lights is not None:
            light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=smooth)
            projected, _ = self._frontend(vertices, faces)
        elif smooth:
            fused = frontend.fusable(self, vertices, faces, None) and frontend.light_fusable(self)
            light = vertex_light(vertices, faces, self.light_intensity_ambient, self.light_intensity_directional,
                                 self.light_color_ambient, self.light_color_directional, self.light_direction,
                                 fill_back=self.fill_back, smooth=True, implementation=None if fused else 'torch')
            projected, _ = self._frontend(vertices, faces, fused=fused)
        else:
            projected, light = self._frontend(vertices, faces, light_colors=True)
        light = light[:, :nf]
        return projected[:, :nf], corner.to(light.dtype) * (light if smooth else light[:, :, None, :])

    def render_soft(self, vertices, faces, colors, sigma=None, gamma=None, per_pixel=False):
        """Not in the reference: the soft colour image rgba [B,4,S,S] of soft_render.py -- coverage as in
        render_soft_silhouettes, the faces' colours aggregated by a depth-weighted softmax -- whose exact gradient reaches
        hidden faces and every z.  `colors`: one colour per face, [B,F,3] / [1,F,3] / [F,3]; a VertexColors (a face takes the
        mean of its three vertex colours); or texture cubes [B|1,F,ts,ts,ts,3] (a face takes the mean of its cube).  The
        colour is multiplied by the per-face light of the face's front copy (the host attributes `light_*`, or `lights`).
        `sigma` (None: `soft_sigma`) sets the width of the coverage's transition, `gamma` (None: `soft_gamma`) the sharpness
        of the depth order; `soft_eps`, `background_color`, `near` and `far` come from the renderer.  The geometry is the
        front-end's, without the fill_back copies; `anti_aliasing` and `shading` are ignored.

        per_pixel=True: the colour varies inside a face -- three lit colours per face, one per corner, interpolated
        perspective-correctly at every pixel (soft_render with corner colours), and `shading` is honoured.  A VertexColors
        gives exactly the corner colours render() would rasterize (lit per face with 'flat', at the vertices with 'smooth';
        from `lights` when set).  A tensor [B,F,3,3] / [1,F,3,3] / [F,3,3] gives the corner colours themselves, a tensor of
        face colours [B,F,3] / [1,F,3] / [F,3] the face colour at all three corners; both are multiplied by the light, per
        face with 'flat', per corner with 'smooth'.  (With exactly three faces a [3,3,3] tensor reads as face colours.)
        A bare tensor of texture cubes raises ValueError: wrap it in a TextureCubes (below) to have it sampled per pixel.

        A UVImages (per_pixel=True only; without it ValueError): its images are sampled at every pixel (soft_render_uv), times
        the per-face light of the face's front copy -- `light_*`, or `lights` when set, as the flat path takes it.  Gradients
        reach the vertices, the images and the camera.  shading = 'smooth' raises ValueError: a light per corner is not done
        for UV images in the soft renderer.

        A TextureCubes (per_pixel=True only; without it ValueError): its cubes [B|1,F,ts,ts,ts,3] are sampled at every pixel
        with the rasterizer's trilinear lookup (soft_render_cubes, texture_eps = `rasterizer_eps`), times the per-face light
        of the face's front copy, as for a UVImages.  Gradients reach the vertices, the cubes and the camera.  shading =
        'smooth' raises ValueError."""
        if isinstance(colors, TextureCubes):
            if not per_pixel:
                raise ValueError('render_soft: a TextureCubes is sampled at every pixel: pass per_pixel=True (a bare tensor of '
                                 'cubes gives the mean of each cube)')
            if self.shading not in ('flat', 'smooth'):
                raise ValueError("Renderer.shading must be 'flat' or 'smooth', got %r" % (self.shading,))
            if self.shading == 'smooth':
                raise ValueError("render_soft: shading = 'smooth' with a TextureCubes: a light per corner is not done for "
                                 "texture cubes in the soft renderer (use 'flat')")
            nf = faces.shape[1]
            if self.lights is not None:
                light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=False)
                projected, _ = self._frontend(vertices, faces)
            else:
                projected, light = self._frontend(vertices, faces, light_colors=True)
            return soft_render_cubes(projected[:, :nf], colors.textures, light[:, :nf], self.image_size,
                                     self.soft_sigma if sigma is None else sigma, self.soft_gamma if gamma is None else gamma,
                                     self.near, self.far, self.soft_eps, self.background_color, self.rasterizer_eps)
        if isinstance(colors, UVImages):
            if not per_pixel:
                raise ValueError('render_soft: a UVImages is sampled at every pixel: pass per_pixel=True')
            if self.shading not in ('flat', 'smooth'):
                raise ValueError("Renderer.shading must be 'flat' or 'smooth', got %r" % (self.shading,))
            if self.shading == 'smooth':
                raise ValueError("render_soft: shading = 'smooth' with a UVImages: a light per corner is not done for UV "
                                 "images in the soft renderer (use 'flat')")
            nf = faces.shape[1]
            if self.lights is not None:
                light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=False)
                projected, _ = self._frontend(vertices, faces)
            else:
                projected, light = self._frontend(vertices, faces, light_colors=True)
            return soft_render_uv(projected[:, :nf], colors, light[:, :nf], self.image_size,
                                  self.soft_sigma if sigma is None else sigma, self.soft_gamma if gamma is None else gamma,
                                  self.near, self.far, self.soft_eps, self.background_color)
        if per_pixel:
            nf = faces.shape[1]
            projected, corner = self._soft_corner_colors(vertices, faces, colors)
            return soft_render(projected[:, :nf], corner[:, :nf], self.image_size,
                               self.soft_sigma if sigma is None else sigma, self.soft_gamma if gamma is None else gamma,
                               self.near, self.far, self.soft_eps, self.background_color)
        nf = faces.shape[1]
        color = self._soft_face_colors(vertices, faces, colors)
        if self.lights is not None:
            light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=False)
            projected, _ = self._frontend(vertices, faces)
        else:
            projected, light = self._frontend(vertices, faces, light_colors=True)
        return soft_render(projected[:, :nf], color.to(light.dtype) * light[:, :nf], self.image_size,
                           self.soft_sigma if sigma is None else sigma, self.soft_gamma if gamma is None else gamma,
                           self.near, self.far, self.soft_eps, self.background_color)

    def _use_face_light(self, vertices, faces, textures):
        if self.face_light is False or not (torch.is_tensor(textures) and textures.dim() == 6):
            return False
        ts = textures.shape[2]
        if self.face_light is None and ts < 3:
            return False
        # (the package attribute `rasterize` is the function; the module of that name holds the switch)
        replay = self.graph_replay if self.graph_replay is not None else sys.modules[rasterize.__module__].GRAPH_REPLAY
        return not replay and frontend.fusable(self, vertices, faces, textures)

    def _render_shared(self, vertices, faces, textures):
        """render() with ONE set of cubes [1,Nf,ts,ts,ts,3] for a batch of B > 1 views (not in the reference).  Lit textures
        would be one copy per view again, so the light goes to the rasterizer as one colour per face (face_light is implied,
        whatever `face_light` and the texture size say), the cubes as they are: from the fused front-end when it takes the
        call, else from lighting() on a ones texture behind the module-by-module front-end.  The cubes' gradient comes back
        summed over the views.  Runs eagerly: graph_replay does not apply."""
        faces, light = self._frontend(vertices, faces, light_colors=True)
        return faces, textures, dict(faces_z_ref=self.faces_z_ref, face_light=light)

    def _render_uv(self, vertices, faces, uv):
        """render() with a UVImages: the images sampled at every covered pixel (not in the reference).  Per-face light colours
        always (face_light is implied): from the fused front-end when it takes the call, else from lighting() on a ones
        texture behind the module-by-module front-end.  Runs eagerly: graph_replay does not apply."""
        if self.shading == 'smooth':
            return self._render_uv_smooth(vertices, faces, uv)
        faces, light = self._frontend(vertices, faces, light_colors=True)
        return faces, uv, dict(face_light=light)

    def _render_uv_smooth(self, vertices, faces, uv):
        """render() with a UVImages and shading = 'smooth' (not in the reference): vertex_light computes the light at the
        vertices in world space (area-weighted normals, a colour per face corner), the front-end projects the geometry, and
        the rasterizer multiplies its image sample by the light interpolated at the pixel.  HIP or torch by the rule of
        _render_vertex_colors; runs eagerly, and a capture needs one eager step first (the vertex adjacency table)."""
        if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3):
            raise ValueError('vertices must be a tensor [batch size, num of vertices, 3]')
        fused = frontend.fusable(self, vertices, faces, None) and frontend.light_fusable(self)
        light = vertex_light(vertices, faces, self.light_intensity_ambient, self.light_intensity_directional,
                             self.light_color_ambient, self.light_color_directional, self.light_direction,
                             fill_back=self.fill_back, smooth=True, implementation=None if fused else 'torch')
        faces, _ = self._frontend(vertices, faces, fused=fused)
        return faces, uv, dict(face_light=light)

    def _render_vertex_colors(self, vertices, faces, vc):
        """render() with a VertexColors (not in the reference): vertex_shade lights the colours per corner, in world space,
        the front-end projects the geometry, and the rasterizer interpolates the corner colours at every covered pixel.
        Both pieces take their HIP kernels when the call fits them (`last_frontend` names the geometry's).  Runs eagerly:
        graph_replay does not apply (a whole step can be captured with neural_renderer_amd.graph.capture once one eager
        step has built the vertex adjacency table)."""
        if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3):
            raise ValueError('vertices must be a tensor [batch size, num of vertices, 3]')
        if vc.num_vertices != vertices.shape[1]:
            raise ValueError('VertexColors: %d colours for %d vertices' % (vc.num_vertices, vertices.shape[1]))
        if vc.color_batch not in (1, vertices.shape[0]):
            raise ValueError('VertexColors: batched colours must have the batch size of the vertices (%d), got %d'
                             % (vertices.shape[0], vc.color_batch))
        if vc.device != vertices.device:
            raise ValueError('VertexColors: colours on %s, vertices on %s' % (vc.device, vertices.device))
        fused = frontend.fusable(self, vertices, faces, None) and frontend.light_fusable(self)
        corner = vertex_shade(vertices, faces, vc.colors, self.light_intensity_ambient, self.light_intensity_directional,
                              self.light_color_ambient, self.light_color_directional, self.light_direction,
                              fill_back=self.fill_back, smooth=self.shading == 'smooth',
                              implementation=None if fused else 'torch')
        faces, _ = self._frontend(vertices, faces, fused=fused)
        return faces, corner, {}

    def _render_lights(self, vertices, faces, textures):
        """render() with `lights` set (not in the reference): light_colors computes the light in world space -- HIP kernels
        on CUDA float32 tensors --, the front-end projects the geometry alone, and the light reaches the rasterizer as its
        `face_light`: one colour per face for texture cubes (per image, or one set shared by the batch; `face_light` and the
        texture size are not asked) and for UVImages with flat shading, one per corner for UVImages with smooth shading.
        VertexColors: the corner colours are `colors[faces]`, flipped for the reversed copies, times the light -- one gather
        and one multiply in torch --, rasterized as CornerColors.  Runs eagerly: graph_replay does not apply."""
        if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3):
            raise ValueError('vertices must be a tensor [batch size, num of vertices, 3]')
        smooth = self.shading == 'smooth'
        if isinstance(textures, VertexColors):
            B = vertices.shape[0]
            if textures.num_vertices != vertices.shape[1]:
                raise ValueError('VertexColors: %d colours for %d vertices' % (textures.num_vertices, vertices.shape[1]))
            if textures.color_batch not in (1, B):
                raise ValueError('VertexColors: batched colours must have the batch size of the vertices (%d), got %d'
                                 % (B, textures.color_batch))
            if textures.device != vertices.device:
                raise ValueError('VertexColors: colours on %s, vertices on %s' % (textures.device, vertices.device))
            light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=smooth)
            idx, colors = faces.long(), textures.colors
            if idx.dim() == 2:
                idx = idx[None].expand(B, -1, -1)
            corner = colors[idx] if colors.dim() == 2 else colors[torch.arange(B, device=idx.device)[:, None, None], idx]
            if self.fill_back:
                corner = torch.cat((corner, torch.flip(corner, dims=[2])), dim=1)
            corner = corner * (light if smooth else light[:, :, None, :])
            projected, _ = self._frontend(vertices, faces)
            return projected, CornerColors(corner), {}
        if isinstance(textures, UVImages):
            light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=smooth)
            projected, _ = self._frontend(vertices, faces)
            return projected, textures, dict(face_light=light)
        if smooth:
            raise ValueError("Renderer.shading = 'smooth' takes UVImages or VertexColors: texture cubes are lit per face "
                             "('flat') only")
        light = light_colors(vertices, faces, self.lights, fill_back=self.fill_back, smooth=False)
        projected, _ = self._frontend(vertices, faces)
        return projected, textures, dict(faces_z_ref=self.faces_z_ref, face_light=light)

    def _shade(self, vertices, faces, textures):
        """The one dispatch of render() and render_rgbad(): everything in front of the rasterizer for the shading source
        `textures` -> (projected faces [B,F,3,3], what the rasterizer takes second, its keyword arguments)."""
        if self.shading not in ('flat', 'smooth'):
            raise ValueError("Renderer.shading must be 'flat' or 'smooth', got %r" % (self.shading,))
        if self.lights is not None:
            return self._render_lights(vertices, faces, textures)
        if isinstance(textures, VertexColors):
            return self._render_vertex_colors(vertices, faces, textures)
        if isinstance(textures, UVImages):
            return self._render_uv(vertices, faces, textures)
        if self.shading == 'smooth':
            raise ValueError("Renderer.shading = 'smooth' takes UVImages or VertexColors: texture cubes are lit per face "
                             "('flat') only")
        if (torch.is_tensor(textures) and textures.dim() == 6 and textures.shape[0] == 1 and torch.is_tensor(vertices)
                and vertices.dim() == 3 and vertices.shape[0] > 1):
            return self._render_shared(vertices, faces, textures)
        if self._use_face_light(vertices, faces, textures):
            faces, light = self._frontend(vertices, faces, light_colors=True, fused=True)
            return faces, textures, dict(faces_z_ref=self.faces_z_ref, face_light=light)
        faces, textures = self._frontend(vertices, faces, textures)
        return faces, textures, dict(faces_z_ref=self.faces_z_ref, graph_replay=self.graph_replay)

    def render(self, vertices, faces, textures):
        """`textures`: cubes [B,Nf,ts,ts,ts,3] as in the reference -- or [1,Nf,ts,ts,ts,3] beside B > 1 views (not in the
        reference): one set shared by the batch, see _render_shared --, or (not in the reference) a UVImages whose images are
        sampled at every covered pixel (uv_textures.py), or a VertexColors (vertex_colors.py), lit as `shading` says."""
        faces, textures, kw = self._shade(vertices, faces, textures)
        return rasterize(faces, textures, self.image_size, self.anti_aliasing, self.near, self.far, self.rasterizer_eps,
                         self.background_color, **kw)

    def render_rgbad(self, vertices, faces, textures, return_rgb=True, return_alpha=True, return_depth=True):
        """Not in the reference: render()'s image together with the silhouette and the depth image from ONE rasterization --
        the dict of rasterize_rgbad, 'rgb' [B,3,is,is], 'alpha' and 'depth' [B,is,is], None for an output that is not asked
        for (its work is skipped).  `textures` is anything render() takes, through render()'s own dispatch (`lights`,
        VertexColors, UVImages flat and smooth, shared cubes, `face_light`, the lit-texture path with `graph_replay`), and
        'rgb' is render()'s image bit for bit.  Without return_rgb only the geometry goes through the front-end, as in
        render_silhouettes, and `textures` is not looked at.

        Alpha and depth here are rasterized with the renderer's `near`, `far` and `rasterizer_eps`, which render_silhouettes
        and render_depth do not forward (quirk Q2 of the reference: they run with the rasterizer's defaults).  Under the
        default near / far the forward images are the same, bit for bit; the BACKWARD differs: the silhouette gradient here
        is taken with eps = rasterizer_eps (1e-3, as render's), render_silhouettes' with 1e-4."""
        if return_rgb:
            faces, textures, kw = self._shade(vertices, faces, textures)
        else:
            if self.shading not in ('flat', 'smooth'):
                raise ValueError("Renderer.shading must be 'flat' or 'smooth', got %r" % (self.shading,))
            faces, _ = self._frontend(vertices, faces)
            textures, kw = None, dict(graph_replay=self.graph_replay)
        return rasterize_rgbad(faces, textures, self.image_size, self.anti_aliasing, self.near, self.far, self.rasterizer_eps,
                               self.background_color, return_rgb, return_alpha, return_depth, **kw)

    def render_normals(self, vertices, faces, space='world', normalize=False, return_dict=False):
        """Not in the reference: a normal map [B,3,is,is] -- the channels are the x, y, z of the surface normal at the pixel,
        signed (lighting()'s sign: a light along `d` lights the faces with n . d > 0), 0 on the background whatever
        `background_color` says.  corner_normals (normals.py) gives every face corner
        its normal in world space -- the face's with shading = 'flat', the area-weighted vertex normal with 'smooth', the
        negated normals on the reversed copies of `fill_back` --, the front-end projects the geometry, once, and the
        rasterizer interpolates the nine numbers of a face perspective-correctly, as it does corner colours, with the
        renderer's image_size, anti_aliasing, near, far and rasterizer_eps.  Interpolated normals are shorter than 1 between
        the vertices of a smooth mesh and fade to 0 across an anti-aliased silhouette; normalize = True divides every pixel
        by |n| + 1e-5 afterwards.

        space = 'world': the axes of `vertices`.  space = 'camera': the normals are rotated by the camera's rotation
        (normals.camera_rotation) before they are rasterized: the axes of look_at / look -- x right, y up, z away from the
        camera --, in 'projection' mode those of `R` (OpenCV: y down).  It is the rotation alone, not the perspective map.
        The gradient reaches the vertices, through the normals and through the geometry, and with 'camera' a learnable `eye`
        or `R`.

        return_dict = True: the dict {'normals', 'alpha', 'depth'} from the one rasterization ('alpha' and 'depth' as
        render_rgbad's).  `lights` and the light_* attributes are ignored: no light enters a normal map.  Runs eagerly:
        graph_replay does not apply (a whole step can be captured once one eager step has built the vertex adjacency
        table)."""
        if self.shading not in ('flat', 'smooth'):
            raise ValueError("Renderer.shading must be 'flat' or 'smooth', got %r" % (self.shading,))
        if space not in ('world', 'camera'):
            raise ValueError("render_normals: space must be 'world' or 'camera', got %r" % (space,))
        if not (torch.is_tensor(vertices) and vertices.dim() == 3 and vertices.shape[2] == 3):
            raise ValueError('vertices must be a tensor [batch size, num of vertices, 3]')
        corner = corner_normals(vertices, faces, smooth=self.shading == 'smooth', fill_back=self.fill_back).colors
        if space == 'camera':
            B, F = corner.shape[:2]
            r = camera_rotation(self, B, vertices)
            corner = torch.matmul(corner.reshape(B, 3 * F, 3), r.transpose(1, 2)).reshape(B, F, 3, 3)
        faces, _ = self._frontend(vertices, faces)
        out = rasterize_rgbad(faces, CornerColors(corner), self.image_size, self.anti_aliasing, self.near, self.far,
                              self.rasterizer_eps, [0, 0, 0], True, bool(return_dict), bool(return_dict))
        normals = out['rgb']
        if normalize:
            normals = normals / (torch.sqrt((normals * normals).sum(1, keepdim=True)) + 1e-5)
        if return_dict:
            return {'normals': normals, 'alpha': out['alpha'], 'depth': out['depth']}
        return normals
