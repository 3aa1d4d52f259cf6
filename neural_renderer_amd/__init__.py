"""neural_renderer_amd -- MI355X-native differentiable mesh rasterizer behind the API of hiroharu-kato/neural_renderer.

The public names are the reference's (neural_renderer/__init__.py:1-16); `import neural_renderer` is an alias package."""
# the operator and its wrappers (HIP kernels behind include/nr_hip.h)
from .rasterize import (Rasterize, rasterize, rasterize_depth, rasterize_rgbad, rasterize_silhouettes,
                        use_unsafe_rasterizer, use_graph_replay, clear_workspace_cache)
from .renderer import Renderer
# geometry / lighting glue in front of the rasterizer
from .cross import cross
from .get_points_from_angles import get_points_from_angles
from .lighting import lighting
from .look import look
from .look_at import look_at
from .perspective import perspective
from .projection import projection
from .vertices_to_faces import vertices_to_faces
# meshes, files, optimiser
from .load_obj import load_obj
from .mesh import Mesh
from .optimizers import Adam
from .save_obj import save_obj
# not in the reference: learnable UV texture images (the load_obj bake as a differentiable step, or sampled per pixel)
from .uv_textures import UVImages, UVLayout, UVTextures, bake_uv_textures
# not in the reference: per-vertex colours and smooth (vertex-normal) shading, interpolated per pixel
from .vertex_colors import CornerColors, VertexColors, vertex_light, vertex_shade
# not in the reference: the Laplacian and flatness losses of a mesh fit (shape priors), HIP in both directions
from .mesh_losses import flatness_loss, laplacian_loss
# ... and the edge-length and the cotangent Laplacian loss, with the edges of a topology and their lengths
from .mesh_losses import cotangent_laplacian_loss, edge_length_loss, edge_lengths, mesh_edges
# not in the reference: the light as tensors -- per image, learnable, with spherical-harmonics coefficients -- HIP in both directions
from .lights import Lights, light_colors
# not in the reference: the objective of a fit on images -- silhouette IoU and masked squared error, optionally on an image
# pyramid -- HIP in both directions
from .image_losses import silhouette_iou_loss, squared_error_loss, ssim_loss, ssim_index
# not in the reference: mesh subdivision -- Loop and midpoint refinement of per-vertex data as a differentiable step, a sphere
# template -- HIP in both directions
from .subdivision import Subdivision, icosphere, subdivide, subdivision
# not in the reference: point-cloud terms of a 3-D fit -- surface sampling, nearest neighbours and the chamfer distance -- HIP in
# both directions
from .point_losses import SurfaceSamples, chamfer_distance, nearest_points, sample_surface, sample_surface_points
# not in the reference: point-to-mesh distance -- for every point the nearest triangle, for every triangle the nearest point,
# with exact gradients to points and vertices -- HIP in both directions
from .point_mesh import closest_cloud_points, closest_surface_points, point_mesh_distance
# not in the reference: generalized winding numbers -- inside / outside, voxel grids and the sign of the distance, with exact
# gradients to points and vertices -- HIP in both directions
from .winding import mesh_occupancy, signed_distance, voxel_centers, voxel_iou, voxelize, winding_number
# not in the reference: ray casting -- the first hit of every ray on a mesh with a differentiable distance, occlusion, vertex
# visibility and the rays of a renderer's camera -- the search in HIP
from .ray_mesh import camera_rays, ray_mesh_intersect, ray_mesh_occluded, vertex_visibility
# not in the reference: isosurface extraction -- marching tetrahedra from a grid of values to a mesh, the way back from
# `voxelize` and `signed_distance`, with vertices differentiable in the values -- the extraction in HIP
from .isosurface import IsoSurface, extract_isosurface, marching_tetrahedra
# not in the reference: vertex, face and corner normals -- HIP in both directions -- for Renderer.render_normals, and the
# rotation of a renderer's camera
from .normals import camera_rotation, corner_normals, face_normals, vertex_normals
# not in the reference: soft silhouettes -- distance-based coverage with its exact gradient, HIP in both directions -- for
# Renderer.render_soft_silhouettes
from .soft_silhouette import soft_silhouettes, soft_silhouettes_torch
# not in the reference: soft colour rendering -- the soft coverage aggregated by a depth-weighted softmax, with its exact
# gradient to x, y, z and the face colours, HIP in both directions -- for Renderer.render_soft
from .soft_render import (TextureCubes, soft_render, soft_render_cubes, soft_render_cubes_torch, soft_render_torch, soft_render_uv,
                          soft_render_uv_torch)
# not in the reference: multi-GPU helpers and the captured-graph helper for fixed-shape loops
from . import distributed, graph

# NR_BACKWARD_ON_CALLER_THREAD=1 (opt-in, read once here): graph.backward_on_caller_thread() for the importing thread -- torch's
# autograd then runs CUDA nodes on the thread that calls backward() instead of handing them to its device thread, which costs a
# host-bound loop ~80 us per step (bench.py shard_rows).  One process per GPU gains nothing from the device thread.
import os as _os
if _os.environ.get('NR_BACKWARD_ON_CALLER_THREAD', '0') not in ('', '0'):
    graph.backward_on_caller_thread()

# the C ABI's version (include/nr_hip.h NR_VERSION = major * 100 + minor), checked against the loaded library by _lib.load()
__version__ = '0.6.0'
__all__ = ['Rasterize', 'rasterize', 'rasterize_depth', 'rasterize_rgbad', 'rasterize_silhouettes', 'use_unsafe_rasterizer', 'use_graph_replay',
           'clear_workspace_cache',
           'Renderer', 'cross', 'get_points_from_angles', 'lighting', 'look', 'look_at', 'perspective', 'projection',
           'vertices_to_faces',
           'load_obj', 'Mesh', 'Adam', 'save_obj', 'UVImages', 'TextureCubes', 'UVLayout', 'UVTextures', 'bake_uv_textures',
           'CornerColors', 'VertexColors', 'vertex_shade', 'vertex_light',
           'laplacian_loss', 'flatness_loss', 'edge_length_loss', 'cotangent_laplacian_loss', 'mesh_edges', 'edge_lengths', 'Lights', 'light_colors', 'silhouette_iou_loss', 'squared_error_loss', 'ssim_loss', 'ssim_index',
           'Subdivision', 'subdivision', 'subdivide', 'icosphere',
           'SurfaceSamples', 'chamfer_distance', 'nearest_points', 'sample_surface', 'sample_surface_points',
           'closest_surface_points', 'closest_cloud_points', 'point_mesh_distance',
           'winding_number', 'mesh_occupancy', 'voxel_centers', 'voxelize', 'voxel_iou', 'signed_distance',
           'ray_mesh_intersect', 'ray_mesh_occluded', 'vertex_visibility', 'camera_rays',
           'IsoSurface', 'extract_isosurface', 'marching_tetrahedra',
           'vertex_normals', 'face_normals', 'corner_normals', 'camera_rotation',
           'soft_silhouettes', 'soft_silhouettes_torch', 'soft_render', 'soft_render_torch', 'soft_render_uv',
           'soft_render_uv_torch', 'soft_render_cubes', 'soft_render_cubes_torch']
