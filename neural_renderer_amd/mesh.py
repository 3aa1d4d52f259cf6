"""Mesh holder with learnable vertices / textures -- reference neural_renderer/mesh.py:7-38 as an nn.Module."""
import torch
import torch.nn as nn

from .load_obj import load_obj


class Mesh(nn.Module):
    def __init__(self, filename_obj, texture_size=4, normalization=True):
        super(Mesh, self).__init__()
        vertices, faces = load_obj(filename_obj, normalization)
        self.vertices = nn.Parameter(torch.from_numpy(vertices))
        self.register_buffer('faces', torch.from_numpy(faces))
        self.num_vertices = self.vertices.shape[0]
        self.num_faces = self.faces.shape[0]
        shape = (self.num_faces, texture_size, texture_size, texture_size, 3)
        # mesh.py:22-24: chainer.initializers.Normal() = N(0, 0.05^2)
        self.textures = nn.Parameter(torch.randn(shape, dtype=torch.float32) * 0.05)
        self.texture_size = texture_size

    def get_batch(self, batch_size, shared_textures=False):
        """broadcast for minibatch (mesh.py:29-34).  `shared_textures` (not in the reference): the textures come back with a
        batch of 1, sigmoid(self.textures)[None] -- one set of cubes that Renderer.render and the rasterizer share among the
        batch_size views, the sigmoid run once -- instead of batch_size expanded copies."""
        vertices = self.vertices[None].expand(batch_size, *self.vertices.shape)
        faces = self.faces[None].expand(batch_size, *self.faces.shape)
        if shared_textures:
            return vertices, faces, torch.sigmoid(self.textures)[None]
        textures = torch.sigmoid(self.textures[None].expand(batch_size, *self.textures.shape))
        return vertices, faces, textures

    def forward(self, batch_size, shared_textures=False):
        """The module's call: get_batch."""
        return self.get_batch(batch_size, shared_textures)

    def laplacian_loss(self, implementation=None):
        """mesh_losses.laplacian_loss of the module's own vertices and faces (not in the reference): a 0-dim tensor."""
        from .mesh_losses import laplacian_loss
        return laplacian_loss(self.vertices, self.faces, implementation)

    def flatness_loss(self, eps=1e-6, implementation=None):
        """mesh_losses.flatness_loss of the module's own vertices and faces (not in the reference): a 0-dim tensor."""
        from .mesh_losses import flatness_loss
        return flatness_loss(self.vertices, self.faces, eps, implementation)

    def edge_length_loss(self, target=0.0, implementation=None):
        """mesh_losses.edge_length_loss of the module's own vertices and faces (not in the reference): a 0-dim tensor."""
        from .mesh_losses import edge_length_loss
        return edge_length_loss(self.vertices, self.faces, target, implementation)

    def cotangent_laplacian_loss(self, eps=1e-12, implementation=None):
        """mesh_losses.cotangent_laplacian_loss of the module's own vertices and faces (not in the reference): a 0-dim tensor."""
        from .mesh_losses import cotangent_laplacian_loss
        return cotangent_laplacian_loss(self.vertices, self.faces, eps, implementation)

    def sample_points(self, num_samples, generator=None):
        """point_losses.sample_surface_points of the module's own vertices and faces (not in the reference): (points
        [num_samples, 3], differentiable in self.vertices, and their SurfaceSamples)."""
        from .point_losses import sample_surface_points
        return sample_surface_points(self.vertices, self.faces, num_samples, generator)

    def point_mesh_distance(self, points, **kw):
        """point_mesh.point_mesh_distance of `points` and the module's own vertices and faces (not in the reference);
        direction, reduction and implementation as keywords."""
        from .point_mesh import point_mesh_distance
        return point_mesh_distance(points, self.vertices, self.faces, **kw)

    def winding_number(self, points, implementation=None):
        """winding.winding_number of `points` and the module's own vertices and faces (not in the reference)."""
        from .winding import winding_number
        return winding_number(points, self.vertices, self.faces, implementation)

    def voxelize(self, grid_size, **kw):
        """winding.voxelize of the module's own vertices and faces (not in the reference): [G,G,G]; bounds, hard and
        implementation as keywords."""
        from .winding import voxelize
        return voxelize(self.vertices, self.faces, grid_size, **kw)

    def signed_distance(self, points, implementation=None):
        """winding.signed_distance of `points` and the module's own vertices and faces (not in the reference)."""
        from .winding import signed_distance
        return signed_distance(points, self.vertices, self.faces, implementation)

    def cast_rays(self, origins, directions, **kw):
        """ray_mesh.ray_mesh_intersect of the rays and the module's own vertices and faces (not in the reference): (t,
        face_ids, barycentric); near, far, cull_backfaces and implementation as keywords."""
        from .ray_mesh import ray_mesh_intersect
        return ray_mesh_intersect(origins, directions, self.vertices, self.faces, **kw)

    def visible_vertices(self, eye, **kw):
        """ray_mesh.vertex_visibility of the module's own vertices and faces from `eye` (not in the reference): bool
        [num_vertices]; eps and implementation as keywords."""
        from .ray_mesh import vertex_visibility
        return vertex_visibility(self.vertices, self.faces, eye, **kw)

    def vertex_normals(self, implementation=None):
        """normals.vertex_normals of the module's own vertices and faces (not in the reference): [num_vertices, 3]."""
        from .normals import vertex_normals
        return vertex_normals(self.vertices, self.faces, implementation)

    def subdivide(self, levels=1, scheme='loop'):
        """Refine the mesh in place by `levels` levels of subdivision.subdivision (not in the reference; 'loop' or 'midpoint'):
        `vertices` becomes a NEW nn.Parameter holding the refined positions, the `faces` buffer is replaced, `num_vertices`
        and `num_faces` are updated, and every child face gets a copy of its parent's texture cube, textures[face_parent],
        as a new nn.Parameter.  Optimiser state for the old parameters is void: build a new optimiser afterwards (the
        multipliers of set_lr are carried over).  Each child repeats its parent's WHOLE cube, so the picture on the surface
        is not resampled: it appears four times per parent, smaller.  Returns the plan (its face_parent maps the new faces
        to the old)."""
        from .subdivision import subdivision
        plan = subdivision(self.faces, self.num_vertices, levels, scheme)
        if plan.levels == 0:
            return plan
        with torch.no_grad():
            vertices = nn.Parameter(plan(self.vertices.detach()).contiguous())
            textures = nn.Parameter(self.textures.detach()[plan.face_parent].contiguous())
        for new, old in ((vertices, self.vertices), (textures, self.textures)):
            if hasattr(old, 'lr'):
                new.lr = old.lr
        self.vertices, self.textures = vertices, textures
        self.faces = plan.faces.clone()
        self.num_vertices, self.num_faces = int(vertices.shape[0]), int(self.faces.shape[0])
        return plan

    def set_lr(self, lr_vertices, lr_textures):
        """Per-parameter learning-rate multipliers read by neural_renderer_amd.Adam (mesh.py:36-38)."""
        self.vertices.lr = lr_vertices
        self.textures.lr = lr_textures
