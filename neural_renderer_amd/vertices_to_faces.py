"""Vertex gather: [bs, nv, 3] x [bs, nf, 3] -> [bs, nf, 3, 3] -- reference vertices_to_faces.py:4-21.

On the GPU both directions are HIP kernels of libnr_hip.so (`nr_vertices_to_faces`, `nr_vertices_to_faces_backward`):
the backward -- the face->vertex gradient scatter, Chainer's get_item backward in the reference -- uses hardware float
atomics instead of torch's sort-based `index_put_(accumulate=True)`, which alone cost more than the whole rasterizer
(scripts/glue_profile.py).  CPU tensors (host-side glue, tests) take the plain torch path."""
import torch

from . import _lib, _util


@_util.once_differentiable
class _VerticesToFaces(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, faces):
        v = _lib.dense(vertices.detach())
        f = _lib.dense(faces.detach().to(torch.int32))
        B, Nv = v.shape[:2]
        Nf = f.shape[1]
        out = torch.empty((B, Nf, 3, 3), dtype=torch.float32, device=v.device)
        _lib.launch('nr_vertices_to_faces', v.device, v.data_ptr(), f.data_ptr(), out.data_ptr(), B, Nv, Nf, 1)
        ctx.save_for_backward(f)
        ctx.dims = (B, Nv, Nf)
        return out

    @staticmethod
    def backward(ctx, grad_faces):
        f, = ctx.saved_tensors
        B, Nv, Nf = ctx.dims
        g = _lib.dense(grad_faces)
        grad_vertices = torch.empty((B, Nv, 3), dtype=torch.float32, device=g.device)
        _lib.launch('nr_vertices_to_faces_backward', g.device, g.data_ptr(), f.data_ptr(), grad_vertices.data_ptr(), B, Nv, Nf,
                    1)
        return grad_vertices, None


def vertices_to_faces(vertices, faces):
    """
    :param vertices: [batch size, number of vertices, 3]
    :param faces: [batch size, number of faces, 3)
    :return: [batch size, number of faces, 3, 3]
    """
    assert vertices.dim() == 3
    assert faces.dim() == 3
    assert vertices.shape[0] == faces.shape[0]
    assert vertices.shape[2] == 3
    assert faces.shape[2] == 3

    if vertices.is_cuda and vertices.dtype == torch.float32:
        _util.check_face_indices(faces, vertices.shape[1], vertices.device)  # IndexError / ValueError, cached per tensor
        return _VerticesToFaces.apply(vertices, faces)
    bs, nv = vertices.shape[:2]
    faces = faces.long() + (torch.arange(bs, device=vertices.device, dtype=torch.long) * nv)[:, None, None]
    vertices = vertices.reshape((bs * nv, 3))
    return vertices[faces]
