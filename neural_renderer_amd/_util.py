import functools
import math

import numpy as np
import torch

SOFT_MAX_FACES = 2 ** 24    # the soft operators' limits (include/nr_hip.h)
SOFT_MAX_SIZE = 16384


class _SecondDerivative(torch.autograd.Function):
    """forward(ctx, n, *tensors) -> the first n tensors, the gradients a backward returned; the others are the inputs of that
    backward's forward and the upstream gradients that require a gradient.  Their edges put this node on every path from the
    returned gradients to whatever a second derivative can be asked for, and its backward raises."""

    @staticmethod
    def forward(ctx, n, *tensors):
        return tuple(t.view_as(t) for t in tensors[:n])

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError('trying to differentiate twice a function that was marked with @once_differentiable: the '
                           'operators of neural_renderer_amd are differentiable once, a second derivative is not implemented')


def once_differentiable(cls):
    """Class decorator of every torch.autograd.Function in this package: a second derivative raises.  The backwards fill
    fresh buffers through the C ABI (or, in the plain-torch winding path, are written for one derivative), so under
    create_graph=True their results would pass for constants, and a gradient penalty or a Hessian-vector product would lose
    that term without a word.  torch.autograd.function.once_differentiable is not enough for that: it puts its error node
    behind the result only when an upstream gradient requires a gradient -- the plain (out * w).sum() does not -- and with
    edges to fresh leaves only, so torch.autograd.grad(f(g), x) finds no path from it to x and never runs it.  Here the
    forward notes its inputs that require a gradient on ctx, the backward runs under no_grad, and while a graph is being
    recorded its results go through _SecondDerivative with those inputs.  `backward.__wrapped__` is the undecorated one."""
    forward, backward = cls.forward, cls.backward

    @functools.wraps(forward)
    def once_forward(ctx, *args):
        ctx._nr_inputs = tuple(a for a in args if torch.is_tensor(a) and a.requires_grad)
        return forward(ctx, *args)

    @functools.wraps(backward)
    def once_backward(ctx, *grads):
        with torch.no_grad():
            outs = backward(ctx, *grads)
        if not torch.is_grad_enabled():
            return outs
        anchors = ctx._nr_inputs + tuple(g for g in grads if torch.is_tensor(g) and g.requires_grad)
        seq = outs if isinstance(outs, tuple) else (outs,)
        live = [i for i, o in enumerate(seq) if torch.is_tensor(o)]
        if not anchors or not live:
            return outs
        seq = list(seq)
        for i, o in zip(live, _SecondDerivative.apply(len(live), *([seq[i] for i in live] + list(anchors)))):
            seq[i] = o
        return tuple(seq) if isinstance(outs, tuple) else seq[0]

    cls.forward, cls.backward = staticmethod(once_forward), staticmethod(once_backward)
    return cls


def normalize(x, eps=1e-5):
    """chainer.functions.normalize: x / (||x||_2 + eps) along axis 1 (NOT torch.nn.functional.normalize,
    which divides by max(norm, eps)) -- used by reference look_at.py:30-32, look.py:29-31, lighting.py:40."""
    return x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + eps)


def as_tensor_like(value, ref, dtype=torch.float32):
    """list / tuple / ndarray / tensor -> tensor on ref's device (differentiable if it already is a tensor)."""
    if torch.is_tensor(value):
        return value.to(device=ref.device, dtype=dtype)
    return torch.as_tensor(np.asarray(value, dtype=np.float32), device=ref.device).to(dtype)


def number(name, what, v):
    """float(v) of a host number for the operator `name`'s argument `what`; a bool, a NaN or anything else raises."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
        raise ValueError('%s: %s must be a number, got %r' % (name, what, v))
    return float(v)


def check_implementation(name, implementation):
    """The first half of takes_hip, for an operator that raises other argument errors before it knows whether the call fits."""
    if implementation not in (None, 'torch', 'hip'):
        raise ValueError("%s: implementation must be None, 'torch' or 'hip'" % name)


def takes_hip(name, implementation, fits, needs):
    """True when the call takes the HIP kernels: `fits` them and is not sent to 'torch'.  Raises ValueError for an unknown
    `implementation`, and for 'hip' when `fits` is false with `needs`, the operator's own sentence."""
    check_implementation(name, implementation)
    if implementation == 'hip' and not fits:
        raise ValueError('%s: %s' % (name, needs))
    return fits and implementation != 'torch'


# what soft_silhouette.py and soft_render.py share

def soft_segment(px, py, ax, ay, bx, by):
    """(d2, edge function, t for the depth) of the segment a -> b at the pixels.  Inside d2 the nearest point's parameter carries
    no gradient: d2's derivative through it is 0 (r orthogonal to the segment, or clamped); the t handed out does, where free."""
    ex, ey, wx, wy = bx - ax, by - ay, px - ax, py - ay
    dot, ee = wx * ex + wy * ey, ex * ex + ey * ey
    pos = ee > 0
    t_raw = torch.where(pos, dot / torch.where(pos, ee, torch.ones_like(ee)), torch.zeros_like(dot))
    t = t_raw.clamp(0, 1).detach()
    rx, ry = (1 - t) * wx + t * (px - bx), (1 - t) * wy + t * (py - by)   # p - c; an end takes (1 - t) or t of the gradient
    return rx * rx + ry * ry, ex * wy - ey * wx, torch.where((t_raw > 0) & (t_raw < 1), t_raw, t)


def soft_check_faces(name, faces):
    """The soft operators' `faces` check -> (batch size, num of faces)."""
    if not (torch.is_tensor(faces) and faces.is_floating_point() and faces.dim() == 4 and tuple(faces.shape[2:]) == (3, 3)
            and faces.shape[0] >= 1 and faces.shape[1] >= 1):
        raise ValueError('%s: faces must be a non-empty float tensor [batch size, num of faces, 3, 3]' % name)
    return int(faces.shape[0]), int(faces.shape[1])


def soft_check_image_size(name, image_size):
    if isinstance(image_size, bool) or not isinstance(image_size, int) or image_size < 1:
        raise ValueError('%s: image_size must be a positive integer, got %r' % (name, image_size))


def soft_fits(faces, image_size):
    """The device, dtype and size part of what the soft HIP kernels take (include/nr_hip.h)."""
    return (faces.is_cuda and faces.dtype == torch.float32 and faces.shape[0] <= 65535 and faces.shape[1] <= SOFT_MAX_FACES
            and faces.numel() < 2 ** 31 and image_size <= SOFT_MAX_SIZE)   # (numel: batch size * faces * 9)


_INDEX_ATTR = '_nr_index_ok'  # verdict stashed on a tensor OBJECT: it dies with the tensor (a cache keyed on data_ptr would
                               # be hit by an unrelated tensor that the caching allocator places at the same address)


def cached_on_index(faces, attr, key, build, not_built_message):
    """What `build()` derives on the host from the index tensor `faces` (and `key`: the vertex count, ...), cached on the
    tensor object -- and, for a view (`faces[None]`, `.expand`), on the tensor it is a view of, which lives on -- in a dict
    `attr` under the tensor's identity: data_ptr, shape, strides, version counter (an in-place edit builds anew), device,
    and `key`.  A build reads the indices back, so inside a HIP-graph capture a miss raises `not_built_message`."""
    stamp = (faces.data_ptr(), tuple(faces.shape), tuple(faces.stride()), faces._version, str(faces.device)) + tuple(key)
    holders = [faces] + ([faces._base] if faces._base is not None else [])
    for h in holders:
        hit = getattr(h, attr, {}).get(stamp)
        if hit is not None:
            return hit
    if faces.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(not_built_message)
    hit = build()
    for h in holders:
        try:
            table = getattr(h, attr, None)
            if table is None or len(table) > 8:
                table = {}
                setattr(h, attr, table)
            table[stamp] = hit
        except Exception:  # (a tensor subclass without __dict__: built every time)
            pass
    return hit


def _stamp(t, num_vertices):
    return (t._version, int(num_vertices), tuple(t.shape), tuple(t.stride()), t.storage_offset())


def check_face_indices(faces, num_vertices, device=None):
    """Vertex indices must lie in [0, num_vertices) and live on the vertices' device (the reference's get_item raises on
    a bad index; a raw kernel would read / atomically add outside the buffers).  The verdict is remembered as (version
    counter, num_vertices, geometry) on the index tensor itself -- and, for a VIEW (`faces[None]`, `.expand`, a slice built
    anew every step), on the tensor it is a view of, whose elements are a superset and whose object lives on: an
    optimisation loop pays the device round trip once, and an in-place edit (also through the view: views share the
    version counter) or another tensor is checked again.  Inside a HIP-graph capture nothing can be read back, so an
    index tensor without a verdict raises there: run one eager step first."""
    if device is not None and faces.device != device:
        raise ValueError('faces are on %s but vertices on %s' % (faces.device, device))
    stamp = _stamp(faces, num_vertices)
    if getattr(faces, _INDEX_ATTR, None) == stamp:
        return
    base = faces._base
    if base is not None and getattr(base, _INDEX_ATTR, None) == _stamp(base, num_vertices):
        return
    if faces.numel():
        if faces.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('face indices cannot be range-checked while a HIP graph is being captured (the check reads two '
                               'values back): call the renderer once with this index tensor before the capture')
        for t in ((base, faces) if base is not None else (faces,)):
            lo, hi = (int(x) for x in torch.aminmax(t.detach()))
            if 0 <= lo and hi < num_vertices:
                try:
                    setattr(t, _INDEX_ATTR, _stamp(t, num_vertices))
                except Exception:  # (a tensor subclass without __dict__: just check every time)
                    pass
                return
        raise IndexError('face vertex index out of range: [%d, %d] with %d vertices' % (lo, hi, num_vertices))
