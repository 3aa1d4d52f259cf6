"""_lib.dense, the tensor boundary of every HIP operator ("Tensor boundary"), on CPU tensors: the pointer
arithmetic is the device's.  An aligned contiguous tensor passes through as the same object; every other layout comes
back as a contiguous copy of the same values on a 16-byte boundary."""
import pytest
import torch

from neural_renderer_amd import _lib


def _aligned(shape, dtype):
    """A contiguous tensor of `shape` whose first element lies on a 16-byte boundary, filled with distinct values."""
    n = 1
    for s in shape:
        n *= s
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    buf = torch.zeros(n + per16, dtype=dtype)
    skip = (-buf.data_ptr() % 16) // buf.element_size()
    t = buf[skip:skip + n].view(shape)
    t.copy_(((torch.arange(n, dtype=torch.float64) * 3 + 1) % 251).reshape(shape).to(dtype))
    assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    return t


def _offset(t, k):
    """The values of t as a contiguous view that starts k elements behind a 16-byte boundary."""
    flat = _aligned((t.numel() + k,), t.dtype)
    v = flat[k:].view(t.shape)
    v.copy_(t)
    return v


def _layouts(t):
    size = t.element_size()
    out = {}
    for k in (1, 2, 3):
        if (k * size) % 16:
            v = _offset(t, k)
            assert v.is_contiguous() and v.data_ptr() % 16 == (k * size) % 16
            out['offset%d' % (k * size)] = v
    wide = _aligned(tuple(t.shape[:-1]) + (2 * t.shape[-1],), t.dtype)
    wide[..., ::2] = t
    out['strided'] = wide[..., ::2]
    perm = _aligned(tuple(reversed(t.shape)), t.dtype)
    perm.copy_(t.permute(*reversed(range(t.dim()))))
    out['permuted'] = perm.permute(*reversed(range(t.dim())))
    out['expanded'] = t[0:1].expand(3, *t.shape[1:])
    for name in ('strided', 'permuted', 'expanded'):
        assert not out[name].is_contiguous(), name
    return out


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64])
def test_dense(dtype):
    t = _aligned((2, 5, 3), dtype)
    assert _lib.dense(t) is t                      # one integer test, no copy
    assert _lib.dense(None) is None
    layouts = _layouts(t)
    if dtype in (torch.float32, torch.int32):
        assert set(layouts) >= {'offset4', 'offset8', 'offset12'}
    for name, v in layouts.items():
        want = v.clone(memory_format=torch.contiguous_format)
        before = v.clone(memory_format=torch.contiguous_format)
        d = _lib.dense(v)
        assert d is not v, name
        assert d.is_contiguous() and d.data_ptr() % 16 == 0, name
        assert d.dtype == v.dtype and d.device == v.device and d.shape == v.shape, name
        assert torch.equal(d, want), name
        assert torch.equal(v, before), name        # the caller's tensor is left alone
        assert _lib.dense(d) is d, name


def test_dense_keeps_aligned_views_and_empty_tensors():
    t = _aligned((4, 8), torch.float32)
    row = t[2]                                     # 32 floats in: contiguous and on the grid
    assert _lib.dense(row) is row
    half = t[1:].view(-1)[4:]
    assert half.data_ptr() % 16 == 0 and _lib.dense(half) is half
    odd = t.view(-1)[5:]
    assert odd.data_ptr() % 16 == 4
    d = _lib.dense(odd)
    assert d.data_ptr() % 16 == 0 and torch.equal(d, odd)
    e = torch.empty((0, 3))
    assert _lib.dense(e).shape == (0, 3)
