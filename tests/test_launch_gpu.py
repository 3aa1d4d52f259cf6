"""The one launch path of the Python operators (neural_renderer_amd/_lib.py: launch, on_device, stream_ptr): which arguments
an entry point receives, which device is current while it runs, which stream it is handed, who owns the workspace, and which
status becomes which exception.  The entries here are Python functions attached to the loaded library object, so no kernel is
launched -- except by the one real operator at the end."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Fake(object):
    """An entry point that records its arguments and the current device, and returns `status`."""

    def __init__(self, status=0):
        self.status, self.calls, self.devices = status, [], []

    def __call__(self, *args):
        self.calls.append(args)
        self.devices.append(torch.cuda.current_device())
        return self.status


def _here():
    return torch.device('cuda', torch.cuda.current_device())


def test_arguments_workspace_and_stream(monkeypatch):
    """Without workspace_bytes the entry gets the arguments and the current stream; with it, (pointer, bytes) in front of the
    stream: a 16-byte aligned buffer on the device, the byte count unchanged, and a real buffer behind 0 bytes."""
    from neural_renderer_amd import _lib
    lib, dev = _lib.load(), _here()
    fake = _Fake()
    monkeypatch.setattr(lib, 'nr_fake', fake, raising=False)
    args = (7, 2.5, None)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert _lib.launch('nr_fake', dev, *args) is None
        _lib.launch('nr_fake', dev, *args, workspace_bytes=48)
        _lib.launch('nr_fake', dev, *args, workspace_bytes=0)
    _lib.launch('nr_fake', dev, *args)
    plain, with_ws, empty_ws, default = fake.calls
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    assert plain == args + (side.cuda_stream,)
    assert with_ws[:3] == args and with_ws[4:] == (48, side.cuda_stream) and len(with_ws) == 6
    assert with_ws[3] != 0 and with_ws[3] % 16 == 0
    assert empty_ws[:3] == args and empty_ws[4:] == (0, side.cuda_stream) and len(empty_ws) == 6
    assert empty_ws[3] != 0
    assert default == args + (torch.cuda.current_stream().cuda_stream,)
    assert _lib.stream_ptr(dev) == torch.cuda.current_stream(dev).cuda_stream


def test_status_becomes_exception(monkeypatch):
    """0 returns; NR_E_INDEX raises IndexError; any other status raises NRError that names the entry."""
    from neural_renderer_amd import _lib
    lib, dev = _lib.load(), _here()
    fake = _Fake()
    monkeypatch.setattr(lib, 'nr_fake_status', fake, raising=False)
    _lib.launch('nr_fake_status', dev, 1)
    fake.status = _lib.NR_E_INDEX
    with pytest.raises(IndexError, match='nr_fake_status'):
        _lib.launch('nr_fake_status', dev, 1)
    fake.status = -1
    with pytest.raises(_lib.NRError, match='nr_fake_status'):
        _lib.launch('nr_fake_status', dev, 1, workspace_bytes=16)
    assert len(fake.calls) == 3
    with pytest.raises(AttributeError):
        _lib.launch('nr_no_such_entry', dev)


def test_entry_is_looked_up_at_every_call(monkeypatch):
    """An attribute replaced after a first call is the one the second call reaches."""
    from neural_renderer_amd import _lib
    lib, dev = _lib.load(), _here()
    first, second = _Fake(), _Fake()
    monkeypatch.setattr(lib, 'nr_fake', first, raising=False)
    _lib.launch('nr_fake', dev, 1)
    monkeypatch.setattr(lib, 'nr_fake', second, raising=False)
    _lib.launch('nr_fake', dev, 2)
    assert [c[0] for c in first.calls] == [1] and [c[0] for c in second.calls] == [2]


def test_current_device_takes_no_guard():
    """A launch for the device that is current takes the shared no-op context, not a torch.cuda.device."""
    from neural_renderer_amd import _lib
    assert _lib.on_device(_here()) is _lib._NO_GUARD
    with _lib.on_device(_here()) as guard:
        assert guard is _lib._NO_GUARD


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
def test_other_device_is_current_during_the_call(monkeypatch):
    """With cuda:0 current, a launch for cuda:1 runs with device 1 current, on cuda:1's current stream, with its workspace
    there, and leaves device 0 current."""
    from neural_renderer_amd import _lib
    lib = _lib.load()
    fake = _Fake()
    monkeypatch.setattr(lib, 'nr_fake', fake, raising=False)
    other = torch.device('cuda', 1)
    with torch.cuda.device(0):
        with torch.cuda.device(other):   # `side` becomes cuda:1's current stream; leaving the block puts device 0 back
            side = torch.cuda.Stream()
            torch.cuda.set_stream(side)
        try:
            assert torch.cuda.current_device() == 0 and _lib.on_device(other) is not _lib._NO_GUARD
            _lib.launch('nr_fake', other, 5, workspace_bytes=32)
            assert torch.cuda.current_device() == 0
            _lib.launch('nr_fake', other, 6)
            assert torch.cuda.current_device() == 0
        finally:
            with torch.cuda.device(other):
                torch.cuda.set_stream(torch.cuda.default_stream(other))
        assert fake.devices == [1, 1]
        assert side.cuda_stream != torch.cuda.default_stream(other).cuda_stream
        assert fake.calls[0][0] == 5 and fake.calls[0][2:] == (32, side.cuda_stream) and fake.calls[0][1] != 0
        assert fake.calls[1] == (6, side.cuda_stream)


def test_face_normals_on_a_side_stream(monkeypatch):
    """One real operator through the helper: nr_face_normals_forward is handed the side stream's handle as its last argument,
    and the result equals the default-stream call bit for bit."""
    import neural_renderer_amd as nr
    from neural_renderer_amd import _lib
    lib, dev = _lib.load(), _here()
    vertices = torch.tensor([[[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]], device=dev)
    faces = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32, device=dev)
    ref = nr.face_normals(vertices, faces, implementation='hip')
    torch.cuda.synchronize()
    real, seen = lib.nr_face_normals_forward, []

    def counting(*args):
        seen.append(args[-1])
        return real(*args)
    monkeypatch.setattr(lib, 'nr_face_normals_forward', counting, raising=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = nr.face_normals(vertices, faces, implementation='hip')
    side.synchronize()
    assert seen == [side.cuda_stream]
    assert got.shape == (1, 4, 3) and bool(got.abs().sum() > 0)
    assert torch.equal(got, ref)
