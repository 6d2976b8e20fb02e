"""``_lib.call`` on the GPU: the launch goes to the current stream of the tensors' device, no device guard is built when that
device is already current, and a device that is not current is made current for the call only."""
import pytest
import torch

from semi_detr_amd import _lib, ema_update_flat_

pytestmark = pytest.mark.gpu
N = 4096


class Recorder:
    """The real handle, keeping the first argument (the stream) of every call made through it."""

    def __init__(self, handle):
        self._handle, self.streams = handle, []

    def __getattr__(self, name):
        fn = getattr(self._handle, name)

        def record(*args):
            if args:
                self.streams.append(getattr(args[0], "value", args[0]))
            return fn(*args)
        return record


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


def _pair(dev, seed):
    """Teacher and student in [0.5, 1.5): both terms of the update have one sign, see ``_check``."""
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(N, device=dev, generator=g) + 0.5, torch.rand(N, device=dev, generator=g) + 0.5


def _check(teacher, t0, s, m):
    """Against ``m * t + (1 - m) * s`` by torch in fp32.  The kernel rounds ``m * t`` and folds ``(1 - m) * s`` into the sum
    unrounded (csrc/ema.hip); torch rounds both products.  For m = 0.5 the second product is exact, so both give the same
    value.  Otherwise the sums differ, before their one rounding, by at most half an ulp of ``(1 - m) * s``, which for terms
    of one sign is at most half an ulp of the sum: the rounded results are equal or neighbours."""
    want = m * t0 + (1 - m) * s
    if m == 0.5:
        assert torch.equal(teacher, want)
    else:
        inf = torch.full_like(want, float("inf"))
        assert ((teacher == want) | (teacher == torch.nextafter(want, inf)) | (teacher == torch.nextafter(want, -inf))).all()


@pytest.mark.parametrize("m", [0.5, 0.999])
def test_launch_goes_to_the_current_stream_of_the_tensors(recorder, m):
    dev = torch.device("cuda", torch.cuda.current_device())
    t, s = _pair(dev, 0)
    t0 = t.clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ema_update_flat_(t, s, m)
    assert recorder.streams == [side.cuda_stream]
    assert side.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    side.synchronize()
    _check(t, t0, s, m)


def test_no_guard_object_for_the_current_device(recorder, monkeypatch):
    dev = torch.device("cuda", torch.cuda.current_device())
    t, s = _pair(dev, 1)
    t0 = t.clone()
    torch.cuda.synchronize(dev)
    made = []

    class Counting(torch.cuda.device):               # a class: torch itself tests ``isinstance(x, torch.cuda.device)``
        def __init__(self, *a, **kw):
            made.append(a)
            super().__init__(*a, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "device", Counting)
        ema_update_flat_(t, s, 0.5)
    assert made == []
    torch.cuda.synchronize(dev)
    _check(t, t0, s, 0.5)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="torch.cuda.device_count() < 2: no second GPU")
def test_device_that_is_not_current(recorder):
    with torch.cuda.device(0):
        dev = torch.device("cuda", 1)
        t, s = _pair(dev, 2)
        t0 = t.clone()
        torch.cuda.synchronize(dev)
        ema_update_flat_(t, s, 0.5)
        assert recorder.streams == [torch.cuda.current_stream(1).cuda_stream]
        assert torch.cuda.current_device() == 0
        torch.cuda.synchronize(dev)
        _check(t, t0, s, 0.5)
