"""The one call path of the host mirrors (semi-detr_amd/_lib.py: ``call``, ``calls``, ``ptr_args``, ``device_guard``, ``small_to_device``,
``offsets``) on the host: argument conversion, name and status handling, and the small host-list helpers.  The library handle
is a fake that records what it is called with; nothing is launched."""
import contextlib
import ctypes
import types

import pytest
import torch

from semi_detr_amd import _lib

CPU = torch.device("cpu")
STREAM = 0x5EED0


class FakeLib:
    """Stands in for the ctypes handle: ``semidetr_ema_flat_f32`` records its arguments and returns ``rc``."""

    def __init__(self, rc=0, error=b"something the library said"):
        self.rc, self.error, self.calls = rc, error, []

    def semidetr_ema_flat_f32(self, *args):
        self.calls.append(args)
        return self.rc

    def semidetr_last_error(self):
        return self.error


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        lib = FakeLib(**kw)
        monkeypatch.setattr(_lib, "_lib", lib)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(cuda_stream=STREAM))
        return lib
    return install


def test_ptr_args_tensor_and_none():
    t = torch.arange(6, dtype=torch.float32)
    got = _lib.ptr_args([t, None, t[2:]])
    assert isinstance(got[0], ctypes.c_void_p) and got[0].value == t.data_ptr()
    assert got[1] is None
    assert isinstance(got[2], ctypes.c_void_p) and got[2].value == t.data_ptr() + 8


def test_ptr_args_passes_everything_else_through():
    params = _lib.CostParams()
    args = [3, 0.25, ctypes.c_float(0.4), ctypes.byref(params), (ctypes.c_int64 * 4)(1, 2, 3, 4)]
    got = _lib.ptr_args(args)
    assert len(got) == len(args) and all(g is a for g, a in zip(got, args))


def test_call_passes_stream_first_then_converted_arguments(fake):
    lib = fake()
    t, s = torch.zeros(8), torch.ones(8)
    assert _lib.call("semidetr_ema_flat_f32", CPU, t, s, 8, 0.5) is None
    (args,) = lib.calls
    assert isinstance(args[0], ctypes.c_void_p) and args[0].value == STREAM
    assert [a.value for a in args[1:3]] == [t.data_ptr(), s.data_ptr()]
    assert args[3:] == (8, 0.5)


def test_calls_share_one_stream_lookup_and_stop_at_a_failing_status(fake, monkeypatch):
    lib = fake()
    looked_up = []
    monkeypatch.setattr(torch.cuda, "current_stream",
                        lambda dev=None: looked_up.append(dev) or types.SimpleNamespace(cuda_stream=STREAM))
    t = torch.zeros(4)
    _lib.calls(CPU, ("semidetr_ema_flat_f32", t, t, 4, 0.5), ("semidetr_ema_flat_f32", t, None, 4, 0.25))
    assert looked_up == [CPU] and [c[0].value for c in lib.calls] == [STREAM, STREAM]
    assert lib.calls[1][2] is None and lib.calls[1][3:] == (4, 0.25)
    with pytest.raises(AttributeError):                      # every name is resolved before the first launch
        _lib.calls(CPU, ("semidetr_ema_flat_f32", t, t, 4, 0.5), ("semidetr_not_in_the_abi", t))
    assert len(lib.calls) == 2
    lib.rc = -1
    with pytest.raises(RuntimeError, match=r"^semidetr_ema_flat_f32 failed \(code -1\)"):
        _lib.calls(CPU, ("semidetr_ema_flat_f32", t, t, 4, 0.5), ("semidetr_ema_flat_f32", t, t, 4, 0.5))
    assert len(lib.calls) == 3                               # the second launch did not happen


def test_call_unknown_name_raises_before_anything_is_launched(fake):
    lib = fake()
    lib.semidetr_not_in_the_abi = lib.semidetr_ema_flat_f32          # present on the handle, absent from SIGNATURES
    with pytest.raises(AttributeError, match="semidetr_not_in_the_abi"):
        _lib.call("semidetr_not_in_the_abi", CPU, torch.zeros(1))
    with pytest.raises(AttributeError):
        _lib.call("semidetr_msda_set_variant_typo", CPU)
    assert lib.calls == []


def test_call_failing_status_raises_with_the_name_once_and_the_last_error(fake):
    lib = fake(rc=-1, error=b"n must be >= 0")
    with pytest.raises(RuntimeError) as e:
        _lib.call("semidetr_ema_flat_f32", CPU, torch.zeros(1), torch.zeros(1), 1, 0.5)
    assert str(e.value) == "semidetr_ema_flat_f32 failed (code -1): n must be >= 0"
    assert len(lib.calls) == 1


def test_device_guard_choice(monkeypatch):
    made = []
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: made.append(dev) or contextlib.nullcontext())
    assert _lib.device_guard(torch.device("cuda", 1)) is _lib.device_guard(torch.device("cuda")) is _lib.device_guard(CPU)
    assert made == []                                   # current device, or no index: the shared no-op, no guard object
    _lib.device_guard(torch.device("cuda", 0))
    assert made == [torch.device("cuda", 0)]


def test_offsets():
    host, dev = _lib.offsets([3, 0, 2], CPU)
    assert host == [0, 3, 3, 5]
    assert dev.dtype == torch.int32 and dev.device == CPU and dev.tolist() == host
    host, dev = _lib.offsets([], CPU)
    assert host == [0] and dev.tolist() == [0]


@pytest.mark.parametrize("dtype", [torch.int32, torch.float32])
def test_small_to_device_on_the_cpu(dtype):
    values = [[1333, 800], [640, 480]]
    t = _lib.small_to_device(values, dtype, CPU)
    assert t.dtype == dtype and t.device == CPU and t.tolist() == values
