"""CPU: `op._dispatch.native`, the one launcher of the operator wrappers, against a recording stand-in for the loaded
library and a stubbed stream — what reaches the C function, in which order, and how a failure is reported."""
import pytest
import torch

from stylerenderer_amd import _lib
from stylerenderer_amd.op._dispatch import native

STREAM = 0x5EED


class Recorder:
    """Stands in for the ctypes handle: every `sr_*` attribute records its arguments and returns `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def sr_error_string(self, rc):
        return b"invalid argument"

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.rc

        return fn


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda device=None: STREAM)
    return rec


def test_tensors_become_pointers_and_the_rest_passes_through_in_order(recorder):
    a, b = torch.zeros(4), torch.zeros(2, 3)
    empty = torch.empty(0)
    raw = b.data_ptr() + 4 * 3
    assert native(a).sr_some_kernel(a, None, empty, 7, 0.25, raw, b, -1) is None
    (name, args), = recorder.calls
    assert name == "sr_some_kernel"
    assert args == (a.data_ptr(), None, None, 7, 0.25, raw, b.data_ptr(), -1, STREAM)
    assert type(args[3]) is int and type(args[4]) is float and type(args[5]) is int


def test_the_stream_is_the_last_argument_even_without_others(recorder):
    native(torch.zeros(1)).sr_no_arguments()
    assert recorder.calls == [("sr_no_arguments", (STREAM,))]


def test_a_failure_raises_under_the_name_that_was_called(recorder):
    recorder.rc = 1
    a = torch.zeros(4)
    with pytest.raises(RuntimeError, match="sr_called_by_this_name failed: invalid argument") as e:
        native(a).sr_called_by_this_name(a, 4)
    assert "code 1" in str(e.value)
    assert recorder.calls == [("sr_called_by_this_name", (a.data_ptr(), 4, STREAM))]
