"""Memory behaviour of every operator wrapper under poisoned buffers (tests/poison.py, the table in tests/poison_cases.py):
no store outside an allocation or an input, every output element written, no unwritten scratch / stale buffer / halo
element beyond an input in a result, no input modified — and the same kernels, in the same order, giving the same bits
as a plain run."""
import importlib

import pytest
import torch

import poison
import poison_cases as pc
from util import launched_kernels

pytestmark = pytest.mark.gpu

LAUNCHED = set()          # sr_* names launched inside poisoned regions
RAN = set()               # ids of the cases that ran
_IN_POISON = [False]

# kernels of the harness itself (fills of the guards and interiors), and of torch.zeros in the plain run
_HARNESS_KERNELS = ("FillFunctor", "emset")


@pytest.fixture(scope="module", autouse=True)
def record_launches():
    """Wraps op._dispatch._launch (the one launcher of the wrappers) and records the names launched while poisoned."""
    from stylerenderer_amd.op import _dispatch

    real = _dispatch._launch

    def spy(fn, name, device, *args):
        if _IN_POISON[0]:
            LAUNCHED.add(name)
        return real(fn, name, device, *args)

    patch = pytest.MonkeyPatch()
    patch.setattr(_dispatch, "_launch", spy)
    yield
    patch.undo()


def _clear_caches():
    """Everything that would let the poisoned run reuse a buffer the plain run filled (per-weight `_sr_scratch` dicts
    do not travel: `embed` does not copy them)."""
    from stylerenderer_amd.op import _dispatch

    for mod in ("stylerenderer_amd.op.upfirdn2d", "stylerenderer_amd.op.rasterize", "stylerenderer_amd.op.weight_prep",
                "stylerenderer_amd.utils_3d"):
        for value in vars(importlib.import_module(mod)).values():
            if isinstance(value, _dispatch.DerivedCache):
                value.clear()


def _flat(out):
    return [out] if isinstance(out, torch.Tensor) or out is None else list(out)


def _kernels(names):
    return [n for n in names if not any(h in n for h in _HARNESS_KERNELS)]


def _plain_copy(t):
    c = t.detach().clone()
    for key, value in t.__dict__.items():
        setattr(c, key, value)
    return c.requires_grad_() if t.requires_grad else c


def _bits_equal(a, b):
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and bool((poison._bits(a) == poison._bits(b)).all())


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_poisoned_run(case, monkeypatch):
    RAN.add(case.id)
    for name in pc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for kv in case.env.items():
        monkeypatch.setenv(*kv)
    fn, inputs, inplace = case.build()
    is_t = [isinstance(t, torch.Tensor) for t in inputs]
    plain_in = [_plain_copy(t) if i in inplace else t for i, t in enumerate(inputs)]
    want, names_plain = launched_kernels(lambda: _flat(fn(*plain_in)))
    _clear_caches()
    with poison.poisoned(monkeypatch) as log:
        emb = [poison.embed(t) if is_t[i] else t for i, t in enumerate(inputs)]
        _IN_POISON[0] = True
        try:
            got, names = launched_kernels(lambda: _flat(fn(*emb)))
        finally:
            _IN_POISON[0] = False
    assert log.entries or inplace, "the call allocated nothing through the patched functions: nothing was poisoned"
    assert _kernels(names), "the profiler saw no kernel"
    waived = [got[case.waive[0]]] if case.waive is not None else []
    poison.check(log, got, [t for i, t in enumerate(emb) if is_t[i]], inplace=[emb[i] for i in inplace],
                 nonfinite_ok=waived)
    assert _kernels(names) == _kernels(names_plain), "the poisoned run launched other kernels than the plain run"
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), i
        if a is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, i
        same = _bits_equal(a, b) if any(a is w for w in waived) else torch.equal(a, b)
        assert same, "output %d %s differs from the plain run in %d element(s)" % (
            i, tuple(a.shape), int((a != b).sum()))


@pytest.mark.parametrize("op, message", [
    ("op_unwritten_output", "unwritten or poisoned value: output 0"), ("op_store_past_end", "stray store: back guard"),
    ("op_store_before_start", "stray store: front guard"), ("op_reads_unwritten_scratch", "index \\(3,\\)"),
    ("op_reads_past_input", "index \\(36,\\)"), ("op_modifies_input", "input modified")])
def test_harness_catches_the_planted_defects_in_device_memory_too(op, message, monkeypatch):
    """The stand-in operators of tests/test_poison_cpu.py on device tensors: plain tensor indexing inside the harness's
    own flat buffers (nothing leaves memory the test owns), so that the guards, the NaN fill and the checks are shown to
    work on the device the table above runs on."""
    import test_poison_cpu as host

    log, y, x = host._run(getattr(host, op), monkeypatch, device="cuda")
    assert y.is_cuda and x.is_cuda and all(flat.is_cuda for flat, _, _ in log)
    with pytest.raises(AssertionError, match=message):
        poison.check(log, [y], [x])
    log, y, x = host._run(host.op_clean, monkeypatch, device="cuda")
    poison.check(log, [y], [x])


def test_every_required_function_was_launched_inside_a_poisoned_region():
    if RAN != {c.id for c in pc.CASES}:
        pytest.skip("needs the whole table above to have run in this process")
    missing = sorted(set(pc.REQUIRED) - LAUNCHED)
    assert not missing, missing
