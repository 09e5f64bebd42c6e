"""The poisoned-buffer harness (tests/poison.py) must be able to fail: stand-in "operators" written with plain tensor
indexing on the host, each with one planted memory defect, and `check` has to raise and name it.  Also the coverage
bookkeeping of tests/poison_cases.py (no device needed)."""
import os
import re

import pytest
import torch

import poison
from poison import check, embed, poisoned

CPU = ("cpu",)
N = 37                                  # odd, no multiple of anything


def _flat_of(log, t):
    """(flat buffer, guard) of the logged allocation or embedded input whose interior is `t`."""
    for e in log.entries + log.inputs:
        if e.view.data_ptr() == t.data_ptr():
            return e.flat, e.guard
    raise AssertionError("not a guarded tensor")


# ---- stand-in operators: y = 2 * x through a scratch buffer, the way a wrapper allocates ------------------------------
def op_clean(x, log):
    scratch = torch.empty(N, dtype=x.dtype, device=x.device)
    y = torch.empty_like(x)
    scratch[:] = x
    y[:] = scratch * 2
    return y


def op_unwritten_output(x, log):
    y = torch.empty_like(x)
    y[:N - 1] = x[:N - 1] * 2           # the last element is never stored
    return y


def op_store_past_end(x, log):
    y = op_clean(x, log)
    flat, g = _flat_of(log, y)
    flat[g + N] = 1.0                   # one element past the output's end
    return y


def op_store_before_start(x, log):
    y = op_clean(x, log)
    flat, g = _flat_of(log, y)
    flat[g - 1] = 1.0                   # one element before the output's start
    return y


def op_reads_unwritten_scratch(x, log):
    scratch = x.new_empty(N)
    scratch[:N - 1] = x[:N - 1]         # slot N - 1 has no producer
    y = torch.zeros_like(x)
    y += x * 2
    y[3] += 0 * scratch[N - 1]          # ... and a consumer
    return y


def op_reads_past_input(x, log):
    flat, g = _flat_of(log, x)
    y = torch.empty_like(x)
    y[:] = x * 2
    y[N - 1] += 0 * flat[g + N]         # the halo element just past the input's end
    return y


def op_modifies_input(x, log):
    y = op_clean(x, log)
    x[5] = -x[5]
    return y


def _run(op, monkeypatch, device="cpu"):
    x0 = torch.arange(1, N + 1, dtype=torch.float32, device=device)
    with poisoned(monkeypatch, devices=(device,)) as log:
        x = embed(x0)
        y = op(x, log)
    return log, y, x


def test_clean_operator_passes(monkeypatch):
    log, y, x = _run(op_clean, monkeypatch)
    check(log, [y], [x])
    assert torch.equal(y, 2 * torch.arange(1, N + 1, dtype=torch.float32))
    assert len(log) == 2 and all(site.startswith(__file__.rsplit(".", 1)[0]) for _, _, site in log)
    flat, view, _ = log[0]
    assert view.shape == (N,) and flat.numel() == N + 2 * 4096


@pytest.mark.parametrize("op, names", [
    (op_unwritten_output, ("unwritten or poisoned value: output 0", "1 non-finite", "index (36,)")),
    (op_store_past_end, ("stray store: back guard", "0 element(s) past its end", "empty_like")),
    (op_store_before_start, ("stray store: front guard", "1 element(s) before its start", "empty_like")),
    (op_reads_unwritten_scratch, ("unwritten or poisoned value: output 0", "index (3,)")),
    (op_reads_past_input, ("unwritten or poisoned value: output 0", "index (36,)")),
    (op_modifies_input, ("input modified", "flat offset 5")),
], ids=lambda v: v.__name__[3:] if callable(v) else "")
def test_planted_defect_is_caught_and_named(op, names, monkeypatch):
    log, y, x = _run(op, monkeypatch)
    with pytest.raises(AssertionError) as err:
        check(log, [y], [x])
    text = str(err.value)
    for part in names:
        assert part in text, (part, text)
    assert len(text.splitlines()) == 1, text                   # the planted defect and nothing else
    assert os.path.basename(__file__) in text or "input modified" in text    # the allocation site is named


def test_inplace_inputs_may_change_but_their_guards_may_not(monkeypatch):
    log, y, x = _run(op_modifies_input, monkeypatch)
    check(log, [y], [x], inplace=[x])
    flat, g = _flat_of(log, x)
    flat[g + N + 7] = 0.0
    with pytest.raises(AssertionError, match="back guard of the input .* 7 element"):
        check(log, [y], [x], inplace=[x])


def test_layout_alignment_zeros_and_integer_buffers(monkeypatch):
    with poisoned(monkeypatch, devices=CPU) as log:
        a = torch.empty((3, 5, 300), dtype=torch.float32)
        z = torch.zeros(size=(2, 7))
        i = torch.empty(11, dtype=torch.int32)
        zi = a.new_zeros((4,), dtype=torch.uint8)
        h = torch.empty_like(a, dtype=torch.float16)
        t = torch.empty_like(a.permute(2, 0, 1))               # dense, not contiguous: strides kept
        elsewhere = torch.empty(3, device="meta")              # another device: the real function
    assert len(log) == 6 and elsewhere.device.type == "meta"
    for e in log.entries:
        assert e.guard >= max(4096, 16 * e.view.shape[-1]) and (e.guard * e.flat.element_size()) % 512 == 0
        assert (e.view.data_ptr() - e.flat.data_ptr()) == e.guard * e.flat.element_size()
    assert log.entries[0].guard == 38 * 128                     # 16 * 300 = 4800 -> next multiple of 128 floats
    assert torch.isnan(a).all() and torch.isnan(h).all() and a.is_contiguous()
    assert t.stride() == a.permute(2, 0, 1).stride() and t.shape == (300, 3, 5)
    assert (z == 0).all() and (zi == 0).all() and z.shape == (2, 7)
    for e in (log.entries[1],):
        assert torch.isnan(e.flat[:e.guard]).all() and torch.isnan(e.flat[e.guard + e.numel:]).all()
    for e in (log.entries[2], log.entries[3]):
        raw = e.flat.view(torch.uint8)
        n = e.guard * e.flat.element_size()
        assert (raw[:n] == poison.INT_FILL).all() and (raw[-n:] == poison.INT_FILL).all()
    check(log, [z], [])
    i[:] = 1                                                   # writing an integer interior is no damage
    check(log, [z], [])
    log.entries[2].flat[log.entries[2].guard + 11] = 0
    with pytest.raises(AssertionError, match="back guard of the empty .* 0 element"):
        check(log, [z], [])


def test_embed_keeps_shape_strides_grad_flag_and_attributes(monkeypatch):
    src = torch.randn(4, 6, 5).permute(1, 0, 2).requires_grad_()
    w = torch.randn(8)
    w._sr_frozen = True
    w._sr_scratch = {"stale": 1}
    with poisoned(monkeypatch, devices=CPU) as log:
        e = embed(src)
        ew = embed(w)
        sliced = embed(torch.randn(4, 8)[:, :5])               # gaps: embedded contiguous
    assert torch.equal(e, src) and e.stride() == src.stride() and e.requires_grad and e.is_leaf
    assert ew._sr_frozen and not hasattr(ew, "_sr_scratch")
    assert sliced.is_contiguous() and sliced.shape == (4, 5)
    assert len(log) == 0 and len(log.inputs) == 3
    check(log, [], [e, ew, sliced])


def test_autograd_works_through_poisoned_allocations(monkeypatch):
    class Double(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            y = torch.empty_like(x)
            y.copy_(x * 2)
            return y

        @staticmethod
        def backward(ctx, g):
            gx = torch.zeros_like(g)
            gx += 2 * g
            return gx

    x0 = torch.randn(5, 3, requires_grad=True)
    with poisoned(monkeypatch, devices=CPU) as log:
        x = embed(x0)
        y = Double.apply(x)
        (gx,) = torch.autograd.grad(y.sum(), x)
    check(log, [y, gx], [x])
    assert len(log) == 2 and torch.equal(gx, torch.full((5, 3), 2.0))


def test_patches_are_gone_after_the_block_also_after_an_exception(monkeypatch):
    names = [(torch, "empty"), (torch, "zeros"), (torch, "empty_like"), (torch, "zeros_like"),
             (torch.Tensor, "new_empty"), (torch.Tensor, "new_zeros")]
    before = [getattr(o, n) for o, n in names]
    with poisoned(monkeypatch, devices=CPU):
        assert all(getattr(o, n) is not b for (o, n), b in zip(names, before))
    assert all(getattr(o, n) is b for (o, n), b in zip(names, before))
    with pytest.raises(RuntimeError, match="planted"):
        with poisoned(monkeypatch, devices=CPU):
            raise RuntimeError("planted")
    assert all(getattr(o, n) is b for (o, n), b in zip(names, before))
    assert not poison._ACTIVE
    monkeypatch.undo()
    assert all(getattr(o, n) is b for (o, n), b in zip(names, before))


# ---- the case table's bookkeeping ------------------------------------------------------------------------------------
def test_required_functions_exist_and_cover_every_native_call_of_the_wrapper_modules():
    import poison_cases as pc
    from stylerenderer_amd import _lib

    assert len(set(pc.REQUIRED)) == len(pc.REQUIRED)
    missing = [n for n in pc.REQUIRED if n not in _lib.SIGNATURES]
    assert not missing, missing
    op_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stylerenderer_amd", "op")
    found = set()
    for mod in pc.WRAPPER_MODULES:
        with open(os.path.join(op_dir, mod + ".py")) as f:
            found |= pc.native_calls(f.read())
    assert found, "the search pattern finds nothing"
    assert found <= set(pc.REQUIRED), sorted(found - set(pc.REQUIRED))
    assert set(pc.REQUIRED) <= found, sorted(set(pc.REQUIRED) - found)


def test_native_call_search_sees_every_way_the_wrappers_spell_a_call():
    import poison_cases as pc

    src = ('native(x).sr_a(1)\nrun = native(x)\nrun.sr_b(2)\nrun.sr_c(3)\n'
           'getattr(native(v), "sr_d_" + suf)(4)\nL.sr_query(5)\n_lib.lib().sr_other_query(6)\n')
    assert pc.native_calls(src) == {"sr_a", "sr_b", "sr_c", "sr_d_f32", "sr_d_f64"}


def test_case_ids_are_unique_and_at_most_one_case_in_ten_carries_a_waiver():
    import poison_cases as pc

    ids = [c.id for c in pc.CASES]
    assert len(set(ids)) == len(ids)
    waived = [c.id for c in pc.CASES if c.waive is not None]
    assert all(re.search(r"\w", c.waive[1]) for c in pc.CASES if c.waive is not None)       # each gives its reason
    assert 10 * len(waived) <= len(ids), waived
