"""Poisoned buffers: every tensor an operator wrapper allocates, and every input a test hands it, sits between two guard
regions inside a larger flat buffer, and what the call never wrote reads as NaN.

    with poisoned(monkeypatch) as log:        # torch.empty / empty_like / new_empty / zeros / zeros_like / new_zeros
        x = embed(x0, log)                    # inputs: copied into a guarded buffer of their own
        y = op(x)
    check(log, [y], [x])

Layout of one flat buffer: [front guard | interior | back guard].  Each guard has max(4096, 16 * last dimension)
elements, rounded up to a multiple of 512 bytes: the interior starts a multiple of 512 bytes into an allocation of the
caching allocator, so its alignment relative to 512 bytes is that of a plain allocation and every alignment-dependent
dispatch rule picks the kernel it picks in production.  The interior is a tensor of its own over the flat buffer's
storage (`set_`, no autograd view relation to the flat buffer), contiguous, or with the dense strides of the source for
`empty_like` / `zeros_like` / `embed` of a dense tensor.

Floating-point buffers: guards and interior are NaN for the `empty` family; for the `zeros` family the guards are NaN
and the interior is zero.  Integer, byte and bool buffers: the guards hold the byte 0xA5; the interior is left as the
allocator returned it (zero for the `zeros` family).

`check` then finds
  * a store before the start or past the end of any allocation or input (a guard no longer holds its fill),
  * an output element the call never wrote, and a result that used unwritten scratch, an unwritten output or an element
    outside an input (it is NaN — or, where a select or a max hides the NaN, differs from the plain run, which the
    caller compares bit for bit),
  * an input the call modified.

Limits, by construction:
  * A stray access further than one guard from the buffer it belongs to is not seen.
  * Integer interiors are never poisoned.  A poisoned index, count or flag that a kernel did read could send that
    kernel out of bounds; this harness must find defects without causing a fault.  An integer scratch slot that is read
    before it is written is therefore visible only through the bit-for-bit comparison with the plain run.
  * Only allocations made through the six patched functions are guarded; what ATen allocates for its own operators
    (`a * b`, `.sum()`, `.contiguous()`) is not.
"""
import contextlib
import math
import sys

import torch

MIN_GUARD = 4096               # elements; the guard tests/test_convt_wino_gpu.py puts behind its output
INT_FILL = 0xA5                # every byte of an integer buffer's guards
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_HERE = __file__.rsplit(".", 1)[0]
_ACTIVE = []                   # the logs of the poisoned blocks that are open, innermost last


class Entry:
    """One guarded buffer: `flat` = [guard | interior | guard], `view` the tensor handed out."""
    __slots__ = ("flat", "view", "site", "guard", "numel", "kind", "before")

    def __init__(self, flat, view, site, guard, numel, kind):
        self.flat, self.view, self.site, self.guard, self.numel, self.kind = flat, view, site, guard, numel, kind
        self.before = None     # embedded inputs: the interior's bits before the call

    def as_tuple(self):
        return self.flat, self.view, self.site


class Log(list):
    """The (flat buffer, interior view, allocating file:line) records of one poisoned region; `entries` holds the same
    with the layout, `inputs` the embedded inputs."""

    def __init__(self):
        super().__init__()
        self.entries = []
        self.inputs = []

    def _add(self, entry, is_input=False):
        (self.inputs if is_input else self.entries).append(entry)
        if not is_input:
            self.append(entry.as_tuple())


def guard_elems(last_dim, itemsize):
    n = max(MIN_GUARD, 16 * int(last_dim))
    unit = max(512 // itemsize, 1)
    return (n + unit - 1) // unit * unit


def _bits(t):
    """A 1-D tensor's elements as integers of the same width."""
    return t.view(_BITS[t.element_size()])


def _site():
    """file:line of the nearest frame outside this module (the wrapper line that allocates)."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename.rsplit(".", 1)[0] == _HERE:
        f = f.f_back
    return "%s:%d" % (f.f_code.co_filename, f.f_lineno) if f is not None else "?"


def _dense_strides(src):
    """The strides to reproduce for a *_like of / an embedding of `src`: its own where they tile a block of numel
    elements without gaps or overlap (torch's preserve_format rule), else contiguous ones."""
    if src.is_contiguous() or src.numel() == 0:
        return None
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(src.shape, src.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return None
        expect *= size
    return tuple(src.stride())


def _guarded(real_empty, shape, dtype, device, zero, strides, site, kind):
    shape = tuple(int(s) for s in shape)
    numel = math.prod(shape)
    item = dtype.itemsize
    guard = guard_elems(shape[-1] if shape else 1, item)
    flat = real_empty(guard + numel + guard, dtype=dtype, device=device)
    if dtype.is_complex:
        raise NotImplementedError("poison: complex buffers")
    if dtype.is_floating_point:
        flat.fill_(float("nan"))
    else:
        raw = flat.view(torch.uint8)
        raw[:guard * item].fill_(INT_FILL)
        raw[(guard + numel) * item:].fill_(INT_FILL)
    if zero and numel:
        flat[guard:guard + numel].zero_()
    view = real_empty(0, dtype=dtype, device=device)
    if strides is None:
        strides = []
        acc = 1
        for s in reversed(shape):
            strides.append(acc)
            acc *= max(s, 1)
        strides = tuple(reversed(strides))
    view.set_(flat.untyped_storage(), flat.storage_offset() + guard, shape, strides)
    return Entry(flat, view, site, guard, numel, kind)


def _shape_of(args, kwargs):
    if "size" in kwargs:
        return tuple(kwargs.pop("size"))
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0])
    return tuple(args)


def _wants(device, devices):
    return torch.device(device).type in devices


_PLAIN_KW = {"dtype", "device", "requires_grad", "layout", "pin_memory", "memory_format"}


@contextlib.contextmanager
def poisoned(monkeypatch, devices=("cuda",)):
    """Replaces the six allocation functions for tensors on `devices`; yields the Log.  The replacements are taken back
    when the block ends, also by an exception (and again, harmlessly, by monkeypatch's own teardown)."""
    devices = tuple(devices)
    log = Log()
    real = {"empty": torch.empty, "zeros": torch.zeros, "empty_like": torch.empty_like, "zeros_like": torch.zeros_like,
            "new_empty": torch.Tensor.new_empty, "new_zeros": torch.Tensor.new_zeros}
    real_empty = real["empty"]

    def finish(entry, requires_grad):
        log._add(entry)
        return entry.view.requires_grad_() if requires_grad else entry.view

    def simple(kw):
        """Whether the keyword arguments are ones the replacement reproduces (else: the real function)."""
        return (set(kw) <= _PLAIN_KW and kw.get("layout", torch.strided) is torch.strided and not kw.get("pin_memory")
                and kw.get("memory_format", torch.contiguous_format) in (torch.contiguous_format, torch.preserve_format))

    def factory(name, zero):
        def fn(*args, **kwargs):
            kw = dict(kwargs)
            out = kw.pop("out", None)
            device = kw.get("device")
            device = torch.device(device) if device is not None else real_empty(0).device
            shape = _shape_of(args, kw)
            if out is not None or not simple(kw) or not _wants(device, devices):
                return real[name](*args, **kwargs)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            return finish(_guarded(real_empty, shape, dtype, device, zero, None, _site(), name), kw.get("requires_grad"))
        fn.__name__ = name
        return fn

    def like(name, zero):
        def fn(src, **kwargs):
            device = torch.device(kwargs["device"]) if kwargs.get("device") is not None else src.device
            if not simple(kwargs) or not _wants(device, devices) or src.layout is not torch.strided:
                return real[name](src, **kwargs)
            dtype = kwargs.get("dtype") or src.dtype
            fmt = kwargs.get("memory_format", torch.preserve_format)
            strides = _dense_strides(src) if fmt is torch.preserve_format else None
            return finish(_guarded(real_empty, src.shape, dtype, device, zero, strides, _site(), name),
                          kwargs.get("requires_grad"))
        fn.__name__ = name
        return fn

    def new(name, zero):
        def fn(self, *args, **kwargs):
            kw = dict(kwargs)
            device = torch.device(kw["device"]) if kw.get("device") is not None else self.device
            shape = _shape_of(args, kw)
            if not simple(kw) or not _wants(device, devices):
                return real[name](self, *args, **kwargs)
            dtype = kw.get("dtype") or self.dtype
            return finish(_guarded(real_empty, shape, dtype, device, zero, None, _site(), name), kw.get("requires_grad"))
        fn.__name__ = name
        return fn

    patches = [(torch, "empty", factory("empty", False)), (torch, "zeros", factory("zeros", True)),
               (torch, "empty_like", like("empty_like", False)), (torch, "zeros_like", like("zeros_like", True)),
               (torch.Tensor, "new_empty", new("new_empty", False)), (torch.Tensor, "new_zeros", new("new_zeros", True))]
    log._real_empty = real_empty
    _ACTIVE.append(log)
    try:
        for owner, name, fn in patches:
            monkeypatch.setattr(owner, name, fn)
        yield log
    finally:
        _ACTIVE.pop()
        for owner, name, _ in patches:
            setattr(owner, name, real[name])


def embed(t, log=None):
    """Inside a `poisoned` block (or with its `log`, also after the block): `t` copied into the interior of a NaN-guarded buffer of its own (same layout rule as the allocations): the
    interior view has t's shape, dtype, device, requires_grad and — for a dense tensor — strides, and starts a multiple
    of 512 bytes into its buffer.  Python attributes of `t` (`_sr_frozen`) are carried over, except cached scratch."""
    if log is None:
        assert _ACTIVE, "embed() outside a poisoned block needs that block's log"
        log = _ACTIVE[-1]
    real_empty = log._real_empty
    src = t.detach()
    entry = _guarded(real_empty, src.shape, src.dtype, src.device, False, _dense_strides(src), _site(), "input")
    entry.view.copy_(src)
    entry.before = _bits(entry.flat[entry.guard:entry.guard + entry.numel].reshape(-1)).clone()
    for key, value in getattr(t, "__dict__", {}).items():
        if key != "_sr_scratch":
            setattr(entry.view, key, value)
    log._add(entry, is_input=True)
    return entry.view.requires_grad_() if t.requires_grad else entry.view


def _damage(entry):
    """[(side, offset of the first damaged element)] of one entry's guards."""
    flat, g, n = entry.flat, entry.guard, entry.numel
    found = []
    for side, part in (("front", flat[:g]), ("back", flat[g + n:])):
        if flat.dtype.is_floating_point:
            want = _bits(torch.full((1,), float("nan"), dtype=flat.dtype, device=flat.device))[0]
            bad = _bits(part) != want
            scale = 1
        else:
            bad = part.view(torch.uint8) != INT_FILL
            scale = flat.element_size()
        if bool(bad.any()):
            first = int(bad.nonzero()[0]) // scale
            # front: elements before the interior's start (1 = the element just before it); back: past its end (0 =
            # the element just past it)
            found.append((side, g - first if side == "front" else first))
    return found


def _same(a, b):
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype)


def check(log, outputs, inputs, inplace=(), nonfinite_ok=()):
    """After the call(s) inside `poisoned`: synchronises, then asserts that
      1. every guard of every logged allocation and every embedded input holds its fill, bit for bit,
      2. every floating-point tensor of `outputs` is finite throughout — except those in `nonfinite_ok` (outputs that
         legitimately hold non-finite values, or a waived partly-written allocation): the caller compares them with the
         plain run bit for bit instead,
      3. every embedded input of `inputs` that is not in `inplace` still holds the bits it held before the call.
    Every failure is collected; the assertion names each one."""
    for e in log.entries + log.inputs:
        if e.flat.is_cuda:
            torch.cuda.synchronize(e.flat.device)
            break
    problems = []
    # 1. guards — one reduction per entry first (cheap), the position only where something is wrong
    for e in log.entries + log.inputs:
        for side, off in _damage(e):
            where = ("%d element(s) before its start" % off) if side == "front" else ("%d element(s) past its end" % off)
            problems.append("stray store: %s guard of the %s %s allocated at %s damaged, first at %s"
                            % (side, e.kind, tuple(e.view.shape), e.site, where))
    # 2. outputs fully written, nothing unwritten read
    for i, o in enumerate(outputs):
        if o is None or not o.dtype.is_floating_point or any(_same(o, w) for w in nonfinite_ok if w is not None):
            continue
        bad = ~torch.isfinite(o.detach())
        if bool(bad.any()):
            first = [int(v) for v in bad.nonzero()[0]]
            site = next((e.site for e in log.entries if e.view.data_ptr() == o.data_ptr()), "an ATen allocation")
            problems.append("unwritten or poisoned value: output %d %s (allocated at %s) has %d non-finite element(s), "
                            "first at index %s" % (i, tuple(o.shape), site, int(bad.sum()), tuple(first)))
    # 3. inputs untouched
    skip = [t for t in inplace if t is not None]
    for e in log.inputs:
        if not any(_same(e.view, t) for t in inputs if t is not None) or any(_same(e.view, t) for t in skip):
            continue
        now = _bits(e.flat[e.guard:e.guard + e.numel].reshape(-1))
        diff = now != e.before
        if bool(diff.any()):
            problems.append("input modified: the input %s embedded at %s changed, first at flat offset %d"
                            % (tuple(e.view.shape), e.site, int(diff.nonzero()[0])))
    assert not problems, "\n".join(problems)
