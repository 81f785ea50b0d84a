"""Footprint harness: guard bands and poison around every buffer a kernel touches.  A plain module (not collected), shared by
tests/test_footprint_cpu.py (CPU: proves that the harness flags a wrong kernel) and tests/test_hip_footprint.py (GPU: every
kernel family inside it).

A guarded tensor is a contiguous view into a larger uint8 buffer filled entirely with the byte 0xFF: GUARD bytes in front
(so the payload keeps a 256-byte alignment), the payload at its exact size (not rounded up: a one-element overrun hits the
guard), GUARD bytes right behind it.  The one pattern is poison and canary for every dtype the project uses: fp32, fp64,
bf16 and fp16 read it as NaN, int32 and int64 as -1, uint8 as 255.  So
  * a write outside an output or a workspace changes a guard byte                      -> Guard.verify() names the allocation;
  * an element never written, or read before it is written, is or yields NaN           -> assert_no_poison / the comparison;
  * a read past an input that reaches the result reads NaN or -1                       -> the comparison with the reference.

Guard replaces torch.empty / torch.empty_like (with zeros=True also torch.zeros / torch.zeros_like) for its duration, so
the wrappers of slu_hip/ops.py, which size outputs and workspaces with torch.empty at exactly what the library reports,
allocate guarded tensors without being touched.  It is not used around hipGraph capture."""
import sys

import torch

GUARD = 256
POISON = 0xFF
DTYPES = (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8)

_REAL = {name: getattr(torch, name) for name in ("empty", "empty_like", "zeros", "zeros_like")}
_HERE = __file__[:-1] if __file__.endswith(".pyc") else __file__


class FootprintError(AssertionError):
    pass


def _site():
    """file:line of the nearest caller outside this module"""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == _HERE:
        f = f.f_back
    return "?" if f is None else "%s:%d" % (f.f_code.co_filename, f.f_lineno)


def _itemsize(dtype):
    return _REAL["empty"]((), dtype=dtype).element_size()


class Allocation:
    """One guarded buffer: [GUARD bytes | payload, nbytes | GUARD bytes], all 0xFF when handed out."""

    def __init__(self, shape, dtype, device, site):
        self.shape, self.dtype, self.site = tuple(shape), dtype, site
        numel = 1
        for s in self.shape:
            numel *= s
        self.nbytes = numel * _itemsize(dtype)
        self.buf = _REAL["empty"](GUARD + self.nbytes + GUARD, dtype=torch.uint8, device=device)
        self.buf.fill_(POISON)                                                                 # the poison fill
        self.tensor = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(self.shape)

    def payload_bytes(self):
        return self.buf[GUARD:GUARD + self.nbytes]

    def damage(self):
        """None, or the offset (in bytes, relative to the payload's first byte; negative = in front) of the first
        guard byte that no longer holds the pattern."""
        front = self.buf[:GUARD]
        back = self.buf[GUARD + self.nbytes:]                                                  # the back guard
        bad = torch.cat([front, back]).ne(POISON).nonzero().flatten().cpu()
        if bad.numel() == 0:
            return None
        i = int(bad[0])
        return i - GUARD if i < GUARD else self.nbytes + (i - GUARD)

    def describe(self):
        return "%s %s allocated at %s" % (self.shape, str(self.dtype).replace("torch.", ""), self.site)


def _alloc(shape, dtype, device, site=None):
    a = Allocation(shape, dtype, device, site or _site())
    a.tensor._footprint = a            # a cycle (tensor -> allocation -> tensor): the buffer lives until the collector runs
    if _ACTIVE:
        _ACTIVE[-1].allocations.append(a)
    return a


def guarded_empty(shape, dtype=torch.float32, device="cpu"):
    """A contiguous tensor of `shape`, every byte 0xFF, between two guards.  Inside a Guard it is kept alive and verified
    with the Guard's own allocations; outside one, check it with damage_of()."""
    if isinstance(shape, int):
        shape = (shape,)
    return _alloc(shape, dtype, device).tensor


def guarded_strided(shape, strides, dtype=torch.float32, device="cpu"):
    """A guarded tensor with the given (positive) strides: the payload spans exactly first to last element, the gaps
    between rows are poison that must survive (gaps_intact)."""
    extent = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if all(shape) else 0
    flat = _alloc((extent,), dtype, device).tensor
    t = flat.as_strided(tuple(shape), tuple(strides))
    t._footprint = flat._footprint
    return t


def guarded_copy(t):
    """`t` inside a guarded buffer, strides preserved: a read one element past it sees NaN or -1."""
    if t.is_contiguous():
        out = _alloc(t.shape, t.dtype, t.device).tensor
    else:
        out = guarded_strided(t.shape, t.stride(), t.dtype, t.device)
    with torch.no_grad():
        out.copy_(t)
    return out


def damage_of(t):
    return t._footprint.damage()


def gaps_intact(t):
    """True when every payload byte that the strided view `t` does not cover still holds the pattern."""
    a = t._footprint
    size = _itemsize(a.dtype)
    covered = _REAL["zeros"](a.nbytes // size, dtype=torch.bool, device=a.buf.device)
    covered.as_strided(tuple(t.shape), tuple(t.stride())).fill_(True)
    rows = a.payload_bytes().view(-1, size)
    return bool(rows[~covered].eq(POISON).all())


def poisoned(t):
    """How many elements of `t` still hold the pattern in every byte (an element never written)."""
    size = t.element_size()
    raw = t.detach().contiguous().view(torch.uint8).view(-1, size)
    return int(raw.eq(POISON).all(dim=1).sum())


def assert_no_poison(t, what):
    """A fully written float output holds no NaN: neither the pattern itself nor anything computed from it."""
    assert t.is_floating_point(), what
    n = int(torch.isnan(t.detach()).sum())
    if n:
        first = int(torch.isnan(t.detach()).flatten().nonzero()[0])
        raise FootprintError("%s: %d of %d elements are NaN (never written, or computed from poison); first at flat index %d"
                             % (what, n, t.numel(), first))


_ACTIVE = []


class Guard:
    """with Guard(device) as g: ...; g.verify()

    For its duration torch.empty and torch.empty_like (zeros=True: also torch.zeros and torch.zeros_like, the payload zeroed
    after the poison fill, the guards kept) return guarded tensors for `device`.  Calls with pin_memory, out=, a layout or
    memory format, or another device go to the real function.  Every buffer handed out stays alive until the Guard is
    dropped, so the allocator recycles nothing."""

    def __init__(self, device="cpu", zeros=False):
        self.device = torch.device(device)
        self.zeros = zeros
        self.allocations = []

    def _mine(self, device):
        d = torch.device("cpu") if device is None else torch.device(device)
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def _make(self, name, args, kwargs, like):
        kw = dict(kwargs)
        requires_grad = kw.pop("requires_grad", False)
        if like:
            (src,) = args
            shape, dtype, device = src.shape, kw.pop("dtype", None) or src.dtype, kw.pop("device", None) or src.device
        else:
            shape = kw.pop("size") if "size" in kw else args[0] if len(args) == 1 and not isinstance(args[0], int) else args
            dtype, device = kw.pop("dtype", None) or torch.get_default_dtype(), kw.pop("device", None)
        fmt = kw.pop("memory_format", torch.contiguous_format)
        dense = fmt == torch.contiguous_format or (like and fmt == torch.preserve_format and args[0].is_contiguous())
        if kw or not dense or not self._mine(device):         # pin_memory, out=, layout, ...: not the project's device forms
            return _REAL[name](*args, **kwargs)
        a = _alloc(tuple(int(s) for s in shape), dtype, self.device if device is None else device)
        if name.startswith("zeros"):
            a.payload_bytes().zero_()
        return a.tensor.requires_grad_() if requires_grad else a.tensor

    def __enter__(self):
        assert not _ACTIVE, "Guards do not nest: leaving the inner one would restore the real functions under the outer one"
        names = ("empty", "empty_like") + (("zeros", "zeros_like") if self.zeros else ())
        for name in names:
            def replacement(*args, _name=name, **kwargs):
                return self._make(_name, args, kwargs, _name.endswith("_like"))
            setattr(torch, name, replacement)                                                  # the torch.empty replacement
        _ACTIVE.append(self)
        return self

    def __exit__(self, *exc):
        _ACTIVE.remove(self)
        for name, fn in _REAL.items():
            setattr(torch, name, fn)
        return False

    def verify(self):
        """Raises FootprintError naming every allocation with a changed guard byte."""
        found = []
        for a in self.allocations:
            at = a.damage()
            if at is not None:
                where = "%d bytes in front of it" % -at if at < 0 else "%d bytes past its end" % (at - a.nbytes)
                found.append("guard changed at payload byte offset %d (%s; payload %d bytes): %s"
                             % (at, where, a.nbytes, a.describe()))
        if found:
            raise FootprintError("\n".join(found))


class Calls:
    """A recording proxy around the object slu_hip.lib.load() returns: lists the entry points a case really reached."""

    def __init__(self, real):
        self._real = real
        self.reached = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("slu_"):
            return fn

        def call(*args):
            self.reached.append(name)
            return fn(*args)
        return call

    @classmethod
    def install(cls, monkeypatch):
        """Replace slu_hip.lib.load by one that returns the proxy (the wrappers call lib.load() per launch)."""
        from slu_hip import lib
        calls = cls(lib.load())
        monkeypatch.setattr(lib, "load", lambda: calls)
        return calls

    def missing(self, claimed):
        return sorted(set(claimed) - set(self.reached))
