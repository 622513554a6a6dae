"""Poisoned, guard-banded allocations for the operator tests.

Every operator wrapper of the package hands its kernels `torch.empty` memory and relies on each kernel writing all that is later
read or returned.  What the allocator hands out is, in a test process, either a driver-zeroed block or the recycled right answer of
the previous, identically shaped case, so a forgotten row, tail block or counter goes unseen.  Inside

    with poisoned(0xFF) as p:
        out = operator(...)
    # leaving the block: torch.cuda.synchronize() if a device was used, then every guard byte is compared with the fill

`torch.empty`, `torch.empty_like` and `Tensor.new_empty` allocate the request with `guard` bytes on either side in ONE uint8 block,
fill the whole block with the byte `fill` and return a contiguous tensor over the middle.  Running an operator under several fills and
comparing what it returns bit for bit shows every element it returned without having written it; the guard bands show every write
just before or past a buffer (the write lands inside the block: nothing faults).

Fills: 0x00 the baseline; 0xFF float NaN / int -1 / counter UINT_MAX; 0x5A float32 0x5A5A5A5A ~ 1.54e16 / int32 1515870810.  Two
poisons, because fminf / fmaxf and every > / < test drop a NaN silently while a huge finite value survives them, and a NaN in turn
survives a sum that is clamped afterwards.

Requests the wrapper cannot reproduce faithfully go to the real function and are counted in `unguarded`: zero elements, `out=`,
`memory_format=`, a non-strided `layout=`, `pin_memory=True`, named tensors, and `empty_like` of a tensor that is not contiguous (the real
function would preserve its strides).
"""
import traceback

import torch

FILLS = (0x00, 0xFF, 0x5A)          # in this order: the baseline first

_REAL = {"empty": torch.empty, "empty_like": torch.empty_like, "new_empty": torch.Tensor.new_empty}
_HERE = __file__[:-1] if __file__.endswith(".pyc") else __file__
_active = []


class GuardViolation(AssertionError):
    pass


class _Record:
    __slots__ = ("parent", "nbytes", "shape", "dtype", "site")

    def __init__(self, parent, nbytes, shape, dtype, site):
        self.parent, self.nbytes, self.shape, self.dtype, self.site = parent, nbytes, shape, dtype, site

    def describe(self):
        return "%s %s on %s allocated at %s" % (tuple(self.shape), self.dtype, self.parent.device, self.site)


def _call_site():
    """the innermost frames outside this module, innermost last: 'file:line in function < ...'"""
    frames = [f for f in traceback.extract_stack(limit=12) if f.filename != _HERE]
    return " < ".join("%s:%d in %s" % (f.filename.rsplit("/", 1)[-1], f.lineno, f.name) for f in reversed(frames[-3:]))


def _size_of(args):
    """the size of torch.empty(2, 3) / torch.empty((2, 3)) / torch.empty(torch.Size(...)) as a tuple of ints, or None if it is no such thing"""
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    try:
        size = tuple(int(s) for s in args)
    except (TypeError, ValueError):
        return None
    return size if all(s >= 0 for s in size) else None


class poisoned:
    """Context manager, see the module's docstring.  After (and inside) the block:
    handed_out   guarded allocations made
    unguarded    requests passed to the real function
    records      one _Record per guarded allocation (parent block, byte count, shape, dtype, call site)
    check()      compare every guard byte with the fill; returns the list of violations (strings)"""

    def __init__(self, fill, guard=4096):
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill is one byte")
        if guard <= 0 or guard % 512:
            raise ValueError("guard must be a positive multiple of 512 bytes: data_ptr() keeps the allocator's alignment")
        self.fill, self.guard = int(fill), int(guard)
        self.handed_out = self.unguarded = 0
        self.records = []
        self._device_used = False

    # ---- the three wrappers -------------------------------------------------------------------------------------------------------------
    def _guarded(self, size, dtype, device, requires_grad):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        device = torch.get_default_device() if device is None else torch.device(device)
        item = _REAL["empty"]((), dtype=dtype).element_size()
        numel = 1
        for s in size:
            numel *= s
        nbytes = numel * item
        parent = _REAL["empty"]((nbytes + 2 * self.guard,), dtype=torch.uint8, device=device)
        parent.fill_(self.fill)
        strides, acc = [], 1
        for s in reversed(size):
            strides.append(acc)
            acc *= max(s, 1)
        # a tensor of its own over the middle of the block's storage (no view relation: autograd and in-place checks see a plain tensor)
        t = _REAL["empty"]((0,), dtype=dtype, device=parent.device).set_(parent.untyped_storage(), self.guard // item, size, tuple(reversed(strides)))
        if requires_grad:
            t.requires_grad_(True)
        self.records.append(_Record(parent, nbytes, size, dtype, _call_site()))
        self.handed_out += 1
        if parent.device.type != "cpu":
            self._device_used = True
        return t

    def _passthrough(self, name, args, kwargs):
        self.unguarded += 1
        return _REAL[name](*args, **kwargs)

    @staticmethod
    def _plain(kwargs, allowed):
        """no keyword beyond `allowed`, strided layout, not pinned"""
        if any(k not in allowed for k in kwargs):
            return False
        if kwargs.get("layout", torch.strided) not in (None, torch.strided) or kwargs.get("pin_memory"):
            return False
        return True

    def _empty(self, *args, **kwargs):
        size = _size_of(args)
        if size is None or 0 in size or not self._plain(kwargs, ("dtype", "layout", "device", "requires_grad", "pin_memory")):
            return self._passthrough("empty", args, kwargs)
        return self._guarded(size, kwargs.get("dtype"), kwargs.get("device"), bool(kwargs.get("requires_grad")))

    def _empty_like(self, *args, **kwargs):
        if (len(args) != 1 or not isinstance(args[0], torch.Tensor) or args[0].numel() == 0 or not args[0].is_contiguous()
                or args[0].layout is not torch.strided or not self._plain(kwargs, ("dtype", "layout", "device", "requires_grad", "pin_memory"))):
            return self._passthrough("empty_like", args, kwargs)
        src = args[0]
        return self._guarded(tuple(src.shape), kwargs.get("dtype") or src.dtype, kwargs.get("device") or src.device, bool(kwargs.get("requires_grad")))

    def _new_empty(self, src, *args, **kwargs):
        size = _size_of(args)
        if size is None or 0 in size or src.layout is not torch.strided or not self._plain(kwargs, ("dtype", "layout", "device", "requires_grad", "pin_memory")):
            return self._passthrough("new_empty", (src,) + args, kwargs)
        return self._guarded(size, kwargs.get("dtype") or src.dtype, kwargs.get("device") or src.device, bool(kwargs.get("requires_grad")))

    # ---- the block ----------------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        if _active:
            raise RuntimeError("poisoned() blocks do not nest")
        _active.append(self)
        self._had_new_empty = "new_empty" in torch.Tensor.__dict__
        me = self
        torch.empty = lambda *a, **k: me._empty(*a, **k)
        torch.empty_like = lambda *a, **k: me._empty_like(*a, **k)
        torch.Tensor.new_empty = lambda src, *a, **k: me._new_empty(src, *a, **k)
        return self

    def _restore(self):
        torch.empty, torch.empty_like = _REAL["empty"], _REAL["empty_like"]
        if self._had_new_empty:
            torch.Tensor.new_empty = _REAL["new_empty"]
        elif "new_empty" in torch.Tensor.__dict__:
            del torch.Tensor.new_empty                    # (inherited from the C base class: the attribute set above only shadowed it)
        _active.remove(self)

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None and self._device_used:
                torch.cuda.synchronize()
        finally:
            self._restore()
        if exc_type is None:
            bad = self.check()
            if bad:
                raise GuardViolation("fill 0x%02X: %d guard band(s) overwritten\n  %s" % (self.fill, len(bad), "\n  ".join(bad)))
        return False

    def check(self):
        """every guard byte against the fill; one line per damaged band: the allocation, the side, the first offset and the byte count"""
        if self._device_used:
            torch.cuda.synchronize()
        out = []
        for r in self.records:
            for side, band in (("before", r.parent[:self.guard]), ("after", r.parent[self.guard + r.nbytes:])):
                wrong = band != self.fill
                if bool(wrong.any()):
                    idx = wrong.nonzero().reshape(-1)
                    first = int(idx[0])
                    # "before": bytes counted back from the tensor's first byte; "after": bytes past its last byte
                    off = first - self.guard if side == "before" else first
                    out.append("%s: guard %s the tensor damaged, %d byte(s), first at byte offset %+d from its %s (found 0x%02X)"
                               % (r.describe(), side, int(idx.numel()), off, "start" if side == "before" else "end", int(band[first])))
        return out


def same_bits(a, b):
    """two results (tensors, None, numbers, or nested tuples / lists / dicts of them) agree bit for bit (NaN payloads included)"""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if a.numel() == 0:
            return True
        return bool(torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8), b.detach().contiguous().reshape(-1).view(torch.uint8)))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return a == b


def run_under_fills(route, fills=FILLS, guard=4096):
    """route() once per fill, in order; returns [(poisoned block, result)].  A damaged guard band raises GuardViolation from the run that did it."""
    runs = []
    for fill in fills:
        with poisoned(fill, guard) as p:
            result = route()
        runs.append((p, result))
    return runs


def differing(runs):
    """names of the fills whose result differs from the first run's, e.g. ['0xFF']: empty when the route returned only what it wrote"""
    base = runs[0][1]
    return ["0x%02X" % p.fill for p, result in runs[1:] if not same_bits(base, result)]
