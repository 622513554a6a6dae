"""The poison / guard-band harness (tests/poison.py) on CPU tensors, with pure-torch stand-in "operators": it must flag an output that was
not fully written and a write one element before / past a buffer, pass a correct function, hand out faithful tensors, count what it
guards and what it does not, and put torch.empty / torch.empty_like / Tensor.new_empty back whatever happens inside the block."""
import pytest
import torch

from poison import FILLS, GuardViolation, differing, poisoned, run_under_fills, same_bits

REAL = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


def _restored():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty) == REAL and "new_empty" not in torch.Tensor.__dict__


X = torch.arange(37, dtype=torch.float32) * 0.25 - 3.0
STRAY = torch.tensor([0x12345678], dtype=torch.int32).view(torch.float32)[0]      # no byte of it equals a fill


def op_correct(x=X):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    return out


def op_forgets_tail(x=X):
    """writes all but the last element of its output (a kernel whose last block returns early)"""
    out = torch.empty((x.numel(),), dtype=torch.float32)
    out[:-1] = x[:-1] * 2
    return out


def op_forgets_counter(x=X):
    """accumulates into a counter it never armed"""
    n = torch.empty((1,), dtype=torch.int32)
    n += int((x > 0).sum())
    return n


def op_clamped_sum(x=X):
    """an unwritten partial summed and clamped: a huge finite poison is clamped away (as is the baseline), only a NaN survives"""
    part = torch.empty((4,), dtype=torch.float32)
    part[:3] = x[-3:]                              # 5.5 + 5.75 + 6.0: above the clamp already
    return part.sum().clamp(-1.0, 1.0).reshape(1)


def op_min_reduce(x=X):
    """an unwritten slot in an fminf-style reduction: NaN is dropped silently, a huge finite value loses too, only 0x00 shows"""
    d = torch.empty((x.numel() + 1,), dtype=torch.float32)
    d[:-1] = x.abs() + 1.0
    best = torch.tensor(float("inf"))
    for v in d:                                    # fminf semantics: a NaN operand is ignored
        best = v if (v < best) else best
    return best.reshape(1)


def _parent_of(p, k=-1):
    return p.records[k].parent


def op_writes_one_past(p, x=X):
    out = torch.empty((x.numel(),), dtype=torch.float32)
    out.copy_(x)
    flat = _parent_of(p)[p.guard:].view(torch.float32)          # the tensor's elements followed by the guard band behind it
    flat[x.numel()] = STRAY                                      # index one past the end, through the flat parent
    return out


def op_writes_one_before(p, x=X):
    out = torch.empty((x.numel(),), dtype=torch.float32)
    out.copy_(x)
    before = torch.as_strided(_parent_of(p).view(torch.float32), (1,), (1,), p.guard // 4 - 1)     # element -1
    before[0] = STRAY
    return out


def test_correct_function_passes():
    runs = run_under_fills(op_correct)
    assert differing(runs) == []
    assert all(p.handed_out == 1 and p.unguarded == 0 and p.check() == [] for p, _ in runs)
    assert torch.equal(runs[0][1], X * 2)
    assert _restored()


@pytest.mark.parametrize("op,seen_by", [(op_forgets_tail, ["0xFF", "0x5A"]), (op_forgets_counter, ["0xFF", "0x5A"]),
                                        (op_clamped_sum, ["0xFF"]), (op_min_reduce, ["0xFF", "0x5A"])])
def test_unwritten_output_differs_between_fills(op, seen_by):
    """each poison is needed: the clamped sum hides the finite one (0x00 and 0x5A agree), the min reduction's baseline (0.0 wins) differs
    from both poisons"""
    runs = run_under_fills(op)
    assert differing(runs) == seen_by
    assert all(p.check() == [] for p, _ in runs)                 # nothing out of bounds here: the guards stay intact


def test_poison_values():
    got = {}
    for fill in FILLS:
        with poisoned(fill):
            got[fill] = (torch.empty((3,), dtype=torch.float32), torch.empty((3,), dtype=torch.int32), torch.empty((5,), dtype=torch.uint8))
    assert (got[0x00][0] == 0).all() and (got[0x00][1] == 0).all()
    assert torch.isnan(got[0xFF][0]).all() and (got[0xFF][1] == -1).all() and (got[0xFF][2] == 255).all()
    assert (got[0x5A][1] == 1515870810).all() and (got[0x5A][1] == 0x5A5A5A5A).all()
    assert ((got[0x5A][0] > 1.5e16) & (got[0x5A][0] < 1.6e16)).all()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("op,side,offset", [(op_writes_one_past, "after", "+0"), (op_writes_one_before, "before", "-4")])
def test_out_of_bounds_write_is_reported(fill, op, side, offset):
    with pytest.raises(GuardViolation) as e:
        with poisoned(fill) as p:
            op(p)
    msg = str(e.value)
    assert "fill 0x%02X" % fill in msg and "guard %s the tensor damaged" % side in msg and "offset %s " % offset in msg, msg
    assert "(37,) torch.float32" in msg and "test_poison_host.py" in msg and op.__name__ in msg, msg      # shape, dtype, call site
    assert len(p.check()) == 1
    assert _restored()


def test_write_that_equals_the_fill_needs_another_fill():
    """a stray store of the fill's own value is invisible under that fill: the three fills have no float32 / int32 value in common"""
    def op(p):
        out = torch.empty((4,), dtype=torch.int32)
        out.zero_()
        _parent_of(p)[p.guard:].view(torch.int32)[4] = 0
        return out
    with poisoned(0x00) as p:
        op(p)
    assert p.check() == []
    for fill in (0xFF, 0x5A):
        with pytest.raises(GuardViolation):
            with poisoned(fill) as p:
                op(p)


@pytest.mark.parametrize("guard", [512, 4096])
def test_tensors_are_faithful(guard):
    src = torch.zeros((3, 5), dtype=torch.float64)
    with poisoned(0x5A, guard) as p:
        made = [torch.empty((2, 3, 4), dtype=torch.float32), torch.empty(7, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int64),
                torch.empty(torch.Size((5, 1)), dtype=torch.uint8), torch.empty((), dtype=torch.float32), torch.empty([4, 4]),
                torch.empty_like(src), torch.empty_like(src, dtype=torch.float16), src.new_empty((6,)), src.new_empty(2, 2, dtype=torch.int16),
                torch.empty((3,), dtype=torch.float32, requires_grad=True), torch.empty((9,), dtype=torch.bool, device="cpu")]
    want = [((2, 3, 4), torch.float32), ((7,), torch.int32), ((2, 3), torch.int64), ((5, 1), torch.uint8), ((), torch.float32), ((4, 4), torch.float32),
            ((3, 5), torch.float64), ((3, 5), torch.float16), ((6,), torch.float64), ((2, 2), torch.int16), ((3,), torch.float32), ((9,), torch.bool)]
    assert p.handed_out == len(made) == len(p.records) and p.unguarded == 0
    for t, (shape, dtype), r in zip(made, want, p.records):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
        assert t._base is None and t.data_ptr() == r.parent.data_ptr() + guard
        assert r.parent.data_ptr() % 64 == 0 and t.data_ptr() % 512 == r.parent.data_ptr() % 512     # the allocator's alignment is kept
        assert r.parent.numel() == t.numel() * t.element_size() + 2 * guard
        ref = torch.empty(shape, dtype=dtype)
        assert t.stride() == ref.stride()
    assert made[10].requires_grad and not made[0].requires_grad
    # writing every element of every tensor leaves every guard alone
    for t in made:
        t.detach().reshape(-1).view(torch.uint8).fill_(1)
    assert p.check() == []


def test_guard_must_keep_the_alignment():
    for g in (0, 100, 4096 + 256, -512):
        with pytest.raises(ValueError):
            poisoned(0, g)
    with pytest.raises(ValueError):
        poisoned(256)


def test_unguarded_requests_are_counted_and_served():
    src = torch.zeros((4, 6))
    with poisoned(0xFF) as p:
        a = torch.empty((0, 3))                                              # zero elements
        b = torch.empty((2, 0), dtype=torch.int32)
        c = torch.empty((2, 3), out=torch.zeros(6))                          # out=
        d = torch.empty((1, 2, 4, 4), memory_format=torch.channels_last)     # memory_format=
        e = torch.empty_like(src, memory_format=torch.contiguous_format)
        f = torch.empty((3, 3), layout=torch.sparse_coo)                     # non-strided layout
        g = torch.empty_like(src.t())                                        # strides to preserve
        h = torch.empty_like(torch.zeros((0,)))
        i = src.new_empty((0,))
        assert p.handed_out == 0 and p.unguarded == 9
        k = torch.empty((2, 3))
        l = torch.empty((2,), layout=torch.strided, pin_memory=False)
    assert p.handed_out == 2 and p.unguarded == 9 and len(p.records) == 2
    assert a.shape == (0, 3) and b.dtype == torch.int32 and c.shape == (2, 3) and d.is_contiguous(memory_format=torch.channels_last)
    assert e.shape == (4, 6) and f.layout == torch.sparse_coo and g.stride() == src.t().stride() and h.numel() == 0 and i.numel() == 0
    assert torch.isnan(k).all() and torch.isnan(l).all()


def test_pinned_request_is_unguarded():
    with poisoned(0xFF) as p:
        try:
            t = torch.empty((4,), pin_memory=True)
        except RuntimeError:                       # a build without an accelerator refuses page-locked memory: the request still went through
            t = None
    assert p.handed_out == 0 and p.unguarded == 1
    assert t is None or (t.is_pinned() and t.untyped_storage().nbytes() == 16)
    assert _restored()


def test_functions_are_restored_after_an_exception():
    with pytest.raises(ZeroDivisionError):
        with poisoned(0xFF):
            assert torch.empty is not REAL[0] and torch.empty_like is not REAL[1] and torch.Tensor.new_empty is not REAL[2]
            torch.empty((3,))
            1 / 0
    assert _restored()
    t = torch.empty((3,))
    assert t._base is None and t.untyped_storage().nbytes() == 12            # the real function again: no guard bands around it
    # ... an exception inside the block is not replaced by a guard report
    with pytest.raises(KeyError):
        with poisoned(0xFF) as p:
            op_writes_one_past(p)
            raise KeyError("the block's own failure")
    assert _restored() and len(p.check()) == 1
    # ... and blocks do not nest (the inner one would restore the outer one's wrappers as "real")
    with poisoned(0x00):
        with pytest.raises(RuntimeError):
            with poisoned(0xFF):
                pass
        assert torch.empty is not REAL[0]
    assert _restored()


def test_same_bits_sees_what_equal_does_not():
    nan = torch.full((2,), float("nan"))
    assert same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not same_bits(torch.zeros(2), -torch.zeros(2))
    assert not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.int32)) and not same_bits(torch.zeros(2), None)
    assert same_bits((1, [torch.ones(2), None], {"a": torch.ones(1)}), (1, [torch.ones(2), None], {"a": torch.ones(1)}))
    assert not same_bits((torch.ones(2),), (torch.ones(2), torch.ones(2)))
