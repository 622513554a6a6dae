"""GPU: gm_plain_activate_fwd / _bwd per element against the float64 definition of plain_activate_ref.py (whose gate
test_plain_activate_ref_host.py shows to reject five wrong kernels), through model_ops.plain_activate with and without joint buffers and
through the C entry points with row0 != 0; bit-level properties; the rows kept out of the gate; N = 0.
Run with -s for the worst ratio over the bar per tensor."""
import numpy as np
import pytest
import torch

import plain_activate_ref as P
import poison

pytestmark = pytest.mark.gpu

G = 64                                            # guard rows on either side of every buffer handed to the C entry points
SENTINEL = 0x5A5A5A5A                             # float32 1.5e16
WIDTH = {"xyz": 3, "scales": 3, "rots": 4, "opac": 1, "d_xyz": 3, "d_scaling": 3, "d_rotation": 4, "d_opacity": 1}
UP_WIDTH = (3, 3, 4, 1)


def _dev(a):
    return torch.as_tensor(np.array(a, np.float32)).cuda()


def _banded(rows, width):
    """[G + rows + G, width] float32 filled with the sentinel"""
    return torch.full((rows + 2 * G, width), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _untouched(buf, lo, hi):
    """every row of a banded buffer outside [G + lo, G + hi) still holds the sentinel"""
    b = _bits(buf)
    return bool((b[:G + lo] == SENTINEL).all() and (b[G + hi:] == SENTINEL).all())


def c_forward(ins, row0=0, cap=None):
    """gm_plain_activate_fwd into sentinel-filled, guard-banded buffers of `cap` rows; returns {tensor: [N, w] device tensor}"""
    from gaussianmesh_amd._op import enqueue
    n = ins[0].shape[0]
    cap = n if cap is None else cap
    bufs = [_banded(cap, WIDTH[t]) for t in P.FWD]
    enqueue(ins[0].device, "gm_plain_activate_fwd", n, *ins, *[b[G:] for b in bufs], row0, cap)
    torch.cuda.synchronize()
    for t, b in zip(P.FWD, bufs):
        assert _untouched(b, row0, row0 + n), (t, row0, cap)
    return {t: b[G + row0:G + row0 + n].clone() for t, b in zip(P.FWD, bufs)}


def c_backward(ins, ups, row0=0, cap=None):
    """gm_plain_activate_bwd: `ups` (each [N, w] or None) placed at rows [row0, row0 + N) of sentinel-filled buffers of `cap` rows"""
    from gaussianmesh_amd._op import enqueue
    n = ins[0].shape[0]
    cap = n if cap is None else cap
    gb = []
    for u, w in zip(ups, UP_WIDTH):
        if u is None:
            gb.append(None)
            continue
        b = _banded(cap, w)
        b[G + row0:G + row0 + n] = u
        gb.append(b)
    keep = [None if b is None else _bits(b).copy() for b in gb]
    outs = [_banded(n, WIDTH[t]) for t in P.BWD]
    enqueue(ins[0].device, "gm_plain_activate_bwd", n, ins[1], ins[2], ins[3], *[None if b is None else b[G:] for b in gb], row0, cap,
            *[b[G:] for b in outs])
    torch.cuda.synchronize()
    for t, b in zip(P.BWD, outs):
        assert _untouched(b, 0, n), (t, row0, cap)
    for b, k in zip(gb, keep):
        assert b is None or np.array_equal(_bits(b), k)                        # inputs are inputs
    return {t: b[G:G + n].clone() for t, b in zip(P.BWD, outs)}


def _python_route(ins, ups, joint_extra=None):
    """model_ops.plain_activate forward and backward; joint_extra: joint buffers with that many tail rows holding 7.0"""
    from gaussianmesh_amd.model_ops import plain_activate
    n = ins[0].shape[0]
    leaves = [t.clone().requires_grad_(True) for t in ins]
    jb = None
    if joint_extra is not None:
        jb = {k: torch.full((n + joint_extra, w), 7.0, dtype=torch.float32, device="cuda") for k, w in zip(("xyz", "scales", "rots", "opac"), UP_WIDTH)}
    outs = plain_activate(*leaves, joint=jb)
    got = {t: (o[:n] if jb is not None else o).detach().clone() for t, o in zip(P.FWD, outs)}
    up = ups
    if jb is not None:                            # the upstream rows of the tail are arbitrary: the kernel never reads them
        up = [torch.cat([u, torch.full((joint_extra, u.shape[1]), 1e30, device="cuda")]) for u in ups]
        assert all(torch.equal(o[n:], torch.full_like(o[n:], 7.0)) for o in outs)
    torch.autograd.backward(outs, up)
    for t, lf in zip(P.BWD, leaves):
        got[t] = lf.grad.reshape(n, -1).clone()
    return got


def _gate(got, n, label):
    ref, s_abs = P.case_reference(n)
    host = {t: v.cpu().numpy() for t, v in got.items()}
    fig = P.check(host, ref, s_abs, P.inputs(n)[3], P.upstream(n)[3])
    print("plain_activate N = %4d %-12s worst ratio / bar: %s" % (n, label, P.table(fig)))
    assert not P.failures(fig), (label, n, P.failures(fig))


def _same(a, b):
    return all(poison.same_bits(a[t], b[t]) for t in a)


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.NS)
def test_every_element_against_float64(n):
    ins = [_dev(a) for a in P.inputs(n)]
    ups = [_dev(a) for a in P.upstream(n)]
    plain = _python_route(ins, ups)
    joint = _python_route(ins, ups, joint_extra=37)
    direct = dict(c_forward(ins), **c_backward(ins, ups))
    for label, got in (("python", plain), ("python joint", joint), ("C", direct)):
        _gate(got, n, label)
    assert poison.same_bits(plain["xyz"], ins[0])                              # xyz passes through
    assert _same(plain, joint) and _same(plain, direct)
    assert _same(direct, dict(c_forward(ins), **c_backward(ins, ups)))         # and again


@pytest.mark.parametrize("n", P.NS)
def test_row0_offsets_outputs_and_upstream_rows(n):
    """37 rows: out_rots + 4 * 37 floats is 16-byte aligned and not 64-byte aligned"""
    ins = [_dev(a) for a in P.inputs(n)]
    ups = [_dev(a) for a in P.upstream(n)]
    base = dict(c_forward(ins), **c_backward(ins, ups))
    for row0, cap in ((0, n), (37, n + 37), (37, n + 100)):
        got = dict(c_forward(ins, row0, cap), **c_backward(ins, ups, row0, cap))    # (both assert the rows outside [row0, row0 + n) intact)
        assert _same(base, got), (row0, cap)
    _gate(got, n, "C row0 = 37")


def test_a_null_upstream_gradient_is_a_zero_one():
    n = 257
    ins = [_dev(a) for a in P.inputs(n)]
    ups = [_dev(a) for a in P.upstream(n)]
    for missing in ([0], [1], [2], [3], [0, 1, 2, 3]):
        null = [None if k in missing else u for k, u in enumerate(ups)]
        zero = [torch.zeros_like(u) if k in missing else u for k, u in enumerate(ups)]
        for row0, cap in ((0, n), (37, n + 100)):
            a, b = c_backward(ins, null, row0, cap), c_backward(ins, zero, row0, cap)
            assert _same(a, b), (missing, row0)
            for k in missing:                                  # (d_rotation too: (0 - y 0) / |q| and 0 / eps)
                assert not a[P.BWD[k]].any(), (missing, k)


def test_same_bits_under_every_fill():
    n = 1025
    ins = [_dev(a) for a in P.inputs(n)]
    ups = [_dev(a) for a in P.upstream(n)]
    for extra in (None, 37):
        runs = poison.run_under_fills(lambda: _python_route(ins, ups, joint_extra=extra))
        assert all(p.handed_out >= 4 for p, _ in runs)
        assert poison.differing(runs) == [], extra
    assert _same(runs[0][1], _python_route(ins, ups))


def test_the_rows_kept_out_of_the_gate():
    c = P.special_case()
    ins = [_dev(c[k]) for k in ("xyz", "scaling", "rot", "opac")]
    ups = [_dev(c[k]) for k in P.UPSTREAM]
    for label, got in (("python", _python_route(ins, ups)), ("C row0 = 37", dict(c_forward(ins, 37, 16 + 100), **c_backward(ins, ups, 37, 16 + 100)))):
        host = {t: v.cpu().numpy() for t, v in got.items()}
        assert not P.special_failures(host), (label, P.special_failures(host))
        ref, s_abs = P.reference(*[c[k] for k in ("xyz", "scaling", "rot", "opac")], *[c[k] for k in P.UPSTREAM])
        rows = P.ordinary_special_rows()
        pick = lambda d: {t: np.asarray(d[t]).reshape(16, -1)[rows] for t in P.TENSORS}
        fig = P.check(pick(host), pick(ref), pick(s_abs), c["opac"][rows], c["g_opac"][rows])
        assert not P.failures(fig), (label, P.failures(fig))


def test_no_rows_touches_nothing():
    from gaussianmesh_amd._op import enqueue
    dev = torch.device("cuda:0")
    bufs = [_banded(8, w) for w in UP_WIDTH * 3]
    ins, outs, gs = bufs[:4], bufs[4:8], bufs[8:]
    enqueue(dev, "gm_plain_activate_fwd", 0, *[b[G:] for b in ins], *[b[G:] for b in outs], 0, 8)
    enqueue(dev, "gm_plain_activate_fwd", 0, *[b[G:] for b in ins], *[b[G:] for b in outs], 8, 8)
    enqueue(dev, "gm_plain_activate_bwd", 0, *[b[G:] for b in ins[1:]], *[b[G:] for b in gs], 3, 8, *[b[G:] for b in outs])
    enqueue(dev, "gm_plain_activate_fwd", 0, *([None] * 8), 0, 0)
    enqueue(dev, "gm_plain_activate_bwd", 0, *([None] * 7), 0, 0, *([None] * 4))
    torch.cuda.synchronize()
    assert all((_bits(b) == SENTINEL).all() for b in bufs)
    from gaussianmesh_amd.model_ops import plain_activate
    empty = [torch.zeros((0, w), device="cuda", requires_grad=True) for w in UP_WIDTH]
    out = plain_activate(*empty)
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 4), (0, 1)]
    sum(o.sum() for o in out).backward()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in empty)
