"""CPU: the numpy definition of the deform / shade backward (deform_bwd_ref.py) on the cases of deform_bwd_cases.py, the C entry point's
declaration and refusals, and pose_fit.MeshPose against the mesh oracle.

  * the float64 backward equals torch-float64 autograd through a torch restatement of the forward, to 1e-12 of each tensor's max-norm;
  * r_f32: what the float32 emulation (vertex lists summed sequentially) reaches against float64 per kind and tensor, in units of 2^-24 S_abs -
    measured here, stored in deform_bwd_ref.R_F32, and under the first-order rounding count;
  * the gate ratio <= 2 r_f32 of test_gpu_deform_bwd.py rejects six wrong backwards;
  * gm_deform_shade_bwd is declared, typed, versioned, and refuses before any GPU work;
  * MeshPose.state() against oracle.mesh_oracle.mesh_rs, gradcheck at the rest pose (repeated singular values) and under the twist, the
    det <= 0 refusal.
Run with -s for the tables."""
import os
import re

import numpy as np
import pytest
import torch

import deform_bwd_cases as bc
import deform_bwd_ref as bref
import deform_cases as dc
import deform_ref as ref
from gaussianmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_M22 = 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference against autograd

def _torch_sh(deg, x, y, z, S):
    C0, C1, C2, C3 = ref.SH_C0, ref.SH_C1, ref.SH_C2, ref.SH_C3
    c = lambda v: float(np.float32(v))
    r = c(C0) * S(0)
    if deg > 0:
        r = r - c(C1) * y * S(1) + c(C1) * z * S(2) - c(C1) * x * S(3)
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = (r + c(C2[0]) * xy * S(4) + c(C2[1]) * yz * S(5) + c(C2[2]) * (2.0 * zz - xx - yy) * S(6) + c(C2[3]) * xz * S(7) + c(C2[4]) * (xx - yy) * S(8))
            if deg > 2:
                r = (r + c(C3[0]) * y * (3.0 * xx - yy) * S(9) + c(C3[1]) * xy * z * S(10) + c(C3[2]) * y * (4.0 * zz - xx - yy) * S(11) +
                     c(C3[3]) * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * S(12) + c(C3[4]) * x * (4.0 * zz - xx - yy) * S(13) +
                     c(C3[5]) * z * (xx - yy) * S(14) + c(C3[6]) * x * (xx - 3.0 * yy) * S(15))
    return r


def _autograd(deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate):
    """torch float64: the forward in matrix form, loss = <g, outputs>, gradients by autograd"""
    t = lambda a, rg=False: torch.tensor(np.asarray(a, np.float64), requires_grad=rg)
    n = (deg + 1) ** 2
    tri = torch.tensor(np.asarray(tri, np.int64))
    w = t(w)
    dV, Rv, Sv, cov, pos = t(dV, True), t(np.reshape(Rv, (-1, 3, 3)), True), t(np.reshape(Sv, (-1, 3, 3)), True), t(np.reshape(cov, (-1, 3, 3)), True), t(pos, True)
    sh = t(np.asarray(shs)[:, :n], True)
    blend = lambda tab: sum(w[:, k].reshape((-1,) + (1,) * (tab.dim() - 1)) * tab[tri[:, k]] for k in range(3))
    d, Rb, Sb = blend(dV), blend(Rv), blend(Sv)
    RS = Rb.transpose(1, 2) @ Sb
    O = RS @ cov @ RS.transpose(1, 2)
    cov6 = torch.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], 1)
    npos = pos + d
    v = npos - t(campos)
    xyz = (Rb @ (v / v.norm(dim=1, keepdim=True))[:, :, None])[:, :, 0]
    r = _torch_sh(deg, xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3], lambda k: sh[:, k, :])
    rgb = torch.where(torch.tensor(np.asarray(gate, bool)), r + 0.5, torch.zeros_like(r))
    ((npos * t(g_pos)).sum() + (cov6 * t(g_cov6)).sum() + (rgb * t(g_rgb)).sum()).backward()
    g_shs = np.zeros(np.shape(shs), np.float64)
    g_shs[:, :n] = sh.grad.numpy()
    return {"g_dV": dV.grad.numpy(), "g_Rv": Rv.grad.numpy().reshape(-1, 9), "g_Sv": Sv.grad.numpy().reshape(-1, 9), "g_shs": g_shs,
            "g_cov": cov.grad.numpy().reshape(-1, 9), "g_rest_pos": pos.grad.numpy()}


def _gate64(kind, deg, campos, n=dc.NMAX):
    return bc.forward64(kind, deg, campos, n)[1] > 0


@pytest.mark.parametrize("kind", bc.KINDS)
def test_float64_backward_equals_autograd(kind):
    worst = dict.fromkeys(bref.TENSORS, 0.0)
    for deg in range(4):
        for _, campos in bc.cameras(kind):
            a = bc.args(kind, deg, campos)
            gate = _gate64(kind, deg, campos)
            got = bref.backward(*a, gate, np.float64)
            want = _autograd(*a, gate)
            for t in bref.TENSORS:
                scale = np.abs(want[t]).max()
                assert scale > 0 or t == "g_shs", (kind, deg, t)
                err = np.abs(got[t] - want[t]).max() / (scale or 1.0)
                worst[t] = max(worst[t], err)
                assert err <= 1e-12, (kind, deg, t, err)
            assert not got["g_shs"][:, (deg + 1) ** 2:].any()
    print("float64 backward against autograd, %s: " % kind + "  ".join("%s %.2g" % (t, worst[t]) for t in bref.TENSORS))


# ---------------------------------------------------------------------------------------------------------------------------------------
# r_f32 and the gate

def _emulation_ratios(kind, deg, campos, variant=None, n=dc.NMAX):
    """ratios of the float32 emulation (or a wrong variant) against float64, both from the emulation's own float32 deformed positions"""
    a = bc.args(kind, deg, campos, n)
    gate = _gate64(kind, deg, campos, n)
    got, npos32 = bref.backward(*a, gate, np.float32, variant=variant, want_npos=True)
    assert all(v.dtype == np.float32 for v in got.values()) and npos32.dtype == np.float32
    want = bref.backward(*a, gate, np.float64, npos_dir=npos32)
    s_abs = bref.backward_abs(*a, gate, npos_dir=npos32)
    return bref.ratios(got, want, s_abs)


@pytest.mark.parametrize("kind", bc.KINDS)
def test_r_f32_is_measured_and_under_its_rounding_count(kind):
    measured = dict.fromkeys(bref.TENSORS, 0.0)
    for deg in range(4):
        for _, campos in bc.cameras(kind):
            for n in bc.NS:                     # the prefixes the device test runs: other vertex lists, other sums
                for t, r in _emulation_ratios(kind, deg, campos, n=n).items():
                    measured[t] = max(measured[t], float(r.max()))
    longest = int(bc.list_lengths(kind).max())
    print("\nr_f32 %-11s (longest list %3d): " % (kind, longest) + "  ".join("%s %.3f / %.1f / %.1f" % (t, measured[t], bref.R_F32[kind][t], bref.count(t, longest))
                                                                              for t in bref.TENSORS))
    for t in bref.TENSORS:
        assert measured[t] <= bref.count(t, longest), (kind, t, measured[t])
        assert measured[t] <= bref.R_F32[kind][t] <= measured[t] + 0.15, (kind, t, measured[t], bref.R_F32[kind][t])


@pytest.mark.parametrize("variant", bref.VARIANTS)
def test_the_gate_rejects_a_wrong_backward(variant):
    """each mutant must exceed 2 r_f32 on some case; the correct emulation is at most half the bar by construction"""
    rejected = []
    for kind in bc.KINDS:
        for deg in range(4):
            r = _emulation_ratios(kind, deg, dc.CAMPOS, variant)
            over = [t for t in r if not r[t].max() <= 2.0 * bref.R_F32[kind][t]]
            if over:
                rejected.append((kind, deg, over))
    print("%s: rejected on %d of %d (kind, degree) pairs, first %s" % (variant, len(rejected), 4 * len(bc.KINDS), rejected[:1]))
    assert rejected, variant


def test_the_cases_are_what_they_claim():
    n = bc.list_lengths("edges")
    assert [int(n[v]) for v in range(6)] == [0, 1, 63, 64, 65, 129] and n[-1] == 0 and n.sum() == 3 * dc.NMAX
    n = bc.list_lengths("hub")
    assert n[bc.HUB] >= 3 * bc.HUB_ROWS > 4 * 64
    assert bc.list_lengths("last_unused")[-1] == 0 and bc.list_lengths("twist")[-1] > 0
    for kind in bc.KINDS:
        u = bc.upstream(kind)
        assert all(not v.flags.writeable and v.dtype == np.float32 for v in u.values())
        off, ent = bref.incidence(bc.case(kind)["tri"], bc.case(kind)["Vm"])
        flat = bc.case(kind)["tri"].reshape(-1)
        for v in (0, 5, 50, 95):
            e = ent[off[v]:off[v + 1]]
            assert (flat[e] == v).all() and (np.diff(e) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the entry point

def test_header_declares_and_lib_types_the_entry_points():
    syms = _lib.header_symbols()
    assert "gm_deform_shade_bwd" in syms and "gm_deform_shade_bwd_workspace_bytes" in syms
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\bint\s+gm_deform_shade_bwd\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 27 == len(_lib.SIGNATURES["gm_deform_shade_bwd"][1])
    assert len(_lib.SIGNATURES["gm_deform_shade_bwd_workspace_bytes"][1]) == 2
    l = _lib.lib()
    assert hasattr(l, "gm_deform_shade_bwd")
    assert re.search(r"#define\s+GM_ABI_VERSION\s+3\b", text) and l.gm_abi_version() == 3
    assert l.gm_deform_shade_bwd_workspace_bytes(1000, 96) >= 1000 * 21 * 4 and l.gm_deform_shade_bwd_workspace_bytes(0, 96) == 0
    assert "gm_deform_bwd.hip" in open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "gm_deform_bwd.hip")).read()
    assert "#pragma clang fp contract(off)" in src and not re.findall(r"atomic\w*\s*\(|hipMalloc\w*|hip\w*Synchronize|hipMemset\w*", src)


NAMES = ("tri", "w", "dV", "Rv", "Sv", "cov", "pos", "shs", "campos", "inc_offsets", "inc_entries", "g_pos", "g_cov6", "g_rgb", "g_dV", "g_Rv", "g_Sv",
         "g_shs", "g_cov", "g_rest_pos", "workspace")


def test_refuses_before_any_gpu_work():
    l = _lib.lib()
    N, Vm, M = 10, 5, 16
    base = {name: (k + 1) << 24 for k, name in enumerate(NAMES)}                # non-null "pointers" 16 MiB apart: never dereferenced, every call is refused first
    need = l.gm_deform_shade_bwd_workspace_bytes(N, Vm)

    def call(N=N, deg=3, M=M, Vm=Vm, ws_bytes=need, **kw):
        p = dict(base, **kw)
        return l.gm_deform_shade_bwd(N, deg, M, Vm, *[p[k] for k in NAMES], ws_bytes, None)

    err = lambda: l.gm_last_error()
    assert call(N=-1) == 1 and b"negative" in err()
    assert call(Vm=-1) == 1 and b"negative" in err()
    for deg in (-1, 4, 100):
        assert call(deg=deg) == 1 and b"degree" in err(), deg
    for deg, m in ((3, 15), (2, 8), (1, 3), (0, 0), (3, -16)):
        assert call(deg=deg, M=m) == 1 and b"coefficients" in err(), (deg, m)
    assert call(Vm=0) == 1 and b"Vm = 0" in err()
    mandatory = [k for k in NAMES if k not in ("g_cov6", "g_rgb", "g_shs", "g_cov", "g_rest_pos")]
    for k in mandatory:
        assert call(**{k: None}) == 1 and b"null" in err(), k
    assert call(g_cov6=None, g_rgb=None) == 1 and b"g_shs" in err()
    assert call(ws_bytes=need - 1) == 1 and b"workspace" in err()
    # outputs against inputs, outputs against each other, the workspace against both
    sizes = dict(g_dV=12 * Vm, g_Rv=36 * Vm, g_Sv=36 * Vm, g_shs=M * 12 * N, g_cov=36 * N, g_rest_pos=12 * N, workspace=need)
    for out, n in sizes.items():
        for other in ("dV", "shs", "inc_entries", "g_pos", "g_cov6", "g_rgb", "campos", "w"):
            assert call(**{other: base[out] + n - 4}) == 1 and (b"%s overlaps %s" % (out.encode(), other.encode())) in err(), (out, other)
    assert call(g_Rv=base["g_dV"] + 4) == 1 and b"g_dV overlaps g_Rv" in err()
    assert call(workspace=base["g_shs"] + 8) == 1 and b"g_shs overlaps workspace" in err()
    assert call(g_rest_pos=base["g_cov"]) == 1 and b"g_cov overlaps g_rest_pos" in err()
    assert call(N=0, Vm=0) == 0 and l.gm_deform_shade_bwd(0, 3, 16, 0, *([None] * 21), 0, None) == 0       # nothing to write: nothing launched


# ---------------------------------------------------------------------------------------------------------------------------------------
# pose_fit.MeshPose

def _poses():
    """rest vertices (float32-representable, as an object holds them), faces, and the three deformed meshes"""
    import math
    verts, faces, V1t, _, _ = dc.mesh()
    verts = verts.astype(np.float32).astype(np.float64)
    ax = np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    rot = np.eye(3) + math.sin(0.7) * K + (1 - math.cos(0.7)) * K @ K
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    return verts, faces, {"identity": verts, "twist": r32(V1t), "rigid": r32(1.3 * verts @ rot.T + np.array([0.3, -0.2, 0.5]))}


@pytest.mark.parametrize("pose", ["identity", "twist", "rigid"])
def test_mesh_pose_state_against_the_oracle(pose):
    """MeshPose.state() (one-ring fit by index_add, Newton polar iteration) against oracle.mesh_oracle.mesh_rs (numpy solve + SVD) on the
    same float64 inputs.  Measured here: the largest float64 difference of R and S over the three poses is 2.0e-15 (x86-64, numpy +
    OpenBLAS); asserted: ten times that, 2e-14, the margin for another libm / BLAS.  The float32 tensors state() returns by default are
    held to 2^-22 max(1, |ref|): the rounding of the cast and no more."""
    from oracle import mesh_oracle
    from gaussianmesh_amd.pose_fit import MeshPose
    verts, faces, poses = _poses()
    V1 = poses[pose]
    R, S = mesh_oracle.mesh_rs(verts, V1, faces)
    mp = MeshPose(torch.tensor(verts, dtype=torch.float32), faces)
    dV64, R64, S64 = (t.detach().numpy() for t in mp.state(torch.tensor(V1), dtype=torch.float64))
    worst = max(np.abs(R64 - R).max(), np.abs(S64 - S).max())
    print("MeshPose against the oracle, %s: largest float64 difference %.3g" % (pose, worst))
    assert worst <= 2e-14 and np.array_equal(dV64, V1 - verts)
    dV32, R32, S32 = mp.state(torch.tensor(V1, dtype=torch.float32))
    assert all(t.dtype is torch.float32 for t in (dV32, R32, S32)) and R32.shape == (verts.shape[0], 3, 3)
    for got, want in ((R32, R), (S32, S), (dV32, V1 - verts)):
        assert (np.abs(got.detach().numpy() - want) <= TWO_M22 * np.maximum(1.0, np.abs(want))).all()
    if pose == "identity":
        assert np.abs(R - np.eye(3)).max() <= 1e-12 and np.abs(S - np.eye(3)).max() <= 1e-12
    if pose == "rigid":
        assert np.abs(S - 1.3 * np.eye(3)).max() <= 1e-5                       # (the vertices are rounded to float32: 1e-7 of edges of 0.5)


@pytest.mark.parametrize("pose", ["identity", "twist"])
def test_mesh_pose_gradcheck(pose):
    """float64 gradcheck of state() - at the rest pose every vertex has three equal singular values, where an SVD's backward is infinite"""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.pose_fit import MeshPose
    verts, faces = scenes.torus_mesh(6, 5)                                      # (30 vertices: gradcheck perturbs every coordinate)
    verts = verts.astype(np.float32).astype(np.float64)
    mp = MeshPose(torch.tensor(verts, dtype=torch.float32), faces)
    V1 = torch.tensor(verts if pose == "identity" else scenes.twist_bend_frame(verts, t=9)[0], requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: mp.state(v, dtype=torch.float64), (V1,), eps=1e-6, atol=1e-6, rtol=1e-4)
    dV, R, S = mp.state(V1, dtype=torch.float64)
    g, = torch.autograd.grad((R * R.detach().roll(1, 0)).sum() + (S ** 3).sum(), V1)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_mesh_pose_refuses_a_mirrored_ring():
    """one vertex's ring mirrored in the vertex's tangent plane: the torus is curved, so the ring's edges have a normal component, and the
    fitted map sends it to its negative - a reflection"""
    from gaussianmesh_amd.pose_fit import MeshPose
    verts, faces, _ = _poses()
    mp = MeshPose(torch.tensor(verts, dtype=torch.float32), faces)
    v = 37
    around = faces[(faces == v).any(1)]
    n = np.zeros(3)
    for f in around:
        k = int(np.where(f == v)[0][0])
        n += np.cross(verts[f[(k + 1) % 3]] - verts[v], verts[f[(k + 2) % 3]] - verts[v])
    n /= np.linalg.norm(n)
    ring = np.setdiff1d(np.unique(around), [v])
    V1 = verts.copy()
    V1[ring] = verts[ring] - 2.0 * ((verts[ring] - verts[v]) @ n)[:, None] * n
    assert float(torch.linalg.det(mp.deformation_gradients(torch.tensor(V1)))[v]) < 0
    with pytest.raises(ValueError, match=r"det T <= 0 at vertex \d+") as e:       # (the first such vertex: the ring's members see a folded ring too)
        mp.state(torch.tensor(V1))
    assert int(re.search(r"vertex (\d+)", str(e.value)).group(1)) in set(ring) | {v}
    mp.state(torch.tensor(verts))                                               # (the rest pose itself is accepted)
