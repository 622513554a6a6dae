"""-m gpu: pose_fit on the device - MeshPose.state() against gm_mesh_rs, and an end-to-end fit of a twisted torus from three views.

The fit's figures (60 Adam steps from rest, the default lr - 1e-3 of the mean edge - and rigidity 1; NOTEBOOK.md "Pose fitting") are printed, not turned into thresholds: the
test asserts only that the loss of every view and the vertex error to the target pose went down, and that the object ends in the fitted pose."""
import numpy as np
import pytest
import torch

import deform_cases as dc

pytestmark = pytest.mark.gpu


def test_mesh_pose_state_against_gm_mesh_rs():
    """the twist frame t = 9 of deform_cases.mesh(): the bar of the host comparison, 2^-22 max(1, |ref|) per element"""
    from gpu_utils import T
    from gaussianmesh_amd import deform
    from gaussianmesh_amd.pose_fit import MeshPose
    verts, faces, V1, _, _ = dc.mesh()
    v0, v1, f = T(verts), T(V1), T(faces, dtype=torch.int32)
    R, S = deform.mesh_rs(v0, v1, f)
    mp = MeshPose(v0, f)
    assert mp.V1.device == v0.device and mp.e_row.device == v0.device
    dV, R1, S1 = mp.state(v1)
    for name, got, want in (("R", R1, R), ("S", S1, S), ("dV", dV, v1 - v0)):
        err = ((got - want).abs() / want.abs().clamp_min(1.0)).max().item()
        print("MeshPose on the device against gm_mesh_rs, %s: worst |diff| / max(1, |ref|) = %.3g (bar %.3g)" % (name, err, 2.0 ** -22))
        assert err <= 2.0 ** -22, name


def test_fit_a_twisted_torus_from_three_views():
    from gpu_utils import T
    from gaussianmesh_amd import GaussianRasterizer, scenes
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.renderer import Camera, _settings
    W, H, steps = 96, 64, 60
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(4000, verts, faces, seed=5)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    obj = SingleObjectDeform(T(cl["means"]), T(cov), T(cl["opac"]), T(cl["shs"]), T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(verts))
    dev = obj.vertex.device
    cams = [Camera(scenes.orbit_camera(k, 3, W, H, radius=6.0), dev) for k in range(3)]
    V1, R, S = (T(a) for a in scenes.twist_bend_frame(verts, t=4))
    bg = torch.ones(3, device=dev)
    views = []
    with torch.no_grad():
        for cam in cams:
            pos, rgb, cov6 = obj.deform_and_shade(V1, R, S, cam.camera_center)
            image, radii = GaussianRasterizer(_settings(cam, bg, 1.0, 3, False))(pos, torch.zeros_like(pos), obj.gaussian_o, colors_precomp=rgb,
                                                                                 cov3D_precomp=cov6)
            assert int((radii > 0).sum()) > 1000
            views.append((cam, image.clone()))
    obj.deform_state = None                                 # the fit starts at rest
    fitter = obj.fit_pose(views, steps, faces=T(faces, dtype=torch.int32))
    losses = torch.stack(fitter.losses).cpu().numpy()
    assert losses.shape == (steps,) and np.isfinite(losses).all()
    fitted = fitter.pose.V1.detach()
    rms = lambda a: float(((a - V1) ** 2).sum(1).mean().sqrt())
    start, end = rms(obj.vertex), rms(fitted)
    print("pose fit, %d steps: loss per view first -> last %s; ratio %.3f; vertex RMS error %.4f -> %.4f, ratio %.3f" % (
        steps, ", ".join("%.4f -> %.4f" % (losses[k], losses[steps - 3 + k]) for k in range(3)), losses[-3:].mean() / losses[:3].mean(), start, end,
        end / start))
    for k in range(3):                                      # steps k and 57 + k saw the same view
        assert losses[steps - 3 + k] < losses[k], k
    assert end < start
    # the object ends in the fitted pose, with gm_mesh_rs's own (R, S)
    from gaussianmesh_amd.deform import mesh_rs
    sV, sR, sS = obj.deform_state
    assert torch.equal(sV, fitted)
    R2, S2 = mesh_rs(obj.vertex, fitted, obj.faces)
    assert torch.equal(sR, R2) and torch.equal(sS, S2)
    assert torch.equal(obj.mesh_vertex_current, fitted) and obj.gaussian_deform_pos.shape == (4000, 3)
