"""-m gpu: python -m gaussianmesh_amd.contribution end to end on a tiny Blender-style data set made from this package alone: one trained
scene PLY (a torus inside a shell of background Gaussians) and views whose alpha channel is the torus's own rendered opacity -> an
object PLY and a background PLY whose rows add up to the input's, and a pruned PLY."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, N_VIEWS = 100, 75, 6


def make_dataset(root):
    """scene.ply and N_VIEWS RGBA views: colour = the whole scene on black, alpha = the opacity of the torus rendered alone"""
    from PIL import Image
    from contribution_scene import render_alpha, torus_in_shell, view_dicts
    from gaussianmesh_amd import contribution as cb, io as gio
    pc, n_obj, cams, alphas = torus_in_shell(W, H, N_VIEWS, 50.0, 40, 18, 0.14, 3000, 1.0, seed=4)
    gio.save_plain_gaussians(os.path.join(root, "scene.ply"), cb.plain_columns(pc))
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    frames = []
    for k, (cd, cam, alpha) in enumerate(zip(view_dicts(N_VIEWS, W, H, 50.0), cams, alphas)):
        rgb = render_alpha(pc, pc.get_number, cam, W, H)[0].clamp(0, 1)
        rgba = (torch.cat([rgb, alpha.clamp(0, 1)[None]], 0) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        Image.fromarray(rgba, "RGBA").save(os.path.join(root, "train", "r_%d.png" % k))
        c2w = np.linalg.inv(np.asarray(cd["view"], np.float64).T)
        c2w[:3, 1:3] *= -1                                                # Blender's axes
        frames.append({"file_path": "./train/r_%d" % k, "transform_matrix": c2w.tolist()})
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": math.radians(50.0), "frames": frames}, f)
    return n_obj, pc.get_number


def test_cli_splits_and_prunes(tmp_path, capsys):
    from gaussianmesh_amd import contribution as cb, dataset, io as gio
    root = str(tmp_path)
    n_obj, P = make_dataset(root)
    scene, obj, bg, pruned = (os.path.join(root, n) for n in ("scene.ply", "obj.ply", "bg.ply", "pruned.ply"))
    capsys.readouterr()
    cb.main(["--gaussian", scene, "-s", root, "-r", "1", "--out_object", obj, "--out_background", bg, "--threshold", "0.5",
             "--out_pruned", pruned, "--min_peak", "0.0039215686"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    rep = json.loads(lines[0])
    assert rep["rows"] == P and rep["views"] == N_VIEWS and rep["seconds"] >= 0 and 0 <= rep["rows_never_seen"] < P
    rows = lambda p: gio.read_ply(p)[1].shape[0]
    assert rows(obj) + rows(bg) == rows(scene) == P and rows(obj) == rep["rows_selected"] and rows(pruned) == rep["rows_kept"]
    # what the CLI saw, by hand: the same views, the views' own masks
    pc = cb.load_plain(scene, 3, "cuda")
    views = [dataset.load_view(v, 1, device="cuda") for v in dataset.load_scene(root).train_cameras]
    con = cb.accumulate(pc, [c for c, _ in views], [g for _, g in views])
    assert all(g.mask is not None for _, g in views)
    sel = cb.select(con, 0.5)
    assert int(sel.sum()) == rep["rows_selected"] and int((con.sums[:, 0] == 0).sum()) == rep["rows_never_seen"]
    is_obj = torch.arange(P, device="cuda") < n_obj
    print("CLI: %d rows, %d selected (%d of the torus's %d, %d of the shell's), %d never seen, %d kept by --min_peak 1/255, %d with a non-zero peak" % (
        P, rep["rows_selected"], int(sel[is_obj].sum()), n_obj, int(sel[~is_obj].sum()), rep["rows_never_seen"], rep["rows_kept"],
        int((con.peak_bits != 0).sum())))
    assert not sel[~is_obj].any() and int(sel[is_obj].sum()) > 0.8 * n_obj
    # the object PLY holds exactly the selected rows, the background PLY the others, in order
    assert np.array_equal(gio.read_ply(obj)[1], gio.read_ply(scene)[1][sel.cpu().numpy()])
    assert np.array_equal(gio.read_ply(bg)[1], gio.read_ply(scene)[1][~sel.cpu().numpy()])
    # --min_peak 1/255 keeps exactly the rows with a non-zero peak
    assert rep["rows_kept"] == int((con.peak_bits != 0).sum())
    assert np.array_equal(gio.read_ply(pruned)[1], gio.read_ply(scene)[1][(con.peak_bits != 0).cpu().numpy()])
    # both halves load the way the edit tool loads a plain cloud and a background
    assert cb.load_plain(obj, 3, "cuda").get_number == rep["rows_selected"]
    assert len(gio.load_plain_gaussians(bg)["xyz"]) == P - rep["rows_selected"]
    # the input is never overwritten
    with pytest.raises(SystemExit):
        cb.main(["--gaussian", scene, "-s", root, "--out_background", scene])
