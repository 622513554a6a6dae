"""Animate an edited object: the animation loop of the reference's edit.py (its commented-out part, edit.py:46-54), batched.

    python -m gaussianmesh_amd.edit_sequence (--object_gaussian fg.ply | --object_plain_gaussian cloud.ply) --object_origin_mesh mesh.obj \
        (--mesh_sequence DIR | --handle_sequence FILE.npz) --camera_path MODEL_DIR --render_path OUT [--object_name Object] [--camera_id N]
        [--frames_per_launch 4] [--save_maps] [--save_meshes] [--background_gaussian BG.ply [--is_exist_bg]]

--object_gaussian: the mesh-bound Gaussian PLY of the training code; --object_plain_gaussian: a plain 3DGS PLY instead, bound to the closest
faces of the mesh on load (ObjectVisualTool.add_plain_gaussian).  Exactly one of the two.
--mesh_sequence: a folder of OBJ files in numeric order (1.obj, 2.obj, ...: the reference's `mesh_sequnce`), one frame each.
--handle_sequence: instead of ready-made meshes, an .npz with `handles` (int [H] vertex ids) and `positions` (float [T,H,3]): frame t is the
as-rigid-as-possible deformation with the handles at positions[t] (arap.ArapSolver), solved from frame t - 1's solution (frame 0 from the
rest pose).  Exactly one of --mesh_sequence / --handle_sequence.  --save_meshes also writes every frame's mesh as {i:05d}.obj.
--camera_id N: every frame from camera N of MODEL_DIR/cameras.json, as in the reference loop; without it the frames step through the
cameras, one per frame, cycling.  Frames go through ObjectVisualTool.render_sequence (K frames per launch chain); each is written as
{i:05d}.png, and with --save_maps also {i:05d}_depth.npy / {i:05d}_alpha.npy ([H,W] float32, gm_forward_1_aux's definitions).  The
files are written on the host while the device renders the next batch (the generator issues batch b + 1 before it yields batch b).
--background_gaussian BG.ply: the object in front of a free-standing background cloud (edit.py's --is_exist_bg mode, SceneVisualTool;
--is_exist_bg is accepted and needs the background): frames through SceneVisualTool.render_sequence.  A scene renders no maps, so
--save_maps with a background is refused.
"""
import os
import re
from argparse import ArgumentParser


def mesh_sequence(folder):
    """The OBJ files of a folder in numeric order of their names (1.obj, 2.obj, ..., 10.obj)."""
    names = [n for n in os.listdir(folder) if n.lower().endswith(".obj")]
    key = lambda n: (int(re.sub(r"\D", "", n) or -1), n)
    return [os.path.join(folder, n) for n in sorted(names, key=key)]


def main(argv=None):
    parser = ArgumentParser(description="Render a mesh-driven animation of a mesh-bound Gaussian object")
    which = parser.add_mutually_exclusive_group(required=True)
    which.add_argument("--object_gaussian", type=str, default=None)
    which.add_argument("--object_plain_gaussian", type=str, default=None)
    parser.add_argument("--object_origin_mesh", type=str, required=True)
    parser.add_argument("--object_name", type=str, default="Object")
    parser.add_argument("--camera_path", type=str, required=True)
    parser.add_argument("--render_path", type=str, required=True)
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--mesh_sequence", type=str, default=None)
    source.add_argument("--handle_sequence", type=str, default=None)
    parser.add_argument("--save_meshes", action="store_true", default=False)
    parser.add_argument("--camera_id", type=int, default=None)
    parser.add_argument("--frames_per_launch", type=int, default=4)
    parser.add_argument("--save_maps", action="store_true", default=False)
    parser.add_argument("--background_gaussian", type=str, default=None)
    parser.add_argument("--is_exist_bg", action="store_true", default=False)
    args = parser.parse_args(argv)
    if args.is_exist_bg and args.background_gaussian is None:
        parser.error("--is_exist_bg needs --background_gaussian (the background cloud's PLY)")
    if args.background_gaussian is not None and args.save_maps:
        parser.error("--save_maps: a scene with a background renders no depth / alpha maps; drop --save_maps or the background")

    import numpy as np
    import torch
    from .edittool import ObjectVisualTool, SceneVisualTool
    from .io import read_obj, save_image, write_obj

    if args.mesh_sequence is not None:
        meshes = mesh_sequence(args.mesh_sequence)
        if not meshes:
            raise SystemExit("edit_sequence: no .obj files in %s" % args.mesh_sequence)
    tool = ObjectVisualTool() if args.background_gaussian is None else SceneVisualTool(args.background_gaussian)
    cams = tool.get_camera(args.camera_path)
    if args.object_plain_gaussian is not None:
        tool.add_plain_gaussian(args.object_plain_gaussian, args.object_origin_mesh, args.object_name)
    else:
        tool.add_gaussian(args.object_gaussian, args.object_origin_mesh, args.object_name)
    if args.handle_sequence is not None:
        with np.load(args.handle_sequence) as z:
            handles, positions = np.asarray(z["handles"]).reshape(-1), np.asarray(z["positions"], np.float32)
        if positions.ndim != 3 or positions.shape[1:] != (len(handles), 3):
            raise SystemExit("edit_sequence: %s: positions must be [T,%d,3], got %s" % (args.handle_sequence, len(handles), positions.shape))
        solver = tool.gaussians_list[-1].set_handles(handles)
        meshes, current = [], None
        for t in range(positions.shape[0]):                       # enqueued back to back: no host wait between the solves
            current = solver.solve(positions[t], init=current)
            meshes.append(current)
    frames = [(cams[args.camera_id] if args.camera_id is not None else cams[i % len(cams)], {args.object_name: m})
              for i, m in enumerate(meshes)]
    os.makedirs(args.render_path, exist_ok=True)
    with torch.no_grad():
        for i, out in enumerate(tool.render_sequence(frames, frames_per_launch=args.frames_per_launch, aux=args.save_maps)):
            stem = os.path.join(args.render_path, "{0:05d}".format(i))
            image = out[0] if args.save_maps else out
            save_image(image, stem + ".png")
            if args.save_maps:
                np.save(stem + "_depth.npy", out[1][0].cpu().numpy())
                np.save(stem + "_alpha.npy", out[2][0].cpu().numpy())
            if args.save_meshes:
                m = meshes[i]
                write_obj(stem + ".obj", read_obj(m)[0] if isinstance(m, str) else m.cpu().numpy(), tool.gaussians_list[-1].faces.cpu().numpy())
    return len(frames)


if __name__ == "__main__":
    main()
