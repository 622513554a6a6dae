"""Animate an edited object: the animation loop of the reference's edit.py (its commented-out part, edit.py:46-54), batched.

    python -m gaussianmesh_amd.edit_sequence (--object_gaussian fg.ply | --object_plain_gaussian cloud.ply) --object_origin_mesh mesh.obj \
        (--mesh_sequence DIR | --handle_sequence FILE.npz | --pick_sequence FILE.json | --pose_sequence FILE.json --skeleton FILE.json)
        --camera_path MODEL_DIR --render_path OUT [--object_name Object] [--camera_id N]
        [--frames_per_launch 4] [--save_maps] [--save_meshes] [--save_baked PATH] [--background_gaussian BG.ply [--is_exist_bg]]
        [--arap_global_step {column,grid}] [--arap_batch K] [--inbetweens N [--ease {linear,smoothstep}]]
        [--skin_blend {dqs,linear}] [--skin_heat C] [--skin_influences K]
        [--dynamics [--settle N] [--dt S] [--stiffness K] [--damping G] [--gravity X Y Z]
                    [--floor H] [--friction MU] [--contact_stiffness KC] [--colliders FILE.json]
                    [--background_contact [RES] [--contact_margin M]]
                    [--obstacle_mesh FILE.obj [--obstacle_resolution RES] [--obstacle_margin M] [--obstacle_motion FILE.json]]]

--object_gaussian: the mesh-bound Gaussian PLY of the training code; --object_plain_gaussian: a plain 3DGS PLY instead, bound to the closest
faces of the mesh on load (ObjectVisualTool.add_plain_gaussian).  Exactly one of the two.
--mesh_sequence: a folder of OBJ files in numeric order (1.obj, 2.obj, ...: the reference's `mesh_sequnce`), one frame each.
--handle_sequence: instead of ready-made meshes, an .npz with `handles` (int [H] vertex ids) and `positions` (float [T,H,3]): frame t is the
as-rigid-as-possible deformation with the handles at positions[t] (arap.ArapSolver), solved from frame t - 1's solution (frame 0 from the
rest pose).
--pick_sequence: the same from the screen, a JSON file with "camera_id" (the camera of MODEL_DIR/cameras.json in which the pixels are
meant), "handles" [[x, y], ...] (the pixels whose picked vertices move), optionally "anchors" [[x, y], ...] (picks held at their rest
position) and "offsets" [T][len(handles)][2] (per frame the pixel offsets from the original pick).  The picks are resolved once, on the
rest mesh (SingleObjectDeform.pick: the hit face's corner nearest the hit); a pick that misses the mesh, or two picks of one vertex, end
the run.  Frame t has the handles at their rest positions moved by offsets[t] parallel to the image plane (mesh_pick.screen_offset) and
the anchors in place, solved from frame t - 1's solution as above.
Two optional keys turn the picks into surface REGIONS (mesh_region): "grab_radius" (a number >= 0, in mesh units; 0 when only
"free_radius" is given) and "free_radius" (a number >= grab_radius).  Every vertex within grab_radius of a handle's picked vertex, measured
along the rest mesh, moves with that handle as one rigid patch; every vertex within grab_radius of an anchor's and, with "free_radius",
every vertex farther than free_radius from all handles stays at its rest position; the band in between bends
(SingleObjectDeform.set_region_handles / drag_region).  Two handle regions that overlap, or a handle region that meets an anchor's, end
the run with a message naming the picks.  With neither key nothing changes: single-vertex handles as above.
--pose_sequence: the mesh posed from a skeleton (skinning.SkinBinding: bone-heat weights solved once on the device, then one skinning launch
for all frames).  --skeleton FILE.json (required with it) holds {"joints": [[x, y, z], ...], "parents": [...], "names": [...] (optional)}:
joint 0 is the root (parent -1), a parent comes before its child, bone b runs from joint parents[b + 1] to joint b + 1.  The pose file
holds {"rotations": [T][Nj][3], "root_translation": [T][3] (optional)}: per frame one axis-angle vector (radians) per joint, about that
joint's rest position, children following their parents, and a translation of the root.  --skin_blend dqs (the default: dual quaternions,
a twisted limb keeps its volume) or linear; --skin_heat C (default 1: larger pins a vertex harder to its nearest bone);
--skin_influences K (default 4: bones kept per vertex, 1 .. 4).  The four are refused without --pose_sequence; --pose_sequence is refused
with --dynamics and with --arap_batch above 1, and composes with --inbetweens, --save_meshes, --save_baked and --background_gaussian as
--mesh_sequence does.
Exactly one of --mesh_sequence / --handle_sequence / --pick_sequence / --pose_sequence.  --save_meshes also writes every frame's mesh as {i:05d}.obj.
--arap_global_step: the solver's global step for --handle_sequence / --pick_sequence, ArapSolver.solve's global_step: column (the default:
one workgroup per coordinate) or grid (rows over the whole chip; the same meshes to within the last bits).
--arap_batch K: for --handle_sequence / --pick_sequence, K frames' solves per launch chain (ArapSolver.solve_sequence, K in 1 .. 64): the
frames go in runs of K, and every frame of a run starts from the last frame of the previous run instead of from its own predecessor, so
the meshes differ a little from K = 1's.  The default 1 is the chain described above, bit for bit.  What K buys and costs: INTEGRATION.md
section Q.
--inbetweens N: the frames of --mesh_sequence / --handle_sequence / --pick_sequence become KEY poses, with the rest pose as key 0, and N
rotation-aware in-betweens are rendered between consecutive keys (pose_interp.PoseInterpolator.sequence: every face's rotation along its
geodesic, its stretch linearly, one Poisson solve per frame): K source frames give K (N + 1) + 1 frames, the keys among them bit for bit.
--ease smoothstep spaces the in-betweens of a segment by 3 t^2 - 2 t^3 instead of evenly.  The default 0 changes nothing: the source's
frames, no rest pose in front.  A face that turns by nearly half a turn between two keys may turn either way: add a key.
--dynamics: the frames of --handle_sequence / --pick_sequence are SIMULATED steps instead of per-frame ARAP solves (SingleObjectDeform.simulate,
dynamics.MeshDynamics): the mesh has velocity, so a dragged part follows through and swings back.  Every handle row is scripted to its
position in each frame; anchors and held regions are rows whose scripted position is their rest position in every frame, which pins them.
--settle N appends N steps with the handles held at their last positions (the mesh comes to rest); --dt (seconds per frame), --stiffness,
--damping and --gravity X Y Z set the material, by default MeshDynamics' own.  Refused with --mesh_sequence (there is nothing to solve),
with --arap_batch above 1 and with --inbetweens above 0; --settle and the material flags are refused without --dynamics.  Without these
flags nothing changes.
--floor H (with --dynamics and a non-zero --gravity): the ground, a half-space whose normal is opposite to gravity and whose surface lies at
height H along that normal (dynamics.floor); the simulated mesh cannot sink through it.  --friction MU: the floor's Coulomb friction, and
the default of the colliders of --colliders (0 without it).  --contact_stiffness KC: MeshDynamics' contact_stiffness (a body rests about
|gravity| / KC deep).  --colliders FILE.json: a list of {"kind": "half_space", "normal": [x, y, z], "offset": d or "point": [x, y, z],
"friction": mu} and {"kind": "sphere", "radius": r, "center": [x, y, z] or "centers": [[x, y, z], ...], "friction": mu}; "centers" gives a
moving ball its centre in every frame (the last one is kept for frames beyond the list, --settle's included).  At most 16 colliders with
the floor.  All four are refused without --dynamics; without them nothing changes.
--background_contact [RES] (with --dynamics and --background_gaussian): the simulated mesh also collides with the background cloud itself.
The cloud's depth and opacity maps from ALL cameras of MODEL_DIR/cameras.json are fused into a signed-distance volume of RES (default 128)
voxels along the longest side of the object's rest box grown by --contact_margin M (default 0.5) times that side
(SceneVisualTool.background_field, dynamics.SdfGrid); the volume is one more collider, behind --floor and --colliders, with --friction as
its friction and --contact_stiffness as everyone's.  Where no view saw the background the volume knows nothing and nothing is in contact
with it.  Refused without --dynamics or without --background_gaussian; --contact_margin is refused without it.
--obstacle_mesh FILE.obj (with --dynamics): the simulated mesh also collides with the triangle mesh of FILE.obj, a static solid - a
table, a bowl, a neighbour's proxy mesh; it may be open or wound inwards (mesh_sdf, the generalized winding number).  Its signed distances
are sampled on a volume of --obstacle_resolution RES (default 128) voxels along the longest side of the OBSTACLE's box grown by
--obstacle_margin M (default 0.5) times that side (dynamics.SdfGrid.from_mesh); the volume is one more collider, behind --floor and
--colliders, with --friction as its friction and --contact_stiffness as everyone's.  Refused without --dynamics and together with
--background_contact (a simulation takes one volume); --obstacle_resolution and --obstacle_margin are refused without it.
--obstacle_motion FILE.json (with --obstacle_mesh): the obstacle MOVES rigidly - a JSON list with one 3x4 or 4x4 matrix (R | t) per
simulated frame (--settle's frames included), world = R p + t for a point p of FILE.obj; the mesh is pushed and carried by it, with
--friction acting in the obstacle's own frame (MeshDynamics(fields=), run(field_poses=)).  Refused without --obstacle_mesh, with another
number of frames than the simulation has, and with a matrix that is not finite or whose R is no rotation (|R^T R - I| <= 1e-6, det R > 0).
--camera_id N: every frame from camera N of MODEL_DIR/cameras.json, as in the reference loop; without it the frames step through the
cameras, one per frame, cycling.  Frames go through ObjectVisualTool.render_sequence (K frames per launch chain); each is written as
{i:05d}.png, and with --save_maps also {i:05d}_depth.npy / {i:05d}_alpha.npy ([H,W] float32, gm_forward_1_aux's definitions).  The
files are written on the host while the device renders the next batch (the generator issues batch b + 1 before it yields batch b).
--save_baked PATH: after rendering, the object in the state of the LAST frame of the sequence as a plain Gaussian PLY (the tool's
save_baked: positions, (scale, quaternion) of the deformed covariances, SH rows re-expressed in the unrotated frame), for any 3DGS viewer or
trainer, or --object_plain_gaussian with that frame's mesh.  One file, not one per frame (about 250 MB each at a million Gaussians).
--background_gaussian BG.ply: the object in front of a free-standing background cloud (edit.py's --is_exist_bg mode, SceneVisualTool;
--is_exist_bg is accepted and needs the background): frames through SceneVisualTool.render_sequence.  A scene renders no maps, so
--save_maps with a background is refused.
"""
import os
import re
from argparse import ArgumentParser


ARAP_BATCH_MAX = 64           # GM_ARAP_BATCH_MAX (include/gmesh_hip.h, _lib.GM_ARAP_BATCH_MAX): here so that --arap_batch is refused before any import


def mesh_sequence(folder):
    """The OBJ files of a folder in numeric order of their names (1.obj, 2.obj, ..., 10.obj)."""
    names = [n for n in os.listdir(folder) if n.lower().endswith(".obj")]
    key = lambda n: (int(re.sub(r"\D", "", n) or -1), n)
    return [os.path.join(folder, n) for n in sorted(names, key=key)]


def read_pick_sequence(path):
    """A --pick_sequence file -> (camera_id, handles float32 [H,2], anchors float32 [A,2], offsets float32 [T,H,2]); SystemExit naming
    what is wrong with it.  Host work only.  A file with "grab_radius" or "free_radius" gives a fifth element, (grab_radius float,
    free_radius float or None)."""
    import json
    import numpy as np
    bad = lambda what: SystemExit("edit_sequence: %s: %s" % (path, what))
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError) as e:
        raise bad("cannot read it as JSON (%s)" % e)
    if not isinstance(doc, dict):
        raise bad("must hold a JSON object")
    cam = doc.get("camera_id")
    if not isinstance(cam, int) or isinstance(cam, bool) or cam < 0:
        raise bad('"camera_id" (the camera in which the pixels are meant) is required: a non-negative integer')

    def pixels(key, required):
        if key not in doc and not required:
            return np.zeros((0, 2), np.float32)
        try:
            a = np.asarray(doc.get(key), np.float32)
        except (TypeError, ValueError):
            a = None
        if a is None or a.ndim != 2 or a.shape[1] != 2 or (required and a.shape[0] == 0) or not np.isfinite(a).all():
            raise bad('"%s" must be a list of [x, y] pixels%s' % (key, ", at least one" if required else ""))
        return a
    handles, anchors = pixels("handles", True), pixels("anchors", False)
    try:
        offsets = np.asarray(doc.get("offsets"), np.float32)
    except (TypeError, ValueError):
        offsets = None
    if offsets is None or offsets.ndim != 3 or offsets.shape[0] == 0 or offsets.shape[1:] != (len(handles), 2) or not np.isfinite(offsets).all():
        raise bad('"offsets" must be [T][%d][2] pixel offsets, T >= 1; got shape %s' % (len(handles), None if offsets is None else offsets.shape))
    if "grab_radius" not in doc and "free_radius" not in doc:
        return cam, handles, anchors, offsets

    def radius(key):
        r = doc.get(key)
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0.0 <= float(r) < float("inf"):
            raise bad('"%s" must be a finite number >= 0 (a distance along the mesh, in its units); got %r' % (key, r))
        return float(r)
    grab = radius("grab_radius") if "grab_radius" in doc else 0.0
    free = radius("free_radius") if "free_radius" in doc else None
    if free is not None and free < grab:
        raise bad('"free_radius" %g is below "grab_radius" %g' % (free, grab))
    return cam, handles, anchors, offsets, (grab, free)


def read_pose_sequence(path, joints=None):
    """A --pose_sequence file -> (rotations float64 [T,Nj,3] axis-angle, root_translation float64 [T,3] or None); SystemExit naming what
    is wrong with it.  joints: the skeleton's joint count, where it is known.  Host work only."""
    import json
    import numpy as np
    bad = lambda what: SystemExit("edit_sequence: %s: %s" % (path, what))
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError) as e:
        raise bad("cannot read it as JSON (%s)" % e)
    if not isinstance(doc, dict):
        raise bad("must hold a JSON object")
    try:
        rot = np.asarray(doc.get("rotations"), np.float64)
    except (TypeError, ValueError):
        rot = None
    if rot is None or rot.ndim != 3 or rot.shape[0] == 0 or rot.shape[2] != 3 or (joints is not None and rot.shape[1] != joints) or not np.isfinite(rot).all():
        raise bad('"rotations" must be [T][%s][3] finite axis-angle vectors, one per joint, T >= 1; got shape %s'
                  % ("Nj" if joints is None else joints, None if rot is None else rot.shape))
    if "root_translation" not in doc:
        return rot, None
    try:
        tr = np.asarray(doc.get("root_translation"), np.float64)
    except (TypeError, ValueError):
        tr = None
    if tr is None or tr.shape != (rot.shape[0], 3) or not np.isfinite(tr).all():
        raise bad('"root_translation" must be [%d][3] finite numbers, one row per frame; got shape %s' % (rot.shape[0], None if tr is None else tr.shape))
    return rot, tr


def read_obstacle_motion(path):
    """An --obstacle_motion file -> poses float64 [T,3,4]; SystemExit naming what is wrong with it.  Host work only."""
    import json
    import numpy as np
    bad = lambda what: SystemExit("edit_sequence: %s: %s" % (path, what))
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError) as e:
        raise bad("cannot read it as JSON (%s)" % e)
    try:
        m = np.asarray(doc, np.float64)
    except (TypeError, ValueError):
        m = None
    if m is None or m.ndim != 3 or m.shape[0] == 0 or tuple(m.shape[1:]) not in ((3, 4), (4, 4)):
        raise bad("must hold a JSON list of 3x4 or 4x4 matrices, one per frame, at least one; got shape %s" % (None if m is None else m.shape,))
    if m.shape[1] == 4 and not (np.isfinite(m).all() and np.array_equal(m[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(m), 1)))):
        raise bad("the last row of a 4x4 matrix must be 0 0 0 1")
    m = m[:, :3]
    R = m[:, :, :3]
    for k in range(len(m)):                                            # MeshDynamics' host check, frame by frame
        if not np.isfinite(m[k]).all() or float(np.abs(R[k].T @ R[k] - np.eye(3)).max()) > 1e-6 or not np.linalg.det(R[k]) > 0.0:
            raise bad("frame %d: the matrix must be finite, (R | t) with R a rotation (|R^T R - I| <= 1e-6, det R > 0)" % k)
    return np.ascontiguousarray(m)


def read_colliders(path, friction):
    """A --colliders file -> (colliders: a list of dicts for MeshDynamics, moving: {index: centres [[x, y, z], ...]}); SystemExit naming
    what is wrong with it.  Host work only, no numpy; the numbers themselves are MeshDynamics' to check."""
    import json
    bad = lambda what: SystemExit("edit_sequence: %s: %s" % (path, what))
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError) as e:
        raise bad("cannot read it as JSON (%s)" % e)
    if not isinstance(doc, list) or not all(isinstance(c, dict) for c in doc):
        raise bad('must hold a JSON list of {"kind": "sphere" | "half_space", ...} objects')
    colliders, moving = [], {}
    for i, c in enumerate(doc):
        c = dict(c)
        c.setdefault("friction", friction)
        if c.get("kind") == "sphere" and "centers" in c:
            cs = c.pop("centers")
            if "center" in c or not isinstance(cs, list) or not cs or not all(isinstance(q, list) and len(q) == 3 for q in cs):
                raise bad('collider %d: "centers" must be a list of [x, y, z], at least one, and stands instead of "center"' % i)
            moving[i], c["center"] = cs, cs[0]
        elif c.get("kind") not in ("sphere", "half_space"):
            raise bad('collider %d: "kind" must be "sphere" or "half_space"; got %r' % (i, c.get("kind")))
        colliders.append(c)
    return colliders, moving


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
    source.add_argument("--pick_sequence", type=str, default=None)
    source.add_argument("--pose_sequence", type=str, default=None, metavar="FILE.json")
    parser.add_argument("--skeleton", type=str, default=None, metavar="FILE.json")
    parser.add_argument("--skin_blend", choices=("dqs", "linear"), default=None)
    parser.add_argument("--skin_heat", type=float, default=None, metavar="C")
    parser.add_argument("--skin_influences", type=int, default=None, metavar="K")
    parser.add_argument("--save_meshes", action="store_true", default=False)
    parser.add_argument("--arap_global_step", choices=("column", "grid"), default="column")
    parser.add_argument("--arap_batch", type=int, default=1)
    parser.add_argument("--inbetweens", type=int, default=0)
    parser.add_argument("--ease", choices=("linear", "smoothstep"), default="linear")
    parser.add_argument("--dynamics", action="store_true", default=False)
    parser.add_argument("--settle", type=int, default=0)
    parser.add_argument("--dt", type=float, default=None)
    parser.add_argument("--stiffness", type=float, default=None)
    parser.add_argument("--damping", type=float, default=None)
    parser.add_argument("--gravity", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    parser.add_argument("--floor", type=float, default=None, metavar="H")
    parser.add_argument("--friction", type=float, default=None, metavar="MU")
    parser.add_argument("--contact_stiffness", type=float, default=None, metavar="KC")
    parser.add_argument("--colliders", type=str, default=None, metavar="FILE.json")
    parser.add_argument("--background_contact", type=int, nargs="?", const=128, default=None, metavar="RES")
    parser.add_argument("--contact_margin", type=float, default=None, metavar="M")
    parser.add_argument("--obstacle_mesh", type=str, default=None, metavar="FILE.obj")
    parser.add_argument("--obstacle_resolution", type=int, default=None, metavar="RES")
    parser.add_argument("--obstacle_margin", type=float, default=None, metavar="M")
    parser.add_argument("--obstacle_motion", type=str, default=None, metavar="FILE.json")
    parser.add_argument("--camera_id", type=int, default=None)
    parser.add_argument("--frames_per_launch", type=int, default=4)
    parser.add_argument("--save_maps", action="store_true", default=False)
    parser.add_argument("--save_baked", type=str, default=None)
    parser.add_argument("--background_gaussian", type=str, default=None)
    parser.add_argument("--is_exist_bg", action="store_true", default=False)
    args = parser.parse_args(argv)
    if args.is_exist_bg and args.background_gaussian is None:
        parser.error("--is_exist_bg needs --background_gaussian (the background cloud's PLY)")
    if args.background_gaussian is not None and args.save_maps:
        parser.error("--save_maps: a scene with a background renders no depth / alpha maps; drop --save_maps or the background")
    if not 1 <= args.arap_batch <= ARAP_BATCH_MAX:
        raise SystemExit("edit_sequence: --arap_batch %d: a launch chain carries 1 .. %d frames' solves" % (args.arap_batch, ARAP_BATCH_MAX))
    if args.inbetweens < 0:
        raise SystemExit("edit_sequence: --inbetweens %d: the number of frames between two keys, 0 or more" % args.inbetweens)
    if args.settle < 0:
        raise SystemExit("edit_sequence: --settle %d: the number of steps appended with the handles held, 0 or more" % args.settle)
    if args.pose_sequence is None:
        for flag, value in (("--skeleton", args.skeleton), ("--skin_blend", args.skin_blend), ("--skin_heat", args.skin_heat),
                            ("--skin_influences", args.skin_influences)):
            if value is not None:
                raise SystemExit("edit_sequence: %s belongs to --pose_sequence (a mesh posed from a skeleton) and needs it" % flag)
    else:
        if args.skeleton is None:
            raise SystemExit("edit_sequence: --pose_sequence poses a skeleton and needs --skeleton FILE.json")
        if args.dynamics:
            raise SystemExit("edit_sequence: --dynamics simulates the frames of --handle_sequence / --pick_sequence; --pose_sequence has posed meshes")
        if args.arap_batch > 1:
            raise SystemExit("edit_sequence: --pose_sequence with --arap_batch %d: there is no ARAP solve to batch; drop --arap_batch" % args.arap_batch)
        if args.skin_heat is not None and not 0.0 < args.skin_heat < float("inf"):
            raise SystemExit("edit_sequence: --skin_heat %r: a finite number > 0" % args.skin_heat)
        if args.skin_influences is not None and not 1 <= args.skin_influences <= 4:
            raise SystemExit("edit_sequence: --skin_influences %d: the bones kept per vertex, 1 .. 4" % args.skin_influences)
        pose_rotations, pose_translation = read_pose_sequence(args.pose_sequence)
    if args.settle > 0 and not args.dynamics:
        raise SystemExit("edit_sequence: --settle needs --dynamics (only a simulated mesh has anything to settle)")
    if not args.dynamics:
        for flag, value in (("--dt", args.dt), ("--stiffness", args.stiffness), ("--damping", args.damping), ("--gravity", args.gravity)):
            if value is not None:
                raise SystemExit("edit_sequence: %s sets the simulated material and needs --dynamics" % flag)
        for flag, value in (("--floor", args.floor), ("--friction", args.friction), ("--contact_stiffness", args.contact_stiffness),
                            ("--colliders", args.colliders), ("--background_contact", args.background_contact),
                            ("--obstacle_mesh", args.obstacle_mesh)):
            if value is not None:
                raise SystemExit("edit_sequence: %s sets what the simulated mesh collides with and needs --dynamics" % flag)
    if args.background_contact is not None:
        if args.background_gaussian is None:
            raise SystemExit("edit_sequence: --background_contact collides with the background cloud and needs --background_gaussian")
        if args.background_contact < 2:
            raise SystemExit("edit_sequence: --background_contact %d: the volume's resolution, 2 or more voxels along its longest side" % args.background_contact)
    if args.contact_margin is not None:
        if args.background_contact is None:
            raise SystemExit("edit_sequence: --contact_margin grows the volume of --background_contact and needs it")
        if not 0.0 <= args.contact_margin < float("inf"):
            raise SystemExit("edit_sequence: --contact_margin %r: a finite number >= 0" % args.contact_margin)
    if args.obstacle_mesh is not None and args.background_contact is not None:
        raise SystemExit("edit_sequence: --obstacle_mesh with --background_contact: a simulation takes one volume; drop one of the two")
    for flag, value in (("--obstacle_resolution", args.obstacle_resolution), ("--obstacle_margin", args.obstacle_margin)):
        if value is not None and args.obstacle_mesh is None:
            raise SystemExit("edit_sequence: %s shapes the volume of --obstacle_mesh and needs it" % flag)
    if args.obstacle_motion is not None and args.obstacle_mesh is None:
        raise SystemExit("edit_sequence: --obstacle_motion moves the solid of --obstacle_mesh and needs it")
    obstacle_poses = None if args.obstacle_motion is None or not args.dynamics else read_obstacle_motion(args.obstacle_motion)
    if args.obstacle_mesh is not None and args.dynamics and not os.path.isfile(args.obstacle_mesh):
        raise SystemExit("edit_sequence: --obstacle_mesh %s: no such file" % args.obstacle_mesh)
    if args.obstacle_resolution is not None and args.obstacle_resolution < 2:
        raise SystemExit("edit_sequence: --obstacle_resolution %d: the volume's resolution, 2 or more voxels along its longest side" % args.obstacle_resolution)
    if args.obstacle_margin is not None and not 0.0 <= args.obstacle_margin < float("inf"):
        raise SystemExit("edit_sequence: --obstacle_margin %r: a finite number >= 0" % args.obstacle_margin)
    if args.dynamics:
        if args.mesh_sequence is not None:
            raise SystemExit("edit_sequence: --dynamics simulates the frames of --handle_sequence / --pick_sequence; --mesh_sequence has ready-made meshes")
        if args.arap_batch > 1:
            raise SystemExit("edit_sequence: --dynamics with --arap_batch %d: a simulated step starts from its predecessor; drop --arap_batch" % args.arap_batch)
        if args.inbetweens > 0:
            raise SystemExit("edit_sequence: --dynamics with --inbetweens %d: simulated frames are no key poses; drop one of the two" % args.inbetweens)
        if args.floor is not None and (args.gravity is None or not any(args.gravity)):
            raise SystemExit("edit_sequence: --floor lies opposite to gravity and needs a non-zero --gravity X Y Z")
        if args.friction is not None and args.floor is None and args.colliders is None and args.background_contact is None and args.obstacle_mesh is None:
            raise SystemExit("edit_sequence: --friction is the friction of --floor and --colliders; give one of them")
        if args.contact_stiffness is not None and args.floor is None and args.colliders is None and args.background_contact is None and args.obstacle_mesh is None:
            raise SystemExit("edit_sequence: --contact_stiffness needs something to collide with: --floor or --colliders")
        colliders, moving = ([], {}) if args.colliders is None else read_colliders(args.colliders, args.friction or 0.0)
        if args.floor is not None:
            colliders.append(dict(kind="half_space", normal=[0.0 - g for g in args.gravity], offset=args.floor, friction=args.friction or 0.0))
    if args.pick_sequence is not None:
        pick = read_pick_sequence(args.pick_sequence)
        (pick_camera, pick_handles, pick_anchors, pick_offsets), pick_radii = pick[:4], (pick[4] if len(pick) > 4 else None)

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
    handles = solver = None
    if args.handle_sequence is not None:
        with np.load(args.handle_sequence) as z:
            handles, positions = np.asarray(z["handles"]).reshape(-1), np.asarray(z["positions"], np.float32)
        if positions.ndim != 3 or positions.shape[1:] != (len(handles), 3):
            raise SystemExit("edit_sequence: %s: positions must be [T,%d,3], got %s" % (args.handle_sequence, len(handles), positions.shape))
    if args.pick_sequence is not None:
        from .mesh_pick import screen_offset
        if pick_camera >= len(cams):
            raise SystemExit("edit_sequence: %s: camera_id %d, but %s has %d cameras" % (args.pick_sequence, pick_camera, args.camera_path, len(cams)))
        obj, cam = tool.gaussians_list[-1], cams[pick_camera]
        pixels = np.concatenate([pick_handles, pick_anchors], 0)
        names = ["handle %d" % i for i in range(len(pick_handles))] + ["anchor %d" % i for i in range(len(pick_anchors))]
        handles = obj.pick(cam, pixels)["vertex"].cpu().numpy()                       # resolved once, on the rest mesh
        for i, v in enumerate(handles):
            if v < 0:
                raise SystemExit("edit_sequence: %s: %s at pixel (%g, %g) misses the mesh" % (args.pick_sequence, names[i], pixels[i, 0], pixels[i, 1]))
            if v in handles[:i]:
                raise SystemExit("edit_sequence: %s: %s and %s pick the same vertex %d" % (args.pick_sequence, names[list(handles[:i]).index(v)], names[i], v))
        rest = obj.vertex[torch.as_tensor(handles, device=obj.vertex.device)]
        offsets = torch.as_tensor(pick_offsets, device=rest.device)
        if pick_radii is None:
            positions = [torch.cat([screen_offset(cam, rest[:len(pick_handles)], offsets[t]), rest[len(pick_handles):]], 0) for t in range(len(offsets))]
        else:                                                                         # the picks grown into surface regions
            H = len(pick_handles)
            try:
                solver = obj.set_region_handles(handles[:H], pick_radii[0], pick_radii[1], anchor_vertices=handles[H:])
            except ValueError as e:
                raise SystemExit("edit_sequence: %s: %s" % (args.pick_sequence, e))
            handles = solver.handles
            positions = [obj.region_targets(screen_offset(cam, rest[:H], offsets[t]) - rest[:H]) for t in range(len(offsets))]
    if handles is not None:
        if solver is None:
            solver = tool.gaussians_list[-1].set_handles(handles)
        if args.dynamics:                                                             # one launch chain per 64 steps, no host wait
            obj = tool.gaussians_list[-1]
            pos = torch.stack([torch.as_tensor(p, dtype=torch.float32, device=obj.vertex.device) for p in positions], 0)
            if args.settle > 0:
                pos = torch.cat([pos, pos[-1:].expand(args.settle, -1, -1)], 0)
            material = {k: v for k, v in (("dt", args.dt), ("stiffness", args.stiffness), ("damping", args.damping),
                                          ("gravity", None if args.gravity is None else tuple(args.gravity))) if v is not None}
            rows = poses = None
            if colliders:
                material["colliders"] = colliders
            if args.background_contact is not None:                                   # the background cloud itself, fused from every camera
                material["field"] = tool.background_field(cams, resolution=args.background_contact,
                                                          margin=0.5 if args.contact_margin is None else args.contact_margin)
                material["field_friction"] = args.friction or 0.0
            if args.obstacle_mesh is not None:                                        # a triangle mesh as a static solid
                from .dynamics import SdfGrid
                if obstacle_poses is not None and len(obstacle_poses) != len(pos):
                    raise SystemExit("edit_sequence: --obstacle_motion %s: %d matrices, but the simulation has %d frames"
                                     % (args.obstacle_motion, len(obstacle_poses), len(pos)))
                try:
                    ov, of = read_obj(args.obstacle_mesh)
                    grid = SdfGrid.from_mesh(ov, of, resolution=128 if args.obstacle_resolution is None else args.obstacle_resolution,
                                             margin=0.5 if args.obstacle_margin is None else args.obstacle_margin, device=obj.vertex.device)
                except ValueError as e:
                    raise SystemExit("edit_sequence: --obstacle_mesh %s: %s" % (args.obstacle_mesh, e))
                if obstacle_poses is None:
                    material["field"], material["field_friction"] = grid, args.friction or 0.0
                else:                                                                 # the solid moves: a field with a pose per frame
                    material["fields"], material["field_frictions"], poses = [grid], [args.friction or 0.0], obstacle_poses[:, None]
            if (colliders or args.background_contact is not None or args.obstacle_mesh is not None) and args.contact_stiffness is not None:
                material["contact_stiffness"] = args.contact_stiffness
            if moving:                                                                # the centres of the moving balls, frame by frame
                from .dynamics import collider_table
                try:
                    rows = np.tile(collider_table(colliders, "--colliders")[1], (len(pos), 1, 1))
                    for i, cs in moving.items():
                        c = np.asarray(cs, np.float32)
                        rows[:, i, :3] = c[np.minimum(np.arange(len(pos)), len(c) - 1)]
                except ValueError as e:
                    raise SystemExit("edit_sequence: --colliders: %s" % e)
            try:
                meshes = list(obj.simulate(len(pos), pos, collider_rows=rows, field_poses=poses, **material))
            except ValueError as e:
                raise SystemExit("edit_sequence: --dynamics: %s" % e)
        else:
            # enqueued back to back: no host wait between the solves; --arap_batch frames per launch chain
            meshes = list(solver.solve_sequence(positions, batch=args.arap_batch, global_step=args.arap_global_step))
    if args.pose_sequence is not None:                                                # weights once, then all frames in one skinning launch
        from .skinning import Skeleton
        obj = tool.gaussians_list[-1]
        try:
            skeleton = Skeleton.read(args.skeleton)
        except ValueError as e:
            raise SystemExit("edit_sequence: --skeleton: %s" % e)
        if pose_rotations.shape[1] != skeleton.Nj:
            read_pose_sequence(args.pose_sequence, joints=skeleton.Nj)
        try:
            obj.attach_skeleton(skeleton, heat=1.0 if args.skin_heat is None else args.skin_heat,
                                max_influences=4 if args.skin_influences is None else args.skin_influences)
            meshes = list(obj.pose_sequence(pose_rotations, pose_translation, blend=args.skin_blend or "dqs"))
        except ValueError as e:
            raise SystemExit("edit_sequence: --pose_sequence: %s" % e)
    if args.inbetweens > 0:                                                           # the frames so far are keys; the rest pose is key 0
        from .pose_interp import PoseInterpolator
        obj = tool.gaussians_list[-1]
        keys = [obj.vertex] + [torch.as_tensor(read_obj(m)[0], dtype=torch.float32, device=obj.vertex.device) if isinstance(m, str) else m for m in meshes]
        try:
            meshes = list(PoseInterpolator(obj.vertex, obj.faces, device=obj.vertex.device).sequence(keys, args.inbetweens, ease=args.ease))
        except ValueError as e:
            raise SystemExit("edit_sequence: --inbetweens: %s" % e)
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
    if args.save_baked is not None:
        last = meshes[-1]
        for o in tool.gaussians_list:
            if o.get_name() == args.object_name:
                o.deform_gaussian(last) if isinstance(last, str) else o.deform_vertices(last)
        tool.save_baked(args.save_baked, name=args.object_name)
    return len(frames)


if __name__ == "__main__":
    main()
