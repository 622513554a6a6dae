"""File-based edit surface: the classes edit.py drives, with the reference's names and call signatures.

Mirrors edittool/__init__.py of the reference:
  SingleObjectDeform(fg_path, mesh_path, name)      :40-131   load_gaussian / load_mesh (both branches) / deform_gaussian(path)
  SceneVisualTool(bg_gaussian_path)                 :133-231  add_gaussian / deform_one_gaussian / render_gaussian (background
                                                              cloud + objects, eigh -> (scale, quaternion) route) / get_camera
  ObjectVisualTool()                                :378-475  the same without a background (colors_precomp + cov3D_precomp route)
Replaced dependencies: plyfile -> io.read_ply, igl.read_triangle_mesh -> io.read_obj, igl.point_mesh_squared_distance ->
closest_triangles() below, pyACAP.GetRS -> gm_mesh_rs (deform.mesh_rs), Jittor tensor algebra -> the HIP kernels behind
deform.SingleObjectDeform / renderer.  Host-side set-up (parsing, barycentric weights) is numpy, once per object; every
per-frame step runs on the GPU.
"""
import os

import numpy as np
import torch

from . import io as gio
from .deform import SingleObjectDeform as _TensorObject
from . import _lib
from .deform import (barycentric_weights, cov_to_scale_rot, mesh_rs, mesh_rs_packed_batch, pack_cov6, pack_mesh_state, plan_sequence,
                     rest_mesh_state, vertex_face_adjacency)
from .rasterizer import GaussianRasterizationSettings, NewGaussianRasterizer
from .renderer import Camera, camera_work_hint, render_deformed


def _covariance(scaling_raw, rotation_raw):
    """build_covariance_from_scaling_rotation (edittool/mesh_based_gaussian.py:23-27, general_utils.py:39-71):
    L = R(q / |q|) diag(exp(s)), cov = L L^T, full [N,3,3]."""
    s = torch.exp(scaling_raw)
    q = torch.nn.functional.normalize(rotation_raw)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    return L @ L.transpose(1, 2)


def point_mesh_squared_distance(points, vertex, triangles, chunk=4096):
    """igl.point_mesh_squared_distance(P, V, F) -> (sqrD [n], I [n], C [n,3]) (edittool/__init__.py:80): squared distance to,
    index of, and closest point on the closest triangle, exact, brute force in chunks: closest point on each triangle by the
    region test of Ericson, "Real-Time Collision Detection" 5.1.5 (ties go to the lowest face index).  Host side (numpy, float64),
    used once per object and only when the Gaussian file carries no face ids."""
    P = np.asarray(points, np.float64).reshape(-1, 3); V = np.asarray(vertex, np.float64); F = np.asarray(triangles, np.int64)
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    ab, ac = b - a, c - a
    idx = np.zeros(len(P), np.int64); sqr = np.zeros(len(P), np.float64); close = np.zeros((len(P), 3), np.float64)
    for s0 in range(0, len(P), chunk):
        p = P[s0:s0 + chunk][:, None, :]
        ap = p - a
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        bp = p - b
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        cp = p - c
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(divide="ignore", invalid="ignore"):
            denom = 1.0 / (va + vb + vc)
            v_in, w_in = vb * denom, vc * denom
            t_ab = d1 / (d1 - d3); t_ac = d2 / (d2 - d6); t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        q = a + ab * v_in[..., None] + ac * w_in[..., None]                          # interior
        m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0); q = np.where(m[..., None], b + (c - b) * t_bc[..., None], q)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0); q = np.where(m[..., None], a + ac * t_ac[..., None], q)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0); q = np.where(m[..., None], a + ab * t_ab[..., None], q)
        m = (d6 >= 0) & (d5 <= d6); q = np.where(m[..., None], c, q)
        m = (d3 >= 0) & (d4 <= d3); q = np.where(m[..., None], b, q)
        m = (d1 <= 0) & (d2 <= 0); q = np.where(m[..., None], a, q)
        d2all = ((p - q) ** 2).sum(-1)
        k = np.argmin(d2all, axis=1)
        rows = np.arange(len(k))
        idx[s0:s0 + chunk] = k; sqr[s0:s0 + chunk] = d2all[rows, k]; close[s0:s0 + chunk] = q[rows, k]
    return sqr, idx, close


def closest_triangles(points, vertex, triangles, chunk=4096):
    """Index of the closest triangle to each point (point_mesh_squared_distance's second output, edittool/__init__.py:82)."""
    return point_mesh_squared_distance(points, vertex, triangles, chunk)[1]


class SingleObjectDeform(_TensorObject):
    """edittool.SingleObjectDeform(fg_path, mesh_path, name): a mesh-bound Gaussian PLY attached to its proxy mesh (OBJ)."""

    def __init__(self, fg_path, mesh_path, name=None, device="cuda"):
        self.device = torch.device(device)
        self.load_gaussian(fg_path)
        self.load_mesh(mesh_path)
        self.name = mesh_path if name is None else name

    @classmethod
    def from_plain(cls, gaussian_path, mesh_path, name=None, device="cuda"):
        """A PLAIN Gaussian PLY (x y z, f_dc / f_rest, opacity, scale, rot: any 3DGS trainer's point_cloud.ply, bg_model.PlainGaussians.save_ply)
        attached to a proxy mesh (OBJ): every Gaussian is bound to the closest face of the mesh - mesh_bind.bind_points, the search on the
        device (gm_closest_face) - with the weights of the foot of its perpendicular on that face's plane, as load_mesh's no-face-id branch
        forms them.  Positions, covariances, opacities and SH rows as load_gaussian forms them.  The object is then like any other
        (deform_gaussian / deform_vertices, the tools' render_gaussian and render_sequence); it keeps bind_sqr_distance [N] (float32, host),
        the squared distance of every Gaussian to its face: how far off the surface the cloud lies."""
        from .mesh_bind import bind_points
        self = cls.__new__(cls)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GmeshError("SingleObjectDeform.from_plain binds on a HIP (cuda) device; there is no CPU path")
        t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)
        m = gio.load_plain_gaussians(gaussian_path)
        vertex, triangles = gio.read_obj(mesh_path)
        pos = t(m["xyz"])
        cov = _covariance(t(m["scaling"]), t(m["rotation"]))
        opacity = torch.sigmoid(t(m["opacity"]))
        feats = torch.cat([t(m["features_dc"]), t(m["features_rest"])], dim=1).contiguous()
        b = bind_points(pos, vertex, triangles)
        self._loaded = m
        self.gaussian_proj_pos = pos
        self.index_tri = b["face_id"][:, None]
        self.bind_sqr_distance = b["sqr_distance"]
        _TensorObject.__init__(self, pos, cov, opacity, feats, t(b["tri"], torch.int32), t(b["weights"]), t(vertex), name=None)
        self.faces = t(triangles, torch.int32)
        off, adj = vertex_face_adjacency(triangles, vertex.shape[0])
        self._adjacency = (t(off, torch.int32), t(adj, torch.int32))
        self.name = mesh_path if name is None else name
        return self

    def baked_rows(self, deg=3):
        """bake() as the raw (pre-activation) columns of a plain Gaussian PLY, host arrays keyed as io.save_plain_gaussians takes them:
        xyz, features_dc / features_rest (the re-expressed SH rows, split), opacity (the raw column of the loaded file, bit for bit: an
        edit does not touch it), scaling = log(max(scales, 1e-12)) (float32, on the host; the floor keeps a degenerate covariance's zero
        scale finite), rotation = bake()'s unit quaternions."""
        b = self.bake(deg)
        host = lambda t: t.detach().cpu().numpy()
        shs = host(b["shs"])
        return dict(xyz=host(b["xyz"]), features_dc=np.ascontiguousarray(shs[:, :1]), features_rest=np.ascontiguousarray(shs[:, 1:]),
                    opacity=np.asarray(self._loaded["opacity"], np.float32).reshape(-1, 1),
                    scaling=np.log(np.maximum(host(b["scales"]), np.float32(1e-12))), rotation=host(b["rotations"]))

    def save_baked(self, path, deg=3):
        """Write the object in its current state as a plain Gaussian PLY (io.save_plain_gaussians' format, unchanged): what another
        3DGS viewer or trainer opens, and what add_plain_gaussian / load_bg_gaussian read back."""
        gio.save_plain_gaussians(path, self.baked_rows(deg))

    def load_gaussian(self, gaussian_path):
        """:48-64.  The edit tool's loader fills _bc from the saved x, y, z (edittool/mesh_based_gaussian.py:183-184), so
        get_proj_xyz = softmax(xyz) . (v1, v2, v3); positions are the SAVED x, y, z (get_load_xyz)."""
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.device)
        m = gio.load_mesh_gaussians(gaussian_path, bc_from_xyz=True)
        self._loaded = m
        pos = t(m["load_xyz"])
        bc = torch.softmax(t(m["bc"]), dim=1)
        self.gaussian_proj_pos = bc[:, 0:1] * t(m["v1"]) + bc[:, 1:2] * t(m["v2"]) + bc[:, 2:3] * t(m["v3"])
        cov = _covariance(t(m["scaling"]), t(m["rotation"]))
        opacity = torch.sigmoid(t(m["opacity"]))
        feats = torch.cat([t(m["features_dc"]), t(m["features_rest"])], dim=1).contiguous()
        self.index_tri = np.asarray(m["fid"], np.int64) if m.get("fid") is not None else None
        self._pending = (pos, cov, opacity, feats)

    def load_mesh(self, mesh_path):
        """:65-102.  With face ids in the file (always, for files written by the training code): gaussian_triangles =
        F[fid] and the weights are taken at the projected positions; without: closest triangle of the projected position,
        weights at the foot of the perpendicular from the Gaussian onto that triangle's plane."""
        vertex, triangles = gio.read_obj(mesh_path)
        pos, cov, opacity, feats = self._pending
        if self.index_tri is None:
            normals = np.cross(vertex[triangles[:, 1]] - vertex[triangles[:, 0]], vertex[triangles[:, 2]] - vertex[triangles[:, 0]])
            normals /= np.linalg.norm(normals, axis=1)[:, None]
            bias = -(vertex[triangles[:, 0]] * normals).sum(axis=1)
            gpos = pos.cpu().numpy().astype(np.float64)
            index_tri = closest_triangles(self.gaussian_proj_pos.cpu().numpy(), vertex, triangles)
            n_g, b_g = normals[index_tri], bias[index_tri]
            distance = -((n_g * gpos).sum(axis=1) + b_g)
            intersection = gpos + distance[:, None] * n_g
            self.index_tri = index_tri[:, None]
        else:
            intersection = self.gaussian_proj_pos.cpu().numpy().astype(np.float64)
        tri = triangles[self.index_tri.reshape(-1)]
        coord = barycentric_weights(intersection, vertex[tri[:, 0]], vertex[tri[:, 1]], vertex[tri[:, 2]])
        t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)
        super().__init__(pos, cov, opacity, feats, t(tri, torch.int32), t(coord), t(vertex), name=None)
        self.faces = t(triangles, torch.int32)
        off, adj = vertex_face_adjacency(triangles, vertex.shape[0])
        self._adjacency = (t(off, torch.int32), t(adj, torch.int32))
        del self._pending

    def deform_gaussian(self, deform_mesh_path):
        """:103-131: read the deformed mesh, per-vertex (R, S) of the deformation (pyACAP.GetRS there, gm_mesh_rs here),
        then the Gaussian deformation; sets gaussian_deform_pos / gaussian_deform_cov / gaussian_deform_rot."""
        deform_vertex, _ = gio.read_obj(deform_mesh_path)
        # (deform_vertices: the same from a [Vm,3] tensor - an animation loop needs no file per frame; the tensor-in class defines it)
        return self.deform_vertices(torch.as_tensor(deform_vertex, dtype=torch.float32, device=self.device))


class ObjectVisualTool:
    """edittool.ObjectVisualTool (:378-475): objects on a white background, colours from SH with the deformation-rotated
    view direction, colors_precomp + cov3D_precomp into NewGaussianRasterizer."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.gaussians_list = []

    def add_gaussian(self, gaussian_path, mesh_path, name=None):
        self.gaussians_list.append(SingleObjectDeform(gaussian_path, mesh_path, name, device=self.device))

    def add_plain_gaussian(self, gaussian_path, mesh_path, name=None):
        """add_gaussian for a plain Gaussian PLY: bound to the mesh's closest faces on load (SingleObjectDeform.from_plain)."""
        self.gaussians_list.append(SingleObjectDeform.from_plain(gaussian_path, mesh_path, name, device=self.device))

    def deform_one_gaussian(self, name, deform_mesh_path):
        for g in self.gaussians_list:
            if g.get_name() == name:
                g.deform_gaussian(deform_mesh_path)

    def drag_one_gaussian(self, name, vertex_ids, handle_positions, **solve_options):
        """deform_one_gaussian without a mesh file: the objects called `name` get their handle vertices vertex_ids dragged to
        handle_positions [H,3] (SingleObjectDeform.drag: as-rigid-as-possible, warm-started from the object's current mesh).  The
        solver is built on the first call and kept while vertex_ids stay the same."""
        ids = np.asarray(vertex_ids.detach().cpu() if torch.is_tensor(vertex_ids) else vertex_ids).reshape(-1)
        for g in self.gaussians_list:
            if g.get_name() == name:
                if g.arap is None or not np.array_equal(g.arap.handles, ids):
                    g.set_handles(ids)
                g.drag(handle_positions, **solve_options)

    def interpolate_one_gaussian(self, name, target, inbetweens, **options):
        """The in-betweens from the current mesh of the objects called `name` to the mesh `target` [Vm,3]
        (SingleObjectDeform.interpolate_to: rotation-aware, pose_interp.PoseInterpolator); the objects are left at the target.  Returns
        the meshes [inbetweens + 2, Vm, 3] of the last such object (None if there is none)."""
        meshes = None
        for g in self.gaussians_list:
            if g.get_name() == name:
                meshes = g.interpolate_to(target, inbetweens, **options)
        return meshes

    def pose_one_gaussian(self, name, rotations, root_translation=None, blend="dqs", skeleton=None, **weight_options):
        """The objects called `name` posed from a skeleton (SingleObjectDeform.pose_sequence: skinning.SkinBinding): rotations
        [T,Nj,3,3] or [T,Nj,3] axis-angle, root_translation [T,3] or None.  skeleton: a skinning.Skeleton to attach first
        (attach_skeleton, with weight_options); None: the one attached before.  The objects are left at the last pose.  Returns the
        meshes [T,Vm,3] of the last such object (None if there is none)."""
        meshes = None
        for g in self.gaussians_list:
            if g.get_name() == name:
                if skeleton is not None:
                    g.attach_skeleton(skeleton, **weight_options)
                meshes = g.pose_sequence(rotations, root_translation, blend=blend)
        return meshes

    def drag_skeleton_one_gaussian(self, name, vertex_ids, targets, skeleton=None, weight_options=None, **ik_options):
        """The objects called `name` with their picked vertices vertex_ids [H] dragged to targets [H,3] and the skeleton following
        (SingleObjectDeform.drag_skeleton: inverse kinematics through gm_skin_pose_bwd).  skeleton: a skinning.Skeleton to attach first
        (attach_skeleton, with the dict weight_options); None: the one attached before.  ik_options: iterations, damping, blend,
        fit_translation.  Returns (rotations, root_translation, history) of the last such object (None if there is none)."""
        result = None
        for g in self.gaussians_list:
            if g.get_name() == name:
                if skeleton is not None:
                    g.attach_skeleton(skeleton, **(weight_options or {}))
                result = g.drag_skeleton(vertex_ids, targets, **ik_options)
        return result

    def simulate_one_gaussian(self, name, steps, handle_targets=None, collider_rows=None, field_poses=None, **options):
        """`steps` simulated steps of the objects called `name` from their current mesh (SingleObjectDeform.simulate: secondary motion,
        dynamics.MeshDynamics) with their handles at handle_targets [steps,H,3] and, with colliders= among the options, those at
        collider_rows [steps,K,4] (None: where they were built), with field= (a dynamics.SdfGrid, SceneVisualTool.background_field's for
        one) and field_friction= the sampled volume as one more collider, with fields= (object_fields' for one), field_frictions= and
        field_poses [steps,F,3,4] up to four volumes that move rigidly; the objects are left at the last frame.  Returns the
        meshes [steps, Vm, 3] of the last such object (None if there is none)."""
        meshes = None
        for g in self.gaussians_list:
            if g.get_name() == name:
                meshes = g.simulate(steps, handle_targets, collider_rows=collider_rows, field_poses=field_poses, **options)
        return meshes

    def drag_region_one_gaussian(self, name, handle_vertices, displacements, grab_radius, free_radius=None, anchor_vertices=(), **solve_options):
        """drag_one_gaussian with surface regions for handles: on the objects called `name`, everything within grab_radius (along the
        rest mesh) of handle_vertices[i] moves by displacements[i] ([H,3]), everything within grab_radius of an anchor vertex or, with
        free_radius, farther than free_radius from every pick stays at rest (SingleObjectDeform.set_region_handles / drag_region).  The
        regions and the solver are built on the first call and kept while the vertices and radii stay the same."""
        as_ids = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a).reshape(-1)
        key = (tuple(as_ids(handle_vertices).tolist()), tuple(as_ids(anchor_vertices).tolist()), float(grab_radius),
               None if free_radius is None else float(free_radius))
        for g in self.gaussians_list:
            if g.get_name() == name:
                if g.region is None or getattr(g, "_region_key", None) != key:
                    g.set_region_handles(key[0], key[2], key[3], key[1])
                    g._region_key = key
                g.drag_region(displacements, **solve_options)

    def pick_one_gaussian(self, name, camera, pixels):
        """What lies under pixels [P,2] of the camera on the current proxy mesh of the (first) object called `name`
        (SingleObjectDeform.pick): dict(face, vertex, point, depth) on the device; the vertex ids are drag_one_gaussian's."""
        for g in self.gaussians_list:
            if g.get_name() == name:
                return g.pick(camera, pixels)
        raise ValueError("pick_one_gaussian: no object named %r" % (name,))

    def _baked_objects(self, name, deg):
        objs = [g for g in self.gaussians_list if name is None or g.get_name() == name]
        if name is not None and not objs:
            raise ValueError("save_baked: no object named %r" % (name,))
        return [g.baked_rows(deg) for g in objs]

    @staticmethod
    def _write_baked(path, parts):
        if not parts:
            raise ValueError("save_baked: nothing to save")
        gio.save_plain_gaussians(path, {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]})

    def save_baked(self, path, name=None, deg=3):
        """Every object (or the ones called `name`) in its current state, in list order, as ONE plain Gaussian PLY
        (SingleObjectDeform.save_baked's columns, concatenated)."""
        self._write_baked(path, self._baked_objects(name, deg))

    def get_camera(self, path):
        """cameras.json of a model directory -> cameras with the reference's attribute names (:547-584)"""
        return [Camera(c, self.device) for c in gio.load_cameras_json(os.path.join(path, "cameras.json"))]

    def get_single_camera(self, path, id=1):
        return self.get_camera(path)[id]

    def render_gaussian(self, viewpoint_camera):
        return render_deformed(viewpoint_camera, self.gaussians_list)

    # ---- edit sequences: K frames per launch chain (rasterizer.forward_deformed_batch) ----
    def _deformations(self, deformation):
        """A frame's {object name: [Vm,3] vertices / OBJ path} -> {object index: [Vm,3] float32 device tensor}."""
        out = {}
        for name, v in (deformation or {}).items():
            idx = [i for i, o in enumerate(self.gaussians_list) if o.get_name() == name]
            if not idx:
                raise ValueError("render_sequence: no object named %r" % (name,))
            if isinstance(v, (str, os.PathLike)):
                v = gio.read_obj(v)[0]
            v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=torch.float32, device=self.device).contiguous()
            for i in idx:
                if v.shape != self.gaussians_list[i].vertex.shape:
                    raise ValueError("render_sequence: object %r: deformed vertices must be [%d,3]" % (name, self.gaussians_list[i].vertex.shape[0]))
                out[i] = v
        return out

    def _sequence_cloud(self):
        """All objects as ONE static cloud (face ids offset by the preceding objects' vertex counts); rebuilt when gaussians_list changes."""
        objs = tuple(self.gaussians_list)
        c = getattr(self, "_seq_cloud", None)
        if c is not None and len(c["objs"]) == len(objs) and all(a is b for a, b in zip(c["objs"], objs)):
            return c
        cat = lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs, dim=0)
        voff = np.cumsum([0] + [o.vertex.shape[0] for o in objs])
        cov = cat([o.gaussian_cov for o in objs])
        c = dict(objs=objs, voff=[int(v) for v in voff], tables={},
                 tri=cat([o.gaussian_triangles + int(voff[i]) for i, o in enumerate(objs)]).to(torch.int32).contiguous(),
                 weights=cat([o.coord for o in objs]).contiguous(), pos=cat([o.gaussian_pos for o in objs]).contiguous(),
                 shs=cat([o.gaussian_feature for o in objs]).contiguous(), opac=cat([o.gaussian_o for o in objs]).contiguous())
        cov6 = pack_cov6(cov)
        c["cov"] = cov.contiguous() if cov6 is None else cov6
        self._seq_cloud = c
        return c

    def _current_table(self, cloud, i):
        """pack_mesh_state of object i's current state (its last deform(), or its rest pose), cached while that state stands."""
        o = cloud["objs"][i]
        st = o.deform_state
        hit = cloud["tables"].get(i)
        if hit is not None and hit[0] is st:
            return hit[1]
        state = rest_mesh_state(o.vertex) if st is None else torch.cat([st[0], st[1].reshape(-1, 9), st[2].reshape(-1, 9)], dim=1)
        table = pack_mesh_state(state, o.vertex)
        cloud["tables"][i] = (st, table)
        return table

    def gather_tables(self, deformations, cloud=None):
        """The combined gather tables [K, sum Vm, 24] of K frames: per frame, the per-object tables concatenated along the vertex axis -
        deform.mesh_rs_packed_batch of the objects a frame names (one launch per object over the frames), the cached pack_mesh_state of
        the current state for the others.  deformations: K dicts as render_sequence takes them (or None)."""
        cloud = self._sequence_cloud() if cloud is None else cloud
        defs = [self._deformations(d) for d in deformations]
        K, voff = len(defs), cloud["voff"]
        tables = torch.empty((K, voff[-1], 24), dtype=torch.float32, device=self.device)
        for i, o in enumerate(cloud["objs"]):
            rows = tables[:, voff[i]:voff[i + 1]]
            named = [k for k in range(K) if i in defs[k]]
            if named:
                mesh_rs_packed_batch(o.vertex, [defs[k][i] for k in named], o.faces, o._adjacency, out=[rows[k] for k in named])
            if len(named) < K:
                cur = self._current_table(cloud, i)
                for k in range(K):
                    if k not in named:
                        rows[k].copy_(cur)
        return tables

    def render_sequence(self, frames, *, frames_per_launch=4, aux=False, bg_color=None):
        """Render an edit sequence: frames = iterable of (camera, deformation); camera a renderer.Camera or any object with the reference's
        camera attributes, deformation None or {object name: [Vm,3] deformed vertices (tensor / array) or an OBJ path}.  An object a frame
        does not name is rendered in its current state (its last deform_gaussian / deform_vertices / deform, or its rest pose).
        A generator: yields, in input order, image [3,H,W] - with aux (image, depth [1,H,W], alpha [1,H,W]) - on a white background
        by default, as render_gaussian(return_aux=...) would; the tensors belong to the caller.  No object attribute changes.
        Route (deform.plan_sequence): every object in one combined static cloud, frames of one resolution in batches of
        frames_per_launch (1..GM_BATCH_MAX) through rasterizer.forward_deformed_batch - the cloud read once per batch, no host wait per
        frame; batch b + 1 is issued before batch b is checked and yielded.  The first frame of a resolution teaches the workspaces
        their capacity (forward_deformed_begin(...).finish()); a frame that outgrows it is rendered again, exactly; a resolution the
        batch refuses (more than 2048 list tiles) takes the single-frame path.  Forward only."""
        if not 1 <= int(frames_per_launch) <= _lib.GM_BATCH_MAX:
            raise ValueError("frames_per_launch: 1..%d, got %r" % (_lib.GM_BATCH_MAX, frames_per_launch))
        return self._render_sequence(list(frames), int(frames_per_launch), bool(aux), bg_color)

    def _render_sequence(self, frames, K, aux, bg_color):
        from . import rasterizer as Rz
        cloud = self._sequence_cloud()
        bg = self._bg(bg_color)

        def issue_batch(idx, cams, ws, hint):
            W, H = _size(frames[idx[0]][0])
            tables = self.gather_tables([frames[i][1] for i in idx], cloud)
            return Rz.forward_deformed_batch(bg, cloud["tri"], cloud["weights"], list(tables), cloud["cov"], cloud["pos"], cloud["shs"],
                                             cloud["opac"], cams, H, W, 3, ws, image_only=True, work_hint=hint, aux=aux)

        def issue_frame(i, c, workspace):
            W, H = _size(frames[i][0])
            table = self.gather_tables([frames[i][1]], cloud)[0]
            return Rz.forward_deformed_begin(bg, cloud["tri"], cloud["weights"], table, cloud["cov"], cloud["pos"], cloud["shs"], cloud["opac"],
                                             c["view"], c["proj"], c["tanx"], c["tany"], H, W, 3, c["campos"], workspace=workspace, aux=aux)
        yield from _run_plan(frames, K, cloud["pos"].shape[0] > 0, issue_batch, issue_frame, aux, self.device)

    def _bg(self, bg_color):
        return torch.ones(3, device=self.device) if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32, device=self.device)


def _size(c):
    return int(c.image_width), int(c.image_height)


def _run_plan(frames, K, batchable, issue_batch, issue_frame, aux, dev):
    """The route both tools' render_sequence take (deform.plan_sequence): frames of one resolution in batches of K through
    issue_batch(frame indices, cameras, workspaces, work hint) -> K PendingForward, the first frame of a resolution (which teaches the
    workspaces their capacity) and frames the batch refuses through issue_frame(frame index, camera, workspace or None) -> PendingForward.
    Batch b + 1 is issued before batch b is checked and yielded; a frame that outgrew the capacity is rendered again, exactly."""
    import math
    from . import rasterizer as Rz
    sizes = [_size(c) for c, _ in frames]
    plan = plan_sequence(sizes, K, batchable=batchable)
    streams = {}                                   # (W, H) -> workspaces (two batches in flight) + one work hint

    def stream_of(size):
        st = streams.get(size)
        if st is None:
            st = streams[size] = dict(ws=[Rz.RasterWorkspace() for _ in range(2 * K)], hint=Rz.new_work_hint(size[0], size[1], dev), next=0)
        return st

    def cam(c):
        return dict(view=c.world_view_transform, proj=c.full_proj_transform, campos=c.camera_center,
                    tanx=math.tan(c.FoVx * 0.5), tany=math.tan(c.FoVy * 0.5))

    def share_capacity(st):
        cap = max(w.capacity for w in st["ws"])
        for w in st["ws"]:
            w.capacity = cap

    def issue(kind, idx):
        st = stream_of(sizes[idx[0]])
        cams = [cam(frames[i][0]) for i in idx]
        if kind == "batch":
            ws = st["ws"][st["next"]:st["next"] + len(idx)]
            st["next"] = K - st["next"]                     # the other half of the workspaces for the next batch
            return issue_batch(idx, cams, ws, st["hint"]), st
        return [issue_frame(idx[0], cams[0], st["ws"][st["next"]] if kind == "learn" else None)], st

    def complete(kind, hs, st):
        for h in hs:
            if kind == "batch":
                ok, _ = h.check()
                out = h.result if ok else h.finish(image_only=True, work_hint=st["hint"])   # outgrew the capacity: again, exactly
            else:
                out = h.finish(image_only=True, work_hint=st["hint"])
            if kind != "single":
                share_capacity(st)
            yield (out[1], out[6], out[7]) if aux else out[1]

    pending = None
    for kind, idx in plan:
        issued = (kind,) + issue(kind, idx)
        if kind == "learn":                             # complete it now: the next batch needs the capacity it learns
            if pending is not None:
                yield from complete(*pending)
                pending = None
            yield from complete(*issued)
            continue
        if pending is not None:
            yield from complete(*pending)
        pending = issued
    if pending is not None:
        yield from complete(*pending)


class SceneVisualTool(ObjectVisualTool):
    """edittool.SceneVisualTool (:133-231): a free-standing background cloud plus deformed objects.  As in the reference
    the concatenated covariances go through the eigen-decomposition route - (scale, quaternion) from eigh, here on the
    device (gm_cov_to_scale_rot) - and the colours come from the rasterizer's own SH evaluation (`shs`, :209-217)."""

    def __init__(self, bg_gaussian_path=None, device="cuda"):
        super().__init__(device)
        self.load_bg_gaussian(bg_gaussian_path)

    def load_bg_gaussian(self, path):
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.device)
        m = gio.load_plain_gaussians(path)
        self._bg_loaded = m                          # the raw rows, for save_baked(include_background=True)
        self.bg_scale = torch.exp(t(m["scaling"]))
        self.bg_rot = torch.nn.functional.normalize(t(m["rotation"]))
        self.bg_cov3D = _covariance(t(m["scaling"]), t(m["rotation"]))
        self.bg_mean3D = t(m["xyz"])
        self.bg_shs = torch.cat([t(m["features_dc"]), t(m["features_rest"])], dim=1).contiguous()
        self.bg_opacity = torch.sigmoid(t(m["opacity"]))
        self.bg_deform_rot = torch.eye(3, device=self.device).repeat(self.bg_scale.shape[0], 1, 1)
        self._scene_seq = None                       # the static scene cloud of render_sequence: rebuilt from the new background

    def background_field(self, cameras, resolution=128, bounds=None, margin=0.5, fill_holes=None):
        """The background cloud as something the objects can stand on: a dynamics.SdfGrid for MeshDynamics(field=) / simulate(field=)
        (INTEGRATION.md section AC).  The cloud's own depth and opacity maps from `cameras` are fused into a TsdfVolume
        (proxy_mesh.fuse_cloud) of `resolution` voxels along the longest side of bounds = (min, max); by default the box of the objects'
        rest meshes grown on every side by margin times its longest side - contact only matters where the objects can get to.
        fill_holes: True or an iteration count closes what no view saw (TsdfVolume.fill_holes) and the grid is that of the filled pair;
        None: the fused volume as it is, unobserved samples unknown.  The volume is kept as self.background_volume.  Reads the objects'
        boxes (a host wait) when bounds is None.  ValueError with neither bounds nor an object."""
        from .bg_model import PlainGaussians
        from .dynamics import SdfGrid
        from .proxy_mesh import fuse_cloud
        if bounds is None:
            if not self.gaussians_list:
                raise ValueError("SceneVisualTool.background_field: no object to take the bounds from; give bounds=(min, max)")
            if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not 0.0 <= margin < float("inf"):
                raise ValueError("SceneVisualTool.background_field: margin = %r; a finite number >= 0" % (margin,))
            lo = torch.stack([o.vertex.min(dim=0).values for o in self.gaussians_list]).min(dim=0).values.cpu().numpy().astype(np.float64)
            hi = torch.stack([o.vertex.max(dim=0).values for o in self.gaussians_list]).max(dim=0).values.cpu().numpy().astype(np.float64)
            grow = float(margin) * max(float((hi - lo).max()), 1e-6)
            bounds = (lo - grow, hi + grow)
        m = self._bg_loaded
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
        feats = torch.cat([t(m["features_dc"]), t(m["features_rest"])], dim=1)
        degree = int(round(feats.shape[1] ** 0.5)) - 1
        pc = PlainGaussians(sh_degree=degree, device=self.device)
        pc._set_params(t(m["xyz"]), feats, t(m["scaling"]), t(m["rotation"]), t(m["opacity"]).reshape(-1, 1))
        pc.active_sh_degree = degree
        vol = fuse_cloud(pc, cameras, resolution=int(resolution), bounds=bounds)
        if fill_holes is not None and fill_holes is not False:
            vol.fill_holes(None if fill_holes is True else int(fill_holes))
        self.background_volume = vol
        return SdfGrid.from_tsdf(vol)

    def object_field(self, names, resolution=128, bounds=None, margin=0.5):
        """Objects of the scene as obstacles of another: one dynamics.SdfGrid for simulate(field=) of an object that is not among
        `names` (INTEGRATION.md section AD).  The source is the CURRENT, deformed proxy mesh of every object called one of `names` (a
        name or a sequence of names); each becomes signed distances on one shared lattice (mesh_sdf.grid_values) and the grid is their
        minimum: the union of the solids.  bounds = (min, max), by default the box of those meshes grown on every side by margin times
        its longest side; `resolution` voxels along the bounds' longest side (background_field's rules).  The grid is static: it shows
        the obstacles as they are now.  Reads the meshes on the host.  ValueError for no names, a name no object has, and what
        mesh_sdf.box_lattice refuses."""
        from .dynamics import SdfGrid
        from .mesh_sdf import box_lattice, grid_values
        who = "SceneVisualTool.object_field"
        names = [names] if isinstance(names, str) else list(names)
        if not names:
            raise ValueError("%s: no object named" % who)
        meshes = []
        for n in names:
            found = [o for o in self.gaussians_list if o.get_name() == n]
            if not found:
                raise ValueError("%s: no object named %r" % (who, n))
            for o in found:
                current = o.mesh_vertex_current
                meshes.append(((o.vertex if current is None else current).detach().cpu().numpy().astype(np.float32), o.faces.cpu().numpy()))
        lo = np.min([v.min(axis=0) for v, _ in meshes], axis=0)
        hi = np.max([v.max(axis=0) for v, _ in meshes], axis=0)
        origin, voxel, shape = box_lattice(who, lo, hi, resolution, bounds, margin)
        values = None
        for v, f in meshes:
            phi = grid_values(v, f, origin, voxel, shape, device=self.device)
            values = phi if values is None else torch.minimum(values, phi)
        return SdfGrid(values, origin, voxel, device=values.device)

    def object_fields(self, names, resolution=128, margin=0.5):
        """Objects of the scene as obstacles that MOVE: one dynamics.SdfGrid per name, in the order of `names`, for simulate(fields=)
        of an object that is not among them (INTEGRATION.md section AG).  Each grid is sampled at the REST mesh of the objects called
        that name, on a lattice of its own (that mesh's box grown by margin times its longest side, `resolution` voxels along the
        longest side), so the pose (R | t) that field_poses gives it is the one that carries the rest mesh to where the object is:
        dynamics.rigid_poses(rest, frames).  Reads the meshes on the host.  ValueError for no names, more than
        GM_MESH_FIELDS_MAX, a name no object has, and what mesh_sdf.box_lattice refuses."""
        from . import _lib
        from .dynamics import SdfGrid
        from .mesh_sdf import box_lattice, grid_values
        who = "SceneVisualTool.object_fields"
        names = [names] if isinstance(names, str) else list(names)
        if not names or len(names) > _lib.GM_MESH_FIELDS_MAX:
            raise ValueError("%s: %d objects named (1 .. %d)" % (who, len(names), _lib.GM_MESH_FIELDS_MAX))
        grids = []
        for n in names:
            found = [o for o in self.gaussians_list if o.get_name() == n]
            if not found:
                raise ValueError("%s: no object named %r" % (who, n))
            meshes = [(o.vertex.detach().cpu().numpy().astype(np.float32), o.faces.cpu().numpy()) for o in found]
            lo = np.min([v.min(axis=0) for v, _ in meshes], axis=0)
            hi = np.max([v.max(axis=0) for v, _ in meshes], axis=0)
            origin, voxel, shape = box_lattice(who, lo, hi, resolution, None, margin)
            values = None
            for v, f in meshes:
                phi = grid_values(v, f, origin, voxel, shape, device=self.device)
                values = phi if values is None else torch.minimum(values, phi)
            grids.append(SdfGrid(values, origin, voxel, device=values.device))
        return grids

    def save_baked(self, path, name=None, deg=3, include_background=False):
        """ObjectVisualTool.save_baked for a scene; with include_background the background's raw rows come first, bit for bit as loaded:
        the whole edited scene as one plain Gaussian PLY."""
        keys = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
        bg = [{k: np.asarray(self._bg_loaded[k], np.float32) for k in keys}] if include_background else []
        self._write_baked(path, bg + self._baked_objects(name, deg))

    def render_sequence(self, frames, *, frames_per_launch=4, aux=False, bg_color=None):
        """ObjectVisualTool.render_sequence for a scene: each frame equals, bit for bit, render_gaussian with the objects the frame names
        deformed for that frame (the others in their current state).  Route: the background and every object as ONE static cloud in
        render_gaussian's row order, with the (scale, rotation) of each row's resting covariance computed once; frames of one resolution in
        batches of frames_per_launch through rasterizer.forward_scene_batch, which deforms (and decomposes) only the rows of the objects a
        frame moves - the objects it names and those in a deformed current state.  The first frame of a resolution goes through the
        single-frame path (render_gaussian's arithmetic) and teaches the workspaces their capacity.  No object attribute changes.  No depth
        / alpha maps (aux=True raises GmeshError)."""
        if aux:
            raise _lib.GmeshError("SceneVisualTool.render_sequence renders no depth / alpha maps")
        if not 1 <= int(frames_per_launch) <= _lib.GM_BATCH_MAX:
            raise ValueError("frames_per_launch: 1..%d, got %r" % (_lib.GM_BATCH_MAX, frames_per_launch))
        return self._scene_sequence(list(frames), int(frames_per_launch), bg_color)

    def _scene_cloud(self):
        """The static scene cloud: background rows then each object's rows (render_gaussian's order), every row's position (the objects'
        rest positions), SH row, opacity and the (scale, rotation) of its resting covariance; the objects' face ids (offset into the
        combined gather table), weights and rest covariances.  Rebuilt when gaussians_list changes or load_bg_gaussian runs."""
        objs = tuple(self.gaussians_list)
        c = getattr(self, "_scene_seq", None)
        if c is not None and len(c["objs"]) == len(objs) and all(a is b for a, b in zip(c["objs"], objs)):
            return c
        if len(objs) > _lib.GM_SCENE_OBJECTS_MAX:
            raise _lib.GmeshError("SceneVisualTool.render_sequence: at most %d objects" % _lib.GM_SCENE_OBJECTS_MAX)
        cat = lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs, dim=0)
        voff = np.cumsum([0] + [o.vertex.shape[0] for o in objs])
        rows = np.cumsum([self.bg_mean3D.shape[0]] + [o.gaussian_pos.shape[0] for o in objs])
        scales, rots = cov_to_scale_rot(cat([self.bg_cov3D] + [o.gaussian_cov for o in objs]))
        c = dict(objs=objs, voff=[int(v) for v in voff], rows=[int(r) for r in rows], tables={}, scales=scales, rots=rots,
                 pos=cat([self.bg_mean3D] + [o.gaussian_pos for o in objs]).contiguous(),
                 shs=cat([self.bg_shs] + [o.gaussian_feature for o in objs]).contiguous(),
                 opac=cat([self.bg_opacity] + [o.gaussian_o for o in objs]).reshape(-1).contiguous(),
                 tri=None, weights=None, cov=None)
        if objs:
            c["tri"] = cat([o.gaussian_triangles + int(voff[i]) for i, o in enumerate(objs)]).to(torch.int32).contiguous()
            c["weights"] = cat([o.coord for o in objs]).contiguous()
            c["cov"] = cat([o.gaussian_cov.reshape(-1, 9) for o in objs]).contiguous()
        self._scene_seq = c
        return c

    def _frame_rows(self, defs):
        """means3D, scales, rotations of one frame as render_gaussian computes them, the objects in defs deformed by mesh_rs + deform
        (SingleObjectDeform.deform_vertices) without touching the objects: the single-frame path of render_sequence."""
        from .deform import deform_tensors
        pos, cov = [self.bg_mean3D], [self.bg_cov3D]
        for i, o in enumerate(self.gaussians_list):
            if i in defs:
                R, S = mesh_rs(o.vertex, defs[i], o.faces, adjacency=o._adjacency)
                p, c, _, _ = deform_tensors(o.gaussian_triangles, o.coord, defs[i] - o.vertex, R.reshape(-1, 3, 3), S.reshape(-1, 3, 3),
                                            o.gaussian_cov, o.gaussian_pos)
            else:
                p, c = o.gaussian_deform_pos, o.gaussian_deform_cov
            pos.append(p); cov.append(c)
        s, q = cov_to_scale_rot(torch.cat(cov, dim=0))
        return torch.cat(pos, dim=0), s, q

    def _scene_sequence(self, frames, K, bg_color):
        from . import rasterizer as Rz
        cloud = self._scene_cloud()
        bg = self._bg(bg_color)
        objs = cloud["objs"]

        def issue_batch(idx, cams, ws, hint):
            W, H = _size(frames[idx[0]][0])
            defs = [self._deformations(frames[i][1]) for i in idx]
            masks = [sum(1 << j for j, o in enumerate(objs) if j in d or o.deform_state is not None) for d in defs]
            tables = [None] * len(idx)
            if any(masks):
                tables = list(self.gather_tables([frames[i][1] for i in idx], cloud))
            return Rz.forward_scene_batch(bg, cloud["rows"], masks, cloud["pos"], cloud["scales"], cloud["rots"], cloud["shs"], cloud["opac"],
                                          cloud["tri"], cloud["weights"], cloud["cov"], [t if m else None for t, m in zip(tables, masks)], cams,
                                          H, W, 3, ws, image_only=True, work_hint=hint)

        def issue_frame(i, c, workspace):
            W, H = _size(frames[i][0])
            means3D, s, q = self._frame_rows(self._deformations(frames[i][1]))
            return Rz.rasterize_forward_begin(bg, means3D, None, cloud["opac"], s, q, 1, None, c["view"], c["proj"], c["tanx"], c["tany"], H, W,
                                              cloud["shs"], 3, c["campos"], False, False, workspace=workspace, force_M=16)
        yield from _run_plan(frames, K, cloud["pos"].shape[0] > 0, issue_batch, issue_frame, False, self.device)

    def render_gaussian(self, viewpoint_camera, bg_color=None):
        import math
        c = viewpoint_camera
        objs = self.gaussians_list
        means3D = torch.cat([self.bg_mean3D] + [o.gaussian_deform_pos for o in objs], dim=0)
        shs = torch.cat([self.bg_shs] + [o.gaussian_feature for o in objs], dim=0)
        cov = torch.cat([self.bg_cov3D] + [o.gaussian_deform_cov for o in objs], dim=0)
        opacity = torch.cat([self.bg_opacity] + [o.gaussian_o for o in objs], dim=0)
        new_s, new_q = cov_to_scale_rot(cov)
        rs = GaussianRasterizationSettings(int(c.image_height), int(c.image_width), math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5),
                                           torch.ones(3, device=self.device) if bg_color is None else bg_color, 1, c.world_view_transform,
                                           c.full_proj_transform, 3,
                                           c.camera_center, False, False, camera_work_hint(c, self.device))
        image, _ = NewGaussianRasterizer(rs)(means3D=means3D, means2D=torch.zeros_like(means3D), shs=shs, colors_precomp=None,
                                             opacities=opacity, scales=new_s, rotations=new_q, cov3D_precomp=None)
        return image
