"""Depth and semantic snapshots of a scene mesh from virtual cameras, on the GPU — the first step of the pipeline, which the reference does
with an open3d OpenGL window (utils/utils_prox_snapshots_virtualcam.py: ``get_new_cams`` :102-180, ``update_render_cam`` :68-79,
``is_body_occluded`` :342-378, the capture loop :502-541) or with the Habitat simulator, and which a headless GPU node cannot run.

* ``SceneMesh`` / ``SnapshotRenderer``  the mesh on the GPU and the batched render call (csrc/raster.hip through ``ops.raster_render``)
* ``sample_virtual_cams``               the reference's camera lattice around a target point, with its two filters
* ``view_is_usable``                    the reference's occlusion test, negated
* ``write_sensor_folder``               ``cam_%06d.npy`` / ``depth_%06d.npy`` / ``seg_%06d.npy`` as ``generation.TestOP.test_habitat`` reads them

Conventions: ``cam_ext`` is camera-to-world (the matrix the generated pkl files carry and ``verts_transform`` applies); the camera looks
along +z with x right and y down; ``cam_int`` is the 3x3 pinhole matrix.  Rendering needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import os
import warnings

import numpy as np
import torch

from . import ops, scene_io


class SceneMesh:
    """A triangle mesh uploaded once: verts [nv,3], faces [nf,3], vertex_labels [nv] (None: all 0).  Owns the ``psi_raster_mesh`` handle;
    a face index outside [0, nv) is refused by ``psi_raster_mesh_create`` (``PsiHipError``).  One render call at a time per mesh."""

    def __init__(self, verts, faces, vertex_labels=None, device='cuda'):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ops.hip.PsiHipError('SceneMesh needs a GPU device (the HIP rasteriser is the only implementation)')
        as_np = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dt)
        v, f = as_np(verts, np.float32).reshape(-1, 3), as_np(faces, np.int64).reshape(-1, 3)
        if len(f) == 0 or len(v) == 0:
            raise ValueError('empty mesh')
        self.nv, self.nf = len(v), len(f)
        self.verts = torch.tensor(v, device=self.device)
        self.faces = torch.tensor(f.astype(np.int32), device=self.device)
        self.labels = None if vertex_labels is None else torch.tensor(as_np(vertex_labels, np.float32).reshape(self.nv), device=self.device)
        self.handle = ops.raster_mesh_create(self.verts, self.faces, self.labels)

    @classmethod
    def from_ply(cls, path, device='cuda'):
        """Positions, triangles and (when the file has red / green / blue) labels = min(mean(rgb) / 5, 41) of a PLY file."""
        verts, faces, rgb = scene_io.read_ply_mesh(path)
        return cls(verts, faces, None if rgb is None else scene_io.labels_from_colors(rgb), device=device)

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                ops.raster_mesh_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def world_to_camera(cam_ext) -> np.ndarray:
    """[n,3,4] fp32 rows of the inverse of camera-to-world ``cam_ext`` [n,4,4]: inverted in fp64, rounded to fp32 once."""
    ext = np.asarray(cam_ext, dtype=np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.linalg.inv(ext)[:, :3, :], dtype=np.float32)


def intrinsics_rows(cam_int, n) -> np.ndarray:
    """[n,4] fp32 = fx, fy, cx, cy from cam_int [n,3,3] or [3,3]."""
    K = np.asarray(cam_int, dtype=np.float64)
    K = np.broadcast_to(K, (n, 3, 3)) if K.ndim == 2 else K.reshape(n, 3, 3)
    return np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], -1), dtype=np.float32)


class SnapshotRenderer:
    def __init__(self, mesh: SceneMesh):
        self.mesh = mesh
        self.last_stats = None

    def render(self, cam_ext, cam_int, size, near=0.05):
        """All views in one call: cam_ext [n,4,4] camera-to-world, cam_int [n,3,3] or [3,3], size = (H, W).  Returns GPU tensors
        depth [n,H,W] fp32 (0 where nothing is hit, like a depth sensor's hole), seg [n,H,W] fp32 (the interpolated vertex label,
        0 where nothing is hit) and tri [n,H,W] int32 (the triangle index, -1 where nothing is hit)."""
        ext = cam_ext.detach().cpu().numpy() if torch.is_tensor(cam_ext) else cam_ext
        K = cam_int.detach().cpu().numpy() if torch.is_tensor(cam_int) else cam_int
        w2c = world_to_camera(ext)
        dev = self.mesh.device
        depth, tri, seg, stats = ops.raster_render(self.mesh.handle, self.mesh.nf, torch.tensor(w2c, device=dev),
                                                   torch.tensor(intrinsics_rows(K, len(w2c)), device=dev), size, near)
        self.last_stats = stats.cpu().numpy()
        for view in np.nonzero(self.last_stats[:, 1])[0]:
            warnings.warn('view %d: %d triangle pieces project beyond the 2^28 sub-pixel range and were not drawn (a vertex very close to '
                          'the plane z = 0 of the camera?)' % (view, self.last_stats[view, 1]))
        return depth, seg, tri


def look_at(eye, target) -> np.ndarray:
    """Camera-to-world pose [4,4] at ``eye`` whose +z axis points at ``target``, x horizontal (utils_prox_snapshots_virtualcam.py:149-160):
    x = (z1, -z0, 0) / |.|, y = z cross x.  For a camera above its target this is the reference's matrix; the reference's own y column
    divides by z2 and turns into a reflection for a camera below its target, where this one stays a rotation."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.array([z[1], -z[0], 0.0])
    nx = np.linalg.norm(x)
    if nx < 1e-9:
        raise ValueError('the camera looks straight up or down: its x axis is undefined')
    x = x / nx
    y = np.cross(z, x)
    out = np.eye(4)
    out[:3, 0], out[:3, 1], out[:3, 2], out[:3, 3] = x, y / np.linalg.norm(y), z, eye
    return out


def sample_virtual_cams(scene_min, scene_max, target, room_planes=None, grid_nodes=10, noise=0.5, rng=None, return_shifts=False):
    """Camera-to-world poses [n,4,4] fp64 on the reference's lattice around ``target`` (utils_prox_snapshots_virtualcam.py:102-180):

    * positions: ``grid_nodes`` x ``grid_nodes`` nodes over the xy box of the scene times ``grid_nodes // 3`` heights from the target's
      to the ceiling (``scene_max[2]``), border nodes left out;
    * orientation: ``look_at`` the target from the node;
    * then ONE scalar N(0, noise^2) draw per node is added to all three coordinates of the position (the orientation is kept);
    * kept when the shifted position is more than 1.65 m and less than 6.5 m from the target and, with ``room_planes`` [k,2,3] =
      (point, inward normal) per plane, on the inner side of every plane.

    ``rng``: a ``numpy.random.RandomState`` (default: RandomState(0)); one draw per node, kept or not, so a seed fixes the list.
    ``return_shifts``: also return the scalar shift of every kept pose."""
    rng = np.random.RandomState(0) if rng is None else rng
    smin, smax, target = (np.asarray(a, np.float64).reshape(3) for a in (scene_min, scene_max, target))
    nz = grid_nodes // 3
    xs, ys = np.linspace(smin[0], smax[0], grid_nodes), np.linspace(smin[1], smax[1], grid_nodes)
    zs = np.linspace(target[2], smax[2], nz)
    planes = None if room_planes is None else np.asarray(room_planes, np.float64).reshape(-1, 2, 3)
    poses, shifts = [], []
    for iy in range(1, grid_nodes - 1):
        for ix in range(1, grid_nodes - 1):
            for iz in range(1, nz - 1):
                node = np.array([xs[ix], ys[iy], zs[iz]])
                shift = noise * rng.randn()
                try:
                    pose = look_at(node, target)
                except ValueError:
                    continue
                pos = node + shift
                pose[:3, 3] = pos
                dist = np.linalg.norm(pos - target)
                if dist <= 1.65 or dist >= 6.5:
                    continue
                if planes is not None and (((pos[None] - planes[:, 0]) * planes[:, 1]).sum(-1) < 0).any():
                    continue
                poses.append(pose)
                shifts.append(shift)
    out = np.stack(poses) if poses else np.zeros((0, 4, 4))
    return (out, np.array(shifts)) if return_shifts else out


def view_is_usable(depth, target_cam, cam_int) -> bool:
    """The reference's ``is_body_occluded`` (:342-378), negated: the target point (camera coordinates) projects more than 10 pixels inside
    the image, and the mean depth of the 20 x 20 window around its pixel exceeds the target's own depth.  The pixel is
    int(x * fx / z + cx) with the principal point of ``cam_int`` (the reference uses the image centre, its window's principal point)."""
    d = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
    K = np.asarray(cam_int, np.float64).reshape(3, 3)
    x, y, z = (float(c) for c in np.asarray(target_cam, np.float64).reshape(3))
    if z <= 0:
        return False
    h, w = d.shape
    cx, cy = int(x * K[0, 0] / z + K[0, 2]), int(y * K[1, 1] / z + K[1, 2])
    if cx <= 10 or cx > w - 10 or cy <= 10 or cy > h - 10:
        return False
    win = d[max(cy - 10, 0):min(cy + 10, h), max(cx - 10, 0):min(cx + 10, w)]
    return bool(np.mean(win) > z)


def write_sensor_folder(folder, depth, seg, cam_ext, cam_int) -> list:
    """One ``cam_%06d.npy`` (a dict with ``cam_ext`` [4,4], ``cam_int`` [3,3]), ``depth_%06d.npy`` and ``seg_%06d.npy`` per view — the files
    ``TestOP.test_habitat`` globs and loads.  Returns the cam files.  (That loader finds a view's images by replacing 'cam' in the whole
    path, so ``folder`` itself must not contain 'cam'.)"""
    if 'cam' in os.path.abspath(folder):
        raise ValueError("the sensor folder's path must not contain 'cam' (test_habitat derives the depth / seg names by replacing it)")
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    depth, seg, ext = to_np(depth), to_np(seg), to_np(cam_ext).reshape(-1, 4, 4)
    K = to_np(cam_int)
    K = np.broadcast_to(K, (len(ext), 3, 3)) if K.ndim == 2 else K.reshape(len(ext), 3, 3)
    os.makedirs(folder, exist_ok=True)
    files = []
    for i in range(len(ext)):
        fn = os.path.join(folder, 'cam_%06d.npy' % i)
        np.save(fn, {'cam_ext': np.asarray(ext[i], np.float32), 'cam_int': np.asarray(K[i], np.float32)}, allow_pickle=True)
        np.save(os.path.join(folder, 'depth_%06d.npy' % i), np.asarray(depth[i], np.float32))
        np.save(os.path.join(folder, 'seg_%06d.npy' % i), np.asarray(seg[i], np.float32))
        files.append(fn)
    return files
