"""Depth and semantic snapshots of a scene mesh from virtual cameras, on the GPU — the first step of the pipeline, which the reference does
with an open3d OpenGL window (utils/utils_prox_snapshots_virtualcam.py: ``get_new_cams`` :102-180, ``update_render_cam`` :68-79,
``is_body_occluded`` :342-378, the capture loop :502-541) or with the Habitat simulator, and which a headless GPU node cannot run.

* ``SceneMesh`` / ``SnapshotRenderer``  the mesh on the GPU and the batched render call (csrc/raster.hip through ``ops.raster_render``)
* ``sample_virtual_cams``               the reference's camera lattice around a target point, with its two filters
* ``view_is_usable``                    the reference's occlusion test, negated
* ``write_sensor_folder``               ``cam_%06d.npy`` / ``depth_%06d.npy`` / ``seg_%06d.npy`` as ``generation.TestOP.test_habitat`` reads them
* ``ResultRenderer`` / ``write_png``    generated bodies drawn, shaded, into the snapshots of their scene (csrc/raster_bodies.hip): the images the
                                        reference captures from its window in utils/utils_show_test_results.py, and per body the pixels it
                                        covers and the pixels of those that the scene does not hide

Conventions: ``cam_ext`` is camera-to-world (the matrix the generated pkl files carry and ``verts_transform`` applies); the camera looks
along +z with x right and y down; ``cam_int`` is the 3x3 pinhole matrix.  Rendering needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import collections
import os
import struct
import warnings
import zlib

import numpy as np
import torch

from . import ops, scene_io


class SceneMesh:
    """A triangle mesh uploaded once: verts [nv,3], faces [nf,3], vertex_labels [nv] (None: all 0).  Owns the ``psi_raster_mesh`` handle;
    a face index outside [0, nv) is refused by ``psi_raster_mesh_create`` (``PsiHipError``).  One render call at a time per mesh.
    ``vertex_rgb`` [nv,3] (uint8 0..255, or floats in [0,1]) are kept as ``rgb`` [nv,3] fp32 in [0,1] for the result images (None: grey)."""

    def __init__(self, verts, faces, vertex_labels=None, device='cuda', vertex_rgb=None):
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
        self.rgb = None
        if vertex_rgb is not None:
            c = vertex_rgb.detach().cpu().numpy() if torch.is_tensor(vertex_rgb) else np.asarray(vertex_rgb)
            scale = np.float32(255.0) if c.dtype == np.uint8 else np.float32(1.0)
            self.rgb = torch.tensor(np.ascontiguousarray(c.reshape(self.nv, 3), dtype=np.float32) / scale, device=self.device)
        self.handle = ops.raster_mesh_create(self.verts, self.faces, self.labels)

    @classmethod
    def from_ply(cls, path, device='cuda'):
        """Positions, triangles and (when the file has red / green / blue) labels = min(mean(rgb) / 5, 41) of a PLY file."""
        verts, faces, rgb = scene_io.read_ply_mesh(path)
        return cls(verts, faces, None if rgb is None else scene_io.labels_from_colors(rgb), device=device, vertex_rgb=rgb)


def world_to_camera(cam_ext) -> np.ndarray:
    """[n,3,4] fp32 rows of the inverse of camera-to-world ``cam_ext`` [n,4,4]: inverted in fp64, rounded to fp32 once."""
    ext = np.asarray(cam_ext, dtype=np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.linalg.inv(ext)[:, :3, :], dtype=np.float32)


def intrinsics_rows(cam_int, n) -> np.ndarray:
    """[n,4] fp32 = fx, fy, cx, cy from cam_int [n,3,3] or [3,3]."""
    K = np.asarray(cam_int, dtype=np.float64)
    K = np.broadcast_to(K, (n, 3, 3)) if K.ndim == 2 else K.reshape(n, 3, 3)
    return np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], -1), dtype=np.float32)


def camera_rows(cam_ext, cam_int, device):
    """The cameras as the rasterisers take them: ``world_to_camera`` [n,3,4] and ``intrinsics_rows`` [n,4], uploaded to ``device``."""
    ext = cam_ext.detach().cpu().numpy() if torch.is_tensor(cam_ext) else cam_ext
    K = cam_int.detach().cpu().numpy() if torch.is_tensor(cam_int) else cam_int
    w2c = world_to_camera(ext)
    return torch.tensor(w2c, device=device), torch.tensor(intrinsics_rows(K, len(w2c)), device=device)


class SnapshotRenderer:
    def __init__(self, mesh: SceneMesh):
        self.mesh = mesh
        self.last_stats = None

    def render(self, cam_ext, cam_int, size, near=0.05):
        """All views in one call: cam_ext [n,4,4] camera-to-world, cam_int [n,3,3] or [3,3], size = (H, W).  Returns GPU tensors
        depth [n,H,W] fp32 (0 where nothing is hit, like a depth sensor's hole), seg [n,H,W] fp32 (the interpolated vertex label,
        0 where nothing is hit) and tri [n,H,W] int32 (the triangle index, -1 where nothing is hit)."""
        return self._render_rows(*camera_rows(cam_ext, cam_int, self.mesh.device), size, near)

    def _render_rows(self, w2c, intr, size, near):
        """``render`` with the cameras as ``camera_rows`` prepares them (``ResultRenderer.render`` makes them once for both of its calls)."""
        depth, tri, seg, stats = ops.raster_render(self.mesh.handle, self.mesh.nf, w2c, intr, size, near)
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


# ------------------------------------------------------------------------------------------
# Result images: bodies in their scene
# ------------------------------------------------------------------------------------------
RESULT_WORKSPACE_BUDGET = 256 << 20     # bytes: ``draws_per_pass=None`` takes the most draws per pass whose workspace stays below this
BODY_RGB = (0.85, 0.62, 0.5)            # the colour of a draw that is given none

ResultImages = collections.namedtuple('ResultImages', 'rgb depth draw body_depth body_id counts')
ResultImages.__doc__ = """Device tensors of one ``ResultRenderer.render`` call: rgb [n,H,W,3] uint8; depth [n,H,W] fp32, the z of whoever owns
the pixel (0: background); draw [n,H,W] int32, the draw whose body owns the pixel (-1: scene or background); body_depth / body_id [n,H,W], the
nearest body triangle alone (z and draw * F + face; 0 / -1); counts [M,2] int32 = per draw (pixels its body covers in front of the other
bodies, those of them the scene does not hide)."""


class ResultRenderer:
    """Bodies of one topology drawn into the snapshots of ``scene_mesh`` (a ``SceneMesh``, or None: bodies over the background).
    ``body_faces`` [F,3]; a face index outside [0, V) is refused when the first bodies arrive (V is theirs).  One call at a time."""

    def __init__(self, scene_mesh, body_faces, device=None):
        self.scene = scene_mesh
        self.device = torch.device(device) if device is not None else (scene_mesh.device if scene_mesh is not None else torch.device('cuda'))
        if self.device.type != 'cuda':
            raise ops.hip.PsiHipError('ResultRenderer needs a GPU device (the HIP rasteriser is the only implementation)')
        f = body_faces.detach().cpu().numpy() if torch.is_tensor(body_faces) else np.asarray(body_faces)
        self.faces = torch.tensor(np.ascontiguousarray(f.reshape(-1, 3), dtype=np.int32), device=self.device)
        self.F = self.faces.shape[0]
        if self.F == 0:
            raise ValueError('no body faces')
        self.V, self.handle = None, None
        self.snapshots = SnapshotRenderer(scene_mesh) if scene_mesh is not None else None
        self.last_stats = None

    def _bodies(self, body_verts):
        if not torch.is_tensor(body_verts) or not body_verts.is_cuda:
            raise ValueError('body vertices must be a GPU tensor [B,V,3] (they come from the skinning kernel; there is no CPU path)')
        if body_verts.dim() != 3 or body_verts.shape[2] != 3:
            raise ValueError('expected body vertices [B,V,3]')
        bv = body_verts.detach().to(self.device, torch.float32).contiguous()
        if self.handle is None:
            try:
                self.handle = ops.raster_bodies_create(self.faces, bv.shape[1])
            except ops.hip.PsiHipError as e:
                raise ValueError(str(e))
            self.V = bv.shape[1]
        if bv.shape[1] != self.V:
            raise ValueError('bodies of %d vertices after bodies of %d: a ResultRenderer draws one topology' % (bv.shape[1], self.V))
        return bv

    def normals(self, body_verts):
        """[B,V,3] fp32 unnormalised vertex normals, as the shading uses them: per vertex the sum, in ascending face index, of its faces'
        (v1 - v0) x (v2 - v0); zeros for a vertex that no face lists."""
        bv = self._bodies(body_verts)
        return ops.raster_bodies_normals(self.handle, self.V, bv)

    def pick_draws_per_pass(self, M, n_views, size):
        """The most draws per pass (at most M) whose workspace stays below ``RESULT_WORKSPACE_BUDGET``; at least 1."""
        H, W = int(size[0]), int(size[1])
        fixed = ops.raster_bodies_workspace_bytes(self.F, 1, n_views, W, H)
        per_draw = ops.raster_bodies_workspace_bytes(self.F, 2, n_views, W, H) - fixed
        return int(max(1, min(max(M, 1), 1 + (RESULT_WORKSPACE_BUDGET - fixed) // max(per_draw, 1), (2 ** 30 - 1) // self.F)))

    def render(self, body_verts, cam_ext, cam_int, size, draw_body=None, draw_view=None, body_rgb=None, near=0.05, background=(1, 1, 1),
               draws_per_pass=None):
        """body_verts [B,V,3] world-frame GPU tensor; cameras and size as ``SnapshotRenderer.render``.  Draw i shows body draw_body[i] in view
        draw_view[i] with the colour body_rgb[i] ([M,3] or one colour for all, in [0,1]); by default draw i is (body i, view i), the
        reference's cam1 picture, which needs B == n.  Returns ``ResultImages``."""
        bv = self._bodies(body_verts)
        t_w2c, t_intr = camera_rows(cam_ext, cam_int, self.device)
        n, B, dev = len(t_w2c), bv.shape[0], self.device
        if (draw_body is None) != (draw_view is None):
            raise ValueError('draw_body and draw_view come together')
        if draw_body is None:
            if B != n:
                raise ValueError('%d bodies and %d views: without draw_body / draw_view, draw i is (body i, view i)' % (B, n))
            draw_body = draw_view = np.arange(B)
        db, dv = (np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.int64).reshape(-1) for a in (draw_body, draw_view))
        if len(db) != len(dv):
            raise ValueError('draw_body and draw_view differ in length')
        M = len(db)
        if M and (db.min() < 0 or db.max() >= B or dv.min() < 0 or dv.max() >= n):
            raise ValueError('a draw names a body outside [0, %d) or a view outside [0, %d)' % (B, n))
        if M * self.F >= 2 ** 31:
            raise ValueError('%d draws of %d faces: draw * F + face must stay below 2^31' % (M, self.F))
        rgb = np.broadcast_to(np.asarray(BODY_RGB if body_rgb is None else (body_rgb.detach().cpu().numpy() if torch.is_tensor(body_rgb) else body_rgb),
                                         dtype=np.float32), (M, 3))
        if draws_per_pass is None:
            draws_per_pass = self.pick_draws_per_pass(M, n, size)
        scene = {}
        if self.scene is not None:
            sdepth, _, stri = self.snapshots._render_rows(t_w2c, t_intr, size, near)
            scene = dict(scene=self.scene.handle, vrgb=self.scene.rgb, sdepth=sdepth, stri=stri)
        out = ops.raster_bodies_render(self.handle, self.V, self.F, bv, torch.tensor(db, dtype=torch.int32, device=dev),
                                       torch.tensor(dv, dtype=torch.int32, device=dev), torch.tensor(np.ascontiguousarray(rgb), device=dev), t_w2c,
                                       t_intr, size, near, background, draws_per_pass, **scene)
        self.last_stats = out[6].cpu().numpy()
        for view in np.nonzero(self.last_stats[:, 1])[0]:
            warnings.warn('view %d: %d body triangle pieces project beyond the 2^28 sub-pixel range and were not drawn' % (view, self.last_stats[view, 1]))
        return ResultImages(*out[:6])


def write_png(path, rgb_uint8):
    """An [H,W,3] uint8 image (array or tensor) as an 8-bit RGB PNG: one zlib stream, every row with filter 0."""
    img = rgb_uint8.detach().cpu().numpy() if torch.is_tensor(rgb_uint8) else np.asarray(rgb_uint8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('expected an [H,W,3] uint8 image')
    H, W = img.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(img).reshape(H, W * 3)], axis=1)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)

    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(rows.tobytes(), 6))
                + chunk(b'IEND', b''))
