"""From a scene mesh to what the fitting loop and the plausibility table need from a scene: the signed distance volume ({scene}.json +
{scene}_sdf.npy) and the scene point cloud (scenes_downsampled/{scene}.ply).  The reference ships both as downloads and has no code that
makes them; here the volume comes from the mesh on the GPU (csrc/mesh_sdf.hip through ``ops.mesh_sdf_compute``; DESIGN.md "Mesh -> SDF
volume" states the contract).

* ``MeshSDF``          the mesh on the GPU: welded, zero-area triangles dropped, pseudonormals; ``compute`` returns a volume
* ``scene_cloud``      the welded vertex positions, optionally one per occupied voxel (NumPy, on the host)
* ``surface_cloud``    points ON the surface, about one per ``spacing`` cell whatever the tessellation (csrc/mesh_cloud.hip through
                       ``ops.mesh_cloud``): for CAD, synthetic and decimated meshes, whose vertices say little
                       about where their floors and walls are
* ``scene_from_mesh``  both, as the ``synth.SceneData`` that ``FittingOP(scene=...)``, ``scenes=[...]`` and ``write_prox_layout`` take

Convention: triangles face free space, so free space is positive and solid is negative — what the collision term and
``psi_lbs_sdf_counts`` assume.  With the default ``sign='pseudonormal'`` an open or non-manifold mesh gets its sign from the orientation
of the nearest triangle, and two coincident, oppositely oriented surfaces (a box standing exactly on the floor) leave the sign below them
ambiguous.  ``sign='winding'`` takes the sign from the generalised winding number instead (csrc/mesh_winding.hip, DESIGN.md
"Winding-number sign"), which is robust to both.  Computing needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import ops, scene_io, synth

MODES = {'grid': 0, 'brute': 1}
SIGNS = ('pseudonormal', 'winding')
LEVELS = {'solid': 0.5, 'free': -0.5}      # a node is solid iff its free-space winding number is below the level
ENGINE_MAX_DIM = 480       # the fitting engine samples a cell-major copy of the volume: D % 4 == 0, D <= PSI_SDF_CELLS_MAX_D (csrc/sdf_device.h)


class MeshSDF:
    """A triangle mesh prepared for distance queries: verts [nv,3], faces [nf,3].  Owns the ``psi_mesh_sdf`` handle.  ``info`` =
    (kept triangles, dropped zero-area triangles, welded vertices, edges not shared by exactly two triangles).  A face index out of range,
    a non-finite vertex and a mesh without a triangle of non-zero area are refused (``PsiHipError``)."""

    def __init__(self, verts, faces, device='cuda'):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ops.hip.PsiHipError('MeshSDF needs a GPU device (the HIP kernel is the only implementation)')
        as_np = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dt)
        v, f = as_np(verts, np.float32).reshape(-1, 3), as_np(faces, np.int64).reshape(-1, 3)
        if len(f) == 0 or len(v) == 0:
            raise ValueError('empty mesh')
        if np.abs(f).max() >= 2 ** 31:
            raise ops.hip.PsiHipError('a face index lies outside [0, nv)')
        self.nv, self.nf = len(v), len(f)
        self.handle = None
        self.handle = ops.mesh_sdf_create(torch.tensor(v, device=self.device), torch.tensor(f.astype(np.int32), device=self.device))
        self.info = ops.mesh_sdf_info(self.handle)
        self._warned = False

    @classmethod
    def from_ply(cls, path, device='cuda'):
        verts, faces, _ = scene_io.read_ply_mesh(path)
        return cls(verts, faces, device=device)

    def winding(self, grid_min, grid_max, dim, beta=3.0, cluster=64):
        """The free-space winding number f [D,D,D] fp32 on the GPU at the nodes of ``compute``: 1 in the free space of a closed room whose
        triangles face free space, 0 inside furniture and outside the room, in between near the holes of an open mesh.  ``beta`` = 0 sums
        every triangle at every node; ``beta`` > 0 replaces clusters of ``cluster`` triangles that lie farther than beta x their radius
        from an 8 x 8 x 8 brick of nodes by their dipoles."""
        return ops.mesh_winding_compute(self.handle, grid_min, grid_max, dim, beta, cluster, device=self.device)

    def compute(self, grid_min, grid_max, dim, mode='grid', sign='pseudonormal', exterior='solid', beta=3.0, cluster=64):
        """The volume [D,D,D] fp32 on the GPU, element [ix][iy][iz]; node i of axis a lies at
        grid_min[a] + i * ((grid_max[a] - grid_min[a]) / (D - 1)).  ``mode``: 'grid' (pruned search) or 'brute' (every node against every
        triangle; the same bits, for checking).  ``sign``: 'pseudonormal' (of the nearest feature: exact for a closed, consistently
        oriented mesh) or 'winding' (the same magnitudes, negative where ``winding(..., beta, cluster)`` is below the level: 0.5 with
        ``exterior='solid'``, a room, what lies behind its walls is solid; -0.5 with ``exterior='free'``, objects standing in open space)."""
        if mode not in MODES:
            raise ValueError("mode is 'grid' or 'brute'")
        if sign not in SIGNS:
            raise ValueError("sign is 'pseudonormal' or 'winding'")
        if exterior not in LEVELS:
            raise ValueError("exterior is 'solid' or 'free'")
        if sign == 'winding':
            f = self.winding(grid_min, grid_max, dim, beta, cluster)
            vol = ops.mesh_sdf_compute(self.handle, grid_min, grid_max, dim, MODES[mode], device=self.device)
            return ops.mesh_sdf_apply_sign(f, LEVELS[exterior], vol)
        if self.info[3] > 0 and not self._warned:
            self._warned = True
            warnings.warn('mesh is not closed: the sign follows the triangle orientation (%d edges are not shared by exactly two triangles)'
                          % self.info[3])
        return ops.mesh_sdf_compute(self.handle, grid_min, grid_max, dim, MODES[mode], device=self.device)

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                ops.mesh_sdf_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def scene_cloud(verts, voxel=None) -> np.ndarray:
    """The welded vertex positions [m,3] fp32 (one per distinct position, -0.0 equal to +0.0, in the order of first appearance).  With
    ``voxel`` the first of them, in that order, of every occupied cell of a ``voxel``-sized lattice anchored at the cloud's minimum: the
    role of scenes_downsampled/*.ply."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3) + np.float32(0.0)
    _, first = np.unique(v.view(np.uint32).reshape(-1, 3), axis=0, return_index=True)
    v = v[np.sort(first)]
    if voxel is None:
        return v
    if not voxel > 0:
        raise ValueError('voxel must be positive')
    cell = np.floor((v.astype(np.float64) - v.min(0).astype(np.float64)) / float(voxel)).astype(np.int64)
    _, first = np.unique(cell, axis=0, return_index=True)
    return v[np.sort(first)]


def surface_cloud_device(verts, faces, spacing, device='cuda'):
    """``surface_cloud`` with both results left on the GPU: (points [m,3] fp32, tri [m] int32).  ``verts`` and ``faces`` are arrays or
    tensors on any device; tensors that already lie on ``device`` as fp32 / int32 are used as they are."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ops.hip.PsiHipError('surface_cloud needs a GPU device (the HIP kernels are the only implementation)')
    if not (spacing is not None and float(spacing) > 0 and np.isfinite(float(spacing))):
        raise ValueError('spacing must be positive and finite')
    v = verts if torch.is_tensor(verts) else torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64))
    v, f = v.reshape(-1, 3), f.reshape(-1, 3)
    if f.numel() == 0 or v.numel() == 0:
        raise ValueError('empty mesh')
    if f.dtype != torch.int32:
        if int(f.abs().max()) >= 2 ** 31:
            raise ops.hip.PsiHipError('a face index lies outside [0, nv)')
        f = f.to(torch.int32)
    return ops.mesh_cloud(v.to(dev, torch.float32).contiguous(), f.to(dev).contiguous(), float(spacing))


def surface_cloud(verts, faces, spacing, device='cuda', return_tri=False):
    """Points on the surface of the mesh, [m,3] fp32 (NumPy, like ``scene_cloud``): about one per cell of a ``spacing``-sized lattice,
    the candidate of a row-by-row sampling of every triangle that lies nearest to the cell's centre, so the density follows the area and
    not the tessellation; every surface point is within 2.3 x ``spacing`` of one (measured: within about one ``spacing``).  Deterministic
    and computed on the GPU.  ``faces`` are the caller's, unwelded: with ``return_tri`` the face index of every point comes along
    ([m] int32), which gives access to normals, labels and colours.  A mesh with more than 2^31 - 1 candidates at this spacing is a
    ``ValueError``."""
    points, tri = surface_cloud_device(verts, faces, spacing, device=device)
    points = points.cpu().numpy()
    return (points, tri.cpu().numpy()) if return_tri else points


CLOUDS = ('vertices', 'surface')


def check_cloud_args(cloud, voxel, spacing):
    """The argument rules of ``scene_from_mesh``'s two clouds (``ValueError``), checked before any work."""
    if cloud not in CLOUDS:
        raise ValueError("cloud is 'vertices' or 'surface'")
    if cloud == 'surface':
        if voxel is not None:
            raise ValueError("voxel thins the vertex cloud: with cloud='surface' pass spacing instead")
        if spacing is None or not (float(spacing) > 0 and np.isfinite(float(spacing))):
            raise ValueError("cloud='surface' needs a positive, finite spacing")
    elif spacing is not None:
        raise ValueError("spacing belongs to cloud='surface'")


def check_engine_dim(dim):
    if dim % 4 != 0 or dim > ENGINE_MAX_DIM or dim < 4:
        raise ValueError('dim = %d: the fitting engine needs a multiple of 4, at most %d (pass check_engine=False for a volume that is '
                         'only sampled elsewhere)' % (dim, ENGINE_MAX_DIM))


def grid_box(verts, margin):
    """(grid_min, grid_max) fp32: the box of the vertices grown by ``margin`` on every side."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    return (v.min(0) - np.float32(margin)).astype(np.float32), (v.max(0) + np.float32(margin)).astype(np.float32)


def scene_from_mesh(verts, faces, dim=256, margin=0.5, voxel=None, contact_parts=None, check_engine=True, device='cuda', sign='pseudonormal',
                    exterior='solid', beta=3.0, cloud='vertices', spacing=None) -> synth.SceneData:
    """The ``synth.SceneData`` of a scene mesh: ``sdf`` [D,D,D] computed on the GPU over the mesh's box grown by ``margin`` on every side,
    ``verts`` = ``scene_cloud(verts, voxel)``.  ``FittingOP(scene=...)``, ``scenes=[...]`` and ``SceneData.write_prox_layout`` take it as
    is.  The several-scenes engine refuses D % 4 != 0 and D > 480: the same ``ValueError`` is raised here, before any work, unless
    ``check_engine=False``.  ``sign``, ``exterior`` and ``beta`` are those of ``MeshSDF.compute``.  ``cloud='surface'`` with a ``spacing``
    puts ``surface_cloud(verts, faces, spacing)`` into ``verts`` instead (``voxel`` then is a ``ValueError``: it thins vertices)."""
    dim = int(dim)
    check_cloud_args(cloud, voxel, spacing)
    if check_engine:
        check_engine_dim(dim)
    if not margin >= 0:
        raise ValueError('margin must not be negative')
    if sign not in SIGNS or exterior not in LEVELS:
        raise ValueError("sign is 'pseudonormal' or 'winding', exterior is 'solid' or 'free'")
    mesh = MeshSDF(verts, faces, device=device)
    lo, hi = grid_box(verts, margin)
    sdf = mesh.compute(lo, hi, dim, sign=sign, exterior=exterior, beta=beta).cpu().numpy()
    points = scene_cloud(verts, voxel) if cloud == 'vertices' else surface_cloud(verts, faces, spacing, device=device)
    return synth.SceneData(points, sdf, lo, hi, dim, dict(contact_parts or {}))
