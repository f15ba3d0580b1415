"""From a scene mesh to what the fitting loop and the plausibility table need from a scene: the signed distance volume ({scene}.json +
{scene}_sdf.npy) and the scene point cloud (scenes_downsampled/{scene}.ply).  The reference ships both as downloads and has no code that
makes them; here the volume comes from the mesh on the GPU (csrc/mesh_sdf.hip through ``ops.mesh_sdf_compute``; DESIGN.md "Mesh -> SDF
volume" states the contract).

* ``MeshSDF``          the mesh on the GPU: welded, zero-area triangles dropped, pseudonormals; ``compute`` returns a volume
* ``scene_cloud``      the welded vertex positions, optionally one per occupied voxel (NumPy, on the host)
* ``surface_cloud``    points ON the surface, about one per ``spacing`` cell whatever the tessellation (csrc/mesh_cloud.hip through
                       ``ops.mesh_cloud``): for CAD, synthetic and decimated meshes, whose vertices say little
                       about where their floors and walls are
* ``orient_faces``     the faces wound so that every triangle faces free space, from one point known to be free (csrc/mesh_orient.hip
                       through ``ops.flood_fill`` and ``ops.mesh_orient_votes``): for meshes with mixed winding
* ``scene_from_mesh``  both, as the ``synth.SceneData`` that ``FittingOP(scene=...)``, ``scenes=[...]`` and ``write_prox_layout`` take

Convention: triangles face free space, so free space is positive and solid is negative — what the collision term and
``psi_lbs_sdf_counts`` assume.  With the default ``sign='pseudonormal'`` an open or non-manifold mesh gets its sign from the orientation
of the nearest triangle, and two coincident, oppositely oriented surfaces (a box standing exactly on the floor) leave the sign below them
ambiguous.  ``sign='winding'`` takes the sign from the generalised winding number instead (csrc/mesh_winding.hip, DESIGN.md
"Winding-number sign"), which is robust to both.  Computing needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

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
                    exterior='solid', beta=3.0, cloud='vertices', spacing=None, orient_seeds=None) -> synth.SceneData:
    """The ``synth.SceneData`` of a scene mesh: ``sdf`` [D,D,D] computed on the GPU over the mesh's box grown by ``margin`` on every side,
    ``verts`` = ``scene_cloud(verts, voxel)``.  ``FittingOP(scene=...)``, ``scenes=[...]`` and ``SceneData.write_prox_layout`` take it as
    is.  The several-scenes engine refuses D % 4 != 0 and D > 480: the same ``ValueError`` is raised here, before any work, unless
    ``check_engine=False``.  ``sign``, ``exterior`` and ``beta`` are those of ``MeshSDF.compute``.  ``cloud='surface'`` with a ``spacing``
    puts ``surface_cloud(verts, faces, spacing)`` into ``verts`` instead (``voxel`` then is a ``ValueError``: it thins vertices).
    ``orient_seeds`` [n,3], points known to lie in free space: the faces go through ``orient_faces(verts, faces, orient_seeds)`` first."""
    dim = int(dim)
    check_cloud_args(cloud, voxel, spacing)
    if check_engine:
        check_engine_dim(dim)
    if not margin >= 0:
        raise ValueError('margin must not be negative')
    if sign not in SIGNS or exterior not in LEVELS:
        raise ValueError("sign is 'pseudonormal' or 'winding', exterior is 'solid' or 'free'")
    if orient_seeds is not None:
        faces = orient_faces(verts, faces, orient_seeds, device=device).faces
    mesh = MeshSDF(verts, faces, device=device)
    lo, hi = grid_box(verts, margin)
    sdf = mesh.compute(lo, hi, dim, sign=sign, exterior=exterior, beta=beta).cpu().numpy()
    points = scene_cloud(verts, voxel) if cloud == 'vertices' else surface_cloud(verts, faces, spacing, device=device)
    return synth.SceneData(points, sdf, lo, hi, dim, dict(contact_parts or {}))


# ---- orienting a mesh towards free space ----
DECIDED_BY_VOTE, DECIDED_BY_PROPAGATION, UNDECIDED, ZERO_AREA = 0, 1, -1, -2


@dataclass
class OrientResult:
    faces: np.ndarray        # the input's dtype and shape; columns 1 and 2 swapped where ``flipped``
    flipped: np.ndarray      # [nf] bool
    votes: np.ndarray        # [nf,2] int32: samples whose front / back probe reached a free node
    decided_by: np.ndarray   # [nf] int8: 0 vote, 1 propagation, -1 undecided, -2 zero area
    free_nodes: int          # free nodes of the grid
    rounds: int              # launches of the flood fill up to and including the first that gained nothing


def _orient_mesh(verts, faces):
    as_np = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dt)
    v, f = as_np(verts, np.float32).reshape(-1, 3), as_np(faces, np.int64).reshape(-1, 3)
    if len(f) == 0 or len(v) == 0:
        raise ValueError('empty mesh')
    if f.min() < 0 or f.max() >= len(v):
        raise ops.hip.PsiHipError('a face index lies outside [0, nv)')
    return v, f


def _free_space(v, f, seeds, dim, margin, device):
    """(free [D,D,D] bool on the device, grid_min, grid_max, h fp32, rounds) of a mesh already checked by ``_orient_mesh``."""
    dim = int(dim)
    if dim < ops.FLOOD_MIN_EDGE or dim > ops.FLOOD_MAX_EDGE:
        raise ValueError('dim = %d: an edge of the grid lies in %d .. %d' % (dim, ops.FLOOD_MIN_EDGE, ops.FLOOD_MAX_EDGE))
    if not margin >= 0:
        raise ValueError('margin must not be negative')
    p = np.asarray(seeds, dtype=np.float32).reshape(-1, 3)
    if len(p) == 0:
        raise ValueError('at least one seed: a point known to lie in free space')
    lo, hi = grid_box(v, margin)
    step = (hi - lo) / np.float32(dim - 1)
    if not (step > 0).all():
        raise ValueError('the mesh is flat along an axis: pass a margin')
    with np.errstate(invalid='ignore'):
        node = np.rint((p - lo[None]) / step[None])
    for i in range(len(p)):
        if not ((node[i] >= 0) & (node[i] <= dim - 1)).all():
            raise ValueError('seed %d = %r lies outside the grid %r .. %r' % (i, p[i].tolist(), lo.tolist(), hi.tolist()))
    h = step.max()
    mesh = MeshSDF(v, f, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                            # only the magnitude is used: an open mesh is no concern here
        U = mesh.compute(lo, hi, dim, sign='pseudonormal').abs_()
    open_mask = U > float(np.float32(0.5) * h)
    try:
        free, rounds = ops.flood_fill(open_mask, node.astype(np.int64), return_rounds=True)
    except ValueError as e:
        msg = str(e)
        if 'is not open' in msg:
            i = int(msg.split()[1].rstrip(':'))
            raise ValueError('seed %d = %r lies on a node that is not open: within %g of the surface' % (i, p[i].tolist(), 0.5 * h)) from None
        raise
    return free, lo, hi, h, rounds


def free_space(verts, faces, seeds, dim=128, margin=0.0, device='cuda'):
    """(free [D,D,D] bool on the device, grid_min, grid_max): the nodes of the grid ``grid_box(verts, margin)`` with ``dim`` nodes per axis
    that a point could reach from one of ``seeds`` [n,3] without coming within half a node spacing of the surface.
    ``ValueError``: a seed outside the grid or on a node that is not open (the message names it), ``dim`` outside 2 .. 1024."""
    v, f = _orient_mesh(verts, faces)
    free, lo, hi, _, _ = _free_space(v, f, seeds, dim, margin, device)
    return free, lo, hi


def _edge_pairs(v, f, with_area):
    """(t, u, consistent) of every ordered pair of triangles with area that share an edge no third one uses; positions identify vertices."""
    _, inv = np.unique((v + np.float32(0.0)).view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    tri = np.nonzero(with_area)[0]
    W = inv.reshape(-1)[f[tri]]
    a, b = W.reshape(-1), np.roll(W, -1, axis=1).reshape(-1)        # edge k of a triangle runs from corner k to corner k + 1
    t = np.repeat(tri, 3)
    key = np.minimum(a, b) * (int(W.max()) + 1) + np.maximum(a, b)
    order = np.argsort(key, kind='stable')
    key, t, fwd = key[order], t[order], (a < b)[order]
    start = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
    count = np.diff(np.r_[start, len(key)])
    i = start[count == 2]
    i = i[t[i] != t[i + 1]]
    same = fwd[i] != fwd[i + 1]                                    # opposite directions along the edge: consistently wound
    return np.r_[t[i], t[i + 1]], np.r_[t[i + 1], t[i]], np.r_[same, same]


def _propagate(v, f, flip, by):
    t, u, same = _edge_pairs(v, f, by != ZERO_AREA)
    flip, by = flip.copy(), by.copy()
    level = by == DECIDED_BY_VOTE
    while level.any():
        k = np.nonzero(level[t] & (by[u] == UNDECIDED))[0]
        if not len(k):
            break
        k = k[np.lexsort((t[k], u[k]))]                             # per undecided triangle its neighbours of this level, lowest index first
        k = k[np.r_[True, u[k][1:] != u[k][:-1]]]
        flip[u[k]] = np.where(same[k], flip[t[k]], ~flip[t[k]])
        by[u[k]] = DECIDED_BY_PROPAGATION
        level = np.zeros(len(by), bool)
        level[u[k]] = True
    return flip, by


def _with_area(v, f):
    """[nf] bool: the fp32 length of (b - a) x (c - a), with the association of csrc/mesh_orient.hip, is > 0."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = b - a, c - a
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2]) > 0


def orient_samples(verts, faces, h, device='cuda'):
    """(points [n,3] fp32, tri [n] int32) on the device: where ``orient_faces`` probes a mesh at node spacing ``h``.  The centroid
    ((a + b) + c) / 3 of every triangle with area, then ``surface_cloud_device(verts, faces, spacing=h)``: a floor of two triangles is
    probed everywhere, not once."""
    dev = torch.device(device)
    v, f = _orient_mesh(verts, faces)
    with_area = _with_area(v, f)
    centre = (((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / np.float32(3))[with_area]
    cloud_p, cloud_t = surface_cloud_device(torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev), float(h), device=dev)
    return (torch.cat([torch.from_numpy(centre).to(dev), cloud_p]).contiguous(),
            torch.cat([torch.from_numpy(np.nonzero(with_area)[0].astype(np.int32)).to(dev), cloud_t]).contiguous())


def orient_faces(verts, faces, seeds, dim=128, margin=0.0, ratio=4, propagate=True, device='cuda') -> OrientResult:
    """The faces with every triangle wound so that its normal (b - a) x (c - a) points into free space, given ``seeds`` [n,3]: points known
    to be free (one is enough).  The rule is DESIGN.md section 10c: nodes farther than half a spacing from the surface are open, the open
    nodes connected to a seed are free (``free_space``), every triangle is probed 1.5 spacings in front of and behind its centroid and
    its ``surface_cloud`` samples, and a side wins with ``ratio`` times the votes of the other; triangles the votes leave undecided take
    their orientation from decided neighbours across edges shared by exactly two triangles (``propagate``).  What is still undecided, and
    triangles without area, stay as they are and are counted in ``decided_by``.  Bit-identical from run to run."""
    if not ratio >= 1:
        raise ValueError('ratio must be at least 1')
    dev = torch.device(device)
    v, f = _orient_mesh(verts, faces)
    free, lo, hi, h, rounds = _free_space(v, f, seeds, dim, margin, dev)
    with_area = _with_area(v, f)
    if not with_area.any():
        raise ValueError('no triangle with area')
    dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
    points, tri = orient_samples(v, f, h, device=dev)
    votes = ops.mesh_orient_votes(points, tri, dv, df, free, lo, hi, float(np.float32(1.5) * h)).cpu().numpy()
    F, B = votes[:, 0].astype(np.int64), votes[:, 1].astype(np.int64)
    keep = (F > 0) & (F >= ratio * B)
    flip = (B > 0) & (B >= ratio * F) & ~keep
    by = np.full(len(f), UNDECIDED, np.int8)
    by[keep | flip] = DECIDED_BY_VOTE
    by[~with_area] = ZERO_AREA
    flip &= with_area
    if propagate:
        flip, by = _propagate(v, f, flip, by)
    flip &= by >= 0
    src = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    out = np.array(src, copy=True)
    rows = out.reshape(-1, 3)
    rows[flip] = rows[flip][:, [0, 2, 1]]
    return OrientResult(out, flip, votes, by, int(free.sum().item()), int(rounds))
