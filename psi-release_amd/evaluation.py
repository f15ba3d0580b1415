"""Physical-plausibility and diversity metrics of generated / fitted bodies.

Plausibility: utils/utils_eval_collision_habitat.py:91-175 — per body: ``non-collision score`` = #(sdf > 0) / 10475 and
``contact score`` = 1 if any vertex has sdf < 0 else 0 (with the all-outside convention: collision 1.0, contact 0).
Same SMPL-X + SDF path as fitting (HIP operators), Habitat camera flip (:160-165).  ``scores`` / ``eval_folder`` score one pkl at a
time through the operators; ``scores_many`` / ``eval_folder_batched`` / ``evaluate_scenes`` score whole folders with one fused
skin + sign-count launch per chunk of bodies (psi_lbs_sdf_counts) and one device -> host copy.

Body against body: ``BodyOverlap.depths`` and ``.penetration_loss`` say how deep the vertices stand and push the bodies apart (psi_body_depth_*,
DESIGN.md section 10f), ``select_shallow`` keeps a set of bodies no deeper in each other than a tolerance.
Body against body: ``BodyOverlap`` counts, per ordered pair of a batch, the vertices of one body inside the other (psi_body_overlap_*,
DESIGN.md section 10d), and ``select_disjoint`` picks a greedy set of bodies that do not stand in each other; the reference has no
counterpart on the path (its BodyInterpenetration needs an external CUDA package).  ``SurfaceCrossings`` lists the pairs of triangles of
the bodies' surfaces that intersect, between bodies and within one body (psi_surface_crossings_*), with
``face_parts`` / ``part_skip_matrix`` for that class's body-part filter and ``select_uncrossed`` for the greedy choice.
Body against the room's mesh: ``SceneCrossings`` lists the pairs of a body triangle and a scene triangle that intersect, with no distance
volume (psi_scene_crossings_*), and ``select_clear`` keeps the bodies that stand clear.

Diversity: utils/utils_eval_diversity.py:93-104 — ``diversity_reference`` runs the reference's ``scipy.cluster.vq.kmeans`` protocol
on the GPU (psi_kmeans_*, psi_vq); ``diversity_scores`` is the older k-means++ variant (a different algorithm, kept as it is).
"""
from __future__ import annotations

import os
import pickle

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import hip, ops
from .geometry import BodyParamParser, GeometryTransformer


class PlausibilityEvaluator:
    def __init__(self, fitting_op, flip_camera_yz=True):
        """``fitting_op``: a FittingOP (supplies vposer, body model, scene SDF on the GPU)."""
        self.op = fitting_op
        self.flip = flip_camera_yz

    @torch.no_grad()
    def scores(self, body_param_input):
        """(non-collision score, contact score) of one pkl.  The reference scores ONE body per file (batch_size 1,
        utils_eval_collision_habitat.py:145-175); a pkl that holds B > 1 bodies gives two lists with one entry per body."""
        op = self.op
        xh, cam_ext, _ = BodyParamParser.body_params_parse_fitting(body_param_input)
        B = xh.shape[0]
        cam = cam_ext
        if self.flip:
            T_mat = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], device=op.device)).unsqueeze(0)
            cam = torch.matmul(cam_ext[:1], T_mat).expand(B, -1, -1).contiguous()
        xh_rec = GeometryTransformer.convert_to_3D_rot(GeometryTransformer.convert_to_6D_rot(xh))
        verts = op.body_verts(xh_rec, cam)
        sdf = ops.sdf_sample(verts, op.s_sdf, op.s_grid_min_batch, op.s_grid_max_batch, align_corners=op.align_corners)
        V = verts.shape[1]
        n_neg = (sdf < 0).sum(dim=1).cpu().tolist()
        n_pos = (sdf > 0).sum(dim=1).cpu().tolist()
        coll, cont = [], []
        for neg, pos in zip(n_neg, n_pos):
            if neg < 1:                                     # utils_eval_collision_habitat.py:131-135: nothing penetrates
                coll.append(10475.0 / 10475.0)
                cont.append(0.0)
            else:
                coll.append(float(pos) / 10475.0)           # :137,139 (the reference hard-codes the SMPL-X vertex count)
                cont.append(1.0)
        return (coll[0], cont[0]) if B == 1 else (coll, cont)

    def eval_folder(self, folder, max_files=8000):
        coll, cont = [], []
        for ii in range(max_files):
            fn = os.path.join(folder, 'body_gen_{:06d}.pkl'.format(ii))
            if not os.path.exists(fn):
                continue
            with open(fn, 'rb') as f:
                c, k = self.scores(pickle.load(f))
            coll.extend(c if isinstance(c, list) else [c])
            cont.extend(k if isinstance(k, list) else [k])
        return coll, cont


    # ---- batched path: psi_lbs_sdf_counts ------------------------------------------------------------------------------------
    def _volumes(self):
        op = self.op
        return op.s_sdf, op.s_grid_min_batch.reshape(-1, 3), op.s_grid_max_batch.reshape(-1, 3)

    @staticmethod
    def _scores_from_counts(counts):
        """counts [N,2] (host, integers) -> (non-collision, contact) float64 [N], formed exactly as ``scores`` forms them."""
        neg, pos = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
        hit = neg >= 1
        coll = np.where(hit, pos.astype(np.float64) / 10475.0, 10475.0 / 10475.0)
        cont = np.where(hit, 1.0, 0.0)
        return coll, cont

    @torch.no_grad()
    def scores_many(self, xh72, cam_ext, scene_id=None, chunk=512, volumes=None):
        """(non-collision scores, contact scores), two float64 arrays [N], of N bodies ``xh72`` [N,72] with cameras ``cam_ext``
        [N,4,4] or [1,4,4] (the pkl's, before the Habitat flip).  One batched 6D round trip and VPoser decode for all N, the fused
        skin + SDF sign count in chunks of ``chunk`` bodies, ONE device -> host copy.  ``scene_id`` [N] selects the volume per body
        when the evaluator holds several (``evaluate_scenes``)."""
        op = self.op
        dev = op.device
        xh = torch.as_tensor(xh72, dtype=torch.float32, device=dev).reshape(-1, 72)
        cam = torch.as_tensor(cam_ext, dtype=torch.float32, device=dev).reshape(-1, 4, 4)
        N = xh.shape[0]
        if cam.shape[0] not in (1, N):
            raise ValueError('scores_many: cam_ext must be [%d,4,4] or [1,4,4], got %s' % (N, tuple(cam.shape)))
        if chunk < 1:
            raise ValueError('scores_many: chunk must be >= 1')
        if N == 0:
            return np.zeros(0), np.zeros(0)
        if self.flip:
            T_mat = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], device=dev)).unsqueeze(0)
            cam = torch.matmul(cam, T_mat)
        cam = cam.expand(N, 4, 4).contiguous()
        sdf, gmin, gmax = volumes if volumes is not None else self._volumes()
        if scene_id is not None:
            scene_id = torch.as_tensor(scene_id, device=dev).to(torch.int32).reshape(N)
        xh_rec = GeometryTransformer.convert_to_3D_rot(GeometryTransformer.convert_to_6D_rot(xh))
        par = BodyParamParser.body_params_encapsulate_batch(xh_rec)
        par['body_pose'] = op.vposer.decode(par.pop('body_pose_vp'), output_type='aa').view(N, -1)
        counts = torch.empty(N, 2, dtype=torch.int32, device=dev)
        for lo in range(0, N, chunk):
            hi = min(N, lo + chunk)
            counts[lo:hi] = op.body_mesh_model.sdf_counts(sdf, gmin, gmax, scene_id=None if scene_id is None else scene_id[lo:hi],
                                                          align_corners=op.align_corners, cam_ext=cam[lo:hi],
                                                          **{k: v[lo:hi] for k, v in par.items()})
        return self._scores_from_counts(counts.cpu().numpy())

    @staticmethod
    def _read_folder(folder, max_files):
        """(xh72 [N,72], cam_ext [N,4,4]) of the pkls of a folder, host arrays; a pkl of B bodies gives B rows with its first camera."""
        xs, cams = [], []
        for ii in range(max_files):
            fn = os.path.join(folder, 'body_gen_{:06d}.pkl'.format(ii))
            if not os.path.exists(fn):
                continue
            with open(fn, 'rb') as f:
                rec = pickle.load(f)
            x = np.asarray(BodyParamParser._vector(rec), dtype=np.float32).reshape(-1, 72)
            c = np.asarray(rec['cam_ext'], dtype=np.float32).reshape(-1, 4, 4)[:1]
            xs.append(x)
            cams.append(np.repeat(c, x.shape[0], axis=0))
        if not xs:
            return np.zeros((0, 72), np.float32), np.zeros((0, 4, 4), np.float32)
        return np.concatenate(xs), np.concatenate(cams)

    def eval_folder_batched(self, folder, max_files=8000, chunk=512):
        """The two lists ``eval_folder`` returns, through ``scores_many``."""
        xh, cam = self._read_folder(folder, max_files)
        coll, cont = self.scores_many(xh, cam, chunk=chunk)
        return coll.tolist(), cont.tolist()

    @classmethod
    def evaluate_scenes(cls, ops_by_scene, gen_path, flip_camera_yz=True, max_files=8000, chunk=512):
        """Several scenes in one pass.  ``ops_by_scene``: ordered mapping (or list of pairs) scene name -> FittingOP; the bodies of
        scene ``name`` are the pkls of ``gen_path/name``.  The volumes are stacked [S,D,D,D] (all scenes must share D) and every body
        carries its ``scene_id``; VPoser and body model are the first op's.  Returns ``{name: (coll list, cont list)}`` in the order given."""
        items = list(ops_by_scene.items()) if hasattr(ops_by_scene, 'items') else list(ops_by_scene)
        if not items:
            return {}
        Ds = [tuple(op.s_sdf.shape[1:]) for _, op in items]
        if any(d != Ds[0] for d in Ds):
            raise ValueError('evaluate_scenes: all scenes must share the SDF resolution D, got %s' % (Ds,))
        if any(bool(op.align_corners) != bool(items[0][1].align_corners) for _, op in items):
            raise ValueError('evaluate_scenes: all scenes must share align_corners')
        ev = cls(items[0][1], flip_camera_yz=flip_camera_yz)
        vols = (torch.cat([op.s_sdf.reshape(1, *Ds[0]) for _, op in items]).contiguous(),
                torch.cat([op.s_grid_min_batch.reshape(1, 3) for _, op in items]).contiguous(),
                torch.cat([op.s_grid_max_batch.reshape(1, 3) for _, op in items]).contiguous())
        xs, cams, sids = [], [], []
        for si, (name, _) in enumerate(items):
            x, c = cls._read_folder(os.path.join(gen_path, name), max_files)
            xs.append(x)
            cams.append(c)
            sids.append(np.full(x.shape[0], si, np.int32))
        coll, cont = ev.scores_many(np.concatenate(xs), np.concatenate(cams), scene_id=np.concatenate(sids), chunk=chunk, volumes=vols)
        out, lo = {}, 0
        for (name, _), x in zip(items, xs):
            out[name] = (coll[lo:lo + x.shape[0]].tolist(), cont[lo:lo + x.shape[0]].tolist())
            lo += x.shape[0]
        return out


def _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, device, what):
    """[N,V,3] world-frame vertices of the records ``xh72`` [N,72] with cameras ``cam_ext`` [N,4,4] or [1,4,4], skinned in chunks of
    ``chunk`` (the documentation of ``BodyOverlap.counts_of_records`` has the two kinds of ``evaluator_or_decoder``)."""
    if chunk < 1:
        raise ValueError(what + ': chunk must be >= 1')
    src = evaluator_or_decoder
    xh = torch.as_tensor(xh72, dtype=torch.float32, device=device).reshape(-1, 72)
    cam = torch.as_tensor(np.asarray(cam_ext, np.float32) if not torch.is_tensor(cam_ext) else cam_ext, dtype=torch.float32,
                          device=device).reshape(-1, 4, 4)
    N = xh.shape[0]
    if N < 1 or cam.shape[0] not in (1, N):
        raise ValueError(what + ': N >= 1 bodies and cam_ext [N,4,4] or [1,4,4], got %d and %s' % (N, tuple(cam.shape)))
    if isinstance(src, PlausibilityEvaluator):
        if src.flip:
            cam = torch.matmul(cam, torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], device=device)).unsqueeze(0))
        xh_rec = GeometryTransformer.convert_to_3D_rot(GeometryTransformer.convert_to_6D_rot(xh))
        skin = lambda lo, hi, c: src.op.body_verts(xh_rec[lo:hi], c)
    else:
        skin = lambda lo, hi, c: src.verts(xh[lo:hi], c.cpu().numpy())
    cam = cam.expand(N, 4, 4).contiguous()
    verts = torch.cat([skin(lo, min(N, lo + chunk), cam[lo:min(N, lo + chunk)]) for lo in range(0, N, chunk)])
    return verts


class OverlapResult(NamedTuple):
    counts: torch.Tensor       # [B,B] int32: counts[i,j] = vertices of body i inside body j (zero diagonal, not symmetric)
    inside: torch.Tensor       # [B,V] bool: the vertex is inside at least one other body
    per_body: torch.Tensor     # [B] int64: inside.sum(1)


def _as_numpy(x, dtype):
    return None if x is None else np.ascontiguousarray((x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(dtype))


class _FacesHandleOwner:
    """Owns the one topology ``faces`` [F,3] of the bodies of a batch and holds the library handle (a ``hip.Handle``) made of it for the
    vertex count last seen.  A subclass says how its handle is made (``_create(V)``).  The handle frees itself when its last holder lets
    go: this object only ever drops its reference, so an autograd graph that still needs the handle keeps it."""

    def __init__(self, faces, device):
        self.device = torch.device(device)
        self.faces = _as_numpy(faces, np.int32)
        self._handle = None

    def _handle_for(self, V):
        if not self._handle or self._handle.V != V:
            self.close()
            with torch.cuda.device(self.device):
                self._handle = self._create(V)
        return self._handle

    def close(self):
        self._handle = None

    @staticmethod
    def _group(group, verts):
        return None if group is None else torch.as_tensor(group, device=verts.device).to(torch.int32).contiguous()


class BodyOverlap(_FacesHandleOwner):
    """Body against body: which vertices of one body of a batch lie inside another (``ops.body_overlap``).  What
    ``BodyInterpenetration`` of the reference tree asks an external CUDA package for, as a count per ordered pair.  ``faces`` [F,3]: the
    one topology of every body, wound outwards."""

    def __init__(self, faces, device='cuda'):
        super().__init__(faces, device)

    def _create(self, V):
        return ops.body_overlap_create(self.faces, V)

    @torch.no_grad()
    def counts(self, verts, group=None):
        """verts [B,V,3] fp32 on the device, world frame (``op.body_verts`` / ``BodyDecoder.verts`` / ``model(..., cam_ext=)``); ``group``
        [B] or None: only bodies of equal group are compared (bodies of different scenes in one batch)."""
        counts, inside = ops.body_overlap(verts.contiguous(), self._handle_for(int(verts.shape[1])), group=self._group(group, verts))
        return OverlapResult(counts, inside, inside.sum(1))

    @torch.no_grad()
    def counts_of_records(self, xh72, cam_ext, evaluator_or_decoder, chunk=512, group=None):
        """The bodies ``xh72`` [N,72] with cameras ``cam_ext`` [N,4,4] or [1,4,4], skinned in chunks of ``chunk`` as ``scores_many`` does,
        then ONE overlap call over all N.  ``evaluator_or_decoder``: a ``PlausibilityEvaluator`` (its Habitat flip applies, as in its
        scores) or an object with ``verts(xh72, pose)`` (the ``BodyDecoder`` of utils_show_test_results.py: ``cam_ext`` is then the pose
        the bodies are placed with, as given)."""
        verts = _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, self.device, 'counts_of_records')
        return self.counts(verts, group)

    @torch.no_grad()
    def depths(self, verts, group=None):
        """How deep the vertices of ``counts`` stand in the other body (``ops.body_penetration``): the inside
        triples with the nearest face, region, depth, r and barycentric coordinates of each, max_depth [B,B] fp32, sum_depth and sum_sq
        [B,B] fp64, depth_of [B,V] fp32, together with ``counts`` and ``inside``.  Returns ``ops.PenetrationResult``."""
        return ops.body_penetration(verts.contiguous(), self._handle_for(int(verts.shape[1])), group=self._group(group, verts))

    @torch.no_grad()
    def depths_of_records(self, xh72, cam_ext, evaluator_or_decoder, chunk=512, group=None):
        """``depths`` of the bodies ``xh72`` [N,72], skinned exactly as ``counts_of_records`` skins them, in ONE call over all N."""
        verts = _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, self.device, 'depths_of_records')
        return self.depths(verts, group)

    def penetration_loss(self, verts, group=None, penalty='depth'):
        """loss [B] fp32, differentiable with respect to ``verts`` (``ops.body_penetration_loss``): the sum of the depths of the vertices
        of body i inside other bodies (``penalty='depth'``) or of their squares (``'squared'``).  ``verts`` must be contiguous."""
        if penalty not in ops.BODY_DEPTH_PENALTIES:
            raise ValueError('penalty is one of %s, got %r' % (sorted(ops.BODY_DEPTH_PENALTIES), penalty))
        return ops.body_penetration_loss(verts, self._handle_for(int(verts.shape[1])), group=self._group(group, verts), penalty=penalty)


def _greedy_walk(name, order, counts, admit, meets):
    """Walk the bodies in ``order`` and keep body i iff ``admit(c, i)`` and ``meets(c, i, k)`` for every body k already kept; ``c`` is
    ``counts`` [B,B] (a tensor or an array) as int64.  Returns the kept indices in ``order``'s order."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError('%s: counts is [B,B], got %s' % (name, c.shape,))
    c = c.astype(np.int64)
    kept = []
    for i in order:
        i = int(i)
        if not 0 <= i < c.shape[0]:
            raise ValueError('%s: body %d outside [0, %d)' % (name, i, c.shape[0]))
        if admit(c, i) and i not in kept and all(meets(c, i, k) for k in kept):
            kept.append(i)
    return kept


def select_disjoint(order, counts, max_inside=0):
    """A greedy set of mutually compatible bodies, on the host: walk the bodies in ``order`` (e.g. best plausibility first) and keep body i
    iff counts[i,k] + counts[k,i] <= max_inside for every body k already kept.  ``counts`` [B,B]: ``OverlapResult.counts`` (a tensor or an
    array).  Returns the kept indices in ``order``'s order."""
    return _greedy_walk('select_disjoint', order, counts, lambda c, i: True, lambda c, i, k: c[i, k] + c[k, i] <= max_inside)


def select_shallow(order, max_depth, tol):
    """``select_disjoint``'s walk over the penetration depths (``PenetrationResult.max_depth`` [B,B] fp32): keep body i iff
    max(max_depth[i,k], max_depth[k,i]) <= tol for every body k already kept.  Returns the kept indices in ``order``'s order."""
    m = max_depth.detach().cpu().numpy() if torch.is_tensor(max_depth) else np.asarray(max_depth)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError('select_shallow: max_depth is [B,B], got %s' % (m.shape,))
    if not tol >= 0:
        raise ValueError('select_shallow: tol must not be negative')
    deeper = (~(m.astype(np.float64) <= float(tol))).astype(np.int64)        # 1 where the pair is deeper than tol (or not a number)
    return _greedy_walk('select_shallow', order, deeper, lambda c, i: True, lambda c, i, k: c[i, k] == 0 and c[k, i] == 0)


class SurfaceCrossings(_FacesHandleOwner):
    """Which pairs of triangles of the body surfaces of a batch properly intersect, between bodies and within one body
    (``ops.surface_crossings``): the search and the body-part filter of the reference tree's
    ``BodyInterpenetration`` (human_body_prior/body_model/body_model.py:460-514); ``field`` and ``penetration_loss`` add a conic
    distance-field loss over the pairs found (section 10g; not the external package's, whose source is not available).  ``faces`` [F,3]: the
    one topology of every body; ``order_verts`` [V,3]: a representative pose (``v_template``) the faces are sorted along once;
    ``face_part`` / ``part_skip``: ``face_parts`` and ``part_skip_matrix`` below."""

    def __init__(self, faces, device='cuda', order_verts=None, face_part=None, part_skip=None):
        super().__init__(faces, device)
        self._order_verts, self._face_part, self._part_skip = _as_numpy(order_verts, np.float32), _as_numpy(face_part, np.int32), _as_numpy(part_skip, np.uint8)

    def _create(self, V):
        return ops.surface_crossings_create(self.faces, V, self._order_verts, self._face_part, self._part_skip)

    @torch.no_grad()
    def crossings(self, verts, group=None, self_pairs=True, between=True, mode='pruned'):
        """verts [B,V,3] fp32 on the device, world frame; ``group`` [B] or None as in ``BodyOverlap.counts``.  Returns
        ``ops.CrossingsResult``."""
        return ops.surface_crossings(verts.contiguous(), self._handle_for(int(verts.shape[1])), group=self._group(group, verts),
                                     self_pairs=self_pairs, between=between, mode=mode)

    @torch.no_grad()
    def crossings_of_records(self, xh72, cam_ext, evaluator_or_decoder, chunk=512, group=None, self_pairs=True, between=True):
        """The bodies ``xh72`` [N,72] with cameras ``cam_ext``, skinned in chunks of ``chunk`` exactly as
        ``BodyOverlap.counts_of_records`` skins them, then ONE crossings call over all N."""
        verts = _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, self.device, 'crossings_of_records')
        return self.crossings(verts, group, self_pairs, between)

    @torch.no_grad()
    def field(self, verts, group=None, self_pairs=True, between=True, sigma=ops.CROSSING_FIELD_SIGMA):
        """``crossings`` and, for its pairs, the conic distance field (``ops.crossing_penetration``): the rows
        ``energy`` [n,2] and ``psi`` [n,2,3], ``pair_energy`` [B,B] fp64 (what body i pays for standing in body j; the diagonal is self
        energy) and ``loss`` [B].  ``sigma`` in (0, 0.5]: the default is the reference's 1e-3, SMPLify-X uses 0.5.  Returns
        ``ops.CrossingFieldResult``."""
        return ops.crossing_penetration(verts.contiguous(), self._handle_for(int(verts.shape[1])), group=self._group(group, verts),
                                        self_pairs=self_pairs, between=between, sigma=sigma)

    def penetration_loss(self, verts, group=None, self_pairs=True, between=True, sigma=ops.CROSSING_FIELD_SIGMA):
        """loss [B] fp32 of ``field``, differentiable with respect to ``verts`` (``ops.crossing_penetration_loss``): the only term that acts
        on a body that passes through itself and on surfaces that cross with no vertex inside.  ``verts`` must be contiguous."""
        return ops.crossing_penetration_loss(verts, self._handle_for(int(verts.shape[1])), group=self._group(group, verts),
                                             self_pairs=self_pairs, between=between, sigma=sigma)

    @torch.no_grad()
    def field_of_records(self, xh72, cam_ext, evaluator_or_decoder, chunk=512, group=None, self_pairs=True, between=True,
                         sigma=ops.CROSSING_FIELD_SIGMA):
        """``field`` of the bodies ``xh72`` [N,72], skinned exactly as ``crossings_of_records`` skins them, in ONE call over all N."""
        verts = _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, self.device, 'field_of_records')
        return self.field(verts, group, self_pairs, between, sigma)


class SceneCrossings(_FacesHandleOwner):
    """Which triangles of the body surfaces of a batch properly intersect which triangles of a scene mesh (``ops.scene_crossings``;
    DESIGN.md section 10i): the one body-against-room question that needs no distance volume, so it sees geometry thinner than the
    volume's node spacing and open, unoriented scans.  ``scene_verts`` [nv,3] and ``scene_faces`` [nf,3], or a ``rendering.SceneMesh`` as
    ``scene_verts`` with ``scene_faces`` None; ``body_faces`` [F,3]: the one topology of every body; ``order_verts`` [V,3]: a
    representative pose the body faces are sorted along once.  The scene handle (``.scene``) is made at construction and lives as long as this
    object; ``close()`` lets go of the body handle only."""

    def __init__(self, scene_verts, scene_faces, body_faces, device='cuda', order_verts=None):
        super().__init__(body_faces, device)
        if scene_faces is None and hasattr(scene_verts, 'verts') and hasattr(scene_verts, 'faces'):
            scene_verts, scene_faces = scene_verts.verts, scene_verts.faces
        self._order_verts = _as_numpy(order_verts, np.float32)
        with torch.cuda.device(self.device):
            self.scene = ops.scene_crossings_create(_as_numpy(scene_verts, np.float32), _as_numpy(scene_faces, np.int32))

    def _create(self, V):
        return ops.surface_crossings_create(self.faces, V, self._order_verts)

    @torch.no_grad()
    def crossings(self, verts, mode='pruned'):
        """verts [B,V,3] fp32 on the device, world frame.  Returns ``ops.SceneCrossingsResult``."""
        return ops.scene_crossings(verts.contiguous(), self.scene, self._handle_for(int(verts.shape[1])), mode=mode)

    @torch.no_grad()
    def crossings_of_records(self, xh72, cam_ext, evaluator_or_decoder, chunk=512):
        """The bodies ``xh72`` [N,72] with cameras ``cam_ext``, skinned in chunks of ``chunk`` exactly as
        ``BodyOverlap.counts_of_records`` skins them, then ONE crossings call over all N."""
        verts = _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, self.device, 'crossings_of_records')
        return self.crossings(verts)


def select_clear(order, counts, max_pairs=0):
    """The bodies that stand clear of the scene, on the host: those of ``order``, in its order and each once, with at most ``max_pairs``
    scene crossings.  ``counts`` [B]: ``SceneCrossingsResult.counts`` (a tensor or an array)."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 1:
        raise ValueError('select_clear: counts is [B], got %s' % (c.shape,))
    kept = []
    for i in order:
        i = int(i)
        if not 0 <= i < c.shape[0]:
            raise ValueError('select_clear: body %d outside [0, %d)' % (i, c.shape[0]))
        if int(c[i]) <= max_pairs and i not in kept:
            kept.append(i)
    return kept


class BodySeparator:
    """Repairs a batch of overlapping bodies: every body is moved rigidly, by a rotation about its pivot and a translation, until no vertex
    of one lies inside another and no surfaces cross (``ops.rigid_separate``).  Shape and pose are kept.  Owns the
    two handles the searches need (``BodyOverlap`` and ``SurfaceCrossings`` of the same ``faces``; the other arguments as
    ``SurfaceCrossings``).  Without a ``scene`` the room is not looked at and a body may be pushed into furniture; with one the bodies
    are kept out of its signed distance volume as well.  ``shift`` / ``angle`` of the result say how far every body went."""

    def __init__(self, faces, device='cuda', order_verts=None, face_part=None, part_skip=None):
        self.device = torch.device(device)
        self.overlap = BodyOverlap(faces, device)
        self.crossings = SurfaceCrossings(faces, device, order_verts=order_verts, face_part=face_part, part_skip=part_skip)

    def close(self):
        self.overlap.close()
        self.crossings.close()

    def scene_table(self, scene, scene_id=None):
        """The tuple (sdf [S,D,D,D], grid_min [S,3], grid_max [S,3], scene_id [B] int32 or None) on this device that ``ops.rigid_separate``
        takes, of a ``synth.SceneData``, of a list of them (all of one D; ``scene_id`` [B] then says which body stands in which) or of such
        a tuple, which is passed on as it is.  One upload."""
        from . import synth
        if isinstance(scene, tuple):
            if scene_id is not None:
                raise ValueError('a scene tuple carries its own scene_id')
            return scene
        many = isinstance(scene, list)
        scenes = scene if many else [scene]
        if not scenes or not all(isinstance(s, synth.SceneData) for s in scenes):
            raise ValueError('scene is a synth.SceneData, a list of them, or a tuple (sdf, grid_min, grid_max, scene_id)')
        if len({tuple(np.asarray(s.sdf).shape) for s in scenes}) != 1:
            raise ValueError('the scenes of one call share one D')
        if scene_id is None and len(scenes) > 1:
            raise ValueError('several scenes need scene_id [B]')
        sdf = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(s.sdf, np.float32) for s in scenes]))).to(self.device)
        lo = torch.from_numpy(np.stack([np.asarray(s.grid_min, np.float32).reshape(3) for s in scenes])).to(self.device)
        hi = torch.from_numpy(np.stack([np.asarray(s.grid_max, np.float32).reshape(3) for s in scenes])).to(self.device)
        if scene_id is not None:
            scene_id = torch.as_tensor(np.asarray(scene_id.detach().cpu().numpy() if torch.is_tensor(scene_id) else scene_id).astype(np.int32)).to(self.device)
        return sdf, lo, hi, scene_id

    @torch.no_grad()
    def separate(self, verts, group=None, scene=None, scene_id=None, w_scene=1.0, **kw):
        """verts [B,V,3] fp32 on the device, world frame; ``group`` as in ``BodyOverlap.counts``; the keywords of ``ops.rigid_separate``
        (fixed, pivot, max_iter, lr_t, lr_r, betas, eps, w_pen, w_cross, penalty, sigma, mode).  ``scene``: what ``scene_table`` takes,
        with ``scene_id`` and ``w_scene``; uploaded once per call.  Returns ``ops.SeparationResult``."""
        V = int(verts.shape[1])
        if scene is not None:
            kw = dict(kw, scene=self.scene_table(scene, scene_id), w_scene=w_scene)
        elif scene_id is not None:
            raise ValueError('scene_id without a scene')
        return ops.rigid_separate(verts.contiguous(), self.overlap._handle_for(V), self.crossings._handle_for(V),
                                  group=_FacesHandleOwner._group(group, verts), **kw)

    @torch.no_grad()
    def separate_records(self, xh72, cam_ext, evaluator_or_decoder, chunk=512, group=None, **kw):
        """The bodies ``xh72`` [N,72] with cameras ``cam_ext`` [N,4,4] or [1,4,4], skinned exactly as ``BodyOverlap.counts_of_records``
        skins them, separated as ONE batch.  Returns (``ops.SeparationResult``, cam_ext' [N,4,4] fp64 host array) with cam_ext'[b] =
        transform[b] cam_ext[b]: a record is repaired by replacing its camera pose and nothing else (an evaluator's Habitat flip
        multiplies from the right and is not affected).  ``scene``, ``scene_id`` and ``w_scene`` as in ``separate``."""
        verts = _verts_of_records(xh72, cam_ext, evaluator_or_decoder, chunk, self.device, 'separate_records')
        res = self.separate(verts, group, **kw)
        cam = (cam_ext.detach().cpu().numpy() if torch.is_tensor(cam_ext) else np.asarray(cam_ext)).astype(np.float64).reshape(-1, 4, 4)
        cam = np.broadcast_to(cam, (verts.shape[0], 4, 4))
        return res, np.matmul(res.transform.cpu().numpy(), cam)


# the pairs of joints human_body_prior/body_model/body_model.py:488 lists for SMPL-X as additionally ignored in self contact
SMPLX_SELF_CONTACT_PAIRS = ((9, 16), (9, 17), (6, 16), (6, 17), (1, 2), (12, 22))


def face_parts(weights, faces):
    """[F] int32: the part of a face is the joint with the largest sum of its three vertices' skinning weights (``weights`` [V,J], the
    model's own), ties to the lower index."""
    w = weights.detach().cpu().numpy() if torch.is_tensor(weights) else np.asarray(weights)
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    if w.ndim != 2 or f.ndim != 2 or f.shape[1] != 3 or f.min() < 0 or f.max() >= w.shape[0]:
        raise ValueError('face_parts: weights [V,J] and faces [F,3] with indices in [0, V)')
    w = w.astype(np.float64)
    return np.argmax(w[f[:, 0]] + w[f[:, 1]] + w[f[:, 2]], axis=1).astype(np.int32)          # argmax returns the first maximum


def part_skip_matrix(parents, same=True, parent_child=True, extra=()):
    """[P,P] uint8, symmetric: non-zero where self pairs of faces of the two parts are ignored: the same part, a part and its kinematic
    parent (``parents`` [P]: the model's ``kintree_table[0]``; a root has a parent outside [0, P)), and the listed ``extra`` pairs."""
    par = np.asarray(parents.detach().cpu().numpy() if torch.is_tensor(parents) else parents).astype(np.int64).reshape(-1)
    P = len(par)
    m = np.zeros((P, P), np.uint8)
    if same:
        m[np.arange(P), np.arange(P)] = 1
    if parent_child:
        for c, p in enumerate(par.tolist()):
            if 0 <= p < P and p != c:
                m[c, p] = m[p, c] = 1
    for a, b in extra:
        if not (0 <= a < P and 0 <= b < P):
            raise ValueError('part_skip_matrix: pair (%d, %d) outside [0, %d)' % (a, b, P))
        m[a, b] = m[b, a] = 1
    return m


def select_uncrossed(order, counts, max_pairs=0, max_self=None):
    """``select_disjoint``'s walk over the crossing counts (``CrossingsResult.counts``, symmetric, self crossings on the diagonal): keep
    body i iff counts[i,k] <= max_pairs for every body k already kept, and, with ``max_self`` given, iff counts[i,i] <= max_self.  Returns
    the kept indices in ``order``'s order."""
    return _greedy_walk('select_uncrossed', order, counts, lambda c, i: max_self is None or c[i, i] <= max_self,
                        lambda c, i, k: c[i, k] <= max_pairs)


class KMeansRestarts:
    """Owns a ``psi_kmeans`` handle: R restarts of scipy's k-means loop on ``obs`` [N,d] from the initial codebooks ``guess`` [R,k,d]."""

    def __init__(self, obs, guess, thresh=1e-5):
        if not obs.is_cuda:
            raise hip.PsiHipError('KMeansRestarts needs GPU tensors (no CPU implementation exists in this package)')
        self.obs = obs.contiguous().float()                       # borrowed by the handle: kept alive here
        guess = guess.to(self.obs.device).contiguous().float()
        self.N, self.d = self.obs.shape
        self.R, self.k = guess.shape[0], guess.shape[1]
        if guess.dim() != 3 or guess.shape[2] != self.d:
            raise ValueError('KMeansRestarts: guess must be [R,k,%d], got %s' % (self.d, tuple(guess.shape)))
        h = hip.Handle('psi_kmeans_destroy')
        with torch.cuda.device(self.obs.device):
            hip.check(hip.lib().psi_kmeans_create(ctypes.byref(h), hip.ptr(self.obs), self.N, self.d, hip.ptr(guess), self.k, self.R,
                                                  float(thresh)), 'psi_kmeans_create')
        self.handle = h
        self.launches = 0             # kernel launches enqueued by iterate() (three per Lloyd iteration)
        self.syncs = 0                # host synchronisations (converged())

    def iterate(self, n_iter):
        hip.check(hip.lib().psi_kmeans_iterate(self.handle, int(n_iter), hip.stream()), 'psi_kmeans_iterate')
        self.launches += 3 * int(n_iter)

    def converged(self):
        """Number of converged restarts (synchronises the stream)."""
        n = ctypes.c_int()
        hip.check(hip.lib().psi_kmeans_read(self.handle, None, None, None, None, ctypes.byref(n), hip.stream()), 'psi_kmeans_read')
        self.syncs += 1
        return n.value

    def read(self):
        """(book [R,k,d] float32, k_eff [R] int32, avg_dist [R] float64, iters [R] int32), device tensors."""
        dev = self.obs.device
        book = torch.empty(self.R, self.k, self.d, device=dev)
        k_eff = torch.empty(self.R, dtype=torch.int32, device=dev)
        avg = torch.empty(self.R, dtype=torch.float64, device=dev)
        iters = torch.empty(self.R, dtype=torch.int32, device=dev)
        hip.check(hip.lib().psi_kmeans_read(self.handle, hip.ptr(book), hip.ptr(k_eff), hip.ptr(avg), hip.ptr(iters), None, hip.stream()),
                  'psi_kmeans_read')
        return book, k_eff, avg, iters

    def close(self):
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.obs.device)
            self.handle.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vq(obs, book):
    """``scipy.cluster.vq.vq`` on the GPU: (code [N] int32 = lowest index of the nearest row of ``book`` [k,d], dist [N] float32)."""
    obs, book = obs.contiguous().float(), book.contiguous().float()
    N, d = obs.shape
    if book.dim() != 2 or book.shape[1] != d:
        raise ValueError('vq: book must be [k,%d], got %s' % (d, tuple(book.shape)))
    code = torch.empty(N, dtype=torch.int32, device=obs.device)
    dist = torch.empty(N, device=obs.device)
    hip.check(hip.lib().psi_vq(hip.ptr(obs), N, d, hip.ptr(book), book.shape[0], hip.ptr(code), hip.ptr(dist), hip.stream()), 'psi_vq')
    return code, dist


def code_histogram(code, n_codes):
    """(counts, entropy) of utils_eval_diversity.py:96-99: ``scipy.histogram(vecs, len(codes))`` — ``n_codes`` equal-width bins over
    [min(code), max(code)], NOT ``bincount`` (they differ when the highest or lowest code has no member) — and ``entropy(counts)``
    = -sum p ln p over p = counts / N."""
    counts = np.histogram(np.asarray(code), int(n_codes))[0]
    p = counts.astype(np.float64) / counts.sum()
    p = p[p > 0]
    return counts, float(-(p * np.log(p)).sum())


def diversity_reference(bodies72, k=20, n_restarts=20, thresh=1e-5, seed=None, device='cuda', stats=None):
    """utils/utils_eval_diversity.py:93-104 in the reference's own protocol — ``scipy.cluster.vq.kmeans(ar, 20)`` (20 restarts from
    codebooks drawn from the observations, iteration until the mean Euclidean distance changes by <= 1e-5, empty codes dropped, the
    lowest-distortion codebook kept), ``vq``, ``histogram(vecs, len(codes))``, ``entropy(counts)``, ``mean(dist)`` — with every restart
    advancing in the same GPU launches.  ``seed``: an int seeds ``np.random.RandomState`` (what scipy builds from it); None draws
    from numpy's global generator like the reference.  Returns dict(entropy, mean_dist, counts, codes, distortion, winner, labels = vecs);
    ``stats`` (a dict, optional) receives the launch / synchronisation counts."""
    x = np.ascontiguousarray(np.asarray(bodies72, dtype=np.float32))
    N = x.shape[0]
    rng = np.random.RandomState(seed) if seed is not None else np.random.mtrand._rand
    idx = np.stack([rng.choice(N, size=int(k), replace=False) for _ in range(n_restarts)])
    dev = torch.device(device)
    obs = torch.tensor(x, device=dev)
    km = KMeansRestarts(obs, obs[torch.tensor(idx.reshape(-1), device=dev)].reshape(n_restarts, int(k), x.shape[1]), thresh)
    try:
        while True:
            km.iterate(16)
            if km.converged() == n_restarts:
                break
        book, k_eff, avg, iters = km.read()
        avg_h, k_eff_h, iters_h = avg.cpu().numpy(), k_eff.cpu().numpy(), iters.cpu().numpy()
        winner, best = 0, np.inf
        for r in range(n_restarts):                      # `if dist < best_dist` of scipy's kmeans: the FIRST on a tie
            if avg_h[r] < best:
                winner, best = r, avg_h[r]
        codes = book[winner, :int(k_eff_h[winner])].contiguous()
        code, dist = vq(obs, codes)
        code_h, dist_h, codes_h = code.cpu().numpy(), dist.cpu().numpy(), codes.cpu().numpy()
        if stats is not None:
            stats.update(launches=km.launches, syncs=km.syncs, iters=iters_h.tolist(), launches_per_iteration=3)
    finally:
        km.close()
    counts, ent = code_histogram(code_h, len(codes_h))
    return dict(entropy=ent, mean_dist=float(np.mean(dist_h.astype(np.float64))), counts=counts,
                codes=codes_h, distortion=float(best), winner=int(winner), labels=code_h)


def diversity_scores(bodies_72: np.ndarray, n_clusters: int = 20, seed: int = 0):
    """utils/utils_eval_diversity.py:93-104: k-means (k=20) on the generated body vectors; returns the entropy of the
    cluster-size histogram and the mean distance of samples to their cluster centre."""
    from sklearn.cluster import KMeans
    x = np.asarray(bodies_72, dtype=np.float64)
    k = min(n_clusters, len(x))
    km = KMeans(n_clusters=k, random_state=seed, n_init=10).fit(x)
    counts = np.bincount(km.labels_, minlength=k).astype(np.float64)
    p = counts / counts.sum()
    entropy = float(-(p[p > 0] * np.log(p[p > 0])).sum())
    mean_dist = float(np.mean(np.linalg.norm(x - km.cluster_centers_[km.labels_], axis=1)))
    return entropy, mean_dist
