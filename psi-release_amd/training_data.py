"""Training records from a scene mesh and recorded bodies — the table that ``train_s1.py`` / ``train_s2.py`` read.

Reference: the second half of utils/utils_prox_snapshots_virtualcam.py (``update_globalRT_for_smplx`` :209-263, ``is_body_occluded``
:342-378, the record loop :456-554), utils/utils_convert2hdf5.py (two more filters, the streams) and the filters of
``BatchGeneratorWithSceneMeshMatfile.next_batch`` (batch_gen_hdf5.py:542-546).  The reference renders one view at a time in an open3d
window and preprocesses each image on the host; here a pass of ``frames_per_pass`` frames is ONE ``SnapshotRenderer.render`` call, ONE
``ops.snapshot_canvas`` call (csrc/canvas.hip) and one device -> host copy.

* ``pelvis_table`` / ``reframe_bodies`` / ``target_windows``   the per-frame geometry, fp64 NumPy on the host (a few numbers per view;
                                                               the camera lattice is sampled on the host anyway)
* ``TrainingSetBuilder``                                      frames in, the stream table / ``.npz`` / ``.mat`` records out
* ``read_proxd_fits``                                         ``results/*/000.pkl`` of a PROX-D fitting folder

Conventions as ``rendering``: ``cam_ext`` is camera-to-world, the camera looks along +z with x right and y down.  One deliberate
difference from the reference: its window test projects the body's ``transl`` (the model's origin, :344-356) with the image centre as
principal point; this one projects the pelvis — the point the virtual cameras look at — with the principal point of ``cam_int``, as
``rendering.view_is_usable`` does.  The filters on ``transl`` (|x| <= 10, 0 < z < max_d) are the reference's.
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from . import rendering

BODY_KEYS = ('transl', 'global_orient', 'betas', 'pose_embedding', 'left_hand_pose', 'right_hand_pose')
BODY_DIMS = (3, 3, 10, 32, 12, 12)
STREAMS = ('depth', 'seg', 'body', 'cam_ext', 'cam_int', 'max_d', 'sceneid')
DROP_RULES = ('border', 'occluded', 'x_range', 'z_range')


def _field(model, key):
    return np.asarray(getattr(model, key) if hasattr(model, key) else model[key], dtype=np.float64)


def pelvis_table(body_model):
    """(J0 [3], dJ0 [3,10]) fp64: row 0 of ``J_regressor`` applied to ``v_template`` and to the first 10 shape directions, so that the pelvis
    of a body with zero global orientation and translation is ``J0 + dJ0 @ betas`` whatever its pose (the reference runs SMPL-X for this,
    :221-234; joint 0 of that run depends on the shape only).  ``body_model``: an object or dict with the SMPL-X arrays (``synth.SMPLXData``)."""
    jr0 = _field(body_model, 'J_regressor')[0]
    return jr0 @ _field(body_model, 'v_template'), np.einsum('v,vkb->kb', jr0, _field(body_model, 'shapedirs')[:, :, :10])


def reframe_bodies(global_orient, transl, delta_T, trans):
    """Steps (2)-(3) of ``update_globalRT_for_smplx``: N bodies expressed in each of n new frames.  global_orient, transl [N,3]; delta_T [N,3]
    or [3], the pelvis of each body at zero orientation and translation; trans [n,4,4] rigid transforms from the bodies' frame to the new
    ones.  Returns fp64 (global_orient' [N,n,3], transl' [N,n,3], pelvis' [N,n,3]) with

        R' = R_t exp(global_orient),   t' = R_t (transl + delta_T) + t_t - delta_T,   global_orient' = log(R'),   pelvis' = t' + delta_T

    exp and log through scipy's quaternion, so the rotation vector stays stable near 0 and near pi."""
    from scipy.spatial.transform import Rotation
    go = np.asarray(global_orient, np.float64).reshape(-1, 3)
    N = len(go)
    tr = np.asarray(transl, np.float64).reshape(N, 3)
    dT = np.broadcast_to(np.asarray(delta_T, np.float64), (N, 3))
    T = np.asarray(trans, np.float64).reshape(-1, 4, 4)
    Rt, tt = T[:, :3, :3], T[:, :3, 3]
    R_new = np.einsum('nij,Njk->Nnik', Rt, Rotation.from_rotvec(go).as_matrix())
    go_new = Rotation.from_matrix(R_new.reshape(-1, 3, 3)).as_rotvec().reshape(N, len(T), 3)
    pelvis = np.einsum('nij,Nj->Nni', Rt, tr + dT) + tt[None]
    return go_new, pelvis - dT[:, None], pelvis


def target_windows(pelvis_cam, cam_int, size):
    """The window test's host half, as ``rendering.view_is_usable``: pelvis_cam [n,3] (camera coordinates), cam_int [3,3] or [n,3,3],
    size = (H, W).  The pixel is (int(x fx / z + cx), int(y fy / z + cy)); a view is rejected when z <= 0 or the pixel is not more than
    10 pixels inside the image; the window is the pixel +-10, cut to the image.  Returns windows [n,4] int32 = x0, y0, x1, y1 (zeros for a
    rejected view), z [n] fp64 and ok [n] bool (False: rejected here)."""
    p = np.asarray(pelvis_cam, np.float64).reshape(-1, 3)
    n = len(p)
    K = np.asarray(cam_int, np.float64)
    K = np.broadcast_to(K, (n, 3, 3)) if K.ndim == 2 else K.reshape(n, 3, 3)
    H, W = int(size[0]), int(size[1])
    z = p[:, 2].copy()
    front = z > 0
    zs = np.where(front, z, 1.0)
    lim = 2.0 ** 30
    cx = np.trunc(np.clip(p[:, 0] * K[:, 0, 0] / zs + K[:, 0, 2], -lim, lim)).astype(np.int64)
    cy = np.trunc(np.clip(p[:, 1] * K[:, 1, 1] / zs + K[:, 1, 2], -lim, lim)).astype(np.int64)
    ok = front & (cx > 10) & (cx <= W - 10) & (cy > 10) & (cy <= H - 10)
    win = np.stack([np.maximum(cx - 10, 0), np.maximum(cy - 10, 0), np.minimum(cx + 10, W), np.minimum(cy + 10, H)], -1)
    return np.where(ok[:, None], win, 0).astype(np.int32), z, ok


def select_views(inside, usable, transl, max_d):
    """The four rules a view must pass, in order: ``inside`` (the border rule of ``target_windows``), ``usable`` (the window test),
    |transl_x| <= 10 (batch_gen_hdf5.py:545) and 0 < transl_z < max_d (utils_convert2hdf5.py:92-98).  Returns (kept [n] bool, dropped):
    every view is counted under the FIRST rule it fails, so the counts and the kept views add up to n."""
    transl = np.asarray(transl, np.float64).reshape(-1, 3)
    rules = (np.asarray(inside, bool), np.asarray(usable, bool), np.abs(transl[:, 0]) <= 10.0,
             (transl[:, 2] > 0) & (transl[:, 2] < np.asarray(max_d, np.float64)))
    alive = np.ones(len(transl), bool)
    dropped = {}
    for name, ok in zip(DROP_RULES, rules):
        dropped[name] = int((alive & ~ok).sum())
        alive &= ok
    return alive, dropped


def read_proxd_fits(fitting_dir, sample_rate=15):
    """``results/*/000.pkl`` of a PROX-D fitting folder, every ``sample_rate``-th frame in sorted order (:456-471; a frame without its file
    is left out).  Returns the dict of arrays ``TrainingSetBuilder.add_frames`` takes; the 32-d ``body_pose`` of the files is
    ``pose_embedding``."""
    res = os.path.join(fitting_dir, 'results')
    rows = {k: [] for k in BODY_KEYS}
    for name in sorted(os.listdir(res))[::sample_rate]:
        fn = os.path.join(res, name, '000.pkl')
        if not os.path.exists(fn):
            continue
        with open(fn, 'rb') as f:
            d = pickle.load(f, encoding='latin1')
        for k, dim in zip(BODY_KEYS, BODY_DIMS):
            src = d[k] if k in d else d['body_pose']
            rows[k].append(np.asarray(src, np.float64).reshape(-1)[:dim])
    return {k: np.stack(v) if v else np.zeros((0, dim)) for (k, v), dim in zip(rows.items(), BODY_DIMS)}


def synthetic_bodies(body_model, box_min, box_max, n=4, seed=0):
    """n seeded world-frame bodies for the stand-in room (z up, floor at box_min[2]): the pelvis 0.9 m above the floor within the middle
    half of the box, upright up to a turn about z and a small tilt.  A dict as ``TrainingSetBuilder.add_frames`` takes."""
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(seed)
    J0, dJ0 = pelvis_table(body_model)
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    betas = rs.standard_normal((n, 10)) * 0.5
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    pelvis = np.stack([rs.uniform(mid[0] - half[0], mid[0] + half[0], n), rs.uniform(mid[1] - half[1], mid[1] + half[1], n),
                       np.full(n, lo[2] + 0.9)], -1)
    turn = Rotation.from_euler('z', rs.uniform(-np.pi, np.pi, n)) * Rotation.from_rotvec(rs.standard_normal((n, 3)) * 0.1)
    return {'transl': pelvis - (J0 + betas @ dJ0.T), 'global_orient': turn.as_rotvec(), 'betas': betas,
            'pose_embedding': rs.standard_normal((n, 32)) * 0.5, 'left_hand_pose': rs.standard_normal((n, 12)) * 0.2,
            'right_hand_pose': rs.standard_normal((n, 12)) * 0.2}


class TrainingSetBuilder:
    """Recorded bodies in, training records out.  ``scene_mesh``: a ``rendering.SceneMesh``; ``body_model``: the SMPL-X arrays
    (``pelvis_table``); ``cam_int`` [3,3] of the virtual cameras; ``size`` = (H, W) of the rendered views.  The camera lattice spans the
    scene's bounding box moved inwards by ``box_shrink`` (the reference's 0.7, :423-425) and outwards by ``box_grow`` (its 2.0 for six
    scenes, :107-111); ``room_planes``, ``grid_nodes`` and ``noise`` go to ``rendering.sample_virtual_cams``.  One ``RandomState(seed)``
    draws the lattice noise and the permutation of each frame, so a seed fixes the set.  ``keep_images``: also keep the rendered images
    of the kept views on the host (``write_mat_records`` needs them; a second copy per pass)."""

    def __init__(self, scene_mesh, body_model, cam_int, size=(270, 480), scene_id=0, room_planes=None, box_shrink=0.7, box_grow=0.0,
                 n_cams=30, grid_nodes=10, noise=0.5, frames_per_pass=8, seed=0, canvas_size=(128, 128), near=0.05, keep_images=False):
        self.mesh = scene_mesh
        self.J0, self.dJ0 = pelvis_table(body_model)
        self.cam_int = np.asarray(cam_int, np.float64).reshape(3, 3)
        self.size = (int(size[0]), int(size[1]))
        self.scene_id, self.room_planes = scene_id, room_planes
        self.n_cams, self.grid_nodes, self.noise = int(n_cams), int(grid_nodes), float(noise)
        self.frames_per_pass = max(1, int(frames_per_pass))
        self.canvas_size, self.near, self.keep_images = (int(canvas_size[0]), int(canvas_size[1])), float(near), bool(keep_images)
        self.rng = np.random.RandomState(seed)
        v = scene_mesh.verts
        v = np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, np.float64).reshape(-1, 3)
        self.box_min, self.box_max = v.min(0) + box_shrink - box_grow, v.max(0) - box_shrink + box_grow
        self._renderer = None
        self._pending = []
        self._rows = {k: [] for k in STREAMS}
        self._ids, self._images = [], []
        self._frame = -1
        self.stats = dict(frames=0, frames_nan=0, views_sampled=0, kept=0, **{'dropped_' + r: 0 for r in DROP_RULES})

    # ---- the two device steps of a pass (a test without a GPU overrides them) ----
    def _render(self, cam_ext):
        """depth, seg [n,H,W] of the views ``cam_ext`` [n,4,4]."""
        if self._renderer is None:
            self._renderer = rendering.SnapshotRenderer(self.mesh)
        depth, seg, _ = self._renderer.render(cam_ext, self.cam_int, self.size, self.near)
        return depth, seg

    def _canvas(self, depth, seg, windows, z):
        """(depth_canvas [n,1,th,tw], seg_canvas, max_d [n], usable [n]) on the host, from one kernel call and one copy."""
        import torch
        from . import ops
        dc, sc, max_d, _, usable = ops.snapshot_canvas(depth, seg, self.canvas_size, windows, z)
        n, px = dc.shape[0], dc.shape[2] * dc.shape[3]
        host = torch.cat([dc.view(n, px), sc.view(n, px), max_d.view(n, 1), usable.to(torch.float32).view(n, 1)], 1).cpu().numpy()
        shape = (n, 1) + self.canvas_size
        return host[:, :px].reshape(shape), host[:, px:2 * px].reshape(shape), host[:, 2 * px], host[:, 2 * px + 1] > 0

    def _host_images(self, images, kept):
        import torch
        if torch.is_tensor(images):
            return images[torch.as_tensor(kept, device=images.device)].cpu().numpy()
        return np.asarray(images)[kept]

    # ---- frames ----
    def add_frames(self, bodies, cam2world=None):
        """bodies: dict of arrays transl [N,3], global_orient [N,3], betas [N,10], pose_embedding [N,32], left_hand_pose [N,12],
        right_hand_pose [N,12], in the frame of a recording camera whose pose is ``cam2world`` [4,4], or in the world frame (None)."""
        cols = [np.asarray(bodies[k], np.float64).reshape(-1, d) for k, d in zip(BODY_KEYS, BODY_DIMS)]
        N = len(cols[0])
        if any(len(c) != N for c in cols):
            raise ValueError('the body arrays differ in length')
        to_world = np.eye(4) if cam2world is None else np.asarray(cam2world, np.float64).reshape(4, 4)
        for i in range(N):
            self.stats['frames'] += 1
            row = [c[i] for c in cols]
            if any(np.isnan(r).any() for r in row):                       # :470
                self.stats['frames_nan'] += 1
                continue
            self._frame += 1
            transl, go, betas = row[0], row[1], row[2]
            dT = self.J0 + self.dJ0 @ betas
            go_w, t_w, pelvis_w = (a[0, 0] for a in reframe_bodies(go, transl, dT, to_world[None]))
            cams = rendering.sample_virtual_cams(self.box_min, self.box_max, pelvis_w, self.room_planes, self.grid_nodes, self.noise, self.rng)
            cams = cams[self.rng.permutation(len(cams))[:self.n_cams]]    # :492-493
            self.stats['views_sampled'] += len(cams)
            if len(cams):
                go_c, t_c, pelvis_c = (a[0] for a in reframe_bodies(go_w, t_w, dT, np.linalg.inv(cams)))
                self._pending.append(dict(frame=self._frame, cams=cams, go=go_c, transl=t_c, pelvis=pelvis_c, rest=np.concatenate(row[2:])))
            if len(self._pending) >= self.frames_per_pass:
                self.flush()

    def flush(self):
        """Run the pass over the frames that wait for one."""
        if not self._pending:
            return
        pend, self._pending = self._pending, []
        cams = np.concatenate([p['cams'] for p in pend])
        go, transl, pelvis = (np.concatenate([p[k] for p in pend]) for k in ('go', 'transl', 'pelvis'))
        rest = np.concatenate([np.tile(p['rest'][None], (len(p['cams']), 1)) for p in pend])
        ids = np.concatenate([np.stack([np.full(len(p['cams']), p['frame']), np.arange(len(p['cams']))], 1) for p in pend])
        windows, z, inside = target_windows(pelvis, self.cam_int, self.size)
        depth, seg = self._render(cams)
        dc, sc, max_d, usable = self._canvas(depth, seg, windows, z.astype(np.float32))
        alive, dropped = select_views(inside, usable, transl, max_d)
        for name, k in dropped.items():
            self.stats['dropped_' + name] += k
        kept = np.nonzero(alive)[0]
        self.stats['kept'] += len(kept)
        if not len(kept):
            return
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self._rows['depth'].append(f32(dc[kept]))
        self._rows['seg'].append(f32(sc[kept]))
        self._rows['body'].append(f32(np.concatenate([transl[kept], go[kept], rest[kept]], 1)))
        self._rows['cam_ext'].append(f32(cams[kept]))
        self._rows['cam_int'].append(f32(np.tile(self.cam_int[None], (len(kept), 1, 1))))
        self._rows['max_d'].append(f32(max_d[kept]))
        self._rows['sceneid'].append(np.full(len(kept), self.scene_id, np.float32))
        self._ids.append(ids[kept])
        if self.keep_images:
            self._images.append((self._host_images(depth, kept), self._host_images(seg, kept)))

    # ---- results ----
    def table(self):
        """The stream dict ``BatchGeneratorWithSceneMesh.from_arrays`` takes: depth, seg [1+k,1,th,tw], body [1+k,72] (transl, global_orient,
        betas, pose_embedding, left hand, right hand, in the view's camera), cam_ext [1+k,4,4] camera-to-world, cam_int [1+k,3,3], max_d
        [1+k] (the clipped depth maximum), sceneid [1+k]; row 0 is a placeholder of zeros, as in the reference's files."""
        self.flush()
        th, tw = self.canvas_size
        shapes = dict(depth=(1, th, tw), seg=(1, th, tw), body=(72,), cam_ext=(4, 4), cam_int=(3, 3), max_d=(), sceneid=())
        return {k: np.concatenate([np.zeros((1,) + shapes[k], np.float32)] + self._rows[k]) for k in STREAMS}

    def record_ids(self):
        """[k,2] int: (frame, camera) of every kept row — frames count the ones that had no NaN, cameras the permuted list."""
        self.flush()
        return np.concatenate(self._ids) if self._ids else np.zeros((0, 2), np.int64)

    def images(self):
        """(depth0, seg0) [k,H,W]: the rendered images of the kept rows, unclipped (needs ``keep_images=True``)."""
        self.flush()
        if not self.keep_images:
            raise ValueError('the rendered images are kept only with keep_images=True')
        if not self._images:
            return np.zeros((0,) + self.size, np.float32), np.zeros((0,) + self.size, np.float32)
        return np.concatenate([a for a, _ in self._images]), np.concatenate([b for _, b in self._images])

    def write_npz(self, path):
        """The table as the ``.npz`` that ``BatchGeneratorWithSceneMesh`` reads."""
        np.savez(path, **self.table())

    def write_mat_records(self, folder):
        """One ``rec_frame%06d_cam%06d.mat`` per kept view with the reference's keys (:546-554): depth0 / seg0 (the rendered images, clipped as
        the reference's in-place clip leaves them), depth / seg (the canvases), scaling_factor, cam (intrinsic; extrinsic = world-to-camera,
        as open3d's) and body; body also carries ``body_pose`` = the 32-d embedding, the name ``BatchGeneratorTest`` reads."""
        import scipy.io as sio
        from . import ops
        d0, s0 = self.images()
        t = self.table()
        ids = self.record_ids()
        H, W = self.size
        factor = float(self.canvas_size[0]) / H if H >= W else float(self.canvas_size[1]) / W
        os.makedirs(folder, exist_ok=True)
        files = []
        for i, (frame, cam) in enumerate(ids):
            body = t['body'][1 + i]
            parts = dict(zip(BODY_KEYS, np.split(body[None], np.cumsum(BODY_DIMS)[:-1], axis=1)))
            parts['body_pose'] = parts['pose_embedding']
            fn = os.path.join(folder, 'rec_frame%06d_cam%06d.mat' % (frame, cam))
            sio.savemat(fn, {'scaling_factor': factor, 'depth': t['depth'][1 + i, 0], 'seg': t['seg'][1 + i, 0],
                             'depth0': np.minimum(d0[i], np.float32(ops.CANVAS_CLIP_DEPTH)), 'seg0': np.minimum(s0[i], np.float32(ops.CANVAS_CLIP_SEG)),
                             'cam': {'intrinsic': t['cam_int'][1 + i].astype(np.float64),
                                     'extrinsic': np.linalg.inv(t['cam_ext'][1 + i].astype(np.float64))},
                             'body': parts})
            files.append(fn)
        return files
