#!/usr/bin/env python
"""python utils_make_training_set.py SCENE_PLY FITS OUT.npz --cam2world JSON --scene_id K [--planes JSON --n_cams 30 --size 270 480 --fx F
                                       --mat_dir DIR --seed S]          (or: OUT.npz --synthetic DIR)

From a scene mesh and recorded body fits to the table that train_s1.py / train_s2.py read, on the GPU and without a window — the second
half of the reference's utils/utils_prox_snapshots_virtualcam.py followed by utils/utils_convert2hdf5.py (psi_release_amd.training_data):
every fitted frame is moved into the world with the recording camera's pose, seen from --n_cams virtual cameras of the reference's
lattice, moved into each of them, and kept where its pelvis is inside the image and not occluded and its translation passes the reference's
range filters.  FITS is a PROX-D fitting folder (results/*/000.pkl, every --sample_rate-th frame); --cam2world the 4 x 4 pose of the
recording camera as PROX's cam2world/<scene>.json; --planes a JSON list of (point, inward normal) pairs that fence the cameras in;
--scene_id the scene's index in the generator's scene list; --mat_dir also writes one rec_frame*_cam*.mat per kept view.
--synthetic DIR writes a stand-in room to DIR/room.ply and uses it with the stand-in body model and a handful of seeded standing bodies."""
import argparse
import json
import os

import _eval_common  # noqa: F401  (path setup)
import numpy as np

from psi_release_amd import rendering, synth
from psi_release_amd import training_data as TD
from psi_release_amd.scene_io import write_ply_mesh


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('scene_ply', nargs='?')
    ap.add_argument('fits', nargs='?')
    ap.add_argument('out_npz', nargs='?')
    ap.add_argument('--cam2world', default=None)
    ap.add_argument('--scene_id', type=int, default=0)
    ap.add_argument('--planes', default=None)
    ap.add_argument('--human_model', default=None, help='SMPLX_NEUTRAL.npz (J_regressor, v_template, shapedirs)')
    ap.add_argument('--n_cams', type=int, default=30)
    ap.add_argument('--size', type=int, nargs=2, default=[270, 480], metavar=('H', 'W'))
    ap.add_argument('--fx', type=float, default=None, help='focal length in pixels (default: 60 degrees vertical field of view)')
    ap.add_argument('--sample_rate', type=int, default=15)
    ap.add_argument('--box_shrink', type=float, default=0.7)
    ap.add_argument('--box_grow', type=float, default=0.0, help='the reference grows the box of six PROX scenes by 2.0')
    ap.add_argument('--frames_per_pass', type=int, default=8)
    ap.add_argument('--mat_dir', default=None)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--synthetic', default=None, help='write a stand-in room mesh to DIR/room.ply and use it with stand-in bodies')
    a = ap.parse_args(argv)
    planes, cam2world = None, None
    if a.synthetic:
        if a.out_npz is None:
            a.out_npz = a.scene_ply
        room = synth.make_room_mesh(a.seed, 180)
        os.makedirs(a.synthetic, exist_ok=True)
        a.scene_ply = os.path.join(a.synthetic, 'room.ply')
        write_ply_mesh(a.scene_ply, room.verts, room.faces, room.rgb())
        planes, model = room.planes(), synth.make_smplx(7)
        bodies = TD.synthetic_bodies(model, room.box_min, room.box_max, 6, seed=a.seed)
        if a.box_shrink == 0.7:
            a.box_shrink = 0.3                    # the stand-in room is 5 x 4 m: the reference's 0.7 leaves too few camera positions
    else:
        if not (a.scene_ply and a.fits and a.out_npz and a.human_model):
            ap.error('SCENE_PLY FITS OUT.npz and --human_model are required (or OUT.npz --synthetic DIR)')
        model = dict(np.load(a.human_model, allow_pickle=True))
        bodies = TD.read_proxd_fits(a.fits, a.sample_rate)
        if a.cam2world:
            with open(a.cam2world) as f:
                cam2world = np.array(json.load(f), np.float64).reshape(4, 4)
        if a.planes:
            with open(a.planes) as f:
                planes = np.array(json.load(f), np.float64).reshape(-1, 2, 3)
    if not a.out_npz:
        ap.error('OUT.npz is required')
    mesh = rendering.SceneMesh.from_ply(a.scene_ply)
    H, W = a.size
    fx = a.fx or (H / 2) / np.tan(np.radians(30.0))
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]])
    b = TD.TrainingSetBuilder(mesh, model, K, size=(H, W), scene_id=a.scene_id, room_planes=planes, box_shrink=a.box_shrink, box_grow=a.box_grow,
                              n_cams=a.n_cams, frames_per_pass=a.frames_per_pass, seed=a.seed, keep_images=a.mat_dir is not None)
    b.add_frames(bodies, cam2world)
    b.write_npz(a.out_npz)
    print('[INFO] %s' % json.dumps(b.stats))
    print('[INFO] wrote %d records to %s' % (b.stats['kept'], a.out_npz))
    if a.mat_dir:
        print('[INFO] wrote %d .mat records to %s' % (len(b.write_mat_records(a.mat_dir)), a.mat_dir))
    if not b.stats['kept']:
        raise SystemExit('no view passed the filters: nothing to train on')
    return b.stats


if __name__ == '__main__':
    main()
