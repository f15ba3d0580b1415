#!/usr/bin/env python
"""python utils_snapshots_virtualcam.py SCENE_PLY OUT_DIR     (or: OUT_DIR --synthetic DIR)

From a scene mesh to a sensor folder (cam_*.npy, depth_*.npy, seg_*.npy) that the generation scripts read, on the GPU and without a
window: virtual cameras on the reference's lattice around a target point (utils/utils_prox_snapshots_virtualcam.py:102-180), all rendered
in one call, the views whose target is outside the image or occluded left out (:342-378), the first --n_cams of the rest written.
Moving recorded bodies into the virtual cameras and writing the training records (the second half of the reference's script) is
utils_make_training_set.py."""
import argparse
import os

import _eval_common  # noqa: F401  (path setup)
import numpy as np

from psi_release_amd import rendering, synth
from psi_release_amd.scene_io import write_ply_mesh


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('scene_ply', nargs='?')
    ap.add_argument('out_dir', nargs='?')
    ap.add_argument('--n_cams', type=int, default=30)
    ap.add_argument('--size', type=int, nargs=2, default=[270, 480], metavar=('H', 'W'))
    ap.add_argument('--fx', type=float, default=None, help='focal length in pixels (default: 60 degrees vertical field of view)')
    ap.add_argument('--fy', type=float, default=None)
    ap.add_argument('--target', type=float, nargs=3, default=None, help='the point the cameras look at (default: 0.9 m above the middle of the floor)')
    ap.add_argument('--grid_nodes', type=int, default=10)
    ap.add_argument('--near', type=float, default=0.05)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--synthetic', default=None, help='write a stand-in room mesh to DIR/room.ply and use it as the scene')
    a = ap.parse_args(argv)
    planes = None
    if a.synthetic:
        if a.out_dir is None:
            a.scene_ply, a.out_dir = None, a.scene_ply
        room = synth.make_room_mesh(a.seed, 180)
        os.makedirs(a.synthetic, exist_ok=True)
        a.scene_ply = os.path.join(a.synthetic, 'room.ply')
        write_ply_mesh(a.scene_ply, room.verts, room.faces, room.rgb())
        planes = room.planes()
    if not a.scene_ply or not a.out_dir:
        ap.error('SCENE_PLY and OUT_DIR are required (or OUT_DIR --synthetic DIR)')
    mesh = rendering.SceneMesh.from_ply(a.scene_ply)
    verts = mesh.verts.cpu().numpy().astype(np.float64)
    smin, smax = verts.min(0), verts.max(0)
    target = np.array(a.target) if a.target else np.array([(smin[0] + smax[0]) / 2, (smin[1] + smax[1]) / 2, smin[2] + 0.9])
    H, W = a.size
    fy = a.fy or a.fx or (H / 2) / np.tan(np.radians(30.0))
    fx = a.fx or fy
    K = np.array([[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]])
    cams = rendering.sample_virtual_cams(smin, smax, target, planes, grid_nodes=a.grid_nodes, rng=np.random.RandomState(a.seed))
    print('--obtain {:d} cams'.format(len(cams)))
    if not len(cams):
        raise SystemExit('no camera position passes the filters: is the scene smaller than 1.65 m around the target?')
    depth, seg, _ = rendering.SnapshotRenderer(mesh).render(cams, K, (H, W), a.near)
    depth_h = depth.cpu().numpy()
    keep = []
    for i, ext in enumerate(cams):
        target_cam = np.linalg.inv(ext)[:3] @ np.append(target, 1.0)
        if rendering.view_is_usable(depth_h[i], target_cam, K):
            keep.append(i)
        else:
            print('-- the target is occluded or not in the image at view %d' % i)
    if not keep:
        raise SystemExit('the target is occluded or outside the image in every one of the %d views: nothing written' % len(cams))
    keep = keep[:a.n_cams]
    files = rendering.write_sensor_folder(a.out_dir, depth_h[keep], seg.cpu().numpy()[keep], cams[keep], K)
    print('[INFO] wrote %d views to %s' % (len(files), a.out_dir))


if __name__ == '__main__':
    main()
