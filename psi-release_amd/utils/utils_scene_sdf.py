#!/usr/bin/env python
"""python utils_scene_sdf.py SCENE_PLY OUT_ROOT --name N [--dim 256 --margin 0.5 --voxel V --sign winding --cloud surface --spacing S
                                                      --orient --seed X Y Z]
                                                                                                   (or: OUT_ROOT --name N --synthetic)

From a scene mesh to the two scene files of the fitting and evaluation scripts, on the GPU: OUT_ROOT/scenes_sdf/N.json + N_sdf.npy (the
signed distance volume over the mesh's box grown by --margin, [ix][iy][iz], positive in free space) and OUT_ROOT/scenes_downsampled/N.ply
(the welded vertices, one per --voxel cell when given; with --cloud surface --spacing S points on the surface instead, about one per
S-sized cell whatever the tessellation: for CAD, synthetic and decimated meshes).  The reference ships these as downloads.  Triangles must
face free space: --orient winds them that way first, from points known to be free (--seed X Y Z, repeatable), and prints how many it
flipped, decided by propagation and left undecided.  With
the default --sign pseudonormal an open mesh gets its sign from the orientation of the nearest triangle, --sign winding takes it from the
generalised winding number (open scans, furniture that touches or enters the floor).  Prints the three config paths of the fitting scripts."""
import argparse

import _eval_common  # noqa: F401  (path setup)

from psi_release_amd import scene_sdf, synth
from psi_release_amd.scene_io import read_ply_mesh


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('scene_ply', nargs='?')
    ap.add_argument('out_root', nargs='?')
    ap.add_argument('--name', required=True, help='scene name: the files are scenes_sdf/NAME.json, scenes_sdf/NAME_sdf.npy, scenes_downsampled/NAME.ply')
    ap.add_argument('--dim', type=int, default=256, help='nodes per axis (a multiple of 4, at most 480: what the fitting engine samples)')
    ap.add_argument('--margin', type=float, default=0.5, help='the grid box is the mesh box grown by this on every side (m)')
    ap.add_argument('--voxel', type=float, default=None, help='keep one vertex per cell of this size in the point cloud')
    ap.add_argument('--cloud', choices=scene_sdf.CLOUDS, default='vertices', help='the point cloud: the welded vertices of the mesh, or even '
                    'samples of its surface (needs --spacing)')
    ap.add_argument('--spacing', type=float, default=None, help='--cloud surface: about one point per cell of this size (m)')
    ap.add_argument('--sign', choices=scene_sdf.SIGNS, default='pseudonormal', help='where the sign comes from: the pseudonormal of the nearest '
                    'feature (closed, clean meshes) or the generalised winding number (open, touching or interpenetrating meshes)')
    ap.add_argument('--exterior', choices=sorted(scene_sdf.LEVELS), default='solid', help='--sign winding: what lies outside the mesh, solid '
                    '(a room) or free (objects standing in open space)')
    ap.add_argument('--beta', type=float, default=3.0, help='--sign winding: clusters farther than beta x their radius count as dipoles; 0 = exact')
    ap.add_argument('--orient', action='store_true', help='wind every triangle towards free space first (scene_sdf.orient_faces); needs --seed')
    ap.add_argument('--seed', type=float, nargs=3, action='append', metavar=('X', 'Y', 'Z'), help='--orient: a point known to lie in free space '
                    '(repeatable); with --synthetic the room centre at 1.5 m by default')
    ap.add_argument('--orient-dim', type=int, default=128, help='--orient: nodes per axis of the grid the free space is found on')
    ap.add_argument('--synthetic', action='store_true', help='use the stand-in room synth.make_oriented_room instead of a PLY')
    ap.add_argument('--subdiv', type=int, default=2, help='--synthetic: cuts per box face edge')
    ap.add_argument('--flip', type=float, default=0.0, help='--synthetic: reverse this share of the triangles first (synth.flip_faces, seed 1): '
                    'the mixed winding that --orient repairs')
    a = ap.parse_args(argv)
    if a.synthetic:
        if a.out_root is None:
            a.scene_ply, a.out_root = None, a.scene_ply
        if a.scene_ply is not None:
            ap.error('--synthetic takes OUT_ROOT only')
    if not a.out_root or not (a.synthetic or a.scene_ply):
        ap.error('SCENE_PLY and OUT_ROOT are required (or OUT_ROOT --synthetic)')
    try:
        scene_sdf.check_engine_dim(a.dim)
    except ValueError as e:
        ap.error(str(e))
    if not (a.beta >= 0 and a.beta < float('inf')):
        ap.error('--beta must be finite and not negative')
    if a.margin < 0 or (a.voxel is not None and a.voxel <= 0):
        ap.error('--margin must not be negative and --voxel must be positive')
    if a.flip and not a.synthetic or not 0.0 <= a.flip <= 1.0:
        ap.error('--flip belongs to --synthetic and lies in [0, 1]')
    if a.seed and not a.orient:
        ap.error('--seed belongs to --orient')
    if a.orient and not a.seed:
        if not a.synthetic:
            ap.error('--orient needs a --seed X Y Z: a point known to lie in free space')
        a.seed = [[0.0, 0.0, 1.5]]
    if a.orient and not 2 <= a.orient_dim <= 1024:
        ap.error('--orient-dim lies in 2 .. 1024')
    try:
        scene_sdf.check_cloud_args(a.cloud, a.voxel, a.spacing)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse(argv)
    parts = None
    if a.synthetic:
        room = synth.make_oriented_room(a.subdiv)
        verts, faces = room.verts, synth.flip_faces(room.faces, a.flip, seed=1)[0]
        parts = synth.make_scene(0, m=8, D=2).contact_parts          # stand-in body_segments/*.json (the real ones ship with PROX)
    else:
        verts, faces, _ = read_ply_mesh(a.scene_ply)
    if a.orient:
        r = scene_sdf.orient_faces(verts, faces, a.seed, dim=a.orient_dim)
        faces = r.faces
        print('[INFO] orient: %d of %d triangles flipped, %d decided by propagation, %d left undecided, %d without area (%d free nodes, %d fill '
              'launches)' % (r.flipped.sum(), len(faces), (r.decided_by == scene_sdf.DECIDED_BY_PROPAGATION).sum(),
                             (r.decided_by == scene_sdf.UNDECIDED).sum(), (r.decided_by == scene_sdf.ZERO_AREA).sum(), r.free_nodes, r.rounds))
    scene = scene_sdf.scene_from_mesh(verts, faces, dim=a.dim, margin=a.margin, voxel=a.voxel, contact_parts=parts, sign=a.sign, exterior=a.exterior,
                                      beta=a.beta, cloud=a.cloud, spacing=a.spacing)
    paths = scene.write_prox_layout(a.out_root, a.name)
    print('[INFO] %d triangles -> %d^3 volume, %d cloud points' % (len(faces), a.dim, len(scene.verts)))
    for k in ('scene_verts_path', 'scene_sdf_path', 'contact_id_folder'):
        print('%s: %s' % (k, paths[k]))
    return paths


if __name__ == '__main__':
    main()
