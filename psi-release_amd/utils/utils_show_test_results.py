#!/usr/bin/env python
"""python utils_show_test_results.py GEN_FOLDER SCENE_PLY OUT_DIR

The captured images of utils/utils_show_test_results.py and utils_show_test_results_habitat.py, on the GPU and without a window: every
body of GEN_FOLDER/body_gen_*.pkl drawn, shaded, into the scene mesh SCENE_PLY ('-': no scene, bodies over the background) as
OUT_DIR/img_%06d_cam1.png from the body's own camera — the matrix the reference transforms the body with, cam_ext . T_mat for Habitat
trees (utils_show_test_results_habitat.py:261-265, 289), cam_ext with --no_flip for PROX-E — and with --fixed_cam as img_%06d_cam2.png
from that overview camera; --together adds img_together.png, all bodies from the fixed camera.  OUT_DIR/visibility.json lists, per
body, the pixels it covers and the pixels of those that the scene does not hide.  With --disjoint [MAX_INSIDE] (it needs --together)
img_together.png draws only the greedy set of bodies that do not stand in each other (evaluation.BodyOverlap and select_disjoint in file
order; MAX_INSIDE vertices, default 0, are tolerated per pair), and every row of visibility.json gains ``inside_others``, the number of
the body's vertices inside other bodies, and ``disjoint``, whether it was drawn.  With --scene_crossings (it needs a scene mesh) every row of
visibility.json gains ``scene_crossings``, the pairs of a body triangle and a scene triangle that intersect, and ``scene_contour``, the
length of their contour in metres (evaluation.SceneCrossings: the mesh itself, no distance volume).  The reference's interactive window is
not included."""
import argparse
import json
import os

import _eval_common as C
import numpy as np
import torch


def habitat_flip():
    """T_mat of utils_show_test_results_habitat.py:261-263: the Habitat camera looks along -z with y up."""
    T = np.eye(4)
    T[1, :] = [0, -1, 0, 0]
    T[2, :] = [0, 0, -1, 0]
    return T


def camera_pose(cam_ext, no_flip):
    """Camera-to-world pose(s) of the picture: cam_ext . T_mat, or cam_ext itself for PROX-E trees."""
    cam_ext = np.asarray(cam_ext, np.float64)
    return cam_ext if no_flip else cam_ext @ habitat_flip()


def fixed_camera(values):
    """--fixed_cam: 16 numbers, row by row, or one .npy file with a [4,4] camera-to-world matrix."""
    if len(values) == 1:
        return np.asarray(np.load(values[0]), np.float64).reshape(4, 4)
    return np.array([float(v) for v in values], np.float64).reshape(4, 4)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('gen_folder')
    ap.add_argument('scene_ply')
    ap.add_argument('out_dir')
    ap.add_argument('--size', type=int, nargs=2, default=[540, 960], metavar=('H', 'W'))
    ap.add_argument('--fixed_cam', nargs='+', default=None, metavar='M', help='camera-to-world pose of the overview camera: 16 numbers or a .npy')
    ap.add_argument('--together', action='store_true', help='also one image of all bodies from the fixed camera')
    ap.add_argument('--disjoint', type=int, nargs='?', const=0, default=None, metavar='MAX_INSIDE',
                    help='with --together: draw only bodies that do not stand in each other; MAX_INSIDE vertices are tolerated per pair')
    ap.add_argument('--no_flip', action='store_true', help='PROX-E trees: no Habitat camera flip')
    ap.add_argument('--pack', type=int, default=64, help='bodies per render call')
    ap.add_argument('--near', type=float, default=0.05)
    ap.add_argument('--max_files', type=int, default=8000)
    ap.add_argument('--human_model_path', default='/is/ps2/yzhang/body_models/VPoser')
    ap.add_argument('--vposer_ckpt_path', default='/is/ps2/yzhang/body_models/VPoser/vposer_v1_0')
    ap.add_argument('--synthetic', default=None, help="stand-in body model and VPoser; with SCENE_PLY '-' also a stand-in room, written to DIR/room.ply")
    ap.add_argument('--scene_crossings', action='store_true', help='also count, per body, the triangle pairs of the body and the scene mesh that intersect')
    a = ap.parse_args(argv)
    if a.scene_crossings and a.scene_ply == '-' and not a.synthetic:
        ap.error('--scene_crossings needs a scene mesh')
    if a.fixed_cam is not None and len(a.fixed_cam) not in (1, 16):
        ap.error('--fixed_cam takes 16 numbers or one .npy file')
    if a.together and a.fixed_cam is None:
        ap.error('--together needs --fixed_cam')
    if a.disjoint is not None and not a.together:
        ap.error('--disjoint needs --together')
    if a.disjoint is not None and a.disjoint < 0:
        ap.error('--disjoint MAX_INSIDE must not be negative')
    if a.pack < 1:
        ap.error('--pack must be at least 1')
    return a


class BodyDecoder:
    """body_gen rows -> world-frame vertices on the GPU: the ``op.body_verts`` path of evaluation.py without a scene."""

    def __init__(self, smplx_src, vposer_src, device):
        from psi_release_amd import body_model
        from psi_release_amd.geometry import BodyParamParser
        from psi_release_amd.vposer import load_vposer
        BodyParamParser.device = device
        self.device = device
        self.vposer, _ = load_vposer(vposer_src, vp_model='snapshot')
        self.vposer.to(device)
        self.model = body_model.create(smplx_src, model_type='smplx', gender='neutral', ext='npz', num_pca_comps=12, create_global_orient=True,
                                       create_body_pose=True, create_betas=True, create_left_hand_pose=True, create_right_hand_pose=True,
                                       create_expression=True, create_jaw_pose=True, create_leye_pose=True, create_reye_pose=True,
                                       create_transl=True, batch_size=1, device=device)
        self.faces = self.model.faces_tensor

    @torch.no_grad()
    def verts(self, xh72, pose):
        from psi_release_amd.geometry import BodyParamParser, GeometryTransformer
        xh = torch.as_tensor(xh72, dtype=torch.float32, device=self.device).reshape(-1, 72)
        cam = torch.as_tensor(np.asarray(pose, np.float32), device=self.device).reshape(-1, 4, 4).contiguous()
        xh_rec = GeometryTransformer.convert_to_3D_rot(GeometryTransformer.convert_to_6D_rot(xh))
        par = BodyParamParser.body_params_encapsulate_batch(xh_rec)
        par['body_pose'] = self.vposer.decode(par.pop('body_pose_vp'), output_type='aa').view(xh.shape[0], -1)
        return self.model(return_verts=True, cam_ext=cam, **par).vertices


def main(argv=None):
    a = parse_args(argv)
    from psi_release_amd import rendering, synth
    from psi_release_amd.evaluation import PlausibilityEvaluator
    from psi_release_amd.scene_io import write_ply_mesh
    device = torch.device('cuda', torch.cuda.current_device())
    smplx_src, vposer_src = a.human_model_path, a.vposer_ckpt_path
    if a.synthetic:
        smplx_src, vposer_src = synth.make_smplx(7), synth.make_vposer_state(3)
        if a.scene_ply == '-':
            room = synth.make_room_mesh(0, 180)
            os.makedirs(a.synthetic, exist_ok=True)
            a.scene_ply = os.path.join(a.synthetic, 'room.ply')
            write_ply_mesh(a.scene_ply, room.verts, room.faces, room.rgb())
    xh, cam = PlausibilityEvaluator._read_folder(a.gen_folder, a.max_files)
    if not len(xh):
        raise SystemExit('no body_gen_*.pkl in %s' % a.gen_folder)
    pose = camera_pose(cam, a.no_flip)
    H, W = a.size
    f = (H / 2) / np.tan(np.radians(30.0))                   # 60 degrees vertical field of view, the window's default
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    decoder = BodyDecoder(smplx_src, vposer_src, device)
    scene = None if a.scene_ply == '-' else rendering.SceneMesh.from_ply(a.scene_ply, device=device)
    renderer = rendering.ResultRenderer(scene, decoder.faces, device=device)
    fixed = None if a.fixed_cam is None else fixed_camera(a.fixed_cam)
    os.makedirs(a.out_dir, exist_ok=True)
    report, all_verts = [], []
    scene_crossings = None
    if a.scene_crossings:
        from psi_release_amd.evaluation import SceneCrossings
        scene_crossings = SceneCrossings(scene, None, decoder.faces, device)
    for lo in range(0, len(xh), a.pack):
        hi = min(len(xh), lo + a.pack)
        verts = decoder.verts(xh[lo:hi], pose[lo:hi])
        shots = [('cam1', renderer.render(verts, pose[lo:hi], K, (H, W), near=a.near))]
        if fixed is not None:
            shots.append(('cam2', renderer.render(verts, np.repeat(fixed[None], hi - lo, 0), K, (H, W), near=a.near)))
            all_verts.append(verts)
        rows = [{'body': i} for i in range(lo, hi)]
        for name, res in shots:
            rgb, counts = res.rgb.cpu().numpy(), res.counts.cpu().numpy()
            for i in range(lo, hi):
                rendering.write_png(os.path.join(a.out_dir, 'img_%06d_%s.png' % (i, name)), rgb[i - lo])
                rows[i - lo][name] = {'covered': int(counts[i - lo, 0]), 'visible': int(counts[i - lo, 1])}
        if scene_crossings is not None:
            sres = scene_crossings.crossings(verts)
            for row, n, length in zip(rows, sres.counts.cpu().tolist(), sres.contour.cpu().tolist()):
                row['scene_crossings'], row['scene_contour'] = int(n), float(length)
        report += rows
    if a.together:
        verts = torch.cat(all_verts)
        drawn = np.arange(len(verts))
        if a.disjoint is not None:
            from psi_release_amd.evaluation import BodyOverlap, select_disjoint
            overlap = BodyOverlap(decoder.faces, device).counts(verts)
            drawn = np.array(select_disjoint(range(len(verts)), overlap.counts, a.disjoint), np.int64)
            for row, n_in in zip(report, overlap.per_body.cpu().tolist()):
                row['inside_others'], row['disjoint'] = int(n_in), bool(row['body'] in drawn)
        res = renderer.render(verts, fixed[None], K, (H, W), draw_body=drawn, draw_view=np.zeros(len(drawn), np.int64), near=a.near)
        rendering.write_png(os.path.join(a.out_dir, 'img_together.png'), res.rgb[0])
        for b, c in zip(drawn.tolist(), res.counts.cpu().numpy()):
            report[b]['together'] = {'covered': int(c[0]), 'visible': int(c[1])}
    with open(os.path.join(a.out_dir, 'visibility.json'), 'w') as fjson:
        json.dump(report, fjson, indent=1)
    print('[INFO] wrote %d bodies to %s' % (len(report), a.out_dir))


if __name__ == '__main__':
    main()
