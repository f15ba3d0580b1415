#!/usr/bin/env python
"""python utils_eval_body_overlap.py GEN_FOLDER [--human_model_path ... --vposer_ckpt_path ... | --synthetic DIR] [--no_flip]
                                                 [--max_inside 0] [--out JSON] [--crossings [--self] [--parts] [--field [--sigma S]]]
                                                 [--depth [--tol M]] [--scene_mesh PLY [--max_scene_pairs 0]]

Which bodies of GEN_FOLDER/body_gen_*.pkl stand in each other: every body is placed as utils_show_test_results.py places it (cam_ext .
T_mat for Habitat trees, cam_ext with --no_flip for PROX-E), and every vertex of every body is tested against every other body
(evaluation.BodyOverlap; the test is vertex-in-body and asymmetric).  Prints the number of overlapping pairs, the bodies ranked by the
number of their vertices inside others, and the greedy set of mutually compatible bodies in file order (evaluation.select_disjoint with
--max_inside); --out writes all of that as JSON.  The reference tree has no counterpart (its BodyInterpenetration needs an external CUDA
package).

--crossings adds the test of the surfaces themselves (evaluation.SurfaceCrossings: which pairs of triangles intersect): the crossing pairs
of every pair of bodies with the length of their contour, the number of irregular pairs, and how many pairs of bodies cross although no
vertex of either is inside the other.  --self also tests every body against itself and ranks the bodies by self crossings; --parts
then ignores pairs of faces of the same body part, of a part and its kinematic parent and of the pairs of parts
human_body_prior/body_model/body_model.py:488 lists, the parts taken from the model's own skinning weights and kinematic tree.  Without
--crossings every printed line and every JSON field is what it was.

--crossings --field adds the conic distance field over the crossing pairs (evaluation.SurfaceCrossings.field): the
energy of every pair of bodies that cross, both ways, the bodies ranked by their loss and, with --self, the energy of every body against
itself.  --sigma is the height of the cones (default 1e-3, the reference's; SMPLify-X uses 0.5).  Without --field every printed line and
every JSON field is what it was.

--depth adds how far in the vertices are (evaluation.BodyOverlap.depths: the distance of every inside vertex to the nearest triangle of
the body it is in): the largest and the mean depth of every overlapping ordered pair, the bodies ranked by their deepest vertex, and the
greedy set of bodies that stand no deeper than --tol metres in each other (evaluation.select_shallow, in file order).  Without --depth
every printed line and every JSON field is what it was.

--scene_mesh PLY adds the bodies against the room's mesh itself (evaluation.SceneCrossings, DESIGN.md section 10i: which body triangles
cut which scene triangles, with no distance volume, so a table top thinner than the volume's node spacing is seen): per body the crossing
pairs and the contour length, the bodies ranked by contour, the irregular pairs, the crossed scene triangles and the bodies that stand
clear in file order (evaluation.select_clear with --max_scene_pairs).  With --synthetic, --scene_mesh - is the stand-in room
synth.make_room_mesh().  Without --scene_mesh every printed line and every JSON field is what it was."""
import argparse
import json

import _eval_common as C  # noqa: F401  (path setup)
import numpy as np
import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('gen_folder')
    ap.add_argument('--human_model_path', default='/is/ps2/yzhang/body_models/VPoser')
    ap.add_argument('--vposer_ckpt_path', default='/is/ps2/yzhang/body_models/VPoser/vposer_v1_0')
    ap.add_argument('--synthetic', default=None, metavar='DIR', help='stand-in body model and VPoser')
    ap.add_argument('--no_flip', action='store_true', help='PROX-E trees: no Habitat camera flip')
    ap.add_argument('--max_inside', type=int, default=0, help='vertices two kept bodies may have inside each other, both ways together')
    ap.add_argument('--max_files', type=int, default=8000)
    ap.add_argument('--chunk', type=int, default=512, help='bodies per skinning call')
    ap.add_argument('--out', default=None, metavar='JSON')
    ap.add_argument('--crossings', action='store_true', help='also list the pairs of triangles of the surfaces that intersect')
    ap.add_argument('--self', dest='self_pairs', action='store_true', help='with --crossings: also every body against itself')
    ap.add_argument('--parts', action='store_true', help='with --crossings --self: ignore pairs of faces of adjacent body parts')
    ap.add_argument('--field', action='store_true', help='with --crossings: the conic distance-field energy of the crossing pairs')
    ap.add_argument('--sigma', type=float, default=None, metavar='S', help='with --field: the height of the cones, in (0, 0.5]; default 1e-3')
    ap.add_argument('--depth', action='store_true', help='also report how deep the inside vertices are')
    ap.add_argument('--tol', type=float, default=0.0, metavar='M', help='with --depth: the depth two kept bodies may reach in each other, in metres')
    ap.add_argument('--scene_mesh', default=None, metavar='PLY', help="also test the bodies against this scene mesh ('-' with --synthetic: the stand-in room)")
    ap.add_argument('--max_scene_pairs', type=int, default=0, help='with --scene_mesh: scene crossings a body of the clear set may have')
    a = ap.parse_args(argv)
    if a.scene_mesh == '-' and not a.synthetic:
        ap.error('--scene_mesh - needs --synthetic')
    if a.max_scene_pairs != 0 and not a.scene_mesh:
        ap.error('--max_scene_pairs needs --scene_mesh')
    if a.max_scene_pairs < 0:
        ap.error('--max_scene_pairs must not be negative')
    if a.tol != 0.0 and not a.depth:
        ap.error('--tol needs --depth')
    if not a.tol >= 0.0:
        ap.error('--tol must not be negative')
    if a.self_pairs and not a.crossings:
        ap.error('--self needs --crossings')
    if a.parts and not a.self_pairs:
        ap.error('--parts needs --crossings --self')
    if a.field and not a.crossings:
        ap.error('--field needs --crossings')
    if a.sigma is not None and not a.field:
        ap.error('--sigma needs --crossings --field')
    if a.sigma is None:
        a.sigma = 1e-3
    if not 0.0 < a.sigma <= 0.5:
        ap.error('--sigma must lie in (0, 0.5]')
    if a.max_inside < 0:
        ap.error('--max_inside must not be negative')
    if a.chunk < 1:
        ap.error('--chunk must be at least 1')
    return a


def report_of(counts, per_body, max_inside):
    """The JSON document: counts [B,B] and per_body [B] as host integers."""
    from psi_release_amd.evaluation import select_disjoint
    counts, per_body = np.asarray(counts, np.int64), np.asarray(per_body, np.int64)
    B = len(per_body)
    pairs = [[i, j, int(counts[i, j]), int(counts[j, i])] for i in range(B) for j in range(i + 1, B) if counts[i, j] or counts[j, i]]
    ranked = sorted(range(B), key=lambda i: (-int(per_body[i]), i))
    return {'bodies': B, 'overlapping_pairs': len(pairs), 'pairs': pairs, 'counts': counts.tolist(), 'per_body': per_body.tolist(),
            'ranked': ranked, 'max_inside': int(max_inside), 'disjoint': select_disjoint(range(B), counts, max_inside)}


def model_parts(smplx_src, faces):
    """(face_part [F], part_skip [P,P]) from the model's own ``weights`` and ``kintree_table``; ``smplx_src`` as body_model.create takes it."""
    import os
    from psi_release_amd import body_model
    from psi_release_amd.evaluation import SMPLX_SELF_CONTACT_PAIRS, face_parts, part_skip_matrix
    data = smplx_src
    if not (isinstance(data, dict) or hasattr(data, 'v_template')):
        p = smplx_src
        if os.path.isdir(p):
            cand = os.path.join(p, 'smplx', 'SMPLX_NEUTRAL.npz')
            p = cand if os.path.exists(cand) else os.path.join(p, 'SMPLX_NEUTRAL.npz')
        data = body_model.load_smplx_npz(p)
    g = (lambda k: np.asarray(data[k])) if not hasattr(data, 'v_template') else (lambda k: np.asarray(getattr(data, k)))
    parents = g('kintree_table')[0].astype(np.int64).copy()
    parents[0] = -1
    extra = [pr for pr in SMPLX_SELF_CONTACT_PAIRS if max(pr) < len(parents)]
    return face_parts(g('weights'), faces), part_skip_matrix(parents, extra=extra), g('v_template').astype(np.float32)


def crossings_report(res, overlap_counts):
    """The JSON fields of --crossings: ``res`` a CrossingsResult, ``overlap_counts`` [B,B] the vertex-in-body counts."""
    counts, contour = res.counts.cpu().numpy().astype(np.int64), res.contour.cpu().numpy()
    ov = np.asarray(overlap_counts, np.int64)
    B = len(counts)
    pairs = [[i, j, int(counts[i, j]), float(contour[i, j])] for i in range(B) for j in range(i + 1, B) if counts[i, j]]
    own = np.diag(counts)
    return {'crossing_pairs': pairs, 'crossing_counts': counts.tolist(), 'contour': contour.tolist(),
            'self_crossings': own.tolist(), 'self_ranked': sorted(range(B), key=lambda i: (-int(own[i]), i)),
            'irregular': int(res.irregular.item()), 'triangle_pairs': int(res.pairs.shape[0]),
            'unseen_by_vertex_test': sum(1 for i, j, _, _ in pairs if ov[i, j] == 0 and ov[j, i] == 0)}


def field_report(pair_energy, loss, crossing_counts, with_self):
    """The JSON fields of --field: pair_energy [B,B] fp64 (not symmetric), loss [B] and the crossing counts [B,B], as host arrays."""
    E, loss, counts = np.asarray(pair_energy, np.float64), np.asarray(loss, np.float32), np.asarray(crossing_counts, np.int64)
    B = len(loss)
    rep = {'field_pairs': [[i, j, float(E[i, j]), float(E[j, i])] for i in range(B) for j in range(i + 1, B) if counts[i, j]],
           'field_loss': loss.astype(np.float64).tolist(), 'field_ranked': sorted(range(B), key=lambda i: (-float(loss[i]), i))}
    if with_self:
        rep['self_energy'] = np.diag(E).tolist()
    return rep


def depth_report(max_depth, sum_depth, counts, depth_of, tol):
    """The JSON fields of --depth: max_depth, sum_depth and counts [B,B], depth_of [B,V], as host arrays."""
    from psi_release_amd.evaluation import select_shallow
    max_depth, sum_depth, counts = np.asarray(max_depth, np.float32), np.asarray(sum_depth, np.float64), np.asarray(counts, np.int64)
    B = len(counts)
    deepest = np.asarray(depth_of, np.float32).max(1)
    pairs = [[i, j, float(max_depth[i, j]), float(sum_depth[i, j] / counts[i, j])] for i in range(B) for j in range(B) if counts[i, j]]
    return {'depth_pairs': pairs, 'max_depth': max_depth.astype(np.float64).tolist(), 'deepest': deepest.astype(np.float64).tolist(),
            'deepest_ranked': sorted(range(B), key=lambda i: (-float(deepest[i]), i)), 'tol': float(tol),
            'shallow': select_shallow(range(B), max_depth, tol)}


def scene_report(res, max_pairs):
    """The JSON fields of --scene_mesh: ``res`` a SceneCrossingsResult."""
    from psi_release_amd.evaluation import select_clear
    counts, contour = res.counts.cpu().numpy().astype(np.int64), res.contour.cpu().numpy()
    B = len(counts)
    return {'scene_crossings': counts.tolist(), 'scene_contour': contour.tolist(),
            'scene_ranked': sorted(range(B), key=lambda i: (-float(contour[i]), i)), 'scene_irregular': int(res.irregular.item()),
            'scene_triangle_pairs': int(res.pairs.shape[0]), 'scene_triangles_crossed': int(res.tri_hit.sum().item()),
            'max_scene_pairs': int(max_pairs), 'clear': select_clear(range(B), counts, max_pairs)}


def main(argv=None):
    a = parse_args(argv)
    from psi_release_amd import synth
    from psi_release_amd.evaluation import BodyOverlap, PlausibilityEvaluator
    from utils_show_test_results import BodyDecoder, camera_pose
    device = torch.device('cuda', torch.cuda.current_device())
    smplx_src, vposer_src = a.human_model_path, a.vposer_ckpt_path
    if a.synthetic:
        smplx_src, vposer_src = synth.make_smplx(7), synth.make_vposer_state(3)
    xh, cam = PlausibilityEvaluator._read_folder(a.gen_folder, a.max_files)
    if not len(xh):
        raise SystemExit('no body_gen_*.pkl in %s' % a.gen_folder)
    decoder = BodyDecoder(smplx_src, vposer_src, device)
    overlap = BodyOverlap(decoder.faces, device)
    if a.depth:
        pen = overlap.depths_of_records(xh, camera_pose(cam, a.no_flip), decoder, chunk=a.chunk)
        rep = report_of(pen.counts.cpu().numpy(), pen.inside.sum(1).cpu().numpy(), a.max_inside)
    else:
        res = overlap.counts_of_records(xh, camera_pose(cam, a.no_flip), decoder, chunk=a.chunk)
        rep = report_of(res.counts.cpu().numpy(), res.per_body.cpu().numpy(), a.max_inside)
    print('[INFO] %d bodies, %d overlapping pairs' % (rep['bodies'], rep['overlapping_pairs']))
    for i in rep['ranked']:
        print('body %6d: %6d vertices inside other bodies' % (i, rep['per_body'][i]))
    print('--disjoint=' + ','.join(str(i) for i in rep['disjoint']))
    if a.crossings:
        from psi_release_amd.evaluation import SurfaceCrossings
        part, skip, rest = model_parts(smplx_src, decoder.faces.cpu().numpy()) if a.parts else (None, None, None)
        sc = SurfaceCrossings(decoder.faces, device, order_verts=rest, face_part=part, part_skip=skip)
        if a.field:
            fres = sc.field_of_records(xh, camera_pose(cam, a.no_flip), decoder, chunk=a.chunk, self_pairs=a.self_pairs, sigma=a.sigma)
            cres = fres.crossings
        else:
            cres = sc.crossings_of_records(xh, camera_pose(cam, a.no_flip), decoder, chunk=a.chunk, self_pairs=a.self_pairs)
        crep = crossings_report(cres, rep['counts'])
        rep.update(crep)
        print('[INFO] %d pairs of bodies cross, %d pairs of triangles (%d irregular)' % (len(crep['crossing_pairs']), crep['triangle_pairs'],
                                                                                       crep['irregular']))
        for i, j, n, length in crep['crossing_pairs']:
            print('bodies %6d %6d: %6d crossing pairs, contour %.4f m' % (i, j, n, length))
        if a.self_pairs:
            for i in crep['self_ranked']:
                print('body %6d: %6d self crossings' % (i, crep['self_crossings'][i]))
        print('[INFO] %d pairs of bodies cross although no vertex of either is inside the other' % crep['unseen_by_vertex_test'])
        if a.field:
            frep = field_report(fres.pair_energy.cpu().numpy(), fres.loss.cpu().numpy(), crep['crossing_counts'], a.self_pairs)
            rep.update(frep)
            rep['sigma'] = float(a.sigma)
            for i, j, e_ij, e_ji in frep['field_pairs']:
                print('bodies %6d %6d: field energy %.6g of the first in the second, %.6g of the second in the first' % (i, j, e_ij, e_ji))
            for i in frep['field_ranked']:
                print('body %6d: field loss %.6g' % (i, frep['field_loss'][i]))
            if a.self_pairs:
                for i in range(rep['bodies']):
                    print('body %6d: self energy %.6g' % (i, frep['self_energy'][i]))
    if a.depth:
        drep = depth_report(pen.max_depth.cpu().numpy(), pen.sum_depth.cpu().numpy(), rep['counts'], pen.depth_of.cpu().numpy(), a.tol)
        rep.update(drep)
        for i, j, mx, mean in drep['depth_pairs']:
            print('body %6d in %6d: deepest %.4f m, mean %.4f m' % (i, j, mx, mean))
        for i in drep['deepest_ranked']:
            print('body %6d: deepest vertex %.4f m' % (i, drep['deepest'][i]))
        print('--shallow=' + ','.join(str(i) for i in drep['shallow']))
    if a.scene_mesh:
        from psi_release_amd import scene_io
        from psi_release_amd.evaluation import SceneCrossings
        if a.scene_mesh == '-':
            room = synth.make_room_mesh()
            sverts, sfaces = room.verts, room.faces
        else:
            sverts, sfaces, _ = scene_io.read_ply_mesh(a.scene_mesh)
        scn = SceneCrossings(sverts, sfaces, decoder.faces, device)
        srep = scene_report(scn.crossings_of_records(xh, camera_pose(cam, a.no_flip), decoder, chunk=a.chunk), a.max_scene_pairs)
        rep.update(srep)
        print('[INFO] scene mesh of %d triangles: %d pairs of triangles cross (%d irregular), %d scene triangles crossed' % (
            len(sfaces), srep['scene_triangle_pairs'], srep['scene_irregular'], srep['scene_triangles_crossed']))
        for i in range(rep['bodies']):
            print('body %6d: %6d scene crossings, contour %.4f m' % (i, srep['scene_crossings'][i], srep['scene_contour'][i]))
        print('--scene_ranked=' + ','.join(str(i) for i in srep['scene_ranked']))
        print('--clear=' + ','.join(str(i) for i in srep['clear']))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rep, f, indent=1)
    return rep


if __name__ == '__main__':
    main()
