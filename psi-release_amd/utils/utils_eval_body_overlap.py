#!/usr/bin/env python
"""python utils_eval_body_overlap.py GEN_FOLDER [--human_model_path ... --vposer_ckpt_path ... | --synthetic DIR] [--no_flip]
                                                 [--max_inside 0] [--out JSON]

Which bodies of GEN_FOLDER/body_gen_*.pkl stand in each other: every body is placed as utils_show_test_results.py places it (cam_ext .
T_mat for Habitat trees, cam_ext with --no_flip for PROX-E), and every vertex of every body is tested against every other body
(evaluation.BodyOverlap; the test is vertex-in-body and asymmetric).  Prints the number of overlapping pairs, the bodies ranked by the
number of their vertices inside others, and the greedy set of mutually compatible bodies in file order (evaluation.select_disjoint with
--max_inside); --out writes all of that as JSON.  The reference tree has no counterpart (its BodyInterpenetration needs an external CUDA
package)."""
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
    a = ap.parse_args(argv)
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
    res = overlap.counts_of_records(xh, camera_pose(cam, a.no_flip), decoder, chunk=a.chunk)
    rep = report_of(res.counts.cpu().numpy(), res.per_body.cpu().numpy(), a.max_inside)
    print('[INFO] %d bodies, %d overlapping pairs' % (rep['bodies'], rep['overlapping_pairs']))
    for i in rep['ranked']:
        print('body %6d: %6d vertices inside other bodies' % (i, rep['per_body'][i]))
    print('--disjoint=' + ','.join(str(i) for i in rep['disjoint']))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rep, f, indent=1)
    return rep


if __name__ == '__main__':
    main()
