#!/usr/bin/env python
"""dev: fwd_scene of a fused fitting engine whose NN index has NO grid (PSI_NN_GRID=0: every contact query walks the tree) at the BASELINE shape
(B = 32, V = 10475, n_c = 2048, m = 32768, 256^3), per library — the cost of the walk's stack in global memory (two slices per search
workgroup) against LDS (one).

    python tools/time_search_walk.py --libs parent=PATH new=PATH new_spw1=PATH,PSI_FIT_SEARCH_SPW=1 [--passes 2] [--rounds 3] [--rep 20]

One child process per arm and pass (PSI_HIP_LIB; a process loads one library), the arms in turn; a reading is the engine's own HIP-event time
of fwd_scene_kernel (psi_fit_profile, ungraphed launches), averaged over --rep iterations 5 iterations into the loop (warm hints).  Prints
one line per arm: median, (max - min) / median, the readings.  A child that does not end with status 0 ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    from psi_release_amd import fitting, synth
    os.environ['PSI_NN_GRID'] = '0'                           # read where the index is created
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.1,
           'num_iter': 1, 'batch_size': 32, 'device': torch.device('cuda'), 'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None,
           'verbose': False, 'smplx_data': synth.make_smplx(7), 'vposer_state': synth.make_vposer_state(3), 'engine': 'fused',
           'scene': synth.make_scene(0, 32768, 256, 2048)}
    op = fitting.FittingOP(cfg, {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5})
    r = op.make_step_runner(synth.make_bodies(12, 32))
    r.steps(5)
    torch.cuda.synchronize()
    dict(r.eng.profile(2))
    print('READINGS ' + json.dumps([dict(r.eng.profile(args.rep))['fwd_scene_kernel'] * 1e3 for _ in range(args.rounds)]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--libs', nargs='+', metavar='NAME=LIB[,ENV=VALUE...]')
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--rep', type=int, default=20)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    got = {}
    for _ in range(args.passes):
        for spec in args.libs:
            name, rest = spec.split('=', 1)
            parts = rest.split(',')
            env = dict(os.environ, PSI_HIP_LIB=os.path.abspath(parts[0]), **dict(p.split('=', 1) for p in parts[1:]))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--rounds', str(args.rounds), '--rep', str(args.rep)],
                               env=env, capture_output=True, text=True, timeout=200)
            if p.returncode != 0:
                sys.exit('arm %s: child ended with status %d\n%s' % (name, p.returncode, p.stderr[-2000:]))
            for line in p.stdout.splitlines():
                if line.startswith('READINGS '):
                    got.setdefault(name, []).extend(json.loads(line[9:]))
    for name, v in got.items():
        print('%s fwd_scene_kernel without a grid: median %.2f us, spread %.4f, readings %s' % (
            name, statistics.median(v), (max(v) - min(v)) / statistics.median(v), [round(x, 2) for x in v]), flush=True)


if __name__ == '__main__':
    main()
