#!/usr/bin/env python
"""fwd_scene and bwd_joint of the fused fitting engine at the BASELINE shape (B = 32, V = 10475, n_c = 2048, m = 32768, 256^3) against the
share of penetrating vertices, with the penetration-mask skip of fit_bwd_joint_kernel and without it (PSI_FIT_PEN_SKIP=0)
-> one JSON (profiles/pen_skip_by_share.json).

    python tools/time_pen_share.py [--out FILE] [--rounds 5] [--rep 20]
    python tools/time_pen_share.py --libs parent=PATH new=PATH,PSI_FIT_BWD_PF=1 ... [--passes 2]     (builds against each other)

Scenes: nothing penetrates (a room wider than the volume), the default room at iteration 0 (about a fifth of the vertices, scattered over
the model's random vertex order), everything penetrates (a ball that swallows the volume).  Times are the engine's own per-kernel HIP-event
times (psi_fit_profile, ungraphed launches) in microseconds.  The first and the last scene keep their share over the iterations: one
reading is the average of --rep iterations.  The default room is dense only in its first iteration: one reading is the median of --rep
single-iteration profiles, each after a restart of the loop.  The two arms are two engines in one process, read alternately, --rounds
readings each; the spread (max - min) / median of an arm's readings is reported next to its median.

--libs: the arms are LIBRARIES (PSI_HIP_LIB, a process loads one) with the skip on, optionally with environment knobs: one child process
per arm and pass, the arms in turn, --passes times, --rounds readings per child; a fourth scene is read, the default room 40 iterations
into the loop (sparse, but a few slices still hold a penetrating vertex: what most iterations of a fit look like).  A child that does not
end with status 0 ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psi_release_amd import fitting, synth  # noqa: E402

DEV = torch.device('cuda')
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
B, M, D, NC = 32, 32768, 256, 2048
KERNELS = ('fwd_scene_kernel', 'bwd_joint_kernel')


def runner(smplx, vposer, scene, skip):
    if skip:
        os.environ.pop('PSI_FIT_PEN_SKIP', None)
    else:
        os.environ['PSI_FIT_PEN_SKIP'] = '0'                  # read once, when the engine is created
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.1,
           'num_iter': 1, 'batch_size': B, 'device': DEV, 'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': smplx, 'vposer_state': vposer, 'engine': 'fused', 'scene': scene}
    op = fitting.FittingOP(cfg, dict(LOSS))
    bodies = synth.make_bodies(12, B)
    r = op.make_step_runner(bodies)
    r.steps(2)
    torch.cuda.synchronize()
    os.environ.pop('PSI_FIT_PEN_SKIP', None)
    return r


def share(r):
    """share of (body, vertex) bits set in the mask of the last forward"""
    Vpad = (10475 + 255) // 256 * 256
    w = r.eng.buffer('penmask', (B, Vpad // 64 * 2)).cpu().numpy().view(np.uint64)
    return float(sum(bin(int(x)).count('1') for x in w.ravel())) / (B * 10475)


def reading(r, first_iteration_only, rep):
    if first_iteration_only == 'late':
        r.restart()
        r.steps(40)
    if first_iteration_only is not True:
        t = dict(r.eng.profile(rep))
        return {k: t[k] * 1e3 for k in KERNELS}, share(r)
    rows, sh = [], 0.0
    for _ in range(rep):
        r.restart()
        t = dict(r.eng.profile(1))
        rows.append([t[k] * 1e3 for k in KERNELS])
        sh = share(r)
    return {k: statistics.median(row[i] for row in rows) for i, k in enumerate(KERNELS)}, sh


def scene_list(with_late):
    scenes = [('nothing', dict(kind='room', radius=10.0), False), ('default_room_iteration_0', {}, True),
              ('everything', dict(kind='sphere', radius=50.0), False)]
    return scenes + ([('default_room_iteration_40', {}, 'late')] if with_late else [])


def child(args):
    """one library (this process's), skip on: --rounds readings per scene -> one line 'READINGS <json>' per scene"""
    smplx, vposer = synth.make_smplx(7), synth.make_vposer_state(3)
    for name, kw, first_only in scene_list(True):
        r = runner(smplx, vposer, synth.make_scene(0, M, D, NC, **kw), True)
        reading(r, first_only, 2)
        got, shares = {k: [] for k in KERNELS}, []
        for _ in range(args.rounds):
            t, sh = reading(r, first_only, args.rep)
            shares.append(sh)
            for k in KERNELS:
                got[k].append(t[k])
        print('READINGS ' + json.dumps({'scene': name, 'share': statistics.median(shares), 'readings': got}), flush=True)
        del r
        torch.cuda.empty_cache()


def compare_libs(args):
    arms = []
    for spec in args.libs:
        name, rest = spec.split('=', 1)
        parts = rest.split(',')
        arms.append((name, os.path.abspath(parts[0]), dict(p.split('=', 1) for p in parts[1:])))
    got = {}
    for _ in range(args.passes):
        for name, lib, env in arms:
            e = dict(os.environ, PSI_HIP_LIB=lib, **env)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--rounds', str(args.rounds), '--rep', str(args.rep)],
                               env=e, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit('arm %s: child ended with status %d\n%s' % (name, p.returncode, p.stderr[-2000:]))
            for line in p.stdout.splitlines():
                if line.startswith('READINGS '):
                    d = json.loads(line[9:])
                    slot = got.setdefault(d['scene'], {}).setdefault(name, {'share': [], **{k: [] for k in KERNELS}})
                    slot['share'].append(d['share'])
                    for k in KERNELS:
                        slot[k] += d['readings'][k]
    out = {'shape': {'B': B, 'V': 10475, 'n_c': NC, 'm': M, 'D': D}, 'unit': 'us per launch (HIP events, psi_fit_profile)',
           'rounds': args.rounds, 'rep': args.rep, 'passes': args.passes,
           'arms': {name: {'lib': os.path.relpath(lib, ROOT), 'env': env} for name, lib, env in arms}, 'scenes': {}}
    for scene, by_arm in got.items():
        res = {}
        for name, slot in by_arm.items():
            res[name] = {'penetrating_share': round(statistics.median(slot['share']), 4)}
            for k in KERNELS:
                v = slot[k]
                med = statistics.median(v)
                res[name][k] = {'median_us': round(med, 2), 'spread': round((max(v) - min(v)) / med, 4), 'readings_us': [round(x, 2) for x in v]}
        out['scenes'][scene] = res
        print(scene, json.dumps({a: {k: res[a][k]['median_us'] for k in KERNELS} for a in res}), flush=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pen_skip_by_share.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--rep', type=int, default=20)
    ap.add_argument('--libs', nargs='+', metavar='NAME=LIB[,ENV=VALUE...]')
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.libs:
        return compare_libs(args)
    smplx, vposer = synth.make_smplx(7), synth.make_vposer_state(3)
    scenes = [(name, synth.make_scene(0, M, D, NC, **kw), first_only) for name, kw, first_only in scene_list(False)]
    out = {'shape': {'B': B, 'V': 10475, 'n_c': NC, 'm': M, 'D': D}, 'unit': 'us per launch (HIP events, psi_fit_profile)',
           'rounds': args.rounds, 'rep': args.rep, 'scenes': {}}
    for name, scene, first_only in scenes:
        arms = {'skip': runner(smplx, vposer, scene, True), 'off': runner(smplx, vposer, scene, False)}
        got = {a: {k: [] for k in KERNELS} for a in arms}
        shares = []
        for a in arms:                                         # one untimed reading each: clocks, caches
            reading(arms[a], first_only, 2)
        for _ in range(args.rounds):
            for a in arms:
                t, sh = reading(arms[a], first_only, args.rep)
                shares.append(sh)
                for k in KERNELS:
                    got[a][k].append(t[k])
        res = {'penetrating_share': round(statistics.median(shares), 4)}
        for a in arms:
            for k in KERNELS:
                v = got[a][k]
                med = statistics.median(v)
                res['%s_%s' % (a, k)] = {'median_us': round(med, 2), 'spread': round((max(v) - min(v)) / med, 4), 'readings_us': [round(x, 2) for x in v]}
        out['scenes'][name] = res
        print(name, json.dumps(res), flush=True)
        del arms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
