#!/usr/bin/env python
"""Timings of the surface-crossing search on the GPU (one JSON: profiles/surface_crossings_times.json).

    python tools/time_surface_crossings.py [--out FILE] [--bodies 32] [--seed 0] [--rounds 5] [--reps 3]
    python tools/time_surface_crossings.py --trace [--calls 10]     # the pruned call alone, a fixed number of times: the program of a
                                                                    # `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_surface_crossings.py --merge STATS_CSV [--out FILE]     # adds that trace's per-kernel averages to the JSON

The batch is that of tools/time_body_overlap.py: --bodies stand-in bodies (synth.make_capsule_mesh(68, 156): 20 904 faces) placed by
--seed in the room box, self + between, on a handle ordered along the rest pose.  Three arms on the same batch:

    pruned  evaluation.SurfaceCrossings.crossings (body-box and chunk-box culling), device events
    brute   the same with mode='brute': every chunk pair of every pair of bodies is a tile
    torch   a plain torch composition of the same rule on the same face-box candidates (fp32, one tensor per operation)

The arms alternate over --rounds rounds (median and spread).  Reported: tiles kept of tiles possible, the (pair, box) tests executed
(counted from the tile table) and the predicate evaluations (the candidates, counted by the torch arm) in all and per second, and
FLOPS_PER_PREDICATE, the additions and multiplications of the fifteen values as written, against the fp32 vector rate of the MI355X."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from time_body_overlap import make_batch, summary  # noqa: E402

KERNELS = ('sc_chunk_box_kernel', 'sc_body_box_kernel', 'sc_tile_kernel', 'sc_test_kernel', 'sc_finish_kernel', 'sc_contour_kernel')
# two normals (6 differences, 9 each), six plane values (3 + 5 each), six edge vectors (3 each), nine edge values (9 + 3 + 5 each)
FLOPS_PER_PREDICATE = 2 * (6 + 9) - 6 + 6 + 6 * 8 + 6 * 3 + 9 * 17
FLOPS_PER_BOX_TEST = 6
PEAK_FP32_VECTOR = 157.3e12                               # MI355X, FLOP/s


def _cross(a, b):
    import torch
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def torch_candidates(torch, verts, faces, rows=1024):
    """[n,4] int64 (i, s, j, t): the face-box candidates of the rule, self + between, for the pairs of bodies whose boxes meet."""
    B, F = verts.shape[0], faces.shape[0]
    tri = verts[:, faces.long()]
    lo, hi = tri.min(2).values, tri.max(2).values
    blo, bhi = verts.min(1).values, verts.max(1).values
    ar = torch.arange(F, device=verts.device)
    out = []
    for i in range(B):
        for j in range(i, B):
            if not bool(((blo[i] <= bhi[j]) & (blo[j] <= bhi[i])).all()):
                continue
            for r0 in range(0, F, rows):
                a = slice(r0, min(F, r0 + rows))
                meet = ((lo[i, a, None] <= hi[j, None]) & (lo[j, None] <= hi[i, a, None])).all(-1)
                if i == j:
                    share = (faces[a, None, :, None] == faces[None, :, None, :]).flatten(2).any(-1)
                    meet &= ~share & (ar[a, None] < ar[None])
                s, t = torch.nonzero(meet, as_tuple=True)
                out.append(torch.stack([torch.full_like(s, i), s + r0, torch.full_like(s, j), t], 1))
    return torch.cat(out)


def torch_arm(torch, verts, faces, cand):
    """events [n] of the candidates by the rule, in plain torch."""
    tri = verts[:, faces.long()]
    P, Q = tri[cand[:, 0], cand[:, 1]], tri[cand[:, 2], cand[:, 3]]
    nP, nQ = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), _cross(Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0])
    sP = torch.stack([_dot(nQ, P[:, i] - Q[:, 0]) for i in range(3)], 1)
    sQ = torch.stack([_dot(nP, Q[:, k] - P[:, 0]) for k in range(3)], 1)
    D = torch.stack([torch.stack([_dot(_cross(P[:, (i + 1) % 3] - P[:, i], Q[:, (k + 1) % 3] - Q[:, k]), Q[:, k] - P[:, i]) for k in range(3)], 1)
                     for i in range(3)], 1)
    opp = lambda a, b: ((a > 0) & (b < 0)) | ((a < 0) & (b > 0))
    ev = torch.zeros(len(cand), dtype=torch.int32, device=verts.device)
    for i in range(3):
        ev += (opp(sP[:, i], sP[:, (i + 1) % 3]) & ((D[:, i] > 0).all(1) | (D[:, i] < 0).all(1))).int()
        ev += (opp(sQ[:, i], sQ[:, (i + 1) % 3]) & ((D[:, :, i] > 0).all(1) | (D[:, :, i] < 0).all(1))).int()
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'surface_crossings_times.json'))
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--merge')
    a = ap.parse_args()

    if a.merge:
        out = json.load(open(a.out))
        kern = {}
        for row in csv.DictReader(open(a.merge)):
            for k in KERNELS:
                if k in row['Name']:
                    e = kern.setdefault(k, {'calls': 0, 'total_us': 0.0})
                    e['calls'] += int(row['Calls'])
                    e['total_us'] += float(row['TotalDurationNs']) / 1e3
        out['kernel_trace'] = kern
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return

    import torch
    from psi_release_amd import evaluation, ops, synth
    verts, faces = make_batch(a.bodies, a.seed)
    rest = synth.make_capsule_mesh(68, 156)[0]
    dv, df = torch.tensor(verts, device='cuda'), torch.tensor(faces, device='cuda')
    sc = evaluation.SurfaceCrossings(faces, 'cuda', order_verts=rest)
    if a.trace:
        for _ in range(a.calls):
            sc.crossings(dv)
        torch.cuda.synchronize()
        return
    h = sc._handle_for(verts.shape[1])
    (pruned, st), (brute, st_b) = ops.surface_crossings(dv, h, return_stats=True), ops.surface_crossings(dv, h, mode='brute', return_stats=True)
    same = all(torch.equal(x, y) for x, y in zip(pruned, brute))
    cand = torch_candidates(torch, dv, df)
    t_ev = torch_arm(torch, dv, df, cand)
    keys = lambda p: ((p[:, 0].long() * len(faces) + p[:, 1]) * a.bodies + p[:, 2]) * len(faces) + p[:, 3]
    t_keys, order = torch.sort(keys(cand[t_ev > 0]))
    torch_equal = bool(torch.equal(t_keys, keys(pruned.pairs)) and torch.equal(t_ev[t_ev > 0][order], pruned.events))
    print('%d bodies, %d faces: tiles %d of %d, %d (pair, box) tests, %d candidates, %d crossing pairs, %d irregular; brute equal %s, torch equal %s'
          % (a.bodies, len(faces), st['tiles'], st_b['tiles'], st['box_tests'], len(cand), st['pairs'], int(pruned.irregular), same, torch_equal), flush=True)
    run = {'pruned': lambda: sc.crossings(dv), 'brute': lambda: sc.crossings(dv, mode='brute'), 'torch': lambda: torch_arm(torch, dv, df, cand)}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / a.reps

    for fn in run.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn))
    sm = {k: summary(v) for k, v in ts.items()}
    sec = sm['pruned']['median_ms'] * 1e-3
    flops = st['box_tests'] * FLOPS_PER_BOX_TEST + len(cand) * FLOPS_PER_PREDICATE
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': a.bodies, 'seed': a.seed,
           'vertices': int(verts.shape[1]), 'faces': int(len(faces)),
           'what': 'SurfaceCrossings.crossings end to end (self + between), vertices on the GPU, device events; torch = the fifteen values and '
                   'the events of the same candidates in plain torch, the candidate search not included',
           'tiles_kept': st['tiles'], 'tiles_possible': st_b['tiles'], 'box_tests': st['box_tests'], 'box_tests_brute': st_b['box_tests'],
           'predicate_evaluations': int(len(cand)), 'crossing_pairs': st['pairs'], 'irregular': int(pruned.irregular),
           'body_pairs_crossing': int((torch.triu(pruned.counts, 1) > 0).sum()), 'self_crossing_bodies': int((torch.diagonal(pruned.counts) > 0).sum()),
           'brute_equals_pruned_bitwise': bool(same), 'torch_equals_pruned': torch_equal,
           'pruned': sm['pruned'], 'brute': sm['brute'], 'torch': sm['torch'],
           'brute_over_pruned': sm['brute']['median_ms'] / sm['pruned']['median_ms'],
           'box_tests_per_s': st['box_tests'] / sec, 'predicates_per_s': len(cand) / sec,
           'box_tests_per_s_brute': st_b['box_tests'] / (sm['brute']['median_ms'] * 1e-3),
           'flops_per_predicate_counted': FLOPS_PER_PREDICATE, 'flops_per_box_test_counted': FLOPS_PER_BOX_TEST,
           'least_ms_at_fp32_vector_peak': flops / PEAK_FP32_VECTOR * 1e3,
           'call_share_of_fp32_vector_peak': flops / PEAK_FP32_VECTOR / sec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
