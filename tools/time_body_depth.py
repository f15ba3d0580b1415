#!/usr/bin/env python
"""Timings of the body-against-body penetration depth on the GPU (one JSON: profiles/body_depth_times.json).

    python tools/time_body_depth.py [--out FILE] [--bodies 32] [--seed 0] [--rounds 5] [--reps 3]
    python tools/time_body_depth.py --trace [--calls 10]          # depths and one backward pass, a fixed number of times: the program
                                                                  # of a `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_body_depth.py --merge STATS_CSV [--out FILE] [--stats-out FILE]
                                                                  # adds that trace's per-kernel averages to the JSON and keeps the
                                                                  # rows of this project's kernels (profiles/body_depth_kernel_stats.csv)

The batch is the one of tools/time_body_overlap.py: --bodies stand-in bodies of 20 904 faces placed by --seed in the room box.  Arms, on
the same batch, alternated over --rounds rounds (median and spread), device events:

    counts    evaluation.BodyOverlap.counts: what the batch cost before, so that the added cost shows
    depths    evaluation.BodyOverlap.depths: the counts, then nearest, finish and pairs for the inside triples
    backward  ops.body_penetration_grad on the rows of one depths call: grad_rows, a stable torch.sort, the segment sum
    torch     a plain torch composition of the same closest-point rule on the same inside triples (one [block, F] matrix per operation)

The (triple, face) tests executed are counted from the inside triples; FLOPS_PER_TEST counts the additions and multiplications of one
closest-point statement on the face branch as written (the division is extra).  The torch arm's winners and depths are compared with the
kernels': torch.min returns A smallest element, not the first, so winners may differ where two faces tie; depths must not."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from time_body_overlap import PEAK_FP32_VECTOR, make_batch, summary  # noqa: E402

KERNELS = ('bo_wind_kernel', 'bd_nearest_kernel', 'bd_finish_kernel', 'bd_pairs_kernel', 'bd_grad_rows_kernel', 'segment_sum3_kernel')
# ap, bp, cp (9), six dot products (30), va vb vc (9), the sum and two products for v, w (4), q (9), r (3), d2 (5); division and key not counted
FLOPS_PER_TEST = 9 + 30 + 9 + 4 + 9 + 3 + 5


def torch_arm(torch, verts, faces, trip, block=1024):
    """The rule in plain torch on the triple list: (face [n] int64, depth [n] fp32)."""
    trip, fl = trip.long(), faces.long()
    face = torch.empty(len(trip), dtype=torch.int64, device=verts.device)
    depth = torch.empty(len(trip), dtype=torch.float32, device=verts.device)
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    inf = torch.tensor(float('inf'), device=verts.device)
    for j in torch.unique(trip[:, 1]).tolist():
        idx = torch.nonzero(trip[:, 1] == j)[:, 0]
        X = verts[j]
        a = X[fl[:, 0]]
        ab, ac = (X[fl[:, 1]] - a)[None], (X[fl[:, 2]] - a)[None]
        for lo in range(0, len(idx), block):
            k = idx[lo:lo + block]
            ap = verts[trip[k, 0], trip[k, 2]][:, None] - a[None]
            d1, d2 = dot(ab, ap), dot(ac, ap)
            bp = ap - ab
            d3, d4 = dot(ab, bp), dot(ac, bp)
            cp = ap - ac
            d5, d6 = dot(ab, cp), dot(ac, cp)
            va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
            denom = 1.0 / ((va + vb) + vc)
            q = ab * (vb * denom)[..., None] + ac * (vc * denom)[..., None]
            pick = lambda cond, value, rest: torch.where(cond[..., None], value, rest)
            q = pick((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), ab + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (ac - ab), q)
            q = pick((vb <= 0) & (d2 >= 0) & (d6 <= 0), (d2 / (d2 - d6))[..., None] * ac, q)
            q = pick((d6 >= 0) & (d5 <= d6), ac.expand_as(q), q)
            q = pick((vc <= 0) & (d1 >= 0) & (d3 <= 0), (d1 / (d1 - d3))[..., None] * ab, q)
            q = pick((d3 >= 0) & (d4 <= d3), ab.expand_as(q), q)
            q = pick((d1 <= 0) & (d2 <= 0), torch.zeros_like(q), q)
            r = ap - q
            dd = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
            best, at = torch.where(torch.isfinite(dd), dd, inf).min(1)
            face[k], depth[k] = at, torch.sqrt(best)
    return face, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'body_depth_times.json'))
    ap.add_argument('--stats-out', default=os.path.join(ROOT, 'profiles', 'body_depth_kernel_stats.csv'))
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
        lines = open(a.merge).read().splitlines()
        kept = [lines[0]] + [ln for ln in lines[1:] if any(k in ln for k in KERNELS)]       # this project's kernels, as rocprofv3 wrote them
        for row in csv.DictReader(kept):
            for k in KERNELS:
                if k in row['Name']:
                    kern[k] = {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3}
        with open(a.stats_out, 'w') as f:
            f.write('\n'.join(kept) + '\n')
        out['kernel_trace'] = kern
        if 'bd_nearest_kernel' in kern:
            t = kern['bd_nearest_kernel']['average_us'] * 1e-6
            out['nearest_kernel'] = {'tests_per_s': out['tests'] / t, 'counted_tflops': out['tests'] * FLOPS_PER_TEST / t / 1e12,
                                     'share_of_fp32_vector_peak': out['tests'] * FLOPS_PER_TEST / t / PEAK_FP32_VECTOR}
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return

    verts, faces = make_batch(a.bodies, a.seed)
    import torch
    from psi_release_amd import evaluation, ops
    B, V = verts.shape[:2]
    dv, df = torch.tensor(verts, device='cuda'), torch.tensor(faces, device='cuda')
    bo = evaluation.BodyOverlap(faces, 'cuda')
    handle = bo._handle_for(V)
    g = torch.ones(B, device='cuda')
    pen = bo.depths(dv)
    if a.trace:
        for _ in range(a.calls):
            r = bo.depths(dv)
            ops.body_penetration_grad((B, V, 3), handle, r.triples, r.rows, g)
        torch.cuda.synchronize()
        return
    n = int(pen.triples.shape[0])
    tests = n * int(len(faces))
    print('%d bodies, %d faces: %d overlapping ordered pairs, %d inside triples, %d (triple, face) tests'
          % (B, len(faces), int((pen.counts > 0).sum()), n, tests), flush=True)
    run = {'counts': lambda: bo.counts(dv), 'depths': lambda: bo.depths(dv),
           'backward': lambda: ops.body_penetration_grad((B, V, 3), handle, pen.triples, pen.rows, g),
           'torch': lambda: torch_arm(torch, dv, df, pen.triples)}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / a.reps

    res = {}
    for k, fn in run.items():                              # warm-up, and the results for the comparison
        res[k] = fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn))
    t_face, t_depth = res['torch']
    s = {k: summary(v) for k, v in ts.items()}
    same_face = t_face == pen.rows.face.long()
    least_ms = tests * FLOPS_PER_TEST / PEAK_FP32_VECTOR * 1e3
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': B, 'seed': a.seed, 'vertices': V,
           'faces': int(len(faces)), 'pairs_overlapping': int((pen.counts > 0).sum().item()), 'inside_triples': n, 'tests': tests,
           'what': 'BodyOverlap.counts / .depths end to end and one backward pass, vertices on the GPU, device events; torch = the same '
                   'closest-point rule on the same inside triples',
           'counts': s['counts'], 'depths': s['depths'], 'backward': s['backward'], 'torch': s['torch'],
           'depths_minus_counts_ms': s['depths']['median_ms'] - s['counts']['median_ms'],
           'depths_over_counts': s['depths']['median_ms'] / s['counts']['median_ms'],
           'tests_per_s_of_the_added_time': tests / max((s['depths']['median_ms'] - s['counts']['median_ms']) * 1e-3, 1e-9),
           'torch_over_added_time': s['torch']['median_ms'] / max(s['depths']['median_ms'] - s['counts']['median_ms'], 1e-9),
           'torch_winners_equal': int(same_face.sum().item()), 'torch_winners_differ': int((~same_face).sum().item()),
           'torch_depth_bits_equal': int((t_depth.view(torch.int32) == pen.rows.depth.view(torch.int32)).sum().item()),
           'torch_depth_max_diff': float((t_depth - pen.rows.depth).abs().max().item()),
           'deepest_m': float(pen.max_depth.max().item()), 'loss_depth_sum': float(pen.loss[0].double().sum().item()),
           'flops_per_test_counted': FLOPS_PER_TEST, 'least_ms_at_fp32_vector_peak': least_ms}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
