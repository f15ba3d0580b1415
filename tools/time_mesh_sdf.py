#!/usr/bin/env python
"""Timings of the mesh -> SDF volume kernel on the GPU (one JSON: profiles/mesh_sdf_times.json).

    python tools/time_mesh_sdf.py [--out FILE] [--subdiv 64] [--dim 256] [--rounds 5] [--reps 3]
    python tools/time_mesh_sdf.py --trace [--calls 5]     # the compute calls alone, a fixed number of times: the program of a
                                                          # `rocprofv3 --kernel-trace --stats` run of its own (profiles/mesh_sdf_kernel_stats.csv)
    python tools/time_mesh_sdf.py --merge STATS_CSV [--out FILE]   # adds the kernel's average times from the trace to the JSON

Scene: synth.make_oriented_room(subdiv) — every box face cut into 2 * subdiv^2 triangles (subdiv = 64: ~147 k triangles) — in its box grown
by 0.5 m.  Measured, with device events after a warm-up: the pruned search at --dim^3 nodes, and at 64^3 nodes the pruned search against
every node against every triangle, the cases alternated over --rounds rounds (median and spread).  The (node, triangle) tests each search
executes are counted by the counting build of the kernel (psi_mesh_sdf_count_pairs, never timed) and set against the fp32 vector rate of
the MI355X: a test is ~95 fp32 operations (six dot products, the region tests, one division, the closest point, the squared distance).
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psi_release_amd import ops, scene_sdf, synth  # noqa: E402

FP32_VECTOR_FLOPS = 157.3e12       # MI355X data sheet, fp32 vector
FLOP_PER_TEST = 95                 # counted from the routine: 6 dot products (30), 2 offsets (6), the edge / face terms (~20), one division
                                   # and the closest point (~25), r and d2 (8), the key and the minimum (~6)


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {'median_ms': med, 'min_ms': ts[0], 'max_ms': ts[-1], 'spread_rel': (ts[-1] - ts[0]) / med}


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_sdf_times.json'))
    ap.add_argument('--subdiv', type=int, default=64)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--merge', default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a)
    room = synth.make_oriented_room(a.subdiv)
    t0 = time.perf_counter()
    mesh = scene_sdf.MeshSDF(room.verts, room.faces)
    torch.cuda.synchronize()
    create_s = time.perf_counter() - t0
    lo, hi = scene_sdf.grid_box(room.verts, 0.5)
    cases = {'grid_%d' % a.dim: (a.dim, 'grid'), 'grid_64': (64, 'grid'), 'brute_64': (64, 'brute')}
    run = {k: (lambda d=d, m=m: mesh.compute(lo, hi, d, mode=m)) for k, (d, m) in cases.items()}
    if a.trace:
        for _ in range(a.calls):
            for fn in run.values():
                fn()
        torch.cuda.synchronize()
        return
    for fn in run.values():                                   # warm-up, and the check that pruning changes nothing at the timed size
        fn()
    same = bool(torch.equal(run['grid_64']().view(torch.int32), run['brute_64']().view(torch.int32)))
    ts = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn, a.reps))
    out = {'device': torch.cuda.get_device_name(0), 'triangles': int(mesh.info[0]), 'mesh_info': list(mesh.info), 'create_s': create_s,
           'grid_equals_brute_at_64': same, 'rounds': a.rounds, 'reps': a.reps, 'flop_per_test': FLOP_PER_TEST,
           'fp32_vector_flops_used': FP32_VECTOR_FLOPS, 'cases': {}}
    for k, (d, m) in cases.items():
        s = summary(ts[k])
        pairs = ops.mesh_sdf_count_pairs(mesh.handle, lo, hi, d, scene_sdf.MODES[m])
        rate = pairs / (s['median_ms'] * 1e-3)
        out['cases'][k] = dict(s, dim=d, mode=m, nodes=d ** 3, pair_tests=pairs, share_of_brute_force=pairs / (float(d) ** 3 * mesh.info[0]),
                               pair_tests_per_s=rate, share_of_fp32_vector_rate=rate * FLOP_PER_TEST / FP32_VECTOR_FLOPS)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def merge(a):
    """The brick kernel's rows of a rocprofv3 --kernel-trace --stats table into the JSON (the trace run issues the three cases in turn, so
    the average is over them; the per-case times are the event timings above)."""
    with open(a.out) as f:
        out = json.load(f)
    rows = {}
    with open(a.merge) as f:
        for row in csv.DictReader(f):
            m = re.search(r'msdf_brick_kernel<[a-z]+>|msdf_brick_kernel', row.get('Name', ''))
            if m:
                rows[m.group(0)] = {'calls': int(row['Calls']), 'avg_us': float(row['AverageNs']) / 1e3, 'total_ms': float(row['TotalDurationNs']) / 1e6,
                                    'share_of_trace': float(row.get('Percentage', 'nan'))}
    out['kernel_trace'] = rows
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
