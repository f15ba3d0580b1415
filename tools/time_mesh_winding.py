#!/usr/bin/env python
"""Timings of the winding-number kernel on the GPU (one JSON: profiles/mesh_winding_times.json).

    python tools/time_mesh_winding.py [--out FILE] [--subdiv 64] [--dim 256] [--beta 3] [--cluster 64] [--rounds 5] [--reps 2]

Scene: synth.make_oriented_room(subdiv) — every box face cut into 2 * subdiv^2 triangles (subdiv = 64: ~147 k triangles) — in its box grown
by 0.5 m.  Measured, with device events after a warm-up (which also builds and caches the clusters): at 64^3 nodes the exact arm (every
node against every triangle) and the pruned arm, at --dim^3 nodes the pruned arm next to ``MeshSDF.compute`` of the same grid (the
distance search whose sign it replaces), the cases alternated over --rounds rounds (median and spread).  The (node, triangle) and
(node, dipole) tests are counted by the counting build of the kernel (psi_mesh_winding_count, never timed)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psi_release_amd import ops, scene_sdf, synth  # noqa: E402


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_winding_times.json'))
    ap.add_argument('--subdiv', type=int, default=64)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--beta', type=float, default=3.0)
    ap.add_argument('--cluster', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=2)
    a = ap.parse_args()
    room = synth.make_oriented_room(a.subdiv)
    mesh = scene_sdf.MeshSDF(room.verts, room.faces)
    lo, hi = scene_sdf.grid_box(room.verts, 0.5)
    wind = lambda d, beta: (lambda: mesh.winding(lo, hi, d, beta=beta, cluster=a.cluster))
    cases = {'exact_64': (64, 0.0), 'pruned_64': (64, a.beta), 'pruned_%d' % a.dim: (a.dim, a.beta)}
    run = {k: wind(d, beta) for k, (d, beta) in cases.items()}
    run['sdf_grid_%d' % a.dim] = lambda: mesh.compute(lo, hi, a.dim)
    first = {}
    for k, fn in run.items():                                 # warm-up; the first pruned call builds and uploads the clusters
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        first[k] = time.perf_counter() - t0
    diff = float((run['exact_64']() - run['pruned_64']()).abs().max())
    ts = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn, a.reps))
    out = {'device': torch.cuda.get_device_name(0), 'triangles': int(mesh.info[0]), 'beta': a.beta, 'cluster': a.cluster, 'rounds': a.rounds,
           'reps': a.reps, 'first_call_s': first, 'max_abs_pruned_minus_exact_at_64': diff, 'cases': {}}
    for k in run:
        s = summary(ts[k])
        if k in cases:
            d, beta = cases[k]
            tri, dip = ops.mesh_winding_count(mesh.handle, lo, hi, d, beta=beta, cluster=a.cluster)
            s.update(dim=d, beta=beta, nodes=d ** 3, triangle_tests=tri, dipole_tests=dip,
                     share_of_all_pairs=tri / (float(d) ** 3 * mesh.info[0]), triangle_tests_per_s=tri / (s['median_ms'] * 1e-3))
        out['cases'][k] = s
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
