#!/usr/bin/env python
"""Timings of the body-against-body overlap counts on the GPU (one JSON: profiles/body_overlap_times.json).

    python tools/time_body_overlap.py [--out FILE] [--bodies 32] [--seed 0] [--rounds 5] [--reps 3] [--host-procs 16] [--no-host]
    python tools/time_body_overlap.py --trace [--calls 10]        # the call alone, a fixed number of times: the program of a
                                                                  # `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_body_overlap.py --merge STATS_CSV [--out FILE]    # adds that trace's per-kernel averages to the JSON

The batch: --bodies stand-in bodies (synth.make_capsule_mesh(68, 156): 10 454 vertices, 20 904 faces, the SMPL-X surface has 20 908)
placed by --seed in the 5 x 4 m room box (0.5 m and 0.4 m from its walls), tilted up to 0.5 rad, so that several pairs overlap; the
number of pairs and of candidates is printed.  Three arms on the same batch:

    hip     evaluation.BodyOverlap.counts (five kernels, two scans, one read-back), device events
    torch   a plain torch composition of the same rule on the same candidate list on the GPU (fp32, one [block, F] matrix per operation)
    numpy   the fp64 restatement (tests/body_overlap_ref.py) on the same candidates, spread over --host-procs host processes, wall clock

hip and torch alternate over --rounds rounds (median and spread).  The (candidate, face) tests executed are counted from the candidate
list; FLOPS_PER_TEST counts the additions and multiplications of one half_omega statement as written (the three square roots and the
arctangent are extra), which gives the least time the fp32 vector rate of the MI355X (157.3 TFLOP/s) allows for them."""
import argparse
import csv
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import body_overlap_cases as C  # noqa: E402
import body_overlap_ref as R  # noqa: E402
from psi_release_amd import synth  # noqa: E402

KERNELS = ('bo_box_kernel', 'bo_count_kernel', 'bo_emit_kernel', 'bo_wind_kernel', 'bo_decide_kernel')
FLOPS_PER_TEST = 9 + 3 * 5 + 5 + (2 + 3 * 5 + 3 + 3)      # differences, three squared lengths, det, den; sqrt x 3 and atan2 not counted
PEAK_FP32_VECTOR = 157.3e12                               # MI355X, FLOP/s


def make_batch(n, seed):
    """([n,V,3] fp32, faces): capsules tilted by up to 0.5 rad about a horizontal axis, turned about z, feet near the floor."""
    v, f = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)
    rs = np.random.RandomState(seed)
    poses = []
    for _ in range(n):
        a = rs.uniform(0, 2 * np.pi)
        tilt = C.rotation((np.cos(a), np.sin(a), 0.0), rs.uniform(0, 0.5))
        turn = C.rotation((0, 0, 1), rs.uniform(0, 2 * np.pi))
        poses.append((turn @ tilt, np.array([rs.uniform(-2.0, 2.0), rs.uniform(-1.6, 1.6), rs.uniform(0.0, 0.3)])))
    verts = np.stack([(v.astype(np.float64) @ Rm.T + t).astype(np.float32) for Rm, t in poses])
    return verts, f


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {'median_ms': med, 'min_ms': ts[0], 'max_ms': ts[-1], 'spread_rel': (ts[-1] - ts[0]) / med}


def _host_part(args):
    verts, faces, cand = args
    w = np.zeros(len(cand))
    for j in np.unique(cand[:, 1]):
        sel = cand[:, 1] == j
        w[sel] = R.winding(verts[cand[sel, 0], cand[sel, 2]], verts[j], faces, block=128)
    return w


def host_arm(procs, verts, faces, cand):
    t0 = time.perf_counter()
    cuts = np.linspace(0, len(cand), procs + 1).astype(int)
    with multiprocessing.get_context('spawn').Pool(procs) as pool:
        w = np.concatenate(pool.map(_host_part, [(verts, faces, cand[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]))
    return w, time.perf_counter() - t0


def torch_arm(torch, verts, faces, cand, block=2048):
    """The same rule in plain torch on the candidate list: (counts [B,B] int64, w [n] fp32)."""
    B = verts.shape[0]
    cand = cand.long()
    w = torch.empty(len(cand), dtype=torch.float32, device=verts.device)
    pair = cand[:, 0] * B + cand[:, 1]
    js = torch.unique(cand[:, 1]).tolist()
    for j in js:
        idx = torch.nonzero(cand[:, 1] == j)[:, 0]
        tri = verts[j][faces.long()]
        A, Bv, Cv = tri[:, 0], tri[:, 1], tri[:, 2]
        n = torch.cross(Bv - A, Cv - A, dim=-1)
        for lo in range(0, len(idx), block):
            k = idx[lo:lo + block]
            p = verts[cand[k, 0], cand[k, 2]][:, None]
            a, b, c = A[None] - p, Bv[None] - p, Cv[None] - p
            la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
            det = (a * n[None]).sum(-1)
            den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
            w[k] = torch.atan2(det, den).sum(1) / (2 * np.pi)
    counts = torch.bincount(pair[w > 0.5], minlength=B * B).reshape(B, B)
    return counts, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'body_overlap_times.json'))
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-procs', type=int, default=16)
    ap.add_argument('--no-host', action='store_true')
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
                    kern[k] = {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3}
        out['kernel_trace'] = kern
        out['kernel_trace_sum_us'] = sum(v['average_us'] for v in kern.values())
        if 'bo_wind_kernel' in kern:
            t = kern['bo_wind_kernel']['average_us'] * 1e-6
            out['wind_kernel'] = {'tests_per_s': out['tests'] / t, 'counted_tflops': out['tests'] * FLOPS_PER_TEST / t / 1e12,
                                  'share_of_fp32_vector_peak': out['tests'] * FLOPS_PER_TEST / t / PEAK_FP32_VECTOR}
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return

    verts, faces = make_batch(a.bodies, a.seed)
    cand = R.candidates(verts)
    per_pair = np.zeros((a.bodies, a.bodies), np.int64)
    np.add.at(per_pair, (cand[:, 0], cand[:, 1]), 1)
    tests = int(len(cand)) * int(len(faces))
    print('%d bodies, %d faces: %d ordered pairs with candidates, %d candidates (largest pair %d), %d (candidate, face) tests'
          % (a.bodies, len(faces), int((per_pair > 0).sum()), len(cand), per_pair.max(), tests), flush=True)
    host_w, host_s = (None, None)
    if not a.trace and not a.no_host:                      # the host arm first: its processes end before this one opens the GPU
        host_w, host_s = host_arm(a.host_procs, verts, faces, cand)
        print('numpy restatement on %d processes: %.1f s' % (a.host_procs, host_s), flush=True)

    import torch
    from psi_release_amd import evaluation, ops
    dv, df = torch.tensor(verts, device='cuda'), torch.tensor(faces, device='cuda')
    bo = evaluation.BodyOverlap(faces, 'cuda')
    if a.trace:
        for _ in range(a.calls):
            bo.counts(dv)
        torch.cuda.synchronize()
        return
    counts, inside, d_cand, w = ops.body_overlap(dv, bo._handle_for(verts.shape[1]), return_candidates=True)
    assert np.array_equal(d_cand.cpu().numpy(), cand)
    run = {'hip': lambda: bo.counts(dv), 'torch': lambda: torch_arm(torch, dv, df, d_cand)}

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
    t_counts, t_w = res['torch']
    hip_ms = summary(ts['hip'])
    least_ms = tests * FLOPS_PER_TEST / PEAK_FP32_VECTOR * 1e3
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': a.bodies, 'seed': a.seed,
           'vertices': int(verts.shape[1]), 'faces': int(len(faces)), 'pairs_with_candidates': int((per_pair > 0).sum()),
           'pairs_overlapping': int((counts > 0).sum().item()), 'candidates': int(len(cand)), 'largest_pair': int(per_pair.max()), 'tests': tests,
           'what': 'BodyOverlap.counts end to end, vertices on the GPU, device events; torch = the same rule on the same candidates; '
                   'numpy = tests/body_overlap_ref.py on host processes, wall clock',
           'hip': hip_ms, 'torch': summary(ts['torch']), 'torch_over_hip': summary(ts['torch'])['median_ms'] / hip_ms['median_ms'],
           'torch_counts_equal': bool(torch.equal(t_counts.to(torch.int32), counts)), 'torch_w_max_diff': float((t_w - w).abs().max().item()),
           'flops_per_test_counted': FLOPS_PER_TEST, 'least_ms_at_fp32_vector_peak': least_ms,
           'call_share_of_fp32_vector_peak': least_ms / hip_ms['median_ms'],
           'bound': 'compute (vector ALU): the call reads %.1f MB of vertices and faces and writes %.1f MB; at HBM rate that is microseconds'
                    % ((verts.nbytes + faces.nbytes) / 1e6, (len(cand) * (12 + 4 + 8 * ((len(faces) + 2047) // 2048))) / 1e6)}
    if host_w is not None:
        out.update(host_processes=a.host_procs, numpy_s=host_s, numpy_over_hip=host_s / (hip_ms['median_ms'] * 1e-3),
                   hip_w_max_err_vs_fp64=float(np.abs(w.cpu().numpy().astype(np.float64) - host_w).max()),
                   hip_counts_equal_numpy=bool(np.array_equal(np.bincount(cand[host_w > 0.5, 0] * a.bodies + cand[host_w > 0.5, 1],
                                                                          minlength=a.bodies ** 2).reshape(a.bodies, a.bodies), counts.cpu().numpy())))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
