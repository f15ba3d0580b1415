#!/usr/bin/env python
"""Timings of the conic distance field of crossing triangle pairs on the GPU (one JSON: profiles/crossing_field_times.json).

    python tools/time_crossing_field.py [--out FILE] [--bodies 32] [--seed 0] [--rounds 5] [--reps 3] [--sigma 1e-3]
    python tools/time_crossing_field.py --trace [--calls 10]      # the field and one backward pass, a fixed number of times: the program
                                                                  # of a `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_crossing_field.py --merge STATS_CSV [--out FILE] [--stats-out FILE]
                                                                  # adds that trace's per-kernel averages to the JSON and keeps the
                                                                  # rows of this project's kernels (profiles/crossing_field_kernel_stats.csv)

The batch is the one of tools/time_body_overlap.py: --bodies stand-in bodies of 20 904 faces placed by --seed in the room box, self +
between, on a Morton-ordered handle.  Arms, on the same batch, alternated over --rounds rounds (median and spread), device events:

    crossings    evaluation.SurfaceCrossings.crossings: what the batch cost before, so that the added cost shows
    penetration  ops.crossing_penetration: the crossings, then eval and pairs on the pairs found
    loss         forward + backward of ops.crossing_penetration_loss: the above, then grad_rows, a stable torch.sort, the segment sum
    field        eval + pairs + grad_rows + sort + segment sum on the pairs of one crossings call: what the field and its gradient add
    torch        a plain torch autograd composition of the same rule on the same pairs, forward + backward: the comparator of `field`

The torch arm's energy and gradient are compared with the kernels'."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from time_body_overlap import make_batch, summary  # noqa: E402

KERNELS = ('sc_chunk_box_kernel', 'sc_body_box_kernel', 'sc_tile_kernel', 'sc_test_kernel', 'sc_finish_kernel', 'sc_contour_kernel',
           'cf_eval_kernel', 'cf_pairs_kernel', 'cf_grad_rows_kernel', 'segment_sum3_kernel')


def _cross(torch, a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def torch_arm(torch, verts, faces, pairs, sigma):
    """The rule in plain torch with autograd on the pair list: (energy [n,2], G [B,V,3]) of sum_i loss[i]."""
    v = verts.detach().clone().requires_grad_(True)
    p, fl = pairs.long(), faces.long()
    bi = torch.stack([p[:, 0], p[:, 2]], 1).reshape(-1)
    fi = torch.stack([p[:, 1], p[:, 3]], 1).reshape(-1)
    br = torch.stack([p[:, 2], p[:, 0]], 1).reshape(-1)
    fr = torch.stack([p[:, 3], p[:, 1]], 1).reshape(-1)
    P, Q = v[bi[:, None], fl[fi]], v[br[:, None], fl[fr]]                                   # [2n,3,3]
    a = Q[:, 0]
    e1, e2 = Q[:, 1] - a, Q[:, 2] - a
    N = _cross(torch, e1, e2)
    N2 = _dot(N, N)
    n = N / torch.sqrt(N2)[:, None]
    m = _dot(e1, e1)[:, None] * _cross(torch, e2, N) + _dot(e2, e2)[:, None] * _cross(torch, N, e1)
    q = m / (2.0 * N2)[:, None]
    o = a + q
    r = torch.sqrt(_dot(q, q))
    s2 = 2.0 * sigma
    c2, c1, c0 = (1.0 - s2) / (s2 * s2), 1.0 / s2, (3.0 - s2) / 4.0
    w = P - o[:, None]
    h = _dot(n[:, None], w)
    t = w - h[..., None] * n[:, None]
    rho = torch.sqrt(_dot(t, t))
    Phi = rho / (r[:, None] * (1.0 - h / sigma))
    Y = torch.where(h <= -sigma, (1.0 - h) - sigma, (c0 - c1 * h) - (c2 * h) * h)
    psi = torch.where((h < sigma) & (Phi < 1.0), (1.0 - Phi) * Y, torch.zeros_like(h))
    energy = (psi[:, 0] * psi[:, 0] + psi[:, 1] * psi[:, 1]) + psi[:, 2] * psi[:, 2]
    energy.sum().backward()
    return energy.detach().reshape(-1, 2), v.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'crossing_field_times.json'))
    ap.add_argument('--stats-out', default=os.path.join(ROOT, 'profiles', 'crossing_field_kernel_stats.csv'))
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sigma', type=float, default=1e-3)
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
                if k in row['Name']:                   # the instances of a template (sc_test_kernel<false>, <true>) are added up
                    calls, total = int(row['Calls']), float(row['TotalDurationNs']) / 1e3
                    if k in kern:
                        calls, total = calls + kern[k]['calls'], total + kern[k]['average_us'] * kern[k]['calls']
                    kern[k] = {'calls': calls, 'average_us': total / calls}
        with open(a.stats_out, 'w') as f:
            f.write('\n'.join(kept) + '\n')
        out['kernel_trace'] = kern
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return

    verts, faces = make_batch(a.bodies, a.seed)
    import torch
    from psi_release_amd import evaluation, ops, synth
    import body_overlap_cases as C  # noqa: F401  (make_batch's mesh)
    B, V = verts.shape[:2]
    rest = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)[0]
    dv, df = torch.tensor(verts, device='cuda'), torch.tensor(faces, device='cuda')
    sc = evaluation.SurfaceCrossings(faces, 'cuda', order_verts=rest)
    handle = sc._handle_for(V)
    g = torch.ones(B, device='cuda')
    first = sc.field(dv, sigma=a.sigma)
    pairs = first.crossings.pairs
    n = int(pairs.shape[0])

    def field_only():
        rows = ops._field_rows(handle, dv, pairs, a.sigma)
        E, loss = ops._field_aggregates(handle, B, pairs, rows.energy)
        return rows, E, loss, ops.crossing_field_grad(dv, handle, pairs, g, a.sigma)

    def loss_arm():
        v = dv.detach().clone().requires_grad_(True)
        loss = ops.crossing_penetration_loss(v, handle, sigma=a.sigma)
        loss.sum().backward()
        return loss.detach(), v.grad

    if a.trace:
        for _ in range(a.calls):
            loss_arm()
        torch.cuda.synchronize()
        return
    print('%d bodies, %d faces: %d crossing pairs of triangles, %d pairs of bodies, %d bodies crossing themselves'
          % (B, len(faces), n, int((torch.triu(first.crossings.counts, 1) > 0).sum()), int((torch.diagonal(first.crossings.counts) > 0).sum())), flush=True)
    run = {'crossings': lambda: sc.crossings(dv), 'penetration': lambda: sc.field(dv, sigma=a.sigma), 'loss': loss_arm, 'field': field_only,
           'torch': lambda: torch_arm(torch, dv, df, pairs, a.sigma)}

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
    s = {k: summary(v) for k, v in ts.items()}
    t_energy, t_G = res['torch']
    G = res['field'][3]
    finite = torch.isfinite(t_G)
    gmax = float(G.abs().max().item())
    below = s['field']['max_ms'] < s['torch']['min_ms'] and \
        s['torch']['median_ms'] - s['field']['median_ms'] > (s['field']['max_ms'] - s['field']['min_ms']) + (s['torch']['max_ms'] - s['torch']['min_ms'])
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': B, 'seed': a.seed, 'vertices': V,
           'faces': int(len(faces)), 'sigma': a.sigma, 'triangle_pairs': n,
           'what': 'SurfaceCrossings.crossings / ops.crossing_penetration / forward + backward of crossing_penetration_loss end to end, '
                   'vertices on the GPU, device events; field = eval, pairs, grad_rows, sort and segment sum on the pairs of one call; '
                   'torch = the same rule with autograd on the same pairs, forward + backward',
           **{k: s[k] for k in run},
           'penetration_minus_crossings_ms': s['penetration']['median_ms'] - s['crossings']['median_ms'],
           'loss_minus_crossings_ms': s['loss']['median_ms'] - s['crossings']['median_ms'],
           'torch_over_field': s['torch']['median_ms'] / s['field']['median_ms'],
           'field_below_torch_by_more_than_both_spreads': bool(below),
           'torch_energy_bits_equal': int((t_energy.view(torch.int32) == first.rows.energy.view(torch.int32)).sum().item()),
           'torch_energy_values': int(t_energy.numel()),
           'torch_energy_max_rel_diff': float(((t_energy - first.rows.energy).abs() / first.rows.energy.abs().clamp_min(1e-30)).max().item()),
           'torch_G_bits_equal': int((t_G.view(torch.int32) == G.view(torch.int32)).sum().item()), 'torch_G_values': int(G.numel()),
           'torch_G_nonfinite': int((~finite).sum().item()),
           'torch_G_max_abs_diff_over_max_abs_G': float((t_G - G).abs()[finite].max().item()) / max(gmax, 1e-30), 'max_abs_G': gmax,
           'loss_sum': float(first.loss.double().sum().item()), 'self_energy_sum': float(torch.diagonal(first.pair_energy).sum().item())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
