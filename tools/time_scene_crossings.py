#!/usr/bin/env python
"""Timings of the scene-crossing search on the GPU (one JSON: profiles/scene_crossings_times.json).

    python tools/time_scene_crossings.py [--out FILE] [--bodies 32] [--seed 0] [--subdiv 64] [--rounds 5] [--reps 3]
    python tools/time_scene_crossings.py --trace [--calls 10]      # the pruned call alone, a fixed number of times: the program of a
                                                                   # `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_scene_crossings.py --merge STATS_CSV [--out FILE]      # adds that trace's per-kernel totals to the JSON

The bodies are those of tools/time_surface_crossings.py: --bodies stand-in bodies (synth.make_capsule_mesh(68, 156): 20 904 faces) placed
by --seed in the room box, on a handle ordered along the rest pose; the scene is synth.make_room_mesh(subdiv=--subdiv) (64: about 197 k
triangles).  Four arms, alternating over --rounds rounds (median and spread), device events but for the handle:

    pruned  evaluation.SceneCrossings.crossings (body-box and chunk-box culling)
    brute   the same with mode='brute': every body chunk against every scene chunk
    torch   a plain torch composition of the fifteen values and the events on the same face-box candidates, their search not included
    create  ops.scene_crossings_create of the scene (host work and one upload), wall clock

Reported: tiles kept of tiles possible, the (face, triangle) box tests executed (counted from the tile table), the predicate evaluations
(the candidates, counted by the torch arm) and the crossing pairs."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from time_body_overlap import make_batch, summary  # noqa: E402
from time_surface_crossings import _cross, _dot  # noqa: E402

KERNELS = ('sc_chunk_box_kernel', 'sc_body_box_kernel', 'scn_tile_kernel', 'scn_test_kernel', 'scn_finish_kernel', 'scn_contour_kernel')


def torch_candidates(torch, verts, faces, sverts, sfaces, rows=512):
    """[n,3] int64 (i, s, t): the face-box candidates of the rule; per body only the scene triangles whose box meets the body's box."""
    tri, stri = verts[:, faces.long()], sverts[sfaces.long()]
    lo, hi = tri.min(2).values, tri.max(2).values
    slo, shi = stri.min(1).values, stri.max(1).values
    blo, bhi = verts.min(1).values, verts.max(1).values
    out = []
    for i in range(verts.shape[0]):
        near = torch.nonzero(((slo <= bhi[i]) & (blo[i] <= shi)).all(-1), as_tuple=True)[0]
        for r0 in range(0, faces.shape[0], rows):
            a = slice(r0, min(faces.shape[0], r0 + rows))
            meet = ((lo[i, a, None] <= shi[None, near]) & (slo[None, near] <= hi[i, a, None])).all(-1)
            s, t = torch.nonzero(meet, as_tuple=True)
            out.append(torch.stack([torch.full_like(s, i), s + r0, near[t]], 1))
    return torch.cat(out)


def torch_arm(torch, verts, faces, sverts, sfaces, cand):
    """events [n] of the candidates by the rule, in plain torch (fp32, one tensor per operation)."""
    P, Q = verts[:, faces.long()][cand[:, 0], cand[:, 1]], sverts[sfaces.long()][cand[:, 2]]
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_crossings_times.json'))
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--subdiv', type=int, default=64)
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
    room = synth.make_room_mesh(subdiv=a.subdiv)
    dv, df = torch.tensor(verts, device='cuda'), torch.tensor(faces, device='cuda')
    sv, sf = torch.tensor(room.verts, device='cuda'), torch.tensor(room.faces, device='cuda')
    sc = evaluation.SceneCrossings(room.verts, room.faces, faces, 'cuda', order_verts=rest)
    if a.trace:
        for _ in range(a.calls):
            sc.crossings(dv)
        torch.cuda.synchronize()
        return
    h = sc._handle_for(verts.shape[1])
    (pruned, st), (brute, st_b) = ops.scene_crossings(dv, sc.scene, h, return_stats=True), ops.scene_crossings(dv, sc.scene, h, mode='brute', return_stats=True)
    same = all(torch.equal(x, y) for x, y in zip(pruned, brute))
    cand = torch_candidates(torch, dv, df, sv, sf)
    t_ev = torch_arm(torch, dv, df, sv, sf, cand)
    F, nf = len(faces), len(room.faces)
    keys = lambda p: (p[:, 0].long() * F + p[:, 1]) * nf + p[:, 2]
    t_keys, order = torch.sort(keys(cand[t_ev > 0]))
    torch_equal = bool(torch.equal(t_keys, keys(pruned.pairs)) and torch.equal(t_ev[t_ev > 0][order], pruned.events))
    print('%d bodies of %d faces, %d scene triangles: tiles %d of %d, %d box tests, %d candidates, %d crossing pairs, %d irregular; brute equal %s, '
          'torch equal %s' % (a.bodies, F, nf, st['tiles'], st_b['tiles'], st['box_tests'], len(cand), st['pairs'], int(pruned.irregular), same,
                              torch_equal), flush=True)
    run = {'pruned': lambda: sc.crossings(dv), 'brute': lambda: sc.crossings(dv, mode='brute'),
           'torch': lambda: torch_arm(torch, dv, df, sv, sf, cand)}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / a.reps

    def create():
        t0 = time.perf_counter()
        ops.scene_crossings_create(room.verts, room.faces).close()
        return (time.perf_counter() - t0) * 1e3

    for fn in run.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in list(run) + ['create']}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn))
        ts['create'].append(create())
    sm = {k: summary(v) for k, v in ts.items()}
    sec = sm['pruned']['median_ms'] * 1e-3
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': a.bodies, 'seed': a.seed,
           'vertices': int(verts.shape[1]), 'faces': F, 'scene_triangles': nf, 'scene_chunks': int(sc.scene.n_chunks),
           'what': 'SceneCrossings.crossings end to end, vertices on the GPU, device events; torch = the fifteen values and the events of the '
                   'same candidates in plain torch, the candidate search not included; create = scene_crossings_create, wall clock',
           'tiles_kept': st['tiles'], 'tiles_possible': st_b['tiles'], 'box_tests': st['box_tests'], 'box_tests_brute': st_b['box_tests'],
           'predicate_evaluations': int(len(cand)), 'crossing_pairs': st['pairs'], 'irregular': int(pruned.irregular),
           'bodies_crossing': int((pruned.counts > 0).sum()), 'scene_triangles_crossed': int(pruned.tri_hit.sum()),
           'brute_equals_pruned_bitwise': bool(same), 'torch_equals_pruned': torch_equal,
           'pruned': sm['pruned'], 'brute': sm['brute'], 'torch': sm['torch'], 'create': sm['create'],
           'brute_over_pruned': sm['brute']['median_ms'] / sm['pruned']['median_ms'],
           'box_tests_per_s': st['box_tests'] / sec, 'predicates_per_s': len(cand) / sec,
           'box_tests_per_s_brute': st_b['box_tests'] / (sm['brute']['median_ms'] * 1e-3)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
