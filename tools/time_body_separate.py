#!/usr/bin/env python
"""Timings of the rigid separation of overlapping bodies on the GPU (one JSON: profiles/body_separate_times.json).

    python tools/time_body_separate.py [--out FILE] [--bodies 32] [--seed 0] [--rounds 5] [--reps 3] [--max_iter 1000]
    python tools/time_body_separate.py --trace [--calls 3]        # the whole loop a fixed number of times: the program of a
                                                                  # `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_body_separate.py --merge STATS_CSV [--out FILE] [--stats-out FILE]
                                                                  # adds that trace's per-kernel averages to the JSON and keeps the
                                                                  # rows of this project's kernels (profiles/body_separate_kernel_stats.csv)

The batch is the one of tools/time_body_overlap.py: --bodies stand-in bodies of 20 904 faces placed by --seed in the room box, on a
Morton-ordered crossings handle.  First the whole loop (ops.rigid_separate): its iterations, its history and its time.  Then the parts of
its FIRST pass, on the same state, alternated over --rounds rounds (median and spread), device events:

    searches   ops.body_penetration and ops.crossing_penetration(self_pairs=False) on the posed bodies
    grads      body_penetration_grad, crossing_field_grad and their sum, from the rows and lists of one search
    rigid      the three new kernels: pose, wrench, step (the chunk sums go straight into the step's launch, as in the loop)
    torch      a plain torch composition of the same pose, reduction (fp64 sums) and Adam step on the same G: the comparator of `rigid`
    pass       one whole pass, ops.rigid_pass, from the same state every time

The torch arm's wrench and state are compared with the kernels'.

    python tools/time_body_separate.py --scene [--out FILE] [--dim 256] [--rounds 5] [--reps 3]      # profiles/body_separate_scene_times.json
    python tools/time_body_separate.py --scene --trace [--calls 3]
    python tools/time_body_separate.py --scene --merge STATS_CSV      # profiles/body_separate_scene_kernel_stats.csv

The scene arm: the same batch in the --dim^3 signed distance volume of synth.make_oriented_room (scene_sdf.MeshSDF), alternated rounds:

    scene        the scene kernel alone (psi_body_separate_scene: sample, hinge, wrench chunks, counts)
    composition  what it replaces: ops.sdf_sample with its gradient rows, the mask sdf < 0 and -w * gradient in torch, and stage one of
                 ops.rigid_wrench (the chunk sums)
    pass         ops.rigid_pass without a scene, from the same state every time
    pass_scene   ops.rigid_pass with the scene"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from time_body_overlap import make_batch, summary  # noqa: E402

KERNELS = ('bs_pose_kernel', 'bs_wrench_kernel', 'bs_step_kernel', 'bo_box_kernel', 'bo_count_kernel', 'bo_emit_kernel', 'bo_wind_kernel',
           'bo_decide_kernel', 'bd_nearest_kernel', 'bd_finish_kernel', 'bd_pairs_kernel', 'bd_grad_rows_kernel', 'segment_sum3_kernel',
           'sc_chunk_box_kernel', 'sc_body_box_kernel', 'sc_tile_kernel', 'sc_test_kernel', 'sc_finish_kernel', 'sc_contour_kernel',
           'cf_eval_kernel', 'cf_pairs_kernel', 'cf_grad_rows_kernel')


def torch_arm(torch, base, state, G, k, lr_t=0.01, lr_r=0.01, b1=0.9, b2=0.999, eps=1e-8):
    """pose, wrench and step in plain torch: (verts, g6, quat, transl, m, s), nothing in place."""
    q, t, c = state.quat, state.transl, state.pivot
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    p = c + t
    verts = torch.matmul(base - c[:, None], R.transpose(1, 2)) + p[:, None]
    a = verts - p[:, None]
    g6 = torch.cat([G.double().sum(1), torch.cross(a, G, dim=2).double().sum(1)], 1).float()
    m = b1 * state.m + (1 - b1) * g6
    s = b2 * state.s + (1 - b2) * g6 * g6
    u = (m / (1 - b1 ** k)) / (torch.sqrt(s / (1 - b2 ** k)) + eps)
    transl = t - lr_t * u[:, :3]
    h = -0.5 * lr_r * u[:, 3:]
    r = torch.cat([torch.ones_like(h[:, :1]), h], 1)
    rw, rx, ry, rz = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    quat = torch.stack([rw * w - rx * x - ry * y - rz * z, rw * x + rx * w + ry * z - rz * y, rw * y - rx * z + ry * w + rz * x,
                        rw * z + rx * y - ry * x + rz * w], 1)
    quat = quat / quat.norm(dim=1, keepdim=True)
    return verts, g6, quat, transl, m, s


def scene_arm(a):
    verts, faces = make_batch(a.bodies, a.seed)
    import torch
    from psi_release_amd import evaluation, ops, scene_sdf, synth
    import body_overlap_cases as C  # noqa: F401  (make_batch's mesh)
    B, V = verts.shape[:2]
    rest = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)[0]
    base = torch.tensor(verts, device='cuda')
    room = synth.make_oriented_room()
    lo, hi = scene_sdf.grid_box(room.verts, 0.5)
    mesh = scene_sdf.MeshSDF(room.verts, room.faces, device='cuda')
    sdf = mesh.compute(lo, hi, a.dim).reshape(1, a.dim, a.dim, a.dim).float().contiguous()
    gmin, gmax = torch.tensor(lo, device='cuda').reshape(1, 3), torch.tensor(hi, device='cuda').reshape(1, 3)
    scene = (sdf, gmin, gmax, None)
    sep = evaluation.BodySeparator(faces, 'cuda', order_verts=rest)
    oh, ch = sep.overlap._handle_for(V), sep.crossings._handle_for(V)
    state0 = ops.rigid_state(torch.tensor(verts.astype('float64').mean(1).astype('float32'), device='cuda'))
    scratch = ops.rigid_state(state0.pivot.clone())
    p = state0.pivot + state0.transl

    def kernel():
        return ops._scene_launch(base, p, scene, 1.0)

    def composition():
        og = torch.empty(B, V, 3, device='cuda')
        val = torch.empty(B, V, device='cuda')
        ops.hip.check(ops.hip.lib().psi_sdf_sample_forward(ops.hip.ptr(sdf), None, ops.hip.ptr(gmin), ops.hip.ptr(gmax), ops.hip.ptr(base), B, V, a.dim,
                                                           1, 1, ops.hip.ptr(val), ops.hip.ptr(og), ops.hip.stream()), 'psi_sdf_sample_forward')
        inside = val < 0
        G = torch.where(inside[..., None], -1.0 * og, torch.zeros_like(og))
        return ops._rigid_chunks(base, G, p, None), inside.sum(1), torch.where(inside, -val, torch.zeros_like(val)).double().sum(1)

    if a.trace:
        for _ in range(a.calls):
            kernel()
            composition()
        torch.cuda.synchronize()
        return

    def timed(fn, reps=a.reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / reps

    def reset():
        for dst, src in zip(scratch, state0):
            dst.copy_(src)

    def one_pass(**kw):
        reset()
        return ops.rigid_pass(base, scratch, 1, oh, ch, **kw)

    table = ops._RigidScene(scene, B, base.device, None)
    table.loss_rows = True                                 # as in the loop: the loss rows are added once after it
    run = {'scene': kernel, 'composition': composition, 'pass': one_pass, 'pass_scene': lambda: one_pass(scene=table)}
    res = {}
    for k, fn in run.items():
        res[k] = fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn))
    s = {k: summary(v) for k, v in ts.items()}
    spread = lambda k: s[k]['max_ms'] - s[k]['min_ms']
    below = s['scene']['max_ms'] < s['composition']['min_ms'] and \
        s['composition']['median_ms'] - s['scene']['median_ms'] > spread('scene') + spread('composition')
    chunks, count, loss = res['scene']
    c_chunks, c_count, c_loss = res['composition']
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': B, 'seed': a.seed, 'vertices': V, 'dim': a.dim,
           'what': 'the scene term of the separation on the batch of body_separate_times.json in the volume of synth.make_oriented_room, device '
                   'events: scene = psi_body_separate_scene alone; composition = psi_sdf_sample_forward with gradient rows, the mask and the '
                   'scaling in torch, psi_body_separate_wrench stage one; pass / pass_scene = ops.rigid_pass without / with the scene',
           'vertices_in_the_scene': int(count.sum().item()), 'composition_vertices_in_the_scene': int(c_count.sum().item()),
           'composition_chunks_max_abs_diff': float((chunks - c_chunks).abs().max().item()),
           'composition_loss_max_abs_diff': float((ops._chunk_order_sum(loss) - c_loss).abs().max().item()),
           **s, 'scene_share_of_pass_scene': s['scene']['median_ms'] / s['pass_scene']['median_ms'],
           'pass_scene_over_pass': s['pass_scene']['median_ms'] / s['pass']['median_ms'],
           'composition_over_scene': s['composition']['median_ms'] / s['scene']['median_ms'],
           'scene_below_composition_by_more_than_both_spreads': bool(below)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    sep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'body_separate_times.json'))
    ap.add_argument('--stats-out', default=os.path.join(ROOT, 'profiles', 'body_separate_kernel_stats.csv'))
    ap.add_argument('--bodies', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max_iter', type=int, default=1000)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--merge')
    ap.add_argument('--scene', action='store_true', help='the scene arm: its own JSON and kernel rows')
    ap.add_argument('--dim', type=int, default=256)
    a = ap.parse_args()
    if a.scene:
        if a.out == ap.get_default('out'):
            a.out = os.path.join(ROOT, 'profiles', 'body_separate_scene_times.json')
        if a.stats_out == ap.get_default('stats_out'):
            a.stats_out = os.path.join(ROOT, 'profiles', 'body_separate_scene_kernel_stats.csv')

    if a.merge:
        out = json.load(open(a.out))
        kern = {}
        lines = open(a.merge).read().splitlines()
        names = KERNELS + ('bs_scene_kernel', 'sdf_sample') if a.scene else KERNELS
        kept = [lines[0]] + [ln for ln in lines[1:] if any(k in ln for k in names)]         # this project's kernels, as rocprofv3 wrote them
        for row in csv.DictReader(kept):
            for k in names:
                if k in row['Name']:                   # the instances of a template are added up
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

    if a.scene:
        return scene_arm(a)
    verts, faces = make_batch(a.bodies, a.seed)
    import torch
    from psi_release_amd import evaluation, ops, synth
    import body_overlap_cases as C  # noqa: F401  (make_batch's mesh)
    B, V = verts.shape[:2]
    rest = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)[0]
    base = torch.tensor(verts, device='cuda')
    sep = evaluation.BodySeparator(faces, 'cuda', order_verts=rest)
    oh, ch = sep.overlap._handle_for(V), sep.crossings._handle_for(V)

    def loop():
        return sep.separate(base, max_iter=a.max_iter)

    if a.trace:
        for _ in range(a.calls):
            loop()
        torch.cuda.synchronize()
        return

    def timed(fn, reps=a.reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / reps

    res = loop()
    torch.cuda.synchronize()
    loop_ms = [timed(loop, 1) for _ in range(a.rounds)]
    clean = not ops.body_overlap(res.verts, oh)[0].any().item() and ops.surface_crossings(res.verts, ch, self_pairs=False).pairs.shape[0] == 0
    print('%d bodies, %d faces: %d iterations, separated %s, triples %s, pairs %s' % (B, len(faces), res.iterations, res.separated,
                                                                                   res.history['triples'], res.history['pairs']), flush=True)

    state0 = ops.rigid_state(res.pivot.clone())
    scratch = ops.rigid_state(res.pivot.clone())
    posed = ops.rigid_pose(base, state0.quat, state0.transl, state0.pivot)
    pen = ops.body_penetration(posed, oh)
    cr = ops.crossing_penetration(posed, ch, self_pairs=False, sigma=0.5)
    ones = torch.ones(B, device='cuda')
    g6 = torch.empty(B, 6, device='cuda')

    def grads():
        return ops.body_penetration_grad(posed.shape, oh, pen.triples, pen.rows, ones, 'depth') + ops.crossing_field_grad(posed, ch, cr.crossings.pairs, ones, 0.5)

    G = grads()

    def reset():
        for dst, src in zip(scratch, state0):
            dst.copy_(src)

    def rigid():
        v = ops.rigid_pose(base, scratch.quat, scratch.transl, scratch.pivot)
        chunks = ops._rigid_chunks(v, G, scratch.pivot + scratch.transl, None)
        ops._rigid_step(scratch, g6, chunks, 1, 0.01, 0.01, (0.9, 0.999), 1e-8, None)
        return v

    def one_pass():
        reset()
        return ops.rigid_pass(base, scratch, 1, oh, ch)

    run = {'searches': lambda: (ops.body_penetration(posed, oh), ops.crossing_penetration(posed, ch, self_pairs=False, sigma=0.5)),
           'grads': grads, 'rigid': rigid, 'torch': lambda: torch_arm(torch, base, state0, G, 1), 'pass': one_pass}
    out_res = {}
    for k, fn in run.items():                              # warm-up, and the results for the comparison
        reset()
        out_res[k] = fn()
        torch.cuda.synchronize()
        if k == 'rigid':
            after = [t.clone() for t in scratch] + [g6.clone()]
    ts = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ts[k].append(timed(fn))
    s = {k: summary(v) for k, v in ts.items()}
    t_verts, t_g6, t_quat, t_transl, t_m, t_s = out_res['torch']
    below = s['rigid']['max_ms'] < s['torch']['min_ms'] and \
        s['torch']['median_ms'] - s['rigid']['median_ms'] > (s['rigid']['max_ms'] - s['rigid']['min_ms']) + (s['torch']['max_ms'] - s['torch']['min_ms'])
    rel = lambda x, y: float(((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item())
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps': a.reps, 'bodies': B, 'seed': a.seed, 'vertices': V,
           'faces': int(len(faces)),
           'what': 'ops.rigid_separate end to end (loop), then the parts of its first pass on the same state, device events: searches = '
                   'body_penetration + crossing_penetration; grads = the two gradients and their sum; rigid = pose, wrench, step; torch = '
                   'the same pose, fp64 reduction and Adam step in plain torch; pass = ops.rigid_pass',
           'iterations': int(res.iterations), 'separated': bool(res.separated), 'clean_by_independent_searches': bool(clean),
           'triples': list(res.history['triples']), 'pairs': list(res.history['pairs']),
           'max_shift_m': float(res.shift.max().item()), 'max_angle_rad': float(res.angle.max().item()),
           'loop': summary(loop_ms), 'loop_ms_per_pass': summary(loop_ms)['median_ms'] / (res.iterations + 1),
           **{k: s[k] for k in run},
           'rigid_share_of_pass': s['rigid']['median_ms'] / s['pass']['median_ms'],
           'searches_share_of_pass': s['searches']['median_ms'] / s['pass']['median_ms'],
           'torch_over_rigid': s['torch']['median_ms'] / s['rigid']['median_ms'],
           'rigid_below_torch_by_more_than_both_spreads': bool(below),
           'torch_g6_max_rel_diff': rel(t_g6, after[5]), 'torch_verts_max_abs_diff': float((t_verts - out_res['rigid']).abs().max().item()),
           'torch_quat_max_abs_diff': float((t_quat - after[0]).abs().max().item()),
           'torch_transl_max_abs_diff': float((t_transl - after[1]).abs().max().item())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    sep.close()


if __name__ == '__main__':
    main()
