#!/usr/bin/env python
"""Timings of the batched evaluation against what it replaces, on the GPU (one JSON: profiles/eval_times.json).

    python tools/bench_eval.py [--out FILE] [--sections scoring,kernel,diversity] [--rounds 3] [--window 0.5]
    python tools/bench_eval.py --trace          # the two kernel sequences only, a fixed number of times: the program of a
                                                # `rocprofv3 --kernel-trace --stats` run of its own (profiles/eval_kernel_stats.csv)

scoring    N = 2048 in-memory records in one 256^3 room: bodies/s of PlausibilityEvaluator.scores per record (what eval_folder does)
           against scores_many.
kernel     B = 512: psi_lbs_sdf_counts against psi_lbs_forward + psi_sdf_sample_forward (out_grad NULL) + the two sign sums.
diversity  evaluation.diversity_reference on fixture C and on N = 35 000 against scipy.cluster.vq.kmeans + vq on the host; launches per
           Lloyd iteration and host synchronisations per call, counted.
Every shape is warmed up, a timed window lasts >= --window seconds and ends in a device synchronisation, old and new alternate inside
the one process, and the spread over the rounds is reported next to the median.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from psi_release_amd import body_model, evaluation, fitting, hip, ops, synth  # noqa: E402

DEV = 'cuda'
T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def window(fn, seconds):
    """Run fn() until `seconds` have passed; (calls, elapsed) with the device drained before and after.  The clock is read, behind a
    device synchronisation, each time the number of calls has doubled: short calls are not timed one by one."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, check = 0, 1
    while True:
        fn()
        n += 1
        if n == check:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
            check *= 2
    return n, time.perf_counter() - t0


def alternate(old, new, rounds, seconds):
    """Per-call seconds of `old` and `new`, alternated; dict of medians, min / max and the relative spread."""
    old()
    new()
    to, tn = [], []
    for _ in range(rounds):
        n, t = window(old, seconds)
        to.append(t / n)
        n, t = window(new, seconds)
        tn.append(t / n)
    s = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), spread=float((max(v) - min(v)) / np.median(v)))
    so, sn = s(to), s(tn)
    return dict(old=so, new=sn, ratio_old_over_new=so['median'] / sn['median'],
                faster_beyond_spread=bool(sn['max'] < so['min']), not_slower_beyond_spread=bool(sn['median'] <= so['max']))


def room_op(D):
    scene = synth.make_scene(seed=4, m=4096, D=D, n_contact=256, radius=1.9)
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.1,
           'num_iter': 1, 'batch_size': 1, 'device': torch.device(DEV), 'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None,
           'verbose': False, 'smplx_data': synth.make_smplx(7), 'vposer_state': synth.make_vposer_state(3), 'scene': scene, 'engine': 'modular'}
    return fitting.FittingOPHabitat(cfg, {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 1, 'weight_collision': 1})


def bench_scoring(a):
    N = a.records
    op = room_op(256)
    ev = evaluation.PlausibilityEvaluator(op, flip_camera_yz=True)
    recs = [synth.make_bodies(1000 + i, 1) for i in range(N)]

    def old():
        return [ev.scores(r) for r in recs]

    def new():
        xh = np.concatenate([synth.body_vector_72(r) for r in recs])
        cam = np.concatenate([r['cam_ext'][:1] for r in recs])
        return ev.scores_many(xh, cam)
    o, n = old(), new()
    dv = np.abs(np.array([c for c, _ in o]) - n[0]) * 10475.0
    res = alternate(old, new, a.rounds, a.window)
    res.update(records=N, D=256, bodies_per_s_old=N / res['old']['median'], bodies_per_s_new=N / res['new']['median'],
               largest_score_difference_in_vertices=float(dv.max()), contact_equal=bool(np.array_equal(np.array([k for _, k in o]), n[1])))
    return res


def kernel_sequences(B):
    layer = body_model.create(synth.make_smplx(7), model_type='smplx', num_pca_comps=12, batch_size=1, device=DEV)
    scene = synth.make_scene(seed=4, m=4096, D=256, n_contact=256, radius=1.9)
    sdf, gmin, gmax = T(scene.sdf[None]), T(scene.grid_min[None]), T(scene.grid_max[None])
    b = synth.make_bodies(5, B)
    rs = np.random.RandomState(6)
    shape, pose = layer._assemble(T(b['betas']), T(b['global_orient']), T(rs.standard_normal((B, 63)) * 0.2), T(b['left_hand_pose']),
                                  T(b['right_hand_pose']))
    shape, pose, transl, cam = shape.contiguous(), pose.contiguous(), T(b['transl']), T(synth.make_cam_ext(5, B))
    m = layer.lbs_model
    ws = m.workspace(B)
    verts = torch.empty(B, m.V, 3, device=DEV)
    vals = torch.empty(B, m.V, device=DEV)
    counts = torch.empty(B, 2, dtype=torch.int32, device=DEV)
    L, st = hip.lib(), hip.stream()
    keep = (layer, sdf, gmin, gmax, shape, pose, transl, cam, ws)
    out = {}

    def old():
        hip.check(L.psi_lbs_forward(m.handle, hip.ptr(shape), hip.ptr(pose), hip.ptr(transl), hip.ptr(cam), B, hip.ptr(verts), None,
                                    hip.ptr(ws), st), 'psi_lbs_forward')
        hip.check(L.psi_sdf_sample_forward(hip.ptr(sdf), None, hip.ptr(gmin), hip.ptr(gmax), hip.ptr(verts), B, m.V, 256, 1, 1,
                                           hip.ptr(vals), None, st), 'psi_sdf_sample_forward')
        out['old'] = torch.stack([(vals < 0).sum(1), (vals > 0).sum(1)], 1)

    def new():
        hip.check(L.psi_lbs_sdf_counts(m.handle, hip.ptr(shape), hip.ptr(pose), hip.ptr(transl), hip.ptr(cam), B, hip.ptr(sdf), None,
                                       hip.ptr(gmin), hip.ptr(gmax), 256, 1, 1, hip.ptr(counts), hip.ptr(ws), st), 'psi_lbs_sdf_counts')
        out['new'] = counts
    return old, new, out, keep


def bench_kernel(a):
    B = 512
    old, new, out, keep = kernel_sequences(B)
    old()
    new()
    diff = int((out['old'].to(torch.int64) - out['new'].to(torch.int64)).abs().max())
    res = alternate(old, new, max(a.rounds, 5), a.window)
    res.update(B=B, D=256, largest_count_difference=diff,
               bytes_not_moved=dict(vertex_store=B * 10475 * 12, vertex_read_back=B * 10475 * 12, sdf_values=B * 10475 * 4))
    return res


def bench_diversity(a):
    import scipy.cluster.vq as vq
    import warnings
    import fixture_inputs_eval as FE
    res = {}
    for name, x, seed in (('C', FE.body_vectors(*FE.DIV['C']['data']), FE.DIV['C']['seed']),
                          ('N35000', FE.body_vectors(4, 35000, 40, 0.2), 3)):
        stats = {}
        last = {}

        def new():
            last['gpu'] = evaluation.diversity_reference(x, seed=seed, stats=stats)

        def old():
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', DeprecationWarning)
                codes, d = vq.kmeans(x, 20, seed=seed)
            last['host'] = (d, vq.vq(x, codes))
        r = alternate(old, new, a.rounds, a.window)
        iters = stats['iters']
        r.update(N=int(x.shape[0]), host_threads=int(os.environ.get('OMP_NUM_THREADS', 0)) or None,
                 launches_per_lloyd_iteration=stats['launches_per_iteration'], launches_per_call=stats['launches'],
                 host_synchronisations_per_call=stats['syncs'], iterations_enqueued_per_synchronisation=16,
                 iterations_until_converged_max=int(max(iters)), distortion_gpu=last['gpu']['distortion'],
                 distortion_host_fp32=float(last['host'][0]), entropy_gpu=last['gpu']['entropy'])
        res[name] = r
    return res


def trace(a):
    old, new, out, keep = kernel_sequences(512)
    for _ in range(a.trace_calls):
        old()
    torch.cuda.synchronize()
    for _ in range(a.trace_calls):
        new()
    torch.cuda.synchronize()
    print('traced %d calls of each sequence' % a.trace_calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_times.json'))
    ap.add_argument('--sections', default='scoring,kernel,diversity')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--records', type=int, default=2048)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--trace_calls', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval.py measures on the GPU; no device found')
    if a.trace:
        return trace(a)
    res = {'_doc': 'tools/bench_eval.py: seconds per call (median over alternated windows of >= %.1f s, each ending in a device synchronisation; '
                   'spread = (max - min) / median over the rounds). scoring: one call = all records. old = the path of the parent commit.' % a.window,
           'device': hip.device_info()}
    fns = {'scoring': bench_scoring, 'kernel': bench_kernel, 'diversity': bench_diversity}
    for s in a.sections.split(','):
        res[s] = fns[s](a)
        print(s, json.dumps(res[s]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
