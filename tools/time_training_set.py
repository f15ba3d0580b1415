#!/usr/bin/env python
"""Timings of one pass of the training-record builder on the GPU (one JSON: profiles/training_set_times.json).

    python tools/time_training_set.py [--out FILE] [--frames 8] [--views 30] [--size 270 480] [--subdiv 64] [--rounds 7] [--calls 10]
    python tools/time_training_set.py --trace [--calls 20]     # the canvas call alone, a fixed number of times: the program of a
                                                               # `rocprofv3 --kernel-trace --stats` run of its own
    python tools/time_training_set.py --merge STATS_CSV [--out FILE]   # adds the two kernels' average times from that trace to the JSON

Scene as tools/time_render.py: synth.make_room_mesh(0, 180, subdiv) (subdiv = 64: ~197 k triangles).  A pass is --frames bodies standing in
the room, each seen from --views virtual cameras of the reference's lattice.  Measured with device events, alternated for --rounds rounds
after a warm-up, median and spread (max - min):

    (a) canvas_call        ops.snapshot_canvas over the pass: both modalities, the maxima and the window test of every view, one call
    (b) per_image_loop     what the package offered before: generation.data_preprocessing per view and modality on the same device tensors,
                           and rendering.view_is_usable per view (which takes the depth image to the host)
    (c) render_call        SnapshotRenderer.render of the pass, for scale

(a) is set against the bytes it must move — every input pixel read once, every canvas pixel written once — as a share of the 6.29 TB/s copy
rate of the device.  add_frames_end_to_end is the host clock around TrainingSetBuilder.add_frames + flush for the same pass (lattice, reframing,
render, canvas, copy, filters), in views and kept records per second.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psi_release_amd import generation, ops, rendering, synth  # noqa: E402
from psi_release_amd import training_data as TD  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s


def sample(fn, calls):
    """Milliseconds per call between two device events around ``calls`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def summary(ts):
    ts = sorted(ts)
    return {'median_ms': ts[len(ts) // 2], 'min_ms': ts[0], 'max_ms': ts[-1], 'spread_ms': ts[-1] - ts[0]}


def merge(a):
    with open(a.out) as f:
        out = json.load(f)
    with open(a.merge) as f:
        rows = {r['Name'].split('(')[0]: r for r in csv.DictReader(f)}
    kern = {}
    for name, r in rows.items():
        for key in ('canvas_max_kernel', 'canvas_write_kernel'):
            if key in name:
                kern[key] = kern.get(key, 0.0) + float(r['AverageNs']) / 1e3
    out['kernel_trace_us'] = kern
    if 'canvas_max_kernel' in kern:
        out['max_pass_input_rate_over_copy_rate'] = out['canvas_bytes']['input'] / (kern['canvas_max_kernel'] * 1e-6) / COPY_RATE
        out['max_pass_note'] = ('the trace repeats the call on the same inputs; where they fit the 256 MB Infinity Cache a ratio near or above 1 '
                                'means the pass was served from that cache, not from HBM')
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'training_set_times.json'))
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--views', type=int, default=30)
    ap.add_argument('--size', type=int, nargs=2, default=[270, 480])
    ap.add_argument('--subdiv', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--merge', default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a)
    if not torch.cuda.is_available():
        raise SystemExit('time_training_set.py measures on the GPU; no device found')
    room = synth.make_room_mesh(0, 180, subdiv=a.subdiv)
    mesh = rendering.SceneMesh(room.verts, room.faces, room.labels)
    data = synth.make_smplx(7)
    H, W = a.size
    f = (H / 2) / np.tan(np.radians(30.0))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    bodies = TD.synthetic_bodies(data, room.box_min, room.box_max, a.frames, seed=3)
    make = lambda: TD.TrainingSetBuilder(mesh, data, K, size=(H, W), room_planes=room.planes(), box_shrink=0.3, n_cams=a.views, grid_nodes=12,
                                         frames_per_pass=a.frames, seed=0)
    # the views of the pass, as the builder makes them
    J0, dJ0 = TD.pelvis_table(data)
    pelvis_w = bodies['transl'] + J0 + bodies['betas'] @ dJ0.T
    rng = np.random.RandomState(0)
    cams, pelvis_c = [], []
    for p in pelvis_w:
        c = rendering.sample_virtual_cams(room.box_min + 0.3, room.box_max - 0.3, p, room.planes(), 12, 0.5, rng)
        c = c[rng.permutation(len(c))[:a.views]]
        cams.append(c)
        pelvis_c.append(np.einsum('nij,j->ni', np.linalg.inv(c)[:, :3], np.append(p, 1.0)))
    cams, pelvis_c = np.concatenate(cams), np.concatenate(pelvis_c)
    n = len(cams)
    windows, z, inside = TD.target_windows(pelvis_c, K, (H, W))
    snap = rendering.SnapshotRenderer(mesh)
    depth, seg, _ = snap.render(cams, K, (H, W))
    d_win, d_z = torch.tensor(windows, device='cuda'), torch.tensor(z.astype(np.float32), device='cuda')
    canvas = lambda: ops.snapshot_canvas(depth, seg, (128, 128), d_win, d_z)
    if a.trace:
        for _ in range(a.calls):
            canvas()
        torch.cuda.synchronize()
        return
    depth_b, seg_b = depth.clone(), seg.clone()         # the loop clips in place, like the reference

    def loop():
        out = []
        for i in range(n):
            dc, _, max_d = generation.data_preprocessing(depth_b[i], 'depth', [128, 128])
            sc, _, _ = generation.data_preprocessing(seg_b[i], 'seg', [128, 128])
            out.append((dc, sc, max_d, rendering.view_is_usable(depth[i], pelvis_c[i], K)))
        return out

    render = lambda: snap.render(cams, K, (H, W))
    new, old = canvas(), loop()
    usable_new = new[4].cpu().numpy() > 0
    agree = int(sum(bool(o[3]) == bool(u) for o, u in zip(old, usable_new)))
    err = max(float((o[0] - new[0][i:i + 1]).abs().max()) for i, o in enumerate(old))
    render()
    ta, tb, tc = [], [], []
    for _ in range(a.rounds):
        ta.append(sample(canvas, a.calls))
        tb.append(sample(loop, 1))
        tc.append(sample(render, a.calls))
    sa, sb, sc_ = summary(ta), summary(tb), summary(tc)
    nbytes = {'input': int(2 * n * H * W * 4), 'output': int(2 * n * 128 * 128 * 4)}
    total = nbytes['input'] + nbytes['output']
    # the builder end to end
    make().add_frames(bodies)
    runs = []
    for _ in range(3):
        b = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.add_frames(bodies)
        b.flush()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    sec = sorted(runs)[1]
    rec = {'device': torch.cuda.get_device_name(0), 'scene_triangles': int(mesh.nf), 'frames': a.frames, 'views': n, 'size_hw': [H, W],
           'canvas_call': sa, 'per_image_loop': sb, 'render_call': sc_, 'speedup_median': sb['median_ms'] / sa['median_ms'],
           'canvas_below_loop_by_more_than_both_spreads': bool(sb['median_ms'] - sa['median_ms'] > sa['spread_ms'] + sb['spread_ms']),
           'canvas_bytes': nbytes, 'canvas_call_share_of_copy_rate': total / (sa['median_ms'] * 1e-3) / COPY_RATE,
           'usable_flags_agreeing_with_view_is_usable': '%d of %d' % (agree, n), 'max_canvas_difference_from_the_loop': err,
           'add_frames_end_to_end': {'seconds_median_of_3': sec, 'seconds_all': runs, 'views_per_s': b.stats['views_sampled'] / sec,
                                     'records_kept': b.stats['kept'], 'records_per_s': b.stats['kept'] / sec, 'stats': b.stats},
           'rounds': a.rounds, 'calls_per_sample': a.calls}
    with open(a.out, 'w') as fo:
        json.dump(rec, fo, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
