#!/usr/bin/env python
"""Timings of the result images on the GPU (one JSON: profiles/result_images_times.json).

    python tools/time_result_images.py [--out FILE] [--views 30] [--size 270 480] [--subdiv 64] [--rounds 7] [--calls 10]

Scene and cameras as tools/time_render.py: synth.make_room_mesh(0, 180, subdiv) (subdiv = 64: ~197 k triangles) seen from --views virtual
cameras inside the room.  One stand-in body per view: a capsule of 20 904 faces (SMPL-X has 20 908) standing near the point the cameras look
at.  Measured with device events, --calls calls per sample, alternated for --rounds rounds after a warm-up, median and spread:

    ResultRenderer.render    scene snapshots + normals-on-the-fly + body passes + compose, draw i = (body i, view i)
    SnapshotRenderer.render  the same views without bodies: what the renderer could do before

and their difference, the cost of the bodies.  Both calls include their host part (pose inverses, small uploads, the reads of the counts).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psi_release_amd import rendering, synth  # noqa: E402


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
    med = ts[len(ts) // 2]
    return {'median_ms': med, 'min_ms': ts[0], 'max_ms': ts[-1], 'spread_rel': (ts[-1] - ts[0]) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'result_images_times.json'))
    ap.add_argument('--views', type=int, default=30)
    ap.add_argument('--size', type=int, nargs=2, default=[270, 480])
    ap.add_argument('--subdiv', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    a = ap.parse_args()
    room = synth.make_room_mesh(0, 180, subdiv=a.subdiv)
    mesh = rendering.SceneMesh(room.verts, room.faces, room.labels, vertex_rgb=room.rgb())
    target = np.array([0.2, -0.1, 0.9])
    cams = rendering.sample_virtual_cams(room.box_min, room.box_max, target, room.planes(), grid_nodes=12, rng=np.random.RandomState(0))
    assert len(cams) >= a.views, 'only %d cameras pass the filters' % len(cams)
    cams = cams[:a.views]
    H, W = a.size
    f = (H / 2) / np.tan(np.radians(30.0))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    cv, cf = synth.make_capsule_mesh(68, 156)
    shift = np.concatenate([np.random.RandomState(1).uniform(-0.5, 0.5, (a.views, 2)) + target[:2], np.zeros((a.views, 1))], 1)
    bverts = torch.tensor((cv[None].astype(np.float64) + shift[:, None]).astype(np.float32), device='cuda')
    snap, res = rendering.SnapshotRenderer(mesh), rendering.ResultRenderer(mesh, cf)
    size = (H, W)
    with_bodies = lambda: res.render(bverts, cams, K, size)
    scene_only = lambda: snap.render(cams, K, size)
    out = with_bodies()
    counts = out.counts.cpu().numpy()
    scene_only()
    tb, ts = [], []
    for _ in range(a.rounds):
        tb.append(sample(with_bodies, a.calls))
        ts.append(sample(scene_only, a.calls))
    sb, ss = summary(tb), summary(ts)
    rec = {'device': torch.cuda.get_device_name(0), 'scene_triangles': int(mesh.nf), 'body_faces': int(len(cf)), 'views': a.views, 'draws': a.views,
           'size_hw': [H, W], 'draws_per_pass': res.pick_draws_per_pass(a.views, a.views, size),
           'body_pixels_covered': int(counts[:, 0].sum()), 'body_pixels_visible': int(counts[:, 1].sum()),
           'result_images_call': sb, 'scene_snapshots_call': ss, 'cost_of_the_bodies_ms': sb['median_ms'] - ss['median_ms'],
           'rounds': a.rounds, 'calls_per_sample': a.calls}
    with open(a.out, 'w') as fo:
        json.dump(rec, fo, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
