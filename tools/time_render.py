#!/usr/bin/env python
"""Timings of the snapshot rasteriser on the GPU (one JSON: profiles/render_times.json).

    python tools/time_render.py [--out FILE] [--views 30] [--size 270 480] [--subdiv 64] [--rounds 5] [--window 0.5]
    python tools/time_render.py --trace [--calls 20]      # the render call alone, a fixed number of times: the program of a
                                                          # `rocprofv3 --kernel-trace --stats` run of its own (profiles/render_kernel_stats.csv)
    python tools/time_render.py --merge STATS_CSV [--out FILE]   # adds the split over the kernels and the tile kernel's byte rate to the JSON

Scene: synth.make_room_mesh(0, 180, subdiv) — every box face cut into 2 * subdiv^2 triangles (subdiv = 64: ~197 k triangles) — seen from
--views virtual cameras of rendering.sample_virtual_cams inside the room.  Measured: one call with all the views against one call per
view, alternated inside the one process after a warm-up, each window >= --window seconds between device synchronisations, median and
spread over --rounds rounds.  The call includes its host part (the inverse of the poses, two small uploads, one read of the counts).
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
from psi_release_amd import rendering, synth  # noqa: E402

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of an MI355X (8.0e12 on the data sheet)
RECORD_BYTES, BIN_ENTRY_BYTES = 48, 4


def window(fn, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            return (time.perf_counter() - t0) / n


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {'median_ms': med * 1e3, 'min_ms': ts[0] * 1e3, 'max_ms': ts[-1] * 1e3, 'spread_rel': (ts[-1] - ts[0]) / med}


def setup(a):
    room = synth.make_room_mesh(0, 180, subdiv=a.subdiv)
    mesh = rendering.SceneMesh(room.verts, room.faces, room.labels)
    target = np.array([0.2, -0.1, 0.9])
    cams = rendering.sample_virtual_cams(room.box_min, room.box_max, target, room.planes(), grid_nodes=12, rng=np.random.RandomState(0))
    assert len(cams) >= a.views, 'only %d cameras pass the filters' % len(cams)
    H, W = a.size
    f = (H / 2) / np.tan(np.radians(30.0))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    return room, mesh, cams[:a.views], K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_times.json'))
    ap.add_argument('--views', type=int, default=30)
    ap.add_argument('--size', type=int, nargs=2, default=[270, 480])
    ap.add_argument('--subdiv', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--merge', default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a)
    room, mesh, cams, K = setup(a)
    r = rendering.SnapshotRenderer(mesh)
    size = tuple(a.size)
    batched = lambda: r.render(cams, K, size)
    one_by_one = lambda: [r.render(cams[i:i + 1], K, size) for i in range(len(cams))]
    if a.trace:
        for _ in range(a.calls):
            batched()
        torch.cuda.synchronize()
        return
    depth, seg, tri = batched()
    stats = r.last_stats
    one_by_one()
    tb, to = [], []
    for _ in range(a.rounds):
        tb.append(window(batched, a.window))
        to.append(window(one_by_one, a.window))
    sb, so = summary(tb), summary(to)
    out = {'device': torch.cuda.get_device_name(0), 'triangles': int(mesh.nf), 'views': len(cams), 'size_hw': list(size),
           'tile_piece_pairs': int(stats[:, 0].sum()), 'dropped_pieces': int(stats[:, 1].sum()),
           'hit_share': float((tri >= 0).float().mean()),
           'one_call_all_views': dict(sb, views_per_s=len(cams) / (sb['median_ms'] * 1e-3)),
           'one_call_per_view': dict(so, views_per_s=len(cams) / (so['median_ms'] * 1e-3)),
           'batched_speedup': so['median_ms'] / sb['median_ms'], 'rounds': a.rounds, 'window_s': a.window}
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def merge(a):
    """Per-kernel averages of a rocprofv3 --kernel-trace --stats table into the JSON: the split over the stages, and the tile kernel's time
    against the bytes it has to move (every binned record and bin entry read once, the three images written once)."""
    with open(a.out) as f:
        out = json.load(f)
    rows = {}
    with open(a.merge) as f:
        for row in csv.DictReader(f):
            m = re.search(r'rs_[a-z_]+_kernel', row.get('Name', ''))
            if m:
                rows[m.group(0)] = {'calls': int(row['Calls']), 'avg_us': float(row['AverageNs']) / 1e3, 'total_ms': float(row['TotalDurationNs']) / 1e6}
    total = sum(v['avg_us'] for v in rows.values())
    for v in rows.values():
        v['share'] = v['avg_us'] / total
    out['kernels_per_call'] = rows
    out['kernel_time_per_call_ms'] = total / 1e3
    tile = [v for k, v in rows.items() if k.startswith('rs_tile')]
    if tile:
        n, (H, W) = out['views'], out['size_hw']
        nbytes = out['tile_piece_pairs'] * (RECORD_BYTES + BIN_ENTRY_BYTES) + 3 * 4 * n * H * W
        rate = nbytes / (tile[0]['avg_us'] * 1e-6)
        out['tile_kernel'] = {'bytes_to_move': nbytes, 'avg_us': tile[0]['avg_us'], 'bytes_per_s': rate, 'share_of_hbm_rate': rate / HBM_BYTES_PER_S,
                              'hbm_rate_used': HBM_BYTES_PER_S}
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
