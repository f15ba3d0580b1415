"""The bodies and pinned figures shared by tests/test_surface_crossings_cpu.py and tests/test_surface_crossings_gpu.py.  Poses and helpers
come from tests/body_overlap_cases.py; the stand-in body is ``synth.make_capsule_mesh`` at r = 0.16, h = 1.7 unless said otherwise.

    six    the six POSES, between bodies only
    thin   a capsule of r = 0.02 turned pi/2 about x and moved by (0.013, 0.85, 0.857) through the trunk of the fat capsule: no vertex of
           either lies inside the other, yet the surfaces cross
    caps   two capsules whose hemispherical caps cross in a circle of radius sqrt(r^2 - 0.1^2)
    fold   one capsule folded onto itself: the vertices with z > h/2 turned about a pivot (self crossings)

A reference is computed once per case (``ref()``), shared and read-only.  Every pinned figure below is what tests/surface_crossings_ref.py
gives; test_surface_crossings_cpu.py asserts them."""
import subprocess

import numpy as np

import body_overlap_cases as BC
import surface_crossings_ref as R
from psi_release_amd import synth

RADIUS, HEIGHT = BC.RADIUS, BC.HEIGHT
POSES = BC.POSES
RESOLUTIONS = {'12x16': (12, 16), '24x46': (24, 46), '48x92': (48, 92)}
WORKLOAD = BC.WORKLOAD

# six: crossing pairs of the body pairs (0,1), (0,5), (1,5) (every other body pair has none) and the pairs of (0,1) with one event
SIX = {'12x16': ((62, 59, 78), 28), '24x46': ((154, 161, 204), 52)}
THIN_PAIRS = 72
CAPS_RADIUS = float(np.sqrt(RADIUS ** 2 - 0.1 ** 2))
CAPS_EXACT = 2.0 * np.pi * CAPS_RADIUS                      # 0.784770
# caps: crossing pairs and the fp64 contour of the meshes (always short of the circle: the meshes are inscribed)
CAPS = {'12x16': (70, 0.773967), '24x46': (190, 0.782417), '48x92': (386, 0.784234)}
# fold: self pairs that share no vertex, of them across the two parts / within one part
FOLD = {'12x16': (72, 61, 11), '24x46': (135, 121, 14)}


def mesh(res):
    return synth.make_capsule_mesh(*RESOLUTIONS[res], RADIUS, HEIGHT)


class Case:
    """verts [B,V,3] fp32, faces [F,3] int32 and the keyword arguments of the call."""

    def __init__(self, verts, faces, **kw):
        self.verts, self.faces, self.kw = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32), kw
        self._ref = {}

    def ref(self, dtype=np.float32):
        key = np.dtype(dtype).name
        if key not in self._ref:
            r = R.crossings(self.verts, self.faces, dtype=dtype, **self.kw)
            for a in (r.cand, r.cand_events, r.pairs, r.events, r.length, r.counts, r.contour, r.face_hit):
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]


def _six(res):
    v, f = mesh(res)
    return Case(BC.posed(v), f, self_pairs=False)


def thin_verts():
    """[2,V,3]: the fat capsule at the identity pose and the thin one (r = 0.02) through its trunk; both are 12 x 16 meshes."""
    v, f = mesh('12x16')
    tv, _ = synth.make_capsule_mesh(12, 16, 0.02, HEIGHT)
    Rm = BC.rotation((1, 0, 0), np.pi / 2)
    t = np.array([0.013, 0.85, 0.857])
    return np.stack([v, (np.asarray(tv, np.float64) @ Rm.T + t).astype(np.float32)]), f, (Rm, t)


def thin_vertex_depths():
    """fp64 signed distances (negative inside) of the thin capsule's vertices to the analytic fat capsule and of the fat capsule's to the
    analytic thin one."""
    verts, _, (Rm, t) = thin_verts()
    fat = BC.capsule_sdf(verts[1], 0)
    q = (np.asarray(verts[0], np.float64) - t) @ Rm
    z = np.clip(q[:, 2], 0.02, HEIGHT - 0.02)
    thin = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + (q[:, 2] - z) ** 2) - 0.02
    return fat, thin


def _thin():
    verts, f, _ = thin_verts()
    return Case(verts, f, self_pairs=False)


def _caps(res):
    v, f = mesh(res)
    u = np.array([0.1, -0.05, 1.0])
    u /= np.linalg.norm(u)
    cA = np.array([0.0, 0.0, HEIGHT - RADIUS])
    cB = cA + 0.2 * u
    Rm = BC.rotation((1, 2, 0), 0.2) @ BC.rotation((0, 0, 1), 0.1)
    vb = (np.asarray(v, np.float64) - np.array([0.0, 0.0, RADIUS])) @ Rm.T + cB
    return Case(np.stack([v, vb.astype(np.float32)]), f, self_pairs=False)


def fold_mesh(res):
    """verts [1,V,3], faces, upper [F] bool (at least two vertices turned)."""
    v, f = mesh(res)
    v64 = np.asarray(v, np.float64)
    turned = v64[:, 2] > HEIGHT / 2
    Rm = BC.rotation((1, 0.3, 0), 2.9) @ BC.rotation((0, 0, 1), 0.37)
    pivot = np.array([0.05, 0.02, 0.85])
    out = v64.copy()
    out[turned] = (v64[turned] - pivot) @ Rm.T + pivot
    return out.astype(np.float32)[None], f, turned[f].sum(1) >= 2


def _fold(res, parts):
    verts, f, upper = fold_mesh(res)
    if not parts:
        return Case(verts, f, between=False)
    return Case(verts, f, between=False, face_part=upper.astype(np.int32), part_skip=np.eye(2, dtype=np.uint8))


_MAKERS = {'six': _six, 'caps': _caps, 'fold': lambda res: _fold(res, False), 'fold_parts': lambda res: _fold(res, True)}
_CASES = {}


def case(name, res='12x16'):
    key = (name, res)
    if key not in _CASES:
        _CASES[key] = _thin() if name == 'thin' else _MAKERS[name](res)
    return _CASES[key]


def pair_keys(pairs):
    """One int64 per (i, s, j, t) row of a batch of at most 8 bodies, for looking pairs up across batches."""
    p = np.asarray(pairs, np.int64)
    assert p.size == 0 or (p[:, [0, 2]].max() < 8 and p[:, [1, 3]].max() < (1 << 21))
    return ((p[:, 0] * 8 + p[:, 2]) << 42) | (p[:, 1] << 21) | p[:, 3]


def ascending(pairs):
    """The rows (i, s, j, t) are in strictly ascending lexicographic order."""
    p = np.asarray(pairs, np.int64)
    if len(p) < 2:
        return True
    d = np.diff(p, axis=0)
    first = (d != 0).argmax(1)
    return bool((d != 0).any(1).all() and (d[np.arange(len(d)), first] > 0).all())


def closedness(rows, mask, faces):
    """On closed surfaces an (edge, other triangle) event occurs in exactly two pairs, because the edge has two faces.  ``mask`` [n,6] is the
    event mask of the rows (i, s, j, t): the edges of face s, then the edges of face t.  Returns {occurrences: number of (edge, triangle)}."""
    faces = np.asarray(faces, np.int64)
    rows = np.asarray(rows, np.int64)
    seen = []
    for e in range(6):
        r = rows[mask[:, e]]
        own, other = (r[:, :2], r[:, 2:]) if e < 3 else (r[:, 2:], r[:, :2])
        a, b = faces[own[:, 1], e % 3], faces[own[:, 1], (e + 1) % 3]
        seen.append(np.stack([own[:, 0], np.minimum(a, b), np.maximum(a, b), other[:, 0], other[:, 1]], 1))
    seen = np.concatenate(seen)
    _, n = np.unique(seen, axis=0, return_counts=True)
    return {int(k): int(c) for k, c in zip(*np.unique(n, return_counts=True))}


def write_batch(path, verts, faces, group=None, self_pairs=True, between=True, face_part=None, part_skip=None):
    verts = np.ascontiguousarray(verts, np.float32)
    P = 0 if face_part is None else len(part_skip)
    with open(path, 'wb') as f:
        f.write(np.array([verts.shape[0], verts.shape[1], len(faces), (1 if self_pairs else 0) | (2 if between else 0),
                          0 if group is None else 1, P], np.int32).tobytes())
        f.write(verts.tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        if group is not None:
            f.write(np.ascontiguousarray(group, np.int32).tobytes())
        if P:
            f.write(np.ascontiguousarray(face_part, np.int32).tobytes())
            f.write(np.ascontiguousarray(part_skip, np.uint8).tobytes())


def run_host_check(exe, tmp, verts, faces, **kw):
    """(pairs, events, length fp32) from tools/surface_crossings_host_check.hip built as ``exe``."""
    src, out = str(tmp / 'batch.bin'), str(tmp / 'out.bin')
    write_batch(src, verts, faces, **kw)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, 'rb').read()
    n = int(np.frombuffer(raw, np.int32, 1)[0])
    pairs = np.frombuffer(raw, np.int32, 4 * n, 4).reshape(n, 4)
    events = np.frombuffer(raw, np.int32, n, 4 + 16 * n)
    length = np.frombuffer(raw, np.float32, n, 4 + 20 * n)
    assert 4 + 24 * n == len(raw)
    return pairs, events, length
