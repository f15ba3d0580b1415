"""The scenes, bodies and pinned figures shared by tests/test_scene_crossings_cpu.py and tests/test_scene_crossings_gpu.py.

    plate_only   a closed plate of 1.2 x 0.8 x 0.01 m at z = 0.9 .. 0.91, every face cut into 2 x 5^2 triangles: 300 triangles
    plate_room   the plate, then ``synth.make_room_mesh(seed=0, n_extra=180, subdiv=1)``: nf = 528, three scene chunks, the last partial
    bodies       the default ``synth.make_capsule_mesh()`` (V = 178, F = 352: two body chunks, the last of 96 faces) at the four POSES:
                 0 through the plate, 1 clear of everything, 2 tilted through the plate's edge region, 3 through the plate and the floor

A reference is computed once per scene (``ref()``), shared and read-only.  Every pinned figure below is what tests/scene_crossings_ref.py
gives; test_scene_crossings_cpu.py asserts them."""
import subprocess

import numpy as np

import body_overlap_cases as BC
import scene_crossings_ref as SR
from psi_release_amd import synth

PLATE_LO, PLATE_HI = (-0.6, -0.4, 0.9), (0.6, 0.4, 0.91)
PLATE_K = 5
N_PLATE = 300
POSES = [(None, 0.0, (0.013, 0.007, 0.003)), (None, 0.0, (1.7, 1.2, 0.003)), ((0, 1, 0), 0.5, (0.35, 0.1, 0.05)),
         (None, 0.0, (0.013, 0.007, -0.4))]
# plate_room: candidates and crossing pairs per body, body-edge and scene-edge events over all pairs
CANDIDATES = (281, 20, 866, 400)
PAIRS = (124, 0, 51, 190)
BODY_EDGE_EVENTS, SCENE_EDGE_EVENTS = 596, 134
PLATE_ONLY_PAIRS_BODY0 = 92             # 46 on each plate face
# body 0 moved down to LIFT, so that only its top cap reaches plate_only: every candidate face lies in the last (96-face) body chunk
LIFT = (0.013, 0.007, -0.78)
LIFT_PAIRS, LIFT_FIRST_FACE = 70, 304


def plate_mesh():
    verts, faces, nv = [], [], 0
    for p0, du, dv, _, _ in synth._box_quads(PLATE_LO, PLATE_HI):
        v, f = synth._quad_grid(p0, du, dv, PLATE_K)
        verts.append(v)
        faces.append(f + nv)
        nv += len(v)
    return np.concatenate(verts).astype(np.float32), np.ascontiguousarray(np.concatenate(faces), dtype=np.int32)


def body_mesh():
    return synth.make_capsule_mesh()


def bodies(poses=POSES):
    v, _ = body_mesh()
    return np.ascontiguousarray(BC.posed(v, poses))


class Scene:
    def __init__(self, verts, faces):
        self.verts, self.faces = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
        self.body_verts, self.body_faces = bodies(), body_mesh()[1]
        self._ref = {}

    def cut(self, nf):
        """The scene with its first nf triangles."""
        return Scene(self.verts, self.faces[:nf])

    def ref(self, dtype=np.float32, body_verts=None):
        key = np.dtype(dtype).name
        if body_verts is not None:
            return SR.crossings(body_verts, self.body_faces, self.verts, self.faces, dtype)
        if key not in self._ref:
            r = SR.crossings(self.body_verts, self.body_faces, self.verts, self.faces, dtype)
            for a in (r.cand, r.cand_events, r.cand_mask, r.pairs, r.events, r.length, r.counts, r.contour, r.face_hit, r.tri_hit):
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        pv, pf = plate_mesh()
        if name == 'plate_only':
            _SCENES[name] = Scene(pv, pf)
        else:
            room = synth.make_room_mesh(seed=0, n_extra=180, subdiv=1)
            _SCENES[name] = Scene(np.concatenate([pv, room.verts]), np.concatenate([pf, room.faces + len(pv)]))
    return _SCENES[name]


def ascending(pairs):
    """The rows (i, s, t) are in strictly ascending lexicographic order."""
    p = np.asarray(pairs, np.int64)
    if len(p) < 2:
        return True
    d = np.diff(p, axis=0)
    first = (d != 0).argmax(1)
    return bool((d != 0).any(1).all() and (d[np.arange(len(d)), first] > 0).all())


def section_perimeter(verts, faces, z):
    """fp64 perimeter of the section of a closed triangle mesh by the plane at height z (no vertex lies on it): the segment of every
    triangle with vertices on both sides."""
    tri = np.asarray(verts, np.float64)[np.asarray(faces)]
    total = 0.0
    for t in tri:
        pts = []
        for k in range(3):
            a, b = t[k], t[(k + 1) % 3]
            if (a[2] - z) * (b[2] - z) < 0:
                pts.append(a + (a[2] - z) / (a[2] - b[2]) * (b - a))
        if len(pts) == 2:
            total += float(np.linalg.norm(pts[1] - pts[0]))
    return total


def write_batch(path, verts, faces, scene_verts, scene_faces):
    verts = np.ascontiguousarray(verts, np.float32)
    with open(path, 'wb') as f:
        f.write(np.array([verts.shape[0], verts.shape[1], len(faces), len(scene_verts), len(scene_faces)], np.int32).tobytes())
        f.write(verts.tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        f.write(np.ascontiguousarray(scene_verts, np.float32).tobytes())
        f.write(np.ascontiguousarray(scene_faces, np.int32).tobytes())


def run_host_check(exe, tmp, verts, faces, scene_verts, scene_faces):
    """What tools/scene_crossings_host_check.hip built as ``exe`` writes: (pairs [n,3], events, length fp32) of the serial run of the rule,
    and (order [nf], chunk_boxes [nK,6], box [6]) of the handle builder."""
    src, out = str(tmp / 'batch.bin'), str(tmp / 'out.bin')
    write_batch(src, verts, faces, scene_verts, scene_faces)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, 'rb').read()
    n, nf, nK = (int(x) for x in np.frombuffer(raw, np.int32, 3))
    at = 12
    pairs = np.frombuffer(raw, np.int32, 3 * n, at).reshape(n, 3)
    at += 12 * n
    events = np.frombuffer(raw, np.int32, n, at)
    at += 4 * n
    length = np.frombuffer(raw, np.float32, n, at)
    at += 4 * n
    order = np.frombuffer(raw, np.int32, nf, at)
    at += 4 * nf
    chunk_boxes = np.frombuffer(raw, np.float32, 6 * nK, at).reshape(nK, 6)
    at += 24 * nK
    box = np.frombuffer(raw, np.float32, 6, at)
    assert at + 24 == len(raw)
    return (pairs, events, length), (order, chunk_boxes, box)
