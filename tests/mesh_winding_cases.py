"""The meshes, grids and the fp32 tolerance shared by tests/test_mesh_winding_cpu.py and tests/test_mesh_winding_gpu.py.

TOL_F, the fp32 tolerance on the winding number f: the kernel's statements run serially on the host (tools/mesh_winding_host_check.hip)
differ from the fp64 restatement (tests/mesh_winding_ref.py, same beta) by at most HOST_ERR = 4.12e-6 over all the cases below, in both arms
(the largest on the triangle soup, at nodes that graze a triangle's plane; 1.7e-6 on the rooms, 1.3e-7 on the rectangle, 1.2e-9 on the
single triangle).  TOL_F = 4 x HOST_ERR: the margin covers the device's arctangent, division, square root and FMA contraction, which the
host run does not have.  A single triangle of these coarse meshes contributes more than 1e-4 at all but grazing nodes, so a lost or doubled
record cannot hide below it."""
import subprocess

import numpy as np

import mesh_sdf_ref as R
import mesh_winding_ref as W
from psi_release_amd import synth

HOST_ERR = 4.12e-6
TOL_F = 4 * HOST_ERR
assert TOL_F <= 1e-4


class Case:
    def __init__(self, verts, faces, lo, hi, dim, room=None):
        self.verts, self.faces = np.asarray(verts, np.float32), np.asarray(faces)
        self.lo, self.hi, self.dim, self.room = np.asarray(lo, np.float32), np.asarray(hi, np.float32), dim, room
        self._ref = {}

    def ref(self, beta=0, cluster=16):
        """The restatement (f fp64, counts), computed once per (beta, cluster) and shared."""
        key = (float(beta), int(cluster) if beta else 0)
        if key not in self._ref:
            f, counts = W.winding(self.verts, self.faces, self.lo, self.hi, self.dim, beta, cluster)
            f.setflags(write=False)
            self._ref[key] = (f, counts)
        return self._ref[key]

    def positions(self):
        return R.node_positions(self.lo, self.hi, self.dim).astype(np.float64)

    def analytic(self):
        return self.room.analytic_sdf(self.positions())


def _room_case(room, dim, grow=0.17):
    return Case(room.verts, room.faces, room.box_min - np.float32(grow), room.box_max + np.float32(grow), dim, room)


def lone_box():
    """The first box of the oriented room alone: closed, oriented outward, standing in open space."""
    s = 2
    room = synth.make_oriented_room(s)
    nq, nt = (s + 1) ** 2, 2 * s * s
    return room.verts[6 * nq:12 * nq], room.faces[6 * nt:12 * nt] - 6 * nq, room.boxes[0]


RECT_V = np.array([[-1.0, -0.7, 0.013], [1.1, -0.7, 0.013], [1.1, 0.9, 0.013], [-1.0, 0.9, 0.013]], np.float32)
RECT_F = np.array([[0, 1, 2], [0, 2, 3]])
TRI_V = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.05, 0.0866, 0.0]], np.float32) + np.float32(0.3)

_MAKERS = {
    'room_s2_d24': lambda: _room_case(synth.make_oriented_room(2), 24),                    # 144 triangles, whole bricks
    'room_s6_d21': lambda: _room_case(synth.make_oriented_room(6), 21),                    # 1296 = 5 chunks + 16, partial bricks
    'room_s6_open_d21': lambda: _room_case(synth.make_open_room(6, True, 0.0), 21),        # the same without ceiling
    'soup_d24': lambda: _room_case(synth.make_room_mesh(0, 180), 24),                      # 228 triangles in general position
    'single_triangle_in_6m_box': lambda: Case(TRI_V, np.array([[0, 1, 2]]), [-3.0] * 3, [3.0] * 3, 24),
    'rectangle_in_16m_box': lambda: Case(RECT_V, RECT_F, [-8.0] * 3, [8.0] * 3, 24),
    'box_on_floor': lambda: _room_case(synth.make_open_room(2, False, 0.05), 24),          # the three defect cases
    'box_in_floor': lambda: _room_case(synth.make_open_room(2, False, 0.15), 24),
    'no_ceiling': lambda: _room_case(synth.make_open_room(2, True, 0.0), 24),
}
DEFECTS = ('box_on_floor', 'box_in_floor', 'no_ceiling')
SHAPES = ('room_s2_d24', 'room_s6_d21', 'soup_d24', 'single_triangle_in_6m_box')
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _MAKERS[name]()
    return _CASES[name]


def brick_gap(c, pos):
    """[nb,nb,nb] fp64: the distance from the point c to the node box of every 8 x 8 x 8 brick of the positions pos [D,D,D,3]."""
    D = pos.shape[0]
    nb = (D + 7) // 8
    out = np.zeros((nb, nb, nb))
    for i in range(nb):
        for j in range(nb):
            for k in range(nb):
                blk = pos[8 * i:8 * i + 8, 8 * j:8 * j + 8, 8 * k:8 * k + 8]
                lo, hi = blk[0, 0, 0], blk[-1, -1, -1]
                out[i, j, k] = np.linalg.norm(np.maximum(np.maximum(lo - c, c - hi), 0.0))
    return out


def rectangle_far_nodes(beta=3.0):
    """(mask [D,D,D] of the nodes of bricks farther than 1.05 beta r from the rectangle's one cluster, the closed-form dipole there)."""
    cs = case('rectangle_in_16m_box')
    m = R.prepare(cs.verts, cs.faces)
    _, c32, r32, N32 = W.clusters(m['a'], m['b'], m['c'], 16)
    assert len(c32) == 1
    c, r, N = c32[0].astype(np.float64), float(r32[0]), N32[0].astype(np.float64)
    # the cluster by hand: the centre of the rectangle, half its diagonal, its area along +z
    assert np.allclose(c, [0.05, 0.1, 0.013], atol=1e-6) and abs(r - np.hypot(1.05, 0.8)) < 1e-6 and np.allclose(N, [0, 0, 2.1 * 1.6], atol=1e-6)
    pos = cs.positions()
    far = brick_gap(c, pos) > 1.05 * beta * r
    mask = np.repeat(np.repeat(np.repeat(far, 8, 0), 8, 1), 8, 2)[:cs.dim, :cs.dim, :cs.dim]
    d = c - pos
    closed = -(d @ N) / (4.0 * np.pi * np.linalg.norm(d, axis=-1) ** 3)
    return mask, closed


def write_mesh(path, verts, faces):
    with open(path, 'wb') as f:
        f.write(np.array([len(verts), len(faces)], np.int32).tobytes())
        f.write(np.ascontiguousarray(verts, np.float32).tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())


def run_host_check(exe, tmp, cs, beta, cluster):
    """(f [D,D,D] fp32, (triangle tests, dipole tests)) from tools/mesh_winding_host_check.hip built as ``exe``."""
    mesh, out = str(tmp / 'mesh.bin'), str(tmp / 'f.f32')
    write_mesh(mesh, cs.verts, cs.faces)
    r = subprocess.run([exe, mesh, str(cs.dim)] + [repr(float(x)) for x in cs.lo] + [repr(float(x)) for x in cs.hi] + [repr(float(beta)), str(cluster), out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    counts = (int(words[words.index('triangle') + 2]), int(words[words.index('dipole') + 2]))
    return np.fromfile(out, np.float32).reshape(cs.dim, cs.dim, cs.dim), counts
