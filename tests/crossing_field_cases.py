"""The cases shared by tests/test_crossing_field_cpu.py and tests/test_crossing_field_gpu.py: the bodies of tests/surface_crossings_cases.py,
each with sigma = 1e-3 (the default) and sigma = 0.5, a planted list with exact zeros, and the host-check plumbing.  A reference is
computed once per (case, sigma), shared and read-only."""
import subprocess

import numpy as np

import crossing_field_ref as FR
import surface_crossings_cases as SC

SIGMAS = (1e-3, 0.5)
# (name, resolution): the crossing pairs of each are pinned by tests/surface_crossings_cases.py
CASES = [('thin', '12x16'), ('caps', '12x16'), ('fold', '12x16'), ('fold_parts', '12x16'), ('six', '12x16'), ('six', '24x46')]
PAIR_COUNTS = {('thin', '12x16'): 72, ('caps', '12x16'): 70, ('fold', '12x16'): 72, ('six', '12x16'): 199, ('six', '24x46'): 519}
UNEVEN_G = np.array([1.0, -0.5, 2.0, 0.25, 3.0, -1.5], np.float32)
_REFS = {}


def uneven_g(B):
    return UNEVEN_G[:B].copy()


class FieldRef:
    """The fp32 restatement of a pair list: psi, energy, pair_energy, loss, and G for g = 1 and an uneven g."""

    def __init__(self, verts, faces, pairs, sigma):
        B = len(verts)
        self.pairs = np.ascontiguousarray(pairs, np.int32)
        self.psi, self.energy = FR.field(verts, faces, pairs, sigma)
        self.pair_energy, self.loss = FR.aggregates(pairs, self.energy, B)
        self.g = {'ones': np.ones(B, np.float32), 'uneven': uneven_g(B)}
        self.rows, self.G = {}, {}
        for name, g in self.g.items():
            self.rows[name], self.targets, self.G[name] = FR.grad(verts, faces, pairs, sigma, g)
        for a in (self.pairs, self.psi, self.energy, self.pair_energy, self.loss, self.targets, *self.rows.values(), *self.G.values()):
            a.setflags(write=False)


def ref(name, res, sigma, which='pairs'):
    """The FieldRef of the crossing pairs (``which='pairs'``) or of all candidates (``'cand'``) of a case."""
    key = (name, res, sigma, which)
    if key not in _REFS:
        c = SC.case(name, res)
        r = c.ref()
        _REFS[key] = FieldRef(c.verts, c.faces, r.pairs if which == 'pairs' else r.cand, sigma)
    return _REFS[key]


def planted():
    """verts [2,V,3], faces, pairs and what the rule gives exactly, with sigma = 0.5.  Receiver face 0 of body 1 is the right triangle
    (0,0,0) (2,0,0) (0,2,0): circumcentre (1,1,0), r = sqrt 2, n = (0,0,1).  Face 1 of body 1 is collinear.  The faces of body 0:
        0  three vertices exactly on the receiver's plane outside the circumcircle (h = 0, Phi >= 1): gate 2
        1  three vertices exactly on the plane h = sigma, the apex (1,1,0.5) among them: gate 1
        2  the circumcentre itself (rho = 0, Psi = c0 = (3 - 2 sigma) / 4 = 0.5), and two points beyond the gates
    Against the collinear receiver every Psi is 0.  The receivers' own corners, evaluated in the faces of body 0, are whatever the rule
    gives: only role 0 is pinned."""
    body1 = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [5, 5, 5], [6, 6, 6], [8, 8, 8], [0, 0, 9], [1, 0, 9], [0, 1, 9]], np.float32)
    body0 = np.array([[3, 3, 0], [-2, 1, 0], [1, 4, 0], [1, 1, 0.5], [0, 0, 0.5], [1.5, 0.5, 0.5], [1, 1, 0], [9, 9, 0.25], [1, 1, 2]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    pairs = np.array([[0, 0, 1, 0], [0, 0, 1, 1], [0, 1, 1, 0], [0, 1, 1, 1], [0, 2, 1, 0], [0, 2, 1, 1]], np.int32)
    psi0 = np.zeros((6, 3), np.float32)
    psi0[4, 0] = 0.5
    return np.stack([body0, body1]), faces, pairs, psi0


def write_batch(path, verts, faces, pairs, sigma, g):
    verts = np.ascontiguousarray(verts, np.float32)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 4)
    with open(path, 'wb') as f:
        f.write(np.array([verts.shape[0], verts.shape[1], len(faces), len(pairs)], np.int32).tobytes())
        f.write(np.float32(sigma).tobytes())
        f.write(verts.tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        f.write(pairs.tobytes())
        f.write(np.ascontiguousarray(g, np.float32).tobytes())


def run_host_check(exe, tmp, verts, faces, pairs, sigma, g):
    """dict(psi, energy, rows, targets, G, pair_energy, loss) from tools/crossing_field_host_check.hip built as ``exe``."""
    src, out = str(tmp / 'batch.bin'), str(tmp / 'out.bin')
    write_batch(src, verts, faces, pairs, sigma, g)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, 'rb').read()
    B, V = np.asarray(verts).shape[:2]
    n = int(np.frombuffer(raw, np.int32, 1)[0])
    at = [4]

    def take(dtype, count, shape):
        a = np.frombuffer(raw, dtype, count, at[0]).reshape(shape)
        at[0] += a.nbytes
        return a

    res = dict(psi=take(np.float32, 6 * n, (n, 2, 3)), energy=take(np.float32, 2 * n, (n, 2)), rows=take(np.float32, 36 * n, (2 * n, 6, 3)),
               targets=take(np.int64, 12 * n, (2 * n, 6)), G=take(np.float32, B * V * 3, (B, V, 3)),
               pair_energy=take(np.float64, B * B, (B, B)), loss=take(np.float32, B, (B,)))
    assert at[0] == len(raw)
    return res


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
