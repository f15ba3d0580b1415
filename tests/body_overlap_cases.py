"""The bodies, poses and the fp32 tolerance shared by tests/test_body_overlap_cpu.py and tests/test_body_overlap_gpu.py.

The stand-in body is ``synth.make_capsule_mesh(n_ring, n_seg)`` (r = 0.16, h = 1.7: closed, wound outwards) in six poses; a case is the
batch of the six.  ``open`` removes the bottom cap (the first n_seg faces): the surface is then not closed.

TOL_W, the fp32 tolerance on the winding number w: the kernel's statements run serially on the host (tools/body_overlap_host_check.hip)
differ from the fp64 restatement (tests/body_overlap_ref.py) by at most HOST_ERR over the four table cases; the figure and the case that
produced it stand below, measured by test_body_overlap_cpu.py::test_host_run_of_the_kernel_statements_against_restatement.  TOL_W = 4 x
HOST_ERR: the margin covers the device's arctangent, square root, division and FMA contraction, which the host run does not have (the
reasoning of TOL_F in mesh_winding_cases.py).  A decision is asserted only where the fp64 |w - 0.5| exceeds AMBIGUOUS = 0.25."""
import subprocess

import numpy as np

import body_overlap_ref as R
from psi_release_amd import synth

HOST_ERR = 2.05e-4      # 2.044e-4 measured, on the case below (2.0e-5 on the 12 x 16 cases: the error grows with F)
HOST_ERR_CASE = 'c24x46'
TOL_W = 4 * HOST_ERR
AMBIGUOUS = 0.25
RADIUS, HEIGHT = 0.16, 1.7

# (axis or None, angle, translation)
POSES = [(None, 0.0, (0.0, 0.0, 0.0)),
         ((0, 0, 1), 0.4, (0.2, 0.05, 0.0)),
         ((1, 0, 0), 1.2, (0.0, -0.6, 0.5)),
         ((0, 1, 0), 0.7, (1.5, 0.0, 0.3)),
         (None, 0.0, (0.0, 0.33, 0.0)),
         ((1, 1, 0), 2.0, (0.1, 0.1, 1.0))]

# name: (n_ring, n_seg, open)
TABLE = {'c12x16': (12, 16, False), 'c24x46': (24, 46, False), 'c12x16_open': (12, 16, True), 'c24x46_open': (24, 46, True)}
# name: F, candidates, largest pair, counts [0,1] [1,0] [5,0] [5,1], a lower bound of min |w - 0.5|
PINNED = {'c12x16': (352, 307, 94, (24, 24, 44, 85), 0.4999), 'c24x46': (2116, 1737, 544, (139, 139, 277, 492), 0.4999),
          'c12x16_open': (336, 307, 94, (24, 24, 44, 85), 0.47), 'c24x46_open': (2070, 1737, 544, (139, 139, 277, 492), 0.49)}
WORKLOAD = (68, 156)    # V = 10 454, F = 20 904: the face count of the SMPL-X surface (20 908)


def rotation(axis, angle):
    """Rodrigues, fp64."""
    if axis is None:
        return np.eye(3)
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def pose_matrices(poses=POSES):
    return [(rotation(ax, ang), np.asarray(t, np.float64)) for ax, ang, t in poses]


def posed(verts, poses=POSES, shift=(0.0, 0.0, 0.0)):
    """[B,V,3] fp32 = fp32(fp64(v) @ R^T + t) per pose (+ shift, in fp64, before the rounding)."""
    v = np.asarray(verts, np.float64)
    return np.stack([(v @ Rm.T + t + np.asarray(shift, np.float64)).astype(np.float32) for Rm, t in pose_matrices(poses)])


def capsule_sdf(points, j, poses=POSES, shift=(0.0, 0.0, 0.0)):
    """fp64 signed distance of world points to the analytic capsule of pose j (negative inside)."""
    Rm, t = pose_matrices(poses)[j]
    q = (np.asarray(points, np.float64) - t - np.asarray(shift, np.float64)) @ Rm          # R^T (p - t)
    z = np.clip(q[..., 2], RADIUS, HEIGHT - RADIUS)
    return np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2 + (q[..., 2] - z) ** 2) - RADIUS


class Case:
    def __init__(self, n_ring, n_seg, open_):
        v, f = synth.make_capsule_mesh(n_ring, n_seg, RADIUS, HEIGHT)
        self.n_ring, self.n_seg = n_ring, n_seg
        self.faces = np.ascontiguousarray(f[n_seg:] if open_ else f)
        self.verts = posed(v)
        self._ref = None

    def ref(self):
        """The restatement (counts, inside, cand, w fp64), computed once and shared, read-only."""
        if self._ref is None:
            self._ref = R.overlap(self.verts, self.faces)
            for a in self._ref:
                a.setflags(write=False)
        return self._ref


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(*TABLE[name])
    return _CASES[name]


def triple_keys(cand):
    """One int64 per (i, j, v) row, for looking triples up across batches."""
    c = np.asarray(cand, np.int64)
    return (c[:, 0] << 40) | (c[:, 1] << 20) | c[:, 2]


def write_batch(path, verts, faces, group=None):
    verts = np.ascontiguousarray(verts, np.float32)
    with open(path, 'wb') as f:
        f.write(np.array([verts.shape[0], verts.shape[1], len(faces), 0 if group is None else 1], np.int32).tobytes())
        f.write(verts.tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        if group is not None:
            f.write(np.ascontiguousarray(group, np.int32).tobytes())


def run_host_check(exe, tmp, verts, faces, group=None):
    """(counts, inside, cand, w fp32) from tools/body_overlap_host_check.hip built as ``exe``."""
    src, out = str(tmp / 'batch.bin'), str(tmp / 'out.bin')
    write_batch(src, verts, faces, group)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    B, V = np.asarray(verts).shape[:2]
    raw = open(out, 'rb').read()
    n = int(np.frombuffer(raw, np.int32, 1)[0])
    off = 4
    cand = np.frombuffer(raw, np.int32, 3 * n, off).reshape(n, 3)
    off += 12 * n
    w = np.frombuffer(raw, np.float32, n, off)
    off += 4 * n
    counts = np.frombuffer(raw, np.int32, B * B, off).reshape(B, B)
    off += 4 * B * B
    inside = np.frombuffer(raw, np.uint8, B * V, off).reshape(B, V).astype(bool)
    assert off + B * V == len(raw)
    return counts, inside, cand, w
