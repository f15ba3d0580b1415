"""The cases shared by tests/test_body_separate_scene_cpu.py and tests/test_body_separate_scene_gpu.py: the scene volumes, the bounds of the
scene statement with their derivation, the inputs of the scene kernel, the loops on c12x16 with the floor and their pinned iteration counts,
and the host-check plumbing.  Every reference is computed once, shared and read-only.

Scenes.  Closed forms sampled in fp64 at the nodes of a D = 24 grid over BOX (which holds c12x16 and its movements), rounded to fp32:
    floor    s = z + 0.005: linear, so the interpolation is exact up to rounding; no base vertex of c12x16 is nearer than 5 mm to s = 0
    corner   min(z + 0.005, x + 0.2): one kink line
    random   sdf_lookup_ref.random_volume

Bounds (C_VALUE, C_GRAD), counted as tests/sdf_lookup_ref.py counts its two statements: first-order errors in units of eps M, M the largest
|corner| of the cell, weights in [0, 1) and exact.  The statement has no fma, so a lerp(a, b, w) = a + w (b - a) of inputs of magnitude
<= m M that carry an error e costs
    the inputs' errors enter as (1 - w) e_a + w e_b                                                    -> e
    d = b - a: one rounding of |d| <= 2 m M, scaled by w                                                -> 2 m
    w d: one rounding of |w d| <= 2 m M                                                                 -> 2 m
    the sum: one rounding of |result| <= m M (a convex combination)                                     -> m
i.e. e + 5 m.  Along z, r = q0 + wz (q1 - q0) is that lerp on exact inputs (5); along y (10); along x: value -> 15 = C_VALUE.
    gx = (r[1] - r[0]) k:  err(r[.]) = 10 twice, a rounding of |gx| <= 2 M, the product's rounding      -> 24
    gy = lerp(r[0][1] - r[0][0], r[1][1] - r[1][0], wx) k:  a difference carries 5 + 5 and its own rounding of <= 2 M: 12, magnitude
         2 M; the lerp adds 5 * 2; the product's rounding 2                                             -> 24
    gz = lerp(lerp(dz00, dz01, wy), lerp(dz10, dz11, wy), wx) k:  dz carries 2, magnitude 2 M; two lerps of 10 each; the product 2  -> 24 = C_GRAD
in units of eps M k_a.  Against the real-number lookup (sdf_lookup_ref.exact_lookup) the coordinate error E_u (eu_cells) is carried into the
value by continuity (transfer_bound) and into the gradient through the other axes' weights (E_u times twice the largest node step), the
rounding of k itself times the largest node step is added, and points within E_u of a cell face or border, where the cell or the mask may
differ, are left out of the gradient comparison."""
import subprocess

import numpy as np

import body_overlap_cases as BC
import body_separate_cases as K
import body_separate_ref as R
import body_separate_scene_ref as SR
import sdf_lookup_ref as LR

D = 24
BOX = (np.array([-0.7, -2.7, -0.5], np.float32), np.array([3.1, 1.0, 2.2], np.float32))
BOX2 = (np.array([-1.0, -3.0, -0.75], np.float32), np.array([3.5, 1.25, 2.5], np.float32))      # the second scene of the S = 2 tables
FLOOR_Z = -0.005
C_VALUE, C_GRAD = 15, 24
CAP = K.CAP             # the condition of tests/body_separate_cases.py, not raised
ITERATIONS = {1.0: 29, 2.0: 17}         # the restatement's counts on c12x16 + floor (tests/test_body_separate_scene_cpu.py asserts them)
BELOW_FLOOR_WITHOUT_SCENE = 119         # vertices of the unscened loop's result with s < 0: 55 + 63 + 1 of bodies 0, 1 and 4
KERNEL_CASES = [(V, B, table) for V in (178, 256, 257, 1060) for B in (1, 6) for table in ('random', 'corner', 'both')]
_SCENES, _KERNEL, _LOOPS = {}, {}, {}


def nodes(box=BOX):
    """The node positions per axis in fp64, from the fp32 box."""
    mn, mx = box[0].astype(np.float64), box[1].astype(np.float64)
    return [mn[a] + (mx[a] - mn[a]) * np.arange(D) / (D - 1) for a in range(3)]


def scene(name, box=BOX):
    """vol [D,D,D] fp32, read-only."""
    if (name, id(box)) not in _SCENES:
        x, y, z = np.meshgrid(*nodes(box), indexing='ij')
        if name == 'floor':
            vol = z - FLOOR_Z
        elif name == 'corner':
            vol = np.minimum(z - FLOOR_Z, x + 0.2)
        else:
            vol = LR.random_volume(24, D)
        vol = np.ascontiguousarray(vol, np.float32)
        vol.setflags(write=False)
        _SCENES[(name, id(box))] = vol
    return _SCENES[(name, id(box))]


def table(name):
    """(sdf [S,D,D,D], gmin [S,3], gmax [S,3]) of 'floor', 'random', 'corner' (S = 1) or 'both' (S = 2: random in BOX, corner in BOX2)."""
    if name == 'both':
        return np.stack([scene('random'), scene('corner', BOX2)]), np.stack([BOX[0], BOX2[0]]), np.stack([BOX[1], BOX2[1]])
    return scene(name)[None], BOX[0][None], BOX[1][None]


def reference(vol, gmin, gmax, pts):
    """The fp64 lookup of pts [N,3] with the bounds of the fp32 statement against it: dict(value, grad, bv [N], bg [N,3], near [N],
    inside [N,3], cls)."""
    ex = LR.exact_lookup(vol, gmin, gmax, pts, True)
    eu = LR.eu_cells(gmin, gmax, D, True, pts)
    k32, _, k, _ = LR.cells_constants(gmin, gmax, D, True)
    bv, bg = LR.interp_bounds(ex['M'], k, C_VALUE, C_GRAD)
    steps = LR.node_steps(vol)
    mixed = np.stack([eu[:, [c for c in range(3) if c != a]].sum(1) * 2 * steps[a] * k[a] for a in range(3)], 1)
    bg = bg + mixed + (np.abs(k32.astype(np.float64) - k) * steps)[None, :]
    return {'value': ex['value'], 'grad': ex['grad'], 'bv': bv + LR.transfer_bound(vol, eu), 'bg': bg, 'near': LR.near_face(ex['u'], eu, D),
            'inside': ex['cls'] == LR.INSIDE, 'cls': ex['cls']}


def crossing_points(seed, n, box=BOX):
    """n fp32 points, uniform in the box widened by a quarter of its extent on every side: they cross every face."""
    mn, mx = box[0].astype(np.float64), box[1].astype(np.float64)
    ext = mx - mn
    return np.random.RandomState(seed).uniform(mn - 0.25 * ext, mx + 0.25 * ext, (n, 3)).astype(np.float32)


class KernelCase:
    """verts [B,V,3], p [B,3], the scene table, scene_id (None for S = 1), w_scene and the restatement's SceneWrench."""

    def __init__(self, V, B, name):
        rng = np.random.default_rng(7000 * V + 10 * B + len(name))
        if V in (178, 1060):                        # the capsule batches, every body lowered so that some of it is in the floor and the wall
            base = BC.case('c12x16' if V == 178 else 'c24x46').verts[:B]
            self.verts = (base + rng.uniform([-0.35, -0.1, -0.3], [0.0, 0.1, 0.05], size=(B, 1, 3))).astype(np.float32)
            out = crossing_points(V + B, 64)        # and 64 points around the box, at both ends of the first chunk and in the last
            self.verts[0, :32], self.verts[0, -32:] = out[:32], out[32:]
        else:
            self.verts = crossing_points(V + B, B * V).reshape(B, V, 3)
        self.p = (R.default_pivot(self.verts) + rng.normal(size=(B, 3)) * 0.05).astype(np.float32)
        self.sdf, self.gmin, self.gmax = table(name)
        self.scene_id = None
        if name == 'both':                          # both scenes, an id past the end (-> 1) and a negative one (-> 0)
            self.scene_id = np.array([1, 0, 2, -1, 0, 1][:B] if B > 1 else [5], np.int32)
        self.w_scene = (1.0, 2.0, 0.3)[(V + B) % 3]
        self.want = SR.wrench(self.verts, self.p, self.sdf, self.gmin, self.gmax, self.scene_id, self.w_scene)
        for a in (self.verts, self.p):
            a.setflags(write=False)


def kernel_case(V, B, name):
    if (V, B, name) not in _KERNEL:
        _KERNEL[(V, B, name)] = KernelCase(V, B, name)
    return _KERNEL[(V, B, name)]


def floor_scene():
    """The scene tuple (sdf, gmin, gmax, scene_id) of the loops."""
    return (scene('floor')[None], BOX[0][None], BOX[1][None], None)


def loop(w_scene):
    """(state, verts, iterations, separated, trace) of SR.separate on c12x16 + floor, max_iter = CAP; w_scene None: without a scene."""
    if w_scene not in _LOOPS:
        c = BC.case('c12x16')
        kw = {} if w_scene is None else dict(scene=floor_scene(), w_scene=w_scene)
        _LOOPS[w_scene] = SR.separate(c.verts, c.faces, max_iter=CAP, **kw)
    return _LOOPS[w_scene]


def write_batch(path, verts, p, sdf, gmin, gmax, scene_id, w_scene):
    B, V = verts.shape[:2]
    with open(path, 'wb') as f:
        f.write(np.array([B, V, sdf.shape[1], sdf.shape[0], 0 if scene_id is None else 1], np.int32).tobytes())
        f.write(np.array([w_scene], np.float32).tobytes())
        for a in (verts, p, sdf, gmin, gmax):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        if scene_id is not None:
            f.write(np.ascontiguousarray(scene_id, np.int32).tobytes())


def run_host_check(exe, tmp, verts, p, sdf, gmin, gmax, scene_id, w_scene):
    """tools/body_separate_scene_host_check.hip built as ``exe``: dict(chunks, count_chunks, loss_chunks, value, G)."""
    src, out = str(tmp / 'scene_batch.bin'), str(tmp / 'scene_out.bin')
    write_batch(src, verts, p, sdf, gmin, gmax, scene_id, w_scene)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, 'rb').read()
    B, V = verts.shape[:2]
    nchunk = (V + R.CHUNK - 1) // R.CHUNK
    at = [0]

    def take(dtype, shape):
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a

    got = dict(chunks=take(np.float64, (B, nchunk, 6)), count_chunks=take(np.int32, (B, nchunk)), loss_chunks=take(np.float64, (B, nchunk)),
               value=take(np.float32, (B, V)), G=take(np.float32, (B, V, 3)))
    assert at[0] == len(raw)
    return got


def assert_wrench(got, want, what=''):
    """``got``: dict(chunks, count_chunks, loss_chunks[, value, G]) of a host-check or GPU run; ``want``: a SceneWrench."""
    for k in ('chunks', 'count_chunks', 'loss_chunks', 'value', 'G'):
        if k in got:
            assert K.same_bits(got[k], getattr(want, k)), (what, k)
