"""fp64 reference of the SDF lookups (csrc/sdf_device.h): NumPy only, no GPU.

Three statements of the same operation, `F.grid_sample(vol, ., padding_mode='border')` behind the normalisation of fitting_proxe.py:147:

  exact_lookup   the real-number definition, in fp64: u = (x - min) / (max - min) * (D - 1) with align_corners, * D - 0.5 without;
                 clamp to [0, D - 1]; a clamped axis has zero gradient (u <= 0 and u >= D - 1 count as clamped: grid_sample's
                 clip_coordinates_set_grad uses the same non-strict tests, i.e. the gradient is non-zero STRICTLY inside), the
                 other axes keep theirs.
  cells_coords   the coordinate statement of psi_sdf_sample_cells (the fused fitting engine), operation for operation in float32:
                 k, o formed in float64 from the float32 box and rounded to float32 (psi_sdf_grid_make), then u = (x - o) * k — one
                 float32 subtract, one float32 multiply (a subtract feeding a multiply cannot be contracted into an fma, and IEEE
                 float32 subtract / multiply are correctly rounded on the GPU and in NumPy alike: this is the engine's u bit for bit),
                 median-of-three clamp, truncation, fraction, and the strict mask in = u > 0 && u < D - 1.
  cells_lookup   fp64 trilinear interpolation and gradient in the cell, with the weights and under the mask of cells_coords; the
                 gradient in grid units times the float32 k.

Bounds.  eps = 2^-24 is the unit roundoff of float32 (round to nearest): fl(a op b) = (a op b)(1 + d), |d| <= eps.

E_u, cells map (eu_cells).  With k^, o^ the rounded constants and k, o their fp64 values,
    u^ = (x - o^)(1 + d1) k^ (1 + d2),      u = (x - o) k,
    u^ - u = (x - o^) k^ ((1 + d1)(1 + d2) - 1)  +  (x - o^)(k^ - k)  +  (o - o^) k,
so  E_u = |x - o^| k^ (2 eps + eps^2) + |x - o^| |k^ - k| + |o^ - o| k + 8 * 2^-53 (|x| + |o|) k.  The two constant errors are taken as
they are (|k^ - k| <= eps k and |o^ - o| <= eps |o| would bound them; o^ = min exactly with align_corners); the last term covers the
fp64 roundings of k and o themselves (a divide, a divide, an add) and of this evaluation.

E_u, operator chain (eu_operator).  psi_axis_setup: t1 = fl(x - mn), t2 = fl(mx - mn), q = fl(t1 / t2), n = fl(2 q - 1) (the doubling
is exact), p = fl(n + 1), then u = fl(p / 2 * (D - 1)) with align_corners, u = fl(fl(p * D) - 1) / 2 without (the halvings are exact).
Every rounding adds eps times the magnitude of the value it rounds; an error carried into a later operation is scaled by that
operation's factor.  The function carries the pair (magnitude, error) through the chain, rounding(m, e) = e + eps (m + e):
    q: three roundings of s = (x - mn) / (mx - mn);   n: 2 err(q) then one rounding of |2 s - 1|;   p: err(n) then one rounding of |2 s|;
    u: err(p) (D - 1) / 2 and one rounding of |u|     (without align_corners: err(p) D and a rounding of |2 s D|, one of |2 s D - 1|, halved).

Interpolation, psi_sdf_sample_cells (C_VALUE, C_GRAD).  Operands: the eight corners q (|q| <= M), the weights wx, wy, wz in [0, 1)
(v_fract of a float is exact).  Statement: e = q_y1 - q_y0;  r_x. = fma(wy, e, q_y0);  ex = r_x1 - r_x0;  r = fma(wx, ex, r_x0) (all of
these for both z ends);  gz = r.z1 - r.z0;  value = fma(wz, gz, r.z0).  Counting first-order errors in units of eps M:
    e:  1 rounding of |e| <= 2 M                                                                      -> 2
    r_x.: wy err(e) + 1 rounding of |r_x.| <= M                                                        -> 3
    r:  the computed r_x0 enters as (1 - wx) r_x0 + wx r_x1: (1 - wx) 3 + wx 3, + wx * rounding of |ex| <= 2 M, + rounding of |r| <= M  -> 6
    value: likewise (1 - wz) 6 + wz 6 + wz * rounding of |gz| <= 2 M + rounding of |value| <= M         -> 9  = C_VALUE
    g_z = gz * k:     err(r.z1) + err(r.z0) = 12, rounding of |gz| <= 2 M, rounding of the product      -> 16
    g_x = fma(wz, ex.z1 - ex.z0, ex.z0) * k:   err(ex) = 3 + 3 + 2 = 8; (1 - wz) 8 + wz 8 + wz * rounding of |ex.z1 - ex.z0| <= 4 M,
                      rounding of |g_x| <= 2 M, rounding of the product                                  -> 16
    g_y = fma(wz, ey.z1 - ey.z0, ey.z0) * k with ey = fma(wx, e_x1 - e_x0, e_x0):   err(ey) = (1 - wx) 2 + wx 2 + wx * rounding of
                      |e_x1 - e_x0| <= 4 M + rounding of |ey| <= 2 M = 8; then as g_x                  -> 16  = C_GRAD
The gradient bounds are in grid units times k: C_GRAD eps M k_a.  The counts are first-order in eps; the neglected products of two
roundings are below C^2 eps^2 M, 1e-6 of the bound.  The worst cases behind each line (|e| = 2 M next to |r| = M ...) exclude each
other in part, so observed errors should stay well inside; profiles/sdf_lookup_bounds.json records the ratios.

Interpolation, psi_trilinear (C_VALUE_OP, C_GRAD_OP).  Three stages c = c0 * w0 + c1 * w1 with w0 = fl(1 - w1): per stage the error
of w0 (1), two products and a sum of magnitudes <= M (3), whether or not the compiler contracts a product into the sum: 4 per stage,
the stages' errors passing through with weights summing to one (+ eps)                                 -> 12 = C_VALUE_OP
    g_x = (c1 - c0) * du: err(c0) + err(c1) = 16, rounding of |c1 - c0| <= 2 M, du = scale * 2 / fl(mx - mn) has two roundings (times
    |g| <= 2 M: 4), the product 2                                                                       -> 24 = C_GRAD_OP
    g_y, g_z: differences of one-stage (error 4) or raw corners, one or two weighted stages of their own — fewer roundings than g_x.
"""
import numpy as np

EPS = 2.0 ** -24
EPS64 = 2.0 ** -53
C_VALUE, C_GRAD = 9, 16
C_VALUE_OP, C_GRAD_OP = 12, 24
assert C_VALUE <= 16 and C_GRAD <= 16

BELOW, INSIDE, ABOVE = -1, 0, 1


def _f64(a):
    return np.asarray(a, np.float64)


def _box(gmin, gmax):
    """the box as the float32 VALUES the kernels receive, held in fp64"""
    return _f64(np.asarray(gmin, np.float32)).reshape(3), _f64(np.asarray(gmax, np.float32)).reshape(3)


def exact_u(gmin, gmax, D, align_corners, pts):
    mn, mx = _box(gmin, gmax)
    s = (_f64(np.asarray(pts, np.float32)) - mn) / (mx - mn)
    return s * (D - 1) if align_corners else s * D - 0.5


def _interp(vol, cell, w):
    """fp64 trilinear value and grid-unit gradient [N,3] in cell `cell` [N,3] (0 .. D - 1; the upper corner of cell D - 1 is the last
    voxel again) at weights w [N,3]; M = the largest |corner| of the cell"""
    vol = _f64(vol)
    D = vol.shape[0]
    i0 = cell.astype(np.int64)
    i1 = np.minimum(i0 + 1, D - 1)
    c = np.empty((len(i0), 2, 2, 2))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c[:, dx, dy, dz] = vol[(i1 if dx else i0)[:, 0], (i1 if dy else i0)[:, 1], (i1 if dz else i0)[:, 2]]
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    W = [np.stack([1.0 - w[:, a], w[:, a]], 1) for a in range(3)]
    val = np.einsum('nxyz,nx,ny,nz->n', c, W[0], W[1], W[2])
    gx = np.einsum('nyz,ny,nz->n', c[:, 1] - c[:, 0], W[1], W[2])
    gy = np.einsum('nxz,nx,nz->n', c[:, :, 1] - c[:, :, 0], W[0], W[2])
    gz = np.einsum('nxy,nx,ny->n', c[:, :, :, 1] - c[:, :, :, 0], W[0], W[1])
    return val, np.stack([gx, gy, gz], 1), np.abs(c).reshape(len(i0), 8).max(1)


def exact_lookup(vol, gmin, gmax, pts, align_corners):
    """value [N], grad [N,3] (d value / d world point), u [N,3] (exact, unclamped), cls [N,3] in {BELOW, INSIDE, ABOVE}, M [N]"""
    vol = np.asarray(vol)
    D = vol.shape[0]
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    mn, mx = _box(gmin, gmax)
    u = exact_u(gmin, gmax, D, align_corners, pts)
    cls = np.where(u <= 0.0, BELOW, np.where(u >= D - 1.0, ABOVE, INSIDE)).astype(np.int8)
    uc = np.clip(u, 0.0, D - 1.0)
    cell = np.floor(uc)
    val, gg, M = _interp(vol, cell, uc - cell)
    dudx = ((D - 1) if align_corners else D) / (mx - mn)
    return {'value': val, 'grad': np.where(cls == INSIDE, gg * dudx, 0.0), 'u': u, 'cls': cls, 'M': M}


def cells_constants(gmin, gmax, D, align_corners):
    """(k, o) as float32 [3], and their fp64 values before the rounding: psi_sdf_grid_make"""
    mn, mx = _box(gmin, gmax)
    k = float(D - 1 if align_corners else D) / (mx - mn)
    o = mn + (0.0 if align_corners else 0.5 / k)
    return k.astype(np.float32), o.astype(np.float32), k, o


def cells_coords(gmin, gmax, D, align_corners, pts):
    """The engine's float32 coordinate statement: u [N,3] float32 (unclamped), cell [N,3] int, w [N,3] float32, inside [N,3] bool."""
    k32, o32, _, _ = cells_constants(gmin, gmax, D, align_corners)
    x = np.asarray(pts, np.float32).reshape(-1, 3)
    d = (x - o32).astype(np.float32)                         # one float32 subtract
    u = (d * k32).astype(np.float32)                         # one float32 multiply
    dm1 = np.float32(D - 1)
    inside = (u > np.float32(0)) & (u < dm1)
    uc = np.minimum(np.maximum(u, np.float32(0)), dm1)       # v_med3(u, 0, D - 1)
    fl = np.floor(uc)
    return {'u': u, 'cell': fl.astype(np.int64), 'w': (uc - fl).astype(np.float32), 'inside': inside}       # (uc - floor: exact = v_fract)


def cells_lookup(vol, gmin, gmax, pts, align_corners):
    """fp64 interpolation in the engine's cell with the engine's weights: value [N], grad [N,3] under the mask, grad_raw before it,
    k [3] (float32 values), M [N], and the coordinates of cells_coords"""
    D = np.asarray(vol).shape[0]
    co = cells_coords(gmin, gmax, D, align_corners, pts)
    k32 = cells_constants(gmin, gmax, D, align_corners)[0]
    val, gg, M = _interp(vol, co['cell'], _f64(co['w']))
    raw = gg * _f64(k32)
    out = dict(co)
    out.update({'value': val, 'grad_raw': raw, 'grad': np.where(co['inside'], raw, 0.0), 'k': _f64(k32), 'M': M})
    return out


def eu_cells(gmin, gmax, D, align_corners, pts):
    """bound [N,3] on |cells_coords u - exact u| (module docstring)"""
    k32, o32, k, o = cells_constants(gmin, gmax, D, align_corners)
    x = _f64(np.asarray(pts, np.float32).reshape(-1, 3))
    d = np.abs(x - _f64(o32))
    return d * _f64(k32) * (2 * EPS + EPS * EPS) + d * np.abs(_f64(k32) - k) + np.abs(_f64(o32) - o) * k + 8 * EPS64 * (np.abs(x) + np.abs(o)) * k


def _rounding(mag, err):
    return err + EPS * (mag + err)


def eu_operator(gmin, gmax, D, align_corners, pts):
    """bound [N,3] on |psi_axis_setup's float32 u - exact u| before the clamp (module docstring)"""
    mn, mx = _box(gmin, gmax)
    x = _f64(np.asarray(pts, np.float32).reshape(-1, 3))
    s = (x - mn) / (mx - mn)
    e = np.zeros_like(s)
    for _ in range(3):                                       # fl(x - mn), fl(mx - mn), the divide: three roundings of s
        e = _rounding(np.abs(s), e)
    e = _rounding(np.abs(2 * s - 1), 2 * e)                  # n = 2 q - 1
    e = _rounding(np.abs(2 * s), e)                          # p = n + 1
    if align_corners:
        return _rounding(np.abs(s * (D - 1)), e * (D - 1) / 2)
    e = _rounding(np.abs(2 * s * D), e * D)                  # p * D
    return _rounding(np.abs(2 * s * D - 1), e) / 2           # - 1, halved


def interp_bounds(M, k, c_value=C_VALUE, c_grad=C_GRAD):
    """(value bound [N], gradient bound [N,3]) of the float32 interpolation: c eps M and c_g eps M k_a"""
    M = _f64(M)
    return c_value * EPS * M, c_grad * EPS * M[:, None] * _f64(k).reshape(1, 3)


def node_steps(vol):
    """[3]: the largest |difference| of two nodes that are neighbours along each axis — the Lipschitz constants of the interpolant
    in grid units (|d f / d u_a| is a convex combination of such differences)"""
    v = _f64(vol)
    return np.array([np.abs(np.diff(v, axis=a)).max() for a in range(3)])


def transfer_bound(vol, eu):
    """|f(u') - f(u)| <= sum_a |u'_a - u_a| L_a: the trilinear interpolant behind the clamp is continuous across cell faces and
    borders, piecewise linear along each axis with slopes bounded by node_steps"""
    return (eu * node_steps(vol)[None, :]).sum(1)


def near_face(u, eu, D):
    """[N] bool: some axis lies within its E_u of an integer (cell face) or of a border — the cell or the mask of a float32 u may
    differ from the exact one's there.  u beyond the borders by more than E_u is clamped in both."""
    u = _f64(u)
    inside_band = (u > -eu) & (u < D - 1 + eu)
    return (inside_band & (np.abs(u - np.rint(u)) <= eu)).any(1)


def random_volume(seed, D):
    """iid U(-1, 1): neither smooth nor symmetric — a wrong corner, weight or mask moves a result by ~0.1"""
    return np.random.RandomState(seed).uniform(-1, 1, (D, D, D)).astype(np.float32)
