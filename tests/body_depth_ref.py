"""NumPy restatement of the penetration-depth contract (csrc/body_depth_shared.h, csrc/closest_point_shared.h), the
arbiter of the body-depth tests.  With ``dtype=np.float32`` every operation is one fp32 NumPy operation in the order the contract writes it,
so the GPU's rows, aggregates and gradient must have the same BITS; with ``np.float64`` the same statements are the reference the fp32
results are measured against.

    record    a = X[f0], ab = X[f1] - a, ac = X[f2] - a of face t of body j, from the fp32 vertices
    test      the seven-region closest point (tests/mesh_sdf_ref.py::closest, here with the quotients v, w it forms), d2 = (rx rx + ry ry) + rz rz
    winner    the smallest key = bits(d2) << 32 | t, unsigned (fp64: the first smallest finite d2)
    row       face, region, depth = sqrt(d2), r, bary
    aggregates and gradient as include/psi_hip.h states them: sequential sums in triple order, rows sorted stably by target"""
import numpy as np

PENALTIES = {'depth': 0, 'squared': 1}


def closest_vw(p, a, ab, ac):
    """mesh_sdf_ref.closest with the quotients: (r [n,m,3], region [n,m], v [n,m], w [n,m]); v, w are 0 where the region forms none."""
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    ap = p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = ap - ab
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = ap - ac
    d5, d6 = dot(ab, cp), dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    region = np.full(d1.shape, -1, np.int64)
    q = np.zeros(ap.shape, ap.dtype)
    v, w = np.zeros(d1.shape, ap.dtype), np.zeros(d1.shape, ap.dtype)
    one = ap.dtype.type(1)

    def take(cond, code, value, vv=None, ww=None):
        m = cond & (region < 0)
        region[m] = code
        q[m] = np.broadcast_to(value, q.shape)[m]
        if vv is not None:
            v[m] = vv[m]
        if ww is not None:
            w[m] = ww[m]

    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        take((d1 <= 0) & (d2 <= 0), 4, np.zeros_like(ab))
        take((d3 >= 0) & (d4 <= d3), 5, ab)
        v1 = d1 / (d1 - d3)
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1, v1[..., None] * ab, vv=v1)
        take((d6 >= 0) & (d5 <= d6), 6, ac)
        w3 = d2 / (d2 - d6)
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), 3, w3[..., None] * ac, ww=w3)
        w2 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        take((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 2, ab + w2[..., None] * (ac - ab), ww=w2)
        denom = one / ((va + vb) + vc)
        v0, w0 = vb * denom, vc * denom
        take(np.ones(d1.shape, bool), 0, ab * v0[..., None] + ac * w0[..., None], vv=v0, ww=w0)
    return ap - q, region, v, w


def bary_of(region, v, w):
    one, zero = v.dtype.type(1), v.dtype.type(0)
    out = np.zeros(region.shape + (3,), v.dtype)
    for code, row in ((4, (one, zero, zero)), (5, (zero, one, zero)), (6, (zero, zero, one))):
        out[region == code] = row
    m = region == 1
    out[m] = np.stack([one - v[m], v[m], np.zeros_like(v[m])], -1)
    m = region == 3
    out[m] = np.stack([one - w[m], np.zeros_like(w[m]), w[m]], -1)
    m = region == 2
    out[m] = np.stack([np.zeros_like(w[m]), one - w[m], w[m]], -1)
    m = region == 0
    out[m] = np.stack([(one - v[m]) - w[m], v[m], w[m]], -1)
    return out


def records(body_verts, faces, dtype):
    X = np.asarray(body_verts, np.float32).astype(dtype)
    f = np.asarray(faces, np.int64)
    a = X[f[:, 0]]
    return a, X[f[:, 1]] - a, X[f[:, 2]] - a


def d2_of(r):
    return (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def keys_of(d2, first_face=0):
    """[n,m] uint64 of fp32 d2 [n,m]: bits(d2) << 32 | face"""
    t = np.arange(first_face, first_face + d2.shape[1], dtype=np.uint64)
    return (np.ascontiguousarray(d2, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | t[None]


def nearest(verts, faces, trip, dtype=np.float32, block=256):
    """The rows of the triples ``trip`` [n,3]: dict of face [n] int32, region [n] int32, depth [n], d2 [n], r [n,3], bary [n,3] in
    ``dtype``, and ties [n] bool: another face has the winner's d2."""
    verts, trip = np.asarray(verts, np.float32), np.asarray(trip, np.int64).reshape(-1, 3)
    n = len(trip)
    out = {'face': np.zeros(n, np.int32), 'region': np.zeros(n, np.int32), 'depth': np.zeros(n, dtype), 'd2': np.zeros(n, dtype),
           'r': np.zeros((n, 3), dtype), 'bary': np.zeros((n, 3), dtype), 'ties': np.zeros(n, bool)}
    for j in np.unique(trip[:, 1]):
        a, ab, ac = records(verts[j], faces, dtype)
        rows_j = np.nonzero(trip[:, 1] == j)[0]
        for lo in range(0, len(rows_j), block):
            rows = rows_j[lo:lo + block]
            p = verts[trip[rows, 0], trip[rows, 2]].astype(dtype)
            r, region, v, w = closest_vw(p[:, None, :], a[None], ab[None], ac[None])
            d2 = d2_of(r)
            if dtype == np.float32:
                win = keys_of(d2).argmin(1)
            else:
                win = np.where(np.isfinite(d2), d2, np.inf).argmin(1)              # the first of equal minima: the lower face
            k = np.arange(len(rows))
            out['face'][rows], out['region'][rows] = win, region[k, win]
            out['d2'][rows], out['r'][rows] = d2[k, win], r[k, win]
            with np.errstate(invalid='ignore'):
                out['depth'][rows] = np.sqrt(d2[k, win])
            out['bary'][rows] = bary_of(region[k, win], v[k, win], w[k, win])
            out['ties'][rows] = (d2 == d2[k, win][:, None]).sum(1) > 1
    return out


def aggregates(trip, depth, B, V):
    """max_depth [B,B] fp32, sum_depth, sum_sq [B,B] fp64, depth_of [B,V] fp32, loss [2,B] fp32 of the inside triples, in triple order."""
    trip, depth = np.asarray(trip, np.int64).reshape(-1, 3), np.asarray(depth, np.float32)
    max_depth, depth_of = np.zeros((B, B), np.float32), np.zeros((B, V), np.float32)
    sum_depth, sum_sq = np.zeros((B, B)), np.zeros((B, B))
    for (i, j, v), d in zip(trip.tolist(), depth):
        dd = float(d)
        sum_depth[i, j] += dd
        sum_sq[i, j] += dd * dd
        max_depth[i, j] = max(max_depth[i, j], d)
        depth_of[i, v] = max(depth_of[i, v], d)
    loss = np.zeros((2, B), np.float32)
    for i in range(B):
        tot, tot_sq = 0.0, 0.0
        for j in range(B):
            tot += sum_depth[i, j]
            tot_sq += sum_sq[i, j]
        loss[0, i], loss[1, i] = np.float32(tot), np.float32(tot_sq)
    return max_depth, sum_depth, sum_sq, depth_of, loss


def grad_rows(trip, rows, faces, g, penalty, V):
    """targets [4n] int64 and rows [4n,3] fp32 (``rows``: the fp32 dict of ``nearest``)."""
    trip, f = np.asarray(trip, np.int64).reshape(-1, 3), np.asarray(faces, np.int64)
    n = len(trip)
    f32 = np.float32
    depth, r, bary = rows['depth'].astype(f32), rows['r'].astype(f32), rows['bary'].astype(f32)
    with np.errstate(divide='ignore'):
        s = np.full(n, f32(2)) if PENALTIES[penalty] == 1 else np.where(depth > 0, f32(1) / depth, f32(0)).astype(f32)
    u = (np.asarray(g, f32)[trip[:, 0]] * s)[:, None] * r
    targets, out = np.zeros((n, 4), np.int64), np.zeros((n, 4, 3), f32)
    targets[:, 0], out[:, 0] = trip[:, 0] * V + trip[:, 2], u
    for m in range(3):
        targets[:, 1 + m] = trip[:, 1] * V + f[rows['face'], m]
        out[:, 1 + m] = -(bary[:, m:m + 1] * u)
    return targets.reshape(-1), out.reshape(-1, 3)


def segment_sum3(targets, rows, n_out):
    """out [n_out,3] fp32: the rows sorted stably by target, every run added ((0 + x0) + x1) + ... in fp32."""
    targets, rows = np.asarray(targets, np.int64), np.asarray(rows, np.float32)
    out = np.zeros((n_out, 3), np.float32)
    order = np.argsort(targets, kind='stable')
    for k in order:
        out[targets[k]] = out[targets[k]] + rows[k]
    return out


def gradient(trip, rows, faces, g, penalty, B, V):
    targets, out = grad_rows(trip, rows, faces, g, penalty, V)
    return segment_sum3(targets, out, B * V).reshape(B, V, 3)


def select_shallow(order, max_depth, tol):
    kept = []
    for i in order:
        i = int(i)
        if i not in kept and all(max(float(max_depth[i, k]), float(max_depth[k, i])) <= tol for k in kept):
            kept.append(i)
    return kept
