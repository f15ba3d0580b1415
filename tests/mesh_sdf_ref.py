"""NumPy restatement of the mesh -> SDF contract (include/psi_hip.h, DESIGN.md "Mesh -> SDF volume"), the arbiter of the mesh SDF tests: weld,
drop degenerate triangles, angle-weighted pseudonormals, the seven-region closest point, the sign — brute force, every node against every
kept triangle, in fp64 by default (``dtype=np.float32`` runs the same statements in fp32)."""
import numpy as np

REGIONS = ('face', 'edge ab', 'edge bc', 'edge ca', 'vertex a', 'vertex b', 'vertex c')


def weld(verts):
    """(wid [nv]: the index of the first vertex with the same position, -0.0 equal to +0.0; number of distinct positions)."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3) + np.float32(0.0)       # -0.0 + 0.0 = +0.0
    _, first, inv = np.unique(v.view(np.uint32).reshape(-1, 3), axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int64), len(first)


def prepare(verts, faces):
    """Kept triangles and their normals: dict with a, b, c [nk,3] fp64, normals [nk,7,3] fp64 (face, edges ab bc ca, vertices a b c; unit
    length or 0), ids [nk,3] welded ids, info = (kept, dropped, welded vertices, edges not shared by exactly two triangles)."""
    V = np.ascontiguousarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    if not np.isfinite(V).all() or F.min() < 0 or F.max() >= len(V):
        raise ValueError('non-finite vertex or face index out of range')
    wid, n_welded = weld(verts)
    W = wid[F]
    N = np.cross(V[W[:, 1]] - V[W[:, 0]], V[W[:, 2]] - V[W[:, 0]])
    keep = (W[:, 0] != W[:, 1]) & (W[:, 1] != W[:, 2]) & (W[:, 2] != W[:, 0]) & (N != 0).any(1)
    W, N = W[keep], N[keep]
    if not len(W):
        raise ValueError('no triangle left')
    n = N / np.linalg.norm(N, axis=1, keepdims=True)
    P = V[W]                                                       # [nk,3,3]
    vacc = np.zeros_like(V)
    for k in range(3):
        u, w = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        ang = np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(1))
        np.add.at(vacc, W[:, k], ang[:, None] * n)
    eacc, ecount = {}, {}
    for t in range(len(W)):
        for k in range(3):
            e = (min(W[t, k], W[t, (k + 1) % 3]), max(W[t, k], W[t, (k + 1) % 3]))
            eacc[e] = eacc.get(e, 0.0) + n[t]
            ecount[e] = ecount.get(e, 0) + 1

    def unit(x):
        l = np.linalg.norm(x, axis=-1, keepdims=True)
        return np.where(l > 0, x / np.where(l > 0, l, 1.0), 0.0)

    normals = np.zeros((len(W), 7, 3))
    normals[:, 0] = n
    for t in range(len(W)):
        for k in range(3):
            normals[t, 1 + k] = eacc[(min(W[t, k], W[t, (k + 1) % 3]), max(W[t, k], W[t, (k + 1) % 3]))]
    normals[:, 4:7] = vacc[W]
    normals = unit(normals)
    info = (int(len(W)), int((~keep).sum()), int(n_welded), int(sum(1 for c in ecount.values() if c != 2)))
    return {'a': P[:, 0], 'b': P[:, 1], 'c': P[:, 2], 'normals': normals, 'ids': W, 'info': info}


def closest(p, a, ab, ac):
    """The contract's routine for points p [n,1,3] against triangles [1,m,3]: (r = p - c [n,m,3], region [n,m])."""
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
    one = ap.dtype.type(1)

    def take(cond, code, value):
        m = cond & (region < 0)
        region[m] = code
        q[m] = np.broadcast_to(value, q.shape)[m]

    with np.errstate(divide='ignore', invalid='ignore'):
        take((d1 <= 0) & (d2 <= 0), 4, np.zeros_like(ab))
        take((d3 >= 0) & (d4 <= d3), 5, ab)
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1, (d1 / (d1 - d3))[..., None] * ab)
        take((d6 >= 0) & (d5 <= d6), 6, ac)
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), 3, (d2 / (d2 - d6))[..., None] * ac)
        take((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 2, ab + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (ac - ab))
        denom = one / ((va + vb) + vc)
        take(np.ones(d1.shape, bool), 0, ab * (vb * denom)[..., None] + ac * (vc * denom)[..., None])
    return ap - q, region


def node_positions(grid_min, grid_max, dim):
    """[D,D,D,3] fp32: gmin[a] + (float)i * ((gmax[a] - gmin[a]) / (float)(D - 1)), each operation rounded to fp32."""
    lo, hi = np.asarray(grid_min, np.float32).reshape(3), np.asarray(grid_max, np.float32).reshape(3)
    step = (hi - lo) / np.float32(dim - 1)
    ax = [lo[a] + np.arange(dim, dtype=np.float32) * step[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), -1).astype(np.float32)


def sdf(verts, faces, grid_min, grid_max, dim, dtype=np.float64, chunk=2048):
    """(volume [D,D,D], region histogram [7] of the winners, info)."""
    m = prepare(verts, faces)
    a32 = m['a'].astype(np.float32)
    if dtype == np.float32:                                        # the fp32 statements: b - a and c - a rounded once
        a, ab, ac = a32, m['b'].astype(np.float32) - a32, m['c'].astype(np.float32) - a32
    else:
        a, ab, ac = m['a'], m['b'] - m['a'], m['c'] - m['a']
    nrm = m['normals'].astype(np.float32).astype(dtype)            # stored as fp32
    pts = node_positions(grid_min, grid_max, dim).reshape(-1, 3).astype(dtype)
    out = np.empty(len(pts), dtype)
    hist = np.zeros(7, np.int64)
    for i in range(0, len(pts), chunk):
        p = pts[i:i + chunk]
        r, region = closest(p[:, None, :], a[None], ab[None], ac[None])
        d2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        win = d2.argmin(1)                                         # the first of equal minima: the lower index
        rows = np.arange(len(p))
        rw, reg = r[rows, win], region[rows, win]
        n = nrm[win, reg]
        side = (rw[:, 0] * n[:, 0] + rw[:, 1] * n[:, 1]) + rw[:, 2] * n[:, 2]
        d = np.sqrt(d2[rows, win])
        out[i:i + chunk] = np.where(side < 0, -d, d)
        hist += np.bincount(reg, minlength=7)
    return out.reshape(dim, dim, dim), hist, m['info']
