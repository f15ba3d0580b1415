"""NumPy fp64 restatement of the winding-number contract (include/psi_hip.h, DESIGN.md "Winding-number sign"), the arbiter of the winding
tests: the kept triangles of ``mesh_sdf_ref.prepare``, the solid-angle formula, the Morton clustering, the per-brick far test (in fp32, the
statements of the kernel, so that the decisions and hence the counts are the kernel's) and the dipoles of far clusters."""
import numpy as np

import mesh_sdf_ref as R

BRICK = 8


def half_omega(p, A, B, C):
    """atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) for points p [n,1,3] and triangles [1,m,3]; atan2(0, 0) = 0."""
    a, b, c = A - p, B - p, C - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    det = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return np.where((det == 0) & (den == 0), 0.0, np.arctan2(det, den))


def morton_codes(cen):
    """10 bits per axis over the box of the centroids, x above y above z in every triple of bits."""
    lo, ext = cen.min(0), cen.max(0) - cen.min(0)
    code = np.zeros(len(cen), np.int64)
    for a in range(3):
        q = np.zeros(len(cen), np.int64)
        if ext[a] > 0:
            q = np.minimum(np.floor((cen[:, a] - lo[a]) / ext[a] * 1024.0).astype(np.int64), 1023)
        for i in range(10):
            code |= ((q >> i) & 1) << (3 * i + 2 - a)
    return code


def clusters(A, B, C, cluster):
    """(order [nk]: kept indices in cluster order; c [nc,3], r [nc], N [nc,3], stored as fp32): the triangles sorted by the Morton code of
    their centroids ((A + B) + C) / 3 (equal codes in kept order), cut into consecutive clusters; sums in the cluster's order."""
    nk = len(A)
    cen = ((A + B) + C) / 3.0
    order = np.argsort(morton_codes(cen), kind='stable')
    n = 0.5 * np.cross(B - A, C - A)
    area = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    nc = (nk + cluster - 1) // cluster
    N, wc, wsum = np.zeros((nc, 3)), np.zeros((nc, 3)), np.zeros(nc)
    for i in range(cluster):                                  # position i of every cluster that has one: the cluster's own order
        t = order[i::cluster]
        N[:len(t)] += n[t]
        wc[:len(t)] += area[t, None] * cen[t]
        wsum[:len(t)] += area[t]
    c = wc / wsum[:, None]
    r2 = np.zeros(nc)
    for i in range(cluster):
        t = order[i::cluster]
        for P in (A, B, C):
            d = P[t] - c[:len(t)]
            r2[:len(t)] = np.maximum(r2[:len(t)], (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return order, c.astype(np.float32), np.sqrt(r2).astype(np.float32), N.astype(np.float32)


def far_mask(c32, r32, lo32, hi32, beta):
    """[nc] bool, the kernel's statement in fp32: the squared distance from c to the box [lo, hi] exceeds (beta r)^2."""
    g = np.maximum(np.maximum(lo32[None] - c32, c32 - hi32[None]), np.float32(0))
    d2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    t = np.float32(beta) * r32
    return d2 > t * t


def dipole(p, c, N):
    """The contribution of far clusters (c, N [m,3]) to f at points p [n,3]: -N . (c - p) / (4 pi |c - p|^3), summed over the clusters."""
    d = c[None] - p[:, None]
    return -((N[None] * d).sum(-1) / (4.0 * np.pi * np.linalg.norm(d, axis=-1) ** 3)).sum(1)


def winding(verts, faces, grid_min, grid_max, dim, beta=0, cluster=64, chunk=4096):
    """(f [D,D,D] fp64, (exact (node, triangle) tests, (node, dipole) tests)).  beta = 0: every node against every kept triangle."""
    m = R.prepare(verts, faces)
    A, B, C = m['a'], m['b'], m['c']
    nk = len(A)
    pos32 = R.node_positions(grid_min, grid_max, dim)
    pos = pos32.astype(np.float64)
    f = np.zeros((dim, dim, dim))
    if beta == 0:
        flat = pos.reshape(-1, 3)
        out = f.reshape(-1)
        for i in range(0, len(flat), chunk):
            out[i:i + chunk] = -half_omega(flat[i:i + chunk, None], A[None], B[None], C[None]).sum(1) / (2.0 * np.pi)
        return f, (dim ** 3 * nk, 0)
    order, c32, r32, N32 = clusters(A, B, C, cluster)
    nc = len(c32)
    tri_cluster = np.arange(nk) // cluster                    # cluster of every position in cluster order
    n_exact = n_dip = 0
    for bx in range(0, dim, BRICK):
        for by in range(0, dim, BRICK):
            for bz in range(0, dim, BRICK):
                sl = (slice(bx, min(bx + BRICK, dim)), slice(by, min(by + BRICK, dim)), slice(bz, min(bz + BRICK, dim)))
                far = far_mask(c32, r32, pos32[sl][0, 0, 0], pos32[sl][-1, -1, -1], beta)
                p = pos[sl].reshape(-1, 3)
                near_t = order[~far[tri_cluster]]
                val = np.zeros(len(p))
                if len(near_t):
                    val -= half_omega(p[:, None], A[None, near_t], B[None, near_t], C[None, near_t]).sum(1) / (2.0 * np.pi)
                if far.any():
                    val += dipole(p, c32[far].astype(np.float64), N32[far].astype(np.float64))
                f[sl] = val.reshape(f[sl].shape)
                n_exact += len(p) * len(near_t)
                n_dip += len(p) * int(far.sum())
    assert nc == len(r32)
    return f, (n_exact, n_dip)
