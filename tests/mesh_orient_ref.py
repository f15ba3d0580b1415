"""NumPy restatement of the orientation rule (include/psi_hip.h "orienting a scene mesh"), the arbiter of the
mesh-orientation tests: open nodes, the flood fill, the samples, the votes, the decision and the propagation.  Every floating-point
operation of the votes is fp32 and rounded where csrc/mesh_orient.hip rounds it (NumPy's fp32 +, -, *, / and sqrt are the IEEE operations,
never contracted), so votes are compared as integers.  ``U``, the unsigned distance at the nodes, is an input: the CPU tests take it from a
brute-force fp64 point-triangle distance, the GPU tests from the kernel under test's own volume."""
from collections import deque

import numpy as np

import mesh_cloud_ref as C
import mesh_sdf_ref as S

F = np.float32
VOTE, PROPAGATION, UNDECIDED, ZERO_AREA = 0, 1, -1, -2


def steps(grid_min, grid_max, dim):
    lo, hi = np.asarray(grid_min, F).reshape(3), np.asarray(grid_max, F).reshape(3)
    return (hi - lo) / F(dim - 1)


def spacing(grid_min, grid_max, dim):
    """h: the largest of the three node spacings, fp32."""
    return steps(grid_min, grid_max, dim).max()


def open_nodes(U, grid_min, grid_max):
    return np.asarray(U, F) > F(0.5) * spacing(grid_min, grid_max, U.shape[0])


def seed_nodes(seeds, grid_min, grid_max, dim):
    """[n,3] int64: rint((p - gmin) / step) in fp32; ``ValueError`` for a seed outside the grid."""
    p = np.asarray(seeds, F).reshape(-1, 3)
    r = np.rint((p - np.asarray(grid_min, F).reshape(1, 3)) / steps(grid_min, grid_max, dim)[None])
    for i, row in enumerate(r):
        if not ((row >= 0) & (row <= dim - 1)).all():
            raise ValueError('seed %d lies outside the grid' % i)
    return r.astype(np.int64)


def flood_fill(open_mask, nodes):
    """The open nodes 6-connected to a seed node through open nodes, level by level over flat indices of the mask padded with one closed
    node on every side.  A seed node outside the mask or on a node that is not open contributes nothing."""
    o = np.pad(np.asarray(open_mask) != 0, 1)
    sy, sz = o.shape[1] * o.shape[2], o.shape[2]
    flat = o.reshape(-1)
    free = np.zeros(flat.shape, bool)
    n = np.asarray(nodes, np.int64).reshape(-1, 3)
    n = n[((n >= 0) & (n < np.array(np.shape(open_mask)))).all(1)] + 1
    level = np.unique(n[:, 0] * sy + n[:, 1] * sz + n[:, 2])
    level = level[flat[level]]
    step = np.array([1, -1, sz, -sz, sy, -sy], np.int64)
    while level.size:
        free[level] = True
        nxt = (level[:, None] + step[None]).reshape(-1)
        level = np.unique(nxt[flat[nxt] & ~free[nxt]])
    return free.reshape(o.shape)[1:-1, 1:-1, 1:-1].copy()


def flood_fill_queue(open_mask, nodes):
    """The same set by a plain queue BFS: the check of ``flood_fill``."""
    o = np.asarray(open_mask) != 0
    free = np.zeros(o.shape, bool)
    q = deque()
    for n in np.asarray(nodes, np.int64).reshape(-1, 3):
        n = tuple(int(v) for v in n)
        if all(0 <= n[k] < o.shape[k] for k in range(3)) and o[n] and not free[n]:
            free[n] = True
            q.append(n)
    while q:
        x, y, z = q.popleft()
        for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            n = (x + dx, y + dy, z + dz)
            if all(0 <= n[k] < o.shape[k] for k in range(3)) and o[n] and not free[n]:
                free[n] = True
                q.append(n)
    return free


def cross_len(verts, faces):
    """(cross [nf,3], len [nf]) of (b - a) x (c - a) in fp32 with the kernel's association."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    with np.errstate(over='ignore', invalid='ignore'):
        return c, np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def centroids(verts, faces):
    """(points [k,3] fp32, tri [k] int32): ((a + b) + c) / 3 of every triangle whose cross product has a length > 0."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.nonzero(cross_len(v, f)[1] > 0)[0]
    p = ((v[f[keep, 0]] + v[f[keep, 1]]) + v[f[keep, 2]]) / F(3)
    return p.astype(F), keep.astype(np.int32)


def samples(verts, faces, h):
    """The centroids followed by the surface cloud at spacing h (tests/mesh_cloud_ref.py)."""
    cp, ct = centroids(verts, faces)
    sp, st, _, _ = C.surface_cloud(verts, faces, float(h))
    return np.concatenate([cp, sp]).astype(F), np.concatenate([ct, st]).astype(np.int32)


def votes(points, tri, verts, faces, free, grid_min, grid_max, delta):
    """[nf,2] int32: samples of each triangle whose front / back probe has a free nearest node."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    free = np.asarray(free) != 0
    D = free.shape[0]
    lo, step = np.asarray(grid_min, F).reshape(1, 3), steps(grid_min, grid_max, D)[None]
    c, ln = cross_len(v, f)
    p, t = np.asarray(points, F).reshape(-1, 3), np.asarray(tri, np.int64)
    ok = ln[t] > 0
    p, t = p[ok], t[ok]
    d = F(delta) * (c[t] / ln[t][:, None])
    out = np.zeros((len(f), 2), np.int32)
    for col, q in ((0, p + d), (1, p - d)):
        with np.errstate(invalid='ignore'):
            r = np.rint((q - lo) / step)
            inside = ((r >= 0) & (r <= F(D - 1))).all(1)
        idx = r[inside].astype(np.int64)
        hit = free[idx[:, 0], idx[:, 1], idx[:, 2]]
        np.add.at(out[:, col], t[inside][hit], 1)
    return out


def decide(vote, area_ok, ratio=4):
    """(flip [nf] bool, decided_by [nf] int8) from the votes alone."""
    Fr, B = vote[:, 0].astype(np.int64), vote[:, 1].astype(np.int64)
    keep = (Fr > 0) & (Fr >= ratio * B)
    flip = (B > 0) & (B >= ratio * Fr) & ~keep
    by = np.full(len(vote), UNDECIDED, np.int8)
    by[keep | flip] = VOTE
    by[~area_ok] = ZERO_AREA
    return flip & area_ok, by


def neighbours(verts, faces, area_ok):
    """{t: [(u, consistent)]} across the edges that exactly two triangles with area share; vertices identified by position."""
    wid, _ = S.weld(verts)
    W = wid[np.asarray(faces, np.int64).reshape(-1, 3)]
    edges = {}
    for t in np.nonzero(area_ok)[0]:
        for k in range(3):
            a, b = int(W[t, k]), int(W[t, (k + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((int(t), a < b))
    nb = {}
    for users in edges.values():
        if len(users) == 2:
            (t, dt), (u, du) = users
            if t != u:
                nb.setdefault(t, []).append((u, dt != du))
                nb.setdefault(u, []).append((t, dt != du))
    return nb


def propagate(verts, faces, flip, by):
    """Breadth-first from all decided triangles at once, level by level; an undecided triangle takes its orientation from the neighbour of
    the current level with the lowest index."""
    flip, by = flip.copy(), by.copy()
    nb = neighbours(verts, faces, by != ZERO_AREA)
    level = sorted(int(t) for t in np.nonzero(by == VOTE)[0])
    while level:
        nxt = {}
        for t in level:                                            # ascending: the first to reach u is the lowest index
            for u, consistent in nb.get(t, ()):
                if by[u] == UNDECIDED and u not in nxt:
                    nxt[u] = flip[t] if consistent else not flip[t]
        for u, fl in nxt.items():
            flip[u], by[u] = fl, PROPAGATION
        level = sorted(nxt)
    return flip, by


def apply_flips(faces, flip):
    out = np.array(faces, copy=True)
    out[flip] = out[flip][:, [0, 2, 1]]
    return out


def orient(verts, faces, seeds, U, grid_min, grid_max, ratio=4, do_propagate=True, points=None, tri=None):
    """dict(faces, flipped, votes, decided_by, free) of the whole rule with ``U`` [D,D,D] given.  ``points`` / ``tri`` replace the samples."""
    D = U.shape[0]
    h = spacing(grid_min, grid_max, D)
    opn = open_nodes(U, grid_min, grid_max)
    nodes = seed_nodes(seeds, grid_min, grid_max, D)
    for i, n in enumerate(nodes):
        if not opn[tuple(n)]:
            raise ValueError('seed %d lies on a node that is not open' % i)
    free = flood_fill(opn, nodes)
    if points is None:
        points, tri = samples(verts, faces, h)
    vt = votes(points, tri, verts, faces, free, grid_min, grid_max, F(1.5) * h)
    flip, by = decide(vt, cross_len(verts, faces)[1] > 0, ratio)
    if do_propagate:
        flip, by = propagate(verts, faces, flip, by)
    flip = flip & (by >= 0)
    return {'faces': apply_flips(faces, flip), 'flipped': flip, 'votes': vt, 'decided_by': by, 'free': free}


def brute_unsigned(verts, faces, grid_min, grid_max, dim):
    """U from the fp64 brute-force distance of tests/mesh_sdf_ref.py."""
    return np.abs(S.sdf(verts, faces, grid_min, grid_max, dim, dtype=np.float64)[0]).astype(F)
