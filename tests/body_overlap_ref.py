"""NumPy restatement of the body-against-body overlap rule (csrc/body_overlap.hip), in fp64.

    box         of body j: the exact min / max of its V vertices per axis (fp32 values, compared as such)
    candidate   an ordered triple (i, j, v), i != j, group[i] == group[j], vertex v of body i inside the closed box of j
    w           (sum over the F triangles of body j of atan2(a . n, |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)) / 2 pi with a = A - p,
                b = B - p, c = C - p, n = (B - A) x (C - A); atan2(0, 0) = 0
    decision    vertex v of body i is inside j iff w > 0.5

The kernel's order of summation (fp32 in chunks of 256 faces, fp64 above) is a property of the fp32 implementation; here every sum is one
fp64 sum over the faces, which is the reference the fp32 results are measured against."""
import numpy as np

CHUNK, SLICE = 256, 2048


def boxes(verts):
    v = np.asarray(verts, np.float32)
    return v.min(1), v.max(1)


def half_omega(p, A, B, C):
    """[n,F] fp64: half the signed solid angle of every triangle (A, B, C [F,3]) seen from every point p [n,3]."""
    p, A, B, C = (np.asarray(x, np.float64) for x in (p, A, B, C))
    n = np.cross(B - A, C - A)
    a, b, c = A[None] - p[:, None], B[None] - p[:, None], C[None] - p[:, None]
    la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
    det = (a * n[None]).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    out = np.arctan2(det, den)
    out[(det == 0) & (den == 0)] = 0.0
    return out


def winding(points, body_verts, faces, block=512):
    """[n] fp64: the winding number of the surface (body_verts [V,3], faces [F,3]) at every point."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    tri = np.asarray(body_verts, np.float32)[np.asarray(faces)]
    out = np.empty(len(points))
    for lo in range(0, len(points), block):
        out[lo:lo + block] = half_omega(points[lo:lo + block], tri[:, 0], tri[:, 1], tri[:, 2]).sum(1) / (2.0 * np.pi)
    return out


def candidates(verts, group=None):
    """[n,3] int32 in ascending (i, j, v) order."""
    verts = np.asarray(verts, np.float32)
    B = len(verts)
    lo, hi = boxes(verts)
    rows = []
    for i in range(B):
        for j in range(B):
            if i == j or (group is not None and group[i] != group[j]):
                continue
            v = np.nonzero(((verts[i] >= lo[j]) & (verts[i] <= hi[j])).all(1))[0]
            rows.append(np.stack([np.full(len(v), i), np.full(len(v), j), v], 1))
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 3), np.int32)


def overlap(verts, faces, group=None, use_box=True):
    """counts [B,B] int32, inside [B,V] bool, cand [n,3] int32, w [n] fp64.  ``use_box=False`` evaluates every vertex of i against every
    other body j of its group (the box then saves nothing and must lose nothing)."""
    verts = np.asarray(verts, np.float32)
    B, V = verts.shape[:2]
    if use_box:
        cand = candidates(verts, group)
    else:
        cand = np.array([(i, j, v) for i in range(B) for j in range(B) if i != j and (group is None or group[i] == group[j])
                         for v in range(V)], np.int32).reshape(-1, 3)
    w = np.zeros(len(cand))
    for j in np.unique(cand[:, 1]):
        sel = cand[:, 1] == j
        w[sel] = winding(verts[cand[sel, 0], cand[sel, 2]], verts[j], faces)
    hit = w > 0.5
    counts = np.zeros((B, B), np.int32)
    np.add.at(counts, (cand[hit, 0], cand[hit, 1]), 1)
    inside = np.zeros((B, V), bool)
    inside[cand[hit, 0], cand[hit, 2]] = True
    return counts, inside, cand, w


def select_disjoint(order, counts, max_inside=0):
    """The rule of evaluation.select_disjoint, restated: walk ``order``; keep i iff counts[i,k] + counts[k,i] <= max_inside for every kept k."""
    kept = []
    for i in order:
        if all(int(counts[i, k]) + int(counts[k, i]) <= max_inside for k in kept):
            kept.append(int(i))
    return kept
