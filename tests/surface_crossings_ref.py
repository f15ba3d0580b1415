"""NumPy restatement of the surface-crossing rule (csrc/surface_crossings_shared.h).

    face box    the exact min / max of the face's three vertices
    candidate   an unordered pair of faces ((i,s),(j,t)), (i,s) < (j,t): between: i < j, group[i] == group[j]; self: i == j, s < t, no shared
                vertex index, part_skip[face_part[s], face_part[t]] == 0; and the closed face boxes meet
    values      nP = (p1-p0) x (p2-p0), nQ alike; sP[i] = dot(nQ, p_i - q0); sQ[k] = dot(nP, q_k - p0); D[i][k] = dot((p_{i+1} - p_i) x
                (q_{k+1} - q_k), q_k - p_i); a cross component is a*b - c*d, dot = (x + y) + z
    event       edge i of P pierces Q iff sP[i], sP[i+1] strictly of opposite sign and D[i][0..2] all > 0 or all < 0; Q against P alike
    decision    crosses iff events >= 1; length (events == 2 only) = |x1 - x0|, x = a + t (b - a), t = s_a / (s_a - s_b)

``values`` / ``events_length`` run the rule in the dtype given: float32 is the restatement of the kernel (NumPy's elementwise float32
operations round once each, and it has no contraction), float64 the same rule in double.  ``independent_events`` is another statement
altogether, in fp64: every edge against the other triangle by solving for the barycentric coordinates of the piercing point."""
import numpy as np


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def values(P, Q, dtype=np.float32):
    """sP [n,3], sQ [n,3], D [n,3,3] of the triangles P, Q [n,3,3]."""
    P, Q = np.asarray(P, dtype), np.asarray(Q, dtype)
    nP = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nQ = _cross(Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0])
    sP = np.stack([_dot(nQ, P[:, i] - Q[:, 0]) for i in range(3)], 1)
    sQ = np.stack([_dot(nP, Q[:, k] - P[:, 0]) for k in range(3)], 1)
    D = np.stack([np.stack([_dot(_cross(P[:, (i + 1) % 3] - P[:, i], Q[:, (k + 1) % 3] - Q[:, k]), Q[:, k] - P[:, i]) for k in range(3)], 1)
                  for i in range(3)], 1)
    return sP, sQ, D


def _opposite(a, b):
    return ((a > 0) & (b < 0)) | ((a < 0) & (b > 0))


def event_mask(sP, sQ, D):
    """[n,6] bool: edges 0, 1, 2 of P, then edges 0, 1, 2 of Q."""
    cols = []
    for i in range(3):
        cols.append(_opposite(sP[:, i], sP[:, (i + 1) % 3]) & ((D[:, i, :] > 0).all(1) | (D[:, i, :] < 0).all(1)))
    for k in range(3):
        cols.append(_opposite(sQ[:, k], sQ[:, (k + 1) % 3]) & ((D[:, :, k] > 0).all(1) | (D[:, :, k] < 0).all(1)))
    return np.stack(cols, 1)


def events_length(P, Q, dtype=np.float32):
    """events [n] int32, length [n] of ``dtype`` (0 unless events == 2), mask [n,6]."""
    P, Q = np.asarray(P, dtype), np.asarray(Q, dtype)
    sP, sQ, D = values(P, Q, dtype)
    mask = event_mask(sP, sQ, D)
    events = mask.sum(1).astype(np.int32)
    length = np.zeros(len(P), dtype)
    two = np.nonzero(events == 2)[0]
    if len(two):
        tri = np.concatenate([P[two], Q[two]], 1)                                           # [m,6,3]: the vertices p0 p1 p2 q0 q1 q2
        s = np.concatenate([sP[two], sQ[two]], 1)                                           # [m,6] their plane values
        nxt = np.array([1, 2, 0, 4, 5, 3])
        e = np.nonzero(mask[two])[1].reshape(-1, 2)                                         # the two edges, in the order P then Q
        rows = np.arange(len(two))
        pts = []
        for c in range(2):
            a, b = tri[rows, e[:, c]], tri[rows, nxt[e[:, c]]]
            sa, sb = s[rows, e[:, c]], s[rows, nxt[e[:, c]]]
            t = sa / (sa - sb)
            pts.append(a + t[:, None] * (b - a))
        d = pts[1] - pts[0]
        length[two] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return events, length, mask


DOUBT = 1e-9      # an fp64 barycentric coordinate this close to a bound is decided in exact rational arithmetic


def _exact_pierces(a, b, c0, c1, c2):
    """The same system in exact rationals (every fp32 / fp64 input is a rational): strict inequalities, zero determinant is no event."""
    from fractions import Fraction
    a, b, c0, c1, c2 = ([Fraction(float(x)) for x in v] for v in (a, b, c0, c1, c2))
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]
    cross = lambda x, y: [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    e1, e2, d, s = sub(c1, c0), sub(c2, c0), sub(b, a), sub(a, c0)
    h = cross(d, e2)
    det = dot(e1, h)
    if det == 0:
        return False
    qv = cross(s, e1)
    u, v, t = dot(s, h) / det, dot(d, qv) / det, dot(e2, qv) / det
    return 0 < t < 1 and u > 0 and v > 0 and u + v < 1


def independent_events(P, Q):
    """events [n] and mask [n,6] by another route: the edge a + t (b - a) against the triangle c0 + u (c1 - c0) + v (c2 - c0), solved for
    (t, u, v) by Cramer's rule in fp64; pierces iff 0 < t < 1, u > 0, v > 0, u + v < 1, all strict; a zero determinant is no event.  Where
    fp64 leaves a coordinate within DOUBT of a bound (an edge through an edge, as between two capsules with rings at equal heights), the
    same system is solved in exact rational arithmetic, so no candidate is left undecided."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    cols = []
    for E, T in ((P, Q), (Q, P)):
        e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
        for i in range(3):
            a, b = E[:, i], E[:, (i + 1) % 3]
            d = b - a
            h = np.cross(d, e2)
            det = (e1 * h).sum(1)
            ok = det != 0
            f = 1.0 / np.where(ok, det, 1.0)
            s = a - T[:, 0]
            u = f * (s * h).sum(1)
            qv = np.cross(s, e1)
            v = f * (d * qv).sum(1)
            t = f * (e2 * qv).sum(1)
            col = ok & (t > 0) & (t < 1) & (u > 0) & (v > 0) & (u + v < 1)
            near = np.minimum.reduce([np.abs(t), np.abs(1 - t), np.abs(u), np.abs(v), np.abs(1 - u - v)]) < DOUBT
            for r in np.nonzero(near | ~ok)[0]:
                col[r] = _exact_pierces(a[r], b[r], T[r, 0], T[r, 1], T[r, 2])
            cols.append(col)
    mask = np.stack(cols, 1)
    return mask.sum(1).astype(np.int32), mask


def face_boxes(tri):
    """lo, hi [..,3] of triangles [..,3,3] (fp32 values, compared as such)."""
    return tri.min(-2), tri.max(-2)


def _boxes_meet(alo, ahi, blo, bhi):
    """[Fa,Fb] bool"""
    return ((alo[:, None, :] <= bhi[None, :, :]) & (blo[None, :, :] <= ahi[:, None, :])).all(-1)


def candidates(verts, faces, group=None, self_pairs=True, between=True, face_part=None, part_skip=None):
    """[n,4] int32 (i, s, j, t) in ascending lexicographic order."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces)
    B, F = len(verts), len(faces)
    lo, hi = face_boxes(verts[:, faces])                                                    # [B,F,3]
    rows = []
    for i in range(B):
        for j in range(i, B):
            if i == j and not self_pairs or i != j and not between:
                continue
            if i != j and group is not None and group[i] != group[j]:
                continue
            meet = _boxes_meet(lo[i], hi[i], lo[j], hi[j])
            if i == j:
                share = (faces[:, None, :, None] == faces[None, :, None, :]).any((2, 3))
                meet &= ~share & np.triu(np.ones((F, F), bool), 1)
                if face_part is not None:
                    fp = np.asarray(face_part)
                    meet &= np.asarray(part_skip)[fp[:, None], fp[None, :]] == 0
            s, t = np.nonzero(meet)
            rows.append(np.stack([np.full(len(s), i), s, np.full(len(s), j), t], 1))
    c = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)
    return c[np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))]


def triangles_of(verts, faces, cand):
    tri = np.asarray(verts, np.float32)[:, np.asarray(faces)]                               # [B,F,3,3]
    return tri[cand[:, 0], cand[:, 1]], tri[cand[:, 2], cand[:, 3]]


class Result:
    """What ops.surface_crossings returns, as host arrays, plus the candidates and their events."""

    def __init__(self, B, F, cand, cand_events, cand_length):
        hit = cand_events >= 1
        self.cand, self.cand_events = cand, cand_events
        self.pairs = np.ascontiguousarray(cand[hit])
        self.events = cand_events[hit]
        self.length = cand_length[hit]
        self.counts = np.zeros((B, B), np.int32)
        self.contour = np.zeros((B, B), np.float64)
        self.face_hit = np.zeros((B, F), bool)
        p = self.pairs
        np.add.at(self.counts, (p[:, 0], p[:, 2]), 1)
        off = p[:, 0] != p[:, 2]
        np.add.at(self.counts, (p[off, 2], p[off, 0]), 1)
        self.face_hit[p[:, 0], p[:, 1]] = True
        self.face_hit[p[:, 2], p[:, 3]] = True
        for i, j in sorted(set(zip(p[:, 0].tolist(), p[:, 2].tolist()))):
            acc = np.float64(0.0)
            for x in self.length[(p[:, 0] == i) & (p[:, 2] == j)]:                          # sequentially, in pair order
                acc = acc + np.float64(x)
            self.contour[i, j] = self.contour[j, i] = acc
        self.irregular = int((self.events != 2).sum())


def crossings(verts, faces, group=None, self_pairs=True, between=True, face_part=None, part_skip=None, dtype=np.float32):
    verts = np.asarray(verts, np.float32)
    cand = candidates(verts, faces, group, self_pairs, between, face_part, part_skip)
    P, Q = triangles_of(verts, faces, cand)
    ev, length, _ = events_length(P, Q, dtype)
    return Result(len(verts), len(faces), cand, ev, length)


def face_parts(weights, faces):
    """The rule of evaluation.face_parts, restated with a loop."""
    w = np.asarray(weights, np.float64)
    out = []
    for f in np.asarray(faces):
        s = w[f[0]] + w[f[1]] + w[f[2]]
        out.append(int(np.nonzero(s == s.max())[0][0]))
    return np.array(out, np.int32)
