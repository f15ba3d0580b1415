"""NumPy restatement of the scene-crossing rule.

    candidate   a body face (i, s) and a scene triangle t whose closed exact face boxes meet
    decision    ``surface_crossings_ref.events_length(P = body face, Q = scene triangle)``: crosses iff events >= 1
    result      rows (i, s, t) ascending; counts [B]; contour [B] fp64, the lengths of a body added one after the other in row order;
                face_hit [B,F]; tri_hit [nf]; irregular = rows with events != 2

``morton_chunks`` restates the host half of ``psi_scene_crossings_create``: the order of the triangles and the boxes of their chunks."""
import numpy as np

import surface_crossings_ref as R


def candidates(verts, faces, scene_verts, scene_faces):
    """[n,3] int32 (i, s, t) in ascending lexicographic order."""
    verts, sv = np.asarray(verts, np.float32), np.asarray(scene_verts, np.float32)
    alo, ahi = R.face_boxes(verts[:, np.asarray(faces)])                                    # [B,F,3]
    blo, bhi = R.face_boxes(sv[np.asarray(scene_faces)])                                    # [nf,3]
    rows = []
    for i in range(len(verts)):
        s, t = np.nonzero(R._boxes_meet(alo[i], ahi[i], blo, bhi))                          # row-major: ascending (s, t)
        rows.append(np.stack([np.full(len(s), i), s, t], 1))
    return np.concatenate(rows).astype(np.int32)


def triangles_of(verts, faces, scene_verts, scene_faces, cand):
    P = np.asarray(verts, np.float32)[:, np.asarray(faces)][cand[:, 0], cand[:, 1]]
    Q = np.asarray(scene_verts, np.float32)[np.asarray(scene_faces)][cand[:, 2]]
    return P, Q


class Result:
    """What ops.scene_crossings returns, as host arrays, plus the candidates, their events and their event masks."""

    def __init__(self, B, F, nf, cand, cand_events, cand_length, cand_mask):
        hit = cand_events >= 1
        self.cand, self.cand_events, self.cand_mask = cand, cand_events, cand_mask
        self.pairs = np.ascontiguousarray(cand[hit])
        self.events, self.length = cand_events[hit], cand_length[hit]
        p = self.pairs
        self.counts = np.bincount(p[:, 0], minlength=B).astype(np.int32)
        self.contour = np.zeros(B, np.float64)
        for i in range(B):
            acc = np.float64(0.0)
            for x in self.length[p[:, 0] == i]:                                             # sequentially, in pair order
                acc = acc + np.float64(x)
            self.contour[i] = acc
        self.face_hit = np.zeros((B, F), bool)
        self.face_hit[p[:, 0], p[:, 1]] = True
        self.tri_hit = np.zeros(nf, bool)
        self.tri_hit[p[:, 2]] = True
        self.irregular = int((self.events != 2).sum())


def crossings(verts, faces, scene_verts, scene_faces, dtype=np.float32):
    verts = np.asarray(verts, np.float32)
    cand = candidates(verts, faces, scene_verts, scene_faces)
    P, Q = triangles_of(verts, faces, scene_verts, scene_faces, cand)
    ev, length, mask = R.events_length(P, Q, dtype)
    return Result(len(verts), len(faces), len(scene_faces), cand, ev, length, mask)


def _spread10(x):
    x = x.astype(np.uint32) & np.uint32(0x3ff)
    for shift, m in ((16, 0x030000ff), (8, 0x0300f00f), (4, 0x030c30c3), (2, 0x09249249)):
        x = (x | (x << np.uint32(shift))) & np.uint32(m)
    return x


def morton_chunks(scene_verts, scene_faces, chunk=256):
    """order [nf] (the caller's triangle at every position), chunk_boxes [ceil(nf / chunk), 6] and box [6], all as the handle builder states
    them: the centroid sums (v0 + v1) + v2 in fp64, quantised per axis to min(1023, trunc((c - lo) / (hi - lo) * 1024)) over their own
    bounding box (0 on an axis without extent), bits interleaved x lowest, a stable sort, boxes by comparisons."""
    tri = np.asarray(scene_verts, np.float32)[np.asarray(scene_faces)]                      # [nf,3,3]
    t64 = tri.astype(np.float64)
    c = (t64[:, 0] + t64[:, 1]) + t64[:, 2]
    lo, hi = c.min(0), c.max(0)
    w = hi - lo
    code = np.zeros(len(tri), np.uint32)
    for a in range(3):
        q = np.minimum(1023.0, (c[:, a] - lo[a]) / w[a] * 1024.0).astype(np.uint32) if w[a] > 0 else np.zeros(len(tri), np.uint32)
        code |= _spread10(q) << np.uint32(a)
    order = np.argsort(code, kind='stable').astype(np.int32)
    boxes = []
    for k in range(0, len(tri), chunk):
        pts = tri[order[k:k + chunk]].reshape(-1, 3)
        boxes.append(np.concatenate([pts.min(0), pts.max(0)]))
    boxes = np.array(boxes, np.float32)
    return order, boxes, np.concatenate([boxes[:, :3].min(0), boxes[:, 3:].max(0)])
