"""NumPy restatement of the snapshot rasteriser's contract (include/psi_hip.h, DESIGN.md "Snapshot rasteriser"), the arbiter of the render tests.

* ``setup_pieces``   stage (a) in fp32 with the contract's association: camera space, near clip, projection, snapping, the 2^28 guard,
                     zero-area removal, re-winding — numpy's float32 operators round once per operation, like the uncontracted kernel
* ``render_ref``     exact integer coverage (top-left rule) of those pieces, then depth and label interpolated in fp64 from the same
                     snapped integer coordinates and fp32 camera-space z: nearest and second-nearest depth per pixel
* ``raycast_fp64``   an independent brute-force fp64 ray / triangle intersection (no snapping, no clipping), the check of the restatement itself
"""
import numpy as np

F = np.float32
SUB = 256
GUARD = 2 ** 28


def world_to_camera_rows(cam_ext):
    """[n,3,4] fp32: the fp64 inverse of camera-to-world [n,4,4], rounded once."""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(cam_ext, np.float64).reshape(-1, 4, 4))[:, :3, :], dtype=F)


def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def _camera(verts, m):
    X, Y, Z = (verts[:, i].astype(F) for i in range(3))
    row = lambda r: ((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * Z) + m[r, 3]
    return np.stack([row(0), row(1), row(2)], -1).astype(F)


def _clip(a, b, near):
    """a, b: [k,4] fp32 (x, y, z, label), a inside: the point of a -> b on z = near."""
    t = ((near - a[:, 2]) / (b[:, 2] - a[:, 2])).astype(F)
    return (a + t[:, None] * (b - a)).astype(F)


def setup_pieces(verts, faces, labels, w2c, intr, near=0.05):
    """Pieces of one view.  Returns dict: U, V [p,3] int64; z [p,3] fp32 camera-space depth of the piece's vertices; lab [p,3] fp32;
    tri [p] triangle index; dropped = number of pieces the 2^28 guard removed."""
    m = np.asarray(w2c, F).reshape(3, 4)
    fx, fy, cx, cy = (F(v) for v in np.asarray(intr, F).reshape(4))
    near = F(near)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.zeros(len(verts), F) if labels is None else np.asarray(labels, F)
    cam = np.concatenate([_camera(np.asarray(verts, F), m), lab[:, None]], -1)          # [nv,4]
    tv = cam[faces]                                                                       # [nf,3,4]
    inside = tv[:, :, 2] >= near
    nin = inside.sum(1)
    tris, ids = [], []
    idx = np.nonzero(nin == 3)[0]
    tris.append(tv[idx])
    ids.append(idx)
    idx = np.nonzero(nin == 1)[0]
    if len(idx):
        i = inside[idx].argmax(1)
        a, b, c = (tv[idx, (i + k) % 3] for k in range(3))
        tris.append(np.stack([a, _clip(a, b, near), _clip(a, c, near)], 1))
        ids.append(idx)
    idx = np.nonzero(nin == 2)[0]
    if len(idx):
        i = inside[idx].argmin(1)
        c, a, b = (tv[idx, (i + k) % 3] for k in range(3))
        bc, ac = _clip(b, c, near), _clip(a, c, near)
        tris += [np.stack([a, b, bc], 1), np.stack([a, bc, ac], 1)]
        ids += [idx, idx]
    P = np.concatenate(tris, 0).astype(F)                                                 # [p,3,4]
    tri = np.concatenate(ids)
    with np.errstate(all='ignore'):
        u = ((fx * P[:, :, 0]) / P[:, :, 2] + cx).astype(F)
        v = ((fy * P[:, :, 1]) / P[:, :, 2] + cy).astype(F)
        ru, rv = np.rint(u * F(SUB)), np.rint(v * F(SUB))
        ok = ((np.abs(ru) <= GUARD) & (np.abs(rv) <= GUARD)).all(1)
    dropped = int((~ok).sum())
    P, tri, ru, rv = P[ok], tri[ok], ru[ok], rv[ok]
    U, V = ru.astype(np.int64), rv.astype(np.int64)
    area = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
    keep = area != 0
    U, V, P, tri, area = U[keep], V[keep], P[keep], tri[keep], area[keep]
    flip = area < 0
    order = np.where(flip[:, None], np.array([[0, 2, 1]]), np.array([[0, 1, 2]]))
    r = np.arange(len(U))[:, None]
    return {'U': U[r, order], 'V': V[r, order], 'z': P[r, order, 2], 'lab': P[r, order, 3], 'tri': tri, 'dropped': dropped}


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns_tie(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (dy > 0) or (dy == 0 and dx < 0)


def render_ref(pieces, W, H):
    """Returns dict of [H,W] arrays: hit (bool), tri (int64, -1), depth, seg (fp64, 0 where no hit), depth2 (second-nearest depth, inf when
    there is none), clear = the two nearest depths differ by more than 1e-4 relative (or only one piece covers the pixel)."""
    d1 = np.full((H, W), np.inf)
    d2 = np.full((H, W), np.inf)
    t1 = np.full((H, W), -1, np.int64)
    s1 = np.zeros((H, W))
    U, V, Z, L, T = pieces['U'], pieces['V'], pieces['z'].astype(np.float64), pieces['lab'].astype(np.float64), pieces['tri']
    for p in range(len(T)):
        u, v = U[p], V[p]
        x0, x1 = max(0, (int(u.min()) - 128 + 255) >> 8), min(W - 1, (int(u.max()) - 128) >> 8)
        y0, y1 = max(0, (int(v.min()) - 128 + 255) >> 8), min(H - 1, (int(v.max()) - 128) >> 8)
        if x0 > x1 or y0 > y1:
            continue
        sx = (np.arange(x0, x1 + 1, dtype=np.int64) * SUB + 128)[None, :]
        sy = (np.arange(y0, y1 + 1, dtype=np.int64) * SUB + 128)[:, None]
        e, inside = [], True
        for a, b in ((1, 2), (2, 0), (0, 1)):
            ei = _edge(u[a], v[a], u[b], v[b], sx, sy)
            e.append(ei)
            inside = inside & ((ei > 0) | ((ei == 0) & _owns_tie(u[a], v[a], u[b], v[b])))
        if not inside.any():
            continue
        area = float(e[0][0, 0] + e[1][0, 0] + e[2][0, 0])
        lam = [ei.astype(np.float64) / area for ei in e]
        invz = lam[0] / Z[p, 0] + lam[1] / Z[p, 1] + lam[2] / Z[p, 2]
        with np.errstate(all='ignore'):
            z = np.where(inside, 1.0 / invz, np.inf)
            seg = np.where(inside, z * (lam[0] * L[p, 0] / Z[p, 0] + lam[1] * L[p, 1] / Z[p, 1] + lam[2] * L[p, 2] / Z[p, 2]), 0.0)
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        c1, c2, ct, cs = d1[sl], d2[sl], t1[sl], s1[sl]
        first = inside & ((z < c1) | ((z == c1) & (T[p] < ct)))
        second = inside & ~first & (z < c2)
        c2[first] = c1[first]
        c2[second] = z[second]
        c1[first], ct[first], cs[first] = z[first], T[p], seg[first]
    hit = t1 >= 0
    with np.errstate(all='ignore'):
        clear = ~np.isfinite(d2) | ((d2 - d1) > 1e-4 * d1)
    return {'hit': hit, 'tri': t1, 'depth': np.where(hit, d1, 0.0), 'seg': s1, 'depth2': d2, 'clear': clear | ~hit}


def render_views(verts, faces, labels, cam_ext, cam_int, size, near=0.05):
    """``render_ref`` for every view of cam_ext [n,4,4] (camera-to-world); cam_int [3,3] or [n,3,3]; size = (H, W).  Stacked [n,H,W] arrays
    plus 'dropped' [n] and 'max_coord' (the largest |snapped coordinate| drawn)."""
    H, W = size
    w2c = world_to_camera_rows(cam_ext)
    K = np.asarray(cam_int, np.float64)
    K = np.broadcast_to(K, (len(w2c), 3, 3)) if K.ndim == 2 else K
    out, dropped, mx = [], [], 0
    for i in range(len(w2c)):
        pc = setup_pieces(verts, faces, labels, w2c[i], np.array([K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]], F), near)
        dropped.append(pc['dropped'])
        if len(pc['tri']):
            mx = max(mx, int(np.abs(pc['U']).max()), int(np.abs(pc['V']).max()))
        out.append(render_ref(pc, W, H))
    res = {k: np.stack([o[k] for o in out]) for k in out[0]}
    res['dropped'] = np.array(dropped)
    res['max_coord'] = mx
    return res


def raycast_fp64(verts, faces, cam_ext, cam_int, size, near=0.05, offset=(0.0, 0.0)):
    """Brute force: the ray through every pixel centre (px + 0.5, py + 0.5) (+ ``offset`` pixels) against every triangle, in fp64, in the
    camera frame of the fp32-rounded world-to-camera matrix.  Returns per view tri [H,W] (-1), depth (nearest hit's z, inf), depth2
    (second nearest, inf)."""
    H, W = size
    w2c = world_to_camera_rows(cam_ext).astype(np.float64)
    K = np.asarray(cam_int, np.float64)
    K = np.broadcast_to(K, (len(w2c), 3, 3)) if K.ndim == 2 else K
    faces = np.asarray(faces, np.int64)
    res = {'tri': [], 'depth': [], 'depth2': []}
    for i in range(len(w2c)):
        cam = np.asarray(verts, np.float64) @ w2c[i, :, :3].T + w2c[i, :, 3]
        a, b, c = cam[faces[:, 0]], cam[faces[:, 1]], cam[faces[:, 2]]
        px, py = np.meshgrid(np.arange(W) + 0.5 + offset[0], np.arange(H) + 0.5 + offset[1])
        d = np.stack([(px - K[i, 0, 2]) / K[i, 0, 0], (py - K[i, 1, 2]) / K[i, 1, 1], np.ones_like(px)], -1).reshape(-1, 1, 3)   # [P,1,3]
        e1, e2 = (b - a)[None], (c - a)[None]
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(-1)
        with np.errstate(all='ignore'):
            inv = 1.0 / det
            tv = -a[None]                                                           # the ray starts at the camera centre
            uu = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1)
            vv = (d * qv).sum(-1) * inv
            t = (e2 * qv).sum(-1) * inv                                             # = z of the hit, because d_z = 1
        ok = (det != 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t >= near)
        t = np.where(ok, t, np.inf)
        order = np.argsort(t, axis=1, kind='stable')[:, :2]
        rows = np.arange(t.shape[0])
        dd1 = t[rows, order[:, 0]]
        dd2 = t[rows, order[:, 1]] if t.shape[1] > 1 else np.full_like(dd1, np.inf)
        res['tri'].append(np.where(np.isfinite(dd1), order[:, 0], -1).reshape(H, W))
        res['depth'].append(dd1.reshape(H, W))
        res['depth2'].append(dd2.reshape(H, W))
    return {k: np.stack(v) for k, v in res.items()}


def triangle_soup(seed, n, reach, z_lo, z_hi, cam_int, size):
    """n loose triangles in front of an identity camera, from RandomState(seed): centres uniform over the image of size = (H, W), every
    vertex offset by uniform +-reach pixels in u and in v, at its own depth uniform in z_lo .. z_hi.  Returns verts [3n,3] fp32 (the points
    that project to those pixel coordinates at those depths), faces [n,3] int32 = (3i, 3i+1, 3i+2), labels [3n] fp32 in 0 .. 41 and the
    number of (tile, triangle) pairs of the triangles' pixel boxes, clipped to the image: a box estimate of the bin entries of either
    rasteriser (16-pixel tiles).  Large triangles in a small image put more entries into the bins than their workspace
    holds: 2 n for the piece slots + 64 per tile."""
    (H, W), K, rs = size, np.asarray(cam_int, np.float64), np.random.RandomState(seed)
    c = np.stack([rs.uniform(0, W, (n, 1)), rs.uniform(0, H, (n, 1))], -1) + rs.uniform(-reach, reach, (n, 3, 2))
    z = rs.uniform(z_lo, z_hi, (n, 3))
    verts = np.stack([(c[..., 0] - K[0, 2]) * z / K[0, 0], (c[..., 1] - K[1, 2]) * z / K[1, 1], z], -1).reshape(-1, 3).astype(F)
    labels = rs.randint(0, 42, 3 * n).astype(F)
    lo, hi = np.floor(c.min(1)), np.ceil(c.max(1))
    seen = (c[..., 0].max(1) >= 0) & (c[..., 0].min(1) < W) & (c[..., 1].max(1) >= 0) & (c[..., 1].min(1) < H)
    tx = np.clip(hi[:, 0], 0, W - 1) // 16 - np.clip(lo[:, 0], 0, W - 1) // 16 + 1
    ty = np.clip(hi[:, 1], 0, H - 1) // 16 - np.clip(lo[:, 1], 0, H - 1) // 16 + 1
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3), labels, int((tx * ty * seen).sum())
