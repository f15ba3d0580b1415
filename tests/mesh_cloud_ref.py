"""NumPy restatement of the surface cloud's rule (include/psi_hip.h "scene contact cloud"): every operation in
fp32 and rounded where csrc/mesh_cloud_shared.h rounds it, so that the kernels and the host-check program can be compared bit for bit.
NumPy's fp32 +, -, *, / and sqrt are the IEEE operations, never contracted."""
import numpy as np

F = np.float32
MAX_SEGMENTS = F(2 ** 23)
MAX_CELLS = 1 << 21
MAX_CANDIDATES = 2 ** 31 - 1
EMPTY, CORNERS, ROWS = 0, 1, 2


def sq3(x, y, z):
    return (x * x + y * y) + z * z


def tri_setup(p0, p1, p2, h):
    """(kind, a, b, c, L, m) of one triangle; corners fp32 [3]."""
    e01, e12, e20 = sq3(*(p1 - p0)), sq3(*(p2 - p1)), sq3(*(p0 - p2))
    a, b, c, e = p0, p1, p2, e01
    if e12 > e:
        a, b, c, e = p1, p2, p0, e12
    if e20 > e:
        a, b, c, e = p2, p0, p1, e20
    L = np.sqrt(e)
    u, v = b - a, c - a
    n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    area2 = np.sqrt(sq3(*n))
    if not (area2 > 0) or not (L > 0):
        return EMPTY, a, b, c, L, 0
    if L < h:
        return CORNERS, p0, p1, p2, L, 0
    if not (L / h <= MAX_SEGMENTS):
        raise ValueError('an edge spans more than 2^21 cells')
    Ht = area2 / L
    return ROWS, a, b, c, L, max(1, int(np.ceil(Ht / h)))


def tri_candidates(p0, p1, p2, h):
    """The candidates of one triangle, [n,3] fp32, in candidate order, and its row count."""
    kind, a, b, c, L, m = tri_setup(p0, p1, p2, h)
    if kind == EMPTY:
        return np.zeros((0, 3), F), 0
    if kind == CORNERS:
        return np.stack([a, b, c]).astype(F), 1
    s = np.arange(m, dtype=F) / F(m)
    k = np.maximum(np.ceil(((F(1) - s) * L) / h).astype(np.int64), 1)
    P = a[None] + s[:, None] * (c - a)[None]
    Q = b[None] + s[:, None] * (c - b)[None]
    row = np.repeat(np.arange(m), k + 1)
    start = np.cumsum(k + 1) - (k + 1)
    j = np.arange(len(row)) - start[row]
    u = j.astype(F) / k[row].astype(F)
    pts = P[row] + u[:, None] * (Q[row] - P[row])
    assert pts.dtype == F
    return np.concatenate([pts, c[None]]), m + 1


def check(verts, faces, spacing):
    verts = np.ascontiguousarray(verts, F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if not (np.isfinite(spacing) and spacing > 0 and F(spacing) * F(0.5) > 0):
        raise ValueError('spacing must be positive and finite')
    if len(faces) < 1 or len(verts) < 1:
        raise ValueError('nf >= 1 and nv >= 1')
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError('a face index lies outside [0, nv)')
    if not np.isfinite(verts[faces.reshape(-1)]).all():
        raise ValueError('a vertex coordinate of a triangle is not finite')
    return verts, faces


def candidates(verts, faces, spacing):
    """(pos [n,3] fp32, tri [n] int32, rows) over the caller's faces."""
    verts, faces = check(verts, faces, spacing)
    h = F(spacing) * F(0.5)
    pos, tri, rows = [], [], 0
    for t, (i0, i1, i2) in enumerate(faces):
        p, nr = tri_candidates(verts[i0], verts[i1], verts[i2], h)
        rows += nr
        if len(p):
            pos.append(p)
            tri.append(np.full(len(p), t, np.int32))
    if not pos:
        raise ValueError('no triangle with area')
    return np.concatenate(pos), np.concatenate(tri), rows


def origin(verts, faces, spacing):
    """o = (minimum over the referenced vertices) - h, and the cells along every axis."""
    verts, faces = check(verts, faces, spacing)
    v, h = F(spacing), F(spacing) * F(0.5)
    ref = verts[faces.reshape(-1)]
    o = ref.min(0) - h
    cells = np.floor((ref.max(0) - o) / v) + F(1)
    if (cells > F(MAX_CELLS)).any():
        raise ValueError('more than 2^21 cells along an axis')
    return o


def cells_and_keys(pos, o, spacing):
    """(cell [n,3] int64, linear index [n] int64, bits of the squared distance to the cell centre [n] uint32)."""
    v = F(spacing)
    c = np.floor((pos - o[None]) / v)
    cell = np.clip(c, 0, MAX_CELLS - 1).astype(np.int64)
    centre = o[None] + (cell.astype(F) + F(0.5)) * v
    d = pos - centre
    d2 = sq3(d[:, 0], d[:, 1], d[:, 2])
    assert d2.dtype == F
    lin = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    return cell, lin, d2.view(np.uint32)


def surface_cloud(verts, faces, spacing):
    """(points [m,3] fp32, tri [m] int32, kept candidate numbers [m], candidate total)."""
    pos, tri, _ = candidates(verts, faces, spacing)
    if len(pos) > MAX_CANDIDATES:
        raise ValueError('%d candidates at spacing %g' % (len(pos), spacing))
    o = origin(verts, faces, spacing)
    _, lin, key = cells_and_keys(pos, o, spacing)
    order = np.lexsort((np.arange(len(pos)), key, lin))         # by cell, then distance bits, then candidate number
    head = np.ones(len(pos), bool)
    head[1:] = lin[order][1:] != lin[order][:-1]
    kept = np.sort(order[head])
    return pos[kept], tri[kept], kept, len(pos)


def sample_surface(verts, faces, n, seed=0):
    """n area-weighted random surface points (fp64) and their triangles."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    rs = np.random.RandomState(seed)
    t = rs.choice(len(faces), n, p=area / area.sum())
    r1, r2 = np.sqrt(rs.rand(n)), rs.rand(n)
    return (1 - r1)[:, None] * a[t] + (r1 * (1 - r2))[:, None] * b[t] + (r1 * r2)[:, None] * c[t], t


def surface_area(verts, faces):
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())


def covering_radius(samples, cloud):
    """max over the samples of the distance to the nearest cloud point (fp64), with a k-d tree when SciPy is there."""
    cloud = np.asarray(cloud, np.float64)
    try:
        from scipy.spatial import cKDTree
        return float(cKDTree(cloud).query(samples)[0].max())
    except ImportError:
        worst = 0.0
        for i in range(0, len(samples), 1024):
            d = ((samples[i:i + 1024, None, :] - cloud[None]) ** 2).sum(-1).min(1)
            worst = max(worst, float(np.sqrt(d.max())))
        return worst


# ---- the shared inputs of the CPU and GPU tests (cases A .. G of the issue) ----
def case_A():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def case_B():
    return np.array([[0, 0, 0], [3, 0, 0], [1.3, 0.013, 0]], F), np.array([[0, 1, 2]], np.int32)


def case_C():
    e = 0.01
    return np.array([[0.2, 0.3, 0.1], [0.2 + e, 0.3, 0.1], [0.2 + e / 2, 0.3 + e * np.sqrt(3) / 2, 0.1]], F), np.array([[0, 1, 2]], np.int32)


def case_D():
    v, f = case_A()
    return v, np.array([f[0], [1, 1, 2], f[1]], np.int32)


def case_E(seed=5):
    rs = np.random.RandomState(seed)
    v = rs.uniform(-1.0, 1.0, (150, 3)).astype(F)
    return v, np.arange(150, dtype=np.int32).reshape(50, 3), float(rs.uniform(0.03, 0.3))


def write_mesh(path, verts, faces):
    """The MESH.bin of the host-check programs: int32 nv, int32 nf, nv*3 float32, nf*3 int32."""
    with open(path, 'wb') as f:
        f.write(np.array([len(verts), len(faces)], np.int32).tobytes())
        f.write(np.ascontiguousarray(verts, F).tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
