"""NumPy restatement of the rigid separation rule (csrc/body_separate_shared.h), line for line.  The only operations
are + - * / sqrt and comparisons, so the fp32 form gives the bits of the kernels and of the host rehearsal; ``dtype=np.float64`` gives the
form the fp32 results are measured against.

    state     quat (w, x, y, z), transl [3], pivot [3], Adam moments m, s [6] per body
    pose      R of quat (nine entries below), d = base - pivot, p = pivot + transl, x_k = ((R_k0 d0 + R_k1 d1) + R_k2 d2) + p_k;
              a body whose state is exactly the identity gets its base bits
    wrench    a = x - p, c = a x G in fp32; (G, c) widened to fp64, a 256-lane tree per chunk of 256 consecutive vertices, the chunks added in
              order, the six sums rounded once: g6 = (F, T)
    step      Adam on g6, transl -= lr_t u[0:3], delta = -(lr_r u[3:6]), quat <- normalise((1, delta / 2) (x) quat) unless delta == 0

``separate`` is the loop of ops.rigid_separate, composed of the restatements of the searches and of the two gradients."""
import numpy as np

CHUNK = 256


class State:
    def __init__(self, B, pivot, dtype=np.float32):
        self.quat = np.zeros((B, 4), dtype)
        self.quat[:, 0] = 1
        self.transl = np.zeros((B, 3), dtype)
        self.pivot = np.array(pivot, dtype).reshape(B, 3)
        self.m = np.zeros((B, 6), dtype)
        self.s = np.zeros((B, 6), dtype)

    def copy(self):
        o = State.__new__(State)
        for k in ('quat', 'transl', 'pivot', 'm', 's'):
            setattr(o, k, getattr(self, k).copy())
        return o

    def arrays(self):
        return dict(quat=self.quat, transl=self.transl, pivot=self.pivot, m=self.m, s=self.s)


def default_pivot(base):
    """[B,3] fp32: the mean of the base vertices, in fp64, rounded once."""
    return np.asarray(base, np.float64).mean(1).astype(np.float32)


def rotation(quat):
    """R [B,3,3] of quat [B,4] in its dtype: the nine entries with their association."""
    q = np.asarray(quat)
    T = q.dtype.type
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = T(1), T(2)
    R = np.empty((len(q), 3, 3), q.dtype)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - w * z)
    R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y)
    R[:, 2, 1] = two * (y * z + w * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def is_identity(quat, transl):
    """[B] bool: quat == (1, 0, 0, 0) and transl == 0 exactly (a negative zero counts as zero)."""
    q, t = np.asarray(quat), np.asarray(transl)
    return (q[:, 0] == 1) & (q[:, 1] == 0) & (q[:, 2] == 0) & (q[:, 3] == 0) & (t == 0).all(1)


def pose(base, quat, transl, pivot, dtype=np.float32):
    base = np.asarray(base, np.float32).astype(dtype)
    quat, transl, pivot = np.asarray(quat, dtype), np.asarray(transl, dtype), np.asarray(pivot, dtype)
    R = rotation(quat)
    d = base - pivot[:, None, :]
    p = pivot + transl
    out = np.empty_like(base)
    for k in range(3):
        out[:, :, k] = ((R[:, k, 0, None] * d[:, :, 0] + R[:, k, 1, None] * d[:, :, 1]) + R[:, k, 2, None] * d[:, :, 2]) + p[:, k, None]
    same = is_identity(quat, transl)
    out[same] = base[same]
    return out


def wrench_terms(verts, G, p, dtype=np.float32):
    """[B,V,6]: (G, a x G) per vertex with a = x - p, every cross component a*b - c*d."""
    x, G, p = np.asarray(verts, dtype), np.asarray(G, dtype), np.asarray(p, dtype)
    a = x - p[:, None, :]
    c = np.stack([a[..., 1] * G[..., 2] - a[..., 2] * G[..., 1], a[..., 2] * G[..., 0] - a[..., 0] * G[..., 2],
                  a[..., 0] * G[..., 1] - a[..., 1] * G[..., 0]], -1)
    return np.concatenate([G, c], -1)


def chunk_sums(terms):
    """[B,nchunk,6] fp64 of terms [B,V,6]: s[l] += s[l + stride], stride = 128 .. 1, lanes past V hold +0."""
    B, V = terms.shape[:2]
    nchunk = (V + CHUNK - 1) // CHUNK
    s = np.zeros((B, nchunk * CHUNK, 6), np.float64)
    s[:, :V] = terms
    s = s.reshape(B, nchunk, CHUNK, 6)
    stride = CHUNK // 2
    while stride >= 1:
        s[:, :, :stride] = s[:, :, :stride] + s[:, :, stride:2 * stride]
        stride //= 2
    return np.ascontiguousarray(s[:, :, 0])


def g6_of(chunks, dtype=np.float32):
    """[B,6]: the chunks added in chunk order in fp64 from +0, rounded once."""
    acc = np.zeros((chunks.shape[0], 6), np.float64)
    for c in range(chunks.shape[1]):
        acc = acc + chunks[:, c]
    return acc.astype(dtype)


def wrench(verts, G, p, dtype=np.float32):
    return g6_of(chunk_sums(wrench_terms(verts, G, p, dtype)), dtype)


def bias_corrections(k, betas):
    """c1 = fp32(1 - b1^k), c2 = fp32(1 - b2^k), in fp64 on the host."""
    return np.float32(1.0 - float(betas[0]) ** int(k)), np.float32(1.0 - float(betas[1]) ** int(k))


def quat_step(quat, delta):
    """normalise((1, delta / 2) (x) quat) per row; a row whose delta is exactly zero is kept as it is."""
    q = np.asarray(quat)
    T = q.dtype.type
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    hx, hy, hz = delta[:, 0] / T(2), delta[:, 1] / T(2), delta[:, 2] / T(2)
    nw = ((w - hx * x) - hy * y) - hz * z
    nx = ((x + hx * w) + hy * z) - hz * y
    ny = ((y - hx * z) + hy * w) + hz * x
    nz = ((z + hx * y) - hy * x) + hz * w
    n2 = ((nw * nw + nx * nx) + ny * ny) + nz * nz
    n = np.sqrt(n2)
    out = np.stack([nw / n, nx / n, ny / n, nz / n], 1)
    keep = (delta == 0).all(1)
    out[keep] = q[keep]
    return out


def step(state, g6, k, lr_t=0.01, lr_r=0.01, betas=(0.9, 0.999), eps=1e-8, fixed=None):
    """The state after step k = 1, 2, ... (a new State; ``fixed``: [B] bool or a list of bodies)."""
    T = state.quat.dtype.type
    B = len(state.quat)
    g = np.array(g6, state.quat.dtype).reshape(B, 6)
    if fixed is not None:
        f = np.asarray(fixed)
        g[f if f.dtype == bool else np.isin(np.arange(B), f)] = 0
    b1, b2, eps, lr_t, lr_r = T(betas[0]), T(betas[1]), T(eps), T(lr_t), T(lr_r)
    c1, c2 = bias_corrections(k, betas)
    c1, c2 = T(c1), T(c2)
    out = state.copy()
    out.m = b1 * state.m + (T(1) - b1) * g
    out.s = b2 * state.s + ((T(1) - b2) * g) * g
    u = (out.m / c1) / (np.sqrt(out.s / c2) + eps)
    out.transl = state.transl - lr_t * u[:, 0:3]
    delta = -(lr_r * u[:, 3:6])
    out.quat = quat_step(state.quat, delta)
    return out


def transform(quat, transl, pivot):
    """M [B,4,4] fp64 with x' = M x for the base vertices: the same nine entries in fp64, t = (pivot + transl) - R pivot."""
    q, t, c = np.asarray(quat, np.float64), np.asarray(transl, np.float64), np.asarray(pivot, np.float64)
    R = rotation(q)
    M = np.zeros((len(q), 4, 4))
    M[:, :3, :3] = R
    M[:, :3, 3] = (c + t) - np.einsum('bkl,bl->bk', R, c)
    M[:, 3, 3] = 1
    return M


def shift_angle(quat, transl):
    q, t = np.asarray(quat, np.float64), np.asarray(transl, np.float64)
    return np.sqrt((t * t).sum(1)), 2.0 * np.arctan2(np.sqrt((q[:, 1:] ** 2).sum(1)), np.abs(q[:, 0]))


class Iteration:
    """What one pass of the loop saw: the state it posed, the searches' lists, G, the chunk sums and g6."""


def search(verts, faces, group=None, w_pen=1.0, w_cross=1.0, penalty='depth', sigma=0.5):
    """One pass of the searches and the gradients on ``verts`` [B,V,3] fp32 -> Iteration (triples, w of the candidates, pairs, both losses,
    G or None when the stop test holds)."""
    import body_depth_ref as DR
    import body_overlap_ref as BR
    import crossing_field_ref as FR
    import surface_crossings_ref as SR
    B, V = verts.shape[:2]
    it = Iteration()
    it.verts = verts
    it.triples, it.pairs, it.cand_w = np.zeros((0, 3), np.int32), np.zeros((0, 4), np.int32), np.zeros(0)
    it.loss_pen, it.loss_cross = np.zeros(B, np.float32), np.zeros(B, np.float32)
    G = []
    if w_pen != 0:
        _, _, cand, w = BR.overlap(verts, faces, group)
        it.cand_w = w
        it.triples = np.ascontiguousarray(cand[w > 0.5])
        if len(it.triples):
            rows = DR.nearest(verts, faces, it.triples)
            it.loss_pen = DR.aggregates(it.triples, rows['depth'], B, V)[4][DR.PENALTIES[penalty]]
            G.append(DR.gradient(it.triples, rows, faces, np.full(B, w_pen, np.float32), penalty, B, V))
        else:
            G.append(np.zeros((B, V, 3), np.float32))
    if w_cross != 0:
        r = SR.crossings(verts, faces, group=group, self_pairs=False, between=True)
        it.pairs = r.pairs
        if len(it.pairs):
            _, energy = FR.field(verts, faces, it.pairs, sigma)
            it.loss_cross = FR.aggregates(it.pairs, energy, B)[1]
            G.append(FR.grad(verts, faces, it.pairs, sigma, np.full(B, w_cross, np.float32))[2])
        else:
            G.append(np.zeros((B, V, 3), np.float32))
    it.clean = len(it.triples) == 0 and len(it.pairs) == 0
    it.G = None if it.clean else (G[0] if len(G) == 1 else G[0] + G[1])
    return it


def separate(base, faces, group=None, fixed=None, pivot=None, max_iter=100, lr_t=0.01, lr_r=0.01, betas=(0.9, 0.999), eps=1e-8, w_pen=1.0,
             w_cross=1.0, penalty='depth', sigma=0.5):
    """The loop of ops.rigid_separate in the fp32 restatement.  Returns (state, verts, iterations, separated, trace): ``trace`` holds one
    Iteration per pass, ``trace[k].state`` the state that pass posed."""
    base = np.asarray(base, np.float32)
    state = State(len(base), default_pivot(base) if pivot is None else pivot)
    trace = []
    k = 0
    while True:
        verts = pose(base, state.quat, state.transl, state.pivot)
        it = search(verts, faces, group, w_pen, w_cross, penalty, sigma)
        it.state = state
        trace.append(it)
        if it.clean or k == max_iter:
            return state, verts, k, it.clean, trace
        it.chunks = chunk_sums(wrench_terms(verts, it.G, state.pivot + state.transl))
        it.g6 = g6_of(it.chunks)
        k += 1
        state = step(state, it.g6, k, lr_t, lr_r, betas, eps, fixed)
