"""NumPy restatement of the conic distance field of a triangle pair (csrc/crossing_field_shared.h, which this file
mirrors line for line: the same operations in the same association, vectorised over the (pair, role) entries).

    record      of the receiver (a, b, c):  e1 = b - a, e2 = c - a, N = e1 x e2, N2 = N.N, len = sqrt(N2), n = N / len,
                m = (e1.e1) (e2 x N) + (e2.e2) (N x e1), den = 2 N2, q = m / den, o = a + q, r = sqrt(q.q)
    evaluation  of p:  w = p - o, h = n.w, t = w - h n, rho = sqrt(t.t);  gate 1: h < sigma;  D = r (1 - h / sigma), Phi = rho / D;
                gate 2: Phi < 1;  Y = (1 - h) - sigma for h <= -sigma, else (c0 - c1 h) - (c2 h) h;  Psi = (1 - Phi) Y
    role 0      the corners of face s of body i in the record of face t of body j;  role 1 the other way round
    energy      (Psi0^2 + Psi1^2) + Psi2^2

With ``dtype=np.float32`` every function is the restatement of the kernels (NumPy's elementwise float32 operations round once each and
never contract; division and square root are IEEE); with ``np.float64`` it is the same rule in double, the fp64 form of the tests."""
import numpy as np


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _scale(s, a):
    return s[..., None] * a


def _over(a, s):
    return a / s[..., None]


class Consts:
    def __init__(self, sigma, dtype=np.float32):
        T = np.dtype(dtype).type
        self.sigma = T(sigma)
        s2 = T(2) * self.sigma
        self.c2 = (T(1) - s2) / (s2 * s2)
        self.c1 = T(1) / s2
        self.c0 = (T(3) - s2) / T(4)
        self.T = T


class Record:
    """cf_record: a, b, c [m,3]"""

    def __init__(self, a, b, c):
        T = a.dtype.type
        self.a = a
        self.e1 = b - a
        self.e2 = c - a
        self.N = _cross(self.e1, self.e2)
        self.N2 = _dot(self.N, self.N)
        self.len = np.sqrt(self.N2)
        self.n = _over(self.N, self.len)
        self.d1 = _dot(self.e1, self.e1)
        self.d2 = _dot(self.e2, self.e2)
        self.u = _cross(self.e2, self.N)
        self.v = _cross(self.N, self.e1)
        m = _scale(self.d1, self.u) + _scale(self.d2, self.v)
        self.den = T(2) * self.N2
        self.q = _over(m, self.den)
        self.o = a + self.q
        self.r = np.sqrt(_dot(self.q, self.q))


class Eval:
    """cf_eval: p [m,3] in the records R"""

    def __init__(self, R, K, p):
        T = K.T
        self.w = p - R.o
        self.h = _dot(R.n, self.w)
        self.t = self.w - _scale(self.h, R.n)
        self.rho = np.sqrt(_dot(self.t, self.t))
        self.k1 = T(1) - self.h / K.sigma
        self.D = R.r * self.k1
        self.Phi = self.rho / self.D
        self.low = self.h <= -K.sigma
        self.Y = np.where(self.low, (T(1) - self.h) - K.sigma, (K.c0 - K.c1 * self.h) - (K.c2 * self.h) * self.h)
        self.active = (self.h < K.sigma) & (self.Phi < T(1))
        self.psi = np.where(self.active, (T(1) - self.Phi) * self.Y, T(0))


def _eval_reverse(R, K, E, g2, A):
    """cf_eval_reverse: the row of p; adds to the adjoints A = [n_bar, o_bar, r_bar]"""
    T = K.T
    psi_b = g2 * E.psi
    Phi_b = -(psi_b * E.Y)
    Y_b = psi_b * (T(1) - E.Phi)
    dY = np.where(E.low, T(-1), -K.c1 - (T(2) * K.c2) * E.h)
    rho_b = Phi_b / E.D
    D_b = -(Phi_b * E.Phi) / E.D
    r_b = D_b * E.k1
    k1_b = D_b * R.r
    h_b = Y_b * dY - k1_b / K.sigma
    t_b = np.where((E.rho > T(0))[:, None], _scale(rho_b / E.rho, E.t), T(0))
    w_b = t_b + _scale(h_b, R.n)
    n_b = _scale(h_b, E.w) - _scale(E.h, t_b)
    act = E.active
    A[0] = np.where(act[:, None], A[0] + n_b, A[0])
    A[1] = np.where(act[:, None], A[1] - w_b, A[1])
    A[2] = np.where(act, A[2] + r_b, A[2])
    return np.where(act[:, None], w_b, T(0))


def _record_reverse(R, A):
    """cf_record_reverse: the rows of a, b, c"""
    T = R.a.dtype.type
    An, Ao, Ar = A
    q_b = np.where((R.r > T(0))[:, None], Ao + _scale(Ar / R.r, R.q), Ao)
    m_b = _over(q_b, R.den)
    den_b = -_dot(q_b, R.q) / R.den
    N2_b = T(2) * den_b
    d1_b, d2_b = _dot(m_b, R.u), _dot(m_b, R.v)
    u_b, v_b = _scale(R.d1, m_b), _scale(R.d2, m_b)
    e1_b = _cross(v_b, R.N) + _scale(T(2) * d1_b, R.e1)
    e2_b = _cross(R.N, u_b) + _scale(T(2) * d2_b, R.e2)
    N_b = _cross(u_b, R.e2) + _cross(R.e1, v_b)
    N_b = N_b + _over(An - _scale(_dot(R.n, An), R.n), R.len)
    N_b = N_b + _scale(T(2) * N2_b, R.N)
    e1_b = e1_b + _cross(R.e2, N_b)
    e2_b = e2_b + _cross(N_b, R.e1)
    return (Ao - e1_b) - e2_b, e1_b, e2_b


def pair_role(P, Q, sigma, g=None, dtype=np.float32):
    """cf_pair_role for m entries: P [m,k,3] the evaluated points (k = 3 corners of the intruder; any k for the tests of one evaluation),
    Q [m,3,3] the receiver.  Returns psi [m,k] and, with ``g`` [m] (the upstream of sum_k Psi_k^2), also rows [m,k+3,3]: the points, then
    a, b, c."""
    P, Q = np.asarray(P, dtype), np.asarray(Q, dtype)
    K = Consts(sigma, dtype)
    T = K.T
    with np.errstate(all='ignore'):
        R = Record(Q[:, 0], Q[:, 1], Q[:, 2])
        E = [Eval(R, K, P[:, k]) for k in range(P.shape[1])]
        psi = np.stack([e.psi for e in E], 1)
        if g is None:
            return psi
        g2 = T(2) * np.asarray(g, dtype)
        m = len(P)
        A = [np.zeros((m, 3), dtype), np.zeros((m, 3), dtype), np.zeros(m, dtype)]
        rows = [_eval_reverse(R, K, e, g2, A) for e in E]
        anyact = np.stack([e.active for e in E], 1).any(1)
        ga, gb, gc = _record_reverse(R, A)
        rows += [np.where(anyact[:, None], x, T(0)) for x in (ga, gb, gc)]
    return psi, np.stack(rows, 1)


def energy_of(psi):
    """[..,3] -> [..]: (Psi0^2 + Psi1^2) + Psi2^2"""
    return (psi[..., 0] * psi[..., 0] + psi[..., 1] * psi[..., 1]) + psi[..., 2] * psi[..., 2]


def entries(verts, faces, pairs):
    """P, Q [2n,3,3] fp32 of the entries e = 2 k + role, and their vertex targets [2n,6] int64 (body V + vertex: intruder, receiver)."""
    verts, faces, pairs = np.asarray(verts, np.float32), np.asarray(faces, np.int64), np.asarray(pairs, np.int64).reshape(-1, 4)
    V = verts.shape[1]
    bi = np.stack([pairs[:, 0], pairs[:, 2]], 1).reshape(-1)
    fi = np.stack([pairs[:, 1], pairs[:, 3]], 1).reshape(-1)
    br = np.stack([pairs[:, 2], pairs[:, 0]], 1).reshape(-1)
    fr = np.stack([pairs[:, 3], pairs[:, 1]], 1).reshape(-1)
    P, Q = verts[bi[:, None], faces[fi]], verts[br[:, None], faces[fr]]
    targets = np.concatenate([bi[:, None] * V + faces[fi], br[:, None] * V + faces[fr]], 1)
    return P, Q, targets


def field(verts, faces, pairs, sigma, dtype=np.float32):
    """psi [n,2,3], energy [n,2] of ``dtype``."""
    P, Q, _ = entries(verts, faces, pairs)
    psi = pair_role(P, Q, sigma, dtype=dtype).reshape(-1, 2, 3)
    return psi, energy_of(psi)


def aggregates(pairs, energy, B):
    """pair_energy [B,B] fp64 and loss [B] fp32: the entries of a cell one after the other in pair order; loss in j order."""
    E = np.zeros((B, B), np.float64)
    for (i, _, j, _), (e0, e1) in zip(np.asarray(pairs).reshape(-1, 4).tolist(), np.asarray(energy).reshape(-1, 2)):
        if i != j:
            E[i, j] = E[i, j] + np.float64(e0)
            E[j, i] = E[j, i] + np.float64(e1)
        else:
            E[i, i] = E[i, i] + (np.float64(e0) + np.float64(e1))
    loss = np.zeros(B, np.float32)
    for i in range(B):
        total = np.float64(0.0)
        for j in range(B):
            total = total + E[i, j]
        loss[i] = np.float32(total)
    return E, loss


def segment_sum(targets, rows, n_out):
    """out [n_out,3] fp32: the rows sorted stably by target, every run added in order in fp32 (psi_segment_sum3)."""
    targets, rows = np.asarray(targets).reshape(-1), np.asarray(rows, np.float32).reshape(-1, 3)
    order = np.argsort(targets, kind='stable')
    out = np.zeros((n_out, 3), np.float32)
    seen = np.zeros(n_out, bool)
    for q in order:
        t = targets[q]
        if not seen[t]:
            seen[t] = True
            out[t] = np.float32(0.0) + rows[q]
        else:
            out[t] = out[t] + rows[q]
    return out


def grad(verts, faces, pairs, sigma, g, dtype=np.float32):
    """rows [2n,6,3], targets [2n,6] and G [B,V,3] (fp32 form only) of sum_i g[i] loss[i]: role 0 scaled by g[i], role 1 by g[j]."""
    verts = np.asarray(verts, np.float32)
    B, V = verts.shape[:2]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 4)
    P, Q, targets = entries(verts, faces, pairs)
    ge = np.asarray(g, dtype)[np.stack([pairs[:, 0], pairs[:, 2]], 1).reshape(-1)]
    _, rows = pair_role(P, Q, sigma, g=ge, dtype=dtype)
    G = segment_sum(targets, rows, B * V).reshape(B, V, 3) if np.dtype(dtype) == np.float32 else None
    return rows, targets, G
