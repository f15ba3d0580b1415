"""NumPy restatement of the scene term of the rigid separation (the scene statements of
csrc/body_separate_shared.h), line for line, and of the loop of ops.rigid_separate with a scene.  It stands beside
tests/body_separate_ref.py, whose pose, wrench, tree and step it uses unchanged.

    table     sdf [S,D,D,D] fp32 (element [ix][iy][iz]), gmin, gmax [S,3] fp32, scene_id [B] or None (scene 0; clamped to [0, S))
    coords    sdf_lookup_ref.cells_coords with align_corners: k = fp32((D - 1) / (max - min)) from fp64, o = min, u = (x - o) k, the
              median-of-three clamp, cell, fraction, in = 0 < u < D - 1; the upper corner is min(i + 1, D - 1)
    interp    fp32, lerp(a, b, w) = a + w (b - a): dz = q..1 - q..0, r[dx][dy] = q..0 + wz dz, r[dx] = lerp(r[dx][0], r[dx][1], wy),
              value = lerp(r[0], r[1], wx); gx = r[1] - r[0], gy = lerp(r[0][1] - r[0][0], r[1][1] - r[1][0], wx),
              gz = lerp(lerp(dz00, dz01, wy), lerp(dz10, dz11, wy), wx); g_a = in_a ? grid_a k_a : 0
    term      value < 0: G = (-w_scene) g, loss -value; every other vertex exact zeros
    wrench    a = x - p, c = a x G in fp32 for the vertices in the scene, +0 for the others; the 256-lane tree per chunk in fp64 for the
              six terms and for -value; the count per chunk"""
import numpy as np

import body_separate_ref as R
import sdf_lookup_ref as LR


def lerp(a, b, w):
    return a + w * (b - a)


def lookup(vol, gmin, gmax, pts):
    """value [N] fp32, g [N,3] fp32 (world gradient under the strict mask), inside-the-box mask [N,3] of one volume [D,D,D] at pts [N,3]."""
    vol = np.asarray(vol, np.float32)
    D = vol.shape[0]
    co = LR.cells_coords(gmin, gmax, D, True, pts)
    k = LR.cells_constants(gmin, gmax, D, True)[0]
    i0 = co['cell']
    i1 = np.minimum(i0 + 1, D - 1)
    wx, wy, wz = co['w'][:, 0], co['w'][:, 1], co['w'][:, 2]
    ix, iy, iz = (i0[:, 0], i1[:, 0]), (i0[:, 1], i1[:, 1]), (i0[:, 2], i1[:, 2])
    dz, r = [[None, None], [None, None]], [[None, None], [None, None]]
    for dx in (0, 1):
        for dy in (0, 1):
            q0, q1 = vol[ix[dx], iy[dy], iz[0]], vol[ix[dx], iy[dy], iz[1]]
            dz[dx][dy] = q1 - q0
            r[dx][dy] = q0 + wz * dz[dx][dy]
    r0, r1 = lerp(r[0][0], r[0][1], wy), lerp(r[1][0], r[1][1], wy)
    value = lerp(r0, r1, wx)
    gx = r1 - r0
    gy = lerp(r[0][1] - r[0][0], r[1][1] - r[1][0], wx)
    gz = lerp(lerp(dz[0][0], dz[0][1], wy), lerp(dz[1][0], dz[1][1], wy), wx)
    zero = np.float32(0)
    g = np.stack([np.where(co['inside'][:, 0], gx * k[0], zero), np.where(co['inside'][:, 1], gy * k[1], zero),
                  np.where(co['inside'][:, 2], gz * k[2], zero)], 1)
    assert value.dtype == np.float32 and g.dtype == np.float32
    return value, g, co['inside']


def scene_of(scene_id, B, S):
    if scene_id is None:
        return np.zeros(B, np.int64)
    return np.clip(np.asarray(scene_id, np.int64), 0, S - 1)


def term(verts, sdf, gmin, gmax, scene_id=None, w_scene=1.0):
    """value [B,V] fp32, G [B,V,3] fp32, in_scene [B,V] bool."""
    verts = np.asarray(verts, np.float32)
    sdf = np.asarray(sdf, np.float32)
    sdf = sdf[None] if sdf.ndim == 3 else sdf
    gmin, gmax = np.asarray(gmin, np.float32).reshape(-1, 3), np.asarray(gmax, np.float32).reshape(-1, 3)
    B, V = verts.shape[:2]
    sc = scene_of(scene_id, B, sdf.shape[0])
    value, G = np.empty((B, V), np.float32), np.empty((B, V, 3), np.float32)
    nw = -np.float32(w_scene)
    for b in range(B):
        value[b], g, _ = lookup(sdf[sc[b]], gmin[sc[b]], gmax[sc[b]], verts[b])
        G[b] = nw * g
    inside = value < np.float32(0)
    G[~inside] = 0
    return value, G, inside


class SceneWrench:
    """chunks [B,nchunk,6] fp64, count_chunks [B,nchunk] int32, loss_chunks [B,nchunk] fp64, count [B] int64, loss [B] fp64, value, G"""


def ordered(chunks):
    """[B, ...]: the chunk rows [B,nchunk,...] added in chunk order from +0."""
    acc = np.zeros(chunks.shape[:1] + chunks.shape[2:], chunks.dtype)
    for c in range(chunks.shape[1]):
        acc = acc + chunks[:, c]
    return acc


def wrench(verts, p, sdf, gmin, gmax, scene_id=None, w_scene=1.0):
    out = SceneWrench()
    out.value, out.G, inside = term(verts, sdf, gmin, gmax, scene_id, w_scene)
    terms = R.wrench_terms(verts, out.G, p).astype(np.float64)
    terms[~inside] = 0.0                                                    # a lane outside the scene holds +0, not a signed product of zeros
    out.chunks = R.chunk_sums(terms)
    out.loss_chunks = R.chunk_sums(np.where(inside, (-out.value).astype(np.float64), 0.0)[..., None])[..., 0]
    B, V = inside.shape
    nchunk = out.chunks.shape[1]
    pad = np.zeros((B, nchunk * R.CHUNK), np.int32)
    pad[:, :V] = inside
    out.count_chunks = pad.reshape(B, nchunk, R.CHUNK).sum(2).astype(np.int32)
    out.count = out.count_chunks.astype(np.int64).sum(1)
    out.loss = ordered(out.loss_chunks)
    return out


def separate(base, faces, scene=None, w_scene=1.0, group=None, fixed=None, pivot=None, max_iter=100, lr_t=0.01, lr_r=0.01, betas=(0.9, 0.999),
             eps=1e-8, w_pen=1.0, w_cross=1.0, penalty='depth', sigma=0.5):
    """The loop of ops.rigid_separate in the fp32 restatement, ``scene`` = (sdf, gmin, gmax, scene_id) or None.  Returns (state, verts,
    iterations, separated, trace); an Iteration of the trace also holds ``scene`` (a SceneWrench or None) and ``stop``."""
    base = np.asarray(base, np.float32)
    B = len(base)
    state = R.State(B, R.default_pivot(base) if pivot is None else pivot)
    free = np.ones(B, bool)
    if fixed is not None:
        f = np.asarray(fixed)
        free = ~(f if f.dtype == bool else np.isin(np.arange(B), f))
    trace = []
    k = 0
    while True:
        verts = R.pose(base, state.quat, state.transl, state.pivot)
        p = state.pivot + state.transl
        sc = None if scene is None else wrench(verts, p, scene[0], scene[1], scene[2], scene[3], w_scene)
        it = R.search(verts, faces, group, w_pen, w_cross, penalty, sigma)
        it.state, it.scene = state, sc
        it.stop = it.clean and (sc is None or sc.count[free].sum() == 0)
        trace.append(it)
        if it.stop or k == max_iter:
            return state, verts, k, it.stop, trace
        if sc is None:
            it.chunks = R.chunk_sums(R.wrench_terms(verts, it.G, p))
        else:
            body = np.zeros_like(sc.chunks) if it.clean else R.chunk_sums(R.wrench_terms(verts, it.G, p))
            it.chunks = body + sc.chunks
        it.g6 = R.g6_of(it.chunks)
        k += 1
        state = R.step(state, it.g6, k, lr_t, lr_r, betas, eps, fixed)
