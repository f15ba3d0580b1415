"""NumPy restatement of DESIGN.md section 12 (psi_snapshot_canvas), statement by statement in fp32 with the window sum in fp64, and of the
reframe formulas of training_data.reframe_bodies in a chosen precision.  The tests compare the kernel and the host code against these."""
import numpy as np

F = np.float32
CLIP_DEPTH, CLIP_SEG = 6.0, 41.0


def clipped_max(img, clip):
    """(c, max, has_nan): c = min(x, clip) in fp32; the maximum of c over the pixels that are not NaN (0 when there is none)."""
    img = np.asarray(img, F)
    nan = np.isnan(img)
    c = np.where(img < F(clip), img, F(clip)).astype(F)
    vals = c[~nan]
    mx = F(max(vals.max(), F(0))) if vals.size else F(0)
    return c, mx, bool(nan.any())


def source_index(n_in, n_out):
    """i0, i1, l0, l1 of F.interpolate(mode='bilinear', align_corners=False) along one axis.  scale (dst + 0.5) - 0.5 is one fused
    multiply-add: the fp64 product of two fp32 numbers is exact, so rounding the fp64 expression once gives the fused result."""
    scale = F(n_in) / F(n_out)
    dst = np.arange(n_out, dtype=F)
    src = np.maximum((np.float64(scale) * (dst + F(0.5)).astype(np.float64) - 0.5).astype(F), F(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(F)).astype(F)
    return i0, i1, (F(1) - l1).astype(F), l1


def placement(H, W, th, tw):
    """(oh, ow, y0, x0): size of the resized image and its first canvas row / column (batch_gen_hdf5.py:398-439)."""
    if H >= W:
        ow = int(W * (float(th) / H)) // 2 * 2
        return th, ow, 0, tw // 2 - ow // 2
    oh = int((float(tw) / W) * H) // 2 * 2
    return oh, tw, th // 2 - oh // 2, 0


def canvas_of(c, mx, size=(128, 128)):
    """The canvas [th,tw] fp32 of one clipped image c [H,W] with maximum mx > 0."""
    th, tw = size
    H, W = c.shape
    oh, ow, y0, x0 = placement(H, W, th, tw)
    v = ((F(2) * c) / F(mx) - F(1)).astype(F)
    iy0, iy1, l0y, l1y = source_index(H, oh)
    ix0, ix1, l0x, l1x = source_index(W, ow)
    a, b = v[iy0][:, ix0], v[iy0][:, ix1]
    cc, d = v[iy1][:, ix0], v[iy1][:, ix1]
    top = (l0x[None] * a).astype(F) + (l1x[None] * b).astype(F)
    bot = (l0x[None] * cc).astype(F) + (l1x[None] * d).astype(F)
    out = (l0y[:, None] * top.astype(F)).astype(F) + (l1y[:, None] * bot.astype(F)).astype(F)
    canvas = np.zeros((th, tw), F)
    canvas[y0:y0 + oh, x0:x0 + ow] = out.astype(F)
    return canvas


def window_mean(depth, window):
    """Mean of the UNCLIPPED depth over [x0,x1) x [y0,y1) cut to the image: fp64, summed row-major by one adder.  None: empty window."""
    H, W = depth.shape
    x0, y0, x1, y1 = (int(v) for v in window)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    if x1 <= x0 or y1 <= y0:
        return None
    vals = np.asarray(depth[y0:y1, x0:x1], np.float64).ravel()
    return float(np.cumsum(vals)[-1]) / vals.size        # cumsum adds in order


def snapshot_canvas(depth, seg, size=(128, 128), windows=None, target_z=None):
    """The five outputs of ops.snapshot_canvas as NumPy arrays; the inputs are not written."""
    depth, seg = np.asarray(depth, F), np.asarray(seg, F)
    n = depth.shape[0]
    th, tw = size
    dc, sc = np.zeros((n, 1, th, tw), F), np.zeros((n, 1, th, tw), F)
    max_d, seg_max, usable = np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int32)
    for i in range(n):
        cd, md, nd = clipped_max(depth[i], CLIP_DEPTH)
        cs, ms, ns = clipped_max(seg[i], CLIP_SEG)
        max_d[i], seg_max[i] = md, ms
        if not (md > 0 and ms > 0) or nd or ns:
            continue
        dc[i, 0], sc[i, 0] = canvas_of(cd, md, size), canvas_of(cs, ms, size)
        if windows is None:
            usable[i] = 1
        else:
            m = window_mean(depth[i], windows[i])
            usable[i] = int(m is not None and m > float(F(target_z[i])))
    return dc, sc, max_d, seg_max, usable


K96 = np.array([[80.0, 0, 48.0], [0, 80.0, 32.0], [0, 0, 1.0]])      # the 64 x 96 test camera


def window_views():
    """Depth images [8,64,96] with a near or a far patch planted around a target pixel, and the targets (camera coordinates): inside the
    image in front of and behind the patch, outside the border, behind the camera.  Shared by the CPU and the GPU test."""
    rs = np.random.RandomState(11)
    H, W = 64, 96
    depth = rs.uniform(2.5, 3.5, (8, H, W)).astype(F)
    pix = [(48, 32), (20, 40), (80, 15), (30, 50), (60, 30), (85, 52), (5, 30), (48, 32)]
    z = [2.0, 2.9, 3.0, 1.5, 2.2, 3.3, 2.0, -1.0]
    patch = [4.0, 1.0, 5.5, 1.0, 9.0, 0.4, 4.0, 4.0]                       # the window's depth: beyond or in front of the target
    pts = []
    for i, ((px, py), zi, d) in enumerate(zip(pix, z, patch)):
        depth[i, max(py - 12, 0):py + 12, max(px - 12, 0):px + 12] = d + rs.uniform(-0.05, 0.05, depth[i, max(py - 12, 0):py + 12, max(px - 12, 0):px + 12].shape)
        pts.append([(px + 0.5 - K96[0, 2]) * zi / K96[0, 0], (py + 0.5 - K96[1, 2]) * zi / K96[1, 1], zi])
    return depth, np.array(pts)


# ---- the reframe formulas in a chosen precision (rotation vector <-> matrix through a quaternion) ----
def _quat_of_rotvec(r, dt):
    r = np.asarray(r, dt)
    ang = np.sqrt((r * r).sum(-1, dtype=dt)).astype(dt)
    small = ang < dt(1e-3)
    a2 = ang * ang
    k = np.where(small, dt(0.5) - a2 / dt(48) + a2 * a2 / dt(3840), np.sin(ang / dt(2)) / np.where(small, dt(1), ang)).astype(dt)
    return np.concatenate([r * k[..., None], np.cos(ang / dt(2))[..., None]], -1).astype(dt)       # x, y, z, w


def _matrix_of_quat(q, dt):
    x, y, z, w = (q[..., i] for i in range(4))
    two = dt(2)
    m = np.stack([dt(1) - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                  two * (x * y + z * w), dt(1) - two * (x * x + z * z), two * (y * z - x * w),
                  two * (x * z - y * w), two * (y * z + x * w), dt(1) - two * (x * x + y * y)], -1)
    return m.reshape(q.shape[:-1] + (3, 3)).astype(dt)


def _quat_of_matrix(m, dt):
    """The branch with the largest of (trace, m00, m11, m22): no cancellation near pi."""
    m = np.asarray(m, dt)
    out = np.zeros(m.shape[:-2] + (4,), dt)
    for idx in np.ndindex(m.shape[:-2]):
        a = m[idx]
        d = [a[0, 0], a[1, 1], a[2, 2], a[0, 0] + a[1, 1] + a[2, 2]]
        k = int(np.argmax(d))
        if k == 3:
            q = [a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1], dt(1) + d[3]]
        else:
            i, j, l = k, (k + 1) % 3, (k + 2) % 3
            q = [dt(0)] * 4
            q[i] = dt(1) - d[3] + dt(2) * a[i, i]
            q[j] = a[j, i] + a[i, j]
            q[l] = a[l, i] + a[i, l]
            q[3] = a[l, j] - a[j, l]
        q = np.array(q, dt)
        out[idx] = q / np.sqrt((q * q).sum(dtype=dt)).astype(dt)
    return out


def _rotvec_of_quat(q, dt):
    q = np.where(q[..., 3:] < 0, -q, q).astype(dt)
    s = np.sqrt((q[..., :3] ** 2).sum(-1, dtype=dt)).astype(dt)
    ang = (dt(2) * np.arctan2(s, q[..., 3])).astype(dt)
    small = ang < dt(1e-3)
    a2 = ang * ang
    k = np.where(small, dt(2) + a2 / dt(12) + dt(7) * a2 * a2 / dt(2880), ang / np.where(small, dt(1), np.sin(ang / dt(2)))).astype(dt)
    return (q[..., :3] * k[..., None]).astype(dt)


def rotation_matrix(rotvec, dt=np.float64):
    return _matrix_of_quat(_quat_of_rotvec(rotvec, dt), dt)


def reframe(global_orient, transl, delta_T, trans, dt=np.float64):
    """training_data.reframe_bodies, every statement in ``dt``: (global_orient', transl', pelvis') [N,n,3]."""
    go, tr = np.asarray(global_orient, dt).reshape(-1, 3), np.asarray(transl, dt).reshape(-1, 3)
    dT = np.broadcast_to(np.asarray(delta_T, dt), tr.shape)
    T = np.asarray(trans, dt).reshape(-1, 4, 4)
    Rt, tt = T[:, :3, :3], T[:, :3, 3]
    R_new = np.einsum('nij,Njk->Nnik', Rt, rotation_matrix(go, dt)).astype(dt)
    go_new = _rotvec_of_quat(_quat_of_matrix(R_new, dt), dt)
    pelvis = (np.einsum('nij,Nj->Nni', Rt, tr + dT).astype(dt) + tt[None]).astype(dt)
    return go_new, (pelvis - dT[:, None]).astype(dt), pelvis
