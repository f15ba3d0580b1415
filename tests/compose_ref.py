"""NumPy restatement of the result images' contract (include/psi_hip.h, DESIGN.md "Result images"), built on tests/raster_ref.py: the bodies of
a view are concatenated into one mesh whose triangle index is the global id draw * F + face; the pieces and their coverage are
``raster_ref.setup_pieces`` / ``render_ref``; the owner rule, the normals, the shading and the colours follow in fp64 from the same snapped
coordinates.  Also the fixture that the CPU and the GPU tests share."""
import functools

import numpy as np

import raster_ref as R

F32 = np.float32


def vertex_normal_sums(bverts, faces):
    """(sums, bounds), both fp64 [B,V,3]: per vertex the sum of its faces' (v1 - v0) x (v2 - v0), and the sum of their absolute values."""
    bv, f = np.asarray(bverts, np.float64), np.asarray(faces, np.int64)
    cr = np.cross(bv[:, f[:, 1]] - bv[:, f[:, 0]], bv[:, f[:, 2]] - bv[:, f[:, 0]])          # [B,F,3]
    n, a = np.zeros_like(bv), np.zeros_like(bv)
    for k in range(3):
        for b in range(len(bv)):
            np.add.at(n[b], f[:, k], cr[b])
            np.add.at(a[b], f[:, k], np.abs(cr[b]))
    return n, a


def csr_of_faces(faces, V):
    """(offsets [V+1], list [3F]): the faces of every vertex in ascending face index."""
    f = np.asarray(faces, np.int64)
    lists = [[] for _ in range(V)]
    for i, tri in enumerate(f):
        for v in tri:
            lists[v].append(i)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    return off, np.array([i for l in lists for i in l], np.int64)


def shade(N):
    """s = 0.3 + 0.7 |N_z| / |N|, 0.3 where the length is 0 or not finite; N [...,3] fp64."""
    with np.errstate(all='ignore'):
        ln = np.sqrt((N ** 2).sum(-1))
        s = 0.3 + 0.7 * np.abs(N[..., 2]) / ln
    return np.where((ln > 0) & np.isfinite(ln), s, 0.3)


def _render_attrs(verts, faces, attrs, w2c, intr, size, near, ids=None):
    """``render_ref`` of one view with three attributes per vertex: returns its dict plus 'attr' [H,W,3] = z * sum l_i a_i / z_i."""
    H, W = size
    out, chans = None, []
    for c in range(3):
        pc = R.setup_pieces(verts, faces, attrs[:, c], w2c, intr, near)
        if ids is not None:
            pc['tri'] = ids[pc['tri']]
        r = R.render_ref(pc, W, H)
        chans.append(r['seg'])
        out = r
    out = dict(out)
    out['attr'] = np.stack(chans, -1)
    return out


def compose_views(scene, bverts, bfaces, draw_body, draw_view, draw_rgb, cam_ext, cam_int, size, near=0.05, background=(1.0, 1.0, 1.0)):
    """scene: None or (verts, faces, vrgb or None).  Returns stacked [n,H,W] arrays: 'draw' (owner draw or -1), 'body_hit', 'body_id',
    'body_clear', 'body_depth', 'scene_hit', 'scene_depth', 'depth', 'near_tie' (body and scene within 1e-4 relative), 'colour' [n,H,W,3]
    fp64 before the rounding, 'rgb' [n,H,W,3] the levels; and 'counts' [M,2]."""
    H, W = size
    w2c = R.world_to_camera_rows(cam_ext)
    n = len(w2c)
    K = np.asarray(cam_int, np.float64)
    K = np.broadcast_to(K, (n, 3, 3)) if K.ndim == 2 else K
    bverts, bfaces = np.asarray(bverts, F32), np.asarray(bfaces, np.int64)
    nF, V = len(bfaces), bverts.shape[1]
    draw_body, draw_view = np.asarray(draw_body, np.int64), np.asarray(draw_view, np.int64)
    draw_rgb = np.asarray(draw_rgb, F32).astype(np.float64).reshape(len(draw_body), 3)
    M = len(draw_body)
    normals = vertex_normal_sums(bverts, bfaces)[0]
    counts = np.zeros((M, 2), np.int64)
    keys = ('draw', 'body_hit', 'body_id', 'body_clear', 'body_depth', 'scene_hit', 'scene_depth', 'depth', 'near_tie', 'colour', 'rgb')
    res = {k: [] for k in keys}
    for v in range(n):
        intr = np.array([K[v, 0, 0], K[v, 1, 1], K[v, 0, 2], K[v, 1, 2]], F32)
        m = w2c[v].astype(np.float64)
        colour = np.broadcast_to(np.asarray(background, F32).astype(np.float64), (H, W, 3)).copy()
        # the scene
        s_hit, zs, s_col = np.zeros((H, W), bool), np.zeros((H, W)), None
        if scene is not None:
            sv, sf, srgb = scene
            sv, sf = np.asarray(sv, F32), np.asarray(sf, np.int64)
            attrs = np.full((len(sv), 3), 0.8, F32) if srgb is None else np.asarray(srgb, F32)
            r = _render_attrs(sv, sf, attrs, w2c[v], intr, size, near)
            s_hit, zs = r['hit'], r['depth']
            cam = R._camera(sv, w2c[v]).astype(np.float64)
            flat = np.cross(cam[sf[:, 1]] - cam[sf[:, 0]], cam[sf[:, 2]] - cam[sf[:, 0]])
            base = r['attr'] if srgb is not None else np.full((H, W, 3), np.float64(F32(0.8)))
            s_col = base * shade(flat[np.maximum(r['tri'], 0)])[..., None]
        # the bodies of this view, as one mesh
        ds = np.nonzero(draw_view == v)[0]
        b_hit, zb, b_id, b_clear = np.zeros((H, W), bool), np.zeros((H, W)), np.full((H, W), -1, np.int64), np.ones((H, W), bool)
        if len(ds):
            cv = np.concatenate([bverts[draw_body[d]] for d in ds])
            cf = np.concatenate([bfaces + i * V for i in range(len(ds))])
            ids = np.concatenate([d * nF + np.arange(nF) for d in ds])
            ncam = np.concatenate([normals[draw_body[d]] for d in ds]) @ m[:, :3].T
            r = _render_attrs(cv, cf, ncam.astype(F32), w2c[v], intr, size, near, ids)
            b_hit, zb, b_id, b_clear = r['hit'], r['depth'], r['tri'], r['clear']
            b_col = draw_rgb[np.maximum(b_id, 0) // nF] * shade(r['attr'])[..., None]      # the factor z of 'attr' does not change the direction
        owns = b_hit & (~s_hit | (zb < zs))
        if scene is not None:
            colour[s_hit & ~owns] = s_col[s_hit & ~owns]
        if len(ds):
            colour[owns] = b_col[owns]
            dd = b_id[b_hit] // nF
            np.add.at(counts[:, 0], dd, 1)
            np.add.at(counts[:, 1], b_id[owns] // nF, 1)
        with np.errstate(all='ignore'):
            tie = b_hit & s_hit & (np.abs(zb - zs) <= 1e-4 * np.minimum(zb, zs))
        for k, a in zip(keys, (np.where(owns, b_id // nF, -1), b_hit, b_id, b_clear, zb, s_hit, zs, np.where(owns, zb, zs), tie, colour,
                               np.rint(255.0 * np.clip(colour, 0.0, 1.0)).astype(np.int64))):
            res[k].append(a)
    out = {k: np.stack(a) for k, a in res.items()}
    out['counts'] = counts
    return out


def counts_from_images(body_id, body_depth, scene_depth, scene_hit, M, nF):
    """counts [M,2] recomputed from returned images: covered = pixels of the draw in body_id, visible = those with no scene hit or a nearer body."""
    counts = np.zeros((M, 2), np.int64)
    hit = body_id >= 0
    d = body_id[hit] // nF
    np.add.at(counts[:, 0], d, 1)
    vis = ~scene_hit[hit] | (body_depth[hit] < scene_depth[hit])
    np.add.at(counts[:, 1], d[vis], 1)
    return counts


# ---- the fixture ----
SIZES = [(48, 64), (45, 70)]
BACKGROUND = (1.0, 1.0, 1.0)


def K_of(size, f=50.0):
    return R.intrinsics(f, f, size[1] / 2.0, size[0] / 2.0)


@functools.lru_cache(None)
def fixture():
    """Scene make_room_mesh(0, 40) with vertex colours from RandomState(5); the four cameras of make_room_cams; six default capsules: five
    translated (two sink 2 cm into the floor, two interpenetrate), one around the third camera's eye, across z = near; every body in every
    view (M = 24), a colour per draw."""
    from psi_release_amd import synth
    room = synth.make_room_mesh(0, 40)
    vrgb = np.random.RandomState(5).uniform(0.05, 1.0, (len(room.verts), 3)).astype(F32)
    cams = np.concatenate([synth.make_room_cams('inside'), synth.make_room_cams('outside')])
    cv, cf = synth.make_capsule_mesh()
    eye, fwd = cams[2][:3, 3], cams[2][:3, 2]
    shifts = [[0.2, -0.1, -0.02], [0.9, 0.6, -0.02], [-0.6, -0.7, -0.02], [0.25, -0.05, 0.0], [2.2, 1.7, 0.0], eye + 0.10 * fwd - np.array([0.0, 0.0, 0.85])]
    bverts = np.stack([cv.astype(np.float64) + np.asarray(s) for s in shifts]).astype(F32)
    draw_body, draw_view = np.repeat(np.arange(6), 4), np.tile(np.arange(4), 6)
    draw_rgb = np.random.RandomState(6).uniform(0.2, 1.0, (24, 3)).astype(F32)
    fx = dict(room=room, vrgb=vrgb, cams=cams, bverts=bverts, bfaces=cf, draw_body=draw_body, draw_view=draw_view, draw_rgb=draw_rgb)
    for a in fx.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return fx


@functools.lru_cache(None)
def fixture_reference(size):
    """The restatement's images of the fixture; computed once, never modified."""
    fx = fixture()
    ref = compose_views((fx['room'].verts, fx['room'].faces, fx['vrgb']), fx['bverts'], fx['bfaces'], fx['draw_body'], fx['draw_view'], fx['draw_rgb'],
                        fx['cams'], K_of(size), size, background=BACKGROUND)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def check_images(got, ref, nF, max_excluded=0.01):
    """The assertions of GPU test 1 for one set of images (dict of numpy arrays: rgb, depth, draw, body_depth, body_id, counts).  Prints and
    returns the measured figures: excluded share, max relative depth errors, max level difference, share of channels that differ."""
    assert np.array_equal(got['body_id'] >= 0, ref['body_hit'])                         # the body-only hit mask, on every pixel
    assert np.array_equal(got['body_id'][ref['body_clear']], ref['body_id'][ref['body_clear']])
    compared = ~ref['near_tie']
    assert np.array_equal(got['draw'][compared], ref['draw'][compared])
    excluded = 1.0 - (compared & ref['body_clear']).mean()
    assert excluded <= max_excluded
    same = (got['draw'] == ref['draw']) & (got['body_id'] == ref['body_id'])
    own = same & ((ref['draw'] >= 0) | ref['scene_hit'])
    derr = np.abs(got['depth'][own] / ref['depth'][own] - 1.0).max() if own.any() else 0.0
    bh = same & ref['body_hit']
    berr = np.abs(got['body_depth'][bh] / ref['body_depth'][bh] - 1.0).max() if bh.any() else 0.0
    assert (got['depth'][same & ~own] == 0).all() and (got['body_depth'][~ref['body_hit']] == 0).all()
    lev = np.abs(got['rgb'][same].astype(np.int64) - ref['rgb'][same])
    share = (lev != 0).mean() if lev.size else 0.0
    print('excluded %.2e, depth rel err %.2e, body depth rel err %.2e, max level difference %d, share of channels that differ %.2e'
          % (excluded, derr, berr, lev.max() if lev.size else 0, share))
    assert derr <= 1e-5 and berr <= 1e-5
    assert lev.size == 0 or lev.max() <= 1
    return excluded, derr, berr, share
