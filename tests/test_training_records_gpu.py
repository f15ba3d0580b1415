"""psi_snapshot_canvas (csrc/canvas.hip) on the GPU against the NumPy restatement of DESIGN.md section 12 (tests/records_ref.py), the host
geometry of training_data.py against the skinning kernel, and TrainingSetBuilder end to end on the stand-in room."""
import functools

import numpy as np
import pytest
import torch

import records_ref as R
from conftest import golden, rel_err
from psi_release_amd import batch_gen, body_model, ops, rendering, synth
from psi_release_amd import training_data as TD

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32
GOLDEN_TAG = {(96, 160): 'wide', (150, 90): 'tall', (64, 64): 'square'}
# (H, W, n): every shape alone and five at a time; 128 x 75 has an odd width and H * W % 4 == 0, 150 x 90 and 1 x 1 take the scalar read,
# 270 x 480 is the production size (32 workgroups per view in the maximum pass)
CASES = [(h, w, n) for (h, w) in [(96, 160), (150, 90), (64, 64), (128, 75), (1, 1)] for n in (1, 5)] + [(270, 480, 3), (15, 21, 5)]
T = lambda a: torch.tensor(np.asarray(a), device=DEV)


@functools.lru_cache(None)
def views(H, W, n):
    """Inputs with values above both clips; view 0 is the reference's recorded input where there is one; of five views, view 1 is all
    zeros and view 3 holds a single NaN.  Read-only."""
    rs = np.random.RandomState(1000 * H + W)
    depth, seg = rs.uniform(0.3, 8.0, (n, H, W)).astype(F), rs.uniform(0.0, 50.0, (n, H, W)).astype(F)
    if (H, W) in GOLDEN_TAG:
        g = golden('preproc')
        depth[0], seg[0] = g[GOLDEN_TAG[(H, W)] + '_depth_in'], g[GOLDEN_TAG[(H, W)] + '_seg_in']
    if H * W == 1:
        depth[0], seg[0] = 7.5, 45.0
    if n == 5:
        depth[1] = 0
        depth[2] *= F(0.5)                      # a view whose maximum is below the clip
        (seg if H * W > 1 else depth)[3, H // 2, W // 3] = np.nan
    for a in (depth, seg):
        a.setflags(write=False)
    return depth, seg


@functools.lru_cache(None)
def expected(H, W, n):
    out = R.snapshot_canvas(*views(H, W, n))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def computed(H, W, n):
    depth, seg = views(H, W, n)
    d, s = T(depth), T(seg)
    out = ops.snapshot_canvas(d, s)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), d.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize('H,W,n', CASES)
def test_canvas_kernel_against_the_restatement(H, W, n):
    depth, seg = views(H, W, n)
    (dc, sc, max_d, seg_max, usable), d_after, s_after = computed(H, W, n)
    rdc, rsc, rmax_d, rseg_max, rusable = expected(H, W, n)
    err_d, err_s = np.abs(dc - rdc).max(), np.abs(sc - rsc).max()
    print('%d x %d n=%d: canvas error depth %.3g seg %.3g' % (H, W, n, err_d, err_s))
    assert dc.shape == sc.shape == (n, 1, 128, 128) and usable.dtype == np.int32
    assert np.array_equal(max_d, rmax_d) and np.array_equal(seg_max, rseg_max) and np.array_equal(usable, rusable)      # exact
    assert max_d[0] == F(6.0) and seg_max[0] == F(41.0)                                                                 # both clips bind
    assert err_d <= 1e-6 and err_s <= 1e-6
    oh, ow, y0, x0 = R.placement(H, W, 128, 128)
    pad = np.ones((128, 128), bool)
    pad[y0:y0 + oh, x0:x0 + ow] = False                          # the padding: exactly 0
    assert not dc[:, 0][:, pad].any() and not sc[:, 0][:, pad].any()
    assert np.array_equal(d_after.view(np.uint32), depth.view(np.uint32)) and np.array_equal(s_after.view(np.uint32), seg.view(np.uint32))
    if n == 5:
        assert list(usable) == [1, 0, 1, 0, 1] and not dc[[1, 3]].any() and not sc[[1, 3]].any()
        assert max_d[1] == 0 and max_d[2] < F(6.0) and np.isfinite(seg_max).all() and np.isfinite(max_d).all()
    if (H, W) in GOLDEN_TAG:
        g = golden('preproc')
        tag = GOLDEN_TAG[(H, W)]
        assert np.abs(dc[0, 0] - g[tag + '_depth_canvas'].reshape(128, 128)).max() <= 2e-6
        assert np.abs(sc[0, 0] - g[tag + '_seg_canvas'].reshape(128, 128)).max() <= 2e-6
        assert float(max_d[0]) == float(g[tag + '_depth_max']) and float(seg_max[0]) == float(g[tag + '_seg_max'])


@pytest.mark.parametrize('H,W', [(96, 160), (128, 75), (15, 21)])
def test_views_do_not_depend_on_their_call(H, W):
    """The five-view call against five one-view calls, and against itself: the same bits."""
    depth, seg = views(H, W, 5)
    whole = computed(H, W, 5)[0]
    d, s = T(depth), T(seg)
    again = [o.cpu().numpy() for o in ops.snapshot_canvas(d, s)]
    for a, b in zip(whole, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i in range(5):
        one = [o.cpu().numpy() for o in ops.snapshot_canvas(d[i:i + 1].clone(), s[i:i + 1].clone())]
        for a, b in zip(whole, one):
            assert np.array_equal(a[i:i + 1].view(np.uint32), b.view(np.uint32)), i


def test_window_flags():
    depth, pts = R.window_views()
    windows, z, inside = TD.target_windows(pts, R.K96, depth.shape[1:])
    for i in np.nonzero(inside)[0]:
        assert abs(R.window_mean(depth[i], windows[i]) - z[i]) > 1e-3          # no view sits on a tie
    seg = np.ones_like(depth)
    want = R.snapshot_canvas(depth, seg, (128, 128), windows, z.astype(F))
    got = ops.snapshot_canvas(T(depth), T(seg), (128, 128), windows, z.astype(F))
    usable = got[4].cpu().numpy()
    assert np.array_equal(usable, want[4]) and set(usable[:6]) == {0, 1} and not usable[6:].any()
    assert [bool(u) for u in usable] == [rendering.view_is_usable(depth[i], pts[i], R.K96) for i in range(len(pts))]
    assert np.abs(got[0].cpu().numpy() - want[0]).max() <= 1e-6
    # a window larger than one 256-pixel round of the adder, cut to the image on two sides
    big = np.array([[-5, 10, 60, 200]] * len(depth), np.int32)
    zz = np.tile([2.9, 3.1], len(depth) // 2).astype(F)
    assert all(abs(R.window_mean(depth[i], big[i]) - float(zz[i])) > 1e-3 for i in range(len(depth)))
    assert np.array_equal(ops.snapshot_canvas(T(depth), T(seg), (128, 128), big, zz)[4].cpu().numpy(), R.snapshot_canvas(depth, seg, (128, 128), big, zz)[4])


def test_refused_arguments():
    d = torch.ones(1, 8, 8, device=DEV)
    for size in ((127, 128), (128, 0), (128, 4)):                # odd, empty, and a resized image (128 x 128) that does not fit
        with pytest.raises(ops.hip.PsiHipError):
            ops.snapshot_canvas(d, d, size)
    with pytest.raises(ValueError):
        ops.snapshot_canvas(d, d, (128, 128), windows=np.zeros((1, 4), np.int32))


# ---- the host geometry against the skinning kernel ----
@functools.lru_cache(None)
def layer():
    return body_model.create(synth.make_smplx(7), num_pca_comps=12, batch_size=4, device=DEV)


def _skin(betas, pose, transl):
    shape = np.concatenate([betas, np.zeros_like(betas)], 1)     # 10 betas | 10 expression coefficients
    v, j = body_model.lbs(layer().lbs_model, T(shape.astype(F)), T(pose.astype(F)), T(transl.astype(F)), return_joints=True)
    return v.cpu().numpy().astype(np.float64), j.cpu().numpy().astype(np.float64)


def test_pelvis_table_is_joint_0_whatever_the_pose():
    rs = np.random.RandomState(4)
    B = 6
    betas, pose = rs.standard_normal((B, 10)), rs.standard_normal((B, 165)) * 0.6        # random body, face and hand poses
    pose[:, :3] = 0
    _, joints = _skin(betas, pose, np.zeros((B, 3)))
    J0, dJ0 = TD.pelvis_table(synth.make_smplx(7))
    err = np.abs(joints[:, 0] - (J0 + betas @ dJ0.T)).max()
    print('pelvis table against joint 0: %.3g' % err)
    assert err <= 1e-5


def test_reframed_bodies_skin_to_the_transformed_world_body():
    """4 bodies x 3 cameras: skinning (global_orient', transl') as they stand equals inv(cam_ext) applied to the skinned world body."""
    rs = np.random.RandomState(8)
    B = 4
    betas, pose, transl = rs.standard_normal((B, 10)), rs.standard_normal((B, 165)) * 0.4, rs.standard_normal((B, 3))
    pose[1, :3] *= (np.pi - 5e-4) / np.linalg.norm(pose[1, :3])                          # an orientation near pi
    cams = synth.make_cam_ext(21, 3).astype(np.float64)
    w2c = np.linalg.inv(cams)
    J0, dJ0 = TD.pelvis_table(synth.make_smplx(7))
    go_c, t_c, pelvis_c = TD.reframe_bodies(pose[:, :3], transl, J0 + betas @ dJ0.T, w2c)
    world, world_j = _skin(betas, pose, transl)
    for j in range(3):
        p = pose.copy()
        p[:, :3] = go_c[:, j]
        got, got_j = _skin(betas, p, t_c[:, j])
        want = world @ w2c[j, :3, :3].T + w2c[j, :3, 3]
        e = rel_err(got, want)
        print('camera %d: rel_err %.3g' % (j, e))
        assert e <= 1e-4
        assert rel_err(got_j[:, 0], pelvis_c[:, j]) <= 1e-4


# ---- the builder ----
class _Recording(TD.TrainingSetBuilder):
    def _render(self, cam_ext):
        depth, seg = super()._render(cam_ext)
        self.passes = getattr(self, 'passes', []) + [(np.asarray(cam_ext).copy(), depth.cpu().numpy(), seg.cpu().numpy())]
        return depth, seg


def test_builder_end_to_end_on_the_stand_in_room():
    room = synth.make_room_mesh(0, 180)
    data = synth.make_smplx(7)
    mesh = rendering.SceneMesh(room.verts, room.faces, room.labels, device=DEV)
    b = _Recording(mesh, data, R.K96, size=(64, 96), scene_id=0, room_planes=room.planes(), box_shrink=0.3, n_cams=4, frames_per_pass=8, seed=1,
                   keep_images=True)
    bodies = TD.synthetic_bodies(data, room.box_min, room.box_max, 3, seed=2)
    b.add_frames(bodies)
    t = b.table()
    assert len(b.passes) == 1                                    # three frames, one pass: one render call
    cams, depth, seg = b.passes[0]
    s = b.stats
    assert s['views_sampled'] == len(cams) == 12 == s['kept'] + sum(s['dropped_' + r] for r in TD.DROP_RULES) and s['frames'] == 3
    # the restatement's decision on the same rendered images
    J0, dJ0 = TD.pelvis_table(data)
    rows = np.repeat(np.arange(3), 4)
    dT = J0 + bodies['betas'] @ dJ0.T
    go_c, t_c, pelvis_c = (np.stack([a[rows[i], i] for i in range(12)]) for a in
                           TD.reframe_bodies(bodies['global_orient'], bodies['transl'], dT, np.linalg.inv(cams)))
    windows, z, inside = TD.target_windows(pelvis_c, R.K96, (64, 96))
    for i in np.nonzero(inside)[0]:
        assert abs(R.window_mean(depth[i], windows[i]) - z[i]) > 1e-3
    rdc, rsc, rmax_d, _, rusable = R.snapshot_canvas(depth, seg, (128, 128), windows, z.astype(F))
    kept, _ = TD.select_views(inside, rusable > 0, t_c, rmax_d)
    k = int(kept.sum())
    print('kept %d of 12 views; stats %s' % (k, s))
    assert k >= 1 and s['kept'] == k == len(t['depth']) - 1
    assert np.array_equal(b.record_ids(), np.stack([rows, np.tile(np.arange(4), 3)], 1)[kept])
    assert np.array_equal(t['max_d'][1:], rmax_d[kept])                                   # exact
    assert np.abs(t['depth'][1:] - rdc[kept]).max() <= 1e-6 and np.abs(t['seg'][1:] - rsc[kept]).max() <= 1e-6
    assert np.abs(t['body'][1:, :3] - t_c[kept]).max() <= 1e-6 and np.array_equal(t['cam_ext'][1:], cams[kept].astype(F))
    d0, s0 = b.images()
    assert np.array_equal(d0, depth[kept]) and np.array_equal(s0, seg[kept])
    scene = synth.make_scene(100, 64, 8, 14)
    bg = batch_gen.BatchGeneratorWithSceneMesh.from_arrays(t, {'room': {q: getattr(scene, q) for q in ('verts', 'sdf', 'grid_min', 'grid_max', 'grid_dim')}}, DEV)
    batch = bg.next_batch(1)
    assert batch is not None and len(batch) == 12 and tuple(batch[0].shape) == (1, 1, 128, 128) and tuple(batch[2].shape) == (1, 72)
