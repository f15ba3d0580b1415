"""Batched GPU evaluation: the fused skin + SDF sign count (psi_lbs_sdf_counts, SMPLXLayer.sdf_counts, PlausibilityEvaluator.scores_many /
eval_folder_batched / evaluate_scenes) against the operator sequence and the reference's recorded scores, and the k-means of the
diversity evaluation (psi_kmeans_*, psi_vq, evaluation.diversity_reference) against an fp64 restatement of scipy's loop
(tests/test_eval_cpu.py) and scipy's recorded results (tests/golden/diversity.npz)."""
import ctypes
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import fixture_inputs as FI
import fixture_inputs_eval as FE
from test_eval_cpu import kmeans_f64, vq_f64
from psi_release_amd import body_model, evaluation, fitting, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
KEYS = ['transl', 'global_orient', 'betas', 'body_pose', 'left_hand_pose', 'right_hand_pose', 'cam_ext', 'cam_int']
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
V = 10475


def _rooms():
    return [synth.make_scene(**FI.PLAUS_SCENE), synth.make_scene(**dict(FI.PLAUS_SCENE, seed=14, radius=1.5)),
            synth.make_scene(**dict(FI.PLAUS_SCENE, seed=24, radius=1.1))]


def _habitat_op(smplx_data, vposer_sd, scene):
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.1,
           'num_iter': 1, 'batch_size': 1, 'device': torch.device(DEV), 'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None,
           'verbose': False, 'smplx_data': smplx_data, 'vposer_state': vposer_sd, 'scene': scene, 'engine': 'modular'}
    return fitting.FittingOPHabitat(cfg, {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5})


def _allowance(sdfv):
    """Per body: the number of vertices of the operator path whose |sdf| is at rounding level (<= 1e-6 max|sdf|), capped at 3 of 10475."""
    a = sdfv.abs()
    return torch.clamp((a <= 1e-6 * a.max(1, keepdim=True)[0]).sum(1), max=3).cpu().numpy()


def _operator_counts(layer, par, cam, sdf, gmin, gmax, sid, ac):
    verts = layer(return_verts=True, cam_ext=cam, **par).vertices
    sdfv = ops.sdf_sample(verts, sdf, gmin, gmax, scene_id=sid, align_corners=ac)
    return torch.stack([(sdfv < 0).sum(1), (sdfv > 0).sum(1)], 1).cpu().numpy(), _allowance(sdfv)


def _layer_params(B, seed):
    b = synth.make_bodies(seed, B)
    rs = np.random.RandomState(seed + 1000)
    return {'betas': T(b['betas']), 'global_orient': T(b['global_orient']), 'transl': T(b['transl']),
            'left_hand_pose': T(b['left_hand_pose']), 'right_hand_pose': T(b['right_hand_pose']),
            'body_pose': T(rs.standard_normal((B, 63)) * 0.2)}


def test_counts_equal_operator_sequence(smplx_data):
    layer = body_model.create(smplx_data, model_type='smplx', num_pca_comps=12, batch_size=1, device=DEV)
    rooms = _rooms()
    sdf = T(np.stack([r.sdf for r in rooms]))
    gmin, gmax = T(np.stack([r.grid_min for r in rooms])), T(np.stack([r.grid_max for r in rooms]))
    worst, both_signs = 0, 0
    for B in (1, 2, 33, 64, 131, 513):
        par = _layer_params(B, 40 + B)
        sid = torch.tensor(np.random.RandomState(B).randint(0, 3, B).astype(np.int32), device=DEV)
        cam = T(synth.make_cam_ext(5 + B, B))
        for ac in (True, False):
            for use_cam, use_transl in ((True, True), (False, True), (True, False), (False, False)):
                p = {k: v for k, v in par.items() if use_transl or k != 'transl'}
                c = cam if use_cam else None
                ref, allow = _operator_counts(layer, p, c, sdf, gmin, gmax, sid, ac)
                got = layer.sdf_counts(sdf, gmin, gmax, scene_id=sid, align_corners=ac, cam_ext=c, **p)
                assert got.dtype == torch.int32 and tuple(got.shape) == (B, 2)
                diff = np.abs(got.cpu().numpy().astype(np.int64) - ref).max(1)
                worst = max(worst, int(diff.max()))
                both_signs += int(((ref[:, 0] > 0) & (ref[:, 1] > 0)).sum())
                assert (diff <= allow).all(), (B, ac, use_cam, use_transl, diff.max(), allow[diff.argmax()])
                assert (got.sum(1) <= V).all()
    print('sdf_counts vs operator sequence: largest per-body count difference = %d (0 expected)' % worst)
    assert both_signs > 0                       # the comparison saw bodies that straddle a surface
    # scene 0 when scene_id is None; a [D,D,D] volume is accepted like ops.sdf_sample accepts it
    par = _layer_params(5, 3)
    ref, allow = _operator_counts(layer, par, None, sdf[0], gmin[0], gmax[0], None, True)
    got = layer.sdf_counts(sdf[0], gmin[0], gmax[0], **par).cpu().numpy()
    assert (np.abs(got - ref).max(1) <= allow).all()


def _write_golden_pkls(gen, g):
    os.makedirs(gen, exist_ok=True)
    n = g['in_transl'].shape[0]
    for i in range(n):
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump({k: g['in_' + k][i] for k in KEYS}, f)
    return n


def _folder_allowance(ev, folder, max_files=8000):
    """The rule of test_counts_equal_operator_sequence for the pkls of a folder: per body, the operator path's rounding-level vertices."""
    out = []
    op = ev.op
    for ii in range(max_files):
        fn = os.path.join(folder, 'body_gen_{:06d}.pkl'.format(ii))
        if not os.path.exists(fn):
            continue
        with open(fn, 'rb') as f:
            xh, cam_ext, _ = evaluation.BodyParamParser.body_params_parse_fitting(pickle.load(f))
        cam = cam_ext
        if ev.flip:
            cam = torch.matmul(cam_ext[:1], torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], device=op.device)).unsqueeze(0))
        cam = cam[:1].expand(xh.shape[0], -1, -1).contiguous()
        xh_rec = evaluation.GeometryTransformer.convert_to_3D_rot(evaluation.GeometryTransformer.convert_to_6D_rot(xh))
        sdfv = ops.sdf_sample(op.body_verts(xh_rec, cam), op.s_sdf, op.s_grid_min_batch, op.s_grid_max_batch, align_corners=op.align_corners)
        out.extend(_allowance(sdfv).tolist())
    return np.array(out)


def _same_under_rule(coll_a, cont_a, coll_b, cont_b, allow):
    d = np.abs(np.array(coll_a) - np.array(coll_b)) * 10475.0
    print('batched vs per-file: largest difference = %.3f vertices' % (d.max() if len(d) else 0.0))
    assert (d <= allow + 1e-6).all(), (d, allow)
    assert all(a == b for a, b, al in zip(cont_a, cont_b, allow) if al == 0)


@pytest.mark.parametrize('tag', ['ac1', 'ac0'])
def test_batched_scores_equal_reference_script(tmp_path, smplx_data, vposer_sd, tag):
    g = golden('plausibility')
    gen = str(tmp_path / 'gen')
    n = _write_golden_pkls(gen, g)
    op = _habitat_op(smplx_data, vposer_sd, synth.make_scene(**FI.PLAUS_SCENE))
    op.align_corners = (tag == 'ac1')
    ev = evaluation.PlausibilityEvaluator(op, flip_camera_yz=True)
    coll, cont = ev.eval_folder_batched(gen)
    assert isinstance(coll, list) and len(coll) == n and cont == list(g['cont_' + tag])
    assert np.abs(np.array(coll) - g['coll_' + tag]).max() <= 3.0 / 10475.0 + 1e-12, (coll, g['coll_' + tag])
    coll_f, cont_f = ev.eval_folder(gen)
    _same_under_rule(coll, cont, coll_f, cont_f, _folder_allowance(ev, gen))


def test_chunking_and_scenes(tmp_path, smplx_data, vposer_sd):
    rooms = _rooms()
    opsl = [_habitat_op(smplx_data, vposer_sd, r) for r in rooms]
    ev = evaluation.PlausibilityEvaluator(opsl[0], flip_camera_yz=True)
    b = synth.make_bodies(77, 40)
    xh = synth.body_vector_72(b)
    cam = np.asarray(synth.make_cam_ext(9, 40), np.float32)
    res = [ev.scores_many(xh, cam, chunk=c) for c in (1, 7, 512)]
    for coll, cont in res:
        assert coll.dtype == np.float64 and cont.dtype == np.float64 and coll.shape == (40,) and cont.shape == (40,)
        assert np.array_equal(coll, res[0][0]) and np.array_equal(cont, res[0][1])
    one = ev.scores_many(xh, cam[:1])                   # [1,4,4]: one camera for all
    assert np.array_equal(one[0][0], res[0][0][0])
    # three rooms in one pass == three single-scene passes
    names = ['roomA', 'roomB', 'roomC']
    gen = str(tmp_path / 'gen')
    for si, name in enumerate(names):
        os.makedirs(os.path.join(gen, name))
        for ii in range(3):
            with open(os.path.join(gen, name, 'body_gen_{:06d}.pkl'.format(ii if ii < 2 else 5)), 'wb') as f:     # a gap in the numbering
                pickle.dump(synth.make_bodies(100 * si + ii, 1 + ii), f)
    allr = evaluation.PlausibilityEvaluator.evaluate_scenes(dict(zip(names, opsl)), gen)
    assert list(allr) == names
    for name, op in zip(names, opsl):
        c1, k1 = evaluation.PlausibilityEvaluator(op, flip_camera_yz=True).eval_folder_batched(os.path.join(gen, name))
        assert len(c1) == 6 and allr[name][0] == c1 and allr[name][1] == k1
    assert len({tuple(v[0]) for v in allr.values()}) > 1               # the rooms differ
    other = _habitat_op(smplx_data, vposer_sd, synth.make_scene(**dict(FI.PLAUS_SCENE, D=16)))
    with pytest.raises(ValueError):
        evaluation.PlausibilityEvaluator.evaluate_scenes({'roomA': opsl[0], 'roomB': other}, gen)


def test_counts_rerun_and_overwrite(smplx_data):
    layer = body_model.create(smplx_data, model_type='smplx', num_pca_comps=12, batch_size=1, device=DEV)
    room = synth.make_scene(**FI.PLAUS_SCENE)
    sdf, gmin, gmax = T(room.sdf[None]), T(room.grid_min[None]), T(room.grid_max[None])
    B = 513
    par = _layer_params(B, 8)
    a = layer.sdf_counts(sdf, gmin, gmax, **par)
    b = layer.sdf_counts(sdf, gmin, gmax, **par)
    assert torch.equal(a, b) and int(a.sum()) > 0
    # the C entry point overwrites `counts`
    shape, pose = layer._assemble(par['betas'], par['global_orient'], par['body_pose'], par['left_hand_pose'], par['right_hand_pose'])
    shape, pose, transl = shape.contiguous(), pose.contiguous(), par['transl'].contiguous()
    m = layer.lbs_model
    ws = m.workspace(B)
    L = hip.lib()

    def call(counts, B_=B, S=1, D=room.sdf.shape[0], sdf_=sdf, gmin_=gmin):
        return L.psi_lbs_sdf_counts(m.handle, hip.ptr(shape), hip.ptr(pose), hip.ptr(transl), None, B_, hip.ptr(sdf_), None, hip.ptr(gmin_),
                                    hip.ptr(gmax), D, S, 1, hip.ptr(counts), hip.ptr(ws), hip.stream())
    c = torch.full((B, 2), -12345, dtype=torch.int32, device=DEV)
    assert call(c) == 0
    assert torch.equal(c, a)
    for kw in (dict(B_=0), dict(B_=16385), dict(S=0), dict(D=1), dict(counts=None), dict(sdf_=None), dict(gmin_=None)):
        cc = kw.pop('counts', c)
        assert call(cc, **kw) != 0, kw
    assert torch.equal(c, a)


def _run_kmeans(x, guess, thresh=1e-5):
    km = evaluation.KMeansRestarts(T(x), T(guess), thresh)
    R = km.R
    while True:
        km.iterate(16)
        if km.converged() == R:
            break
    out = [t.cpu().numpy() for t in km.read()]
    km.close()
    return out


def test_kmeans_easy_case_from_explicit_guess():
    x = FE.easy_case()
    book, k_eff, avg, iters = _run_kmeans(x, x[[0, 0, 150, 250]][None])
    b64, a64, it64 = kmeans_f64(x, x[[0, 0, 150, 250]])
    assert k_eff.tolist() == [3] and iters.tolist() == [it64]
    assert abs(avg[0] - 0.8335614) <= 1e-5 * 0.8335614 and abs(avg[0] - a64) <= 1e-5 * a64
    code, dist = evaluation.vq(T(x), T(book[0, :3]))
    assert np.array_equal(code.cpu().numpy(), vq_f64(x, b64)[0])
    assert np.bincount(code.cpu().numpy()).tolist() == [100, 100, 100]
    far = x[[0, 150, 250, 0]].copy()
    far[3] = 50.0
    book2, k_eff2, avg2, _ = _run_kmeans(x, far[None])
    assert k_eff2.tolist() == [3] and np.array_equal(book2[0, :3], book[0, :3]) and avg2[0] == avg[0]
    # argument checks of the C entry points
    L, h = hip.lib(), ctypes.c_void_p()
    obs, gs = T(x), T(x[:4][None])
    assert L.psi_kmeans_create(ctypes.byref(h), hip.ptr(obs), 3, 72, hip.ptr(gs), 4, 1, 1e-5) != 0         # N < k
    assert L.psi_kmeans_create(ctypes.byref(h), hip.ptr(obs), 300, 129, hip.ptr(gs), 4, 1, 1e-5) != 0      # d > 128
    assert L.psi_kmeans_create(ctypes.byref(h), hip.ptr(obs), 300, 72, hip.ptr(gs), 65, 1, 1e-5) != 0      # k > 64
    assert L.psi_kmeans_create(ctypes.byref(h), hip.ptr(obs), 300, 72, hip.ptr(gs), 4, 65, 1e-5) != 0      # R > 64


@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_diversity_fixtures_against_arbiter_and_scipy(name):
    g = golden('diversity')
    spec = FE.DIV[name]
    x = FE.body_vectors(*spec['data'])
    stats = {}
    res = evaluation.diversity_reference(x, seed=spec['seed'], stats=stats)
    winner = int(g[name + '_winner'])
    # the arbiter's winning restart and the precondition of the equalities below: no near-tie in its final assignment
    b64, a64, _ = kmeans_f64(x, x[g[name + '_init'][winner]].astype(np.float64))
    lab64, dist64, gap = vq_f64(x, b64, with_gap=True)
    print('%s: smallest nearest / second-nearest gap of the final assignment = %.3e' % (name, gap.min()))
    assert gap.min() >= 1e-4
    ref_d, ref_m = float(g[name + '_f64_distortion']), float(g[name + '_f64_mean_dist'])
    assert abs(a64 - ref_d) <= 1e-9 * ref_d
    print('%s: winner %d (committed %d), distortion %.9f (scipy fp64 %.9f), mean_dist %.9f (%.9f), entropy %.12f (%.12f), launches %d, syncs %d' % (
        name, res['winner'], winner, res['distortion'], ref_d, res['mean_dist'], ref_m, res['entropy'], float(g[name + '_f64_entropy']),
        stats['launches'], stats['syncs']))
    assert res['winner'] == winner
    assert np.array_equal(res['counts'], g[name + '_f64_counts'])
    assert np.array_equal(res['labels'], lab64)
    assert res['codes'].shape == g[name + '_f64_codes'].shape
    assert abs(res['entropy'] - float(g[name + '_f64_entropy'])) <= 1e-12
    assert abs(res['distortion'] - ref_d) <= 1e-5 * ref_d
    assert abs(res['mean_dist'] - ref_m) <= 1e-5 * ref_m
    assert stats['syncs'] * 16 * 3 == stats['launches']          # one synchronisation per 16 iterations, three launches per iteration


def test_kmeans_split_independence():
    g = golden('diversity')
    x = FE.body_vectors(*FE.DIV['A']['data'])
    obs = T(x)
    guess = obs[torch.tensor(g['A_init'].reshape(-1), device=DEV)].reshape(FE.RESTARTS, FE.K, 72)

    def run(split):
        km = evaluation.KMeansRestarts(obs, guess)
        for n in split:
            km.iterate(n)
        return km, [t.clone() for t in km.read()]
    km1, a = run([1] * 40)
    km2, b = run([40])
    km3, c = run([40])
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert int(a[3].max()) <= 40 and int(a[3].min()) >= 2
    # frozen once converged
    while km1.converged() < FE.RESTARTS:
        km1.iterate(16)
    done = [t.clone() for t in km1.read()]
    km1.iterate(5)
    for u, v in zip(done, km1.read()):
        assert torch.equal(u, v)
    assert int(done[1].min()) >= 1 and int(done[1].max()) <= FE.K
    for km in (km1, km2, km3):
        km.close()


def test_vq_against_fp64_argmin():
    g = golden('diversity')
    x = FE.body_vectors(*FE.DIV['B']['data'])
    obs = T(x)
    books = [g['B_f64_codes'].astype(np.float32), x[np.random.RandomState(5).choice(len(x), 20, replace=False)]]
    for book in books:
        lab64, dist64, gap = vq_f64(x, book.astype(np.float64), with_gap=True)
        clear = gap >= 1e-5
        assert (~clear).sum() <= 0.001 * len(x)                               # the fp64 side alone
        code, dist = evaluation.vq(obs, T(book))
        code, dist = code.cpu().numpy(), dist.cpu().numpy()
        assert code.dtype == np.int32 and np.array_equal(code[clear], lab64[clear])
        ok = dist64 > 0
        assert (np.abs(dist[ok] - dist64[ok]) <= 1e-5 * dist64[ok]).all() and (dist[~ok] == 0).all()
    dup = np.concatenate([books[1][:5], books[1][:5], books[1][5:]])          # rows 5..9 repeat rows 0..4: the lower index wins
    code = evaluation.vq(obs, T(dup))[0].cpu().numpy()
    assert not ((code >= 5) & (code < 10)).any() and (code < 5).any()
    lab64 = vq_f64(x, dup.astype(np.float64))[0]
    assert (code == lab64).mean() > 0.999


def _run_script(args, timeout=600):
    r = subprocess.run(['timeout', '-k', '10', str(timeout), sys.executable] + args, capture_output=True, text=True, cwd=UTILS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_entry_script_collision(tmp_path, smplx_data, vposer_sd):
    syn = str(tmp_path / 'syn')
    out = _run_script([os.path.join(UTILS, 'utils_eval_collision_habitat.py'), '--synthetic', syn, '--scenes', 'roomA', 'roomB'])
    coll = float(re.search(r'^--collision_mean=(\S+)$', out, re.M).group(1))
    cont = float(re.search(r'^--contact_mean=(\S+)$', out, re.M).group(1))
    assert np.isfinite([coll, cont]).all() and 0.0 <= coll <= 1.0 and 0.0 <= cont <= 1.0
    # the same tree through eval_folder, one pkl at a time
    sys.path.insert(0, os.path.join(ROOT, 'psi-release_amd', 'source'))
    try:
        import _common
        root, gen, sx, vp = _common.synthetic_prox_tree(syn, ['roomA', 'roomB'], write=False)
    finally:
        sys.path.pop(0)
    cl, kl, allow = [], [], []
    for name in ('roomA', 'roomB'):
        cfg = {'scene_verts_path': os.path.join(root, 'scenes_downsampled', name + '.ply'), 'scene_sdf_path': os.path.join(root, 'scenes_sdf', name),
               'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.1, 'num_iter': 1, 'batch_size': 1, 'device': torch.device(DEV),
               'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False, 'smplx_data': sx, 'vposer_state': vp,
               'engine': 'modular'}
        op = fitting.FittingOPHabitat(cfg, {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 1, 'weight_collision': 1})
        ev = evaluation.PlausibilityEvaluator(op, flip_camera_yz=True)
        c, k = ev.eval_folder(os.path.join(gen, name))
        cl += c
        kl += k
        allow += _folder_allowance(ev, os.path.join(gen, name)).tolist()
    assert len(cl) == 4
    assert abs(coll - np.mean(cl)) * 10475.0 * len(cl) <= sum(allow) + 1e-6, (coll, np.mean(cl), allow)
    if sum(allow) == 0:
        assert cont == np.mean(kl)


def test_entry_script_diversity(tmp_path):
    out = _run_script([os.path.join(UTILS, 'utils_eval_diversity.py'), '--synthetic', str(tmp_path / 'syn'), '--seed', '0'])
    ent = float(re.search(r'^entropy:(\S+)$', out, re.M).group(1))
    md = float(re.search(r'^mean distance:(\S+)$', out, re.M).group(1))
    assert np.isfinite([ent, md]).all() and 0.0 <= ent <= np.log(20.0) + 1e-12 and md > 0.0
