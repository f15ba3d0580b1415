"""The fused fitting engine over SEVERAL scenes (psi_fit_create_scenes): body b of a run is fitted in scene slot[b].

The scenes differ in everything a wrong slot could hide behind — number of points, grid size, extent, radius, kind — and share only
the contact ids, which belong to the body.  The autograd reference is the modular engine over the per-scene HIP operators
(ops.sdf_sample with scene_id, ops.SceneSet), themselves pinned to the oracle in test_hip_ops_gpu.py / test_cvae_glue_gpu.py; it is
anchored here to the single-scene modular engine."""
import ctypes
import dataclasses
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
from psi_release_amd import fitting, hip, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
SRC = os.path.join(ROOT, 'psi-release_amd', 'source')
_cache = {}


def scenes_abc():
    if 'scenes' not in _cache:
        a = synth.make_scene(3, 3000, 24, 300)
        b = dataclasses.replace(synth.make_scene(4, 1777, 16, 300, extent=1.5, radius=0.5), contact_parts=a.contact_parts)
        c = dataclasses.replace(synth.make_scene(5, 2500, 24, 300, kind='sphere'), contact_parts=a.contact_parts)
        _cache['scenes'] = (a, b, c)
    return _cache['scenes']


def make_op(smplx_data, vposer_sd, scenes, B, engine, num_iter=1, align_corners=True, cls=fitting.FittingOP, **extra):
    """scenes: one SceneData (the existing single-scene op) or a list of them."""
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.1, 'num_iter': num_iter, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': smplx_data, 'vposer_state': vposer_sd, 'engine': engine, 'align_corners': align_corners}
    cfg['scenes' if isinstance(scenes, (list, tuple)) else 'scene'] = list(scenes) if isinstance(scenes, (list, tuple)) else scenes
    cfg.update(extra)
    torch.manual_seed(0)
    return cls(cfg, dict(LOSS))


def bodies_of(B, seed=21, cam_seed=7):
    b = synth.make_bodies(seed, B)
    b['cam_ext'] = synth.make_cam_ext(cam_seed, B)
    return b


def modular_first_step(smplx_data, vposer_sd, scenes, B, bodies, slots, align_corners=True):
    """(gradient [B,75], the four losses) of the modular engine's first step."""
    op = make_op(smplx_data, vposer_sd, scenes, B, 'modular', align_corners=align_corners)
    if slots is not None:
        op.set_scene_ids(slots)
    r = op.make_step_runner(dict(bodies))
    r.step()
    return op.xhr_rec.grad.detach().cpu().numpy().copy(), np.array(r.last_losses())


def fused_first_step(smplx_data, vposer_sd, scenes, B, bodies, slots, align_corners=True):
    op = make_op(smplx_data, vposer_sd, scenes, B, 'fused', align_corners=align_corners)
    op.set_scene_ids(slots)
    r = op.make_step_runner(dict(bodies))
    r.step()
    g = op._fused.buffer('adam_m', (B, 75)).cpu().numpy() / 0.1
    assert hip.lib().psi_fit_scene_count(op._fused.handle) == len(scenes)
    return g, np.array(r.last_losses())


# ---- 1. first step against autograd, coupled batch ----------------------------------------------------------------------
def _reference(key, smplx, vposer_sd, align_corners):
    if key not in _cache:
        A, B_, _ = scenes_abc()
        _cache[key] = modular_first_step(smplx, vposer_sd, [A, B_], 3, bodies_of(3), [1, 0, 1], align_corners)
    return _cache[key]


def test_modular_reference_is_anchored_to_the_single_scene_op(smplx_data, vposer_sd):
    """With all slots equal to s the several-scenes modular op IS the single-scene modular op of scene s."""
    A, B_, _ = scenes_abc()
    bodies = bodies_of(3)
    for s, scene in enumerate((A, B_)):
        g1, l1 = modular_first_step(smplx_data, vposer_sd, scene, 3, bodies, None)
        gm, lm = modular_first_step(smplx_data, vposer_sd, [A, B_], 3, bodies, s)
        print('anchor scene %d: gradient rel %.3g, losses rel %.3g' % (s, rel_err(gm, g1), rel_err(lm, l1)))
        assert rel_err(gm, g1) < 1e-6 and rel_err(lm, l1) < 1e-6
    # and the two scenes really are different problems
    assert rel_err(modular_first_step(smplx_data, vposer_sd, [A, B_], 3, bodies, 0)[0], modular_first_step(smplx_data, vposer_sd, [A, B_], 3, bodies, 1)[0]) > 1e-2


@pytest.mark.parametrize('variant', ['default', 'skin_nb2', 'split_scene', 'split_scene_nb2', 'unfused_bwd', 'align_corners0', 'sparse_weights'])
def test_first_step_matches_autograd(smplx_data, vposer_sd, monkeypatch, variant):
    """B = 3 over scenes (A, B), slots [1, 0, 1]: gradient (Adam's first moment / 0.1) and the four loss values of the fused engine's first
    step against autograd over the per-scene operators — the bounds test_full_baseline_size_properties uses for the same comparison.
    skin_nb2: two bodies of DIFFERENT scenes in one workgroup of the scene launch, the third alone; split_scene_nb2: the same pairing in the
    skinning + SDF kernel as a launch of its own."""
    A, B_, _ = scenes_abc()
    env = {'skin_nb2': {'PSI_SKIN_NB': '2'}, 'split_scene': {'PSI_SPLIT_SCENE': '1'}, 'split_scene_nb2': {'PSI_SPLIT_SCENE': '1', 'PSI_SKIN_NB': '2'},
           'unfused_bwd': {'PSI_FIT_FUSED_BWD': '0'}}
    for k, v in env.get(variant, {}).items():
        monkeypatch.setenv(k, v)
    ac = variant != 'align_corners0'
    smplx = synth.make_smplx(7, weight_nnz=4) if variant == 'sparse_weights' else smplx_data
    g_ref, l_ref = _reference(('ref', ac, variant == 'sparse_weights'), smplx, vposer_sd, ac)
    g, l = fused_first_step(smplx, vposer_sd, [A, B_], 3, bodies_of(3), [1, 0, 1], ac)
    print('%s: gradient rel_err %.3g, loss abs err %s' % (variant, rel_err(g, g_ref), np.abs(l - l_ref)))
    assert rel_err(g, g_ref) < 1e-4
    assert np.abs(l - l_ref).max() < 1e-5


# ---- 2. bodies keep to their own scene -----------------------------------------------------------------------------------
def test_independent_bodies_keep_to_their_own_scene(smplx_data, vposer_sd):
    """independent_bodies, B = 5 over scenes (A, B, C), slots [2, 0, 2, 1, 0], 8 iterations: row b equals row b of the SINGLE-scene engine
    (psi_fit_create) run on the same five bodies in scene slot[b] (bound of test_packed_independent_bodies_equal_one_by_one_fits); against the
    runs of the slots rotated by one the rows differ."""
    scenes = list(scenes_abc())
    B, slots = 5, np.array([2, 0, 2, 1, 0])
    bodies = bodies_of(B, 60, 60)
    bodies['transl'] = (bodies['transl'] * np.arange(1, B + 1)[:, None]).astype(np.float32)      # different amounts of penetration per body
    single = []
    for sc in scenes:
        op = make_op(smplx_data, vposer_sd, sc, B, 'fused', num_iter=8, independent_bodies=True)
        single.append(op.fitting(dict(bodies)).detach().cpu().numpy().copy())
        assert hip.lib().psi_fit_scene_count(op._fused.handle) == 1
    op = make_op(smplx_data, vposer_sd, scenes, B, 'fused', num_iter=8, independent_bodies=True)
    multi = op.fitting(dict(bodies), scene_id=slots).detach().cpu().numpy()
    want = np.stack([single[slots[b]][b] for b in range(B)])
    wrong = np.stack([single[(slots[b] + 1) % 3][b] for b in range(B)])
    d = np.abs(multi - want).max()
    print('several scenes vs single-scene engines: max abs %.3g, bit-exact: %s' % (d, np.array_equal(multi, want)))
    assert d < 2e-5
    assert np.abs(multi - wrong).max() > 1e-3


ONE_SCENE_ARMS = {'default': {}, 'skin_nb2': {'PSI_SKIN_NB': '2'}, 'split_scene': {'PSI_SPLIT_SCENE': '1'},
                  'split_scene_nb2': {'PSI_SPLIT_SCENE': '1', 'PSI_SKIN_NB': '2'}}


@pytest.mark.parametrize('arm', list(ONE_SCENE_ARMS))
def test_table_of_one_scene_equals_the_single_scene_engine(smplx_data, vposer_sd, monkeypatch, arm):
    """A several-scenes engine (psi_fit_create_scenes) over a table of ONE scene, A, against the psi_fit_create engine of A: the same B = 3
    bodies, independent_bodies, 4 iterations, both engines built under the arm's knobs.  The two run the same scene stage, with the scene
    selected per body or taken from the kernel arguments, so they agree bit for bit: all four arms were bit-equal (np.array_equal) when the
    two forms of the stage were still separate kernels, which is where this bound comes from."""
    A = scenes_abc()[0]
    for k, v in ONE_SCENE_ARMS[arm].items():
        monkeypatch.setenv(k, v)
    B = 3
    bodies = bodies_of(B, 60, 60)
    op1 = make_op(smplx_data, vposer_sd, A, B, 'fused', num_iter=4, independent_bodies=True)
    single = op1.fitting(dict(bodies)).detach().cpu().numpy().copy()
    assert op1._fused.n_scenes == 0
    opS = make_op(smplx_data, vposer_sd, [A], B, 'fused', num_iter=4, independent_bodies=True, scene_table_engine=True)
    table = opS.fitting(dict(bodies), scene_id=0).detach().cpu().numpy()
    assert opS._fused.n_scenes == 1
    d = np.abs(table - single).max()
    print('%s: table of one scene vs single-scene engine: max abs %.3g, bit-exact: %s' % (arm, d, np.array_equal(table, single)))
    assert np.isfinite(single).all()
    assert np.array_equal(table, single)


# ---- 3. slots change under captured graphs ------------------------------------------------------------------------------
def test_slots_change_under_captured_graphs(smplx_data, vposer_sd):
    """The slots live in an engine-owned buffer: the graphs captured with slots X are replayed after psi_fit_set_scene_slots(Y) and give
    what a fresh engine that only ever had slots Y gives, bit for bit."""
    scenes = list(scenes_abc())
    B, X, Y = 3, [1, 0, 2], [2, 1, 0]
    bodies = bodies_of(B)

    def fresh(slots):
        op = make_op(smplx_data, vposer_sd, scenes, B, 'fused', num_iter=12)
        op.reset_optimizer, op.use_graph = True, True
        return op, op.fitting(dict(bodies), scene_id=slots).detach().cpu().numpy().copy()

    op, x_first = fresh(X)
    x_second = op.fitting(dict(bodies), scene_id=Y).detach().cpu().numpy().copy()      # slots, then set_problem with reset, then 12 iterations
    _, y1 = fresh(Y)
    _, y2 = fresh(Y)
    assert np.array_equal(y1, y2)
    assert np.array_equal(x_second, y1)
    assert not np.array_equal(x_first, y1)


# ---- 4. large-batch structure --------------------------------------------------------------------------------------------
def test_large_batch_structure_matches_autograd(smplx_data, vposer_sd):
    """B = 130: the skinning + SDF kernel and the NN search as separate launches, two bodies (of different scenes) per skinning workgroup
    with dense rows, the contact rows in slot order."""
    A, B_, _ = scenes_abc()
    B = 130
    slots = np.arange(B) % 2
    bodies = bodies_of(B)
    g_ref, l_ref = modular_first_step(smplx_data, vposer_sd, [A, B_], B, bodies, slots)
    g, l = fused_first_step(smplx_data, vposer_sd, [A, B_], B, bodies, slots)
    print('B=130: gradient rel_err %.3g, loss abs err %s' % (rel_err(g, g_ref), np.abs(l - l_ref)))
    assert rel_err(g, g_ref) < 1e-4


# ---- 5. argument errors -------------------------------------------------------------------------------------------------
def test_create_scenes_argument_errors(smplx_data, vposer_sd):
    A, B_, _ = scenes_abc()
    op = make_op(smplx_data, vposer_sd, [A, B_], 2, 'fused')
    bm = op.body_mesh_model
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    sd = {k: f32(v.detach().cpu().numpy()) for k, v in op.vposer.state_dict().items() if 'dec' in k}
    host = [sd['bodyprior_dec_fc1.weight'], sd['bodyprior_dec_fc1.bias'], sd['bodyprior_dec_fc2.weight'], sd['bodyprior_dec_fc2.bias'],
            sd['bodyprior_dec_out.weight'], sd['bodyprior_dec_out.bias'], f32(bm.left_hand_components.cpu().numpy()),
            f32(bm.right_hand_components.cpu().numpy()), f32(bm.pose_mean.cpu().numpy()),
            np.ascontiguousarray(op.contact_vertex_ids().cpu().numpy(), dtype=np.int32)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L = hip.lib()

    def table(D_of=None, null_verts=False):
        arr = (hip.FitScene * 2)()
        for i, (s_, sc) in enumerate(zip(arr, op._scene_tab)):
            s_.d_verts, s_.d_sdf, s_.m, s_.D = (None if null_verts and i == 1 else hip.ptr(sc['verts'])), hip.ptr(sc['sdf']), sc['verts'].shape[0], sc['sdf'].shape[0]
            if D_of is not None and i == 1:
                s_.D = D_of
            s_.gmin[:], s_.gmax[:] = [float(v) for v in sc['gmin']], [float(v) for v in sc['gmax']]
        return arr

    def create(arr, S, **over):
        kw = dict(B=2, n_contact=len(host[-1]), m_scene=0, D=0, align_corners=1, world_size=1, num_pca_comps=12, max_history=64, nn_mode=1,
                  w_rec=1.0, w_vposer=0.01, w_contact=0.1, w_collision=0.5, contact_const=0.01, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8)
        kw.update(over)
        cfg = hip.FitConfig(**kw)
        h = ctypes.c_void_p()
        rc = L.psi_fit_create_scenes(ctypes.byref(h), bm.lbs_model.handle, ctypes.byref(cfg), *[p(a) for a in host], arr, S)
        return rc, h

    cases = {'S < 1': (table(), 0, {}), 'null scene table': (None, 2, {}), 'null scene pointer': (table(null_verts=True), 2, {}),
             'brute-force search': (table(), 2, {'nn_mode': 0}), 'D % 4 != 0': (table(D_of=18), 2, {}), 'D > 480': (table(D_of=484), 2, {}),
             'world_size > 1': (table(), 2, {'world_size': 2})}
    for name, (arr, S, over) in cases.items():
        rc, h = create(arr, S, **over)
        msg = hip.last_error()
        print('%s -> %d: %s' % (name, rc, msg))
        assert rc == -22 and not h.value and len(msg) > 10, name
    rc, h = create(table(), 2)                 # (and the table itself is fine)
    assert rc == 0 and h.value and L.psi_fit_scene_count(h) == 2
    torch.cuda.synchronize()
    L.psi_fit_destroy(h)
    single = fitting.FusedEngine(make_op(smplx_data, vposer_sd, A, 2, 'fused'))
    assert L.psi_fit_scene_count(single.handle) == 1


def test_contact_parts_must_agree(smplx_data, vposer_sd):
    A = scenes_abc()[0]
    other = synth.make_scene(4, 1777, 16, 300, extent=1.5, radius=0.5)          # its own contact ids
    with pytest.raises(ValueError):
        make_op(smplx_data, vposer_sd, [A, other], 2, 'fused')
    op = make_op(smplx_data, vposer_sd, list(scenes_abc()), 2, 'fused')
    with pytest.raises(ValueError):
        op.set_scene_ids([0, 3])


# ---- 6. entry point -------------------------------------------------------------------------------------------------------
def test_fitting_habitat_across_scenes(tmp_path):
    """--pack 4 --across_scenes (one FittingOP over the three rooms, their six files packed into two runs) writes the files that the per-room
    loop with --pack 4 --reset_optimizer writes."""
    names = ['roomA', 'roomB', 'roomC']
    syn = str(tmp_path / 'syn')
    sys.path.insert(0, SRC)
    try:
        import _common as C
        C.synthetic_prox_tree(syn, names)
    finally:
        sys.path.remove(SRC)
    outs = {}
    for tag, flags in (('loop', ['--reset_optimizer']), ('across', ['--across_scenes'])):
        fit = str(tmp_path / ('fit_' + tag))
        r = subprocess.run([sys.executable, os.path.join(SRC, 'fitting_habitat.py'), fit, '--synthetic', syn, '--scenes'] + names +
                           ['--num_iter', '8', '--pack', '4'] + flags, capture_output=True, text=True, timeout=600, cwd=SRC)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[tag] = {os.path.relpath(f, fit): f for f in sorted(glob.glob(os.path.join(fit, '*', 'body_gen_*.pkl')))}
    assert sorted(outs['loop']) == sorted(outs['across']) and len(outs['loop']) == 6
    worst = 0.0
    for rel in outs['loop']:
        with open(outs['loop'][rel], 'rb') as f1, open(outs['across'][rel], 'rb') as f2:
            a, b = pickle.load(f1), pickle.load(f2)
        assert set(a) == set(b)
        for k in a:
            worst = max(worst, float(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).max()))
    print('across scenes vs per-room loop: max abs %.3g' % worst)
    assert worst < 2e-5
