"""GPU parity of the fitting loop (FittingOP) against the trajectory recorded from the reference's own FittingOP
(tests/golden/fitting_proxe.npz, made by oracle/make_golden.py) and against the oracle at other settings."""
import dataclasses

import numpy as np
import pytest
import torch

import arbiter
import per_body
import psi_oracle as O
from conftest import golden, rel_err
from psi_release_amd import fitting, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}


def make_op(smplx_data, vposer_sd, scene, B, engine, num_iter=5, align_corners=True, cls=fitting.FittingOP, lr=0.1):
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': lr, 'num_iter': num_iter, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': smplx_data, 'vposer_state': vposer_sd, 'scene': scene, 'engine': engine,
           'align_corners': align_corners}
    torch.manual_seed(0)
    return cls(cfg, dict(LOSS))


@pytest.mark.parametrize('engine', ['modular'])
@pytest.mark.parametrize('tag', ['ac1', 'ac0'])
def test_cal_loss_and_gradient_golden(smplx_data, vposer_sd, engine, tag):
    g = golden('fitting_proxe')
    B, m, n_c, D = int(g['B']), int(g['m']), int(g['n_c']), int(g['D'])
    scene = synth.make_scene(0, m, D, n_c)
    op = make_op(smplx_data, vposer_sd, scene, B, engine, align_corners=(tag == 'ac1'))
    assert np.array_equal(op.contact_vertex_ids().cpu().numpy(), g['contact_ids'])
    op.xhr_rec.data = T(g['xhr_rec0_' + tag])
    losses = op.cal_loss(T(g['xhr_' + tag]), T(g['cam_ext']))
    got = np.array([float(l) for l in losses])
    assert rel_err(got, g['loss0_' + tag]) < 1e-4
    assert np.abs(got - g['loss0_' + tag]).max() < 1e-5
    sum(losses).backward()
    assert rel_err(op.xhr_rec.grad.cpu(), g['grad0_' + tag]) < 1e-4
    if tag == 'ac1':
        xh = fitting.GeometryTransformer.convert_to_3D_rot(op.xhr_rec)
        v = op.body_verts(xh, T(g['cam_ext']))
        assert rel_err(v.detach().cpu(), g['verts0']) < 1e-4


@pytest.mark.parametrize('engine', ['modular', 'fused'])
@pytest.mark.parametrize('tag', ['ac1', 'ac0'])
def test_five_iteration_trajectory_golden(smplx_data, vposer_sd, engine, tag, capsys):
    g = golden('fitting_proxe')
    B, m, n_c, D = int(g['B']), int(g['m']), int(g['n_c']), int(g['D'])
    scene = synth.make_scene(0, m, D, n_c)
    op = make_op(smplx_data, vposer_sd, scene, B, engine, align_corners=(tag == 'ac1'))
    op.verbose = True
    bodies = synth.make_bodies(11, B)
    bodies['cam_ext'] = g['cam_ext']
    xh = op.fitting(bodies)
    out = capsys.readouterr().out
    rec = []
    for line in out.splitlines():
        if line.startswith('[INFO][fitting] iter='):
            rec.append([float(tok.split('=')[1]) for tok in line.split(', ')[1:]])
    rec = np.array(rec)
    assert rec.shape == (5, 4)
    assert np.abs(rec - g['traj_loss_' + tag]).max() < 2e-5          # printed with 6 decimals
    assert rel_err(op.xhr_rec.detach().cpu(), g['traj_final_xhr_' + tag]) < 1e-4
    assert np.abs(xh.detach().cpu().numpy() - g['traj_final_' + tag]).max() < 1e-3


@pytest.mark.parametrize('tag', ['ac1', 'ac0'])
def test_fused_engine_losses_and_first_gradient(smplx_data, vposer_sd, tag):
    """Fused engine at the golden perturbed point: loss values, body vertices and d(loss)/d(verts)-driven first Adam
    step agree with the reference (loss0 / verts0 / grad0 of tests/golden/fitting_proxe.npz)."""
    g = golden('fitting_proxe')
    B, m, n_c, D = int(g['B']), int(g['m']), int(g['n_c']), int(g['D'])
    scene = synth.make_scene(0, m, D, n_c)
    op = make_op(smplx_data, vposer_sd, scene, B, 'fused', align_corners=(tag == 'ac1'))
    eng = fitting.FusedEngine(op)
    x0 = T(g['xhr_rec0_' + tag])
    eng.set_problem(T(g['xhr_' + tag]), x0, T(g['cam_ext']), reset=True)
    eng.iterate(1, use_graph=False)
    x1, hist, step = eng.read(1)
    assert step == 1
    assert np.abs(hist[0].cpu().numpy() - g['loss0_' + tag]).max() < 1e-5
    if tag == 'ac1':
        assert rel_err(eng.buffer('verts', (B, 10475, 3)).cpu(), g['verts0']) < 1e-4
    # first Adam step from zero state: x1 = x0 - lr * g/(|g| + eps*sqrt-terms)  =>  recover sign and size of g
    m1 = eng.buffer('adam_m', (B, 75)).cpu().numpy() / 0.1            # m = (1-beta1) g
    assert rel_err(m1, g['grad0_' + tag]) < 2e-4
    gref = g['grad0_' + tag]
    expect = g['xhr_rec0_' + tag] - 0.1 * gref / (np.abs(gref) + 1e-8)
    big = np.abs(gref) > 1e-6
    assert np.abs(x1.cpu().numpy() - expect)[big].max() < 1e-4


@pytest.mark.parametrize('B,cls,lr,graph', [(3, fitting.FittingOP, 0.05, True), (1, fitting.FittingOPHabitat, 0.1, True),
                                           (6, fitting.FittingOP, 0.1, False)])
def test_fused_matches_modular(smplx_data, vposer_sd, B, cls, lr, graph):
    """Same trajectory from the hand-derived fused backward and from autograd over the HIP operators (random camera,
    other batch sizes, Habitat variant: contact constant 1.0 + flipped camera).  Horizon 3 iterations: Adam's
    normalised steps make the loop chaotic (a 3e-7 gradient difference grows ~5x per iteration and jumps when a
    vertex crosses the sdf<0 mask or switches nearest neighbour), so longer horizons only measure that."""
    scene = synth.make_scene(3, 3000, 24, 300)
    bodies = synth.make_bodies(21, B)
    bodies['cam_ext'] = synth.make_cam_ext(7, B)
    res = {}
    for engine in ('modular', 'fused'):
        op = make_op(smplx_data, vposer_sd, scene, B, engine, num_iter=3, cls=cls, lr=lr)
        op.use_graph = graph
        xh = op.fitting(dict(bodies))
        res[engine] = (xh.detach().cpu().numpy(), op.xhr_rec.detach().cpu().numpy())
    assert np.abs(res['fused'][1] - res['modular'][1]).max() < 2e-4
    assert np.abs(res['fused'][0] - res['modular'][0]).max() < 1e-3


@pytest.mark.parametrize('B', [40, 64, 136, 137])     # 136 / 137: the large-batch kernels (B >= 128); 137 is odd: two-body skinning workgroups with a ragged last pair
def test_fused_gradient_matches_modular_large_batch(smplx_data, vposer_sd, B):
    """B > 32 selects the 4-row-tile MFMA variants (blend_fwd<4>, bwd_joint<4>).  Compared on the FIRST-iteration gradient
    (Adam's first moment after one step = 0.1 * gradient in both engines): with 1/B normalisers some elements have
    |g| < 1e-8 ~ Adam's eps, so trajectories differ by the eps-sensitivity of those elements even for gradients that
    agree to 1e-7."""
    scene = synth.make_scene(3, 3000, 24, 300)
    bodies = synth.make_bodies(21, B)
    bodies['cam_ext'] = synth.make_cam_ext(7, B)
    g = {}
    for engine in ('modular', 'fused'):
        op = make_op(smplx_data, vposer_sd, scene, B, engine, num_iter=1, lr=0.05)
        op.fitting(dict(bodies))
        g[engine] = (op._fused.buffer('adam_m', (B, 75)) if engine == 'fused' else op.optimizer.state[op.xhr_rec]['exp_avg']).detach().cpu().numpy() * 10
    d = np.abs(g['fused'] - g['modular'])
    if B <= 64:
        assert d.max() < 2e-6 and d.max() < 1e-4 * np.abs(g['modular']).max(), (d.max(), np.abs(g['modular']).max())
        return
    # B >= 128 (large-batch skinning kernels, separate statistics kernel): both engines against the ORACLE's autograd gradient by the rules
    # of tests/arbiter.py — per body within 1e-4 of the largest entry of the fp32 oracle's gradient, or no further from the fp64 arbiter than
    # 4 x the fp32 oracle itself is, or (a body holding a vertex whose SDF value is within fp32 rounding of zero: with ~4e5 penetrating
    # vertices one vertex counted the other way is 2e-4 of the gradient scale) the same against the oracle with those vertices counted in / out
    make = lambda dt: O.FittingOracle(O.SMPLXOracle(smplx_data, dtype=dt), vposer_sd, scene.verts, scene.sdf, scene.grid_min, scene.grid_max,
                                      synth.contact_ids_from_parts(scene.contact_parts), B)
    xhr = O.convert_to_6d_rot(torch.tensor(synth.body_vector_72(bodies))).numpy().astype(np.float64)   # the loop starts AT the target
    f32, f64 = make(torch.float32), make(torch.float64)
    for k in g:
        _, info = arbiter.check_gradient(g[k].astype(np.float64), f32, f64, xhr, xhr, np.asarray(bodies['cam_ext'], np.float64))
        arbiter.record('fused_vs_modular_gradient_B%d_%s' % (B, k), info)
    assert np.median(np.abs(d).max(axis=1)) < 1e-5 * np.abs(g['modular']).max()


def test_nn_modes_agree(smplx_data, vposer_sd, monkeypatch):
    """kd-tree index and brute-force Chamfer give the same fitting step in both engines (they are bit-identical ops): bit for bit where the
    rest of the iteration is the same sequence of kernels (PSI_FIT_FUSED_BWD=0: the per-vertex backward launch, which the brute-force mode
    always uses), to fp32 rounding against the default kd-tree iteration, whose skinning backward rides on the forward launch and carries the
    penetration and contact parts of the gradient separately up to the sums of the split contractions (fit.hip: fit_bwd_joint_kernel)."""
    scene = synth.make_scene(3, 3000, 16, 300)
    B = 3
    bodies = synth.make_bodies(41, B)
    out = {}
    for engine in ('fused', 'modular'):
        for mode in ('kdtree', 'bruteforce') + (('kdtree_unfused',) if engine == 'fused' else ()):
            monkeypatch.setenv('PSI_FIT_FUSED_BWD', '0' if mode == 'kdtree_unfused' else '1')
            op = make_op(smplx_data, vposer_sd, scene, B, engine, num_iter=2)
            op.nn_mode = mode.split('_')[0]
            op.fitting(dict(bodies))
            out[(engine, mode)] = op.xhr_rec.detach().cpu().numpy()
    assert np.array_equal(out[('fused', 'kdtree_unfused')], out[('fused', 'bruteforce')])
    assert np.abs(out[('fused', 'kdtree')] - out[('fused', 'bruteforce')]).max() < 1e-4   # two Adam steps of 0.1: entries with near-zero gradients amplify the rounding
    assert np.abs(out[('modular', 'kdtree')] - out[('modular', 'bruteforce')]).max() < 1e-6


def test_fused_adam_state_persists_and_resets(smplx_data, vposer_sd):
    """fitting_proxe.py:74,175: the optimizer is created once and reused for every file."""
    scene = synth.make_scene(3, 2000, 16, 200)
    B = 2
    outs = {}
    for engine in ('modular', 'fused'):
        op = make_op(smplx_data, vposer_sd, scene, B, engine, num_iter=2)
        a = op.fitting(synth.make_bodies(31, B))
        b = op.fitting(synth.make_bodies(32, B))          # second file: Adam moments carried over
        outs[engine] = (a.detach().cpu().numpy(), b.detach().cpu().numpy())
    assert np.abs(outs['fused'][0] - outs['modular'][0]).max() < 1e-3
    assert np.abs(outs['fused'][1] - outs['modular'][1]).max() < 1e-3


def test_full_baseline_size_properties(smplx_data, vposer_sd, monkeypatch):
    """BASELINE shape (B=32, n_c=2048, m=32768, SDF 256^3): the oracle needs seconds per iteration here, so parity is shown
    through properties: (1) the hand-derived fused backward equals autograd over the HIP operators for the first step
    (gradient recovered from Adam's first moment), (2) kd-tree and brute-force NN give bit-identical parameters behind the same backward
    kernels (PSI_FIT_FUSED_BWD=0) and the default iteration (skinning backward inside the forward launch) the same first gradient to fp32
    rounding, (3) graph replay equals eager launches, (4) the objective decreases over 20 iterations."""
    B = 32
    scene = synth.make_scene(0, 32768, 256, 2048)
    bodies = synth.make_bodies(11, B)
    bodies['cam_ext'] = synth.make_cam_ext(5, B)
    opm = make_op(smplx_data, vposer_sd, scene, B, 'modular', num_iter=1)
    rm = opm.make_step_runner(dict(bodies))
    rm.step()
    g_mod = opm.xhr_rec.grad.detach().cpu().numpy()
    res = {}
    for mode, graph in (('kdtree', True), ('bruteforce', True), ('kdtree', False), ('kdtree_unfused', True)):
        monkeypatch.setenv('PSI_FIT_FUSED_BWD', '0' if mode == 'kdtree_unfused' else '1')
        op = make_op(smplx_data, vposer_sd, scene, B, 'fused', num_iter=1)
        op.nn_mode, op.use_graph = mode.split('_')[0], graph
        r = op.make_step_runner(dict(bodies))
        r.step()
        m1 = op._fused.buffer('adam_m', (B, 75)).cpu().numpy() / 0.1
        l0 = r.last_losses()
        for _ in range(19):
            r.step()
        r.finish()
        res[(mode, graph)] = (m1, op.xhr_rec.detach().cpu().numpy(), l0, r.last_losses())
    m1 = res[('kdtree', True)][0]
    assert rel_err(m1, g_mod) < 1e-4
    assert np.array_equal(res[('kdtree_unfused', True)][1], res[('bruteforce', True)][1])
    assert rel_err(m1, res[('bruteforce', True)][0]) < 2e-6
    assert rel_err(res[('kdtree_unfused', True)][0], g_mod) < 1e-4
    assert np.array_equal(res[('kdtree', True)][1], res[('kdtree', False)][1])
    l0, l19 = res[('kdtree', True)][2], res[('kdtree', True)][3]
    assert abs(sum(l0) - sum(rm.last_losses())) < 1e-5
    assert l19[2] + l19[3] < l0[2] + l0[3]                      # contact + collision terms go down


def test_long_graph_equals_single_iteration_graphs(smplx_data, vposer_sd):
    """psi_fit_iterate(23) = 2 replays of the 10-iteration graph + 3 single-iteration replays; bit-identical to 23 calls of
    psi_fit_iterate(1) (the iteration has no host-side state), including the recorded loss history."""
    scene = synth.make_scene(3, 3000, 24, 300)
    B = 3
    bodies = synth.make_bodies(21, B)
    bodies['cam_ext'] = synth.make_cam_ext(7, B)
    res = {}
    for mode in ('one_call', 'per_iteration'):
        op = make_op(smplx_data, vposer_sd, scene, B, 'fused', num_iter=23, lr=0.05)
        runner = op.make_step_runner(dict(bodies))
        if mode == 'one_call':
            runner.steps(23)
        else:
            for _ in range(23):
                runner.step()
        losses = runner.last_losses()
        runner.finish()
        res[mode] = (op.xhr_rec.detach().cpu().numpy().copy(), np.array(losses))
    assert np.array_equal(res['one_call'][0], res['per_iteration'][0])
    assert np.array_equal(res['one_call'][1], res['per_iteration'][1])


def test_fitting_many_equals_sequential_fits(smplx_data, vposer_sd):
    """FittingOP.fitting_many (independent files in flight on separate engines / streams) returns, file by file, exactly what
    sequential fitting() calls with a fresh Adam state return."""
    scene = synth.make_scene(3, 3000, 24, 300)
    files = []
    for i in range(7):
        b = synth.make_bodies(40 + i, 1)
        b['cam_ext'] = synth.make_cam_ext(40 + i, 1)
        files.append(b)
    op = make_op(smplx_data, vposer_sd, scene, 1, 'fused', num_iter=12, cls=fitting.FittingOPHabitat)
    op.reset_optimizer = True
    seq = [op.fitting(dict(f)).detach().clone() for f in files]
    op2 = make_op(smplx_data, vposer_sd, scene, 1, 'fused', num_iter=12, cls=fitting.FittingOPHabitat)
    many, cams = op2.fitting_many([dict(f) for f in files], concurrency=3)
    assert len(many) == 7 and len(op2._fused_pool) == 3
    for a, b_, f, (ce, ci) in zip(seq, many, files, cams):
        assert torch.equal(a, b_)
        assert np.array_equal(ce.cpu().numpy(), f['cam_ext'])


@pytest.mark.parametrize('cls', [fitting.FittingOP, fitting.FittingOPHabitat])
def test_packed_independent_bodies_equal_one_by_one_fits(smplx_data, vposer_sd, cls):
    """independent_bodies: an engine run over B bodies with per-body loss normalisers == B runs of the loop at batch size 1 (one
    generated-body file each) — the penetration mean, the contact mean and the reconstruction / prior means are per body, so 7
    files packed 5 per run (the second run padded) give the same fitted bodies as 7 sequential fits."""
    scene = synth.make_scene(3, 3000, 24, 300)
    files = []
    for i in range(7):
        b = synth.make_bodies(60 + i, 1)
        b['cam_ext'] = synth.make_cam_ext(60 + i, 1)
        b['transl'] = (b['transl'] * (1.0 + i)).astype(np.float32)            # different amounts of penetration per file
        files.append(b)
    one = make_op(smplx_data, vposer_sd, scene, 1, 'fused', num_iter=8, cls=cls)
    one.reset_optimizer = True
    seq = [one.fitting(dict(f)).detach().cpu().numpy() for f in files]
    cfg_op = make_op(smplx_data, vposer_sd, scene, 5, 'fused', num_iter=8, cls=cls)
    cfg_op.independent_bodies = True
    packed, _ = cfg_op.fitting_many([dict(f) for f in files], concurrency=2)
    assert len(packed) == 7
    for a, b_ in zip(seq, packed):
        assert b_.shape == (1, 72)
        assert np.abs(a - b_.detach().cpu().numpy()).max() < 2e-5
    # and the coupled (reference batch semantics) engine really differs on the same stack of bodies
    coupled = make_op(smplx_data, vposer_sd, scene, 5, 'fused', num_iter=8, cls=cls)
    stack = {k: np.concatenate([f[k] for f in files[:5]]) for k in files[0]}
    xc = coupled.fitting(stack).detach().cpu().numpy()
    assert np.abs(xc - np.concatenate(seq[:5])).max() > 1e-3


def test_head_cluster_widths_agree_and_repeat_exactly(smplx_data, vposer_sd, monkeypatch):
    """The per-body head / tail kernels spread a body over 1, 2, 4 or 8 workgroups that exchange partial sums inside the launch
    (fit.hip: tagged 64-bit words, summed in cluster order).  Every width must (a) repeat bit-for-bit from run to run over a long
    fit — a stale or torn exchange word would show up as run-to-run differences — and (b) agree with the single-workgroup kernel up
    to the fp32 re-association of the split sums (compared after 3 iterations: Adam's normalised steps amplify last-bit differences
    over a long trajectory).  B = 5, so that clusters straddle XCDs."""
    scene = synth.make_scene(3, 3000, 24, 300)
    B = 5
    bodies = synth.make_bodies(33, B)
    bodies['cam_ext'] = synth.make_cam_ext(9, B)
    short = {}
    for hc in (1, 2, 4, 8):
        monkeypatch.setenv('PSI_HEAD_CLUSTER', str(hc))
        runs = []
        for rep in range(3):
            op = make_op(smplx_data, vposer_sd, scene, B, 'fused', num_iter=40, lr=0.05)
            runs.append(op.fitting(dict(bodies)).detach().cpu().numpy().copy())
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), 'width %d is not repeatable' % hc
        op = make_op(smplx_data, vposer_sd, scene, B, 'fused', num_iter=3, lr=0.05)
        short[hc] = op.fitting(dict(bodies)).detach().cpu().numpy().copy()
    for hc in (2, 4, 8):
        assert np.abs(short[hc] - short[1]).max() < 1e-4, (hc, np.abs(short[hc] - short[1]).max())



@pytest.mark.parametrize('B', [3, 32])
def test_fused_backward_with_duplicate_contact_vertices(smplx_data, vposer_sd, B, monkeypatch):
    """The skinning backward inside fwd_scene (fit.hip: fused_bwd) on a contact list as cvae.py:99-115 builds it — per part ``list(set(.))``,
    parts concatenated, so a vertex that two parts list has TWO slots (duplicates kept) — and a slot count that does not fill its last
    256-slot slice (the padding slots must stay zero rows of the contact class).  Checked: the first-iteration gradient against autograd over
    the HIP operators (the modular engine), and the reduced joint-transform / blend-shape-feature / translation gradients against the same
    engine with the per-vertex backward as its own launch (PSI_FIT_FUSED_BWD=0), which adds the two parts per vertex before the contractions."""
    scene = synth.make_scene(5, 3000, 24, 300)
    parts = {k: dict(v) for k, v in scene.contact_parts.items()}
    names = list(parts)
    shared = parts[names[0]]['verts_ind'][:17]                       # 17 vertices listed by two parts, 5 of them by three
    parts[names[1]] = dict(parts[names[1]], verts_ind=parts[names[1]]['verts_ind'] + shared)
    parts[names[4]] = dict(parts[names[4]], verts_ind=parts[names[4]]['verts_ind'] + shared[:5])
    scene = dataclasses.replace(scene, contact_parts=parts)
    ids = synth.contact_ids_from_parts(parts)
    assert len(ids) == 322 and len(set(ids.tolist())) == 300
    bodies = synth.make_bodies(23, B)
    bodies['cam_ext'] = synth.make_cam_ext(9, B)
    g, buf = {}, {}
    for mode in ('modular', 'fused', 'unfused'):
        monkeypatch.setenv('PSI_FIT_FUSED_BWD', '0' if mode == 'unfused' else '1')
        op = make_op(smplx_data, vposer_sd, scene, B, 'modular' if mode == 'modular' else 'fused', num_iter=1, lr=0.05)
        assert np.array_equal(op.contact_vertex_ids().cpu().numpy(), ids)
        op.fitting(dict(bodies))
        g[mode] = (op._fused.buffer('adam_m', (B, 75)) if mode != 'modular' else op.optimizer.state[op.xhr_rec]['exp_avg']).detach().cpu().numpy() * 10
        if mode != 'modular':
            buf[mode] = {k: op._fused.buffer(k, s).cpu().numpy() for k, s in (('gA', (B, 64, 16)), ('gfeat', (B, 512)), ('g_transl', (B, 3)))}
    scale = np.abs(g['modular']).max()
    assert np.abs(g['fused'] - g['modular']).max() < 1e-5 * scale, np.abs(g['fused'] - g['modular']).max() / scale
    assert np.abs(g['unfused'] - g['modular']).max() < 1e-5 * scale
    for k in buf['fused']:
        ref = buf['unfused'][k]
        assert np.abs(buf['fused'][k] - ref).max() <= 2e-6 * np.abs(ref).max(), (k, np.abs(buf['fused'][k] - ref).max() / np.abs(ref).max())


def test_fused_blend_backward_is_in_the_fp32_accuracy_class(smplx_data, vposer_sd):
    """fit_bwd_joint_kernel multiplies the gradient rows with the blend-shape matrix on the fp16 matrix pipe (two fp16 parts per operand,
    lbs_joint_device.h: blend_bwd_h_body).  From the engine's own operands (g_vposed of both classes, the global penetration count) the
    reduced feature gradient is recomputed in fp64 and, for the distance a plain fp32 product has from that, in fp32: the engine must be
    as close to fp64 as the fp32 product is (K = 4, the arbiter's constant) — not merely within the 1e-4 of the parity bar."""
    B = 32
    scene = synth.make_scene(5, 3000, 24, 300)
    bodies = synth.make_bodies(23, B)
    bodies['cam_ext'] = synth.make_cam_ext(9, B)
    op = make_op(smplx_data, vposer_sd, scene, B, 'fused', num_iter=1, lr=0.05)
    op.fitting(dict(bodies))
    V, K = 10475, 506
    ids = op.contact_vertex_ids().cpu().numpy()
    n_c = len(ids)
    ncp3 = 3 * ((n_c + 255) // 256 * 256)
    Npad = 3 * ((V + 255) // 256 * 256)
    eng = op._fused
    gvp = eng.buffer('g_vp', (B, Npad)).cpu().numpy()[:, :3 * V]
    gvpc = eng.buffer('gvpc', (B, ncp3)).cpu().numpy()[:, :3 * n_c]
    gfeat = eng.buffer('gfeat', (B, 512)).cpu().numpy()[:, :K]
    stats = eng.buffer('stats', (8,)).cpu().numpy()
    m = O.SMPLXOracle(smplx_data)
    D = np.concatenate([m.shapedirs.numpy().reshape(3 * V, -1).T, m.posedirs.numpy()], 0)          # [506][3 V] fp32 values
    assert D.shape == (K, 3 * V) and stats[4] > 0 and np.abs(gvp).max() > 0 and np.abs(gvpc).max() > 0
    cols = (3 * ids[:, None] + np.arange(3)[None]).reshape(-1)
    sp = np.float32(-LOSS['weight_collision']) / np.float32(stats[4])
    ref = float(sp) * (gvp.astype(np.float64) @ D.T.astype(np.float64)) + gvpc.astype(np.float64) @ D[:, cols].T.astype(np.float64)
    r32 = sp * (gvp @ D.T) + gvpc @ D[:, cols].T
    scale = np.abs(ref).max(1, keepdims=True)
    d_prod, d_f32 = (np.abs(gfeat - ref) / scale).max(), (np.abs(r32 - ref) / scale).max()
    assert d_prod <= 4.0 * d_f32 + 2e-7, (d_prod, d_f32)


# ---- one steep body in a batch: the fp16 split products of the fused blend backward take a scale PER BODY -----------------------------
STEEP_X0 = 1.0          # the room's SDF is multiplied by 1e10 at grid points with x > STEEP_X0 (all of them are inside the wall)


def _steep_scene():
    """synth's room with its SDF multiplied by 1e10 on the x > STEEP_X0 side: a body that reaches there has a penetration gradient 1e10
    times everyone else's.  (D = 32, align_corners: grid points at linspace(-2, 2, 32); the volume is [x][y][z], psi_oracle.sdf_sample.)"""
    scene = synth.make_scene(5, 3000, 32, 300, kind='room')
    ax = np.linspace(-2.0, 2.0, scene.grid_dim, dtype=np.float32)
    sdf = scene.sdf.copy()
    sdf[ax > STEEP_X0] *= np.float32(1e10)
    assert (sdf[ax > STEEP_X0] < -1e9).all()
    return dataclasses.replace(scene, sdf=sdf)


def _steep_bodies(B, j, where):
    """B bodies on the x < 0 side of the room (each with vertices inside its wall), body j at `where`: 'normal' (with the others),
    'steep' (reaching into the x > STEEP_X0 region) or 'outside' (two scene-cloud box sizes beyond the scene)."""
    bodies = synth.make_bodies(71, B)
    bodies['transl'][:, 0] = -1.0
    bodies['transl'][j, 0] = {'normal': -1.0, 'steep': 1.2, 'outside': 6.0}[where]
    return bodies


def _run_one_iteration(smplx_data, vposer_sd, scene, bodies, indep, w_contact=0.1):
    B = len(bodies['transl'])
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.05, 'num_iter': 1, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': smplx_data, 'vposer_state': vposer_sd, 'scene': scene, 'engine': 'fused', 'align_corners': True}
    torch.manual_seed(0)
    op = fitting.FittingOP(cfg, dict(LOSS, weight_contact=w_contact))
    op.independent_bodies = indep
    op.fitting(dict(bodies))
    return op


@pytest.mark.parametrize('B,indep,w_contact', [(5, False, 0.1), (5, True, 0.1), (40, False, 0.1), (40, True, 0.1), (128, False, 0.1),
                                               (128, True, 0.1), (40, False, 0.0)])
def test_fused_blend_backward_per_body_with_one_steep_body(smplx_data, vposer_sd, B, indep, w_contact):
    """fit_bwd_joint_kernel's fp16 split products with one body whose penetration rows are 1e10 times everyone else's (the SDF is steep
    where only that body reaches): every body's reduced feature gradient, recomputed in fp64 / fp32 from the engine's own g_vposed rows
    of both classes, must be in the fp32 accuracy class on the body's OWN scale (per_body.py).  Coupled (reference batch semantics: one
    penetration count N) and independent bodies (per-body -w / N_b); weight_contact = 0: the penetration class alone."""
    j = B - 2
    scene = _steep_scene()
    op = _run_one_iteration(smplx_data, vposer_sd, scene, _steep_bodies(B, j, 'steep'), indep, w_contact)
    V, K = 10475, 506
    ids = op.contact_vertex_ids().cpu().numpy()
    n_c = len(ids)
    ncp3 = 3 * ((n_c + 255) // 256 * 256)
    Npad = 3 * ((V + 255) // 256 * 256)
    eng = op._fused
    verts = eng.buffer('verts', (B, V, 3)).cpu().numpy()
    gvp = eng.buffer('g_vp', (B, Npad)).cpu().numpy()[:, :3 * V]
    gvpc = eng.buffer('gvpc', (B, ncp3)).cpu().numpy()[:, :3 * n_c]
    gfeat = eng.buffer('gfeat', (B, 512)).cpu().numpy()[:, :K]
    stats = eng.buffer('stats', (8,)).cpu().numpy()
    # preconditions: only body j reaches the steep region (no grid corner of another body's vertices lies there), and the bodies'
    # penetration rows differ by at least 1e9
    h = 4.0 / (scene.grid_dim - 1)
    others = np.arange(B) != j
    assert verts[others, :, 0].max() < STEEP_X0 - h, verts[others, :, 0].max()
    assert (verts[j, :, 0] > STEEP_X0 + h).sum() > 100
    gmax = np.abs(gvp).max(1)
    assert gmax[others].min() > 0 and gmax[j] >= 1e9 * gmax[others].max(), gmax
    if w_contact == 0:
        assert not np.any(gvpc)
    else:
        assert np.abs(gvpc).max(1).min() > 0
    if indep:
        sp = eng.buffer('spb', (B,)).cpu().numpy()
        assert (sp < 0).all()
    else:
        assert stats[4] > 0
        sp = np.full(B, np.float32(-LOSS['weight_collision']) / np.float32(stats[4]), np.float32)
    m = O.SMPLXOracle(smplx_data)
    D = np.concatenate([m.shapedirs.numpy().reshape(3 * V, -1).T, m.posedirs.numpy()], 0)          # [506][3 V] fp32 values
    cols = (3 * ids[:, None] + np.arange(3)[None]).reshape(-1)
    D64 = D.astype(np.float64)
    ref = sp.astype(np.float64)[:, None] * (gvp.astype(np.float64) @ D64.T) + gvpc.astype(np.float64) @ D64[:, cols].T
    r32 = sp[:, None] * (gvp @ D.T) + gvpc @ D[:, cols].T
    per_body.assert_per_body_accuracy_class(gfeat, ref, r32, 'gfeat (B=%d, %s, w_contact=%g)' % (B, 'indep' if indep else 'coupled', w_contact))


@pytest.mark.parametrize('where', ['steep', 'outside'])
def test_fused_independent_bodies_do_not_see_each_other(smplx_data, vposer_sd, where):
    """independent_bodies: every body is its own problem, so moving ONE body — into the region where the SDF is 1e10 times steeper, or two
    scene-box sizes out of the scene (large contact distances: the contact class's rows) — leaves every other body's reduced gradients
    (gA, gfeat, g_transl) after one iteration bit for bit as they were."""
    B, j = 40, 17
    scene = _steep_scene()
    out = {}
    for w in ('normal', where):
        op = _run_one_iteration(smplx_data, vposer_sd, scene, _steep_bodies(B, j, w), True)
        out[w] = {k: op._fused.buffer(k, s).cpu().numpy() for k, s in (('gA', (B, 64, 16)), ('gfeat', (B, 512)), ('g_transl', (B, 3)))}
    others = np.arange(B) != j
    for k in out['normal']:
        a, b = out['normal'][k], out[where][k]
        assert np.isfinite(b).all(), k
        assert not np.array_equal(a[j], b[j]), k                                     # (body j itself did change)
        assert np.array_equal(a[others], b[others]), '%s of the other bodies changed when body %d moved (%s)' % (k, j, where)
