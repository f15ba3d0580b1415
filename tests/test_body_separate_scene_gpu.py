"""The scene term of the rigid separation on the GPU: the kernel bit for bit against the fp32 NumPy restatement on
the host check's inputs and run to run, the loop with the floor teacher-forced and free-running, its result checked by independent
searches and an independent lookup, the loop without a scene against the restatement of the parent's, a fixed body, the refusals and the
entry script."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import body_overlap_cases as BC
import body_separate_cases as K
import body_separate_ref as R
import body_separate_scene_cases as SC
import body_separate_scene_ref as SR
import sdf_lookup_ref as LR
from psi_release_amd import evaluation, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _state(st):
    return ops.RigidState(_t(st.quat), _t(st.transl), _t(st.pivot), _t(st.m), _t(st.s))


def _scene(tup):
    return tuple(_t(a) for a in tup)


@pytest.fixture(scope='module')
def h12():
    c = BC.case('c12x16')
    oh, ch = ops.body_overlap_create(c.faces, c.verts.shape[1]), ops.surface_crossings_create(c.faces, c.verts.shape[1])
    yield type('H', (), dict(oh=oh, ch=ch))
    ops.body_overlap_destroy(oh)
    ops.surface_crossings_destroy(ch)


@pytest.mark.parametrize('V,B,name', SC.KERNEL_CASES)
def test_kernel_bit_for_bit_and_run_to_run(V, B, name):
    kc = SC.kernel_case(V, B, name)
    args = (_t(kc.verts), _t(kc.p), _t(kc.sdf), _t(kc.gmin), _t(kc.gmax), _t(kc.scene_id))
    chunks, count, loss, value, G = ops.rigid_scene_wrench(*args, w_scene=kc.w_scene, return_fields=True)
    w = kc.want
    assert K.same_bits(chunks.cpu().numpy(), w.chunks) and K.same_bits(count.cpu().numpy(), w.count) and K.same_bits(loss.cpu().numpy(), w.loss)
    assert K.same_bits(value.cpu().numpy(), w.value) and K.same_bits(G.cpu().numpy(), w.G)
    again = ops.rigid_scene_wrench(*args, w_scene=kc.w_scene)
    assert len(again) == 3
    for a, b in zip(again, (chunks, count, loss)):
        assert K.same_bits(a.cpu().numpy(), b.cpu().numpy())
    # the chunk rows of the count and the loss, as the loop reads them
    raw = ops._scene_launch(args[0], args[1], args[2:], kc.w_scene)
    SC.assert_wrench(dict(chunks=raw[0].cpu().numpy(), count_chunks=raw[1].cpu().numpy(), loss_chunks=raw[2].cpu().numpy()), w)


def test_no_vertex_in_the_scene_gives_exact_zeros():
    c = BC.case('c12x16')
    sdf, gmin, gmax, _ = SC.floor_scene()
    for verts in (c.verts, c.verts[:1]):                                    # the base stands on the floor; and B = 1
        chunks, count, loss = ops.rigid_scene_wrench(_t(verts), _t(R.default_pivot(verts)), _t(sdf), _t(gmin), _t(gmax))
        assert not count.any().item() and not loss.any().item() and count.dtype == torch.int64 and loss.dtype == torch.float64
        assert K.same_bits(chunks.cpu().numpy(), np.zeros((len(verts), 1, 6)))


@pytest.mark.parametrize('w_scene', [1.0, 2.0])
def test_loop_teacher_forced(h12, w_scene):
    """Every pass of the restatement's trajectory from the restatement's own state: the lists, the vertices in the scene, its loss, the
    summed chunks, g6 and the next state have the restatement's bits.  No pass of these trajectories is ambiguous, neither in w nor in the
    sign of the scene value (tests/test_body_separate_scene_cpu.py)."""
    st, _, n_iter, _, trace = SC.loop(w_scene)
    base = _t(BC.case('c12x16').verts)
    scene = _scene(SC.floor_scene())
    for k, it in enumerate(trace):
        state = _state(it.state)
        one = ops.rigid_pass(base, state, k + 1, h12.oh, h12.ch, scene=scene, w_scene=w_scene)
        assert K.same_bits(one.verts.cpu().numpy(), it.verts)
        assert (one.triples, one.pairs, one.clean, one.stop) == (len(it.triples), len(it.pairs), it.clean, it.stop), k
        assert K.same_bits(one.loss_pen.cpu().numpy(), it.loss_pen) and K.same_bits(one.loss_cross.cpu().numpy(), it.loss_cross)
        assert not one.scene_inside.is_cuda and K.same_bits(one.scene_inside.numpy(), it.scene.count), k
        assert K.same_bits(one.loss_scene.cpu().numpy(), it.scene.loss), k
        if it.stop:
            assert not one.stepped and k == n_iter
            continue
        nxt = trace[k + 1].state
        assert one.stepped and K.same_bits(one.chunks.cpu().numpy(), it.chunks) and K.same_bits(one.g6.cpu().numpy(), it.g6), k
        for key in ('quat', 'transl', 'm', 's'):
            assert K.same_bits(getattr(state, key).cpu().numpy(), getattr(nxt, key)), (k, key)


def _fields(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ('verts', 'quat', 'transl', 'pivot', 'transform', 'shift', 'angle')}
    out['loss_pen'], out['loss_cross'] = res.history['loss_pen'].cpu().numpy(), res.history['loss_cross'].cpu().numpy()
    out['counts'] = np.array([res.iterations, int(res.separated)] + res.history['triples'] + res.history['pairs'])
    if isinstance(res, ops.SceneSeparationResult):
        out['scene_inside'] = np.stack([c.numpy() for c in res.history['scene_inside']])
        out['loss_scene'] = res.history['loss_scene'].cpu().numpy()
    return out


def _assert_clean(verts, faces, scene=None):
    counts, inside = ops.body_overlap(verts, _t(faces))
    cr = ops.surface_crossings(verts, faces, self_pairs=False)
    assert not counts.any().item() and not inside.any().item() and cr.pairs.shape[0] == 0 and not cr.counts.any().item()
    if scene is not None:
        # psi_trilinear is another statement of the lookup: its sign counts only beyond the bound of the operator's statement
        sdf, gmin, gmax = scene[:3]
        got = ops.sdf_sample(verts, _t(sdf), _t(gmin), _t(gmax)).cpu().numpy().astype(np.float64)
        pts = verts.cpu().numpy().reshape(-1, 3)
        ex = LR.exact_lookup(sdf[0], gmin[0], gmax[0], pts, True)
        k = (SC.D - 1) / (gmax[0].astype(np.float64) - gmin[0].astype(np.float64))
        bound = LR.interp_bounds(ex['M'], k, LR.C_VALUE_OP, LR.C_GRAD_OP)[0] + LR.transfer_bound(sdf[0], LR.eu_operator(gmin[0], gmax[0], SC.D, True, pts))
        assert (got.reshape(-1) >= -bound).all() and (ex['value'] >= 0).all()


@pytest.mark.parametrize('w_scene', [1.0, 2.0])
def test_loop_free_running(h12, w_scene):
    c = BC.case('c12x16')
    base, limit = _t(c.verts), SC.ITERATIONS[w_scene] + 4
    sep = evaluation.BodySeparator(c.faces, DEV)
    floor = synth.SceneData(np.zeros((0, 3), np.float32), SC.scene('floor'), SC.BOX[0], SC.BOX[1], SC.D)
    try:
        res = sep.separate(base, max_iter=limit, scene=floor, w_scene=w_scene)
        again = sep.separate(base, max_iter=limit, scene=_scene(SC.floor_scene()), w_scene=w_scene)
    finally:
        sep.close()
    print('w_scene = %g: %d iterations, in the scene %s' % (w_scene, res.iterations, [int(c.sum()) for c in res.history['scene_inside']]))
    assert isinstance(res, ops.SeparationResult) and isinstance(res, ops.SceneSeparationResult) and res.separated and 1 <= res.iterations <= limit
    n = res.iterations + 1
    assert len(res.history['triples']) == len(res.history['pairs']) == len(res.history['scene_inside']) == n
    assert res.history['loss_scene'].shape == (n, 6) and res.history['loss_scene'].dtype == torch.float64 and res.history['loss_pen'].shape == (n, 6)
    assert res.history['triples'][-1] == 0 and res.history['pairs'][-1] == 0 and not res.scene_inside.any().item()
    assert res.scene_inside.dtype == torch.int64 and tuple(res.scene_inside.shape) == (6,) and not res.history['loss_scene'][-1].any().item()
    assert res.history['loss_scene'].max().item() > 0
    _assert_clean(res.verts, c.faces, SC.floor_scene())
    a, b = _fields(res), _fields(again)
    assert all(K.same_bits(a[k], b[k]) for k in a)
    # the restatement, end to end
    st, verts, n_iter, separated, trace = SC.loop(w_scene)
    assert (res.iterations, res.separated) == (n_iter, separated) and res.history['triples'] == [len(t.triples) for t in trace]
    assert res.history['pairs'] == [len(t.pairs) for t in trace] and K.same_bits(a['scene_inside'], np.stack([t.scene.count for t in trace]))
    assert K.same_bits(a['loss_scene'], np.stack([t.scene.loss for t in trace]))
    assert K.same_bits(a['verts'], verts) and K.same_bits(a['quat'], st.quat) and K.same_bits(a['transl'], st.transl)
    for bdy in K.UNTOUCHED:
        assert K.same_bits(a['verts'][bdy], c.verts[bdy])


def test_without_the_scene_the_bodies_end_in_the_floor(h12):
    """What fails without the feature: the call with the floor ends with no vertex in it; the call without, scored by the same kernel,
    ends with the 119 the restatement pins.  And ``scene=None`` is the parent's loop: the restatement of it, bit for bit, with the
    parent's fields and history keys."""
    c = BC.case('c12x16')
    base, scene = _t(c.verts), _scene(SC.floor_scene())
    res = ops.rigid_separate(base, h12.oh, h12.ch, max_iter=SC.CAP, scene=scene)
    assert res.separated and res.scene_inside.sum().item() == 0
    plain = ops.rigid_separate(base, h12.oh, h12.ch, max_iter=SC.CAP)
    st, verts, n_iter, separated, trace = K.loop('c12x16')
    assert plain.separated and plain.iterations == n_iter == K.ITERATIONS['c12x16'] and type(plain) is ops.SeparationResult
    assert sorted(plain.history) == ['loss_cross', 'loss_pen', 'pairs', 'triples']
    assert K.same_bits(plain.verts.cpu().numpy(), verts) and K.same_bits(plain.quat.cpu().numpy(), st.quat)
    assert K.same_bits(plain.transl.cpu().numpy(), st.transl) and plain.history['triples'] == [len(t.triples) for t in trace]
    assert K.same_bits(plain.history['loss_pen'].cpu().numpy(), np.stack([t.loss_pen for t in trace]))
    assert K.same_bits(plain.history['loss_cross'].cpu().numpy(), np.stack([t.loss_cross for t in trace]))
    count = ops.rigid_scene_wrench(plain.verts, plain.pivot + plain.transl, *scene)[1]
    assert count.sum().item() == SC.BELOW_FLOOR_WITHOUT_SCENE and count.tolist() == [55, 63, 0, 0, 1, 0]
    one = ops.rigid_pass(base, ops.rigid_state(_t(R.default_pivot(c.verts))), 1, h12.oh, h12.ch)
    assert one.scene_inside is None and one.stop is None and one.loss_scene is None and one.chunks is None and one.stepped


def test_a_fixed_body_in_the_floor_does_not_hold_the_loop_open(h12):
    c = BC.case('c12x16')
    base_np = c.verts.copy()
    base_np[3, :, 2] -= base_np[3, :, 2].min() + np.float32(0.05)
    scene = SC.floor_scene()
    st, verts, n_iter, separated, trace = SR.separate(base_np, c.faces, scene=scene, fixed=[3], max_iter=SC.CAP)
    res = ops.rigid_separate(_t(base_np), h12.oh, h12.ch, max_iter=SC.CAP, scene=_scene(scene), fixed=[3])
    assert res.separated and separated and res.iterations == n_iter
    assert res.scene_inside[3].item() == trace[-1].scene.count[3] > 0 and res.scene_inside.sum().item() == res.scene_inside[3].item()
    assert K.same_bits(res.verts.cpu().numpy(), verts) and K.same_bits(res.verts[3].cpu().numpy(), base_np[3])
    assert K.same_bits(res.quat[3].cpu().numpy(), np.array([1, 0, 0, 0], np.float32)) and not res.transl[3].any().item()


def test_refusals_leave_the_handles_usable(h12):
    c = BC.case('c12x16')
    base = _t(c.verts)
    sdf, lo, hi, _ = _scene(SC.floor_scene())
    nan = float('nan')
    for kw in (dict(scene=(sdf, lo, hi)), dict(scene=(sdf.cpu(), lo, hi, None)), dict(scene=(sdf.double(), lo, hi, None)),
               dict(scene=(sdf[:, :, :, :-1].contiguous(), lo, hi, None)), dict(scene=(sdf[:, :1, :1, :1].contiguous(), lo, hi, None)),
               dict(scene=(sdf, lo[0], hi, None)), dict(scene=(sdf, lo, hi, torch.zeros(6, device=DEV))),
               dict(scene=(sdf, lo, hi, torch.zeros(5, dtype=torch.int32, device=DEV))), dict(scene=(sdf, lo, hi, None), w_scene=0.0),
               dict(scene=(sdf, lo, hi, None), w_scene=-1.0), dict(scene=(sdf, lo, hi, None), w_scene=nan)):
        with pytest.raises(ValueError):
            ops.rigid_separate(base, h12.oh, h12.ch, **kw)
    with pytest.raises(hip.PsiHipError):
        ops.rigid_scene_wrench(base, base[:, 0, :], sdf, lo, hi)             # p is not contiguous
    L = hip.lib()
    p = base[:, 0, :].contiguous()
    nchunk = 1
    ch, cn, ls = torch.full((6, nchunk, 6), 7.0, dtype=torch.float64, device=DEV), torch.full((6, nchunk), 7, dtype=torch.int32, device=DEV), \
        torch.full((6, nchunk), 7.0, dtype=torch.float64, device=DEV)
    args = lambda **kw: [hip.ptr(base), hip.ptr(p), hip.ptr(sdf), hip.ptr(lo), hip.ptr(hi), None, kw.get('B', 6), kw.get('V', 178), kw.get('D', SC.D),
                         kw.get('S', 1), kw.get('w', 1.0), hip.ptr(ch), hip.ptr(cn), hip.ptr(ls), None, None, None]
    for bad in (dict(B=0), dict(B=46341), dict(V=0), dict(V=(1 << 24) + 1), dict(D=1), dict(S=0), dict(w=-1.0), dict(w=nan), dict(w=float('inf'))):
        assert L.psi_body_separate_scene(*args(**bad)) == -22
    for i in (0, 1, 2, 3, 4, 11, 12, 13):
        a = args()
        a[i] = None
        assert L.psi_body_separate_scene(*a) == -22
    assert (ch == 7).all().item() and (cn == 7).all().item() and (ls == 7).all().item()     # nothing was touched
    res = ops.rigid_separate(base, h12.oh, h12.ch, max_iter=SC.CAP, scene=(sdf, lo, hi, None), w_scene=2.0)
    assert res.separated and res.iterations == SC.ITERATIONS[2.0]
    sep = evaluation.BodySeparator(c.faces, DEV)
    floor = synth.SceneData(np.zeros((0, 3), np.float32), SC.scene('floor'), SC.BOX[0], SC.BOX[1], SC.D)
    small = synth.SceneData(np.zeros((0, 3), np.float32), SC.scene('floor')[:8, :8, :8], SC.BOX[0], SC.BOX[1], 8)
    try:
        for kw in (dict(scene=[floor, small], scene_id=[0] * 6), dict(scene=[floor, floor]), dict(scene='room'), dict(scene_id=[0] * 6),
                   dict(scene=(sdf, lo, hi, None), scene_id=[0] * 6)):
            with pytest.raises(ValueError):
                sep.separate(base, **kw)
        two = sep.separate(base, max_iter=SC.CAP, scene=[floor, floor], scene_id=[0, 1, 1, 0, 5, -1], w_scene=2.0)
        assert two.separated and K.same_bits(two.verts.cpu().numpy(), res.verts.cpu().numpy())
    finally:
        sep.close()


def test_script_end_to_end_with_a_floor(tmp_path, capsys):
    """utils_separate_bodies.py --scene_floor on generated bodies with the stand-in model: the pkls it writes, read back and skinned, have no
    vertex inside another body, no crossing surfaces and no vertex in the floor; without the option every line and field is what it was.
    These four bodies nearly coincide (4609 inside triples): Adam's second moment remembers those gradients, so the last vertex in the floor
    moves slowly, and the default w_scene = 1 needs 235 passes, more than the script's default limit; 10 needs 62."""
    sys.path.insert(0, os.path.join(ROOT, 'psi-release_amd', 'utils'))
    try:
        import utils_separate_bodies as E
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    gen, out = str(tmp_path / 'gen'), str(tmp_path / 'out')
    os.makedirs(gen)
    for i in range(4):
        rec = synth.make_bodies(40 + i, 1)
        rec['transl'] = (rec['transl'] * 0.2 + np.array([6.0 * (i // 2), 0.0, 0.0])).astype(np.float32)
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump(rec, f)
    device = torch.device(DEV, torch.cuda.current_device())
    decoder = S.BodyDecoder(synth.make_smplx(7), synth.make_vposer_state(3), device)
    xh0, cam0 = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    verts0 = decoder.verts(xh0, S.camera_pose(cam0, True))
    z = float(verts0[..., 2].min().item()) + 0.02                           # the lowest vertex stands 2 cm in the floor
    common = [gen, out, '--synthetic', str(tmp_path / 'syn'), '--no_flip']
    plain = E.main(common + ['--out', str(tmp_path / 'plain.json')])
    lines_plain = capsys.readouterr().out.splitlines()
    rep = E.main(common + ['--scene_floor', repr(z), '--w_scene', '10', '--out', str(tmp_path / 'rep.json')])
    lines = capsys.readouterr().out.splitlines()
    print('script: %s' % {k: rep[k] for k in ('iterations', 'separated', 'scene_inside_before', 'scene_inside_after', 'max_shift')})
    assert json.load(open(str(tmp_path / 'rep.json'))) == rep and len(lines) == 5 and len(lines_plain) == 4
    assert 'scene_inside_before' not in plain and 'w_scene' not in plain and json.load(open(str(tmp_path / 'plain.json'))) == plain
    assert rep['separated'] and 1 <= rep['iterations'] <= 100 and rep['w_scene'] == 10.0
    assert sum(rep['scene_inside_before']) > 0 and rep['scene_inside_after'] == [0, 0, 0, 0] and rep['scene_inside'][0] == rep['scene_inside_before']
    assert 'vertices in the scene: %d before, 0 after' % sum(rep['scene_inside_before']) in lines[3]
    assert rep['overlapping_pairs_after'] == [] and rep['crossing_pairs_after'] == []
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(out, 100)
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    faces = decoder.faces.to(torch.int32).cpu().numpy()
    counts, inside = ops.body_overlap(verts, _t(faces))
    assert not counts.any().item() and ops.surface_crossings(verts, faces, self_pairs=False).pairs.shape[0] == 0
    # the class under the script, with the script's own floor volume
    floor = E.floor_scene(verts0, z)
    sep = evaluation.BodySeparator(decoder.faces, DEV)
    try:
        res, cam_new = sep.separate_records(xh0, S.camera_pose(cam0, True), decoder, scene=floor, w_scene=10.0)
        bare, _ = sep.separate_records(xh0, S.camera_pose(cam0, True), decoder)
        table = sep.scene_table(floor)
    finally:
        sep.close()
    assert res.separated and res.iterations == rep['iterations'] and K.same_bits(cam_new.astype(np.float32), cam)
    assert ops.rigid_scene_wrench(res.verts, res.pivot + res.transl, *table)[1].sum().item() == 0
    assert ops.rigid_scene_wrench(verts, res.pivot + res.transl, *table)[1].sum().item() == 0          # the records, skinned again
    assert bare.separated and bare.iterations == plain['iterations'] and type(bare) is ops.SeparationResult
