"""The rigid separation of overlapping bodies on the GPU: the three kernels bit for bit against the fp32 NumPy
restatement at the chunk boundaries, run to run, the loop teacher-forced and free-running on the capsule batches, the results checked by
independent searches, groups, the empty cases, the refusals and the entry script."""
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
from psi_release_amd import evaluation, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    """As tests/test_surface_crossings_gpu.py does: what this module's calls leave in PyTorch's caching allocator goes back to the
    runtime when the module ends."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _state(st):
    """A restatement State as a RigidState on the device (copies)."""
    return ops.RigidState(_t(st.quat), _t(st.transl), _t(st.pivot), _t(st.m), _t(st.s))


def _host_state(state):
    return {k: getattr(state, k).cpu().numpy() for k in ('quat', 'transl', 'm', 's')}


def _kernel_steps(kc, B, fused):
    """The STEPS steps of a kernel case on the GPU, as dicts like those of K.run_host_check.  ``fused``: the chunk sums go straight into the
    step's launch (what the loop does); otherwise rigid_wrench finishes g6 and rigid_step reads it."""
    base, G = _t(kc.base), _t(kc.G)
    state = ops.rigid_state(_t(kc.pivot))
    out = []
    for k in range(1, K.STEPS + 1):
        verts = ops.rigid_pose(base, state.quat, state.transl, state.pivot)
        p = state.pivot + state.transl
        if fused:
            g6 = torch.empty(B, 6, dtype=torch.float32, device=DEV)
            chunks = ops._rigid_chunks(verts, G[k - 1], p, None)
            ops._rigid_step(state, g6, chunks, k, 0.01, 0.01, (0.9, 0.999), 1e-8, ops._fixed_mask(kc.fixed, B, torch.device(DEV, torch.cuda.current_device())))
        else:
            g6, chunks = ops.rigid_wrench(verts, G[k - 1], p, return_chunks=True)
            assert ops.rigid_step(state, g6, k, fixed=kc.fixed) is state
        out.append(dict(verts=verts.cpu().numpy(), chunks=chunks.cpu().numpy(), g6=g6.cpu().numpy(), **_host_state(state)))
    return out


@pytest.mark.parametrize('V,B', K.KERNEL_CASES)
def test_kernels_bit_for_bit_and_run_to_run(V, B):
    kc = K.kernel_case(V, B)
    got = _kernel_steps(kc, B, fused=False)
    for k, (g, want) in enumerate(zip(got, kc.steps), 1):
        K.assert_step(g, want, 'step %d' % k)
    again = _kernel_steps(kc, B, fused=True)
    for g, a in zip(got, again):
        assert all(K.same_bits(g[key], a[key]) for key in g)
    if B > K.FIXED_BODY:
        for b in (K.ZERO_BODY, K.FIXED_BODY):
            assert K.same_bits(got[-1]['verts'][b], kc.base[b]) and K.same_bits(got[-1]['quat'][b], np.array([1, 0, 0, 0], np.float32))
        assert np.abs(got[0]['g6'][K.FIXED_BODY]).max() > 0
    moved = [b for b in range(B) if B == 1 or b not in (K.ZERO_BODY, K.FIXED_BODY)]
    assert all(not K.same_bits(got[-1]['verts'][b], kc.base[b]) for b in moved)


def test_pose_identity_and_negative_zero():
    c = BC.case('c24x46')
    base = _t(c.verts)
    st = ops.rigid_state(_t(R.default_pivot(c.verts)))
    assert K.same_bits(ops.rigid_pose(base, st.quat, st.transl, st.pivot).cpu().numpy(), c.verts)
    st.transl[1, 2] = -0.0
    st.transl[3, 0] = 1e-3
    out = ops.rigid_pose(base, st.quat, st.transl, st.pivot).cpu().numpy()
    assert K.same_bits(out[[0, 1, 2, 4, 5]], c.verts[[0, 1, 2, 4, 5]]) and not np.array_equal(out[3], c.verts[3])
    assert K.same_bits(out, R.pose(c.verts, st.quat.cpu().numpy(), st.transl.cpu().numpy(), st.pivot.cpu().numpy()))


class _Handles:
    def __init__(self, faces, V):
        self.oh = ops.body_overlap_create(faces, V)
        self.ch = ops.surface_crossings_create(faces, V)

    def close(self):
        ops.body_overlap_destroy(self.oh)
        ops.surface_crossings_destroy(self.ch)


@pytest.fixture(scope='module')
def h12():
    c = BC.case('c12x16')
    h = _Handles(c.faces, c.verts.shape[1])
    yield h
    h.close()


@pytest.mark.parametrize('name', ['c12x16', 'c12x16_fixed0'])
def test_loop_teacher_forced(h12, name):
    """Every pass of the restatement's trajectory from the restatement's own state: the lists agree, and the next state has its bits.  A
    pass is compared only where no candidate's fp64 winding number is within AMBIGUOUS of 0.5; at most a tenth may be left out."""
    st, _, n_iter, _, trace = K.loop(name)
    base_np, _ = K.loop_inputs(name)
    base = _t(base_np)
    mask = ops._fixed_mask(K.LOOPS[name].get('fixed'), 6, base.device)
    skipped = 0
    for k, it in enumerate(trace):
        if len(it.cand_w) and np.abs(it.cand_w - 0.5).min() <= BC.AMBIGUOUS:
            skipped += 1
            continue
        state = _state(it.state)
        one = ops.rigid_pass(base, state, k + 1, h12.oh, h12.ch, fixed_mask=mask)
        assert K.same_bits(one.verts.cpu().numpy(), it.verts)
        assert (one.triples, one.pairs, one.clean) == (len(it.triples), len(it.pairs), it.clean), k
        assert K.same_bits(one.loss_pen.cpu().numpy(), it.loss_pen) and K.same_bits(one.loss_cross.cpu().numpy(), it.loss_cross)
        if it.clean:
            assert not one.stepped and k == n_iter
            continue
        nxt = trace[k + 1].state
        assert one.stepped and K.same_bits(one.g6.cpu().numpy(), it.g6), k
        for key, v in _host_state(state).items():
            assert K.same_bits(v, getattr(nxt, key)), (k, key)
    assert skipped <= len(trace) // 10


def _fields(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ('verts', 'quat', 'transl', 'pivot', 'transform', 'shift', 'angle')}
    out['loss_pen'], out['loss_cross'] = res.history['loss_pen'].cpu().numpy(), res.history['loss_cross'].cpu().numpy()
    out['counts'] = np.array([res.iterations, int(res.separated)] + res.history['triples'] + res.history['pairs'])
    return out


def _assert_clean(verts, faces):
    counts, inside = ops.body_overlap(verts, _t(faces))
    cr = ops.surface_crossings(verts, faces, self_pairs=False)
    assert not counts.any().item() and not inside.any().item() and cr.pairs.shape[0] == 0 and not cr.counts.any().item()


@pytest.mark.parametrize('name,limit', [('c12x16', K.ITERATIONS['c12x16'] + 4), ('c24x46', K.CAP + 4)])
def test_loop_free_running(name, limit):
    c = BC.case(name)
    base = _t(c.verts)
    sep = evaluation.BodySeparator(c.faces, DEV)
    try:
        res = sep.separate(base, max_iter=limit)
        again = sep.separate(base, max_iter=limit)
    finally:
        sep.close()
    print('%s: %d iterations, triples %s, pairs %s, shift %.4f m, angle %.4f rad' % (name, res.iterations, res.history['triples'], res.history['pairs'],
                                                                                       res.shift.max().item(), res.angle.max().item()))
    assert isinstance(res, ops.SeparationResult) and res.separated and 1 <= res.iterations <= limit
    assert len(res.history['triples']) == len(res.history['pairs']) == res.iterations + 1 == res.history['loss_pen'].shape[0]
    assert res.history['triples'][-1] == 0 and res.history['pairs'][-1] == 0 and res.history['loss_pen'].shape == res.history['loss_cross'].shape
    assert not res.history['loss_pen'][-1].any().item() and res.history['loss_pen'][0].max().item() > 0
    _assert_clean(res.verts, c.faces)
    a, b = _fields(res), _fields(again)
    assert all(K.same_bits(a[k], b[k]) for k in a)
    assert res.transform.dtype == torch.float64 and res.transform.shape == (6, 4, 4)
    M = a['transform']
    x = np.einsum('bkl,bvl->bvk', M[:, :3, :3], c.verts.astype(np.float64)) + M[:, None, :3, 3]
    assert np.abs(x - a['verts']).max() <= 2 * K.pose_bound(c.verts, a['pivot'], a['transl'])
    assert K.same_bits(a['verts'], R.pose(c.verts, a['quat'], a['transl'], a['pivot'])) and K.same_bits(a['pivot'], R.default_pivot(c.verts))
    want_shift, want_angle = R.shift_angle(a['quat'], a['transl'])
    assert np.allclose(a['shift'], want_shift, rtol=1e-12, atol=1e-15) and np.allclose(a['angle'], want_angle, rtol=1e-9, atol=1e-12)
    assert a['shift'].max() < 0.5 and a['angle'].max() < 0.5
    if name == 'c12x16':
        for bdy in K.UNTOUCHED:
            assert K.same_bits(a['verts'][bdy], c.verts[bdy])


def test_loop_matches_the_restatement_end_to_end(h12):
    """No pass of this trajectory is ambiguous (tests/test_body_separate_cpu.py), so the free-running loop is the restatement's, bit for
    bit; with body 0 fixed, body 0 keeps its bits."""
    base_np, _ = K.loop_inputs('c12x16')
    for name in ('c12x16', 'c12x16_fixed0'):
        st, verts, n_iter, separated, trace = K.loop(name)
        res = ops.rigid_separate(_t(base_np), h12.oh, h12.ch, max_iter=K.CAP, **K.LOOPS[name])
        assert (res.iterations, res.separated) == (n_iter, separated) and res.history['triples'] == [len(t.triples) for t in trace]
        assert res.history['pairs'] == [len(t.pairs) for t in trace]
        assert K.same_bits(res.verts.cpu().numpy(), verts) and K.same_bits(res.quat.cpu().numpy(), st.quat) and K.same_bits(res.transl.cpu().numpy(), st.transl)
        assert np.abs(res.transform.cpu().numpy() - R.transform(st.quat, st.transl, st.pivot)).max() < 1e-14
    assert K.same_bits(res.verts[0].cpu().numpy(), base_np[0]) and K.same_bits(res.quat[0].cpu().numpy(), np.array([1, 0, 0, 0], np.float32))


def test_terms_alone_thin_and_the_iteration_limit(h12):
    base_np, faces = K.loop_inputs('c12x16')
    base = _t(base_np)
    res = ops.rigid_separate(base, h12.oh, h12.ch, w_cross=0.0, max_iter=K.CAP)
    assert res.separated and res.iterations == K.ITERATIONS['c12x16_pen_only'] and set(res.history['pairs']) == {-1}
    assert not ops.body_overlap(res.verts, h12.oh)[0].any().item()
    assert ops.surface_crossings(res.verts, h12.ch, self_pairs=False).pairs.shape[0] == K.PAIRS_LEFT
    cut = ops.rigid_separate(base, h12.oh, h12.ch, max_iter=3)
    assert not cut.separated and cut.iterations == 3 and len(cut.history['triples']) == 4 and cut.history['triples'][-1] > 0
    assert K.same_bits(cut.verts.cpu().numpy(), K.loop('c12x16')[4][3].verts)
    sq = ops.rigid_separate(base, h12.oh, h12.ch, penalty='squared', sigma=1e-3, max_iter=K.CAP)
    assert sq.separated and sq.iterations == K.ITERATIONS['c12x16_squared']
    thin_np, thin_faces = K.loop_inputs('thin')
    thin = ops.rigid_separate(_t(thin_np), _t(thin_faces), _t(thin_faces), max_iter=K.CAP)
    assert thin.separated and thin.iterations == K.ITERATIONS['thin'] and set(thin.history['triples']) == {0} and thin.history['pairs'][0] == 72
    _assert_clean(thin.verts, thin_faces)
    only = ops.rigid_separate(_t(thin_np), _t(thin_faces), _t(thin_faces), w_pen=0.0, max_iter=K.CAP)
    assert only.separated and set(only.history['triples']) == {-1} and K.same_bits(only.verts.cpu().numpy(), thin.verts.cpu().numpy())


def test_groups_no_overlap_and_own_pivot(h12):
    base_np, faces = K.loop_inputs('c12x16')
    base = _t(base_np)
    group = _t(np.array([0, 1, 0, 0, 0, 2], np.int32))                                     # the overlapping pairs (0,1), (0,5), (1,5) are split
    res = ops.rigid_separate(base, h12.oh, h12.ch, group=group)
    assert res.separated and res.iterations == 0 and K.same_bits(res.verts.cpu().numpy(), base_np)
    assert res.history['triples'] == [0] and res.history['pairs'] == [0] and not res.shift.any().item() and not res.angle.any().item()
    assert np.array_equal(res.transform.cpu().numpy(), np.tile(np.eye(4), (6, 1, 1)))
    apart = base_np + (np.arange(6, dtype=np.float32) * 5.0)[:, None, None]
    res = ops.rigid_separate(_t(apart), h12.oh, h12.ch)
    assert res.separated and res.iterations == 0 and K.same_bits(res.verts.cpu().numpy(), apart)       # no step was launched
    one = ops.rigid_separate(base[:1].contiguous(), h12.oh, h12.ch)
    assert one.separated and one.iterations == 0
    two = ops.rigid_separate(base, h12.oh, h12.ch, group=_t(np.array([0, 0, 1, 1, 1, 2], np.int32)), max_iter=K.CAP)
    assert two.separated and two.iterations >= 1 and K.same_bits(two.verts[2:].cpu().numpy(), base_np[2:])
    pivot = _t(base_np[:, 0].copy())                                                        # a vertex of each body as its pivot
    own = ops.rigid_separate(base, h12.oh, h12.ch, pivot=pivot, max_iter=K.CAP)
    st, verts, n_iter, separated, _ = R.separate(base_np, faces, pivot=base_np[:, 0], max_iter=K.CAP)
    assert own.separated and separated and own.iterations == n_iter <= K.CAP and K.same_bits(own.verts.cpu().numpy(), verts)
    assert K.same_bits(own.pivot.cpu().numpy(), base_np[:, 0])


def test_refusals_leave_the_handles_usable(h12):
    base_np, _ = K.loop_inputs('c12x16')
    base = _t(base_np)
    for kw in (dict(max_iter=0), dict(lr_t=0.0), dict(lr_r=float('inf')), dict(sigma=0.75), dict(w_pen=-1.0), dict(w_pen=0.0, w_cross=0.0),
               dict(fixed=[6]), dict(pivot=torch.zeros(6, 3)), dict(group=torch.zeros(6, dtype=torch.int32)), dict(penalty='cubed')):
        with pytest.raises(ValueError):
            ops.rigid_separate(base, h12.oh, h12.ch, **kw)
    with pytest.raises(ValueError):
        ops.rigid_separate(base[:, :100].contiguous(), h12.oh, h12.ch)                      # the handles were made for 178 vertices
    nan = base.clone()
    nan[2, 3, 0] = float('nan')
    with pytest.raises(ValueError, match='body 2 '):
        ops.rigid_separate(nan, h12.oh, h12.ch)
    with pytest.raises(hip.PsiHipError):
        ops.rigid_pose(base[:, ::2], *ops.rigid_state(_t(R.default_pivot(base_np)))[:3])    # not contiguous
    L = hip.lib()
    st = ops.rigid_state(_t(R.default_pivot(base_np)))
    g6 = torch.zeros(6, 6, device=DEV)
    args = lambda **kw: [None, 0, hip.ptr(g6), hip.ptr(st.quat), hip.ptr(st.transl), hip.ptr(st.m), hip.ptr(st.s), None, kw.get('B', 6),
                         kw.get('b1', 0.9), 0.999, kw.get('c1', 0.1), 0.001, kw.get('eps', 1e-8), kw.get('lr', 0.01), 0.01, None]
    for bad in (dict(B=0), dict(B=46341), dict(b1=1.0), dict(c1=0.0), dict(c1=1.5), dict(eps=-1.0), dict(lr=0.0), dict(lr=float('inf'))):
        assert L.psi_body_separate_step(*args(**bad)) == -22
    a = args()
    a[1] = 3                                                                                # chunks are missing
    assert L.psi_body_separate_step(*a) == -22
    assert L.psi_body_separate_pose(hip.ptr(base), hip.ptr(st.quat), hip.ptr(st.transl), hip.ptr(st.pivot), 6, 0, hip.ptr(base), None) == -22
    assert L.psi_body_separate_wrench(hip.ptr(base), hip.ptr(base), hip.ptr(st.pivot), 6, (1 << 24) + 1, hip.ptr(g6), None, None) == -22
    assert K.same_bits(st.quat.cpu().numpy(), R.State(6, np.zeros((6, 3))).quat) and not st.m.any().item()      # nothing was touched
    res = ops.rigid_separate(base, h12.oh, h12.ch, max_iter=K.CAP)
    assert res.separated and res.iterations == K.ITERATIONS['c12x16']


def test_script_end_to_end(tmp_path, capsys):
    """utils_separate_bodies.py on generated bodies with the stand-in model: the pkls it writes, read back and skinned, have no vertex
    inside another body and no crossing surfaces; nothing but cam_ext differs from the records read."""
    sys.path.insert(0, os.path.join(ROOT, 'psi-release_amd', 'utils'))
    try:
        import utils_separate_bodies as E
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    gen, out = str(tmp_path / 'gen'), str(tmp_path / 'out')
    os.makedirs(gen)
    recs = []
    for i in range(4):
        rec = synth.make_bodies(40 + i, 1)
        rec['transl'] = (rec['transl'] * 0.2 + np.array([6.0 * (i // 2), 0.0, 0.0])).astype(np.float32)
        recs.append(rec)
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump(rec, f)
    rep = E.main([gen, out, '--synthetic', str(tmp_path / 'syn'), '--no_flip', '--out', str(tmp_path / 'rep.json')])
    lines = capsys.readouterr().out.splitlines()
    print('script: %s' % {k: rep[k] for k in ('iterations', 'separated', 'max_shift', 'max_angle', 'triples', 'pairs')})
    assert json.load(open(str(tmp_path / 'rep.json'))) == rep and len(lines) == 4
    assert rep['separated'] and 1 <= rep['iterations'] <= 100 and rep['bodies'] == 4
    assert len(rep['overlapping_pairs_before']) + len(rep['crossing_pairs_before']) > 0
    assert rep['overlapping_pairs_after'] == [] and rep['crossing_pairs_after'] == []
    assert sorted(os.listdir(out)) == ['body_gen_{:06d}.pkl'.format(i) for i in range(4)]
    for i, rec in enumerate(recs):
        new = pickle.load(open(os.path.join(out, 'body_gen_{:06d}.pkl'.format(i)), 'rb'))
        assert set(new) == set(rec) and new['cam_ext'].shape == (1, 4, 4) and new['cam_ext'].dtype == np.float32
        assert all(K.same_bits(np.asarray(new[k]), np.asarray(rec[k])) for k in rec if k != 'cam_ext')
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(out, 100)
    decoder = S.BodyDecoder(synth.make_smplx(7), synth.make_vposer_state(3), torch.device(DEV, torch.cuda.current_device()))
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    _assert_clean(verts, decoder.faces.to(torch.int32).cpu().numpy())
    moved = [i for i in range(4) if not np.array_equal(cam[i], np.eye(4, dtype=np.float32))]
    assert moved and abs(rep['max_shift']) < 1.0
    # the class under the script: the same loop, and the camera poses it returns are the ones the script wrote
    xh0, cam0 = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    sep = evaluation.BodySeparator(decoder.faces, DEV)
    try:
        res, cam_new = sep.separate_records(xh0, S.camera_pose(cam0, True), decoder)
    finally:
        sep.close()
    assert res.separated and res.iterations == rep['iterations'] and res.history['triples'] == rep['triples']
    assert cam_new.dtype == np.float64 and cam_new.shape == (4, 4, 4) and K.same_bits(cam_new.astype(np.float32), cam)
    assert np.abs(verts.cpu().numpy() - res.verts.cpu().numpy()).max() < 1e-5            # re-skinned through cam_ext': the same bodies
