"""Penetration depth on the GPU (csrc/body_depth.hip; ops.body_depth, ops.body_penetration, ops.body_penetration_loss;
evaluation.BodyOverlap.depths / .penetration_loss): the rows of the shared lists and of the planted case against the fp32 NumPy restatement
(tests/body_depth_ref.py) BIT FOR BIT, the aggregates and the gradient G likewise, the bits of a triple's row under subsets, a permutation
and groups, run-to-run determinism, autograd, degenerate batches, the workload's face count against the analytic capsule, the refusals and
the script end to end.  Every test prints its figures before it asserts."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import body_depth_cases as K
import body_depth_ref as D
import body_handles_cases as H
import body_overlap_cases as C
from psi_release_amd import evaluation, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
G_UNEVEN = np.array([1.0, -0.5, 2.0, 0.25, 3.0, 0.75], np.float32)
ROW_KEYS = ('face', 'region', 'depth', 'r', 'bary')


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    """As tests/test_body_overlap_gpu.py: the handles are freed and the allocator's cached blocks go back to the runtime after the module."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _rows(rows):
    """DepthRows -> dict of host arrays"""
    assert [t.dtype for t in rows] == [torch.int32, torch.int32, torch.float32, torch.float32, torch.float32] and all(t.is_cuda for t in rows)
    return dict(zip(ROW_KEYS, (t.cpu().numpy() for t in rows)))


def _differing(got, want):
    return {k: int((np.ascontiguousarray(got[k]).view(np.uint32).reshape(len(got[k]), -1) !=
                    np.ascontiguousarray(want[k]).view(np.uint32).reshape(len(want[k]), -1)).any(1).sum()) for k in ROW_KEYS}


def _case(name):
    return K.PLANTED if name == 'planted' else C.case(name)


@pytest.mark.parametrize('name,which', K.LISTS + [('planted', '')])
def test_rows_against_restatement_bit_for_bit(name, which):
    cs = _case(name)
    trip = K.PLANTED.trip if name == 'planted' else K.triples(name, which)
    want = K.ref(name, which)
    got = _rows(ops.body_depth(_dev(cs.verts), torch.tensor(cs.faces), _dev(trip)))
    diff = _differing(got, want)
    print('%s %s: %d triples, rows with other bits %s, regions %s' % (name, which, len(trip), diff, np.bincount(got['region'], minlength=7).tolist()))
    assert all(len(got[k]) == len(trip) for k in ROW_KEYS)
    assert not any(diff.values())
    if name == 'planted':
        assert set(got['region'].tolist()) == set(range(7))                             # all seven regions, through `region`
    elif which == 'all':
        assert set(got['region'].tolist()) == {0, 1, 2, 3, 6} and int(want['ties'].sum()) == K.TIES[(name, which)]


def test_a_non_finite_face_loses():
    """The batch of test_body_depth_cpu.py::test_a_collinear_face_with_a_non_finite_d2_loses: face 0 of body 1 gives a NaN, face 1 wins."""
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    verts = np.zeros((2, 6, 3), np.float32)
    verts[1] = [[0, 0, 0], [1e20, 0, 0], [2e20, 0, 0], [10, 0, 0], [11, 0, 0], [10, 1, 0]]
    verts[0, :2] = [[3, 1, 0], [10.25, 0.25, 2.0]]
    trip = np.array([[0, 1, 0], [0, 1, 1]], np.int32)
    with np.errstate(all='ignore'):
        want = D.nearest(verts, faces, trip)
    got = _rows(ops.body_depth(_dev(verts), torch.tensor(faces), _dev(trip)))
    print('faces %s regions %s depths %s' % (got['face'].tolist(), got['region'].tolist(), got['depth'].tolist()))
    assert got['face'].tolist() == [1, 1] and got['depth'].tolist() == [7.0, 2.0] and not any(_differing(got, want).values())


@pytest.fixture(scope='module')
def penetration():
    """name -> (PenetrationResult, its evaluator): one forward run per case, shared, read-only.  The evaluator comes along for the tests
    that go on with its handle (``_handle_for``) or its methods; nothing here depends on it for the handle's lifetime."""
    cache = {}

    def get(name):
        if name not in cache:
            cs = C.case(name)
            bo = evaluation.BodyOverlap(cs.faces, DEV)
            cache[name] = (bo.depths(_dev(cs.verts)), bo)
        return cache[name]
    return get


@pytest.mark.parametrize('name', ['c12x16', 'c24x46'])
def test_penetration_aggregates_and_gradient_bit_for_bit(name, penetration):
    cs = C.case(name)
    B, V = cs.verts.shape[:2]
    res, bo = penetration(name)
    trip, want = K.triples(name, 'inside'), K.ref(name, 'inside')
    got_trip = res.triples.cpu().numpy()
    assert got_trip.dtype == np.int32 and np.array_equal(got_trip, trip)
    diff = _differing(_rows(res.rows), want)
    agg = dict(zip(('max_depth', 'sum_depth', 'sum_sq', 'depth_of', 'loss'), D.aggregates(trip, want['depth'], B, V)))
    got = {k: getattr(res, k).cpu().numpy() for k in agg}
    agg_same = {k: K.same_bits(got[k], agg[k]) for k in agg}
    print('%s: %d inside triples, rows with other bits %s, aggregates equal %s; loss %s, deepest %.4f m'
          % (name, len(trip), diff, agg_same, got['loss'][0].tolist(), got['max_depth'].max()))
    assert not any(diff.values()) and all(agg_same.values())
    assert np.array_equal(res.counts.cpu().numpy(), cs.ref()[0]) and np.array_equal(res.inside.cpu().numpy(), cs.ref()[1])
    assert res.sum_depth.dtype == torch.float64 and res.sum_sq.dtype == torch.float64 and res.depth_of.shape == (B, V)
    assert np.array_equal(got['depth_of'] > 0, cs.ref()[1] & (got['depth_of'] > 0)) and (got['depth_of'] > 0).sum() >= cs.ref()[1].sum() - 2
    handle = bo._handle_for(V)
    for penalty in ('depth', 'squared'):
        for g in (np.ones(B, np.float32), G_UNEVEN):
            G = ops.body_penetration_grad((B, V, 3), handle, res.triples, res.rows, _dev(g), penalty).cpu().numpy()
            ref_G = D.gradient(trip, want, cs.faces, g, penalty, B, V)
            other = int((G.view(np.uint32) != ref_G.view(np.uint32)).any(2).sum())
            print('   G %s, g %s: %d vertices with other bits of %d touched' % (penalty, 'ones' if g[1] == 1 else 'uneven', other, ref_G.any(2).sum()))
            assert other == 0 and ref_G.any()


def _by_triple(trip, rows, relabel=None):
    """{(i, j, v): the bits of the row}, the bodies renamed by ``relabel`` (batch index -> name)."""
    c = np.asarray(trip, np.int64)
    if relabel is not None:
        c = np.stack([np.asarray(relabel)[c[:, 0]], np.asarray(relabel)[c[:, 1]], c[:, 2]], 1)
    packed = np.concatenate([np.ascontiguousarray(rows[k]).view(np.uint32).reshape(len(c), -1) for k in ROW_KEYS], 1)
    return dict(zip(C.triple_keys(c).tolist(), map(bytes, packed)))


def test_row_of_a_triple_does_not_depend_on_the_batch(penetration):
    cs = C.case('c24x46')
    res, _ = penetration('c24x46')
    full = _by_triple(res.triples.cpu().numpy(), _rows(res.rows))
    faces = torch.tensor(cs.faces)
    for sub in ([0, 1], [5, 1], [5, 3, 1, 0, 4, 2]):
        s = ops.body_penetration(_dev(cs.verts[sub]), faces)
        got = _by_triple(s.triples.cpu().numpy(), _rows(s.rows), relabel=sub)
        want = {k: b for k, b in full.items() if (k >> 40) in sub and ((k >> 20) & 0xfffff) in sub}
        print('bodies %s: %d triples, %d with other bits' % (sub, len(got), sum(got[k] != want.get(k) for k in got)))
        assert got == want and len(got) > 0
        assert K.same_bits(s.max_depth.cpu().numpy(), res.max_depth.cpu().numpy()[np.ix_(sub, sub)])
        assert K.same_bits(s.sum_depth.cpu().numpy(), res.sum_depth.cpu().numpy()[np.ix_(sub, sub)])
    g = np.array([0, 0, 1, 1, 0, 1], np.int32)
    s = ops.body_penetration(_dev(cs.verts), faces, group=_dev(g))
    got = _by_triple(s.triples.cpu().numpy(), _rows(s.rows))
    print('groups: %d of %d triples left' % (len(got), len(full)))
    assert len(got) == 278 and all(full[k] == b for k, b in got.items())                 # pairs (0,1) and (1,0) only
    assert (s.max_depth.cpu().numpy()[g[:, None] != g[None, :]] == 0).all()


def test_run_to_run(penetration):
    cs = C.case('c24x46')
    B, V = cs.verts.shape[:2]
    first, bo = penetration('c24x46')
    again = bo.depths(_dev(cs.verts))
    flat = lambda r: [r.triples] + list(r.rows) + [r.max_depth, r.sum_depth, r.sum_sq, r.depth_of, r.loss, r.counts, r.inside]
    assert all(torch.equal(a, b) for a, b in zip(flat(first), flat(again)))
    g = _dev(G_UNEVEN)
    for penalty in ('depth', 'squared'):
        Gs = [ops.body_penetration_grad((B, V, 3), bo._handle_for(V), r.triples, r.rows, g, penalty) for r in (first, again, again)]
        assert K.same_bits(Gs[0].cpu().numpy(), Gs[1].cpu().numpy()) and K.same_bits(Gs[1].cpu().numpy(), Gs[2].cpu().numpy())


@pytest.mark.parametrize('penalty', ['depth', 'squared'])
def test_autograd(penalty, penetration):
    """verts = base + t[:, None]: the gradient of sum_i g_i loss_i with respect to t is G.sum(1), which torch adds in fp32 in an order of
    its own: the two differ by at most (V - 1) 2^-24 sum_v |G[i,v]| per component (the bound of any-order summation)."""
    cs = C.case('c12x16')
    B, V = cs.verts.shape[:2]
    res, bo = penetration('c12x16')
    base = _dev(cs.verts)
    t = torch.zeros(B, 3, device=DEV, requires_grad=True)
    verts = base + t[:, None]
    loss = bo.penetration_loss(verts, penalty=penalty)
    assert loss.shape == (B,) and loss.dtype == torch.float32 and loss.requires_grad
    assert torch.equal(loss.detach(), res.loss[ops.BODY_DEPTH_PENALTIES[penalty]])
    g = _dev(G_UNEVEN)
    (loss * g).sum().backward()
    G = ops.body_penetration_grad((B, V, 3), bo._handle_for(V), res.triples, res.rows, g, penalty).cpu().numpy().astype(np.float64)
    err = np.abs(t.grad.cpu().numpy().astype(np.float64) - G.sum(1))
    bound = (V - 1) * 2.0 ** -24 * np.abs(G).sum(1)
    print('%s: loss %s; t.grad %s; largest error / bound %.3g' % (penalty, loss.tolist(), t.grad.cpu().numpy().round(4).tolist(),
                                                                   (err / np.maximum(bound, 1e-30)).max()))
    assert (err <= bound).all() and np.abs(G.sum(1)).max() > 0 and (t.grad[[2, 3, 4]] == 0).all()
    # the op itself, from a faces tensor (the handle then lives as long as the graph) and with a leaf
    leaf = base.clone().requires_grad_(True)
    ops.body_penetration_loss(leaf, torch.tensor(cs.faces), penalty=penalty).sum().backward()
    ones = ops.body_penetration_grad((B, V, 3), bo._handle_for(V), res.triples, res.rows, torch.ones(B, device=DEV), penalty)
    assert torch.equal(leaf.grad, ones)


@pytest.mark.parametrize('what', H.LET_GO)
def test_the_graph_keeps_the_handle_its_evaluator_let_go_of(what, monkeypatch):
    """``BodyOverlap(faces).penetration_loss(verts)`` whose evaluator is deleted, closed or given a batch of another V before
    ``.backward()`` (tests/body_handles_cases.py)."""
    cs, other = C.case('c12x16'), C.case('c24x46')
    assert cs.verts.shape[1] != other.verts.shape[1]
    H.graph_outlives_evaluator(monkeypatch, 'psi_body_overlap_destroy', lambda: evaluation.BodyOverlap(cs.faces, DEV),
                               lambda bo, leaf: bo.penetration_loss(leaf), lambda bo: bo.counts(_dev(other.verts)), _dev(cs.verts),
                               _dev(G_UNEVEN), what)


def test_nothing_inside_and_single_body():
    cs = C.case('c12x16')
    faces = torch.tensor(cs.faces)
    far = cs.verts[0][None] + (3.0 * np.arange(6, dtype=np.float32))[:, None, None] * np.array([1, 0, 0], np.float32)
    near = cs.verts[[1, 4]]                                                              # their boxes meet, nothing is inside
    for verts in (far, near, cs.verts[:1]):
        B = len(verts)
        res = ops.body_penetration(_dev(verts), faces)
        assert res.triples.shape == (0, 3) and all(len(t) == 0 for t in res.rows)
        for t, shape in ((res.max_depth, (B, B)), (res.sum_depth, (B, B)), (res.sum_sq, (B, B)), (res.depth_of, (B, 178)), (res.loss, (2, B))):
            assert tuple(t.shape) == shape and not t.any()
        leaf = _dev(verts).requires_grad_(True)
        loss = ops.body_penetration_loss(leaf, faces)
        loss.sum().backward()
        assert loss.tolist() == [0.0] * B and not leaf.grad.any() and leaf.grad.shape == leaf.shape
    empty = ops.body_depth(_dev(cs.verts), faces, torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert all(len(t) == 0 for t in empty)
    assert not ops.segment_sum3(torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, 3, device=DEV), 4).any()


def test_segment_sum_by_hand():
    """The rows and targets of test_body_depth_cpu.py::test_segment_sum_by_hand, unsorted: a stable sort, then runs added in order."""
    e = 2.0 ** -24
    rows = torch.tensor([[1, 1, -1], [5, 0, 0], [e, 2, 0], [7, 7, 7], [e, 3, 0.5], [0.25, 0, 1]], dtype=torch.float32, device=DEV)
    targets = torch.tensor([3, 1, 3, 0, 3, 1], device=DEV)
    srt = torch.sort(targets, stable=True)
    out = ops.segment_sum3(srt.values, rows, 5, order=srt.indices).cpu().numpy()
    assert K.same_bits(out, D.segment_sum3(targets.cpu().numpy(), rows.cpu().numpy(), 5)) and out[3].tolist() == [1.0, 6.0, -0.5]
    assert K.same_bits(ops.segment_sum3(srt.values, rows[srt.indices].contiguous(), 5).cpu().numpy(), out)
    wild = ops.segment_sum3(torch.tensor([-1, 2, 2, 9], device=DEV), rows[:4].contiguous(), 5).cpu().numpy()      # targets outside are ignored
    assert wild[2].tolist() == [5.0, 2.0, 0.0] and not wild[[0, 1, 3, 4]].any()                 # 5 + 2^-24 rounds to 5


def test_workload_face_count_against_the_analytic_capsule():
    """make_capsule_mesh(68, 156): F = 20 904 (11 slices), the six poses.  The arbiter is the analytic capsule and the tessellation bound
    m = r ((1 - cos(pi / 68)) + (1 - cos(pi / 156))) = 2.0e-4 m: the exact mesh depth D of an inside vertex obeys cap - m <= D <= cap (the
    derivation stands in test_body_depth_cpu.py), and fp32 d2 is within T = TOL_D2_WORKLOAD of D^2 (body_depth_cases.py has how T was
    obtained for this mesh), so sqrt(max((cap - m)^2 - T, 0)) <= depth <= sqrt(cap^2 + T).  Triples within 3e-4 m of the capsule's
    surface, where the overlap decision itself is open (test_body_overlap_gpu.py), get no bound from cap: theirs only has to be below
    3e-4 + sqrt(T)."""
    v, f = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)
    verts = C.posed(v)
    res = ops.body_penetration(_dev(verts), torch.tensor(f))
    trip, depth = res.triples.cpu().numpy(), res.rows.depth.cpu().numpy().astype(np.float64)
    m = K.tessellation_bound(*C.WORKLOAD)
    cap = np.empty(len(trip))
    for j in range(6):
        sel = trip[:, 1] == j
        cap[sel] = -C.capsule_sdf(verts[trip[sel, 0], trip[sel, 2]], j)
    T = K.TOL_D2_WORKLOAD
    lo = np.sqrt(np.maximum(np.maximum(cap - m, 0) ** 2 - T, 0))
    hi = np.sqrt(np.maximum(cap, 0) ** 2 + T)
    band = cap <= K.WORKLOAD_BAND
    print('workload: %d inside triples (%d in the band), m %.3g, cap - depth in [%.3g, %.3g], deepest %.4f m, regions %s'
          % (len(trip), band.sum(), m, (cap - depth)[~band].min(), (cap - depth)[~band].max(), depth.max(),
             np.bincount(res.rows.region.cpu().numpy(), minlength=7).tolist()))
    assert len(trip) == int(res.counts.sum()) and 10000 < len(trip) < 10300 and band.sum() <= 30
    assert ((depth >= lo) & (depth <= hi))[~band].all()
    assert (depth[band] <= K.WORKLOAD_BAND + np.sqrt(T)).all() and np.isfinite(depth).all()
    assert abs(float(res.max_depth.max()) - depth.max()) == 0 and float(res.sum_depth.sum()) > 0


def test_refusals_leave_the_handle_usable():
    cs = C.case('c12x16')
    V = cs.verts.shape[1]
    h = ops.body_overlap_create(cs.faces, V)
    try:
        good, trip = _dev(cs.verts), K.triples('c12x16', 'all')
        swapped, same, far, neg, twice = trip.copy(), trip.copy(), trip.copy(), trip.copy(), trip.copy()
        swapped[[3, 4]] = swapped[[4, 3]]
        same[7, 1] = same[7, 0]
        far[-1, 2] = V
        neg[0, 0] = -1
        twice[10] = twice[9]
        for bad in (swapped, same, far, neg, twice, np.where(trip == 5, 6, trip).astype(np.int32)):
            with pytest.raises(ValueError, match='triples'):
                ops.body_depth(good, h, _dev(bad))
        with pytest.raises(ValueError):
            ops.body_depth(good, h, torch.tensor(trip))                                # triples on another device
        with pytest.raises(ValueError):
            ops.body_depth(good[:, :-1].contiguous(), h, _dev(trip))                   # another vertex count than the handle's
        with pytest.raises(hip.PsiHipError):
            ops.body_depth(good.cpu(), h, torch.tensor(trip))
        with pytest.raises(hip.PsiHipError):
            ops.body_penetration_loss(good.transpose(0, 1).contiguous().transpose(0, 1), h)      # not contiguous
        bad = good.clone()
        bad[2, 3, 0] = float('inf')
        with pytest.raises(ValueError, match='body 2 '):
            ops.body_penetration(bad, h)
        with pytest.raises(ValueError):
            ops.body_penetration_loss(good, h, penalty='l2')
        got = _rows(ops.body_depth(good, h, _dev(trip)))
        assert not any(_differing(got, K.ref('c12x16', 'all')).values())
    finally:
        ops.body_overlap_destroy(h)


def test_eval_script_with_depth_end_to_end(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_eval_body_overlap as E
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    gen = os.path.join(str(tmp_path), 'gen')
    os.makedirs(gen)
    for i in range(4):
        rec = synth.make_bodies(40 + i, 1)
        rec['transl'] = (rec['transl'] * 0.2 + np.array([6.0 * (i // 2), 0.0, 0.0])).astype(np.float32)      # two clusters 6 m apart
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump(rec, f)
    out = str(tmp_path / 'depth.json')
    plain = E.main([gen, '--synthetic', str(tmp_path / 'syn'), '--no_flip'])
    rep = E.main([gen, '--synthetic', str(tmp_path / 'syn'), '--no_flip', '--depth', '--tol', '0.01', '--out', out])
    assert json.load(open(out)) == rep and {k: rep[k] for k in plain} == plain          # the old fields are what they were
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    decoder = S.BodyDecoder(synth.make_smplx(7), synth.make_vposer_state(3), torch.device(DEV, torch.cuda.current_device()))
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    res = ops.body_penetration(verts, decoder.faces.to(torch.int32))
    print('script: pairs %s, deepest %s, shallow %s' % (rep['depth_pairs'], rep['deepest'], rep['shallow']))
    assert rep['max_depth'] == res.max_depth.cpu().double().tolist() and rep['deepest'] == res.depth_of.max(1).values.cpu().double().tolist()
    assert rep['shallow'] == D.select_shallow(range(4), res.max_depth.cpu().numpy(), 0.01) and rep['tol'] == 0.01
    assert [p[:2] for p in rep['depth_pairs']] == [[i, j] for i in range(4) for j in range(4) if plain['counts'][i][j]] and rep['depth_pairs']
    assert all(0 < mean <= mx for _, _, mx, mean in rep['depth_pairs']) and {0, 2} <= set(rep['shallow'])
