"""The conic distance field of crossing triangle pairs on the GPU: rows, aggregates and gradient bit for bit against
the fp32 NumPy restatement, independence of the batch, of groups and of the handle's face order, run to run, brute against pruned,
autograd, the empty results, the planted zeros, the refusals and the entry script."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import body_handles_cases as H
import crossing_field_cases as K
import crossing_field_ref as FR
import surface_crossings_cases as SC
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


def _handle(cs, **kw):
    return ops.surface_crossings_create(cs.faces, cs.verts.shape[1], face_part=cs.kw.get('face_part'), part_skip=cs.kw.get('part_skip'), **kw)


def _flags(cs):
    return {k: v for k, v in cs.kw.items() if k in ('self_pairs', 'between')}


def _host(res):
    """A CrossingFieldResult as host arrays: pairs, psi, energy, pair_energy, loss."""
    assert isinstance(res, ops.CrossingFieldResult) and isinstance(res.rows, ops.FieldRows)
    n, B = res.crossings.pairs.shape[0], res.loss.shape[0]
    assert res.rows.energy.shape == (n, 2) and res.rows.psi.shape == (n, 2, 3) and res.pair_energy.shape == (B, B)
    assert (res.rows.energy.dtype, res.rows.psi.dtype, res.pair_energy.dtype, res.loss.dtype) == (torch.float32, torch.float32, torch.float64, torch.float32)
    return dict(pairs=res.crossings.pairs.cpu().numpy(), psi=res.rows.psi.cpu().numpy(), energy=res.rows.energy.cpu().numpy(),
                pair_energy=res.pair_energy.cpu().numpy(), loss=res.loss.cpu().numpy())


def _same(a, b, keys=('pairs', 'psi', 'energy', 'pair_energy', 'loss')):
    return all(K.same_bits(a[k], b[k]) for k in keys)


def _row_bits(got, relabel=None, face_map=None):
    """{(i, s, j, t) with (i, s) < (j, t): the bits of energy[2] and psi[2,3] in that orientation}"""
    p = np.asarray(got['pairs'], np.int64)
    i, s, j, t = p.T
    if relabel is not None:
        i, j = np.asarray(relabel)[i], np.asarray(relabel)[j]
    if face_map is not None:
        s, t = np.asarray(face_map)[s], np.asarray(face_map)[t]
    swap = (i > j) | ((i == j) & (s > t))
    e, q = got['energy'].view(np.uint32), got['psi'].view(np.uint32)
    out = {}
    for k in range(len(p)):
        key = (int(j[k]), int(t[k]), int(i[k]), int(s[k])) if swap[k] else (int(i[k]), int(s[k]), int(j[k]), int(t[k]))
        ek, qk = (e[k, ::-1], q[k, ::-1]) if swap[k] else (e[k], q[k])
        out[key] = (tuple(ek.tolist()), tuple(qk.reshape(-1).tolist()))
    return out


@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('name,res', K.CASES)
def test_cases_bit_for_bit_and_brute_against_pruned(name, res, sigma):
    cs, r = SC.case(name, res), K.ref(name, res, sigma)
    verts = _t(cs.verts)
    h = _handle(cs)
    try:
        got = _host(ops.crossing_penetration(verts, h, sigma=sigma, **_flags(cs)))
        brute = _host(ops.crossing_penetration(verts, h, sigma=sigma, mode='brute', **_flags(cs)))
        rows = ops.crossing_field(verts, h, _t(r.pairs), sigma=sigma)
        G = {g: ops.crossing_field_grad(verts, h, _t(r.pairs), _t(r.g[g]), sigma=sigma).cpu().numpy() for g in ('ones', 'uneven')}
    finally:
        ops.surface_crossings_destroy(h)
    bad = {k: int((np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(getattr(r, k)).view(np.uint8)).sum())
           for k in ('psi', 'energy', 'pair_energy', 'loss')} if np.array_equal(got['pairs'], r.pairs) else None
    print('%s %s sigma %g: %d pairs, bytes that differ %s, loss %s' % (name, res, sigma, len(got['pairs']), bad, got['loss'].tolist()))
    assert bad is not None and not any(bad.values())
    assert _same(got, brute)
    assert K.same_bits(rows.psi.cpu().numpy(), r.psi) and K.same_bits(rows.energy.cpu().numpy(), r.energy)
    for g in ('ones', 'uneven'):
        print('   G %s: %d values with other bits, largest %.4g' % (g, int((G[g].view(np.uint32) != r.G[g].view(np.uint32)).sum()), np.abs(G[g]).max()))
        assert K.same_bits(G[g], r.G[g])
    assert got['loss'].max() > 0


@pytest.mark.parametrize('sigma', K.SIGMAS)
def test_all_candidates_of_a_case(sigma):
    """Both gates: the candidate list holds many evaluations with h >= sigma or Phi >= 1."""
    cs, r = SC.case('six', '12x16'), K.ref('six', '12x16', sigma, 'cand')
    rows = ops.crossing_field(_t(cs.verts), cs.faces, _t(r.pairs), sigma=sigma)
    G = ops.crossing_field_grad(_t(cs.verts), _crossings_handle_once(cs), _t(r.pairs), _t(r.g['uneven']), sigma=sigma).cpu().numpy()
    assert K.same_bits(rows.psi.cpu().numpy(), r.psi) and K.same_bits(rows.energy.cpu().numpy(), r.energy) and K.same_bits(G, r.G['uneven'])
    assert (r.psi == 0).mean() > 0.2


_HANDLES = {}


def _crossings_handle_once(cs):
    """One handle per case for the tests that pass it on (freed when the process ends with its context)."""
    if id(cs) not in _HANDLES:
        _HANDLES[id(cs)] = _handle(cs)
    return _HANDLES[id(cs)]


def test_row_bits_do_not_depend_on_batch_groups_or_face_order():
    sigma = 1e-3
    cs = SC.case('six', '24x46')
    full = _host(ops.crossing_penetration(_t(cs.verts), cs.faces, self_pairs=False, sigma=sigma))
    rows = _row_bits(full)
    assert len(rows) == 519
    for sub in ([0, 5], [1, 5], [5, 3, 1, 0, 4, 2]):
        got = _host(ops.crossing_penetration(_t(cs.verts[sub]), cs.faces, self_pairs=False, sigma=sigma))
        mine = _row_bits(got, relabel=sub)
        want = {k: v for k, v in rows.items() if k[0] in sub and k[2] in sub}
        print('bodies %s: %d pairs, %d with other bits' % (sub, len(mine), sum(mine[k] != want.get(k) for k in mine)))
        assert mine == want and len(mine) > 0
    g = np.array([0, 0, 1, 1, 0, 1], np.int32)
    grouped = _host(ops.crossing_penetration(_t(cs.verts), cs.faces, group=_t(g), self_pairs=False, sigma=sigma))
    assert _row_bits(grouped) == {k: v for k, v in rows.items() if g[k[0]] == g[k[2]]} and len(grouped['pairs']) == 154
    h = ops.surface_crossings_create(cs.faces, cs.verts.shape[1], order_verts=SC.mesh('24x46')[0])
    try:
        assert _same(_host(ops.crossing_penetration(_t(cs.verts), h, self_pairs=False, sigma=sigma)), full)
    finally:
        ops.surface_crossings_destroy(h)
    perm = np.random.RandomState(11).permutation(len(cs.faces))
    h = ops.surface_crossings_create(np.ascontiguousarray(cs.faces[perm]), cs.verts.shape[1])
    try:
        shuffled = _host(ops.crossing_penetration(_t(cs.verts), h, self_pairs=False, sigma=sigma))
    finally:
        ops.surface_crossings_destroy(h)
    assert _row_bits(shuffled, face_map=perm) == rows
    # self pairs on a Morton-ordered handle with the part filter
    cs = SC.case('fold_parts', '12x16')
    r = K.ref('fold_parts', '12x16', sigma)
    h = _handle(cs, order_verts=SC.mesh('12x16')[0])
    try:
        got = _host(ops.crossing_penetration(_t(cs.verts), h, sigma=sigma, **_flags(cs)))
    finally:
        ops.surface_crossings_destroy(h)
    assert all(K.same_bits(got[k], getattr(r, k)) for k in got)


def test_run_to_run():
    cs = SC.case('six', '24x46')
    verts, g = _t(cs.verts), _t(K.uneven_g(6))
    h = _crossings_handle_once(cs)
    a, b = (ops.crossing_penetration(verts, h, sigma=1e-3) for _ in range(2))
    assert _same(_host(a), _host(b))
    Ga, Gb = (ops.crossing_field_grad(verts, h, a.crossings.pairs, g, sigma=1e-3) for _ in range(2))
    assert torch.equal(Ga.view(torch.int32), Gb.view(torch.int32)) and Ga.abs().max().item() > 0


@pytest.mark.parametrize('sigma', K.SIGMAS)
def test_autograd(sigma):
    """verts = base + t[:,None]: t.grad equals G.sum(1) within the bound of any-order fp32 summation, (V - 1) eps sum |G| per component
    (torch's reduction of the V rows against the fp64 sum of the same rows).  Then self pairs only: the gradient stays in one body."""
    cs, r = SC.case('six', '12x16'), K.ref('six', '12x16', sigma)
    base = _t(cs.verts)
    t = torch.zeros(6, 3, device=DEV, requires_grad=True)
    w = _t(K.uneven_g(6))
    h = _crossings_handle_once(cs)
    loss = ops.crossing_penetration_loss(base + t[:, None], h, self_pairs=False, sigma=sigma)
    assert K.same_bits(loss.detach().cpu().numpy(), r.loss)
    (loss * w).sum().backward()
    G64 = r.G['uneven'].astype(np.float64)
    V = G64.shape[1]
    bound = (V - 1) * 2.0 ** -24 * np.abs(G64).sum(1) + 1e-30
    err = np.abs(t.grad.cpu().numpy().astype(np.float64) - G64.sum(1))
    print('sigma %g: t.grad against G.sum(1): largest error / bound %.3g' % (sigma, (err / bound).max()))
    assert (err <= bound).all() and np.abs(t.grad.cpu().numpy()).max() > 0
    # through the evaluation class with faces given as a tensor, and a leaf verts
    cs, r = SC.case('fold', '12x16'), K.ref('fold', '12x16', sigma)
    sc = evaluation.SurfaceCrossings(cs.faces, DEV)
    v = _t(cs.verts).requires_grad_(True)
    loss = sc.penetration_loss(v, between=False, sigma=sigma)
    loss.sum().backward()
    assert K.same_bits(loss.detach().cpu().numpy(), r.loss) and K.same_bits(v.grad.cpu().numpy(), r.G['ones'])
    two = torch.cat([_t(cs.verts), _t(cs.verts) + 5.0]).requires_grad_(True)
    ops.crossing_penetration_loss(two, torch.tensor(cs.faces), between=False, sigma=sigma)[0].backward()
    assert K.same_bits(two.grad[0].cpu().numpy(), r.G['ones'][0]) and not two.grad[1].any().item()
    sc.close()


@pytest.mark.parametrize('what', H.LET_GO)
def test_the_graph_keeps_the_handle_its_evaluator_let_go_of(what, monkeypatch):
    """``SurfaceCrossings(faces).penetration_loss(verts)`` whose evaluator is deleted, closed or given a batch of another V before
    ``.backward()`` (tests/body_handles_cases.py)."""
    cs, other = SC.case('six', '12x16'), SC.case('six', '24x46')
    assert cs.verts.shape[1] != other.verts.shape[1]
    H.graph_outlives_evaluator(monkeypatch, 'psi_surface_crossings_destroy', lambda: evaluation.SurfaceCrossings(cs.faces, DEV),
                               lambda sc, leaf: sc.penetration_loss(leaf, self_pairs=False, sigma=0.5), lambda sc: sc.crossings(_t(other.verts)),
                               _t(cs.verts), _t(K.uneven_g(6)), what)


def test_empty_results_launch_nothing():
    """Batches with no crossing, and B = 1 without self crossings: zeros, a zero gradient, and no launch (an empty grid would be an error of
    the launch; the library refuses n = 0 outright)."""
    cs = SC.case('six', '12x16')
    far = cs.verts[0][None] + (3.0 * np.arange(6, dtype=np.float32))[:, None, None] * np.array([1, 0, 0], np.float32)
    for verts, kw in ((cs.verts[:1], {}), (far, {}), (cs.verts[[1, 4]], dict(self_pairs=False)), (cs.verts, dict(self_pairs=False, between=False))):
        v = _t(verts).requires_grad_(True)
        res = ops.crossing_penetration(v.detach(), cs.faces, **kw)
        got = _host(res)
        assert got['pairs'].shape == (0, 4) and got['psi'].shape == (0, 2, 3) and got['energy'].shape == (0, 2)
        assert not got['pair_energy'].any() and not got['loss'].any()
        loss = ops.crossing_penetration_loss(v, torch.tensor(cs.faces), **kw)
        loss.sum().backward()
        assert not loss.any().item() and v.grad.shape == v.shape and not v.grad.any().item()
    empty = torch.empty(0, 4, dtype=torch.int32, device=DEV)
    rows = ops.crossing_field(_t(cs.verts), cs.faces, empty)
    assert rows.energy.shape == (0, 2) and rows.psi.shape == (0, 2, 3)
    h = _crossings_handle_once(cs)
    assert not ops.crossing_field_grad(_t(cs.verts), h, empty, _t(K.uneven_g(6))).any().item()
    L, z = hip.lib(), torch.zeros(64, dtype=torch.int64, device=DEV)
    assert L.psi_crossing_field_eval(h, hip.ptr(z), 6, hip.ptr(z), 0, 1e-3, hip.ptr(z), hip.ptr(z), None) == -22
    assert L.psi_crossing_field_grad_rows(h, hip.ptr(z), 6, hip.ptr(z), 0, 1e-3, hip.ptr(z), hip.ptr(z), hip.ptr(z), None) == -22
    assert L.psi_crossing_field_pairs(h, 6, hip.ptr(z), 0, hip.ptr(z), hip.ptr(z), hip.ptr(z), hip.ptr(z), hip.ptr(z), hip.ptr(z), None) == -22
    torch.cuda.synchronize()


def test_thin_has_a_loss_where_the_vertex_test_has_none():
    """Why the feature exists: the thin capsule passes through the trunk of the fat one between its vertices.  body_penetration_loss is
    zero with a zero gradient; the crossing field's loss is positive for both bodies and has a gradient."""
    cs = SC.case('thin')
    v = _t(cs.verts).requires_grad_(True)
    old = ops.body_penetration_loss(v, torch.tensor(cs.faces))
    new = ops.crossing_penetration_loss(v, torch.tensor(cs.faces))
    new.sum().backward()
    print('thin: body_penetration_loss %s, crossing_penetration_loss %s' % (old.tolist(), new.tolist()))
    assert not old.any().item() and (new > 0).all().item() and v.grad.abs().max().item() > 0
    assert K.same_bits(new.detach().cpu().numpy(), K.ref('thin', '12x16', 1e-3).loss)


def test_planted_zeros():
    verts, faces, pairs, psi0 = K.planted()
    r = K.FieldRef(verts, faces, pairs, 0.5)
    h = ops.surface_crossings_create(faces, verts.shape[1])
    try:
        d_verts, d_pairs, d_g = _t(verts), _t(pairs), _t(r.g['uneven'])
        rows = ops.crossing_field(d_verts, h, d_pairs, sigma=0.5)
        G = ops.crossing_field_grad(d_verts, h, d_pairs, d_g, sigma=0.5).cpu().numpy()
        targets = torch.empty(72, dtype=torch.int64, device=DEV)
        grows = torch.empty(72, 3, dtype=torch.float32, device=DEV)
        hip.check(hip.lib().psi_crossing_field_grad_rows(h, hip.ptr(d_verts), 2, hip.ptr(d_pairs), 6, 0.5, hip.ptr(d_g), hip.ptr(targets),
                                                         hip.ptr(grows), hip.stream()), 'grad_rows')
        torch.cuda.synchronize()
    finally:
        ops.surface_crossings_destroy(h)
    psi = rows.psi.cpu().numpy()
    assert K.same_bits(psi[:, 0], psi0) and K.same_bits(psi, r.psi) and K.same_bits(rows.energy.cpu().numpy(), r.energy) and K.same_bits(G, r.G['uneven'])
    grows = grows.cpu().numpy().reshape(6, 2, 6, 3)
    assert K.same_bits(grows.reshape(12, 6, 3), r.rows['uneven']) and np.array_equal(targets.cpu().numpy().reshape(12, 6), r.targets)
    assert K.same_bits(grows[[0, 1, 2, 3, 5], 0], np.zeros((5, 6, 3), np.float32))


def test_workload_face_count_rows_against_restatement():
    """make_capsule_mesh(68, 156): F = 20 904, bodies POSES[0], [1], [5], self + between, on a Morton-ordered handle: the reported rows equal
    the restatement's on the reported pairs."""
    v, f = synth.make_capsule_mesh(*SC.WORKLOAD, SC.RADIUS, SC.HEIGHT)
    verts = SC.BC.posed(v, [SC.POSES[k] for k in (0, 1, 5)])
    h = ops.surface_crossings_create(f, len(v), order_verts=v)
    try:
        got = _host(ops.crossing_penetration(_t(verts), h))
    finally:
        ops.surface_crossings_destroy(h)
    psi, energy = FR.field(verts, f, got['pairs'], 1e-3)
    print('workload: %d pairs, loss %s' % (len(got['pairs']), got['loss'].tolist()))
    assert len(got['pairs']) > 1000 and K.same_bits(got['psi'], psi) and K.same_bits(got['energy'], energy)


def test_refusals_leave_the_handle_usable():
    cs, r = SC.case('six', '12x16'), K.ref('six', '12x16', 1e-3)
    V, F = cs.verts.shape[1], len(cs.faces)
    h = ops.surface_crossings_create(cs.faces, V)
    try:
        good, pairs = _t(cs.verts), _t(r.pairs)
        p = r.pairs
        for bad in (p[::-1], np.concatenate([p[:1], p[:1]]), np.array([[1, 0, 0, 0]], np.int32), np.array([[0, 0, 6, 0]], np.int32),
                    np.array([[0, F, 1, 0]], np.int32), np.array([[0, 0, 1, -1]], np.int32), np.array([[-1, 0, 1, 0]], np.int32)):
            with pytest.raises(ValueError, match='ascending'):
                ops.crossing_field(good, h, _t(bad))
        with pytest.raises(ValueError):
            ops.crossing_field(good, h, pairs.cpu())                                       # the pairs on another device
        with pytest.raises(ValueError):
            ops.crossing_field(good[:, :-1].contiguous(), h, pairs)                        # another vertex count than the handle's
        for sigma in (0.0, 0.6, float('nan')):
            with pytest.raises(ValueError, match='sigma'):
                ops.crossing_field(good, h, pairs, sigma=sigma)
        with pytest.raises(hip.PsiHipError):
            ops.crossing_field(good.cpu(), h, pairs.cpu())
        with pytest.raises(hip.PsiHipError):
            ops.crossing_penetration_loss(good.transpose(0, 1).contiguous().transpose(0, 1), h)       # not contiguous
        nan = good.clone()
        nan[2, 3, 0] = float('nan')
        with pytest.raises(ValueError, match='body 2 '):
            ops.crossing_penetration(nan, h)
        with pytest.raises(ValueError):
            ops.crossing_field_grad(good, h, pairs, torch.zeros(5, device=DEV))
        L = hip.lib()
        z = torch.zeros(64, dtype=torch.int64, device=DEV)
        assert L.psi_crossing_field_eval(h, hip.ptr(good), 6, hip.ptr(pairs), 199, 0.75, hip.ptr(z), hip.ptr(z), None) == -22
        assert L.psi_crossing_field_eval(h, hip.ptr(good), 46341, hip.ptr(pairs), 199, 0.5, hip.ptr(z), hip.ptr(z), None) == -22
        assert L.psi_crossing_field_eval(h, hip.ptr(good), 6, hip.ptr(pairs) + 4, 198, 0.5, hip.ptr(z), hip.ptr(z), None) == -22
        rows = ops.crossing_field(good, h, pairs)
        assert K.same_bits(rows.psi.cpu().numpy(), r.psi)
    finally:
        ops.surface_crossings_destroy(h)


def test_eval_script_with_field_end_to_end(tmp_path, capsys):
    """utils_eval_body_overlap.py --crossings --self --parts --field on four generated bodies with the stand-in model: without --field the
    report and the printed lines are what they were; with it the new fields equal a direct call on the same vertices."""
    sys.path.insert(0, os.path.join(ROOT, 'psi-release_amd', 'utils'))
    try:
        import utils_eval_body_overlap as E
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    gen = str(tmp_path / 'gen')
    os.makedirs(gen)
    for i in range(4):
        rec = synth.make_bodies(40 + i, 1)
        rec['transl'] = (rec['transl'] * 0.2 + np.array([6.0 * (i // 2), 0.0, 0.0])).astype(np.float32)
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump(rec, f)
    base = [gen, '--synthetic', str(tmp_path / 'syn'), '--no_flip', '--crossings', '--self', '--parts']
    plain = E.main(base)
    plain_lines = capsys.readouterr().out.splitlines()
    out = str(tmp_path / 'field.json')
    rep = E.main(base + ['--field', '--sigma', '0.5', '--out', out])
    lines = capsys.readouterr().out.splitlines()
    assert json.load(open(out)) == rep
    assert {k: rep[k] for k in plain} == plain and lines[:len(plain_lines)] == plain_lines      # nothing that was there has changed
    assert set(rep) - set(plain) == {'field_pairs', 'field_loss', 'field_ranked', 'self_energy', 'sigma'} and rep['sigma'] == 0.5
    assert len(lines) == len(plain_lines) + len(rep['field_pairs']) + 8
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    model = synth.make_smplx(7)
    decoder = S.BodyDecoder(model, synth.make_vposer_state(3), torch.device(DEV, torch.cuda.current_device()))
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    faces = decoder.faces.to(torch.int32).cpu().numpy()
    parents = np.asarray(model.kintree_table)[0].astype(np.int64)
    parents[0] = -1
    h = ops.surface_crossings_create(faces, verts.shape[1], face_part=evaluation.face_parts(model.weights, faces),
                                     part_skip=evaluation.part_skip_matrix(parents, extra=evaluation.SMPLX_SELF_CONTACT_PAIRS))
    try:
        res = ops.crossing_penetration(verts, h, sigma=0.5)
    finally:
        ops.surface_crossings_destroy(h)
    E_, counts = res.pair_energy.cpu().numpy(), res.crossings.counts.cpu().numpy()
    print('script: field pairs %s, loss %s, self %s' % (rep['field_pairs'], rep['field_loss'], rep['self_energy']))
    assert rep['field_pairs'] == [[i, j, float(E_[i, j]), float(E_[j, i])] for i in range(4) for j in range(i + 1, 4) if counts[i, j]]
    assert rep['field_loss'] == res.loss.cpu().double().tolist() and rep['self_energy'] == np.diag(E_).tolist()
    psi, energy = FR.field(verts.cpu().numpy(), faces, res.crossings.pairs.cpu().numpy(), 0.5)
    assert K.same_bits(res.rows.energy.cpu().numpy(), energy) and res.crossings.pairs.shape[0] == rep['triangle_pairs'] > 0
