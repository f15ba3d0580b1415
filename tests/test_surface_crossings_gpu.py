"""Surface crossings on the GPU (csrc/surface_crossings.hip, ops.surface_crossings, evaluation.SurfaceCrossings): every case of
tests/surface_crossings_cases.py against the NumPy restatement (tests/surface_crossings_ref.py) — pairs row for row, events, counts,
face_hit and irregular exact, length and contour bit-equal — 'brute' against 'pruned' bit for bit, the bits of a pair's row under
sub-batches, a permutation of the bodies, groups, a Morton-ordered handle and a handle on permuted face rows, empty results, run-to-run
determinism, the case the vertex test cannot see, the workload's face count, the refusals, and the entry script end to end.  Every test prints its figures before it
asserts."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import surface_crossings_cases as C
import surface_crossings_ref as R
from psi_release_amd import evaluation, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FIELDS = ('pairs', 'events', 'length', 'counts', 'contour', 'face_hit', 'irregular')
DTYPES = (torch.int32, torch.int32, torch.float32, torch.int32, torch.float64, torch.bool, torch.int32)


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    """As tests/test_body_overlap_gpu.py does, and for its reason: what this module's calls leave in PyTorch's caching allocator goes back
    to the runtime when the module ends."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run(verts, faces_or_handle, group=None, stats=False, **kw):
    """The CrossingsResult as host arrays (irregular as an int), checked for dtype, device and shape."""
    g = None if group is None else torch.tensor(np.asarray(group, np.int32), device=DEV)
    out = ops.surface_crossings(torch.tensor(np.ascontiguousarray(verts), device=DEV), faces_or_handle, group=g, return_stats=stats, **kw)
    res, st = out if stats else (out, None)
    assert isinstance(res, ops.CrossingsResult) and res._fields == FIELDS
    assert tuple(t.dtype for t in res) == DTYPES and all(t.is_cuda for t in res)
    B, n = len(verts), res.pairs.shape[0]
    assert res.pairs.shape == (n, 4) and res.events.shape == (n,) and res.length.shape == (n,) and res.irregular.shape == ()
    assert res.counts.shape == (B, B) and res.contour.shape == (B, B) and res.face_hit.shape[0] == B
    host = ops.CrossingsResult(*(t.cpu().numpy() for t in res[:6]), int(res.irregular.item()))
    return (host, st) if stats else host


def _handle(cs, **kw):
    return ops.surface_crossings_create(cs.faces, cs.verts.shape[1], face_part=cs.kw.get('face_part'), part_skip=cs.kw.get('part_skip'), **kw)


def _flags(cs):
    return {k: v for k, v in cs.kw.items() if k in ('self_pairs', 'between')}


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a[:6], b[:6])) \
        and a.irregular == b.irregular


def _rows(res, relabel=None, face_map=None):
    """{(i, s, j, t) with (i, s) < (j, t): (events, bits of length)}, bodies renamed by ``relabel`` and faces by ``face_map``."""
    p = np.asarray(res.pairs, np.int64)
    i, s, j, t = p.T
    if relabel is not None:
        i, j = np.asarray(relabel)[i], np.asarray(relabel)[j]
    if face_map is not None:
        s, t = np.asarray(face_map)[s], np.asarray(face_map)[t]
    swap = (i > j) | ((i == j) & (s > t))
    i, j, s, t = np.where(swap, j, i), np.where(swap, i, j), np.where(swap, t, s), np.where(swap, s, t)
    return {k: v for k, v in zip(zip(i.tolist(), s.tolist(), j.tolist(), t.tolist()), zip(res.events.tolist(), res.length.view(np.uint32).tolist()))}


CASES = [('six', '12x16'), ('six', '24x46'), ('thin', '12x16'), ('caps', '12x16'), ('caps', '24x46'), ('fold', '12x16'), ('fold', '24x46'),
         ('fold_parts', '12x16'), ('fold_parts', '24x46')]


@pytest.mark.parametrize('name,res', CASES)
def test_cases_against_restatement_and_brute_against_pruned(name, res):
    cs = C.case(name, res)
    r = cs.ref()
    h = _handle(cs)
    try:
        (got, st), (brute, st_b) = _run(cs.verts, h, stats=True, **_flags(cs)), _run(cs.verts, h, stats=True, mode='brute', **_flags(cs))
    finally:
        ops.surface_crossings_destroy(h)
    same_pairs = np.array_equal(got.pairs, r.pairs)
    bad_len = int((got.length.view(np.uint32) != r.length.view(np.uint32)).sum()) if same_pairs else -1
    print('%s %s: %d pairs (restatement %d), tiles %d pruned / %d brute, irregular %d, lengths with other bits %d, contour %s'
          % (name, res, len(got.pairs), len(r.pairs), st['tiles'], st_b['tiles'], got.irregular, bad_len, got.contour[got.contour > 0].tolist()))
    assert same_pairs and np.array_equal(got.events, r.events)
    assert bad_len == 0
    assert np.array_equal(got.counts, r.counts) and np.array_equal(got.face_hit, r.face_hit) and got.irregular == r.irregular
    assert np.array_equal(got.contour.view(np.uint64), r.contour.view(np.uint64))
    assert _same_bits(got, brute) and st['pairs'] == st_b['pairs'] == len(r.pairs) and 0 < st['tiles'] <= st_b['tiles']
    B, nC = len(cs.verts), -(-len(cs.faces) // 256)
    jobs_self, jobs_between = (B if cs.kw.get('self_pairs', True) else 0), (B * (B - 1) // 2 if cs.kw.get('between', True) else 0)
    assert st_b['tiles'] == jobs_self * (nC * (nC + 1) // 2) + jobs_between * nC * nC


def test_row_bits_do_not_depend_on_the_batch():
    cs = C.case('six', '24x46')
    full = _run(cs.verts, cs.faces, self_pairs=False)
    rows = _rows(full)
    assert len(rows) == 519
    for sub in ([0, 5], [1, 5], [5, 3, 1, 0, 4, 2]):
        got = _run(cs.verts[sub], cs.faces, self_pairs=False)
        mine = _rows(got, relabel=sub)
        want = {k: v for k, v in rows.items() if k[0] in sub and k[2] in sub}
        print('bodies %s: %d pairs, %d with other bits' % (sub, len(mine), sum(mine[k] != want.get(k) for k in mine)))
        assert mine == want and len(mine) > 0
        assert C.ascending(got.pairs) and np.array_equal(got.counts, full.counts[np.ix_(sub, sub)])
        assert np.array_equal(got.face_hit, full.face_hit[sub]) if len(sub) == 6 else True
    g = np.array([0, 0, 1, 1, 0, 1], np.int32)
    grouped = _run(cs.verts, cs.faces, group=g, self_pairs=False)
    want = {k: v for k, v in rows.items() if g[k[0]] == g[k[2]]}
    print('groups: %d of %d pairs left' % (len(grouped.pairs), len(full.pairs)))
    assert _rows(grouped) == want and grouped.counts[0, 1] == 154 and grouped.counts.sum() == 308
    for same in (np.zeros(6, np.int32), np.full(6, 7, np.int32)):
        assert _same_bits(_run(cs.verts, cs.faces, group=same, self_pairs=False), full)


@pytest.mark.parametrize('name', ['six', 'fold_parts'])
def test_chunk_order_does_not_change_a_bit(name):
    """A handle built with order_verts (Morton order of the faces) gives the identical result; a handle built on a random permutation of
    the face rows gives the same rows once the indices are mapped back."""
    cs = C.case(name, '24x46')
    h = _handle(cs)
    try:
        plain = _run(cs.verts, h, **_flags(cs))
    finally:
        ops.surface_crossings_destroy(h)
    rest = C.mesh('24x46')[0]
    h = _handle(cs, order_verts=rest)
    try:
        ordered, st = _run(cs.verts, h, stats=True, **_flags(cs))
        ordered_brute = _run(cs.verts, h, mode='brute', **_flags(cs))
    finally:
        ops.surface_crossings_destroy(h)
    print('%s: Morton-ordered handle: %d tiles, %d pairs' % (name, st['tiles'], st['pairs']))
    assert _same_bits(ordered, plain) and _same_bits(ordered_brute, plain) and len(plain.pairs) > 100
    perm = np.random.RandomState(11).permutation(len(cs.faces))
    part = cs.kw.get('face_part')
    h = ops.surface_crossings_create(np.ascontiguousarray(cs.faces[perm]), cs.verts.shape[1], face_part=None if part is None else part[perm],
                                     part_skip=cs.kw.get('part_skip'))
    try:
        shuffled = _run(cs.verts, h, **_flags(cs))
    finally:
        ops.surface_crossings_destroy(h)
    assert _rows(shuffled, face_map=perm) == _rows(plain) and C.ascending(shuffled.pairs)
    assert np.array_equal(shuffled.counts, plain.counts) and np.array_equal(shuffled.face_hit[:, np.argsort(perm)], plain.face_hit)


def test_empty_results():
    """B = 1 with between only, a batch whose boxes do not meet, all flags off, and bodies whose boxes meet but whose surfaces do not cross:
    zeros and empty arrays; a pass with nothing to do is not launched (an empty grid would be an error of the launch)."""
    cs = C.case('six', '12x16')
    far = cs.verts[0][None] + (3.0 * np.arange(6, dtype=np.float32))[:, None, None] * np.array([1, 0, 0], np.float32)
    for verts, kw, tiles_expected in ((cs.verts[:1], dict(self_pairs=False), False), (far, dict(self_pairs=False), False),
                                      (cs.verts, dict(self_pairs=False, between=False), False), (cs.verts[[1, 4]], dict(self_pairs=False), True)):
        for mode in ('pruned', 'brute'):
            got, st = _run(verts, cs.faces, stats=True, mode=mode, **kw)
            print('%d bodies %s %s: %s' % (len(verts), kw, mode, st))
            assert got.pairs.shape == (0, 4) and got.events.shape == (0,) and got.length.shape == (0,) and got.irregular == 0
            assert not got.counts.any() and not got.contour.any() and not got.face_hit.any() and got.face_hit.shape == (len(verts), 352)
            assert st['pairs'] == 0
            if mode == 'pruned':
                assert (st['tiles'] > 0) == tiles_expected
    torch.cuda.synchronize()
    got, st = _run(cs.verts[:1], cs.faces, stats=True)                                     # self pairs of one capsule: tiles, no pair
    assert 0 < st['tiles'] <= 3 and st['pairs'] == 0 and not got.counts.any()


def test_run_to_run():
    cs = C.case('six', '24x46')
    assert _same_bits(_run(cs.verts, cs.faces), _run(cs.verts, cs.faces))
    cs = C.case('fold', '24x46')
    assert _same_bits(_run(cs.verts, cs.faces), _run(cs.verts, cs.faces))


def test_surfaces_cross_although_no_vertex_is_inside():
    """Why the feature exists: the thin capsule passes through the trunk of the fat one between its vertices.  ops.body_overlap counts no
    vertex of either inside the other; 72 pairs of triangles cross."""
    cs = C.case('thin')
    verts = torch.tensor(cs.verts, device=DEV)
    counts, inside = ops.body_overlap(verts, torch.tensor(cs.faces))
    got = _run(cs.verts, cs.faces)
    print('overlap counts %s, crossing pairs %d, contour %.4f m' % (counts.cpu().tolist(), got.counts[0, 1], got.contour[0, 1]))
    assert not counts.any().item() and not inside.any().item()
    assert got.counts.tolist() == [[0, C.THIN_PAIRS], [C.THIN_PAIRS, 0]] and got.irregular == 0 and got.contour[0, 1] > 0


def test_evaluation_class_parts_and_selection():
    verts, faces, upper = C.fold_mesh('24x46')
    skip = evaluation.part_skip_matrix([-1, 0], parent_child=False)
    assert skip.tolist() == [[1, 0], [0, 1]]
    sc = evaluation.SurfaceCrossings(faces, DEV, order_verts=C.mesh('24x46')[0], face_part=upper.astype(np.int32), part_skip=skip)
    plain = evaluation.SurfaceCrossings(faces, DEV)
    away = verts + np.array([3.0, 0.0, 0.0], np.float32)                                    # the folded body, and two bodies that cross
    v = torch.tensor(np.concatenate([away, C.case('six', '24x46').verts[:2]]), device=DEV)
    res, res_plain = sc.crossings(v), plain.crossings(v, group=[0, 0, 0])
    print('with parts: counts %s; without: %s' % (res.counts.cpu().tolist(), res_plain.counts.cpu().tolist()))
    assert res.counts[0, 0].item() == C.FOLD['24x46'][1] and res_plain.counts[0, 0].item() == C.FOLD['24x46'][0]
    assert res.counts[1, 2].item() == res_plain.counts[1, 2].item() == 154 and torch.equal(res.counts, res.counts.T)
    assert res.counts[0, 1:].cpu().tolist() == [0, 0]
    assert evaluation.select_uncrossed(range(3), res.counts) == [0, 1] and evaluation.select_uncrossed([2, 1, 0], res.counts, max_self=0) == [2]
    only_self = sc.crossings(v, between=False)
    assert only_self.counts.cpu().tolist() == [[121, 0, 0], [0, 0, 0], [0, 0, 0]]
    sc.close(), plain.close()


def test_workload_face_count_pruned_against_brute():
    """make_capsule_mesh(68, 156): F = 20 904 (82 chunks), bodies POSES[0], [1], [5], self + between, on a Morton-ordered handle.  'brute'
    (every chunk pair of every job) is the arbiter of the pruning: the same bits.  The reported pairs are then put through the NumPy rule
    (the pairs only: no candidate search at this size): same events and length bits, and on the pairs of (0,5) and (1,5) every
    (edge, triangle) event occurs in exactly two pairs."""
    v, f = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)
    verts = C.BC.posed(v, [C.POSES[k] for k in (0, 1, 5)])
    assert f.shape == (20904, 3)
    h = ops.surface_crossings_create(f, len(v), order_verts=v)
    try:
        (got, st), (brute, st_b) = _run(verts, h, stats=True), _run(verts, h, stats=True, mode='brute')
    finally:
        ops.surface_crossings_destroy(h)
    print('workload: %d pairs, counts %s, irregular %d, tiles %d of %d' % (len(got.pairs), got.counts.tolist(), got.irregular, st['tiles'], st_b['tiles']))
    assert st_b['tiles'] == 3 * (82 * 83 // 2) + 3 * 82 * 82 and 0 < st['tiles'] < st_b['tiles'] // 10
    assert _same_bits(got, brute) and len(got.pairs) > 1000 and C.ascending(got.pairs)
    assert not np.diag(got.counts).any() and got.counts[0, 2] > 0 and got.counts[1, 2] > 0
    P, Q = R.triangles_of(verts, f, got.pairs)
    ev, length, mask = R.events_length(P, Q)
    assert np.array_equal(ev, got.events) and np.array_equal(length.view(np.uint32), got.length.view(np.uint32))
    for i, j in ((0, 2), (1, 2)):
        sel = (got.pairs[:, 0] == i) & (got.pairs[:, 2] == j)
        hist = C.closedness(got.pairs[sel], mask[sel], f)
        print('(%d,%d): %d pairs, occurrences %s' % (i, j, sel.sum(), hist))
        assert list(hist) == [2]


def test_refusals_leave_the_handle_usable():
    cs = C.case('six', '12x16')
    V = cs.verts.shape[1]
    h = ops.surface_crossings_create(cs.faces, V)
    try:
        good = torch.tensor(cs.verts, device=DEV)
        bad = good.clone()
        bad[4, 17, 1] = float('nan')
        bad[2, 3, 0] = float('inf')
        with pytest.raises(ValueError, match='body 2 '):
            ops.surface_crossings(bad, h)
        with pytest.raises(ValueError):
            ops.surface_crossings(good[:, :-1].contiguous(), h)                             # another vertex count than the handle's
        with pytest.raises(ValueError):
            ops.surface_crossings(good, h, group=torch.zeros(6, dtype=torch.int32))        # the group on another device
        with pytest.raises(hip.PsiHipError):
            ops.surface_crossings(good.cpu(), h)
        with pytest.raises(hip.PsiHipError):
            ops.surface_crossings(good.transpose(0, 1).contiguous().transpose(0, 1), h)    # not contiguous
        # the library's own bounds
        L = hip.lib()
        t = torch.zeros(16, dtype=torch.int32, device=DEV)
        assert L.psi_surface_crossings_boxes(h, hip.ptr(good), 46341, hip.ptr(t), hip.ptr(t), hip.ptr(t), None) == -22
        assert L.psi_surface_crossings_test(h, hip.ptr(good), 6, hip.ptr(t), 0, hip.ptr(t), None, 0, None, None, None, None) == -22
        assert L.psi_surface_crossings_tiles(h, None, 6, 8, hip.ptr(t), hip.ptr(t), hip.ptr(t), None, 0, None, None) == -22
        got = _run(cs.verts, h, self_pairs=False)
        r = cs.ref()
        assert np.array_equal(got.pairs, r.pairs) and np.array_equal(got.length.view(np.uint32), r.length.view(np.uint32))
    finally:
        ops.surface_crossings_destroy(h)


def test_eval_script_with_crossings_end_to_end(tmp_path, capsys):
    """utils_eval_body_overlap.py on four generated bodies in two clusters 6 m apart, with the stand-in model (64 random faces over a
    cloud of vertices): without --crossings the report and the printed lines are what they were; with it the new fields equal a direct
    call on the same vertices, and the clusters do not cross each other."""
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
    base = [gen, '--synthetic', str(tmp_path / 'syn'), '--no_flip']
    plain = E.main(base)
    plain_lines = capsys.readouterr().out.splitlines()
    out = str(tmp_path / 'crossings.json')
    rep = E.main(base + ['--crossings', '--self', '--parts', '--out', out])
    lines = capsys.readouterr().out.splitlines()
    assert json.load(open(out)) == rep
    assert {k: rep[k] for k in plain} == plain and lines[:len(plain_lines)] == plain_lines      # nothing that was there has changed
    new = set(rep) - set(plain)
    assert new == {'crossing_pairs', 'crossing_counts', 'contour', 'self_crossings', 'self_ranked', 'irregular', 'triangle_pairs', 'unseen_by_vertex_test'}
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    model = synth.make_smplx(7)
    decoder = S.BodyDecoder(model, synth.make_vposer_state(3), torch.device(DEV, torch.cuda.current_device()))
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    faces = decoder.faces.to(torch.int32).cpu().numpy()
    parents = np.asarray(model.kintree_table)[0].astype(np.int64)
    parents[0] = -1
    part = evaluation.face_parts(model.weights, faces)
    skip = evaluation.part_skip_matrix(parents, extra=evaluation.SMPLX_SELF_CONTACT_PAIRS)
    h = ops.surface_crossings_create(faces, verts.shape[1], face_part=part, part_skip=skip)
    try:
        res = ops.surface_crossings(verts, h)
    finally:
        ops.surface_crossings_destroy(h)
    counts = res.counts.cpu().numpy()
    print('script: triangle pairs %d, crossing body pairs %s, self %s, unseen %d' % (rep['triangle_pairs'], rep['crossing_pairs'],
                                                                                 rep['self_crossings'], rep['unseen_by_vertex_test']))
    assert rep['crossing_counts'] == counts.tolist() and rep['triangle_pairs'] == res.pairs.shape[0] and rep['irregular'] == int(res.irregular)
    assert rep['contour'] == res.contour.cpu().tolist() and rep['self_crossings'] == np.diag(counts).tolist()
    assert [p[:3] for p in rep['crossing_pairs']] == [[i, j, int(counts[i, j])] for i in range(4) for j in range(i + 1, 4) if counts[i, j]]
    assert not counts[:2, 2:].any()
    ov = np.asarray(plain['counts'])
    assert rep['unseen_by_vertex_test'] == sum(1 for i, j, _, _ in rep['crossing_pairs'] if ov[i, j] == 0 and ov[j, i] == 0)
    with pytest.raises(SystemExit):
        E.parse_args([gen, '--self'])
    with pytest.raises(SystemExit):
        E.parse_args([gen, '--crossings', '--parts'])
