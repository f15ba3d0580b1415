"""Body against body on the GPU (csrc/body_overlap.hip, ops.body_overlap, evaluation.BodyOverlap): the four table cases against the NumPy
fp64 restatement (tests/body_overlap_ref.py) — candidates row for row, counts and inside exact, w within TOL_W, zero ambiguous candidates
— the bits of w under subsets, a permutation and groups, empty batches, run-to-run determinism, the workload's face count against the
analytic capsule, the case the feature exists for, refusals, and the two entry scripts end to end.

TOL_W = 4 x HOST_ERR = 8.2e-4 (tests/body_overlap_cases.py has how it was obtained).  Every test prints its figures before it asserts."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import body_overlap_cases as C
import body_overlap_ref as R
from psi_release_amd import evaluation, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    """After this module its handles are freed and the blocks PyTorch's caching allocator holds for it go back to the runtime, as
    tests/test_mesh_cloud_gpu.py does and for its reason: tests/test_stress_gpu.py, which runs later in the same process and none of this
    module's code, has been seen to depend on what the allocator holds when its engines call hipMalloc.  This module's largest blocks
    are the scripts' render targets and the workload case's vertices and slice sums."""
    yield
    import gc
    gc.collect()                                                                        # BodyOverlap handles of objects in cycles
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run(verts, faces, group=None):
    """(counts, inside, cand, w) as host arrays."""
    g = None if group is None else torch.tensor(np.asarray(group, np.int32), device=DEV)
    out = ops.body_overlap(torch.tensor(np.ascontiguousarray(verts), device=DEV), torch.tensor(faces), group=g, return_candidates=True)
    assert [t.dtype for t in out] == [torch.int32, torch.bool, torch.int32, torch.float32] and all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _bits_by_triple(cand, w, relabel=None):
    """{(i, j, v): bits of w}, the bodies renamed by ``relabel`` (batch index -> name)."""
    c = np.asarray(cand, np.int64)
    if relabel is not None:
        c = np.stack([np.asarray(relabel)[c[:, 0]], np.asarray(relabel)[c[:, 1]], c[:, 2]], 1)
    return dict(zip(C.triple_keys(c).tolist(), np.asarray(w).view(np.uint32).tolist()))


@pytest.mark.parametrize('name', list(C.TABLE))
def test_table_cases_against_restatement(name):
    cs = C.case(name)
    r_counts, r_inside, r_cand, r_w = cs.ref()
    counts, inside, cand, w = _run(cs.verts, cs.faces)
    same_cand = np.array_equal(cand, r_cand)
    err = float(np.abs(w.astype(np.float64) - r_w).max()) if same_cand else float('nan')
    ambiguous = int((np.abs(r_w - 0.5) <= C.AMBIGUOUS).sum())
    print('%s: %d candidates (restatement %d), gpu vs restatement %.4g (TOL_W %.4g), ambiguous %d, counts %s'
          % (name, len(cand), len(r_cand), err, C.TOL_W, ambiguous, counts[counts > 0].tolist()))
    assert same_cand
    assert ambiguous == 0
    assert err <= C.TOL_W
    assert np.array_equal(counts, r_counts) and np.array_equal(inside, r_inside)
    assert inside.shape == cs.verts.shape[:2] and counts.shape == (6, 6)


def test_w_of_a_triple_does_not_depend_on_the_batch():
    cs = C.case('c24x46')
    counts, inside, cand, w = _run(cs.verts, cs.faces)
    full = _bits_by_triple(cand, w)
    for sub in ([0, 1], [5, 1], [5, 3, 1, 0, 4, 2]):
        s_counts, s_inside, s_cand, s_w = _run(cs.verts[sub], cs.faces)
        got = _bits_by_triple(s_cand, s_w, relabel=sub)
        want = {k: b for k, b in full.items() if (k >> 40) in sub and ((k >> 20) & 0xfffff) in sub}
        print('bodies %s: %d triples, %d with other bits' % (sub, len(got), sum(got[k] != want.get(k) for k in got)))
        assert got == want and len(got) > 0
        assert np.array_equal(s_counts, counts[np.ix_(sub, sub)])
        assert (np.diff(C.triple_keys(s_cand)) > 0).all()                               # ascending in the batch's own numbering
        if len(sub) == 6:
            assert np.array_equal(s_inside, inside[sub])


def test_groups():
    cs = C.case('c24x46')
    counts, inside, cand, w = _run(cs.verts, cs.faces)
    g = np.array([0, 0, 1, 1, 0, 1], np.int32)
    g_counts, g_inside, g_cand, g_w = _run(cs.verts, cs.faces, g)
    assert np.array_equal(g_cand, R.candidates(cs.verts, g))
    cross = g[:, None] != g[None, :]
    print('groups: %d of %d candidates left, counts %s' % (len(g_cand), len(cand), g_counts[g_counts > 0].tolist()))
    assert (g_counts[cross] == 0).all() and g_counts[0, 1] == counts[0, 1] == 139 and g_counts[1, 0] == counts[1, 0] == 139 and g_counts.sum() == 278
    full, got = _bits_by_triple(cand, w), _bits_by_triple(g_cand, g_w)
    assert all(full[k] == b for k, b in got.items()) and {k >> 20 for k in got} >= {(0 << 20) | 1, (1 << 20) | 0}
    assert g_inside[5].sum() == 0 and np.array_equal(g_inside[:2], inside[:2])
    for same in (np.zeros(6, np.int32), np.full(6, 7, np.int32)):
        out = _run(cs.verts, cs.faces, same)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out, (counts, inside, cand, w)))


def test_nothing_overlaps_and_single_body():
    cs = C.case('c12x16')
    far = cs.verts[0][None] + (3.0 * np.arange(6, dtype=np.float32))[:, None, None] * np.array([1, 0, 0], np.float32)
    counts, inside, cand, w = _run(far, cs.faces)
    assert counts.shape == (6, 6) and not counts.any() and inside.shape == (6, 178) and not inside.any() and cand.shape == (0, 3) and w.shape == (0,)
    counts, inside, cand, w = _run(cs.verts[:1], cs.faces)
    assert counts.tolist() == [[0]] and inside.shape == (1, 178) and not inside.any() and len(cand) == 0
    torch.cuda.synchronize()
    res = evaluation.BodyOverlap(cs.faces, DEV).counts(torch.tensor(far, device=DEV))
    assert res.per_body.tolist() == [0] * 6


def test_run_to_run():
    cs = C.case('c24x46')
    a, b = _run(cs.verts, cs.faces), _run(cs.verts, cs.faces)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_workload_face_count_against_the_analytic_capsule():
    """make_capsule_mesh(68, 156): V = 10 454, F = 20 904 (11 slices; the SMPL-X surface has 20 908 faces), the six poses.  The arbiter is the
    analytic capsule: a candidate is inside j iff its signed distance to j's capsule is negative; candidates within BAND = 3e-4 m of that
    surface are left out (the mesh's cone trunk departs from the capsule by r (1 - cos(pi / 68)) = 1.7e-4 m).  At most 0.5 % may be left out;
    the arbiter leaves out 27 of 16 806."""
    BAND = 3e-4
    v, f = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)
    verts = C.posed(v)
    assert verts.shape == (6, 10454, 3) and f.shape == (20904, 3)
    counts, inside, cand, w = _run(verts, f)
    r_cand = R.candidates(verts)
    d = np.empty(len(r_cand))
    for j in range(6):
        sel = r_cand[:, 1] == j
        d[sel] = C.capsule_sdf(verts[r_cand[sel, 0], r_cand[sel, 2]], j)
    left_out = np.abs(d) <= BAND
    per_pair = np.zeros((6, 6), np.int64)
    np.add.at(per_pair, (r_cand[:, 0], r_cand[:, 1]), 1)
    an_counts, lo_counts = np.zeros((6, 6), np.int64), np.zeros((6, 6), np.int64)
    np.add.at(an_counts, (r_cand[d < 0, 0], r_cand[d < 0, 1]), 1)
    np.add.at(lo_counts, (r_cand[left_out, 0], r_cand[left_out, 1]), 1)
    same_cand = np.array_equal(cand, r_cand)
    wrong = int((((w > 0.5) != (d < 0)) & ~left_out).sum()) if same_cand else -1
    print('workload: %d candidates, largest pair %d, left out %d (%.2f %%), wrong decisions outside the band %d; counts %s, analytic %s'
          % (len(r_cand), per_pair.max(), left_out.sum(), 100.0 * left_out.mean(), wrong, counts[counts > 0].tolist(), an_counts[an_counts > 0].tolist()))
    assert len(r_cand) == 16806 and per_pair.max() == 5243
    assert same_cand
    assert left_out.sum() == 27 and left_out.mean() <= 0.005
    assert wrong == 0
    assert (an_counts[0, 1], an_counts[1, 0], an_counts[5, 0], an_counts[5, 1]) == (1321, 1321, 2807, 4756)
    assert (np.abs(counts - an_counts) <= lo_counts).all()
    assert np.isfinite(w).all()


def test_bodies_in_free_space_of_a_room_still_stand_in_each_other():
    """Why the feature exists: bodies 0 and 1, shifted into the free space of the oriented room, have a positive scene distance at every
    vertex (non-collision score 1.0 for both by the reference's metric), yet each has vertices inside the other."""
    cs = C.case('c24x46')
    v, _ = synth.make_capsule_mesh(24, 46, C.RADIUS, C.HEIGHT)
    verts = C.posed(v, C.POSES[:2], shift=(0.0, 0.0, 0.2))
    room = synth.make_oriented_room(2)
    sdf = room.analytic_sdf(verts)
    counts, inside, _, _ = _run(verts, cs.faces)
    print('smallest scene distance %.3f m; counts %s' % (sdf.min(), counts.tolist()))
    assert sdf.min() > 0
    assert counts[0, 1] > 0 and counts[1, 0] > 0 and inside.any(1).all()


def test_refusals_leave_the_handle_usable():
    cs = C.case('c12x16')
    V = cs.verts.shape[1]
    with pytest.raises(hip.PsiHipError):
        ops.body_overlap_create(np.where(cs.faces == 5, V, cs.faces).astype(np.int32), V)
    h = ops.body_overlap_create(cs.faces, V)
    try:
        good = torch.tensor(cs.verts, device=DEV)
        bad = good.clone()
        bad[4, 17, 1] = float('nan')
        bad[2, 3, 0] = float('inf')
        with pytest.raises(ValueError, match='body 2 '):
            ops.body_overlap(bad, h)
        with pytest.raises(ValueError):
            ops.body_overlap(good[:, :-1].contiguous(), h)                              # another vertex count than the handle's
        with pytest.raises(hip.PsiHipError):
            ops.body_overlap(good.cpu(), h)
        with pytest.raises(hip.PsiHipError):
            ops.body_overlap(good.transpose(0, 1).contiguous().transpose(0, 1), h)     # not contiguous
        counts, inside = ops.body_overlap(good, h)
        assert np.array_equal(counts.cpu().numpy(), cs.ref()[0]) and np.array_equal(inside.cpu().numpy(), cs.ref()[1])
    finally:
        ops.body_overlap_destroy(h)


def _scripts():
    sys.path.insert(0, UTILS)
    try:
        import utils_eval_body_overlap as E
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    return E, S


def _gen_folder(tmp, n=4):
    gen = os.path.join(tmp, 'gen')
    os.makedirs(gen)
    for i in range(n):
        rec = synth.make_bodies(40 + i, 1)
        # two clusters 6 m apart: the bodies of a cluster stand in each other, the clusters do not meet
        rec['transl'] = (rec['transl'] * 0.2 + np.array([6.0 * (i // 2), 0.0, 0.0])).astype(np.float32)
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump(rec, f)
    return gen


def test_eval_script_end_to_end(tmp_path):
    E, S = _scripts()
    gen, out = _gen_folder(str(tmp_path)), str(tmp_path / 'overlap.json')
    rep = E.main([gen, '--synthetic', str(tmp_path / 'syn'), '--no_flip', '--out', out])
    on_disk = json.load(open(out))
    assert on_disk == rep and rep['bodies'] == 4
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    decoder = S.BodyDecoder(synth.make_smplx(7), synth.make_vposer_state(3), torch.device(DEV, torch.cuda.current_device()))
    verts = decoder.verts(xh, S.camera_pose(cam, True))
    counts, inside = ops.body_overlap(verts.contiguous(), decoder.faces.to(torch.int32))
    print('script: %d overlapping pairs, per body %s, disjoint %s' % (rep['overlapping_pairs'], rep['per_body'], rep['disjoint']))
    assert rep['counts'] == counts.cpu().tolist() and rep['per_body'] == inside.sum(1).cpu().tolist()
    assert rep['disjoint'] == R.select_disjoint(range(4), counts.cpu().numpy(), 0)
    assert not counts[:2, 2:].any() and not counts[2:, :2].any() and {0, 2} <= set(rep['disjoint']) and rep['overlapping_pairs'] >= 1
    assert rep['overlapping_pairs'] == sum(1 for i in range(4) for j in range(i + 1, 4) if counts[i, j] or counts[j, i])


def test_show_script_disjoint_end_to_end(tmp_path):
    E, S = _scripts()
    gen = _gen_folder(str(tmp_path))
    cam = ['--fixed_cam'] + [str(x) for x in np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 3.0], [0, 0, 0, 1]], np.float64).reshape(-1)]
    base = [gen, '-', None, '--synthetic', str(tmp_path / 'syn'), '--size', '54', '96', '--no_flip', '--together'] + cam
    outs = {}
    for tag, extra in (('plain', []), ('again', []), ('disjoint', ['--disjoint'])):
        outs[tag] = str(tmp_path / tag)
        S.main(base[:2] + [outs[tag]] + base[3:] + extra)
    names = sorted(os.listdir(outs['plain']))
    assert 'img_together.png' in names and 'visibility.json' in names and sorted(os.listdir(outs['disjoint'])) == names
    read = lambda tag, n: open(os.path.join(outs[tag], n), 'rb').read()
    for n in names:                                                                     # without the flag: the same bytes, run after run
        assert read('plain', n) == read('again', n)
    for n in names:
        if n not in ('img_together.png', 'visibility.json'):
            assert read('plain', n) == read('disjoint', n)                             # the flag touches nothing else
    plain, rows = json.load(open(os.path.join(outs['plain'], 'visibility.json'))), json.load(open(os.path.join(outs['disjoint'], 'visibility.json')))
    assert all('inside_others' not in r and 'disjoint' not in r and 'together' in r for r in plain)
    rep = E.main([gen, '--synthetic', str(tmp_path / 'syn'), '--no_flip'])
    print('rows: %s' % [(r['body'], r['inside_others'], r['disjoint']) for r in rows])
    assert [r['inside_others'] for r in rows] == rep['per_body']
    assert [r['body'] for r in rows if r['disjoint']] == rep['disjoint']
    assert all(('together' in r) == r['disjoint'] for r in rows)
    for r, p in zip(rows, plain):
        assert {k: r[k] for k in p if k != 'together'} == {k: p[k] for k in p if k != 'together'}
