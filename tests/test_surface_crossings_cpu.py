"""Surface crossings without a GPU: the NumPy restatement (tests/surface_crossings_ref.py) in float32 against the same rule in float64 and
against an independent fp64 / exact statement on every candidate of every case, the pinned counts of tests/surface_crossings_cases.py,
the contour of two crossing caps against the circle, closedness, role-swap bit identity, self mode against between mode on the folded
capsule, the statements of csrc/surface_crossings_shared.h run serially on the host (tools/surface_crossings_host_check.hip) bit for bit
against the restatement, the part helpers and ``select_uncrossed`` by hand, the new symbols and the refusals that need no GPU.

Nothing is excluded anywhere: no candidate is left out of a comparison for being close to a decision."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import body_overlap_ref as BR
import surface_crossings_cases as C
import surface_crossings_ref as R

SYMBOLS = ['psi_surface_crossings_' + s for s in ('face_order', 'create', 'destroy', 'info', 'boxes', 'tiles', 'test', 'finish')]
ALL_CASES = [('six', '12x16'), ('six', '24x46'), ('thin', '12x16'), ('caps', '12x16'), ('caps', '24x46'), ('caps', '48x92'),
             ('fold', '12x16'), ('fold', '24x46'), ('fold_parts', '12x16'), ('fold_parts', '24x46')]


@pytest.mark.parametrize('name,res', ALL_CASES)
def test_restatement_against_float64_and_independent_statement(name, res):
    """Equal events on EVERY candidate: float32 rule = float64 rule = independent statement."""
    cs = C.case(name, res)
    r32, r64 = cs.ref(np.float32), cs.ref(np.float64)
    P, Q = R.triangles_of(cs.verts, cs.faces, r32.cand)
    ind, ind_mask = R.independent_events(P, Q)
    mask32 = R.events_length(P, Q, np.float32)[2]
    print('%s %s: %d candidates, %d crossing pairs, fp32 != fp64 on %d, fp32 != independent on %d' % (
        name, res, len(r32.cand), len(r32.pairs), (r32.cand_events != r64.cand_events).sum(), (ind != r32.cand_events).sum()))
    assert np.array_equal(r32.cand, r64.cand) and len(r32.cand) > 0
    assert np.array_equal(r32.cand_events, r64.cand_events)
    assert np.array_equal(ind, r32.cand_events) and np.array_equal(ind_mask, mask32)       # edge for edge, not only the count
    assert np.array_equal(r32.pairs, r64.pairs) and C.ascending(r32.pairs) and C.ascending(r32.cand)
    rel = np.abs(r32.length.astype(np.float64) - r64.length) / np.maximum(r64.length, 1e-30)
    assert (rel[r64.length > 1e-3] < 1e-3).all()                                            # a sanity bound, not the contract


def test_every_face_pair_not_only_the_candidates():
    """six at 12 x 16: fp32 = fp64 = independent on EVERY face pair of all fifteen body pairs (15 x 352^2), and a pair whose face boxes do not
    meet has no event: the candidate rule loses nothing."""
    cs = C.case('six', '12x16')
    F = len(cs.faces)
    tri = cs.verts[:, cs.faces]
    s, t = np.divmod(np.arange(F * F), F)
    cand_keys = set(C.pair_keys(cs.ref().cand).tolist())
    total = 0
    for i in range(6):
        for j in range(i + 1, 6):
            P, Q = tri[i, s], tri[j, t]
            e32, e64, ind = R.events_length(P, Q, np.float32)[0], R.events_length(P, Q, np.float64)[0], R.independent_events(P, Q)[0]
            assert np.array_equal(e32, e64) and np.array_equal(e32, ind)
            hit = np.nonzero(e32)[0]
            rows = np.stack([np.full(len(hit), i), s[hit], np.full(len(hit), j), t[hit]], 1)
            assert set(C.pair_keys(rows).tolist()) <= cand_keys
            total += len(hit)
    assert total == len(cs.ref().pairs) == 199


@pytest.mark.parametrize('res', ['12x16', '24x46'])
def test_six_pinned(res):
    cs = C.case('six', res)
    r = cs.ref()
    (c01, c05, c15), one_event = C.SIX[res]
    p = r.pairs
    of = lambda i, j: (p[:, 0] == i) & (p[:, 2] == j)
    print('six %s: F %d, counts (0,1) %d (0,5) %d (1,5) %d, irregular %d' % (res, len(cs.faces), r.counts[0, 1], r.counts[0, 5], r.counts[1, 5],
                                                                             r.irregular))
    assert len(cs.faces) == {'12x16': 352, '24x46': 2116}[res]
    assert (r.counts[0, 1], r.counts[0, 5], r.counts[1, 5]) == (c01, c05, c15)
    assert r.counts.sum() == 2 * (c01 + c05 + c15) and np.array_equal(r.counts, r.counts.T) and not np.diag(r.counts).any()
    assert (r.events[of(0, 5)] == 2).all() and (r.events[of(1, 5)] == 2).all()
    assert (r.events[of(0, 1)] == 1).sum() == one_event == r.irregular                    # rings at equal heights: edges through edges
    lo, hi = cs.verts.min(1), cs.verts.max(1)
    for i, j in ((1, 4), (2, 5)):                                                           # body boxes meet, nothing crosses
        assert (lo[i] <= hi[j]).all() and (lo[j] <= hi[i]).all() and r.counts[i, j] == 0
    assert r.face_hit.sum(1).tolist()[2:5] == [0, 0, 0] and r.face_hit[0].any() and r.face_hit[5].any()
    assert r.contour[0, 5] > 0 and r.contour[0, 5] == r.contour[5, 0]


def test_thin_pinned_and_invisible_to_the_vertex_test():
    """72 crossing pairs, all regular, although no vertex of either capsule lies inside the other: by the analytic capsule distance, and by
    the restatement of BodyOverlap (tests/body_overlap_ref.py), whose counts are zero both ways."""
    cs = C.case('thin')
    r = cs.ref()
    fat, thin = C.thin_vertex_depths()
    counts = BR.overlap(cs.verts, cs.faces)[0]
    print('thin: %d pairs, irregular %d; smallest vertex distance to the other capsule %.4f / %.4f; overlap counts %s'
          % (len(r.pairs), r.irregular, fat.min(), thin.min(), counts.tolist()))
    assert len(r.pairs) == C.THIN_PAIRS == r.counts[0, 1] and r.irregular == 0
    assert fat.min() > 0 and thin.min() > 0
    assert not counts.any()


def test_caps_contour_against_the_circle():
    errs = {}
    for res in C.RESOLUTIONS:
        cs = C.case('caps', res)
        r, r64 = cs.ref(), cs.ref(np.float64)
        n, pinned = C.CAPS[res]
        errs[res] = r64.contour[0, 1] / C.CAPS_EXACT - 1.0
        print('caps %s: %d pairs, contour fp64 %.6f fp32 %.6f, exact %.6f, error %.3f %%' % (res, len(r.pairs), r64.contour[0, 1], r.contour[0, 1],
                                                                                           C.CAPS_EXACT, 100 * errs[res]))
        assert len(r.pairs) == n and r.irregular == 0
        assert abs(r64.contour[0, 1] - pinned) < 5e-7 and abs(r.contour[0, 1] - r64.contour[0, 1]) < 1e-5
        assert r64.contour[0, 1] < C.CAPS_EXACT                                             # inscribed meshes: always short
    assert abs(C.CAPS_EXACT - 0.784770) < 5e-7
    assert abs(errs['12x16']) > abs(errs['24x46']) > abs(errs['48x92'])
    assert abs(errs['24x46']) < abs(errs['12x16']) / 3


@pytest.mark.parametrize('name,res,body_pairs', [('six', '12x16', ((0, 5), (1, 5))), ('six', '24x46', ((0, 5), (1, 5))),
                                                 ('caps', '12x16', ((0, 1),)), ('caps', '24x46', ((0, 1),))])
def test_closedness(name, res, body_pairs):
    """On two closed surfaces every (edge, triangle) event occurs in exactly two pairs: the edge has two faces."""
    cs = C.case(name, res)
    r = cs.ref()
    for i, j in body_pairs:
        rows = r.pairs[(r.pairs[:, 0] == i) & (r.pairs[:, 2] == j)]
        mask = R.events_length(*R.triangles_of(cs.verts, cs.faces, rows))[2]
        hist = C.closedness(rows, mask, cs.faces)
        print('%s %s (%d,%d): %d pairs, occurrences %s' % (name, res, i, j, len(rows), hist))
        assert list(hist) == [2] and hist[2] == len(rows)               # two events per pair, each event in two pairs


@pytest.mark.parametrize('name,res', [('six', '12x16'), ('caps', '24x46'), ('fold', '24x46')])
def test_role_swap_bit_identity(name, res):
    cs = C.case(name, res)
    P, Q = R.triangles_of(cs.verts, cs.faces, cs.ref().cand)
    sP, sQ, D = R.values(P, Q)
    tP, tQ, tD = R.values(Q, P)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    def same(a, b):
        """Equal values everywhere and equal bits wherever the value is not zero (a zero may come out as +0 in one role and -0 in the
        other: a cross component a*b - a*b is +0 in both roles; no comparison of the rule tells the two apart)."""
        return np.array_equal(a, b) and np.array_equal(bits(a)[a != 0], bits(b)[a != 0])
    assert same(sP, tQ) and same(sQ, tP) and same(D, tD.transpose(0, 2, 1))
    e, l, _ = R.events_length(P, Q)
    f, m, _ = R.events_length(Q, P)
    assert np.array_equal(e, f) and np.array_equal(bits(l), bits(m)) and (l > 0).sum() > 50


@pytest.mark.parametrize('res', ['12x16', '24x46'])
def test_fold_pinned_and_self_mode_against_between_mode(res):
    """The set compared: the self-mode pairs (s, t) of the folded mesh whose faces are of different parts (they share no vertex, by the
    candidate rule), written (lower face, upper face); against the between-mode pairs (0, s, 1, t) of a batch of two copies of the same
    mesh with s a lower face, t an upper face and no shared vertex index.  Faces across the hinge that share a vertex are excluded by the
    candidate rule in self mode and by this filter in between mode.  Events and length bits are equal (the roles may be swapped)."""
    verts, faces, upper = C.fold_mesh(res)
    r, rp = C.case('fold', res).ref(), C.case('fold_parts', res).ref()
    n_all, n_across, n_within = C.FOLD[res]
    across = upper[r.pairs[:, 1]] != upper[r.pairs[:, 3]]
    print('fold %s: %d self pairs, %d across the parts, %d within one; irregular %d' % (res, len(r.pairs), across.sum(), (~across).sum(), r.irregular))
    assert (len(r.pairs), int(across.sum()), int((~across).sum())) == (n_all, n_across, n_within) and r.irregular == 0
    assert np.array_equal(rp.pairs, r.pairs[across]) and np.array_equal(rp.length.view(np.uint32), r.length[across].view(np.uint32))
    assert r.counts.tolist() == [[n_all]] and rp.counts.tolist() == [[n_across]]
    two = R.crossings(np.concatenate([verts, verts]), faces, self_pairs=False)
    s, t = two.pairs[:, 1], two.pairs[:, 3]
    share = (faces[s][:, :, None] == faces[t][:, None, :]).any((1, 2))
    keep = ~upper[s] & upper[t] & ~share
    between = {(int(a), int(b)): (int(e), int(l)) for a, b, e, l in zip(s[keep], t[keep], two.events[keep], two.length[keep].view(np.uint32))}
    lower_first = np.where(upper[rp.pairs[:, 1]], rp.pairs[:, 3], rp.pairs[:, 1]), np.where(upper[rp.pairs[:, 1]], rp.pairs[:, 1], rp.pairs[:, 3])
    self_mode = {(int(a), int(b)): (int(e), int(l)) for a, b, e, l in zip(*lower_first, rp.events, rp.length.view(np.uint32))}
    assert self_mode == between and len(self_mode) == n_across


def test_groups_and_flags_in_the_restatement():
    cs = C.case('six', '12x16')
    g = np.array([0, 0, 1, 1, 0, 1])
    r = R.crossings(cs.verts, cs.faces, group=g, self_pairs=False)
    assert (g[r.cand[:, 0]] == g[r.cand[:, 2]]).all() and r.counts[0, 1] == 62 and r.counts.sum() == 124
    assert len(R.crossings(cs.verts, cs.faces, self_pairs=False, between=False).cand) == 0
    assert len(R.crossings(cs.verts, cs.faces, between=False).pairs) == 0                  # a capsule does not cross itself


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('sc_host') / 'surface_crossings_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off',
                        os.path.join(ROOT, 'tools', 'surface_crossings_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize('name,res', [c for c in ALL_CASES if c != ('caps', '48x92')])
def test_host_run_of_the_kernel_statements_equals_restatement(host_check, tmp_path, name, res):
    """tools/surface_crossings_host_check.hip runs sc_pair and the candidate rule of csrc/surface_crossings_shared.h serially on the CPU:
    its rows equal the restatement's row for row and bit for bit (pairs, events, length)."""
    cs = C.case(name, res)
    r = cs.ref()
    pairs, events, length = C.run_host_check(host_check, tmp_path, cs.verts, cs.faces, **cs.kw)
    assert np.array_equal(pairs, r.pairs) and np.array_equal(events, r.events)
    assert np.array_equal(length.view(np.uint32), r.length.view(np.uint32))


def test_host_run_with_groups(host_check, tmp_path):
    cs = C.case('six', '12x16')
    g = np.array([0, 0, 1, 1, 0, 1], np.int32)
    pairs, events, length = C.run_host_check(host_check, tmp_path, cs.verts, cs.faces, group=g, self_pairs=False)
    r = R.crossings(cs.verts, cs.faces, group=g, self_pairs=False)
    assert np.array_equal(pairs, r.pairs) and np.array_equal(length.view(np.uint32), r.length.view(np.uint32))


def test_face_parts_and_part_skip_matrix_by_hand():
    """A 5-joint tree 0 -> 1 -> 2, 0 -> 3 -> 4 (parents -1 0 1 0 3) and 5 vertices."""
    from psi_release_amd.evaluation import SMPLX_SELF_CONTACT_PAIRS, face_parts, part_skip_matrix
    w = np.array([[1.0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0], [0, 0.5, 0.5, 0, 0], [0, 0, 0, 0.75, 0.25], [0, 0, 0, 0.25, 0.75]], np.float32)
    faces = np.array([[0, 1, 2],      # sums 1, 1.5, .5, 0, 0 -> joint 1
                      [0, 3, 4],      # sums 1, 0, 0, 1, 1 -> a three-way tie: the lowest, joint 0
                      [2, 3, 4],      # sums 0, .5, .5, 1, 1 -> tie of 3 and 4: joint 3
                      [1, 2, 4]],     # sums 0, 1.5, .5, .25, .75 -> joint 1
                     np.int32)
    assert face_parts(w, faces).tolist() == [1, 0, 3, 1] == R.face_parts(w, faces).tolist()
    assert face_parts(w, faces).dtype == np.int32
    par = [-1, 0, 1, 0, 3]
    m = part_skip_matrix(par)
    want = np.eye(5, dtype=np.uint8)
    for a, b in ((0, 1), (1, 2), (0, 3), (3, 4)):
        want[a, b] = want[b, a] = 1
    assert m.dtype == np.uint8 and np.array_equal(m, want)
    assert np.array_equal(part_skip_matrix(par, same=False, parent_child=False), np.zeros((5, 5), np.uint8))
    m2 = part_skip_matrix(par, extra=[(2, 4)])
    assert m2[2, 4] == m2[4, 2] == 1 and (m2 != want).sum() == 2
    with pytest.raises(ValueError):
        part_skip_matrix(par, extra=[(2, 5)])
    with pytest.raises(ValueError):
        face_parts(w, np.array([[0, 1, 5]], np.int32))
    assert SMPLX_SELF_CONTACT_PAIRS == ((9, 16), (9, 17), (6, 16), (6, 17), (1, 2), (12, 22))
    # the SMPL-X tree of the package: the root's parent is outside [0, P)
    from psi_release_amd import synth
    big = part_skip_matrix(synth.SMPLX_PARENTS, extra=SMPLX_SELF_CONTACT_PAIRS)
    assert np.array_equal(big, big.T) and big[9, 16] == 1 and big[12, 22] == 1 and big.shape[0] == len(synth.SMPLX_PARENTS)


def test_select_uncrossed_by_hand():
    from psi_release_amd.evaluation import select_uncrossed
    counts = np.array([[0, 5, 0, 2], [5, 9, 0, 0], [0, 0, 0, 0], [2, 0, 0, 3]])
    assert select_uncrossed(range(4), counts) == [0, 2]                                    # 1 meets 0 with 5, 3 meets 0 with 2
    assert select_uncrossed(range(4), counts, max_pairs=2) == [0, 2, 3]
    assert select_uncrossed(range(4), counts, max_pairs=5) == [0, 1, 2, 3]
    assert select_uncrossed([1, 0, 3, 2], counts) == [1, 3, 2]                             # 0 meets 1; 3 meets neither 1 nor (absent) 0
    assert select_uncrossed([1, 0, 3, 2], counts, max_self=3) == [0, 2]                    # 1 drops (9 > 3), then 3 meets 0
    assert select_uncrossed([1, 0, 3, 2], counts, max_self=2) == [0, 2]
    assert select_uncrossed([3, 3, 2], counts, max_self=3) == [3, 2] and select_uncrossed([], counts) == []
    six = C.case('six', '12x16').ref().counts
    assert select_uncrossed(range(6), six) == [0, 2, 3, 4] and select_uncrossed([5, 1, 0], six) == [5]
    with pytest.raises(ValueError):
        select_uncrossed([4], counts)
    with pytest.raises(ValueError):
        select_uncrossed([0], counts[:3])


def test_symbols_declared_bound_and_refusals_without_a_gpu():
    import torch
    from psi_release_amd import build, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    assert build.PER_FILE['surface_crossings.hip'][0] == '-ffp-contract=off' and 'surface_crossings.hip' in build.sources()
    cs = C.case('thin')
    V, F = cs.verts.shape[1], len(cs.faces)
    for bad in (cs.faces.astype(np.int64), cs.faces[:, :2], np.zeros((0, 3), np.int32), np.where(cs.faces == 5, V, cs.faces).astype(np.int32),
                np.where(cs.faces == 5, -1, cs.faces).astype(np.int32)):
        with pytest.raises(ValueError):
            ops.surface_crossings_create(bad, V)
    with pytest.raises(ValueError):
        ops.surface_crossings_create(cs.faces, 0)
    with pytest.raises(ValueError):
        ops.surface_crossings_create(cs.faces, V, order_verts=cs.verts[0][:-1])
    part, skip = np.zeros(F, np.int32), np.eye(2, dtype=np.uint8)
    with pytest.raises(ValueError):
        ops.surface_crossings_create(cs.faces, V, face_part=part)                          # one without the other
    with pytest.raises(ValueError):
        ops.surface_crossings_create(cs.faces, V, face_part=np.where(np.arange(F) == 7, 2, part).astype(np.int32), part_skip=skip)
    with pytest.raises(ValueError):
        ops.surface_crossings_create(cs.faces, V, face_part=part, part_skip=np.array([[1, 1], [0, 1]], np.uint8))
    EINVAL = -22                                                                            # PSI_EINVAL of include/psi_hip.h
    assert '#define PSI_EINVAL (-22)' in header
    # the library's own refusals (the C entry points refuse what the Python layer would have caught)
    h = ctypes.c_void_p()
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad_faces = np.where(cs.faces == 5, V, cs.faces).astype(np.int32)
    assert L.psi_surface_crossings_create(ctypes.byref(h), as_p(bad_faces), V, F, None, None, None, 0) == EINVAL
    assert L.psi_surface_crossings_create(ctypes.byref(h), as_p(cs.faces), V, 0, None, None, None, 0) == EINVAL
    assert L.psi_surface_crossings_create(ctypes.byref(h), as_p(cs.faces), 0, F, None, None, None, 0) == EINVAL
    bad_part = np.full(F, 2, np.int32)
    assert L.psi_surface_crossings_create(ctypes.byref(h), as_p(cs.faces), V, F, None, as_p(bad_part), as_p(skip), 2) == EINVAL
    assert not h
    # wrong arguments of the call are refused before anything touches a device
    for v in (torch.zeros(2, V, 3, dtype=torch.float64), torch.zeros(2, V, 2), torch.zeros(V, 3), np.zeros((2, V, 3), np.float32)):
        with pytest.raises(ValueError):
            ops.surface_crossings(v, cs.faces)
    with pytest.raises(ValueError):
        ops.surface_crossings(torch.zeros(2, V, 3), cs.faces, mode='fast')
    with pytest.raises(ValueError):
        ops.surface_crossings(torch.zeros(2, V, 3), cs.faces, group=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.surface_crossings(torch.zeros(46341, 1, 3), cs.faces)
    with pytest.raises(hip.PsiHipError):
        ops.surface_crossings(torch.zeros(2, V, 3), cs.faces)                               # a CPU tensor: there is no CPU path


def test_face_order_is_a_permutation_and_deterministic():
    """The host half of create: without order_verts the identity; with it a permutation that keeps ties in face order and puts faces of one
    chunk close together (the chunk boxes of the Morton order are smaller than those of the face order on a shuffled mesh)."""
    from psi_release_amd import hip
    L = hip.lib()
    from psi_release_amd import synth
    v, f = synth.make_capsule_mesh(*C.WORKLOAD, C.RADIUS, C.HEIGHT)               # 82 chunks
    F, V = len(f), len(v)
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    order = np.empty(F, np.int32)
    assert L.psi_surface_crossings_face_order(as_p(f), V, F, None, as_p(order)) == 0 and np.array_equal(order, np.arange(F))
    fs = np.ascontiguousarray(f[np.random.RandomState(5).permutation(F)])
    again = np.empty(F, np.int32)
    assert L.psi_surface_crossings_face_order(as_p(fs), V, F, as_p(v), as_p(order)) == 0
    assert L.psi_surface_crossings_face_order(as_p(fs), V, F, as_p(v), as_p(again)) == 0
    assert np.array_equal(np.sort(order), np.arange(F)) and np.array_equal(order, again)

    def chunk_volume(faces):
        tri = v[faces]
        vol = 0.0
        for lo in range(0, F, 256):
            c = tri[lo:lo + 256].reshape(-1, 3)
            vol += float(np.prod(c.max(0) - c.min(0)))
        return vol
    print('chunk box volume: shuffled %.4f, Morton order %.4f' % (chunk_volume(fs), chunk_volume(fs[order])))
    assert chunk_volume(fs[order]) < 0.25 * chunk_volume(fs)
