"""Scene crossings without a GPU: the NumPy restatement (tests/scene_crossings_ref.py) in float32 against the same
rule in float64 and against the independent fp64 / exact statement on every candidate, the pinned counts of
tests/scene_crossings_cases.py, the contour of a body through the plate against the perimeter of its two sections, the candidate rule
losing nothing, the kernel's statements and the handle builder run serially on the host (tools/scene_crossings_host_check.hip) bit for
bit against the restatement, the key at its limits, ``select_clear`` by hand, the new symbols and the refusals that need no GPU.

Nothing is excluded anywhere: no candidate is left out of a comparison for being close to a decision."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import scene_crossings_cases as C
import scene_crossings_ref as SR
import surface_crossings_ref as R

SYMBOLS = ['psi_scene_crossings_' + s for s in ('create', 'destroy', 'info', 'tiles', 'test', 'finish')]
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def test_restatement_against_float64_and_independent_statement():
    """Equal events on EVERY candidate of plate_room: float32 rule = float64 rule = independent statement, edge for edge."""
    sc = C.scene('plate_room')
    r32, r64 = sc.ref(np.float32), sc.ref(np.float64)
    P, Q = SR.triangles_of(sc.body_verts, sc.body_faces, sc.verts, sc.faces, r32.cand)
    ind, ind_mask = R.independent_events(P, Q)
    print('plate_room: %d candidates, %d crossing pairs, fp32 != fp64 on %d, fp32 != independent on %d' % (
        len(r32.cand), len(r32.pairs), (r32.cand_events != r64.cand_events).sum(), (ind != r32.cand_events).sum()))
    assert np.array_equal(r32.cand, r64.cand) and len(r32.cand) == sum(C.CANDIDATES)
    assert np.array_equal(r32.cand_events, r64.cand_events)
    assert np.array_equal(ind, r32.cand_events) and np.array_equal(ind_mask, r32.cand_mask)
    assert np.array_equal(r32.pairs, r64.pairs) and C.ascending(r32.pairs) and C.ascending(r32.cand)


def test_plate_room_pinned():
    sc = C.scene('plate_room')
    r = sc.ref()
    assert len(sc.faces) == 528 and sc.body_verts.shape == (4, 178, 3) and len(sc.body_faces) == 352
    assert len(C.plate_mesh()[1]) == C.N_PLATE
    cand = np.bincount(r.cand[:, 0], minlength=4)
    m = r.cand_mask[r.cand_events >= 1]
    print('plate_room: candidates %s, pairs %s, irregular %d, body-edge events %d, scene-edge events %d, contour %s' % (
        cand.tolist(), r.counts.tolist(), r.irregular, m[:, :3].sum(), m[:, 3:].sum(), r.contour.tolist()))
    assert tuple(cand) == C.CANDIDATES and tuple(r.counts) == C.PAIRS and r.irregular == 0
    assert (int(m[:, :3].sum()), int(m[:, 3:].sum())) == (C.BODY_EDGE_EVENTS, C.SCENE_EDGE_EVENTS)         # both edge roles occur
    assert r.contour[1] == 0.0 and (r.contour[[0, 2, 3]] > 0).all()
    assert r.face_hit.sum(1).tolist()[1] == 0 and r.tri_hit.sum() == len(np.unique(r.pairs[:, 2]))
    assert r.counts.sum() == len(r.pairs) == len(r.events) == len(r.length)
    # body 3 stands through the plate and the floor: it crosses plate triangles and room triangles
    t3 = r.pairs[r.pairs[:, 0] == 3][:, 2]
    assert (t3 < C.N_PLATE).any() and (t3 >= C.N_PLATE).any()


def test_plate_only_contour_against_the_two_sections():
    """Body 0 through the closed plate: 46 pairs on each plate face, no vertex inside the plate, and the summed fp32 lengths against the
    fp64 perimeter of the capsule's sections at z = 0.9 and z = 0.91 computed from the mesh.  The observed fp32-against-fp64 difference of
    one length here is <= 1.2e-7, so the sum is bounded by pairs x 1e-6: a sanity bound, not the contract."""
    sc = C.scene('plate_only')
    r, r64 = sc.ref(), sc.ref(np.float64)
    p = r.pairs[r.pairs[:, 0] == 0]
    v0 = sc.body_verts[0]
    lo, hi = np.array(C.PLATE_LO, np.float32), np.array(C.PLATE_HI, np.float32)
    assert not ((v0 >= lo) & (v0 <= hi)).all(1).any()                                       # no vertex of the body lies in the plate
    assert len(p) == C.PLATE_ONLY_PAIRS_BODY0 and r.irregular == 0
    assert np.bincount(p[:, 2] // 50, minlength=6).tolist() == [0, 0, 0, 0, 46, 46]        # the two faces of constant z
    want = C.section_perimeter(v0, sc.body_faces, 0.9) + C.section_perimeter(v0, sc.body_faces, 0.91)
    l32, l64 = r.length[r.pairs[:, 0] == 0], r64.length[r64.pairs[:, 0] == 0]
    print('plate_only body 0: %d pairs, contour fp32 %.7f fp64 %.7f, sections %.7f, largest fp32 - fp64 of a length %.3g' % (
        len(p), r.contour[0], r64.contour[0], want, np.abs(l32.astype(np.float64) - l64).max()))
    assert abs(r.contour[0] - want) < len(p) * 1e-6 and abs(r64.contour[0] - want) < len(p) * 1e-6


def test_every_face_triangle_pair_not_only_the_candidates():
    """Body 0 against plate_only, all 352 x 300 pairs: fp32 = fp64 = independent, and a pair whose boxes do not meet has no event."""
    sc = C.scene('plate_only')
    F, nf = len(sc.body_faces), len(sc.faces)
    s, t = np.divmod(np.arange(F * nf), nf)
    P, Q = sc.body_verts[0][sc.body_faces][s], sc.verts[sc.faces][t]
    e32, e64, ind = R.events_length(P, Q, np.float32)[0], R.events_length(P, Q, np.float64)[0], R.independent_events(P, Q)[0]
    assert np.array_equal(e32, e64) and np.array_equal(e32, ind)
    r = sc.ref()
    cand0 = r.cand[r.cand[:, 0] == 0]
    is_cand = np.zeros(F * nf, bool)
    is_cand[cand0[:, 1].astype(np.int64) * nf + cand0[:, 2]] = True
    assert not e32[~is_cand].any() and int((e32 > 0).sum()) == C.PLATE_ONLY_PAIRS_BODY0


def test_lifted_body_reaches_the_plate_with_its_last_chunk_only():
    sc = C.scene('plate_only')
    r = sc.ref(body_verts=C.bodies([(None, 0.0, C.LIFT)]))
    assert len(r.pairs) == C.LIFT_PAIRS and r.cand[:, 1].min() == C.LIFT_FIRST_FACE >= 256


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('scn_host') / 'scene_crossings_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off',
                        os.path.join(ROOT, 'tools', 'scene_crossings_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize('name', ['plate_room', 'plate_only'])
def test_host_run_of_the_kernel_statements_equals_restatement(host_check, tmp_path, name):
    """tools/scene_crossings_host_check.hip runs the candidate rule, sc_pair, the key and the un-key serially on the CPU over the handle
    builder's records: its rows equal the restatement's row for row and bit for bit."""
    sc = C.scene(name)
    r = sc.ref()
    (pairs, events, length), _ = C.run_host_check(host_check, tmp_path, sc.body_verts, sc.body_faces, sc.verts, sc.faces)
    assert np.array_equal(pairs, r.pairs) and np.array_equal(events, r.events)
    assert np.array_equal(bits(length), bits(r.length))


@pytest.mark.parametrize('name,nf', [('plate_room', 528), ('plate_room', 257), ('plate_room', 256), ('plate_room', 1), ('plate_only', 300)])
def test_handle_builder_against_the_numpy_statement(host_check, tmp_path, name, nf):
    """The host half of psi_scene_crossings_create (scn_build): the Morton order is a permutation, ties to the lower index, and equals
    the NumPy statement; the chunk boxes and the scene's box are exact."""
    sc = C.scene(name).cut(nf)
    _, (order, chunk_boxes, box) = C.run_host_check(host_check, tmp_path, sc.body_verts[:1], sc.body_faces, sc.verts, sc.faces)
    want_order, want_boxes, want_box = SR.morton_chunks(sc.verts, sc.faces)
    assert np.array_equal(np.sort(order), np.arange(nf)) and np.array_equal(order, want_order)
    assert chunk_boxes.shape == ((nf + 255) // 256, 6) and np.array_equal(chunk_boxes, want_boxes) and np.array_equal(box, want_box)
    pts = sc.verts[sc.faces].reshape(-1, 3)
    assert np.array_equal(box, np.concatenate([pts.min(0), pts.max(0)]))


def _flat_plate_face():
    """The 50 triangles of the plate's face of constant z = 0.9: their centroid sums have no extent along z."""
    v, f = C.plate_mesh()
    flat = np.ascontiguousarray(f[200:250])
    assert (v[flat][:, :, 2] == v[flat][0, 0, 2]).all()
    return v, flat


@pytest.mark.parametrize('name', ['capsule_24x46', 'plate_only', 'flat_plate_face'])
def test_one_morton_order_for_body_handle_scene_handle_and_restatement(host_check, tmp_path, name):
    """One mesh as a body topology with a pose and as a scene: the face order of psi_surface_crossings_face_order, the triangle order of
    scn_build (through tools/scene_crossings_host_check.hip) and ``morton_chunks`` are equal element for element.  The 24 x 46 capsule has
    F = 2116, nine chunks; on the flat face one axis has zero width."""
    import surface_crossings_cases as SC
    from psi_release_amd import hip
    v, f = {'capsule_24x46': lambda: SC.mesh('24x46'), 'plate_only': C.plate_mesh, 'flat_plate_face': _flat_plate_face}[name]()
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    V, F = len(v), len(f)
    assert F == {'capsule_24x46': 2116, 'plate_only': 300, 'flat_plate_face': 50}[name]
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    body_order = np.full(F, -1, np.int32)
    assert hip.lib().psi_surface_crossings_face_order(as_p(f), V, F, as_p(v), as_p(body_order)) == 0, hip.last_error()
    sc = C.scene('plate_only')
    _, (scene_order, _, _) = C.run_host_check(host_check, tmp_path, sc.body_verts[:1], sc.body_faces, v, f)
    want = SR.morton_chunks(v, f)[0]
    assert np.array_equal(np.sort(want), np.arange(F)) and not np.array_equal(want, np.arange(F))
    assert np.array_equal(body_order, want) and np.array_equal(scene_order, want)


def test_morton_order_tightens_the_chunks():
    """On a shuffled room the chunk boxes of the Morton order are far smaller than those of the given order."""
    from psi_release_amd import synth
    room = synth.make_room_mesh(seed=0, n_extra=0, subdiv=8)
    f = np.ascontiguousarray(room.faces[np.random.RandomState(3).permutation(len(room.faces))])
    _, boxes, _ = SR.morton_chunks(room.verts, f)
    vol = lambda b: float(np.prod(b[:, 3:] - b[:, :3] + 1e-3, axis=1).sum())
    given = []
    for k in range(0, len(f), 256):
        pts = room.verts[f[k:k + 256]].reshape(-1, 3)
        given.append(np.concatenate([pts.min(0), pts.max(0)]))
    print('chunk box volume: shuffled %.3f, Morton order %.3f' % (vol(np.array(given)), vol(boxes)))
    assert vol(boxes) < 0.25 * vol(np.array(given))


def test_key_round_trips_at_the_limits(host_check):
    rr = subprocess.run([host_check, '--keys'], capture_output=True, text=True)
    assert rr.returncode == 0 and 'keys round-trip at the limits' in rr.stdout, rr.stdout + rr.stderr


def test_select_clear_by_hand():
    from psi_release_amd.evaluation import select_clear
    counts = np.array([0, 5, 0, 2])
    assert select_clear(range(4), counts) == [0, 2]
    assert select_clear(range(4), counts, max_pairs=2) == [0, 2, 3]
    assert select_clear([3, 1, 0, 2], counts, max_pairs=5) == [3, 1, 0, 2]
    assert select_clear([2, 2, 0], counts) == [2, 0] and select_clear([], counts) == []
    assert select_clear(range(4), C.scene('plate_room').ref().counts) == [1]
    with pytest.raises(ValueError):
        select_clear([4], counts)
    with pytest.raises(ValueError):
        select_clear([0], counts[None])


def test_symbols_declared_bound_and_refusals_without_a_gpu():
    import torch
    from psi_release_amd import build, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    assert build.PER_FILE['scene_crossings.hip'] == build.PER_FILE['surface_crossings.hip'] and 'scene_crossings.hip' in build.sources()
    assert ops.SceneCrossingsResult._fields == ('pairs', 'events', 'length', 'counts', 'contour', 'face_hit', 'tri_hit', 'irregular')
    sc = C.scene('plate_only')
    nv = len(sc.verts)
    nan_used = sc.verts.copy()
    nan_used[sc.faces[7, 1], 2] = np.nan
    for v, f in ((sc.verts.astype(np.float64), sc.faces), (sc.verts, sc.faces.astype(np.int64)), (sc.verts[:, :2], sc.faces),
                 (sc.verts, sc.faces[:, :2]), (sc.verts, np.zeros((0, 3), np.int32)), (sc.verts, np.where(sc.faces == 5, nv, sc.faces).astype(np.int32)),
                 (sc.verts, np.where(sc.faces == 5, -1, sc.faces).astype(np.int32)), (nan_used, sc.faces)):
        with pytest.raises(ValueError):
            ops.scene_crossings_create(v, f)
    # the library's own refusals (the C entry point refuses what the Python layer would have caught), before anything touches a device
    EINVAL = -22
    h = ctypes.c_void_p()
    as_p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    bad_faces = np.where(sc.faces == 5, nv, sc.faces).astype(np.int32)
    assert L.psi_scene_crossings_create(ctypes.byref(h), as_p(sc.verts), nv, as_p(bad_faces), len(bad_faces)) == EINVAL
    assert 'outside' in hip.last_error()
    assert L.psi_scene_crossings_create(ctypes.byref(h), as_p(nan_used), nv, as_p(sc.faces), len(sc.faces)) == EINVAL
    assert 'non-finite' in hip.last_error()
    assert L.psi_scene_crossings_create(ctypes.byref(h), as_p(sc.verts), nv, as_p(sc.faces), 0) == EINVAL
    assert L.psi_scene_crossings_create(ctypes.byref(h), None, nv, as_p(sc.faces), 1) == EINVAL
    assert not h
    # wrong arguments of the call are refused in the order of the checks, before anything touches a device
    V = sc.body_verts.shape[1]
    for v in (torch.zeros(2, V, 3, dtype=torch.float64), torch.zeros(2, V, 2), torch.zeros(V, 3), np.zeros((2, V, 3), np.float32)):
        with pytest.raises(ValueError):
            ops.scene_crossings(v, None, sc.body_faces)
    with pytest.raises(ValueError):
        ops.scene_crossings(torch.zeros(2, V, 3), None, sc.body_faces, mode='fast')
    with pytest.raises(ValueError):
        ops.scene_crossings(torch.zeros(2, V, 3), ctypes.c_void_p(), sc.body_faces)         # not a handle of scene_crossings_create
    with pytest.raises(ValueError):
        ops.scene_crossings(torch.zeros(2, V, 3), hip.Handle('psi_scene_crossings_destroy'), sc.body_faces)   # a closed handle
