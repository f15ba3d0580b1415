"""Scene crossings on the GPU (csrc/scene_crossings.hip, ops.scene_crossings, evaluation.SceneCrossings): the cases
of tests/scene_crossings_cases.py against the NumPy restatement (tests/scene_crossings_ref.py) — pairs row for row, events, counts,
face_hit, tri_hit and irregular exact, length and contour bit-equal — 'brute' against 'pruned' bit for bit, the rows of a body alone
against its rows in the batch, a permuted scene, a Morton-ordered body handle, the partial ends of both kinds of chunk, empty results,
the case a distance volume cannot see, the refusals, run-to-run determinism, a handle dropped before its result, and the two entry
scripts in child processes.  Every test prints its figures before it asserts."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import scene_crossings_cases as C
from psi_release_amd import evaluation, hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FIELDS = ('pairs', 'events', 'length', 'counts', 'contour', 'face_hit', 'tri_hit', 'irregular')
DTYPES = (torch.int32, torch.int32, torch.float32, torch.int32, torch.float64, torch.bool, torch.bool, torch.int32)
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    """As tests/test_body_overlap_gpu.py does, and for its reason: what this module's calls leave in PyTorch's caching allocator goes back
    to the runtime when the module ends."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def handles():
    """name -> (scene handle, body handle in face order), made once."""
    out = {}
    for name in ('plate_room', 'plate_only'):
        sc = C.scene(name)
        out[name] = (ops.scene_crossings_create(sc.verts, sc.faces), ops.surface_crossings_create(sc.body_faces, sc.body_verts.shape[1]))
    yield out
    for s, b in out.values():
        s.close(), b.close()


def _host(res):
    assert isinstance(res, ops.SceneCrossingsResult) and res._fields == FIELDS
    assert tuple(t.dtype for t in res) == DTYPES and all(t.is_cuda for t in res)
    n = res.pairs.shape[0]
    assert res.pairs.shape == (n, 3) and res.events.shape == (n,) and res.length.shape == (n,) and res.irregular.shape == ()
    return ops.SceneCrossingsResult(*(t.cpu().numpy() for t in res[:7]), int(res.irregular.item()))


def _run(verts, scene_handle, body, stats=False, **kw):
    """The SceneCrossingsResult as host arrays (irregular as an int), checked for dtype, device and shape."""
    out = ops.scene_crossings(torch.tensor(np.ascontiguousarray(verts), device=DEV), scene_handle, body, return_stats=stats, **kw)
    res, st = out if stats else (out, None)
    host = _host(res)
    assert host.counts.shape == (len(verts),) and host.contour.shape == (len(verts),) and host.face_hit.shape[0] == len(verts)
    return (host, st) if stats else host


def _same_bits(a, b):
    for name, x, y in zip(FIELDS, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, name
        assert np.array_equal(x.view(np.uint8) if x.dtype.kind == 'f' else x, y.view(np.uint8) if y.dtype.kind == 'f' else y), name


def _equals_ref(got, r):
    assert np.array_equal(got.pairs, r.pairs) and C.ascending(got.pairs)
    assert np.array_equal(got.events, r.events) and np.array_equal(got.counts, r.counts) and got.irregular == r.irregular
    assert np.array_equal(got.face_hit, r.face_hit) and np.array_equal(got.tri_hit, r.tri_hit)
    assert np.array_equal(got.length.view(np.uint32), r.length.view(np.uint32))
    assert np.array_equal(got.contour.view(np.uint64), r.contour.view(np.uint64))


def test_plate_room_equals_the_restatement(handles):
    sc = C.scene('plate_room')
    got, st = _run(sc.body_verts, *handles['plate_room'], stats=True)
    print('plate_room: pairs %s, contour %s, irregular %d, stats %s' % (got.counts.tolist(), got.contour.tolist(), got.irregular, st))
    _equals_ref(got, sc.ref())
    assert tuple(got.counts) == C.PAIRS and st['pairs'] == sum(C.PAIRS)
    assert handles['plate_room'][0].F == 528 and handles['plate_room'][0].n_chunks == 3 and handles['plate_room'][1].n_chunks == 2


def test_brute_equals_pruned_bit_for_bit(handles):
    sc = C.scene('plate_room')
    pruned, sp = _run(sc.body_verts, *handles['plate_room'], stats=True)
    brute, sb = _run(sc.body_verts, *handles['plate_room'], stats=True, mode='brute')
    print('pruned %s, brute %s' % (sp, sb))
    _same_bits(pruned, brute)
    assert sb['tiles'] == 4 * 2 * 3 and sp['tiles'] < sb['tiles'] and sp['pairs'] == sb['pairs']
    assert sb['box_tests'] == 4 * 352 * 528 and sp['box_tests'] < sb['box_tests']


def test_a_body_alone_has_the_rows_it_has_in_the_batch(handles):
    sc = C.scene('plate_room')
    r = sc.ref()
    for b in range(4):
        got = _run(sc.body_verts[b:b + 1], *handles['plate_room'])
        rows = r.pairs[:, 0] == b
        assert np.array_equal(got.pairs[:, 1:], r.pairs[rows][:, 1:]) and not got.pairs[:, 0].any()
        assert np.array_equal(got.events, r.events[rows]) and np.array_equal(got.length.view(np.uint32), r.length[rows].view(np.uint32))
        assert got.contour.view(np.uint64)[0] == r.contour.view(np.uint64)[b] and got.counts[0] == r.counts[b]
        assert np.array_equal(got.face_hit[0], r.face_hit[b])


def test_a_permuted_scene_gives_the_same_rows(handles):
    sc = C.scene('plate_room')
    r = sc.ref()
    perm = np.random.RandomState(11).permutation(len(sc.faces))
    h = ops.scene_crossings_create(sc.verts, sc.faces[perm])
    got = _run(sc.body_verts, h, handles['plate_room'][1])
    mapped = got.pairs.copy()
    mapped[:, 2] = perm[got.pairs[:, 2]]                    # position t of the permuted array is the caller's triangle perm[t]
    order = np.lexsort((mapped[:, 2], mapped[:, 1], mapped[:, 0]))
    assert np.array_equal(mapped[order], r.pairs) and np.array_equal(got.events[order], r.events)
    assert np.array_equal(got.length[order].view(np.uint32), r.length.view(np.uint32))
    assert np.array_equal(got.counts, r.counts) and np.array_equal(got.face_hit, r.face_hit) and np.array_equal(got.tri_hit[np.argsort(perm)], r.tri_hit)
    # the contour adds the lengths of a body in ITS row order, which the permutation changes among the triangles one face crosses; the
    # fp64 sum of these fp32 lengths is exact (about forty bits between the sum's top bit and the smallest length's last), so the bits
    # are those of the unpermuted scene, and of the restatement of the permuted one
    rp = C.Scene(sc.verts, sc.faces[perm]).ref()
    assert np.array_equal(got.contour.view(np.uint64), rp.contour.view(np.uint64)) and np.array_equal(got.pairs, rp.pairs)
    assert np.array_equal(got.contour.view(np.uint64), r.contour.view(np.uint64))


def test_a_morton_ordered_body_handle_gives_the_same_bits(handles):
    sc = C.scene('plate_room')
    plain = _run(sc.body_verts, *handles['plate_room'])
    h = ops.surface_crossings_create(sc.body_faces, sc.body_verts.shape[1], order_verts=C.body_mesh()[0])
    _same_bits(plain, _run(sc.body_verts, handles['plate_room'][0], h))
    _same_bits(plain, _run(sc.body_verts, handles['plate_room'][0], sc.body_faces))           # faces instead of a handle


@pytest.mark.parametrize('nf', [1, 255, 256, 257, 528])
def test_partial_scene_chunks(handles, nf):
    sc = C.scene('plate_room').cut(nf)
    h = ops.scene_crossings_create(sc.verts, sc.faces)
    assert (h.F, h.n_chunks) == (nf, (nf + 255) // 256)
    got = _run(sc.body_verts, h, handles['plate_room'][1])
    r = sc.ref()
    print('first %d triangles: pairs %s' % (nf, got.counts.tolist()))
    _equals_ref(got, r)
    assert got.tri_hit.shape == (nf,)
    _same_bits(got, _run(sc.body_verts, h, handles['plate_room'][1], mode='brute'))


def test_only_the_last_partial_body_chunk_meets_the_scene(handles):
    sc = C.scene('plate_only')
    verts = C.bodies([(None, 0.0, C.LIFT)])
    got, st = _run(verts, *handles['plate_only'], stats=True)
    r = sc.ref(body_verts=verts)
    print('lifted body: %d pairs, first face %d, stats %s' % (len(got.pairs), got.pairs[:, 1].min(), st))
    _equals_ref(got, r)
    assert len(got.pairs) == C.LIFT_PAIRS and got.pairs[:, 1].min() >= 256
    assert 1 <= st['tiles'] <= 2 and st['box_tests'] <= 96 * 300            # tiles of the 96-face chunk only
    _same_bits(got, _run(verts, *handles['plate_only'], mode='brute'))


def test_empty_results(handles):
    sc = C.scene('plate_room')
    got, st = _run(sc.body_verts[1:2], *handles['plate_room'], stats=True)         # candidates, but nothing crosses: no emit pass
    assert st['pairs'] == 0 and st['tiles'] >= 1
    far, st_far = _run(sc.body_verts[1:2], *handles['plate_only'], stats=True)     # the body's box misses the scene's: no test kernel at all
    assert st_far == {'tiles': 0, 'pairs': 0, 'box_tests': 0}
    for res, nf in ((got, 528), (far, 300)):
        assert res.pairs.shape == (0, 3) and res.events.shape == (0,) and res.length.shape == (0,)
        assert res.counts.tolist() == [0] and res.contour.tolist() == [0.0] and res.irregular == 0
        assert not res.face_hit.any() and res.tri_hit.shape == (nf,) and not res.tri_hit.any()


def test_the_case_a_distance_volume_cannot_see(handles):
    """A 64^3 signed distance volume over the room (2.8 m / 63 = 4.4 cm between nodes along z) has no node in the 1 cm plate: sampled at
    the vertices of body 0, which stands through the plate, it reports no penetration, while the mesh itself is crossed 92 times."""
    from psi_release_amd import scene_sdf
    sc, po = C.scene('plate_room'), C.scene('plate_only')
    gmin, gmax = np.array([-2.6, -2.1, -0.1], np.float32), np.array([2.6, 2.1, 2.7], np.float32)
    D = 64
    step = (gmax - gmin) / np.float32(D - 1)
    axes = [gmin[a] + np.arange(D, dtype=np.float32) * step[a] for a in range(3)]
    inside = [(ax >= np.float32(C.PLATE_LO[a])) & (ax <= np.float32(C.PLATE_HI[a])) for a, ax in enumerate(axes)]
    assert inside[0].any() and inside[1].any() and not inside[2].any()      # no node lies in the closed plate box: none at its heights
    # plate_room has 180 free triangles and a room box wound outwards, so the sign comes from the winding number with free space outside
    # (at the nodes around body 0 the fp64 winding number of the restatement stays 0.36 away from the level)
    vol = scene_sdf.MeshSDF(sc.verts, sc.faces, device=DEV).compute(gmin, gmax, D, sign='winding', exterior='free')
    v0 = torch.tensor(sc.body_verts[:1], device=DEV)
    sdf = ops.sdf_sample(v0, vol, torch.tensor(gmin, device=DEV), torch.tensor(gmax, device=DEV))
    got = _run(sc.body_verts[:1], *handles['plate_room'])
    r = sc.ref()
    plate_rows = int(((r.pairs[:, 0] == 0) & (r.pairs[:, 2] < C.N_PLATE)).sum())
    print('smallest sampled distance of body 0 to the scene %.4f m; %d crossings with the plate, %d with the whole scene' % (
        float(sdf.min()), plate_rows, got.counts[0]))
    assert not (sdf < 0).any()
    assert plate_rows == C.PLATE_ONLY_PAIRS_BODY0 == int((got.pairs[:, 2] < C.N_PLATE).sum())
    assert _run(sc.body_verts[:1], *handles['plate_only']).counts[0] == plate_rows


def test_refusals(handles):
    sc = C.scene('plate_only')
    scene_h, body_h = handles['plate_only']
    nv, V = len(sc.verts), sc.body_verts.shape[1]
    nan_used = sc.verts.copy()
    nan_used[sc.faces[7, 1], 2] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        ops.scene_crossings_create(nan_used, sc.faces)
    with pytest.raises(ValueError, match='outside'):
        ops.scene_crossings_create(sc.verts, np.where(sc.faces == 5, nv, sc.faces).astype(np.int32))
    unused = np.concatenate([sc.verts, np.full((1, 3), np.nan, np.float32)])               # a non-finite vertex nobody refers to is no error
    ops.scene_crossings_create(unused, sc.faces).close()
    verts = torch.tensor(C.scene('plate_room').body_verts, device=DEV)
    bad = verts.clone()
    bad[2, 17, 1] = float('nan')
    with pytest.raises(ValueError, match='body 2 '):
        ops.scene_crossings(bad, scene_h, body_h)
    with pytest.raises(hip.PsiHipError):
        ops.scene_crossings(verts.cpu(), scene_h, body_h)
    with pytest.raises(ValueError, match='vertices per body'):
        ops.scene_crossings(verts[:, :-1].contiguous(), scene_h, body_h)
    with pytest.raises(ValueError, match='mode'):
        ops.scene_crossings(verts, scene_h, body_h, mode='fast')
    with pytest.raises(ValueError, match='scene_handle'):
        ops.scene_crossings(verts, body_h, body_h)
    with pytest.raises(ValueError, match='46340'):
        ops.scene_crossings(torch.zeros(46341, 1, 3, device=DEV), scene_h, np.zeros((1, 3), np.int32))


def test_two_runs_give_equal_bits_and_a_dropped_handle_leaves_the_result(handles):
    sc = C.scene('plate_room')
    first = _run(sc.body_verts, *handles['plate_room'])
    _same_bits(first, _run(sc.body_verts, *handles['plate_room']))
    scene_h = ops.scene_crossings_create(sc.verts, sc.faces)
    body_h = ops.surface_crossings_create(sc.body_faces, sc.body_verts.shape[1])
    res = ops.scene_crossings(torch.tensor(sc.body_verts, device=DEV), scene_h, body_h)
    ops.scene_crossings_destroy(scene_h)
    del scene_h, body_h
    scratch = torch.zeros(1 << 20, device=DEV)                                              # something else takes memory meanwhile
    torch.cuda.synchronize()
    _same_bits(first, _host(res))
    del scratch


def _write_bodies(gen, n):
    os.makedirs(gen)
    for i in range(n):
        rec = synth.make_bodies(40 + i, 1)
        rec['transl'] = (rec['transl'] * 0.2 + np.array([0.4 * i, 0.0, 0.0])).astype(np.float32)
        with open(os.path.join(gen, 'body_gen_{:06d}.pkl'.format(i)), 'wb') as f:
            pickle.dump(rec, f)


def _decoder_verts(gen):
    sys.path.insert(0, UTILS)
    try:
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    xh, cam = evaluation.PlausibilityEvaluator._read_folder(gen, 100)
    decoder = S.BodyDecoder(synth.make_smplx(7), synth.make_vposer_state(3), torch.device(DEV, torch.cuda.current_device()))
    return xh, cam, decoder, S


def _child(code, *args):
    r = subprocess.run([sys.executable, '-c', code] + [str(a) for a in args], capture_output=True, text=True, cwd=UTILS, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_records_and_the_overlap_script_in_a_child_process(tmp_path):
    """evaluation.SceneCrossings.crossings_of_records against a direct call on the same vertices, and utils_eval_body_overlap.py
    --scene_mesh - under --synthetic in a fresh process: without the flag the report and the printed lines are what they are without
    the feature's code taking part; with it the new fields equal the direct call."""
    gen = str(tmp_path / 'gen')
    _write_bodies(gen, 3)
    xh, cam, decoder, S = _decoder_verts(gen)
    room = synth.make_room_mesh()
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    owner = evaluation.SceneCrossings(room.verts, room.faces, decoder.faces, device=DEV)
    res = owner.crossings_of_records(xh, S.camera_pose(cam, True), decoder, chunk=2)
    scene_h = ops.scene_crossings_create(room.verts, room.faces)
    direct = ops.scene_crossings(verts, scene_h, decoder.faces.to(torch.int32).cpu().numpy())
    _same_bits(_host(res), _host(direct))
    _same_bits(_host(res), _host(owner.crossings(verts, mode='brute')))
    mesh = evaluation.SceneCrossings(synth.make_room_mesh(), None, decoder.faces, device=DEV)      # an object with .verts and .faces
    _same_bits(_host(res), _host(mesh.crossings(verts)))
    a, b = str(tmp_path / 'plain.json'), str(tmp_path / 'scene.json')
    code = ('import sys, utils_eval_body_overlap as E\n'
            'base = [sys.argv[1], "--synthetic", sys.argv[2], "--no_flip"]\n'
            'E.main(base + ["--out", sys.argv[3]])\nprint("=====")\n'
            'E.main(base + ["--scene_mesh", "-", "--out", sys.argv[4]])\n')
    plain_out, scene_out = _child(code, gen, tmp_path / 'syn', a, b).split('=====\n')
    plain, rep = json.load(open(a)), json.load(open(b))
    new = {'scene_crossings', 'scene_contour', 'scene_ranked', 'scene_irregular', 'scene_triangle_pairs', 'scene_triangles_crossed',
           'max_scene_pairs', 'clear'}
    assert set(rep) - set(plain) == new and {k: rep[k] for k in plain} == plain
    assert scene_out.startswith(plain_out) and not any(w in plain_out for w in ('scene', 'clear'))
    counts = res.counts.cpu().tolist()
    print('script: scene crossings %s, contour %s, %d scene triangles crossed' % (rep['scene_crossings'], rep['scene_contour'],
                                                                                 rep['scene_triangles_crossed']))
    assert rep['scene_crossings'] == counts and rep['scene_contour'] == res.contour.cpu().tolist()
    assert rep['scene_triangle_pairs'] == res.pairs.shape[0] and rep['scene_irregular'] == int(res.irregular)
    assert rep['scene_triangles_crossed'] == int(res.tri_hit.sum()) and rep['clear'] == [i for i in range(3) if counts[i] == 0]
    assert rep['scene_ranked'] == sorted(range(3), key=lambda i: (-rep['scene_contour'][i], i))
    for i in range(3):
        assert 'body %6d: %6d scene crossings, contour %.4f m' % (i, counts[i], rep['scene_contour'][i]) in scene_out
    assert '--clear=' + ','.join(str(i) for i in rep['clear']) in scene_out
    sys.path.insert(0, UTILS)
    try:
        import utils_eval_body_overlap as E
    finally:
        sys.path.pop(0)
    with pytest.raises(SystemExit):
        E.parse_args([gen, '--scene_mesh', '-'])
    with pytest.raises(SystemExit):
        E.parse_args([gen, '--max_scene_pairs', '2'])


def test_the_result_viewer_in_a_child_process(tmp_path):
    """utils_show_test_results.py --scene_crossings under --synthetic in a fresh process: every row of visibility.json gains the two
    fields, equal to a direct call; everything else, the images included, is byte-equal to the run without the flag."""
    gen = str(tmp_path / 'gen')
    _write_bodies(gen, 3)
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'scene')
    code = ('import sys, utils_show_test_results as S\n'
            'base = [sys.argv[1], "-", None, "--synthetic", sys.argv[2], "--no_flip", "--size", "48", "64", "--pack", "2"]\n'
            'for out, extra in ((sys.argv[3], []), (sys.argv[4], ["--scene_crossings"])):\n'
            '    S.main(base[:2] + [out] + base[3:] + extra)\n')
    _child(code, gen, tmp_path / 'syn', a, b)
    plain, rows = json.load(open(os.path.join(a, 'visibility.json'))), json.load(open(os.path.join(b, 'visibility.json')))
    assert [{k: v for k, v in row.items() if k not in ('scene_crossings', 'scene_contour')} for row in rows] == plain
    assert all('scene_crossings' not in row and 'scene_contour' not in row for row in plain)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for name in os.listdir(a):
        if name.endswith('.png'):
            assert open(os.path.join(a, name), 'rb').read() == open(os.path.join(b, name), 'rb').read(), name
    xh, cam, decoder, S = _decoder_verts(gen)
    room = synth.make_room_mesh(0, 180)
    verts = decoder.verts(xh, S.camera_pose(cam, True)).contiguous()
    # the script reads the room back from the PLY it wrote: the same fp32 vertices and faces
    from psi_release_amd import scene_io
    pv, pf, _ = scene_io.read_ply_mesh(os.path.join(str(tmp_path / 'syn'), 'room.ply'))
    assert np.array_equal(pv, room.verts) and np.array_equal(pf, room.faces)
    res = evaluation.SceneCrossings(pv, pf, decoder.faces, device=DEV).crossings(verts)
    print('viewer: scene crossings %s' % [row['scene_crossings'] for row in rows])
    assert [row['scene_crossings'] for row in rows] == res.counts.cpu().tolist()
    assert [row['scene_contour'] for row in rows] == res.contour.cpu().tolist()
