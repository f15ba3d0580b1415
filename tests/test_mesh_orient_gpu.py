"""Orienting a mesh on the GPU (csrc/mesh_orient.hip through ops.flood_fill, ops.mesh_orient_votes and scene_sdf.orient_faces): the fill
and the votes equal the NumPy restatement (tests/mesh_orient_ref.py) exactly, flipped stand-in rooms come back face for face and give the
volume of the original mesh, runs are bit-identical, every refusal is raised, and the entry script runs in a child process.  The grid size
is the one tests/test_mesh_orient_cpu.py found sufficient on the CPU (profiles/mesh_orient_cases.json)."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_orient_ref as R
from psi_release_amd import hip, ops, scene_sdf, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
DIM = json.load(open(os.path.join(ROOT, 'profiles', 'mesh_orient_cases.json')))['dim']
SEED = np.array([[0.0, 0.0, 1.5]], np.float32)


@pytest.fixture(scope='module', autouse=True)
def _give_cached_blocks_back():
    """As tests/test_mesh_cloud_gpu.py does: the blocks PyTorch's allocator cached for this module go back to the runtime when it ends."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _spiral(n=40):
    """A corridor one node wide: every second layer z holds a serpentine over every second row x, the rows joined at alternating ends of
    y, and the layers joined at alternating corners.  It passes through every brick that holds a corridor row several times."""
    m = np.zeros((n, n, n), bool)
    for li, z in enumerate(range(0, n, 2)):
        rows = list(range(0, n, 2))
        for ri, x in enumerate(rows):
            m[x, :, z] = True
            if ri + 1 < len(rows):
                m[x + 1, n - 1 if ri % 2 == 0 else 0, z] = True
        if z + 2 < n:                                               # the serpentine of a layer ends in row rows[-1]; the next one runs back
            end_y = 0 if len(rows) % 2 == 0 else n - 1
            m[rows[-1] if li % 2 == 0 else 0, end_y if li % 2 == 0 else 0, z + 1] = True
    return m


def _fill_cases():
    rs = np.random.RandomState(7)
    rand = rs.uniform(size=(20, 17, 9)) < 0.6
    opn = np.argwhere(rand)
    cases = [('random_20x17x9', rand, opn[rs.choice(len(opn), 3, replace=False)])]
    cases.append(('spiral_40', _spiral(40), np.array([[0, 0, 0]])))
    cases.append(('open_9', np.ones((9, 9, 9), bool), np.array([[4, 4, 4]])))
    lonely = rs.uniform(size=(12, 10, 19)) < 0.5
    seeds = np.array([[0, 0, 0], [7, 8, 8], [8, 3, 16], [11, 9, 18]])         # brick corners, brick borders, the grid's far corner
    for s in seeds:
        for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            q = s + d
            if ((q >= 0) & (q < lonely.shape)).all():
                lonely[tuple(q)] = False
        lonely[tuple(s)] = True
    cases.append(('lonely_seeds', lonely, seeds))
    odd = rs.uniform(size=(8, 9, 16)) < 0.7
    cases.append(('edges_8_9_16', odd, np.argwhere(odd)[[0, -1]]))
    for e in (8, 9, 16):
        cube = rs.uniform(size=(e, e, e)) < 0.65
        cases.append(('cube_%d' % e, cube, np.argwhere(cube)[[0, len(np.argwhere(cube)) // 2]]))
    return cases


FILL_CASES = _fill_cases()


@pytest.mark.parametrize('case', FILL_CASES, ids=[c[0] for c in FILL_CASES])
def test_fill_equals_the_restatement(case):
    name, mask, seeds = case
    want = R.flood_fill(mask, seeds)
    got, rounds = ops.flood_fill(torch.tensor(mask, device=DEV), seeds, return_rounds=True)
    raw = got.view(torch.uint8)
    print('%-16s %d of %d open nodes free, %d launches' % (name, int(want.sum()), int(mask.sum()), rounds))
    assert got.dtype == torch.bool and tuple(got.shape) == mask.shape and int(raw.max()) <= 1          # no stamp is left behind
    assert np.array_equal(got.cpu().numpy(), want)
    got8, rounds8 = ops.flood_fill(torch.tensor(mask.astype(np.uint8) * 255, device=DEV), torch.tensor(seeds, device=DEV), return_rounds=True)
    assert torch.equal(got8, got) and rounds8 == rounds                                                 # uint8 masks, device seeds, a second run
    if name.startswith('spiral'):
        assert want.sum() == mask.sum() > 15000 and rounds > 1
        assert rounds > 40                           # the corridor enters a new brick at least every 8 nodes of a 40-node row
    if name == 'open_9':
        assert want.all() and rounds > 1             # the seed's brick first, its neighbours in the next launches
    if name == 'lonely_seeds':
        assert want.sum() == len(seeds) and rounds == 1             # the seeds are set before the first launch, and it gains nothing


def _unsigned(verts, faces, lo, hi, dim):
    mesh = scene_sdf.MeshSDF(verts, faces, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return mesh.compute(lo, hi, dim).abs().cpu().numpy()


def _flipped_room(fraction=0.4):
    room = synth.make_oriented_room(2)
    return room, *synth.flip_faces(room.faces, fraction, seed=1)


def _mixed_room():
    rm = synth.make_room_mesh(subdiv=1)
    return rm, synth.flip_faces(rm.faces, 0.4, seed=1)[0]


@pytest.mark.parametrize('which', ['oriented_room_2_flipped', 'room_mesh_1'])
def test_votes_equal_the_restatement(which):
    if which == 'room_mesh_1':
        rm, faces = _mixed_room()
    else:
        rm, faces, _ = _flipped_room()
    verts = rm.verts
    lo, hi = scene_sdf.grid_box(verts, 0.0)
    U = _unsigned(verts, faces, lo, hi, DIM)                        # the kernel's own magnitudes
    h = R.spacing(lo, hi, DIM)
    free, lo2, hi2 = scene_sdf.free_space(verts, faces, SEED, dim=DIM)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2) and free.dtype == torch.bool and tuple(free.shape) == (DIM,) * 3
    want_free = R.flood_fill(R.open_nodes(U, lo, hi), R.seed_nodes(SEED, lo, hi, DIM))
    assert np.array_equal(free.cpu().numpy(), want_free) and 0 < want_free.sum() < DIM ** 3
    points, tri = scene_sdf.orient_samples(verts, faces, h, device=DEV)
    rp, rt = R.samples(verts, faces, h)
    assert np.array_equal(points.cpu().numpy().view(np.uint32), rp.view(np.uint32)) and np.array_equal(tri.cpu().numpy(), rt)
    dv, df = torch.tensor(verts, device=DEV), torch.tensor(np.ascontiguousarray(faces, np.int32), device=DEV)
    delta = np.float32(1.5) * h
    got = ops.mesh_orient_votes(points, tri, dv, df, free, lo, hi, float(delta)).cpu().numpy()
    want = R.votes(rp, rt, verts, faces, want_free, lo, hi, delta)
    print('%s: %d samples on %d triangles, %d front and %d back votes' % (which, len(rp), len(faces), want[:, 0].sum(), want[:, 1].sum()))
    assert got.dtype == np.int32 and got.shape == (len(faces), 2) and np.array_equal(got, want)
    assert want.sum() > len(faces)                                  # the cloud adds to the centroids
    r = scene_sdf.orient_faces(verts, faces, SEED, dim=DIM)
    ref = R.orient(verts, faces, SEED, U, lo, hi)
    assert np.array_equal(r.votes, want) and np.array_equal(r.faces, ref['faces']) and np.array_equal(r.flipped, ref['flipped'])
    assert np.array_equal(r.decided_by, ref['decided_by']) and r.free_nodes == int(want_free.sum())
    # a sample that names no triangle and a triangle without area cast no vote
    tri_bad = tri.clone()
    tri_bad[0], tri_bad[1] = -1, len(faces)
    df_bad = df.clone()
    df_bad[int(tri[2])] = df_bad[int(tri[2]), 0]
    got_bad = ops.mesh_orient_votes(points, tri_bad, dv, df_bad, free, lo, hi, float(delta)).cpu().numpy()
    fb = df_bad.cpu().numpy()
    assert np.array_equal(got_bad, R.votes(rp[2:], rt[2:], verts, fb, want_free, lo, hi, delta)) and (got_bad[int(tri[2])] == 0).all()


@pytest.fixture(scope='module')
def original_volume():
    room = synth.make_oriented_room(2)
    return scene_sdf.scene_from_mesh(room.verts, room.faces, dim=32)


@pytest.mark.parametrize('fraction', [0.4, 0.0, 1.0])
def test_flipped_room_comes_back_and_gives_the_same_volume(fraction, original_volume):
    room, faces, mask = _flipped_room(fraction)
    r = scene_sdf.orient_faces(room.verts, faces, SEED, dim=DIM)
    by = r.decided_by
    print('fraction %g: %d flipped, %d by vote, %d by propagation, %d undecided, %d free nodes, %d launches'
          % (fraction, r.flipped.sum(), (by == 0).sum(), (by == 1).sum(), (by == -1).sum(), r.free_nodes, r.rounds))
    assert r.faces.dtype == faces.dtype and r.faces.shape == faces.shape and np.array_equal(r.faces, room.faces)
    assert r.flipped.dtype == bool and np.array_equal(r.flipped, mask) and by.dtype == np.int8 and (by >= 0).all()
    assert r.votes.dtype == np.int32 and r.votes.shape == (144, 2) and r.rounds > 1 and r.free_nodes > 0
    nop = scene_sdf.orient_faces(room.verts, faces, SEED, dim=DIM, propagate=False)
    assert (nop.decided_by == 1).sum() == 0 and (nop.decided_by == -1).sum() == (by == 1).sum() > 0
    assert np.array_equal(nop.faces[nop.decided_by == -1], faces[nop.decided_by == -1])
    scene = scene_sdf.scene_from_mesh(room.verts, faces, dim=32, orient_seeds=SEED)
    assert np.array_equal(scene.sdf.view(np.uint32), original_volume.sdf.view(np.uint32))
    assert np.array_equal(scene.verts.view(np.uint32), original_volume.verts.view(np.uint32))


def test_the_flipped_mesh_is_a_real_defect(original_volume):
    room, faces, _ = _flipped_room(0.4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        broken = scene_sdf.scene_from_mesh(room.verts, faces, dim=32)
    pts = R.S.node_positions(broken.grid_min, broken.grid_max, 32)
    exact = room.analytic_sdf(pts)
    clear = np.abs(exact) > 1e-4                                    # a node on the surface has no sign to get wrong
    wrong = int(((broken.sdf < 0) != (exact < 0))[clear].sum())
    fine = int(((original_volume.sdf < 0) != (exact < 0))[clear].sum())
    print('sign differs from the analytic field at %d of %d nodes without orientation, at %d with the original faces' % (wrong, clear.sum(), fine))
    assert wrong > 0 and fine == 0


def test_two_runs_are_bit_identical_and_repeated_seeds_change_nothing():
    rm, faces = _mixed_room()
    runs = [scene_sdf.orient_faces(rm.verts, faces, SEED, dim=DIM) for _ in range(2)]
    runs.append(scene_sdf.orient_faces(rm.verts, faces, np.repeat(SEED, 5, axis=0), dim=DIM))
    a = runs[0]
    print('mixed room: %d flipped, %d by vote, %d by propagation, %d undecided, %d launches'
          % (a.flipped.sum(), (a.decided_by == 0).sum(), (a.decided_by == 1).sum(), (a.decided_by == -1).sum(), a.rounds))
    for b in runs[1:]:
        for field in ('faces', 'flipped', 'votes', 'decided_by'):
            x, y = getattr(a, field), getattr(b, field)
            assert x.dtype == y.dtype and np.array_equal(x, y), field
        assert (a.free_nodes, a.rounds) == (b.free_nodes, b.rounds)
    f1, _, _ = scene_sdf.free_space(rm.verts, faces, SEED, dim=DIM)
    f5, _, _ = scene_sdf.free_space(rm.verts, faces, np.repeat(SEED, 5, axis=0), dim=DIM)
    assert torch.equal(f1, f5)


def test_refusals():
    room, faces, _ = _flipped_room(0.4)
    v = room.verts
    with pytest.raises(ValueError, match='seed 1 .*outside the grid'):
        scene_sdf.orient_faces(v, faces, [[0.0, 0.0, 1.5], [9.0, 0.0, 1.5]], dim=DIM)
    with pytest.raises(ValueError, match='seed 0 .*outside the grid'):
        scene_sdf.free_space(v, faces, [[0.0, 0.0, -0.2]], dim=DIM)
    with pytest.raises(ValueError, match='seed 1 .*not open'):                    # on the floor, and inside the axis-aligned box
        scene_sdf.orient_faces(v, faces, [[0.0, 0.0, 1.5], [0.0, 0.0, 0.0]], dim=DIM)
    with pytest.raises(ValueError, match='seed 0 .*not open'):
        scene_sdf.free_space(v, faces, [[0.9, -0.8, 0.06]], dim=DIM)
    for dim in (1, 1025):
        with pytest.raises(ValueError, match='2 .. 1024'):
            scene_sdf.orient_faces(v, faces, SEED, dim=dim)
    for ratio in (0.5, 0, float('nan')):
        with pytest.raises(ValueError, match='ratio'):
            scene_sdf.orient_faces(v, faces, SEED, dim=DIM, ratio=ratio)
    with pytest.raises(ValueError):
        scene_sdf.orient_faces(v, faces, np.zeros((0, 3)), dim=DIM)
    mask = torch.ones(8, 8, 8, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match='2 .. 1024'):
        ops.flood_fill(torch.ones(1, 8, 8, dtype=torch.bool, device=DEV), [[0, 0, 0]])
    with pytest.raises(ValueError, match='2 .. 1024'):
        ops.flood_fill(torch.ones(2, 1025, 2, dtype=torch.bool, device=DEV), [[0, 0, 0]])
    with pytest.raises(ValueError, match='seed 1: .*outside'):
        ops.flood_fill(mask, [[0, 0, 0], [0, 8, 0]])
    with pytest.raises(ValueError, match='seed 0: .*outside'):
        ops.flood_fill(mask, [[-1, 0, 0]])
    shut = mask.clone()
    shut[3, 3, 3] = False
    with pytest.raises(ValueError, match='seed 2: .*not open'):
        ops.flood_fill(shut, [[0, 0, 0], [1, 1, 1], [3, 3, 3]])
    with pytest.raises(ValueError):
        ops.flood_fill(mask, np.zeros((0, 3), np.int64))
    with pytest.raises(hip.PsiHipError):
        ops.flood_fill(torch.ones(8, 8, 8, dtype=torch.bool), [[0, 0, 0]])        # a CPU tensor
    # the library refuses the same on its own
    import ctypes
    seeds = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    out = torch.zeros(8, 8, 8, dtype=torch.uint8, device=DEV)
    L = hip.lib()
    m8 = mask.view(torch.uint8)
    for args in ((1, 8, 8, 1), (8, 8, 1025, 1), (8, 8, 8, 0)):
        assert L.psi_flood_fill(hip.ptr(m8), args[0], args[1], args[2], hip.ptr(seeds), args[3], hip.ptr(out), None, hip.stream()) != 0
    torch.cuda.synchronize()
    assert int(out.sum()) == 0


def test_entry_script_in_a_child_process(tmp_path, original_volume):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    cmd = [sys.executable, os.path.join(UTILS, 'utils_scene_sdf.py'), '--synthetic', str(tmp_path), '--name', 'roomO', '--dim', '32', '--orient',
           '--flip', '0.4', '--orient-dim', str(DIM)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    assert 'orient: 58 of 144 triangles flipped, 16 decided by propagation, 0 left undecided' in r.stdout
    sdf = np.load(str(tmp_path / 'scenes_sdf' / 'roomO_sdf.npy'))
    assert np.array_equal(sdf.astype(np.float32).view(np.uint32).reshape(-1), original_volume.sdf.view(np.uint32).reshape(-1))
    # a mesh from a file needs a seed; a seed without --orient is refused (argparse exits with 2)
    sys.path.insert(0, UTILS)
    try:
        import utils_scene_sdf as S
    finally:
        sys.path.pop(0)
    for extra in (['--orient'], ['--seed', '0', '0', '1.5'], ['--flip', '0.4']):
        with pytest.raises(SystemExit) as e:
            S.parse(['x.ply', str(tmp_path), '--name', 'n'] + extra)
        assert e.value.code == 2
    a = S.parse(['x.ply', str(tmp_path), '--name', 'n', '--orient', '--seed', '0', '0', '1.5', '--seed', '1', '1', '1'])
    assert a.seed == [[0.0, 0.0, 1.5], [1.0, 1.0, 1.0]]
    assert S.parse([str(tmp_path), '--name', 'n', '--synthetic', '--orient']).seed == [[0.0, 0.0, 1.5]]
