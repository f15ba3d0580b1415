"""The orientation rule on the CPU (tests/mesh_orient_ref.py) with U from a brute-force fp64 point-triangle
distance: flipped stand-in rooms come back exactly, the undersides of the floating boxes need the propagation, what is decided on the room
without ceiling is right, the fill equals a queue BFS and the propagation rule holds on a hand-made strip.  profiles/mesh_orient_cases.json
holds what was measured here (the grid size the GPU tests use among it) and is pinned."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import mesh_orient_ref as R
from psi_release_amd import scene_sdf, synth

CASES = json.load(open(os.path.join(ROOT, 'profiles', 'mesh_orient_cases.json')))
DIM = CASES['dim']
SEED = np.array([[0.0, 0.0, 1.5]], np.float32)
SUB = 2
NT = 2 * SUB * SUB                                                  # triangles per box face
UNDERSIDES = list(range(10 * NT, 11 * NT)) + list(range(16 * NT, 17 * NT))      # face axis 2, lower side, of the two boxes


@pytest.fixture(scope='module')
def fields():
    """U [D,D,D] fp32 of make_oriented_room(2) and of the same room without its ceiling, from one brute-force pass: the distance to the
    closed room is the smaller of the distance to the open room and the distance to the ceiling's triangles."""
    room, opened = synth.make_oriented_room(SUB), synth.make_open_room(SUB, drop_ceiling=True)
    assert np.array_equal(room.verts.view(np.uint32), opened.verts.view(np.uint32))
    assert np.array_equal(np.concatenate([room.faces[:5 * NT], room.faces[6 * NT:]]), opened.faces)
    lo, hi = scene_sdf.grid_box(room.verts, 0.0)
    u_open = R.brute_unsigned(opened.verts, opened.faces, lo, hi, DIM)
    u_ceiling = R.brute_unsigned(room.verts, room.faces[5 * NT:6 * NT], lo, hi, DIM)
    return {'room': room, 'opened': opened, 'lo': lo, 'hi': hi, 'U': np.minimum(u_open, u_ceiling), 'U_open': u_open}


@pytest.mark.parametrize('fraction', [0.4, 0.0, 1.0])
def test_flipped_room_comes_back_exactly(fields, fraction):
    assert DIM == min(CASES['dims_tried']) == 64                   # the smallest of {64, 96, 128} already holds
    room = fields['room']
    assert len(room.faces) == 144 == CASES['oriented_room_2']['triangles']
    flipped, mask = synth.flip_faces(room.faces, fraction, seed=1)
    assert mask.sum() == round(fraction * 144) and (fraction in (0.0, 1.0) or not np.array_equal(flipped, room.faces))
    r = R.orient(room.verts, flipped, SEED, fields['U'], fields['lo'], fields['hi'])
    by = r['decided_by']
    got = {'restored': bool(np.array_equal(r['faces'], room.faces)), 'by_vote': int((by == R.VOTE).sum()),
           'by_propagation': int((by == R.PROPAGATION).sum()), 'undecided': int((by == R.UNDECIDED).sum())}
    print(fraction, got, 'free nodes', int(r['free'].sum()))
    assert r['faces'].dtype == room.faces.dtype and np.array_equal(r['faces'], room.faces)
    assert np.array_equal(r['flipped'], mask) and got['undecided'] == 0 and not (by == R.ZERO_AREA).any()
    assert got == CASES['oriented_room_2']['by_fraction'][str(fraction)]
    assert int(r['free'].sum()) == CASES['oriented_room_2']['free_nodes']


def test_undersides_need_the_propagation(fields):
    room = fields['room']
    flipped, mask = synth.flip_faces(room.faces, 0.4, seed=1)
    r = R.orient(room.verts, flipped, SEED, fields['U'], fields['lo'], fields['hi'], do_propagate=False)
    by = r['decided_by']
    # 5 cm above the floor: the node layer in the gap is not open, the front probe ends below the grid, the back probe inside the box
    assert (r['votes'][UNDERSIDES] == 0).all() and (by[UNDERSIDES] == R.UNDECIDED).all()
    assert np.nonzero(by == R.UNDECIDED)[0].tolist() == CASES['oriented_room_2']['undecided_without_propagation'] == UNDERSIDES
    decided = by >= 0
    assert np.array_equal(r['flipped'][decided], mask[decided]) and not r['flipped'][~decided].any()
    assert np.array_equal(r['faces'][~decided], flipped[~decided]) and np.array_equal(r['faces'][decided], room.faces[decided])


def test_open_room_decides_nothing_wrongly(fields):
    opened = fields['opened']
    want = CASES['open_room_2_no_ceiling']
    flipped, mask = synth.flip_faces(opened.faces, want['fraction'], seed=1)
    r = R.orient(opened.verts, flipped, SEED, fields['U_open'], fields['lo'], fields['hi'])        # margin 0: the fill ends at the box
    by = r['decided_by']
    decided = by >= 0
    share = float((by == R.UNDECIDED).sum()) / len(by)
    print('open room: %d by vote, %d by propagation, undecided share %r, %d free nodes' % ((by == 0).sum(), (by == 1).sum(), share, r['free'].sum()))
    assert len(by) == want['triangles'] and np.array_equal(r['flipped'][decided], mask[decided])
    assert np.array_equal(r['faces'][decided], opened.faces[decided])
    assert share == want['undecided_share'] and int((by == R.UNDECIDED).sum()) == want['undecided']
    assert (int((by == R.VOTE).sum()), int((by == R.PROPAGATION).sum())) == (want['by_vote'], want['by_propagation'])
    assert int(r['free'].sum()) == want['free_nodes']
    # the top layer of nodes is free (there is no ceiling) and nothing outside the grid ever is: the fill left only through the box
    assert r['free'][DIM // 2, DIM // 2, DIM - 1]


def test_fill_equals_a_queue_bfs():
    rs = np.random.RandomState(7)
    mask = rs.uniform(size=(20, 17, 9)) < 0.6
    opn = np.argwhere(mask)
    seeds = opn[rs.choice(len(opn), 3, replace=False)]
    a, b = R.flood_fill(mask, seeds), R.flood_fill_queue(mask, seeds)
    assert np.array_equal(a, b) and a[tuple(seeds.T)].all() and not (a & ~mask).any() and 3 < a.sum() < mask.sum()
    # a seed on a closed node or outside the mask contributes nothing
    shut = np.argwhere(~mask)[0]
    assert not R.flood_fill(mask, [shut, [-1, 0, 0], [20, 0, 0]]).any() and not R.flood_fill_queue(mask, [shut, [0, 17, 0]]).any()


def test_propagation_rule_on_a_strip():
    """Four triangles in the plane z = 0, a strip 0-1-2-3 over the vertices of two rows; triangle 1 is wound against the others."""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0], [-0.0, 0.0, 0.0]], np.float32)
    f = np.array([[6, 1, 3], [1, 3, 4], [1, 2, 4], [2, 5, 4]], np.int32)      # 6 is vertex 0 again, with -0.0: welded by position
    area = np.ones(4, bool)
    nb = R.neighbours(v, f, area)
    assert {t: sorted(x) for t, x in nb.items()} == {0: [(1, False)], 1: [(0, False), (2, False)], 2: [(1, False), (3, True)], 3: [(2, True)]}
    undec = lambda: np.full(4, R.UNDECIDED, np.int8)
    # one decided triangle at the end: the orientation runs down the strip
    by = undec()
    by[0] = R.VOTE
    flip, by2 = R.propagate(v, f, np.zeros(4, bool), by)
    assert flip.tolist() == [False, True, False, False] and by2.tolist() == [0, 1, 1, 1]
    by = undec()
    by[0] = R.VOTE
    flip, _ = R.propagate(v, f, np.array([True, False, False, False]), by)
    assert flip.tolist() == [True, False, True, True]
    # triangles 0 and 2 decided and contradicting each other about triangle 1: the lower index wins
    by = undec()
    by[[0, 2]] = R.VOTE
    flip, by2 = R.propagate(v, f, np.array([False, False, True, False]), by)
    assert flip.tolist() == [False, True, True, True] and by2.tolist() == [0, 1, 0, 1]
    # an edge shared by three triangles carries nothing; a triangle without area neither
    f3 = np.concatenate([f, [[1, 3, 5]]]).astype(np.int32)
    nb3 = R.neighbours(v, f3, np.ones(5, bool))
    assert 1 not in [u for u, _ in nb3.get(0, [])] and 4 not in nb3
    by = np.array([R.VOTE, R.ZERO_AREA, R.UNDECIDED, R.UNDECIDED], np.int8)
    flip, by2 = R.propagate(v, f, np.zeros(4, bool), by)
    assert by2.tolist() == [R.VOTE, R.ZERO_AREA, R.UNDECIDED, R.UNDECIDED] and not flip.any()
    # the library's vectorised propagation states the same rule
    rs = np.random.RandomState(0)
    room = synth.make_oriented_room(2)
    ff, _ = synth.flip_faces(room.faces, 0.5, seed=3)
    for trial in range(4):
        by = np.where(rs.uniform(size=len(ff)) < 0.15, R.VOTE, R.UNDECIDED).astype(np.int8)
        fl = (rs.uniform(size=len(ff)) < 0.5) & (by == R.VOTE)
        want = R.propagate(room.verts, ff, fl, by)
        got = scene_sdf._propagate(room.verts, ff.astype(np.int64), fl, by)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and (got[1] >= 0).all()


def test_flip_faces():
    f = np.arange(30, dtype=np.int32).reshape(10, 3)
    g, mask = synth.flip_faces(f, 0.3, seed=1)
    assert mask.sum() == 3 and g.dtype == f.dtype and np.array_equal(g[~mask], f[~mask]) and np.array_equal(g[mask], f[mask][:, [0, 2, 1]])
    g2, mask2 = synth.flip_faces(f, 0.3, seed=1)
    assert np.array_equal(g, g2) and np.array_equal(mask, mask2) and not np.array_equal(mask, synth.flip_faces(f, 0.3, seed=2)[1])
    assert np.array_equal(R.apply_flips(g, mask), f) and f[0].tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        synth.flip_faces(f, 1.5, seed=0)
