"""Mesh -> SDF volume without a GPU: the NumPy restatement of the contract (tests/mesh_sdf_ref.py) against the analytic distance field of
the oriented stand-in room, welding and degenerate triangles, the scene point cloud, the entry script's arguments, and the search of
csrc/mesh_sdf.hip itself run serially on the host (tools/mesh_sdf_host_check.hip) against the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import mesh_sdf_ref as R
from psi_release_amd import scene_sdf, synth

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ['psi_mesh_sdf_create', 'psi_mesh_sdf_destroy', 'psi_mesh_sdf_info', 'psi_mesh_sdf_compute', 'psi_mesh_sdf_count_pairs']


def _room_grid(room, grow=0.17):
    return room.box_min - np.float32(grow), room.box_max + np.float32(grow)


@pytest.fixture(scope='module')
def room():
    return synth.make_oriented_room(2)


@pytest.fixture(scope='module')
def room_ref(room):
    lo, hi = _room_grid(room)
    return R.sdf(room.verts, room.faces, lo, hi, 24)


def test_oriented_room_is_closed_and_oriented(room):
    assert room.verts.dtype == np.float32 and room.faces.dtype == np.int32
    assert len(room.faces) == 144 and len(room.verts) == 18 * 9           # 18 faces of (2 + 1)^2 vertices of their own
    m = R.prepare(room.verts, room.faces)
    assert m['info'] == (144, 0, 78, 0)                                    # every edge shared by exactly two triangles after welding
    # every triangle faces free space: a point just in front of its centroid has a positive analytic distance
    cen = (m['a'] + m['b'] + m['c']) / 3.0
    assert (room.analytic_sdf(cen + 1e-3 * m['normals'][:, 0]) > 0).all() and (room.analytic_sdf(cen - 1e-3 * m['normals'][:, 0]) < 0).all()
    big = synth.make_oriented_room(5)
    assert len(big.faces) == 18 * 2 * 25 and R.prepare(big.verts, big.faces)['info'][3] == 0


def test_restatement_against_analytic_field(room, room_ref):
    """Bound 1e-6 m: the field of the fp32-rounded vertices differs from the exact one by the rounding of the vertices (~1e-7 m); the
    restatement itself is fp64.  No node lies on a surface, so every sign is decided."""
    vol, hist, info = room_ref
    lo, hi = _room_grid(room)
    an = room.analytic_sdf(R.node_positions(lo, hi, 24).astype(np.float64))
    err = np.abs(vol - an).max()
    print('restatement vs analytic: %.3g m; smallest |sdf| %.3g m; regions %s' % (err, np.abs(an).min(), hist.tolist()))
    assert vol.shape == (24, 24, 24) and info == (144, 0, 78, 0)
    assert err <= 1e-6
    assert np.abs(an).min() > 1e-3
    assert (np.sign(vol) == np.sign(an)).all()
    assert (an > 0).any() and (an < 0).any()


DEGENERATE_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0.0, -0.0], [1, 1, 0], [2, 2, 0], [3, 3, 0], [0.5, 0.5, 7]], np.float32)
DEGENERATE_F = np.array([[0, 1, 2],        # kept
                         [3, 1, 4],        # kept: vertex 3 is vertex 0 (-0.0 equals +0.0)
                         [0, 3, 1],        # two equal welded ids
                         [0, 4, 5],        # collinear: cross product exactly 0
                         [4, 5, 6],        # collinear
                         [2, 2, 1]])       # repeated index


def test_welding_and_degenerate_triangles():
    v, f = DEGENERATE_V, DEGENERATE_F
    wid, n = R.weld(v)
    assert n == 7 and wid[3] == 0 and (wid[[0, 1, 2, 4, 5, 6, 7]] == [0, 1, 2, 4, 5, 6, 7]).all()
    m = R.prepare(v, f)
    assert m['info'] == (2, 4, 7, 4)                                       # five edges; the two triangles share edge (0, 1), four are open
    assert (m['ids'] == [[0, 1, 2], [0, 1, 4]]).all()
    with pytest.raises(ValueError):
        R.prepare(v, f[2:])
    with pytest.raises(ValueError):
        R.prepare(v, np.array([[0, 1, 8]]))
    # an edge pseudonormal is the sum of the unit normals of its triangles; a vertex pseudonormal weighs them by the corner angle
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    m2 = R.prepare(v2, np.array([[0, 1, 2], [0, 3, 1]]))                    # normals +z and +y, sharing edge (0, 1)
    assert np.allclose(m2['normals'][0, 1], np.array([0, 1, 1]) / np.sqrt(2)) and np.allclose(m2['normals'][1, 3], m2['normals'][0, 1])
    assert np.allclose(m2['normals'][0, 4], np.array([0, 1, 1]) / np.sqrt(2))           # both corners at vertex 0 are right angles
    assert np.allclose(m2['normals'][0, 5], np.array([0, 1, 1]) / np.sqrt(2))           # and both at vertex 1 are 45 degrees
    assert np.allclose(m2['normals'][0, 6], [0, 0, 1]) and np.allclose(m2['normals'][0, 2], [0, 0, 1])


def test_closest_point_regions_by_hand():
    a, ab, ac = np.zeros((1, 1, 3)), np.array([[[1.0, 0, 0]]]), np.array([[[0.0, 1, 0]]])
    pts = np.array([[0.25, 0.25, 2], [0.5, -1, 0], [1, 1, 0], [-1, 0.5, 0], [-1, -1, 0], [2, -0.5, 0], [-0.5, 2, 0]], np.float64)
    r, region = R.closest(pts[:, None, :], a, ab, ac)
    assert region[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6]
    want = np.array([[0, 0, 2], [0, -1, 0], [0.5, 0.5, 0], [-1, 0, 0], [-1, -1, 0], [1, -0.5, 0], [-0.5, 1, 0]])
    assert np.allclose(r[:, 0], want)
    r32, region32 = R.closest(pts[:, None, :].astype(np.float32), a.astype(np.float32), ab.astype(np.float32), ac.astype(np.float32))
    assert r32.dtype == np.float32 and (region32 == region).all()


def test_scene_cloud(room):
    c = scene_sdf.scene_cloud(room.verts)
    assert c.dtype == np.float32 and c.shape == (78, 3)
    wid, _ = R.weld(room.verts)
    assert np.array_equal(c, room.verts[np.unique(wid)])                  # first appearance, in index order
    assert np.array_equal(scene_sdf.scene_cloud(np.array([[0.0, 1, 2], [-0.0, 1, 2], [3, 4, 5]])), np.array([[0, 1, 2], [3, 4, 5]], np.float32))
    pts = np.array([[0.0, 0, 0], [0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [1.0, 0, 0], [1.2, 0.3, 0.2], [0.05, 0.0, 0.0]], np.float32)
    assert np.array_equal(scene_sdf.scene_cloud(pts, voxel=1.0), pts[[0, 3]])
    assert np.array_equal(scene_sdf.scene_cloud(pts, voxel=0.5), pts[[0, 2, 3]])
    assert len(scene_sdf.scene_cloud(pts, voxel=1e-3)) == 6
    big = synth.make_oriented_room(16)
    down = scene_sdf.scene_cloud(big.verts, voxel=0.25)
    assert 100 < len(down) < len(scene_sdf.scene_cloud(big.verts)) == 4614
    with pytest.raises(ValueError):
        scene_sdf.scene_cloud(pts, voxel=0.0)
    lo, hi = scene_sdf.grid_box(room.verts, 0.5)
    assert np.allclose(lo, [-3.0, -2.5, -0.5]) and np.allclose(hi, [3.0, 2.5, 3.1]) and lo.dtype == np.float32


def test_engine_dim_is_checked_before_any_work(room):
    for dim in (30, 484, 0):
        with pytest.raises(ValueError):
            scene_sdf.scene_from_mesh(room.verts, room.faces, dim=dim)        # raised before a device is touched
    scene_sdf.check_engine_dim(256)
    scene_sdf.check_engine_dim(480)


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_scene_sdf as S
    finally:
        sys.path.pop(0)
    a = S.parse([str(tmp_path), '--name', 'roomS', '--synthetic', '--dim', '32'])
    assert a.synthetic and a.out_root == str(tmp_path) and a.scene_ply is None and a.name == 'roomS' and a.dim == 32 and a.margin == 0.5 and a.voxel is None
    b = S.parse(['scene.ply', str(tmp_path), '--name', 'N', '--voxel', '0.05', '--margin', '0.25'])
    assert not b.synthetic and b.scene_ply == 'scene.ply' and b.dim == 256 and b.voxel == 0.05 and b.margin == 0.25
    for bad in ([str(tmp_path), '--name', 'N'], ['--name', 'N', '--synthetic'], ['a.ply', str(tmp_path), '--name', 'N', '--synthetic'],
                [str(tmp_path), '--name', 'N', '--synthetic', '--dim', '30'], [str(tmp_path), '--name', 'N', '--synthetic', '--dim', '484'],
                [str(tmp_path), '--synthetic'], [str(tmp_path), '--name', 'N', '--synthetic', '--voxel', '0']):
        with pytest.raises(SystemExit):
            S.parse(bad)


def test_symbols_declared_bound_and_refuse_cpu_tensors():
    import torch
    from psi_release_amd import hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    with pytest.raises(hip.PsiHipError):
        ops.mesh_sdf_create(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(hip.PsiHipError):
        scene_sdf.MeshSDF(np.zeros((3, 3)), np.zeros((1, 3)), device='cpu')
    from psi_release_amd import build
    assert build.PER_FILE['mesh_sdf.hip'] == ['-ffp-contract=off']


def test_host_run_of_the_search_against_restatement(tmp_path, room, room_ref):
    """tools/mesh_sdf_host_check.hip runs the brick search of csrc/mesh_sdf.hip serially on the CPU, with the functions the kernel calls:
    the pruned search must equal brute force bit for bit (its exit status), and the volume must meet the restatement within the GPU
    tests' tolerance, 2e-6 x the grid diagonal (~32 fp32 roundings of quantities no larger than the diagonal)."""
    from psi_release_amd import build
    exe = str(tmp_path / 'mesh_sdf_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off',
                        os.path.join(ROOT, 'tools', 'mesh_sdf_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lo, hi = _room_grid(room)
    tol = 2e-6 * float(np.linalg.norm(hi.astype(np.float64) - lo))

    def run(verts, faces, glo, ghi, D):
        mesh = str(tmp_path / 'mesh.bin')
        with open(mesh, 'wb') as f:
            f.write(np.array([len(verts), len(faces)], np.int32).tobytes())
            f.write(np.ascontiguousarray(verts, np.float32).tobytes())
            f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        out = str(tmp_path / 'out.f32')
        rr = subprocess.run([exe, mesh, str(D)] + [repr(float(x)) for x in glo] + [repr(float(x)) for x in ghi] + [out], capture_output=True, text=True)
        assert rr.returncode == 0, rr.stdout + rr.stderr
        return np.fromfile(out, np.float32).reshape(D, D, D), rr.stdout

    vol, log = run(room.verts, room.faces, lo, hi, 24)
    assert 'kept 144 dropped 0 welded 78 open_edges 0' in log and 'nodes that differ: 0' in log
    ref = room_ref[0]
    print(log.strip(), '| host fp32 vs restatement: %.3g m (tol %.3g)' % (np.abs(vol - ref).max(), tol))
    assert np.abs(vol - ref).max() <= tol and (np.sign(vol) == np.sign(ref)).all()
    # the same welding and dropping in the library's host code
    _, log = run(DEGENERATE_V, DEGENERATE_F, [-1, -1, -1], [2, 2, 2], 9)
    assert 'kept 2 dropped 4 welded 7 open_edges 4' in log and 'nodes that differ: 0' in log
    # partial bricks, several cells per axis, a grid box that leaves the cell grid far behind
    fine = synth.make_oriented_room(6)
    for glo, ghi, D in ((lo, hi, 13), (room.box_min - np.float32(5), room.box_max + np.float32(5), 10)):
        _, log = run(fine.verts, fine.faces, glo, ghi, D)
        assert 'nodes that differ: 0' in log
