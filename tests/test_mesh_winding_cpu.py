"""Winding-number sign without a GPU: the NumPy fp64 restatement (tests/mesh_winding_ref.py) against the analytic field of the stand-in
room and of its three defects (the reason for the feature: the pseudonormal sign fails on each), the pruned arm's error and counts, the
closed-form dipole far from an open rectangle, ``exterior='free'``, the kernel's statements run serially on the host
(tools/mesh_winding_host_check.hip) against the restatement, the new symbols and the entry script's arguments.

TOL_F = 4 x 4.12e-6 (tests/mesh_winding_cases.py has how it was obtained); the host run must stay within TOL_F / 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import mesh_sdf_ref as R
import mesh_winding_ref as W
import mesh_winding_cases as C
from psi_release_amd import scene_sdf, synth

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ['psi_mesh_winding_compute', 'psi_mesh_winding_count', 'psi_mesh_sdf_apply_sign']


def test_closed_room_is_integer_and_matches_analytic_sign():
    cs = C.case('room_s2_d24')
    f, counts = cs.ref(0)
    an = cs.analytic()
    print('closed room: max |f - rint(f)| %.3g; values %s' % (np.abs(f - np.rint(f)).max(), np.unique(np.rint(f)).tolist()))
    assert counts == (24 ** 3 * 144, 0)
    assert np.abs(f - np.rint(f)).max() <= 1e-12
    assert ((f >= 0.5) == (an > 0)).all()
    assert (f > 0.5).any() and (f < 0.5).any()


def test_make_open_room():
    closed = synth.make_oriented_room(2)
    same = synth.make_open_room(2, drop_ceiling=False, sink=0.0)
    assert np.array_equal(same.verts, closed.verts) and np.array_equal(same.faces, closed.faces)
    o = synth.make_open_room(2)
    assert len(o.faces) == 136 and R.prepare(o.verts, o.faces)['info'] == (136, 0, 78, 8)
    assert o.verts[o.faces].reshape(-1, 3)[:, 2].max() == np.float32(2.6)               # the walls still reach the ceiling's height
    s = synth.make_open_room(2, drop_ceiling=False, sink=0.05)
    assert R.prepare(s.verts, s.faces)['info'] == (144, 0, 78, 0)
    moved = s.verts[6 * 9:12 * 9]
    assert abs(moved[:, 2].min()) < 1e-7 and np.array_equal(np.delete(s.verts, np.s_[54:108], 0), np.delete(closed.verts, np.s_[54:108], 0))
    assert s.boxes[0][0][2] == closed.boxes[0][0][2] - 0.05 and s.analytic_sdf(np.array([0.9, -0.8, 0.02])) < 0 < closed.analytic_sdf(np.array([0.9, -0.8, 0.02]))


@pytest.mark.parametrize('name', C.DEFECTS)
def test_defect_cases_winding_sign_is_right_and_pseudonormal_sign_is_not(name):
    cs = C.case(name)
    f, _ = cs.ref(0)
    an = cs.analytic()
    wrong_w = int(((f >= 0.5) != (an > 0)).sum())
    vol, _, _ = R.sdf(cs.verts, cs.faces, cs.lo, cs.hi, cs.dim)
    wrong_p = int(((vol > 0) != (an > 0)).sum())
    print('%s: wrong signs of %d: winding %d, pseudonormal %d; smallest |f - 0.5| %.4f' % (name, an.size, wrong_w, wrong_p, np.abs(f - 0.5).min()))
    assert wrong_w == 0
    assert wrong_p >= 1
    assert np.abs(f - 0.5).min() > 10 * C.TOL_F                                          # the reference alone excludes no node (GPU sign test)


@pytest.mark.parametrize('name', ['room_s6_d21', 'room_s6_open_d21'])
def test_pruned_arm_error_and_counts(name):
    cs = C.case(name)
    exact, counts0 = cs.ref(0)
    pruned, counts = cs.ref(3.0, 16)
    nodes, nk = cs.dim ** 3, R.prepare(cs.verts, cs.faces)['info'][0]
    E = np.abs(pruned - exact).max()
    print('%s: E(beta 3, cluster 16) = %.4g; tests %s of %d (%.1f %%)' % (name, E, counts, nodes * nk, 100.0 * counts[0] / (nodes * nk)))
    assert E <= 0.02                                                                     # a 25 x margin to the 0.5 decision gap
    assert counts0 == (nodes * nk, 0)
    assert counts[1] > 0 and counts[0] < nodes * nk


def test_clusters_by_hand():
    cs = C.case('room_s6_d21')
    m = R.prepare(cs.verts, cs.faces)
    order, c, r, N = W.clusters(m['a'], m['b'], m['c'], 16)
    assert sorted(order.tolist()) == list(range(1296)) and len(c) == 81 and c.dtype == r.dtype == N.dtype == np.float32
    codes = W.morton_codes(((m['a'] + m['b']) + m['c']) / 3.0)[order]
    assert (np.diff(codes) >= 0).all()
    tri_n = 0.5 * np.cross(m['b'] - m['a'], m['c'] - m['a'])
    assert np.allclose(N.sum(0), tri_n.sum(0), atol=1e-5) and np.allclose(tri_n.sum(0), 0, atol=1e-6)      # a closed mesh: the area vectors cancel
    for j in (0, 40, 80):
        P = np.concatenate([m[k][order[16 * j:16 * j + 16]] for k in 'abc'])
        assert np.isclose(np.linalg.norm(P - c[j], axis=1).max(), r[j], rtol=1e-6)
    soup = C.case('soup_d24')
    ms = R.prepare(soup.verts, soup.faces)
    assert len(W.clusters(ms['a'], ms['b'], ms['c'], 16)[1]) == 15                       # 228 = 14 x 16 + 4


def test_far_bricks_of_open_rectangle_equal_closed_form_dipole():
    cs = C.case('rectangle_in_16m_box')
    f, counts = cs.ref(3.0, 16)
    mask, closed = C.rectangle_far_nodes(3.0)
    err = np.abs(f - closed)[mask].max()
    print('rectangle: %d far nodes of %d, |f - dipole| %.3g; counts %s' % (mask.sum(), mask.size, err, counts))
    assert mask.sum() >= 512 and err <= 1e-12
    assert counts[1] >= mask.sum() and counts[0] + counts[1] * 2 == mask.size * 2        # one cluster of two triangles: a dipole or both
    exact, _ = cs.ref(0)
    assert np.abs(f - exact).max() <= 0.02 and np.abs(exact).max() <= 0.5 + 1e-12        # an open sheet never winds more than half


def test_exterior_free_lone_box():
    v, fc, (centre, half, _) = C.lone_box()
    lo, hi = centre - half - 0.37, centre + half + 0.37
    f, _ = W.winding(v, fc, lo, hi, 12)
    inside = (np.abs(R.node_positions(lo, hi, 12).astype(np.float64) - centre) < half).all(-1)
    assert inside.any() and (~inside).any()
    assert np.abs(f[inside] + 1.0).max() <= 1e-12 and np.abs(f[~inside]).max() <= 1e-12
    assert ((f < scene_sdf.LEVELS['free']) == inside).all()                             # solid iff f < -0.5
    assert scene_sdf.LEVELS == {'solid': 0.5, 'free': -0.5}


def test_atan2_of_zero_counts_as_zero():
    A, B, Cc = (np.array([[x]], np.float64) for x in ([0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0]))
    assert W.half_omega(np.array([[[0.0, 0, 0]]]), A[None], B[None], Cc[None])[0, 0] == 0.0     # the node on a vertex: det = 0, den = -0


def test_host_run_of_the_kernel_statements_against_restatement(tmp_path):
    """tools/mesh_winding_host_check.hip runs the per-pair, per-dipole and per-cluster statements of csrc/mesh_winding.hip serially on the
    CPU, in the kernel's order of summation: within TOL_F / 4 of the restatement with the same beta on every case, and the same counts."""
    from psi_release_amd import build
    exe = str(tmp_path / 'mesh_winding_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'mesh_winding_host_check.hip'),
                        '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    worst = 0.0
    for name in C.SHAPES + ('room_s6_open_d21', 'rectangle_in_16m_box') + C.DEFECTS:
        cs = C.case(name)
        for beta in (0.0, 3.0):
            ref, counts = cs.ref(beta, 16)
            f, host_counts = C.run_host_check(exe, tmp_path, cs, beta, 16)
            err = float(np.abs(f.astype(np.float64) - ref).max())
            worst = max(worst, err)
            print('%s beta %g: host fp32 vs restatement %.3g; counts %s' % (name, beta, err, host_counts))
            assert host_counts == counts
            assert err <= C.TOL_F / 4
    print('largest: %.3g (TOL_F / 4 = %.3g)' % (worst, C.TOL_F / 4))


def test_symbols_declared_bound_and_refuse_cpu_tensors():
    import torch
    from psi_release_amd import build, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    assert 'mesh_winding.hip' in build.PER_FILE and 'mesh_winding.hip' in build.sources()
    with pytest.raises(hip.PsiHipError):
        ops.mesh_sdf_apply_sign(torch.zeros(8), 0.5, torch.zeros(8))
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    for bad in (dict(beta=-1.0), dict(beta=float('nan')), dict(cluster=4), dict(cluster=257), dict(dim=1)):
        kw = dict(dim=8, beta=3.0, cluster=64)
        kw.update(bad)
        with pytest.raises(hip.PsiHipError):
            ops.mesh_winding_compute(None, lo, hi, **kw)
        with pytest.raises(hip.PsiHipError):
            ops.mesh_winding_count(None, lo, hi, **kw)
    room = synth.make_oriented_room(2)
    with pytest.raises(ValueError):
        scene_sdf.scene_from_mesh(room.verts, room.faces, dim=32, sign='normals')       # raised before a device is touched
    with pytest.raises(ValueError):
        scene_sdf.scene_from_mesh(room.verts, room.faces, dim=32, sign='winding', exterior='void')


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_scene_sdf as S
    finally:
        sys.path.pop(0)
    a = S.parse([str(tmp_path), '--name', 'roomS', '--synthetic', '--dim', '32'])
    assert a.sign == 'pseudonormal' and a.exterior == 'solid' and a.beta == 3.0
    b = S.parse(['scene.ply', str(tmp_path), '--name', 'N', '--sign', 'winding', '--exterior', 'free', '--beta', '0'])
    assert b.sign == 'winding' and b.exterior == 'free' and b.beta == 0.0 and b.dim == 256
    for bad in (['--sign', 'normals'], ['--exterior', 'void'], ['--beta', '-1'], ['--beta', 'nan'], ['--beta', 'inf']):
        with pytest.raises(SystemExit):
            S.parse([str(tmp_path), '--name', 'N', '--synthetic'] + bad)
