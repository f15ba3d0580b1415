"""Body against body without a GPU: the NumPy fp64 restatement (tests/body_overlap_ref.py) against the analytic capsule, the pinned rows of
the shared cases (tests/body_overlap_cases.py), the box rule, the kernel's statements run serially on the host
(tools/body_overlap_host_check.hip) against the restatement, ``select_disjoint`` by hand, the new symbols, the refusals and the entry
scripts' arguments.

HOST_ERR and TOL_W = 4 x HOST_ERR (tests/body_overlap_cases.py) are measured by the host-run test below."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import body_overlap_cases as C
import body_overlap_ref as R
from psi_release_amd import synth

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ['psi_body_overlap_create', 'psi_body_overlap_destroy', 'psi_body_overlap_info', 'psi_body_overlap_workspace_bytes',
           'psi_body_overlap_boxes', 'psi_body_overlap_count', 'psi_body_overlap_emit', 'psi_body_overlap_wind', 'psi_body_overlap_decide']


def test_restatement_against_the_analytic_capsule():
    """The mesh is inscribed in the analytic capsule (its vertices lie on it, and both are convex), so a point outside the capsule is
    outside the mesh.  The mesh departs inwards from the capsule by at most m = r ((1 - cos(pi / n_ring)) + (1 - cos(pi / n_seg))): the
    first term is the cone trunk between the two middle rings (it also covers the polar chords' sagitta r (1 - cos(pi / (2 n_ring)))),
    the second the sagitta of the n_seg-gon of a ring, and 1 - cd <= (1 - c) + (1 - d).  12 x 16: m = 0.16 (0.03407 + 0.01921) = 0.00853 m.
    A point deeper than m below the capsule's surface is therefore inside the mesh."""
    n_ring, n_seg = 12, 16
    m = C.RADIUS * ((1 - np.cos(np.pi / n_ring)) + (1 - np.cos(np.pi / n_seg)))
    assert abs(m - 0.00853) < 5e-6
    cs = C.case('c12x16')
    rs = np.random.RandomState(3)
    for j in (0, 2, 5):
        lo, hi = cs.verts[j].min(0) - 0.05, cs.verts[j].max(0) + 0.05
        p = (lo + rs.random_sample((1500, 3)) * (hi - lo)).astype(np.float32)
        d = C.capsule_sdf(p, j)
        w = R.winding(p, cs.verts[j], cs.faces)
        deep, out = d < -m, d > 0
        print('pose %d: %d deep, %d outside, %d in the shell; max |w - 1| deep %.3g, max |w| outside %.3g'
              % (j, deep.sum(), out.sum(), (~deep & ~out).sum(), np.abs(w[deep] - 1).max(), np.abs(w[out]).max()))
        assert deep.sum() >= 100 and out.sum() >= 500
        assert np.abs(w[deep] - 1).max() <= 1e-9 and np.abs(w[out]).max() <= 1e-9


@pytest.mark.parametrize('name', list(C.TABLE))
def test_table_rows_are_pinned(name):
    cs = C.case(name)
    counts, inside, cand, w = cs.ref()
    F, n_cand, largest, nz, margin = C.PINNED[name]
    per_pair = np.zeros((6, 6), np.int64)
    np.add.at(per_pair, (cand[:, 0], cand[:, 1]), 1)
    gap = np.abs(w - 0.5)
    print('%s: F %d, candidates %d, largest pair %d, counts %s, min |w - 0.5| %.5f' % (name, len(cs.faces), len(cand), per_pair.max(),
                                                                                 counts[counts > 0].tolist(), gap.min()))
    assert len(cs.faces) == F and len(cand) == n_cand and per_pair.max() == largest == per_pair[5, 1]
    assert (counts[0, 1], counts[1, 0], counts[5, 0], counts[5, 1]) == nz and counts.sum() == sum(nz)
    assert gap.min() >= margin and (gap <= C.AMBIGUOUS).sum() == 0                       # the restatement alone excludes no candidate
    assert per_pair[1, 4] > 0 and per_pair[4, 1] > 0 and per_pair[2, 5] == (31 if cs.n_seg == 16 else 172)      # boxes meet, nothing inside
    assert per_pair[3].sum() == 0 and per_pair[:, 3].sum() == 0                         # body 3 overlaps nothing
    assert counts[0, 5] == counts[1, 5] == 0                                            # the asymmetry
    per_body = inside.sum(1)
    assert np.array_equal(per_body[:5], counts.sum(1)[:5]) and max(counts[5]) < per_body[5] < counts[5].sum()   # some vertices of 5 are inside 0 AND 1: once in `inside`
    assert (np.diff(C.triple_keys(cand)) > 0).all()                                     # ascending (i, j, v)
    assert (F % R.SLICE) % R.CHUNK != 0                                                 # the last chunk is partial


@pytest.mark.parametrize('name', ['c12x16', 'c12x16_open'])
def test_box_rule_loses_nothing(name):
    cs = C.case(name)
    counts, inside = cs.ref()[:2]
    full_counts, full_inside, full_cand, _ = R.overlap(cs.verts, cs.faces, use_box=False)
    assert len(full_cand) == 6 * 5 * cs.verts.shape[1]
    assert np.array_equal(full_counts, counts) and np.array_equal(full_inside, inside)


def test_groups_in_the_restatement():
    cs = C.case('c12x16')
    g = np.array([0, 0, 1, 1, 0, 1])
    counts, _, cand, _ = R.overlap(cs.verts, cs.faces, group=g)
    assert (g[cand[:, 0]] == g[cand[:, 1]]).all()
    assert counts[0, 1] == 24 and counts[1, 0] == 24 and counts.sum() == 48


def test_host_run_of_the_kernel_statements_against_restatement(tmp_path):
    """tools/body_overlap_host_check.hip runs the statements of csrc/body_overlap_shared.h serially on the CPU in the kernels' chunk and
    slice order: the same candidate list and the same decisions as the restatement on the four table cases.  The largest |w_host - w_fp64|
    is HOST_ERR: this test measures it (it is printed), and body_overlap_cases.py holds the figure and the case that produced it."""
    from psi_release_amd import build
    exe = str(tmp_path / 'body_overlap_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'body_overlap_host_check.hip'),
                        '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    worst, worst_case = 0.0, ''
    for name in C.TABLE:
        cs = C.case(name)
        counts, inside, cand, w = cs.ref()
        h_counts, h_inside, h_cand, h_w = C.run_host_check(exe, tmp_path, cs.verts, cs.faces)
        assert np.array_equal(h_cand, cand)
        err = float(np.abs(h_w.astype(np.float64) - w).max())
        print('%s: host fp32 vs restatement %.4g' % (name, err))
        assert np.array_equal(h_counts, counts) and np.array_equal(h_inside, inside)
        if err > worst:
            worst, worst_case = err, name
    print('HOST_ERR measured: %.4g on %s (recorded: %.4g on %s); TOL_W = %.4g' % (worst, worst_case, C.HOST_ERR, C.HOST_ERR_CASE, C.TOL_W))
    assert worst <= C.HOST_ERR and worst > C.HOST_ERR / 2 and worst_case == C.HOST_ERR_CASE      # the recorded figure is this measurement
    assert C.TOL_W == 4 * C.HOST_ERR and C.TOL_W <= 0.01                                  # the tolerance never reaches into the 0.25 band
    # groups in the host program: the same list as the restatement's
    g = np.array([0, 0, 1, 1, 0, 1], np.int32)
    cs = C.case('c12x16')
    assert np.array_equal(C.run_host_check(exe, tmp_path, cs.verts, cs.faces, g)[2], R.candidates(cs.verts, g))


def test_select_disjoint_by_hand():
    """On the 12 x 16 counts ([0,1] = [1,0] = 24, [5,0] = 44, [5,1] = 85, all else 0), by the rule: in order 0..5 with max_inside 0, body 1
    meets 0 with 24 + 24 = 48 and body 5 meets 0 with 44 + 0, so [0, 2, 3, 4] stay.  With 48, body 1 is admitted (48 <= 48) and body 5
    passes 0 (44) but not 1 (85).  Against body 0 alone, body 5 is rejected only below 44."""
    from psi_release_amd.evaluation import select_disjoint
    counts = C.case('c12x16').ref()[0]
    assert select_disjoint(range(6), counts) == [0, 2, 3, 4]
    assert select_disjoint(range(6), counts, max_inside=48) == [0, 1, 2, 3, 4]
    assert select_disjoint(range(6), counts, max_inside=47) == [0, 2, 3, 4, 5]           # 1 is out (48 > 47), so 5 meets only 0: 44 <= 47
    assert select_disjoint([0, 5], counts, max_inside=43) == [0] and select_disjoint([0, 5], counts, max_inside=44) == [0, 5]
    assert select_disjoint([5, 0, 1], counts) == [5]
    assert select_disjoint([5, 1, 0], counts, max_inside=84) == [5, 0] and select_disjoint([5, 1, 0], counts, max_inside=85) == [5, 1, 0]
    assert select_disjoint([3, 3, 2], counts) == [3, 2] and select_disjoint([], counts) == []
    for order, mx in ((range(6), 0), ([5, 4, 3, 2, 1, 0], 0), ([1, 5, 0], 50)):
        assert select_disjoint(order, counts, mx) == R.select_disjoint(order, counts, mx)
    with pytest.raises(ValueError):
        select_disjoint([6], counts)
    with pytest.raises(ValueError):
        select_disjoint([0], counts[:3])


def test_symbols_declared_bound_and_refusals():
    import ctypes
    import torch
    from psi_release_amd import build, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    assert build.PER_FILE['body_overlap.hip'] == [] and 'body_overlap.hip' in build.sources()
    # the workspace query runs on the host: one fp64 per (slice of 2048 faces, candidate)
    assert L.psi_body_overlap_workspace_bytes(1737, 2116) == 2 * 1737 * 8 and L.psi_body_overlap_workspace_bytes(1, 2048) == 8
    assert L.psi_body_overlap_workspace_bytes(5, 20904) == 11 * 5 * 8
    assert L.psi_body_overlap_workspace_bytes(0, 352) == 0 and L.psi_body_overlap_workspace_bytes(2 ** 31, 352) == 0 and L.psi_body_overlap_workspace_bytes(4, 0) == 0
    # creation refuses before it touches a device
    faces = np.array([[0, 1, 2], [1, 2, 4]], np.int32)
    for bad, V in ((faces, 4), (-faces, 5), (np.zeros((0, 3), np.int32), 4), (faces, 0)):
        with pytest.raises(hip.PsiHipError):
            ops.body_overlap_create(bad, V)
    for bad in (faces.astype(np.int64), faces.reshape(-1), faces[:, :2]):
        with pytest.raises(ValueError):
            ops.body_overlap_create(bad, 5)
    h, EINVAL = ctypes.c_void_p(), -22
    assert L.psi_body_overlap_create(ctypes.byref(h), None, 5, 2) == EINVAL and L.psi_body_overlap_create(None, faces.ctypes.data_as(ctypes.c_void_p), 5, 2) == EINVAL
    for fn, n_args in ((L.psi_body_overlap_boxes, 6), (L.psi_body_overlap_count, 7), (L.psi_body_overlap_emit, 13), (L.psi_body_overlap_wind, 10),
                       (L.psi_body_overlap_decide, 10)):
        assert fn(*([None] + [0] * (n_args - 1))) == EINVAL                                # PSI_EINVAL for null pointers
    # the op: shapes and dtypes first, then the device
    v = torch.zeros(2, 5, 3)
    with pytest.raises(hip.PsiHipError):
        ops.body_overlap(v, torch.tensor(faces))
    for bad in (v.double(), v[0], torch.zeros(2, 5, 2), torch.zeros(2, 0, 3), v.numpy()):
        with pytest.raises(ValueError):
            ops.body_overlap(bad, torch.tensor(faces))
    for g in (torch.zeros(2), torch.zeros(3, dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError):
            ops.body_overlap(v, torch.tensor(faces), group=g)


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_eval_body_overlap as E
        import utils_show_test_results as S
    finally:
        sys.path.pop(0)
    a = E.parse_args([str(tmp_path)])
    assert a.gen_folder == str(tmp_path) and a.max_inside == 0 and not a.no_flip and a.out is None and a.synthetic is None and a.chunk == 512
    b = E.parse_args([str(tmp_path), '--synthetic', 'dir', '--no_flip', '--max_inside', '3', '--out', 'o.json'])
    assert b.synthetic == 'dir' and b.no_flip and b.max_inside == 3 and b.out == 'o.json'
    for bad in ([], [str(tmp_path), '--max_inside', '-1'], [str(tmp_path), '--chunk', '0'], [str(tmp_path), '--max_inside', 'x']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    rep = E.report_of(C.case('c12x16').ref()[0], C.case('c12x16').ref()[1].sum(1), 0)
    assert rep['overlapping_pairs'] == 3 and rep['pairs'] == [[0, 1, 24, 24], [0, 5, 0, 44], [1, 5, 0, 85]]
    assert rep['ranked'] == [5, 0, 1, 2, 3, 4] and rep['per_body'] == [24, 24, 0, 0, 0, 95] and rep['disjoint'] == [0, 2, 3, 4]
    cam = ['--fixed_cam'] + ['0'] * 16
    base = ['gen', '-', 'out']
    assert S.parse_args(base + cam + ['--together']).disjoint is None
    assert S.parse_args(base + cam + ['--together', '--disjoint']).disjoint == 0
    assert S.parse_args(base + cam + ['--together', '--disjoint', '12']).disjoint == 12
    for bad in (base + ['--disjoint'], base + cam + ['--disjoint'], base + cam + ['--together', '--disjoint', '-2']):
        with pytest.raises(SystemExit):
            S.parse_args(bad)
