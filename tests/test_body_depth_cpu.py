"""Penetration depth without a GPU: the NumPy restatement (tests/body_depth_ref.py) in fp64 against the analytic capsule and in fp32
against fp64, the pinned rows of the shared lists (tests/body_depth_cases.py), the kernel's statements run serially on the host
(tools/body_depth_host_check.hip) bit for bit against the fp32 restatement, the gradient formula against central differences, its sign, the
segment sum, a non-finite face, ``select_shallow`` by hand, the new symbols, the refusals and the script's arguments.

D2_ERR and TOL_D2 = 4 x D2_ERR (tests/body_depth_cases.py) are measured by test_fp32_against_fp64_restatement below."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import body_depth_cases as K
import body_depth_ref as D
import body_overlap_cases as C
import mesh_sdf_ref as M

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ['psi_body_depth_workspace_bytes', 'psi_body_depth_nearest', 'psi_body_depth_finish', 'psi_body_depth_pairs',
           'psi_body_depth_grad_rows', 'psi_segment_sum3']
G_UNEVEN = np.array([1.0, -0.5, 2.0, 0.25, 3.0, 0.75], np.float32)


def _points_and_records(name, which, dtype):
    cs = K.PLANTED if name == 'planted' else C.case(name)
    trip = K.PLANTED.trip if name == 'planted' else K.triples(name, which)
    return cs, trip


def test_restated_routine_is_the_mesh_sdf_routine():
    """closest_vw of tests/body_depth_ref.py hands out v and w; its r and region have the bits of tests/mesh_sdf_ref.py::closest, the
    restatement of the routine csrc/mesh_sdf.hip and csrc/body_depth.hip now share (csrc/closest_point_shared.h), on every (triple, face)
    of the planted case and of the 12 x 16 candidates, in both precisions."""
    for name, which in (('planted', ''), ('c12x16', 'all')):
        cs, trip = _points_and_records(name, which, np.float32)
        for dtype in (np.float32, np.float64):
            a, ab, ac = D.records(cs.verts[trip[0, 1]], cs.faces, dtype)
            p = cs.verts[trip[:, 0], trip[:, 2]].astype(dtype)[:, None, :]
            r, region, v, w = D.closest_vw(p, a[None], ab[None], ac[None])
            r0, region0 = M.closest(p, a[None], ab[None], ac[None])
            assert K.same_bits(r, r0) and np.array_equal(region, region0)
            assert set(np.unique(region)) == set(range(7))
            assert (v[np.isin(region, (2, 3, 4, 5, 6))] == 0).all() and (w[np.isin(region, (1, 4, 5, 6))] == 0).all()


@pytest.mark.parametrize('name,which', K.LISTS)
def test_lists_are_pinned(name, which):
    trip, r32, r64 = K.triples(name, which), K.ref(name, which), K.ref(name, which, np.float64)
    n, hist = K.PINNED[(name, which)]
    got = np.bincount(r32['region'], minlength=7)
    per_pair = np.zeros((6, 6), np.int64)
    np.add.at(per_pair, (trip[:, 0], trip[:, 1]), 1)
    print('%s %s: %d triples, largest pair %d, regions %s, ties %d, fp32 and fp64 winners differ on %d'
          % (name, which, len(trip), per_pair.max(), got.tolist(), r32['ties'].sum(), (r32['face'] != r64['face']).sum()))
    assert len(trip) == n and tuple(got) == hist
    assert (np.diff(C.triple_keys(trip)) > 0).all() and (trip[:, 0] != trip[:, 1]).all()
    assert np.isfinite(r32['depth']).all() and (r32['depth'] >= 0).all()
    assert np.abs(r32['bary'].sum(1) - 1).max() <= 4 * np.finfo(np.float32).eps
    if which == 'all':
        assert int(r32['ties'].sum()) == K.TIES[(name, which)]                          # the tie rule is exercised
        assert (r32['face'] != r64['face']).sum() == (32 if name == 'c12x16' else 78)
        assert set(np.nonzero(got)[0]) == {0, 1, 2, 3, 6}
    else:
        assert got[0] >= 0.99 * n                                                       # seen from inside a convex body: faces
    if name == 'c24x46':
        assert per_pair[5, 1] == (492 if which == 'inside' else 544)                    # two and three triple chunks
        assert per_pair.max() == per_pair[5, 1]


def test_planted_case_reaches_all_seven_regions():
    r32 = K.ref('planted', '')
    got = np.bincount(r32['region'], minlength=7)
    print('planted: regions %s, ties %d' % (got.tolist(), r32['ties'].sum()))
    assert (got > 0).all() and got.sum() == 24 and r32['ties'].sum() > 0
    r64 = K.ref('planted', '', np.float64)
    assert np.abs(r32['depth'] - r64['depth']).max() < 1e-6


@pytest.mark.parametrize('name', ['c12x16', 'c24x46'])
def test_fp64_restatement_against_the_analytic_capsule(name):
    """An inside vertex is inside the mesh, which is inscribed in the analytic capsule (both convex): its distance to the mesh is at most
    its distance to the capsule.  The capsule shrunk by m = r ((1 - cos(pi / n_ring)) + (1 - cos(pi / n_seg))) lies inside the mesh (the
    derivation stands in test_body_overlap_cpu.py), so a ball about the vertex of radius (capsule depth - m) does too: the mesh depth is
    at least the capsule depth - m.  Hence 0 <= -capsule_sdf - depth <= m."""
    cs, trip, r64 = C.case(name), K.triples(name, 'inside'), K.ref(name, 'inside', np.float64)
    m = K.tessellation_bound(cs.n_ring, cs.n_seg)
    cap = np.empty(len(trip))
    for j in np.unique(trip[:, 1]):
        sel = trip[:, 1] == j
        cap[sel] = -C.capsule_sdf(cs.verts[trip[sel, 0], trip[sel, 2]], j)
    gap = cap - r64['depth']
    print('%s: capsule depth - mesh depth in [%.3g, %.3g], bound m = %.3g; deepest %.4f m' % (name, gap.min(), gap.max(), m, r64['depth'].max()))
    slack = 1e-7                                                                        # the vertices are fp32 roundings of the posed mesh
    assert gap.min() >= -slack and gap.max() <= m + slack
    assert r64['depth'].max() > 0.05


def test_fp32_against_fp64_restatement():
    """On d2, not on depth: depth reaches 7e-6 m on c24x46, where the square root turns an absolute error of 1e-9 in d2 into 3e-5.  The
    largest |d2_fp32 - d2_fp64| over the four lists is D2_ERR: measured here (printed), recorded in body_depth_cases.py."""
    worst, worst_case = 0.0, None
    for name, which in K.LISTS:
        r32, r64 = K.ref(name, which), K.ref(name, which, np.float64)
        err = np.abs(r32['d2'].astype(np.float64) - r64['d2'])
        k = int(err.argmax())
        print('%s %s: max |d2 err| %.4g at depth %.4g; smallest depth %.3g' % (name, which, err[k], r64['depth'][k], r64['depth'].min()))
        assert err.max() <= K.TOL_D2
        if err.max() > worst:
            worst, worst_case = float(err.max()), (name, which)
    print('D2_ERR measured: %.4g on %s (recorded %.4g on %s)' % (worst, worst_case, K.D2_ERR, K.D2_ERR_CASE))
    assert worst <= K.D2_ERR and worst > K.D2_ERR / 2 and worst_case == K.D2_ERR_CASE and K.TOL_D2 == 4 * K.D2_ERR
    assert max(np.abs(C.case(n).verts).max() for n in ('c12x16', 'c24x46')) < K.EXTENT


def test_fp32_against_fp64_on_the_workload_mesh():
    """The workload's face count has triangles 1.4 m long and 6.4e-3 m wide, which condition the barycentric quotients worse than the table
    cases do: the largest |d2_fp32 - d2_fp64| over the fixed sample of body_depth_cases.workload() is WORKLOAD_D2_ERR (measured here,
    printed), and the GPU test of that mesh allows 4 x it.  The fp64 depths of the sample obey the tessellation bound."""
    verts, faces, trip, cap = K.workload()
    r32, r64 = D.nearest(verts, faces, trip, np.float32, block=64), D.nearest(verts, faces, trip, np.float64, block=64)
    err = np.abs(r32['d2'].astype(np.float64) - r64['d2'])
    m = K.tessellation_bound(*C.WORKLOAD)
    gap = cap - r64['depth']
    print('workload sample: %d triples, max |d2 err| %.4g at depth %.4g (recorded %.4g); capsule depth - mesh depth in [%.3g, %.3g], m = %.3g'
          % (len(trip), err.max(), r64['depth'][err.argmax()], K.WORKLOAD_D2_ERR, gap.min(), gap.max(), m))
    assert len(trip) == 638 and verts.shape == (6, 10454, 3) and faces.shape == (20904, 3)
    assert err.max() <= K.WORKLOAD_D2_ERR and err.max() > K.WORKLOAD_D2_ERR / 2 and K.TOL_D2_WORKLOAD == 4 * K.WORKLOAD_D2_ERR
    assert gap.min() >= -1e-7 and gap.max() <= m + 1e-7


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('bd') / 'body_depth_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'body_depth_host_check.hip'),
                        '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _assert_rows(got, want):
    for k in ('face', 'region'):
        assert np.array_equal(got[k], want[k]), k
    for k in ('depth', 'r', 'bary'):
        assert K.same_bits(got[k], want[k]), k


@pytest.mark.parametrize('name,which', K.LISTS + [('planted', '')])
def test_host_run_of_the_kernel_statements_bit_for_bit(host_exe, tmp_path, name, which):
    """tools/body_depth_host_check.hip runs the statements of csrc/body_depth_shared.h serially in slice and chunk order: face, region,
    depth, r, bary, the aggregates and G have the bits of the fp32 restatement."""
    cs, trip = _points_and_records(name, which, np.float32)
    want = K.ref(name, which)
    B, V = cs.verts.shape[:2]
    aggregates = which == 'inside'
    g = G_UNEVEN[:B] if B <= 6 else np.ones(B, np.float32)
    for penalty, gg in (('depth', np.ones(B, np.float32)), ('squared', g)) + ((('depth', g), ('squared', np.ones(B, np.float32))) if aggregates else ()):
        got = K.run_host_check(host_exe, tmp_path, cs.verts, cs.faces, trip, gg, penalty, aggregates)
        _assert_rows(got, want)
        assert K.same_bits(got['G'], D.gradient(trip, want, cs.faces, gg, penalty, B, V)), penalty
        assert np.isfinite(got['G']).all() and np.abs(got['G']).max() > 0
    if aggregates:
        for k, a in zip(('max_depth', 'sum_depth', 'sum_sq', 'depth_of', 'loss'), D.aggregates(trip, want['depth'], B, V)):
            assert K.same_bits(got[k], a), k
        assert got['loss'][0].max() > 0 and (got['max_depth'] > 0).sum() == 4


def _tri_distance(p, A, Bv, Cv):
    r, region, _, _ = D.closest_vw(p, A, Bv - A, Cv - A)
    return np.sqrt(D.d2_of(r)), region


@pytest.mark.parametrize('name,which', [('c12x16', 'inside'), ('c24x46', 'inside'), ('c12x16', 'all'), ('planted', '')])
def test_gradient_formula_by_central_differences(name, which):
    """The rows of the gradient, in fp64: for every triple the distance of p to its ONE winning triangle (C1 off the triangle, so no kink
    from a change of winner) is differenced centrally with h = 1e-6.  The formula says +r / d for p and -bary_m r / d for the corners.

    p: the third derivatives of a distance are of the order 1 / d^2, so with d >= 1e-3 the truncation term h^2 / (6 d^2) is about
    1e-12 * 1e6 / 6 = 2e-7; required: < 1e-6 on every row with depth >= 1e-3 (left out: 0 of 177 and 6 of 1047 inside rows).

    Corners: the same bound, on the rows whose three-point stencil stays within ONE of the seven regions.  Moving a corner moves the
    borders of the regions, and where the closest point lies within h of an edge of its triangle the stencil straddles a border: the
    distance is C1 there but its second derivative jumps, and a central difference is then off by h * jump / 4 whatever the formula is
    (c24x46 inside has two such rows, with barycentric coordinates 2.2e-4 and 6.7e-5: their differences miss by 8.1e-6 and 4.3e-6 with
    h = 1e-6 and by 3.3e-10 with h = 1e-7).  Those rows are left out of the corner columns and counted with the shallow ones: together at
    most 1 % of a list."""
    cs, trip = _points_and_records(name, which, np.float64)
    rows = K.ref(name, which, np.float64)
    keep = rows['depth'] >= 1e-3
    if which == 'inside':
        assert (~keep).sum() == (0 if name == 'c12x16' else 6)
    t, face = trip[keep], rows['face'][keep]
    X = cs.verts.astype(np.float64)
    p = X[t[:, 0], t[:, 2]]
    tri = X[t[:, 1][:, None], cs.faces[face]]                                           # [n,3,3]
    d, region = _tri_distance(p, tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.abs(d - rows['depth'][keep]).max() < 1e-12 and np.array_equal(region, rows['region'][keep])
    u = rows['r'][keep] / d[:, None]
    want = np.concatenate([u[:, None, :], -rows['bary'][keep][:, :, None] * u[:, None, :]], 1)      # [n,4,3]
    h, worst_p, worst_c = 1e-6, 0.0, 0.0
    straddles = np.zeros(len(p), bool)
    for who in range(4):
        for a in range(3):
            args = [p.copy(), tri[:, 0].copy(), tri[:, 1].copy(), tri[:, 2].copy()]
            args[who][:, a] += h
            up, region_up = _tri_distance(*args)
            args[who][:, a] -= 2 * h
            down, region_down = _tri_distance(*args)
            err = np.abs((up - down) / (2 * h) - want[:, who, a])
            if who == 0:
                worst_p = max(worst_p, float(err.max()))
            else:
                one_region = (region_up == region) & (region_down == region)
                straddles |= ~one_region
                worst_c = max(worst_c, float(err[one_region].max()))
    left_out = int((~keep).sum() + straddles.sum())
    print('%s %s: %d shallow rows and %d whose corner stencil straddles a border left out of %d; largest |central difference - formula| '
          '%.3g for p, %.3g for the corners; regions %s' % (name, which, (~keep).sum(), straddles.sum(), len(keep), worst_p, worst_c,
                                                            np.bincount(region, minlength=7).tolist()))
    assert worst_p < 1e-6 and worst_c < 1e-6
    assert left_out <= 0.01 * len(keep)
    if name == 'planted':
        assert (np.bincount(region, minlength=7) > 0).all() and left_out == 0          # all seven regions


@pytest.mark.parametrize('penalty', ['depth', 'squared'])
def test_gradient_pushes_the_bodies_apart(penalty):
    """Bodies 0 and 1 of c12x16 stand in each other.  Moving body 0 towards body 1 (t_1 - t_0 = (0.2, 0.05, 0)) raises the loss:
    <dL/dt_0, t_1 - t_0> > 0 with dL/dt_0 = the sum of G over the vertices of body 0, and the opposite for body 1."""
    cs, trip, rows = C.case('c12x16'), K.triples('c12x16', 'inside'), K.ref('c12x16', 'inside')
    sel = ((trip[:, 0] == 0) & (trip[:, 1] == 1)) | ((trip[:, 0] == 1) & (trip[:, 1] == 0))
    sub = {k: v[sel] for k, v in rows.items()}
    G = D.gradient(trip[sel], sub, cs.faces, np.ones(6, np.float32), penalty, 6, cs.verts.shape[1]).astype(np.float64)
    towards = np.asarray(C.POSES[1][2]) - np.asarray(C.POSES[0][2])
    a, b = float(G[0].sum(0) @ towards), float(G[1].sum(0) @ towards)
    print('%s: <dL/dt_0, t_1 - t_0> = %.4g, <dL/dt_1, t_1 - t_0> = %.4g' % (penalty, a, b))
    assert sel.sum() == 48 and a > 0 and b < 0
    assert abs(a + b) <= 1e-4 * abs(a)                                                  # a translation of both bodies changes nothing
    assert not G[2:].any()


def test_segment_sum_by_hand():
    """Rows 0..5 with targets 3, 1, 3, 0, 3, 1: target 3 gets ((0 + x0) + x2) + x4 in that order, which in fp32 is not x4 + x2 + x0:
    with x0 = 1, x2 = 2^-24, x4 = 2^-24 the ordered sum is 1 (each addend is half an ulp and rounds to even), the reverse 1 + 2^-23."""
    e = np.float32(2.0 ** -24)
    rows = np.array([[1, 1, -1], [5, 0, 0], [e, 2, 0], [7, 7, 7], [e, 3, 0.5], [0.25, 0, 1]], np.float32)
    targets = np.array([3, 1, 3, 0, 3, 1])
    out = D.segment_sum3(targets, rows, 5)
    assert out[3].tolist() == [1.0, 6.0, -0.5] and out[1].tolist() == [5.25, 0.0, 1.0] and out[0].tolist() == [7.0, 7.0, 7.0]
    assert not out[2].any() and not out[4].any()
    assert np.float32(np.float32(e + e) + np.float32(1)) == np.float32(1 + 2.0 ** -23) != out[3, 0]
    # the gradient of one triple by hand: region 0 at the centroid of a unit right triangle, one unit above it
    faces = np.array([[0, 1, 2]], np.int32)
    verts = np.zeros((2, 3, 3), np.float32)
    verts[1] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    verts[0, 0] = [0.25, 0.25, 1.0]
    trip = np.array([[0, 1, 0]], np.int32)
    rows1 = D.nearest(verts, faces, trip)
    assert rows1['region'].tolist() == [0] and rows1['depth'].tolist() == [1.0] and rows1['bary'].tolist() == [[0.5, 0.25, 0.25]]
    G = D.gradient(trip, rows1, faces, np.array([2.0, 1.0], np.float32), 'depth', 2, 3)
    assert G[0, 0].tolist() == [0, 0, 2.0] and G[1].tolist() == [[0, 0, -1.0], [0, 0, -0.5], [0, 0, -0.5]]
    G2 = D.gradient(trip, rows1, faces, np.array([2.0, 1.0], np.float32), 'squared', 2, 3)
    assert G2[0, 0].tolist() == [0, 0, 4.0]


def _nonfinite_case():
    """Body 1: face 0 is collinear with corners at 0, 1e20 and 2e20 on the x axis (its products overflow: d2 is a NaN), face 1 a proper
    triangle far from the point; body 0 holds the points."""
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    verts = np.zeros((2, 6, 3), np.float32)
    verts[1] = [[0, 0, 0], [1e20, 0, 0], [2e20, 0, 0], [10, 0, 0], [11, 0, 0], [10, 1, 0]]
    verts[0, :2] = [[3, 1, 0], [10.25, 0.25, 2.0]]
    return verts, faces, np.array([[0, 1, 0], [0, 1, 1]], np.int32)


def test_a_collinear_face_with_a_non_finite_d2_loses(host_exe, tmp_path):
    verts, faces, trip = _nonfinite_case()
    a, ab, ac = D.records(verts[1], faces, np.float32)
    with np.errstate(all='ignore'):
        r, region, _, _ = D.closest_vw(verts[0, :2][:, None, :], a[None], ab[None], ac[None])
        d2 = D.d2_of(r)
        assert np.isnan(d2[:, 0]).all() and np.isfinite(d2[:, 1]).all() and region[:, 0].tolist() == [0, 0]
        keys = D.keys_of(d2)
        assert (keys[:, 0] > keys[:, 1]).all()                                         # the lower face index does not help a NaN
        rows = D.nearest(verts, faces, trip)
    assert rows['face'].tolist() == [1, 1] and rows['region'].tolist() == [6, 0] and rows['depth'].tolist() == [7.0, 2.0]
    for bad in (np.float32(np.inf), np.float32(np.nan), -np.float32(np.nan)):
        assert D.keys_of(np.array([[bad, np.finfo(np.float32).max]], np.float32)).argmin(1).tolist() == [1]
    got = K.run_host_check(host_exe, tmp_path, verts, faces, trip, np.ones(2, np.float32))
    _assert_rows(got, rows)


def test_select_shallow_by_hand():
    """max_depth of four bodies (binary fractions, so that fp32 holds them exactly): 0 and 1 stand 1/32 and 1/16 m in each other, 2 stands
    1/64 m in 0, 3 in nothing.  In order 0..3 with tol 0: 1 and 2 meet 0, so [0, 3].  With tol 1/64: 2 is admitted.  With 1/16: everybody;
    with 0.05 not yet, because the larger of the two directions counts."""
    from psi_release_amd.evaluation import select_shallow
    m = np.zeros((4, 4), np.float32)
    m[0, 1], m[1, 0], m[2, 0] = 1 / 32, 1 / 16, 1 / 64
    assert select_shallow(range(4), m, 0.0) == [0, 3]
    assert select_shallow(range(4), m, 1 / 64) == [0, 2, 3] and select_shallow(range(4), m, 0.0156) == [0, 3]
    assert select_shallow(range(4), m, 0.05) == [0, 2, 3] and select_shallow(range(4), m, 1 / 16) == [0, 1, 2, 3]
    assert select_shallow([1, 2, 0, 3], m, 0.0) == [1, 2, 3] and select_shallow([], m, 0.0) == [] and select_shallow([3, 3], m, 0.0) == [3]
    import torch
    assert select_shallow(range(4), torch.tensor(m), 1 / 64) == [0, 2, 3]
    for order, tol in ((range(4), 0.0), ([3, 2, 1, 0], 0.04), ([1, 0, 2], 0.07)):
        assert select_shallow(order, m, tol) == D.select_shallow(order, m, tol)
    nan = m.copy()
    nan[3, 0] = np.nan
    assert select_shallow(range(4), nan, 1.0) == [0, 1, 2]                               # a depth that is not a number is not shallow
    for bad in (lambda: select_shallow([4], m, 0.0), lambda: select_shallow([0], m[:3], 0.0), lambda: select_shallow([0], m, -1.0)):
        with pytest.raises(ValueError):
            bad()


def test_symbols_declared_bound_and_refusals():
    import ctypes
    import torch
    from psi_release_amd import build, evaluation, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    flags = ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt']
    assert build.PER_FILE['body_depth.hip'] == flags == build.PER_FILE['surface_crossings.hip'] and 'body_depth.hip' in build.sources()
    # the workspace query runs on the host: one 64-bit key per (slice of 2048 faces, triple)
    assert L.psi_body_depth_workspace_bytes(1737, 2116) == 2 * 1737 * 8 and L.psi_body_depth_workspace_bytes(1, 2048) == 8
    assert L.psi_body_depth_workspace_bytes(5, 20904) == 11 * 5 * 8
    assert L.psi_body_depth_workspace_bytes(0, 352) == 0 and L.psi_body_depth_workspace_bytes(2 ** 29, 352) == 0 and L.psi_body_depth_workspace_bytes(4, 0) == 0
    EINVAL = -22
    for fn, n_args in ((L.psi_body_depth_nearest, 10), (L.psi_body_depth_finish, 13), (L.psi_body_depth_pairs, 12), (L.psi_body_depth_grad_rows, 13),
                       (L.psi_segment_sum3, 7)):
        assert fn(*([None] + [0] * (n_args - 1))) == EINVAL                              # PSI_EINVAL for null pointers
    # the ops: shapes and dtypes first, then the device
    faces = torch.tensor([[0, 1, 2], [1, 2, 4]], dtype=torch.int32)
    v = torch.zeros(2, 5, 3)
    trip = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for call in (lambda: ops.body_depth(v, faces, trip), lambda: ops.body_penetration(v, faces), lambda: ops.body_penetration_loss(v, faces)):
        with pytest.raises(hip.PsiHipError):
            call()
    for bad in (v.double(), v[0], torch.zeros(2, 5, 2), torch.zeros(2, 0, 3), v.numpy()):
        for call in (lambda: ops.body_depth(bad, faces, trip), lambda: ops.body_penetration(bad, faces), lambda: ops.body_penetration_loss(bad, faces)):
            with pytest.raises(ValueError):
                call()
    for bad in (trip.long(), trip[0], trip[:, :2], trip.numpy(), trip.float()):
        with pytest.raises(ValueError):
            ops.body_depth(v, faces, bad)
    for g in (torch.zeros(2), torch.zeros(3, dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError):
            ops.body_penetration(v, faces, group=g)
    for pen in ('l1', None, 0):
        with pytest.raises(ValueError):
            ops.body_penetration_loss(v, faces, penalty=pen)
        with pytest.raises(ValueError):
            evaluation.BodyOverlap(faces.numpy()).penetration_loss(v, penalty=pen)
    with pytest.raises(ValueError):
        ops.segment_sum3(torch.zeros(3), torch.zeros(3, 3), 4)
    with pytest.raises(ValueError):
        ops.segment_sum3(torch.zeros(3, dtype=torch.int64), torch.zeros(2, 3), 4)
    with pytest.raises(hip.PsiHipError):
        ops.segment_sum3(torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3), 4)
    assert ops.BODY_DEPTH_PENALTIES == D.PENALTIES and {'depths', 'depths_of_records', 'penetration_loss'} <= set(dir(evaluation.BodyOverlap))


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_eval_body_overlap as E
    finally:
        sys.path.pop(0)
    a = E.parse_args([str(tmp_path)])
    assert not a.depth and a.tol == 0.0
    b = E.parse_args([str(tmp_path), '--depth', '--tol', '0.02', '--out', 'o.json'])
    assert b.depth and b.tol == 0.02 and b.out == 'o.json'
    for bad in ([str(tmp_path), '--tol', '0.02'], [str(tmp_path), '--depth', '--tol', '-1'], [str(tmp_path), '--depth', '--tol', 'x'],
                [str(tmp_path), '--depth', '--tol', 'nan']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    cs, trip, rows = C.case('c12x16'), K.triples('c12x16', 'inside'), K.ref('c12x16', 'inside')
    counts = cs.ref()[0]
    max_depth, sum_depth, _, depth_of, _ = D.aggregates(trip, rows['depth'], 6, cs.verts.shape[1])
    rep = E.depth_report(max_depth, sum_depth, counts, depth_of, 0.05)
    assert [p[:2] for p in rep['depth_pairs']] == [[0, 1], [1, 0], [5, 0], [5, 1]]
    assert all(0 < mean <= mx for _, _, mx, mean in rep['depth_pairs'])
    assert rep['deepest_ranked'][0] == int(depth_of.max(1).argmax()) and sorted(rep['deepest_ranked']) == list(range(6))
    assert rep['shallow'] == D.select_shallow(range(6), max_depth, 0.05) and rep['tol'] == 0.05
    assert set(rep) == {'depth_pairs', 'max_depth', 'deepest', 'deepest_ranked', 'tol', 'shallow'}
    before = E.report_of(counts, cs.ref()[1].sum(1), 0)
    assert not set(before) & set(rep)                                                    # the old fields are what they were
