"""The scene term of the rigid separation without a GPU: the fp32 restatement against the fp64 lookup within the
bounds derived in tests/body_separate_scene_cases.py, the analytic floor, the defect of the loop without a scene, the loop with one, the
host rehearsal of the kernel's statements bit for bit (also built with the host sanitizers, as a stand-alone program), the symbol and the
refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import body_overlap_cases as BC
import body_separate_cases as K
import body_separate_ref as R
import body_separate_scene_cases as SC
import body_separate_scene_ref as SR
import sdf_lookup_ref as LR

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')


def _inputs():
    """The capsule vertices and points that cross every face of the box."""
    pts = np.concatenate([BC.case('c12x16').verts.reshape(-1, 3), BC.case('c24x46').verts.reshape(-1, 3), SC.crossing_points(3, 20000)])
    return np.ascontiguousarray(pts, np.float32)


@pytest.mark.parametrize('name', ['random', 'corner'])
def test_restatement_against_the_exact_lookup(name):
    vol, (gmin, gmax) = SC.scene(name), SC.BOX
    pts = _inputs()
    value, g, inside = SR.lookup(vol, gmin, gmax, pts)
    ref = SC.reference(vol, gmin, gmax, pts)
    for a in range(3):                                                      # the points cross every face
        assert (ref['cls'][:, a] == LR.BELOW).sum() > 100 and (ref['cls'][:, a] == LR.ABOVE).sum() > 100
    ev = np.abs(value.astype(np.float64) - ref['value'])
    print('%s: largest value error / bound %.3f, largest bound %.3g' % (name, (ev / ref['bv']).max(), ref['bv'].max()))
    assert (ev <= ref['bv']).all() and ev.max() > 0
    keep = ~ref['near']
    assert ref['near'].mean() <= 0.01
    eg = np.abs(g.astype(np.float64) - ref['grad'])
    print('%s: largest gradient error / bound %.3f, %d points near a face left out' % (name, (eg[keep] / ref['bg'][keep]).max(), int(ref['near'].sum())))
    assert (eg[keep] <= ref['bg'][keep]).all()
    # a clamped axis gives an exact zero, and the mask is the strict one of the fp32 u
    co = LR.cells_coords(gmin, gmax, SC.D, True, pts)
    assert np.array_equal(inside, co['inside']) and (g[~inside] == 0).all()
    assert np.array_equal(inside[keep], ref['inside'][keep])
    planted = np.stack([gmin, gmax]).astype(np.float32)                    # u = 0 exactly, and u = D - 1 within its rounding
    pv, pg, pin = SR.lookup(vol, gmin, gmax, planted)
    assert not pin[0].any() and (pg[0] == 0).all() and pv[0] == vol[0, 0, 0]
    # the sign is the fp64 sign wherever the exact value is beyond the bound; at most 1 % of the points may be nearer
    sure = np.abs(ref['value']) > ref['bv']
    print('%s: %d of %d points within the bound of the sign change' % (name, int((~sure).sum()), len(pts)))
    assert (~sure).mean() <= 0.01
    assert np.array_equal(value[sure] < 0, ref['value'][sure] < 0)


def test_term_gradient_loss_and_count_on_the_floor():
    """Analytic: s = z + 0.005 for every point whose z lies in the box, so grad s = (0, 0, 1) and, by the rule G = -w_scene grad s,
    G = (0, 0, -w_scene) below the floor (the descent step then lifts the body) and exactly 0 above it."""
    c = BC.case('c12x16')
    rng = np.random.default_rng(2)
    verts = (c.verts + rng.uniform([-0.3, -0.3, -0.4], [0.3, 0.3, 0.1], size=(6, 1, 3))).astype(np.float32)
    sdf, gmin, gmax = SC.table('floor')
    ref = SC.reference(sdf[0], gmin[0], gmax[0], verts.reshape(-1, 3))
    s64 = verts[..., 2].astype(np.float64) - SC.FLOOR_Z
    bv, bg = ref['bv'].reshape(6, -1), ref['bg'].reshape(6, -1, 3)
    assert ref['inside'].all() and np.abs(ref['value'].reshape(6, -1) - s64).max() < 1e-6      # the node values are rounded to fp32
    for w in (1.0, 2.0, 0.3):
        p = R.default_pivot(verts)
        out = SR.wrench(verts, p, sdf, gmin, gmax, None, w)
        below, above = s64 < -bv, s64 > bv
        assert below.sum() > 100 and above.sum() > 100 and (below | above).all()
        assert np.array_equal(out.value < 0, below)
        assert (out.G[above] == 0).all() and not np.signbit(out.G[above]).any()
        want = np.array([0.0, 0.0, -np.float32(w)])
        assert (np.abs(out.G[below].astype(np.float64) - want) <= np.float32(w) * bg[below]).all()
        assert (out.G[below][:, :2] == 0).all()                             # the floor does not vary along x or y: differences of equal nodes
        assert np.array_equal(out.count, below.sum(1)) and out.count.dtype == np.int64
        assert np.array_equal(out.count_chunks.sum(1), out.count) and out.count_chunks.dtype == np.int32
        loss64 = np.where(below, -s64, 0.0).sum(1)
        assert (np.abs(out.loss - loss64) <= np.where(below, bv, 0.0).sum(1) + 178 * LR.EPS64 * loss64).all() and out.loss.dtype == np.float64
        # the wrench of these G in fp64: F = (0, 0, -w count), T = sum a x G
        F = R.g6_of(out.chunks, np.float64)
        assert (np.abs(F[:, 2] + np.float32(w) * out.count) <= np.float32(w) * np.where(below, bg[..., 2], 0.0).sum(1) + 1e-12).all()
        terms = R.wrench_terms(verts, out.G, p).astype(np.float64)
        assert K.same_bits(out.chunks, R.chunk_sums(np.where(below[..., None], terms, 0.0)))
    none = SR.wrench(c.verts, R.default_pivot(c.verts), sdf, gmin, gmax, None, 1.0)            # the base stands on the floor
    assert not none.count.any() and not none.chunks.any() and not np.signbit(none.chunks).any() and not none.loss.any() and not none.G.any()


def test_scene_id_is_clamped_and_picks_the_volume():
    kc = SC.kernel_case(178, 6, 'both')
    assert kc.scene_id.tolist() == [1, 0, 2, -1, 0, 1]
    for b, s in enumerate([1, 0, 1, 0, 0, 1]):
        value, g, _ = SR.lookup(kc.sdf[s], kc.gmin[s], kc.gmax[s], kc.verts[b])
        assert K.same_bits(kc.want.value[b], value)
        other = SR.lookup(kc.sdf[1 - s], kc.gmin[1 - s], kc.gmax[1 - s], kc.verts[b])[0]
        assert not K.same_bits(other, value)


def test_the_loop_without_a_scene_pushes_bodies_through_the_floor():
    """The defect this term is for: the existing restatement separates c12x16 in 11 iterations by pushing bodies 0 and 1 under z = 0."""
    st, verts, k, separated, _ = K.loop('c12x16')
    s64 = verts[..., 2].astype(np.float64) - SC.FLOOR_Z
    print('without a scene: %d iterations, %s vertices below the floor, the deepest at s = %.4f m' % (k, (s64 < 0).sum(1).tolist(), s64.min()))
    assert separated and k == K.ITERATIONS['c12x16']
    assert (s64 < 0).sum() > 0 and (s64 < 0).sum() == SC.BELOW_FLOOR_WITHOUT_SCENE and (s64 < 0).sum(1).tolist() == [55, 63, 0, 0, 1, 0]
    assert -0.1 < s64.min() < -0.08
    sdf, gmin, gmax, _ = SC.floor_scene()
    assert SR.wrench(verts, st.pivot + st.transl, sdf, gmin, gmax).count.sum() == SC.BELOW_FLOOR_WITHOUT_SCENE


@pytest.mark.parametrize('w_scene', [1.0, 2.0])
def test_loop_with_the_floor_separates_within_the_cap(w_scene):
    import body_overlap_ref as BR
    import surface_crossings_ref as XR
    st, verts, k, separated, trace = SC.loop(w_scene)
    print('w_scene = %g: %d iterations, in the scene %s, triples %s, pairs %s' % (w_scene, k, [int(t.scene.count.sum()) for t in trace],
                                                                                   [len(t.triples) for t in trace], [len(t.pairs) for t in trace]))
    assert separated and k <= SC.CAP and k == SC.ITERATIONS[w_scene] and len(trace) == k + 1
    c = BC.case('c12x16')
    assert not BR.overlap(verts, c.faces)[0].any() and len(XR.crossings(verts, c.faces, self_pairs=False).pairs) == 0
    assert (verts[..., 2].astype(np.float64) - SC.FLOOR_Z >= 0).all()
    assert not trace[-1].scene.count.any() and trace[-1].clean and trace[-1].stop
    # the loop keeps stepping after the bodies are clear of each other: passes that are clean and still have vertices in the floor
    held = [i for i, t in enumerate(trace) if t.clean and t.scene.count.sum() > 0]
    assert held and not any(trace[i].stop for i in held)
    for b in K.UNTOUCHED:                                                    # bodies 2 and 3 are never reached, by a body or by the floor
        assert K.same_bits(verts[b], c.verts[b]) and R.is_identity(st.quat, st.transl)[b] and not st.m[b].any()
    shift, angle = R.shift_angle(st.quat, st.transl)
    assert shift.max() < 0.3 and angle.max() < 0.3


def test_no_vertex_of_the_loops_is_within_the_bound_of_the_floor():
    """The GPU tests compare counts and lists pass for pass; that needs every vertex of every pass to lie beyond the value bound from
    s = 0, as section 10h needs it of w.  On these trajectories all do."""
    sdf, gmin, gmax, _ = SC.floor_scene()
    for w_scene in (1.0, 2.0):
        for i, t in enumerate(SC.loop(w_scene)[4]):
            ref = SC.reference(sdf[0], gmin[0], gmax[0], t.verts.reshape(-1, 3))
            assert (np.abs(ref['value']) > ref['bv']).all(), (w_scene, i)
            assert np.array_equal(t.scene.value.reshape(-1) < 0, ref['value'] < 0)
            out = [len(t.cand_w) and np.abs(t.cand_w - 0.5).min() <= BC.AMBIGUOUS]
            assert not any(out), (w_scene, i)


def test_without_a_scene_the_loop_is_todays():
    st, verts, k, separated, trace = SC.loop(None)
    st0, verts0, k0, separated0, trace0 = K.loop('c12x16')
    assert (k, separated) == (k0, separated0) == (K.ITERATIONS['c12x16'], True) and K.same_bits(verts, verts0)
    for key in ('quat', 'transl', 'pivot', 'm', 's'):
        assert K.same_bits(getattr(st, key), getattr(st0, key))
    assert all(K.same_bits(a.chunks, b.chunks) and K.same_bits(a.g6, b.g6) for a, b in zip(trace[:-1], trace0[:-1]))


def test_a_fixed_body_in_the_floor_does_not_hold_the_loop_open():
    c = BC.case('c12x16')
    base = c.verts.copy()
    base[3, :, 2] -= base[3, :, 2].min() + np.float32(0.05)                # body 3 meets no other body; now it stands 5 cm in the floor
    st, verts, k, separated, trace = SR.separate(base, c.faces, scene=SC.floor_scene(), fixed=[3], max_iter=SC.CAP)
    assert separated and k <= SC.CAP and trace[-1].scene.count[3] > 0 and trace[-1].scene.count.sum() == trace[-1].scene.count[3]
    assert K.same_bits(verts[3], base[3]) and R.is_identity(st.quat, st.transl)[3] and not st.m[3].any()
    free = SR.separate(base, c.faces, scene=SC.floor_scene(), max_iter=SC.CAP)
    assert free[3] and not free[4][-1].scene.count.any() and not K.same_bits(free[1][3], base[3])


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def host_exe(request, tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('bss') / ('body_separate_scene_host_check_' + request.param))
    extra = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'] if request.param == 'sanitized' else []
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off'] + extra +
                       [os.path.join(ROOT, 'tools', 'body_separate_scene_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize('V,B,name', SC.KERNEL_CASES)
def test_host_run_of_the_scene_statements_bit_for_bit(host_exe, tmp_path, V, B, name):
    kc = SC.kernel_case(V, B, name)
    got = SC.run_host_check(host_exe, tmp_path, kc.verts, kc.p, kc.sdf, kc.gmin, kc.gmax, kc.scene_id, kc.w_scene)
    SC.assert_wrench(got, kc.want, '%d %d %s' % (V, B, name))
    w = kc.want
    assert w.count.sum() > 0 and (w.value >= 0).sum() > 0 and np.abs(w.chunks).max() > 0 and w.loss.max() > 0
    sc = SR.scene_of(kc.scene_id, B, len(kc.sdf))
    for a in range(3):                                                      # points outside the box on every side
        assert (kc.verts[..., a] < kc.gmin[sc][:, None, a]).any() and (kc.verts[..., a] > kc.gmax[sc][:, None, a]).any()


def test_symbol_declared_bound_and_refusals():
    import torch
    from psi_release_amd import hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    s = 'psi_body_separate_scene'
    assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    assert L.psi_body_separate_scene(None, None, None, None, None, None, 1, 1, 2, 1, 1.0, None, None, None, None, None, None) == -22
    assert ops.SeparationResult._fields == ('verts', 'quat', 'transl', 'pivot', 'transform', 'iterations', 'separated', 'history', 'shift', 'angle')
    assert issubclass(ops.SceneSeparationResult, ops.SeparationResult) and ops.SceneSeparationResult._fields == ops.SeparationResult._fields
    r = ops.SceneSeparationResult(*range(10), scene_inside='s')
    assert tuple(r) == tuple(range(10)) and r.angle == 9 and r.scene_inside == 's' and not hasattr(ops.SeparationResult(*range(10)), 'scene_inside')
    faces = torch.tensor([[0, 1, 2], [1, 2, 4]], dtype=torch.int32)
    v, p = torch.zeros(2, 5, 3), torch.zeros(2, 3)
    sdf, lo, hi = torch.zeros(1, 4, 4, 4), torch.zeros(1, 3), torch.ones(1, 3)
    with pytest.raises(hip.PsiHipError):                                    # CPU tensors
        ops.rigid_scene_wrench(v, p, sdf, lo, hi)
    nan, inf = float('nan'), float('inf')
    for bad in (dict(sdf=sdf.double()), dict(sdf=torch.zeros(1, 4, 4, 5)), dict(sdf=torch.zeros(1, 1, 1, 1)), dict(sdf=torch.zeros(4, 4)),
                dict(grid_min=torch.zeros(2, 3)), dict(grid_max=torch.ones(1, 3).double()), dict(grid_max=torch.ones(1, 2)),
                dict(scene_id=torch.zeros(2)), dict(scene_id=torch.zeros(3, dtype=torch.int32)), dict(w_scene=-1.0), dict(w_scene=nan),
                dict(w_scene=inf), dict(w_scene='1'), dict(w_scene=True)):
        kw = dict(sdf=sdf, grid_min=lo, grid_max=hi)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.rigid_scene_wrench(v, p, **kw)
    for call in (lambda: ops.rigid_scene_wrench(v[0], p, sdf, lo, hi), lambda: ops.rigid_scene_wrench(v, p[:1], sdf, lo, hi)):
        with pytest.raises(ValueError):
            call()
    for kw in (dict(scene=(sdf, lo, hi)), dict(scene=sdf), dict(scene=(sdf.double(), lo, hi, None)), dict(scene=(sdf, lo, hi, None), w_scene=0.0),
               dict(scene=(sdf, lo, hi, None), w_scene=-2.0), dict(scene=(sdf, lo, hi, None), w_scene=nan),
               dict(scene=(torch.zeros(1, 4, 5, 4), lo, hi, None)), dict(scene=(sdf, lo, hi, torch.zeros(2)))):
        with pytest.raises(ValueError):
            ops.rigid_separate(v, faces, faces, **kw)
    with pytest.raises(hip.PsiHipError):                                    # a well-formed scene, CPU tensors
        ops.rigid_separate(v, faces, faces, scene=(sdf, lo, hi, None))


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_separate_bodies as E
    finally:
        sys.path.pop(0)
    a = E.parse_args([str(tmp_path), 'o'])
    assert (a.scene_sdf, a.scene_floor, a.w_scene) == (None, None, 1.0)
    b = E.parse_args([str(tmp_path), 'o', '--scene_sdf', 'room', '--w_scene', '2'])
    assert (b.scene_sdf, b.w_scene) == ('room', 2.0)
    c = E.parse_args([str(tmp_path), 'o', '--synthetic', 's', '--scene_floor', '-0.005'])
    assert c.scene_floor == -0.005
    for bad in (['--w_scene', '0'], ['--w_scene', '-1'], ['--w_scene', 'nan'], ['--scene_floor', 'inf'], ['--scene_floor', '0.0'],
                ['--scene_sdf', 'room', '--synthetic', 's', '--scene_floor', '0']):
        with pytest.raises(SystemExit):
            E.parse_args([str(tmp_path), 'o'] + bad)
