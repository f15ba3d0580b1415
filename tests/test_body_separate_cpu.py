"""The rigid separation rule without a GPU: the fp32 restatement against its fp64 form within bounds derived from the
operation counts, the Cayley update, the loop on the capsule batches and on thin, the host rehearsal of the kernels' statements bit for
bit (also built with the host sanitizers, as a stand-alone program), the symbols, the refusals and the script's arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import body_overlap_cases as BC
import body_separate_cases as K
import body_separate_ref as R

U = 2.0 ** -24          # the unit roundoff of fp32
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ('psi_body_separate_pose', 'psi_body_separate_wrench', 'psi_body_separate_step')


def _unit_quats(rng, B, max_angle=np.pi):
    axis = rng.normal(size=(B, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-max_angle, max_angle, size=(B, 1))
    return np.concatenate([np.cos(ang / 2), np.sin(ang / 2) * axis], 1).astype(np.float32)


pose_bound = K.pose_bound


def test_pose_fp32_against_fp64_and_orthonormal_R():
    rng = np.random.default_rng(5)
    c = BC.case('c24x46')
    base = c.verts
    quat, transl = _unit_quats(rng, 6), rng.normal(size=(6, 3)).astype(np.float32)
    pivot = R.default_pivot(base)
    x32 = R.pose(base, quat, transl, pivot)
    x64 = R.pose(base, quat, transl, pivot, dtype=np.float64)
    assert x32.dtype == np.float32 and x64.dtype == np.float64
    err, bound = np.abs(x32 - x64).max(), pose_bound(base, pivot, transl)
    print('pose: largest error %.3g, bound %.3g' % (err, bound))
    assert 0 < err <= bound
    # R R^T - I: the entries carry <= 4 U each (above), a row product of three terms twice that: 24 U; the quaternion's own norm, rounded
    # to fp32 per component (|n^2 - 1| <= 2 U to first order), scales R by n^2: 4 U more on the diagonal.  28 U.
    R32 = R.rotation(quat).astype(np.float64)
    dev = np.abs(np.einsum('bij,bkj->bik', R32, R32) - np.eye(3)).max()
    print('R R^T - I: %.3g, bound %.3g' % (dev, 28 * U))
    assert dev <= 28 * U
    # against an independent fp64 rotation of the same quaternion (Rodrigues through the angle and the axis)
    q = quat.astype(np.float64)
    ang = 2 * np.arctan2(np.linalg.norm(q[:, 1:], axis=1), q[:, 0])
    for b in range(6):
        assert np.abs(BC.rotation(q[b, 1:], ang[b]) - R32[b]).max() <= 28 * U


def test_identity_state_returns_the_base_bits():
    c = BC.case('c12x16')
    pivot = R.default_pivot(c.verts)
    st = R.State(6, pivot)
    assert K.same_bits(R.pose(c.verts, st.quat, st.transl, st.pivot), c.verts)
    # without the rule (base - pivot) + pivot would round: the test has teeth
    assert not K.same_bits((c.verts - pivot[:, None]) + pivot[:, None], c.verts)
    st.transl[1, 2] = np.float32(1e-3)
    st.quat[3] = _unit_quats(np.random.default_rng(1), 1, 0.1)
    out = R.pose(c.verts, st.quat, st.transl, st.pivot)
    keep = [0, 2, 4, 5]
    assert K.same_bits(out[keep], c.verts[keep]) and not np.array_equal(out[1], c.verts[1]) and not np.array_equal(out[3], c.verts[3])
    st.transl[1, 2] = np.float32(-0.0)                                                      # a negative zero is zero
    assert K.same_bits(R.pose(c.verts, st.quat, st.transl, st.pivot)[1], c.verts[1])


@pytest.mark.parametrize('V,B', [(178, 6), (1060, 6), (257, 1)])
def test_wrench_against_fp64_sum_of_exact_products(V, B):
    """F: the terms are the fp32 G themselves, exact in fp64; the fp64 sums carry V 2^-53 relative, the one rounding to fp32 U |F|.
    T: a = x - p rounds once (U |a_i|), each product once more, the difference of the two products once: a component (a_i G_j - a_k G_l)
    is off by at most 3 U (|a_i||G_j| + |a_k||G_l|) to first order, hence the sum by 3 U S with S = sum_v (|a_i||G_j| + |a_k||G_l|), a
    small multiple of 2^-24 sum |a||G|; the rounding of the sum adds U |T|.  1 % for the higher orders and the fp64 sums."""
    kc = K.kernel_case(V, B)
    verts, G = kc.steps[3]['verts'], kc.G[3]
    p = kc.steps[3]['before'].pivot + kc.steps[3]['before'].transl
    g6 = R.wrench(verts, G, p)
    assert K.same_bits(g6, kc.steps[3]['g6'])
    a, G64 = verts.astype(np.float64) - p[:, None].astype(np.float64), G.astype(np.float64)
    F, T = G64.sum(1), np.cross(a, G64).sum(1)
    aa, gg = np.abs(a), np.abs(G64)
    S = np.stack([aa[..., 1] * gg[..., 2] + aa[..., 2] * gg[..., 1], aa[..., 2] * gg[..., 0] + aa[..., 0] * gg[..., 2],
                  aa[..., 0] * gg[..., 1] + aa[..., 1] * gg[..., 0]], -1).sum(1)
    errF, errT = np.abs(g6[:, :3] - F), np.abs(g6[:, 3:] - T)
    print('wrench V = %d: force error %.3g, torque error / bound %.3g' % (V, errF.max(), (errT / np.maximum(1.01 * (3 * U * S + U * np.abs(T)), 1e-300)).max()))
    assert (errF <= 1.01 * U * np.abs(F) + 1e-300).all()
    assert (errT <= 1.01 * (3 * U * S + U * np.abs(T)) + 1e-300).all()
    assert errT.max() > 0


def test_chunk_tree_by_hand_and_grid_independence():
    terms = np.zeros((1, 300, 6))
    terms[0, :, 0] = np.arange(300)
    terms[0, 0, 1], terms[0, 128, 1], terms[0, 1, 1] = 1e300, -1e300, 1.0                   # the tree adds lane 0 and lane 128 first
    ch = R.chunk_sums(terms)
    assert ch.shape == (1, 2, 6) and ch[0, 0, 0] == sum(range(256)) and ch[0, 1, 0] == sum(range(256, 300))
    assert ch[0, 0, 1] == 1.0                                                               # a serial sum would give 0
    assert np.array_equal(R.g6_of(ch)[0, :2], np.array([sum(range(300)), 1.0], np.float32))


@pytest.mark.parametrize('scale', [0.1, 1e-2, 1e-4])
def test_cayley_update(scale):
    """The angle of q' q^-1 against |delta|: the Cayley map turns by 2 atan(|delta| / 2) = |delta| - |delta|^3 / 12 + ..., so the two
    differ by at most |delta|^3 / 12; rounding: the four components of q' carry about 4 U each (three products and sums, the division by
    n), an angle is twice an arc: 32 U covers it.  |q'| = 1 within 2 ulp of 1 (2^-22): every component rounds once after a division by
    a norm that is itself good to 1.5 U."""
    rng = np.random.default_rng(17)
    n = 4000
    q = _unit_quats(rng, n)
    delta = rng.normal(size=(n, 3))
    delta = (delta / np.linalg.norm(delta, axis=1, keepdims=True) * rng.uniform(0.1, 1.0, size=(n, 1)) * scale).astype(np.float32)
    q2 = R.quat_step(q, delta)
    assert q2.dtype == np.float32
    norm = np.linalg.norm(q2.astype(np.float64), axis=1)
    assert np.abs(norm - 1).max() <= 2.0 ** -22
    a, b = q2.astype(np.float64), q.astype(np.float64)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    bc = b * np.array([1, -1, -1, -1.0])
    w = a[:, 0] * bc[:, 0] - (a[:, 1:] * bc[:, 1:]).sum(1)
    v = a[:, :1] * bc[:, 1:] + bc[:, :1] * a[:, 1:] + np.cross(a[:, 1:], bc[:, 1:])
    angle = 2 * np.arctan2(np.linalg.norm(v, axis=1), np.abs(w))
    d = np.linalg.norm(delta.astype(np.float64), axis=1)
    excess = np.abs(angle - d) - d ** 3 / 12
    print('cayley at %g: largest |angle - |delta|| beyond |delta|^3 / 12: %.3g (allowed %.3g)' % (scale, excess.max(), 32 * U))
    assert excess.max() <= 32 * U
    axis = v / np.linalg.norm(v, axis=1, keepdims=True) * np.sign(w)[:, None]
    assert np.abs(axis - delta / d[:, None]).max() <= 1e-3 / scale * 1e-2 + 1e-3           # it turns about delta
    delta[::7] = 0
    delta[7, 0] = np.float32(-0.0)
    kept = R.quat_step(q, delta)
    assert K.same_bits(kept[::7], q[::7]) and not K.same_bits(kept[1::7], q[1::7])


def test_step_by_hand():
    st = R.State(2, np.zeros((2, 3), np.float32))
    g = np.array([[1, -2, 0, 0, 0, 4], [3, 3, 3, 3, 3, 3]], np.float32)
    one = R.step(st, g, 1, fixed=[1])
    # the first Adam step moves every touched component by lr (m / c1 = g, sqrt(s / c2) = |g|), whatever its size
    assert np.allclose(one.transl[0], [-0.01, 0.01, 0.0], rtol=1e-5, atol=0) and one.transl[0, 2] == 0
    assert K.same_bits(one.quat[1], st.quat[1]) and not one.transl[1].any() and not one.m[1].any() and not one.s[1].any()
    ang = R.shift_angle(one.quat, one.transl)[1]
    assert abs(ang[0] - 0.01) < 1e-6 and one.quat[0, 3] < 0 and one.quat[0, 1] == 0         # -lr about z
    c1, c2 = R.bias_corrections(3, (0.9, 0.999))
    assert c1 == np.float32(1 - 0.9 ** 3) and c2 == np.float32(1 - 0.999 ** 3)


@pytest.mark.parametrize('name', ['c12x16', 'c12x16_squared'])
def test_loop_separates_within_the_cap(name):
    st, verts, k, separated, trace = K.loop(name)
    print('%s: %d iterations, triples %s, pairs %s' % (name, k, [len(t.triples) for t in trace], [len(t.pairs) for t in trace]))
    assert separated and k <= K.CAP and k == K.ITERATIONS[name] and len(trace) == k + 1
    assert len(trace[-1].triples) == 0 and len(trace[-1].pairs) == 0 and len(trace[0].triples) == 177 and len(trace[0].pairs) == 199
    import body_overlap_ref as BR
    import surface_crossings_ref as SR
    base, faces = K.loop_inputs(name)
    assert not BR.overlap(verts, faces)[0].any() and len(SR.crossings(verts, faces, self_pairs=False).pairs) == 0
    shift, angle = R.shift_angle(st.quat, st.transl)
    assert shift.max() < 0.3 and angle.max() < 0.3
    M = R.transform(st.quat, st.transl, st.pivot)
    x = np.einsum('bkl,bvl->bvk', M[:, :3, :3], base.astype(np.float64)) + M[:, None, :3, 3]
    assert np.abs(x - verts).max() <= 2 * pose_bound(base, st.pivot, st.transl)             # M's own t is one more fp64 form of the same sum


def test_untouched_bodies_keep_their_bits():
    """Bodies 2, 3 and 4 of c12x16 have no inside vertex at the start, and no crossing either; 2 and 3 are never reached and end on their
    base bits.  Body 4 is: the bodies it stands next to are pushed into it."""
    st, verts, k, _, trace = K.loop('c12x16')
    base, _ = K.loop_inputs('c12x16')
    first = trace[0]
    assert set(first.triples[:, 0]) | set(first.triples[:, 1]) | set(first.pairs[:, 0]) | set(first.pairs[:, 2]) == {0, 1, 5}
    touched = set()
    for it in trace:
        touched |= set(it.triples[:, 0]) | set(it.triples[:, 1]) | set(it.pairs[:, 0]) | set(it.pairs[:, 2])
    assert set(range(6)) - touched == set(K.UNTOUCHED)
    for b in K.UNTOUCHED:
        assert K.same_bits(verts[b], base[b]) and R.is_identity(st.quat, st.transl)[b] and not st.m[b].any()
    assert not K.same_bits(verts[4], base[4])


def test_penetration_term_alone_leaves_crossings():
    import surface_crossings_ref as SR
    st, verts, k, separated, trace = K.loop('c12x16_pen_only')
    base, faces = K.loop_inputs('c12x16')
    assert separated and k == K.ITERATIONS['c12x16_pen_only'] and all(len(t.pairs) == 0 for t in trace)
    assert len(SR.crossings(verts, faces, self_pairs=False).pairs) == K.PAIRS_LEFT > 0


def test_fixed_body_keeps_its_state():
    st, verts, k, separated, trace = K.loop('c12x16_fixed0')
    base, _ = K.loop_inputs('c12x16')
    assert separated and k <= K.CAP and k == K.ITERATIONS['c12x16_fixed0']
    start = R.State(6, R.default_pivot(base))
    for key in ('quat', 'transl', 'pivot', 'm', 's'):
        assert K.same_bits(getattr(st, key)[0], getattr(start, key)[0])
    assert K.same_bits(verts[0], base[0]) and any(np.abs(t.g6[0]).max() > 0 for t in trace[:-1])


def test_thin_is_cleared_by_the_crossing_term():
    """72 crossing pairs and not one inside vertex: only the conic field acts."""
    st, verts, k, separated, trace = K.loop('thin')
    assert len(trace[0].pairs) == 72 and all(len(t.triples) == 0 for t in trace)
    assert separated and k <= K.CAP and k == K.ITERATIONS['thin']


def test_no_iteration_of_the_loops_is_ambiguous():
    """The teacher-forced GPU test compares an iteration only where every candidate's fp64 |w - 0.5| exceeds AMBIGUOUS; at most a tenth of
    the iterations may be left out.  On these trajectories none is."""
    for name in ('c12x16', 'c12x16_fixed0'):
        trace = K.loop(name)[4]
        out = [i for i, t in enumerate(trace) if len(t.cand_w) and np.abs(t.cand_w - 0.5).min() <= BC.AMBIGUOUS]
        assert len(out) <= len(trace) // 10 and out == []


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def host_exe(request, tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('bs') / ('body_separate_host_check_' + request.param))
    extra = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'] if request.param == 'sanitized' else []
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off'] + extra +
                       [os.path.join(ROOT, 'tools', 'body_separate_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize('V,B', K.KERNEL_CASES)
def test_host_run_of_the_kernel_statements_bit_for_bit(host_exe, tmp_path, V, B):
    kc = K.kernel_case(V, B)
    got = K.run_host_check(host_exe, tmp_path, kc.base, R.State(B, kc.pivot), kc.G, kc.fixed)
    assert len(got) == K.STEPS
    for k, (g, want) in enumerate(zip(got, kc.steps), 1):
        K.assert_step(g, want, 'step %d' % k)
    last = kc.steps[-1]['state']
    assert np.abs(last.transl).max() > 1e-3 and np.abs(last.quat[:, 1:]).max() > 1e-4 and np.isfinite(last.quat).all()     # it moved
    if B > K.FIXED_BODY:
        start = R.State(B, kc.pivot)
        for b in (K.ZERO_BODY, K.FIXED_BODY):                       # delta == 0 at every step, and a fixed body: the bits they started with
            assert K.same_bits(got[-1]['quat'][b], start.quat[b]) and not got[-1]['transl'][b].any()
            assert K.same_bits(got[-1]['verts'][b], kc.base[b])
        assert np.abs(got[0]['g6'][K.FIXED_BODY]).max() > 0 and not got[0]['g6'][K.ZERO_BODY].any()


def test_host_run_from_a_moved_state_and_with_other_constants(host_exe, tmp_path):
    kc = K.kernel_case(257, 6)
    state = kc.steps[4]['state']
    kw = dict(lr_t=0.003, lr_r=0.02, betas=(0.8, 0.99), eps=1e-6)
    want = K.rehearse(kc.base, state, kc.G[:3], None, **kw)
    got = K.run_host_check(host_exe, tmp_path, kc.base, state, kc.G[:3], None, **kw)
    for g, w in zip(got, want):
        K.assert_step(g, w)


def test_symbols_declared_bound_and_refusals():
    import torch
    from psi_release_amd import build, evaluation, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    assert build.PER_FILE['body_separate.hip'] == ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt']
    assert 'body_separate.hip' in build.sources()
    EINVAL = -22
    assert L.psi_body_separate_pose(None, None, None, None, 1, 1, None, None) == EINVAL
    assert L.psi_body_separate_wrench(None, None, None, 1, 1, None, None, None) == EINVAL
    assert L.psi_body_separate_step(None, 0, None, None, None, None, None, None, 1, 0.9, 0.999, 0.1, 0.001, 1e-8, 0.01, 0.01, None) == EINVAL
    faces = torch.tensor([[0, 1, 2], [1, 2, 4]], dtype=torch.int32)
    v = torch.zeros(2, 5, 3)
    with pytest.raises(hip.PsiHipError):                                                    # CPU tensors
        ops.rigid_separate(v, faces, faces)
    for bad in (v.double(), v[0], torch.zeros(2, 5, 2), torch.zeros(2, 0, 3), torch.zeros(0, 5, 3), v.numpy()):
        with pytest.raises(ValueError):
            ops.rigid_separate(bad, faces, faces)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(max_iter=0), dict(max_iter=-3), dict(max_iter=2.5), dict(lr_t=0.0), dict(lr_t=-0.01), dict(lr_t=nan), dict(lr_t=inf),
               dict(lr_r=0.0), dict(lr_r=nan), dict(lr_r=inf), dict(lr_r='0.01'), dict(sigma=0.0), dict(sigma=0.6), dict(sigma=nan),
               dict(w_pen=-1.0), dict(w_cross=-1e-9), dict(w_pen=0.0, w_cross=0.0), dict(w_pen=nan), dict(penalty='cubed'), dict(mode='fast'),
               dict(betas=(0.9,)), dict(betas=(1.0, 0.999)), dict(eps=-1.0), dict(pivot=torch.zeros(3, 3)), dict(pivot=torch.zeros(2, 3).double()),
               dict(fixed=[2]), dict(fixed=[-1]), dict(fixed=torch.zeros(3, dtype=torch.bool)), dict(group=torch.zeros(2))):
        with pytest.raises(ValueError):
            ops.rigid_separate(v, faces, faces, **kw)
    q, t = torch.zeros(2, 4), torch.zeros(2, 3)
    for call in (lambda: ops.rigid_pose(v, q[:1], t, t), lambda: ops.rigid_pose(v, q, t.double(), t), lambda: ops.rigid_pose(v[0], q, t, t),
                 lambda: ops.rigid_wrench(v, v[:, :4], t), lambda: ops.rigid_wrench(v, v, q), lambda: ops.rigid_state(q),
                 lambda: ops.rigid_step(ops.rigid_state(t), torch.zeros(2, 5), 1), lambda: ops.rigid_step(ops.rigid_state(t), torch.zeros(2, 6), 0),
                 lambda: ops.rigid_step((q, t), torch.zeros(2, 6), 1), lambda: ops.rigid_step(ops.rigid_state(t), torch.zeros(2, 6), 1, lr_t=0.0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(hip.PsiHipError):
        ops.rigid_pose(v, q, t, t)
    assert {'separate', 'separate_records', 'close'} <= set(dir(evaluation.BodySeparator))
    assert ops.SeparationResult._fields == ('verts', 'quat', 'transl', 'pivot', 'transform', 'iterations', 'separated', 'history', 'shift', 'angle')


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_separate_bodies as E
    finally:
        sys.path.pop(0)
    a = E.parse_args([str(tmp_path), str(tmp_path / 'out')])
    assert (a.fixed, a.max_iter, a.lr_t, a.lr_r, a.sigma, a.no_crossings, a.parts, a.no_flip) == ([], 100, 0.01, 0.01, 0.5, False, False, False)
    b = E.parse_args([str(tmp_path), 'o', '--fixed', '0,3', '--max_iter', '7', '--lr_t', '0.02', '--lr_r', '0.005', '--sigma', '1e-3',
                      '--no_crossings', '--parts', '--no_flip', '--out', 'r.json'])
    assert (b.fixed, b.max_iter, b.lr_t, b.lr_r, b.sigma, b.no_crossings, b.parts, b.no_flip, b.out) == ([0, 3], 7, 0.02, 0.005, 1e-3, True, True, True, 'r.json')
    for bad in (['--fixed', 'a'], ['--fixed', '-1'], ['--max_iter', '0'], ['--lr_t', '0'], ['--lr_r', 'nan'], ['--lr_t', 'inf'], ['--sigma', '0'],
                ['--sigma', '0.6'], ['--chunk', '0']):
        with pytest.raises(SystemExit):
            E.parse_args([str(tmp_path), 'o'] + bad)
    with pytest.raises(SystemExit):
        E.parse_args([str(tmp_path)])
    assert E.pairs_of(np.array([[0, 2, 0], [0, 0, 0], [1, 0, 0]])) == [[0, 1, 2, 0], [0, 2, 0, 1]]
