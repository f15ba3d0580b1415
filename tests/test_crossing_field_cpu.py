"""The conic distance field of crossing triangle pairs without a GPU: the fp32 restatement against its fp64 form, the
hand-derived reverse mode against central differences, the sign of the gradient, continuity at the two gates, role swap, the host run of
the kernels' statements bit for bit, the aggregates by hand, the planted zeros, the new symbols, the refusals and the script's arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import crossing_field_cases as K
import crossing_field_ref as FR
import surface_crossings_cases as SC

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ['psi_crossing_field_eval', 'psi_crossing_field_pairs', 'psi_crossing_field_grad_rows']

# fp32 against fp64 where the gates agree: |Psi32 - Psi64| and |e32 - e64| / max(1, |e64|).  Four times the largest figure measured over
# every case and both lists (pairs, all candidates), per sigma: 1.15e-3 and 1.16e-3 at sigma = 1e-3 (six 24x46, whose pair of bodies (0, 1)
# is degenerate: h / sigma magnifies the rounding of h a thousandfold), 1.14e-5 and 1.55e-5 at sigma = 0.5.
FP32_TOL = {1e-3: (4.6e-3, 4.7e-3), 0.5: (4.6e-5, 6.2e-5)}
GATE_DISAGREE_SHARE = 0.01
# the reverse mode against central differences: four times the largest |reverse - difference| / max(1, largest |partial| of the evaluation)
# measured over every case, per sigma: 1.38e-6 at sigma = 1e-3 and 2.66e-6 at sigma = 0.5, both on six 24x46 (elsewhere at most 2.4e-8)
GRAD_TOL = {1e-3: 5.6e-6, 0.5: 1.1e-5}
GRAD_LEFT_OUT_SHARE = 0.02
STEP = 1e-7


def _gates(P, Q, sigma, dtype):
    K_, Qd, Pd = FR.Consts(sigma, dtype), np.asarray(Q, dtype), np.asarray(P, dtype)
    with np.errstate(all='ignore'):
        R = FR.Record(Qd[:, 0], Qd[:, 1], Qd[:, 2])
        return np.stack([FR.Eval(R, K_, Pd[:, k]).active for k in range(Pd.shape[1])], 1)


@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('name,res', K.CASES)
@pytest.mark.parametrize('which', ['pairs', 'cand'])
def test_fp32_against_fp64_restatement(name, res, sigma, which):
    c, r = SC.case(name, res), K.ref(name, res, sigma, which)
    if (name, res) in K.PAIR_COUNTS and which == 'pairs':
        assert len(r.pairs) == K.PAIR_COUNTS[(name, res)]
    psi64, e64 = FR.field(c.verts, c.faces, r.pairs, sigma, np.float64)
    P, Q, _ = FR.entries(c.verts, c.faces, r.pairs)
    agree = (_gates(P, Q, sigma, np.float32) == _gates(P, Q, sigma, np.float64)).reshape(-1, 2, 3)
    d_psi = np.abs(r.psi.astype(np.float64) - psi64)[agree].max()
    d_e = (np.abs(r.energy.astype(np.float64) - e64) / np.maximum(1.0, np.abs(e64)))[agree.all(2)].max()
    print('%s %s sigma %g %s: %d evaluations, gates disagree on %d, |dPsi| %.3g, energy %.3g' % (name, res, sigma, which, agree.size,
                                                                                              (~agree).sum(), d_psi, d_e))
    assert (~agree).sum() <= GATE_DISAGREE_SHARE * agree.size
    assert d_psi <= FP32_TOL[sigma][0] and d_e <= FP32_TOL[sigma][1]
    if which == 'cand':                         # both gates close on many evaluations of a candidate list
        assert (r.psi == 0).sum() > 0.2 * r.psi.size and (r.psi != 0).sum() > 0.1 * r.psi.size


def _one_evaluation_lists(name, res, sigma):
    """Every evaluation of the crossing pairs of a case on its own: p [m,1,3] and its receiver [m,3,3], in fp64."""
    c, r = SC.case(name, res), K.ref(name, res, sigma)
    P, Q, _ = FR.entries(c.verts, c.faces, r.pairs)
    return np.asarray(P, np.float64).reshape(-1, 1, 3), np.repeat(np.asarray(Q, np.float64), 3, axis=0)


@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('name,res', K.CASES)
def test_reverse_mode_by_central_differences(name, res, sigma):
    """The fp64 form of the reverse mode, per evaluation and for all 12 partials of Psi^2 (the point, then a, b, c), against central
    differences of the fp64 forward with h = 1e-7.  An evaluation whose stencil straddles h = sigma or Phi = 1 (a gate that differs at any
    of its 24 displaced positions) is left out."""
    p, Q = _one_evaluation_lists(name, res, sigma)
    act = _gates(p, Q, sigma, np.float64)[:, 0]
    p, Q = p[act], Q[act]
    m = len(p)
    ones = np.ones(m)
    _, rows = FR.pair_role(p, Q, sigma, g=ones, dtype=np.float64)                         # [m,4,3]
    x0 = np.concatenate([p, Q], 1)                                                          # [m,4,3]
    diff = np.zeros((m, 4, 3))
    straddles = np.zeros(m, bool)
    for k in range(4):
        for a in range(3):
            f = []
            for s in (+1.0, -1.0):
                x = x0.copy()
                x[:, k, a] += s * STEP
                straddles |= ~_gates(x[:, :1], x[:, 1:], sigma, np.float64)[:, 0]
                f.append(FR.pair_role(x[:, :1], x[:, 1:], sigma, dtype=np.float64)[:, 0] ** 2)
            diff[:, k, a] = (f[0] - f[1]) / (2 * STEP)
    keep = ~straddles
    err = np.abs(rows - diff).reshape(m, 12).max(1) / np.maximum(1.0, np.abs(rows).reshape(m, 12).max(1))
    print('%s %s sigma %g: %d active evaluations, %d left out, largest error %.3g, largest partial %.3g'
          % (name, res, sigma, m, straddles.sum(), err[keep].max(), np.abs(rows).max()))
    assert m > 100 and straddles.sum() <= GRAD_LEFT_OUT_SHARE * m
    assert err[keep].max() <= GRAD_TOL[sigma]


@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('res', ['12x16', '24x46'])
def test_gradient_pushes_the_bodies_apart(res, sigma):
    c, r = SC.case('caps', res), K.ref('caps', res, sigma)
    centre = c.verts.astype(np.float64).mean(1)
    slope = float(r.G['ones'][1].astype(np.float64).sum(0) @ (centre[1] - centre[0]))
    print('caps %s sigma %g: <sum_v dL/dverts[1,v], c1 - c0> = %.6g' % (res, sigma, slope))
    assert slope < 0


def test_whole_loss_directional_derivative():
    """sum_i loss[i] of the fp64 form along a smooth direction, against G of the fp64 rows, where no kink is near."""
    c, sigma = SC.case('caps', '12x16'), 0.5
    pairs = K.ref('caps', '12x16', sigma).pairs
    d = np.random.default_rng(5).standard_normal(c.verts.shape).astype(np.float32)
    rows, targets, _ = FR.grad(c.verts, c.faces, pairs, sigma, np.ones(2), np.float64)
    G = np.zeros((c.verts.size // 3, 3))
    np.add.at(G, targets.reshape(-1), rows.reshape(-1, 3))
    want = float((G.reshape(c.verts.shape) * d.astype(np.float64)).sum())
    (P, Q, _), (Pd, Qd, _) = FR.entries(c.verts, c.faces, pairs), FR.entries(d, c.faces, pairs)
    P, Q, Pd, Qd = (np.asarray(x, np.float64) for x in (P, Q, Pd, Qd))

    def total(s):
        return float((FR.pair_role(P + s * Pd, Q + s * Qd, sigma, dtype=np.float64) ** 2).sum())

    got = (total(1e-7) - total(-1e-7)) / 2e-7
    print('directional derivative: reverse %.9g, differences %.9g' % (want, got))
    assert abs(got - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize('sigma', K.SIGMAS)
def test_continuity_at_both_gates(sigma):
    """Psi of the fp64 form is continuous across h = sigma and Phi = 1: on the receiver (0,0,0) (2,0,0) (0,2,0) (o = (1,1,0), r = sqrt 2) a
    point on the axis just below the apex, and a point just inside the cone at h = 0 and at h = -2 sigma."""
    Q = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]], np.float64)
    psi = lambda p: float(FR.pair_role(np.asarray(p, np.float64).reshape(1, 1, 3), Q, sigma, dtype=np.float64)[0, 0])
    eps = 1e-9
    assert psi([1, 1, sigma]) == 0.0 and psi([1, 1, sigma + eps]) == 0.0
    assert 0 < psi([1, 1, sigma * (1 - eps)]) < 4 * eps                                     # Y(sigma) = 0
    for h in (0.0, -2 * sigma):
        edge = np.sqrt(2.0) * (1 - h / sigma)                                               # rho at Phi = 1
        assert psi([1 + edge * (1 + eps), 1, h]) == 0.0
        inside = psi([1 + edge * (1 - eps), 1, h])
        assert 0 < inside < 4 * eps * (1 + 2 * sigma + 1)
    # Y is C1 at -sigma: value and slope from both sides
    k = FR.Consts(sigma, np.float64)
    quad = lambda h: (k.c0 - k.c1 * h) - (k.c2 * h) * h
    assert abs(quad(-sigma) - ((1 + sigma) - sigma)) < 1e-12 and abs((-k.c1 - 2 * k.c2 * -sigma) - -1.0) < 1e-9


@pytest.mark.parametrize('sigma', K.SIGMAS)
def test_role_swap_bit_for_bit(sigma):
    """A pair given the other way round, (j,t,i,s) in the batch with the two bodies exchanged: the energy columns and psi swap, bit for bit."""
    c, r = SC.case('caps', '12x16'), K.ref('caps', '12x16', sigma)
    swapped = r.pairs[:, [0, 3, 2, 1]]                                                      # bodies stay (0, 1), the faces change places
    order = np.lexsort((swapped[:, 3], swapped[:, 1]))
    psi, energy = FR.field(c.verts[::-1], c.faces, swapped[order], sigma)
    assert K.same_bits(energy, r.energy[order][:, ::-1]) and K.same_bits(psi, r.psi[order][:, ::-1])


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('cf') / 'crossing_field_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off',
                        os.path.join(ROOT, 'tools', 'crossing_field_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _assert_host(h, r, gname):
    for k in ('psi', 'energy', 'pair_energy', 'loss'):
        assert K.same_bits(h[k], getattr(r, k)), k
    assert np.array_equal(h['targets'], r.targets)
    assert K.same_bits(h['rows'], r.rows[gname]) and K.same_bits(h['G'], r.G[gname])


@pytest.mark.parametrize('gname', ['ones', 'uneven'])
@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('name,res', K.CASES)
def test_host_run_of_the_kernel_statements_bit_for_bit(host_exe, tmp_path, name, res, sigma, gname):
    c, r = SC.case(name, res), K.ref(name, res, sigma)
    _assert_host(K.run_host_check(host_exe, tmp_path, c.verts, c.faces, r.pairs, sigma, r.g[gname]), r, gname)
    assert r.loss.max() > 0 and np.abs(r.G[gname]).max() > 0


def test_host_run_on_all_candidates_and_on_the_planted_list(host_exe, tmp_path):
    c, r = SC.case('six', '12x16'), K.ref('six', '12x16', 1e-3, 'cand')
    _assert_host(K.run_host_check(host_exe, tmp_path, c.verts, c.faces, r.pairs, 1e-3, r.g['uneven']), r, 'uneven')
    verts, faces, pairs, psi0 = K.planted()
    r = K.FieldRef(verts, faces, pairs, 0.5)
    _assert_host(K.run_host_check(host_exe, tmp_path, verts, faces, pairs, 0.5, r.g['uneven']), r, 'uneven')
    # no pair: zeros
    h = K.run_host_check(host_exe, tmp_path, verts, faces, pairs[:0], 0.5, r.g['ones'])
    assert not h['G'].any() and not h['pair_energy'].any() and not h['loss'].any() and h['psi'].shape == (0, 2, 3)


def test_planted_zeros():
    """Exact values of the rule: evaluations beyond gate 1, beyond gate 2 and in a collinear receiver give Psi = 0 and zero rows; the
    circumcentre gives Psi = c0 with a zero row through rho = 0."""
    verts, faces, pairs, psi0 = K.planted()
    r = K.FieldRef(verts, faces, pairs, 0.5)
    assert K.same_bits(r.psi[:, 0], psi0)
    rows = r.rows['uneven'].reshape(6, 2, 6, 3)
    dead = [0, 1, 2, 3, 5]
    assert not rows[dead, 0].any() and K.same_bits(rows[dead, 0], np.zeros((5, 6, 3), np.float32))
    assert K.same_bits(r.energy[:, 0], np.array([0, 0, 0, 0, 0.25, 0], np.float32))
    live = rows[4, 0]                       # p = o: h = 0, rho = 0, Psi = 0.5; d Psi^2 / dp = 2 g Psi (1 - 0) Y'(0) n = -g c1 n = -n for g = 1
    assert np.array_equal(live[0], np.array([0, 0, -1.0], np.float32) * K.uneven_g(2)[0])
    assert not live[1:3].any() and np.isfinite(live).all() and np.abs(live[3:]).max() > 0
    assert np.isfinite(r.psi).all() and np.isfinite(r.G['uneven']).all()


def test_aggregates_by_hand():
    pairs = np.array([[0, 1, 0, 5], [0, 1, 2, 0], [0, 2, 2, 7], [1, 0, 2, 0]], np.int32)
    energy = np.array([[1.0, 2.0], [0.5, 0.25], [4.0, 8.0], [16.0, 32.0]], np.float32)
    E, loss = FR.aggregates(pairs, energy, 3)
    assert np.array_equal(E, np.array([[3.0, 0, 4.5], [0, 0, 16.0], [8.25, 32.0, 0]]))
    assert np.array_equal(loss, np.array([7.5, 16.0, 40.25], np.float32))
    # fp64 sums of fp32 values, in pair order: an order another association would round differently
    big = np.array([[1e8, 0], [1.0, 0], [-1e8, 0], [1.0, 0]], np.float32)
    E, _ = FR.aggregates(np.array([[0, k, 1, 0] for k in range(4)], np.int32), big, 2)
    assert E[0, 1] == 2.0 and E[1, 0] == 0.0


def test_symbols_declared_bound_and_refusals():
    import torch
    from psi_release_amd import build, evaluation, hip, ops
    header = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    L = hip.lib()
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.SIGNATURES and hasattr(L, s)
    flags = ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt']
    assert build.PER_FILE['crossing_field.hip'] == flags and 'crossing_field.hip' in build.sources()
    EINVAL = -22
    assert L.psi_crossing_field_eval(None, 0, 0, 0, 0, 0.5, 0, 0, 0) == EINVAL
    assert L.psi_crossing_field_pairs(*([None] + [0] * 10)) == EINVAL
    assert L.psi_crossing_field_grad_rows(None, 0, 0, 0, 0, 0.5, 0, 0, 0, 0) == EINVAL
    faces = torch.tensor([[0, 1, 2], [1, 2, 4]], dtype=torch.int32)
    v = torch.zeros(2, 5, 3)
    pairs = torch.tensor([[0, 0, 1, 1]], dtype=torch.int32)
    calls = (lambda x, **kw: ops.crossing_field(x, faces, pairs, **kw), lambda x, **kw: ops.crossing_penetration(x, faces, **kw),
             lambda x, **kw: ops.crossing_penetration_loss(x, faces, **kw))
    for call in calls:
        with pytest.raises(hip.PsiHipError):                                                # a CPU tensor
            call(v)
        for bad in (v.double(), v[0], torch.zeros(2, 5, 2), torch.zeros(2, 0, 3), v.numpy()):
            with pytest.raises(ValueError):
                call(bad)
        for sigma in (0.0, -1e-3, 0.5000001, float('nan'), float('inf'), None, '1e-3', True):
            with pytest.raises(ValueError):
                call(v, sigma=sigma)
    for bad in (pairs.long(), pairs[0], pairs[:, :3], pairs.numpy(), pairs.float()):
        with pytest.raises(ValueError):
            ops.crossing_field(v, faces, bad)
    for g in (torch.zeros(2), torch.zeros(3, dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError):
            ops.crossing_penetration(v, faces, group=g)
    with pytest.raises(ValueError):
        ops.crossing_penetration_loss(v, faces, mode='fast')
    assert ops.CROSSING_FIELD_SIGMA == 1e-3
    assert {'field', 'penetration_loss', 'field_of_records'} <= set(dir(evaluation.SurfaceCrossings))


def test_entry_script_arguments(tmp_path):
    sys.path.insert(0, UTILS)
    try:
        import utils_eval_body_overlap as E
    finally:
        sys.path.pop(0)
    a = E.parse_args([str(tmp_path), '--crossings'])
    assert not a.field and a.sigma == 1e-3
    b = E.parse_args([str(tmp_path), '--crossings', '--self', '--field', '--sigma', '0.5'])
    assert b.field and b.sigma == 0.5
    for bad in ([str(tmp_path), '--field'], [str(tmp_path), '--crossings', '--sigma', '0.5'], [str(tmp_path), '--crossings', '--field', '--sigma', '0'],
                [str(tmp_path), '--crossings', '--field', '--sigma', '0.6'], [str(tmp_path), '--crossings', '--field', '--sigma', 'nan']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    r = K.ref('six', '12x16', 1e-3)
    rep = E.field_report(r.pair_energy, r.loss, SC.case('six').ref().counts, True)
    assert [p[:2] for p in rep['field_pairs']] == [[0, 1], [0, 5], [1, 5]]
    assert all(e_ij > 0 and e_ji > 0 for _, _, e_ij, e_ji in rep['field_pairs'])
    assert rep['field_ranked'][0] == int(r.loss.argmax()) and sorted(rep['field_ranked']) == list(range(6))
    assert rep['self_energy'] == [0.0] * 6 and set(rep) == {'field_pairs', 'field_loss', 'field_ranked', 'self_energy'}
    assert 'self_energy' not in E.field_report(r.pair_energy, r.loss, SC.case('six').ref().counts, False)
