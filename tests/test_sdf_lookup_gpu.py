"""The SDF lookups on the GPU against the fp64 reference of tests/sdf_lookup_ref.py, per vertex, at borders and bricks.

The fused fitting engine samples through psi_sdf_sample_cells (csrc/sdf_device.h): its own world -> grid map, border mask, cell-major
brick layout and interpolation order, and a grid table per scene in the several-scenes engine.  The vertices come out of the skinning
and cannot be placed, so the GRID is placed around them: a first run in an all-free scene gives the vertices of iteration 1 (they do
not depend on the scene), the box of each case is cut out of their distribution.  Every volume is iid U(-1, 1).

Read back after ONE iteration: `verts`, `penmask`, `gl` (the masked SDF gradient rows, camera-rotated; UNSCALED in the fused backward,
scaled by -w / N where psi_skin_bwd_v_kernel writes them), `stats` (sum of -sdf and count over the penetrating vertices) and the loss
history.  The cell, the weights and the border mask of the reference come from the emulated float32 u (cells_coords, the engine's
statement bit for bit), so no vertex is left out of any comparison; the bounds are sdf_lookup_ref's, derived there.

PSI_WRITE_PROFILES=1 in the environment: the observed error / bound ratios of every case go to profiles/sdf_lookup_bounds.json."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import sdf_lookup_ref as R
from psi_release_amd import ops, synth
from test_pen_skip_gpu import DEV, LOSS, V_SMALL, make_op, read_mask, scene_nothing

pytestmark = pytest.mark.gpu
V = V_SMALL
VPAD = (V + 255) // 256 * 256
W_COL = LOSS['weight_collision']
MAX_AMBIGUOUS = 2
LEFT_OUT_CAP = 0.01
_cache = {}
_records = {}


@pytest.fixture(scope='module', autouse=True)
def _profile_writer():
    yield
    if os.environ.get('PSI_WRITE_PROFILES') == '1' and _records:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        doc = {'what': 'tests/test_sdf_lookup_gpu.py on an MI355X: largest observed error / derived bound per case (sdf_lookup_ref.py)',
               'constants': {'c_value': R.C_VALUE, 'c_grad': R.C_GRAD, 'c_value_operator': R.C_VALUE_OP, 'c_grad_operator': R.C_GRAD_OP},
               'cases': _records}
        with open(os.path.join(root, 'profiles', 'sdf_lookup_bounds.json'), 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


# ---- engines -------------------------------------------------------------------------------------------------------------------------
def bodies_of(B, cam):
    b = synth.make_bodies(21, B)               # (its cam_ext is the identity)
    if cam:
        b['cam_ext'] = synth.make_cam_ext(7, B)
    return b


def read_engine(op, B):
    eng = op._fused
    x, hist, step = eng.read(1)
    assert step == 1
    out = {'verts': eng.buffer('verts', (B, V, 3)).cpu().numpy(),
           'gl': eng.buffer('gl', (B, 3 * VPAD)).cpu().numpy().reshape(B, VPAD, 3),
           'stats': eng.buffer('stats', (8,)).cpu().numpy(), 'loss': float(hist.cpu().numpy()[0, 3])}
    try:
        out['mask'] = read_mask(eng, B, V)
    except Exception:                          # (no fused backward: the engine has no such buffer)
        out['mask'] = None
    return out


def run_once(scenes, B, cam=False, ac=True, slots=None, **extra):
    op = make_op(V, scenes, B, align_corners=ac, **extra)
    if slots is not None:
        op.set_scene_ids(slots)
    r = op.make_step_runner(bodies_of(B, cam))
    r.steps(1)
    return op, r, read_engine(op, B)


def first_verts(B, cam=False):
    """camera-frame (cam: world-frame) vertices [B,V,3] of the first forward"""
    if ('verts0', B, cam) not in _cache:
        _, _, out = run_once(scene_nothing(V), B, cam)
        _cache[('verts0', B, cam)] = out['verts']
    return _cache[('verts0', B, cam)]


def scene_of(vol, gmin, gmax):
    return dataclasses.replace(scene_nothing(V), sdf=np.ascontiguousarray(vol, np.float32), grid_min=np.asarray(gmin, np.float32),
                               grid_max=np.asarray(gmax, np.float32), grid_dim=int(vol.shape[0]))


def straddled_box(verts, q=0.25):
    """per axis the 25 % / 75 % quantiles of the vertex coordinates of ONE body (the first), as float32.  (The quantiles of several
    bodies pooled do not do: the bodies stand 0.3 m apart and are 0.15 m wide, so the pooled coordinates are correlated across the axes
    and whole corner classes stay empty — 0 of 3300 vertices in three of the 27 classes at B = 3.  Around one body every class is
    populated, and the other bodies' vertices only add to them; assert_straddled counts over all of them.)"""
    p = verts[0].reshape(-1, 3).astype(np.float64)
    return np.quantile(p, q, axis=0).astype(np.float32), np.quantile(p, 1.0 - q, axis=0).astype(np.float32)


# ---- the checks ----------------------------------------------------------------------------------------------------------------------
def class_counts(cls):
    code = (cls[:, 0].astype(int) + 1) * 9 + (cls[:, 1].astype(int) + 1) * 3 + (cls[:, 2].astype(int) + 1)
    return np.bincount(code, minlength=27)


def assert_straddled(verts, sc, ac):
    """input condition, from exact_lookup's classes alone: every (below | inside | above)^3 class holds at least 5 vertices; without
    align_corners at least 5 per axis lie inside the box but within its clamped half-cell margin"""
    ex = R.exact_lookup(sc.sdf, sc.grid_min, sc.grid_max, verts.reshape(-1, 3), ac)
    counts = class_counts(ex['cls'])
    assert counts.min() >= 5, 'border classes of the input: %s' % counts.tolist()
    margin = None
    if not ac:
        p = verts.reshape(-1, 3)
        margin = ((p > sc.grid_min[None]) & (ex['u'] <= 0)).sum(0)
        assert margin.min() >= 5, 'vertices in the lower half-cell margin per axis: %s' % margin.tolist()
    return counts, margin


def reference(verts, scs, ac, lookup='cells'):
    """per body its scene's reference: value, masked gradient, value bound, gradient bound — [B,V], [B,V,3], [B,V], [B,V,3]"""
    val, grad, bv, bg, inside, near = [], [], [], [], [], []
    for b, sc in enumerate(scs):
        if lookup == 'cells':
            ce = R.cells_lookup(sc.sdf, sc.grid_min, sc.grid_max, verts[b], ac)
            v_b, g_b = R.interp_bounds(ce['M'], ce['k'])
            val.append(ce['value']); grad.append(ce['grad']); inside.append(ce['inside']); near.append(np.zeros(len(verts[b]), bool))
        else:
            # psi_trilinear has no emulated coordinates here: the exact lookup, with the operator's E_u carried into the value
            # (continuity) and into the gradient (the other axes' weights), and the vertices within E_u of a cell face left out
            D = sc.sdf.shape[0]
            ex = R.exact_lookup(sc.sdf, sc.grid_min, sc.grid_max, verts[b], ac)
            eu = R.eu_operator(sc.grid_min, sc.grid_max, D, ac, verts[b])
            k = ((D - 1) if ac else D) / (sc.grid_max.astype(np.float64) - sc.grid_min.astype(np.float64))
            v_b, g_b = R.interp_bounds(ex['M'], k, R.C_VALUE_OP, R.C_GRAD_OP)
            v_b = v_b + R.transfer_bound(sc.sdf, eu)
            steps = R.node_steps(sc.sdf)
            g_b = g_b + np.stack([eu[:, [c for c in range(3) if c != a]].sum(1) * 2 * steps[a] * k[a] for a in range(3)], 1)
            val.append(ex['value']); grad.append(ex['grad']); inside.append(ex['cls'] == R.INSIDE); near.append(R.near_face(ex['u'], eu, D))
        bv.append(v_b); bg.append(g_b)
    return {'value': np.stack(val), 'grad': np.stack(grad), 'bv': np.stack(bv), 'bg': np.stack(bg), 'inside': np.stack(inside),
            'near': np.stack(near)}


def check_loss(out, ref, neg, amb, rec):
    """stats[3] = sum(-sdf), stats[4] = N over the penetrating vertices, history column 3 = w * sum / N.  Bound of the float32 sum:
    the values' own bounds plus (N - 1) roundings of partial sums <= sum|sdf|; the loss adds the product and the quotient."""
    n_amb = int(amb.sum())
    N_ref = int((neg & ~amb).sum())
    N = float(out['stats'][4])
    assert N == int(N) and N_ref <= N <= N_ref + n_amb, 'count %r against %d (+ %d ambiguous)' % (N, N_ref, n_amb)
    S_ref = float(-ref['value'][neg & ~amb].sum())
    b_sum = float(ref['bv'][neg].sum()) + N * R.EPS * S_ref + float(np.abs(ref['value'][amb]).sum())
    rec['value_sum_ratio'] = abs(float(out['stats'][3]) - S_ref) / b_sum if N_ref else 0.0
    assert abs(float(out['stats'][3]) - S_ref) <= b_sum
    loss_ref = W_COL * S_ref / N if N else 0.0
    b_loss = W_COL * b_sum / max(N, 1.0) + 3 * R.EPS * abs(loss_ref)
    rec['loss_ratio'] = abs(out['loss'] - loss_ref) / b_loss if N_ref else 0.0
    rec['n_penetrating'] = int(N)
    print('  N = %d, loss %.9g against %.9g, |d| / bound = %.3f' % (N, out['loss'], loss_ref, rec['loss_ratio']))
    assert abs(out['loss'] - loss_ref) <= b_loss


def check_case(name, out, scs, ac, cam=None, lookup='cells', scaled=False, contact=None):
    """The assertions of a case over ALL vertices.  scs: the scene of every body.  cam [B,4,4]: gl = C^T g.  scaled: gl carries the factor
    -w / N and there is no mask (no fused backward); `contact` are the vertices whose rows also hold the contact term there."""
    verts, gl, mask = out['verts'], out['gl'], out['mask']
    B = verts.shape[0]
    ref = reference(verts, scs, ac, lookup)
    neg = ref['value'] < 0
    amb = np.abs(ref['value']) <= ref['bv']
    rec = {'n_sign_ambiguous': int(amb.sum()), 'n_left_out': int(ref['near'].sum())}
    assert ref['near'].mean() <= LEFT_OUT_CAP
    assert amb.sum() <= MAX_AMBIGUOUS, '%d vertices within their value bound of zero' % int(amb.sum())
    assert not (gl[:, V:] != 0).any(), 'padding rows'
    g_ref, b_g = np.where(neg[..., None], ref['grad'], 0.0), ref['bg'].copy()
    if mask is not None:
        assert not mask[:, V:].any(), 'padding bits set'
        assert np.array_equal(mask[:, :V][~amb], neg[~amb]), 'penmask is not sdf < 0 of the reference'
        set_ = mask[:, :V]
    else:
        set_ = neg
    if cam is not None:
        C = cam[:, :3, :3].astype(np.float64)
        l1 = np.abs(g_ref).sum(2)
        g_ref = np.einsum('brj,bvr->bvj', C, g_ref)
        b_g = np.einsum('brj,bvr->bvj', np.abs(C), b_g) + 3 * R.EPS * l1[..., None]
    check = ~amb & ~ref['near']
    if scaled:
        N = np.float32(out['stats'][4])
        sp = np.float32(-np.float32(W_COL) / N) if N > 0 else np.float32(0)            # FitGradSource::take: one float32 divide
        g_ref, b_g = g_ref * float(sp), b_g * abs(float(sp)) + R.EPS * np.abs(g_ref * float(sp))      # ... and one more product
        check = check & ~np.isin(np.arange(V), contact)[None, :]
        assert np.array_equal((gl[:, :V] != 0).any(2)[check], (neg & ref['inside'].any(2))[check]), 'a row is non-zero exactly where sdf < 0'
    err = np.abs(gl[:, :V].astype(np.float64) - g_ref)
    ratio = np.where(check[..., None] & set_[..., None], err / np.maximum(b_g, 1e-300), 0.0)
    rec['grad_ratio'] = float(ratio.max())
    print('%s: %d of %d rows set, max gradient |d| / bound = %.3f, %d sign-ambiguous' % (name, int(set_.sum()), B * V, ratio.max(), int(amb.sum())))
    assert (err[check & set_] <= b_g[check & set_]).all(), 'gl rows against the reference: max |d| / bound = %.3f' % ratio.max()
    assert (gl[:, :V][check & ~set_] == 0).all(), 'a row with a clear bit is not zero'
    if cam is None:
        # the border rule, as numbers: the component of a clamped axis is exactly zero while the row's other components are not
        rows = check & set_
        clamped = rows[..., None] & ~ref['inside']
        assert (gl[:, :V][clamped] == 0).all(), 'a clamped axis has a non-zero gradient component'
        assert (gl[:, :V][rows[..., None] & ref['inside']] != 0).all(), 'an unclamped component of a penetrating vertex is zero'
        rec['n_rows_partly_clamped'] = int((clamped.any(2) & ~clamped.all(2)).sum())
    check_loss(out, ref, neg, amb, rec)
    _records[name] = rec
    return ref, rec


def straddled_case(D, ac, B, seed, cam=False):
    gmin, gmax = straddled_box(first_verts(B, cam))
    return scene_of(R.random_volume(seed, D), gmin, gmax)


# ---- (a) straddled box, default engine ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('D', [4, 12, 16])
def test_straddled_box(D, ac, B):
    """one brick, three bricks per axis (not a power of two), four; the box cuts the body on every side"""
    sc = straddled_case(D, ac, B, 1000 + D)
    op, _, out = run_once(sc, B, ac=ac)
    assert out['mask'] is not None, 'the default engine has the fused backward'
    counts, margin = assert_straddled(out['verts'], sc, ac)
    name = 'straddled D=%d ac=%d B=%d' % (D, ac, B)
    _, rec = check_case(name, out, [sc] * B, ac)
    rec['border_classes'] = counts.tolist()
    if margin is not None:
        rec['half_cell_margin'] = margin.tolist()


# ---- (b) planted exact hits -----------------------------------------------------------------------------------------------------------
PLANT_H = 2.0 ** -4


def plant(axis, where, verts):
    """box and vertex v* (body 0) so that the engine's float32 u[axis] of v* is exactly 0 | 3 | D - 1 = 7; the other axes straddled"""
    D, h = 8, PLANT_H
    gmin, gmax = straddled_box(verts)
    off = {'lower': 0.0, 'node': 3 * h, 'upper': 7 * h}[where]
    target = {'lower': 0.0, 'node': 3.0, 'upper': 7.0}[where]
    for v in np.argsort(np.abs(verts[0, :, axis] - 0.6)):                    # x* > 7 h: x* - 7 h .. x* all on x*'s own float32 lattice
        x = verts[0, v, axis]
        if not x > 7 * h:
            continue
        lo, hi = gmin.copy(), gmax.copy()
        lo[axis] = np.float32(np.float64(x) - off)
        hi[axis] = np.float32(np.float64(lo[axis]) + 7 * h)
        if np.float64(lo[axis]) != np.float64(x) - off or np.float64(hi[axis]) - np.float64(lo[axis]) != 7 * h:
            continue
        co = R.cells_coords(lo, hi, D, True, verts[0, v])
        if co['u'][0, axis] == np.float32(target):
            return lo, hi, int(v)
    raise AssertionError('no vertex can be planted')


@pytest.mark.parametrize('where', ['lower', 'node', 'upper'])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_planted_exact_hits(axis, where):
    D, B, ac = 8, 1, True
    v0 = first_verts(B)
    lo, hi, vs = plant(axis, where, v0)
    vol = R.random_volume(2000 + 3 * axis + len(where), D)
    if R.cells_lookup(vol, lo, hi, v0[0, vs], ac)['value'][0] > 0:
        vol = -vol                                                             # v* penetrates
    sc = scene_of(vol, lo, hi)
    op, _, out = run_once(sc, B, ac=ac)
    assert np.array_equal(out['verts'], v0), 'the first forward does not depend on the scene'
    ce = R.cells_lookup(vol, lo, hi, out['verts'][0, vs], ac)
    target = {'lower': 0.0, 'node': 3.0, 'upper': 7.0}[where]
    assert ce['u'][0, axis] == np.float32(target) and ce['w'][0, axis] == 0 and ce['cell'][0, axis] == int(target)
    assert ce['value'][0] < -R.interp_bounds(ce['M'], ce['k'])[0][0], 'v* must penetrate beyond its value bound'
    assert out['mask'][0, vs]
    g = out['gl'][0, vs]
    if where == 'node':
        # the node belongs to the UPPER cell (weight 0): its slope, which is not the lower cell's
        assert ce['inside'][0, axis]
        cell = ce['cell'].copy()
        cell[0, axis] -= 1
        w = ce['w'].astype(np.float64).copy()
        w[0, axis] = 1.0
        _, gg, M = R._interp(vol, cell, w)
        bound = R.interp_bounds(ce['M'], ce['k'])[1][0, axis]
        assert abs(g[axis] - ce['grad'][0, axis]) <= bound
        assert abs(gg[0, axis] * ce['k'][axis] - ce['grad'][0, axis]) > 1e3 * bound, 'the two cells have the same slope: broken test'
    else:
        assert not ce['inside'][0, axis]
        assert g[axis] == 0, 'u == 0 and u == D - 1 are outside: the inequalities of in[] are strict'
        others = [a for a in range(3) if a != axis and ce['inside'][0, a]]
        assert all(g[a] != 0 for a in others)
    check_case('planted axis=%d %s' % (axis, where), out, [sc], ac)


# ---- (c) the whole body outside -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['+x', '-z'])
def test_whole_body_outside(side):
    """a box 100 m away: every vertex is clamped on that axis, its component is exactly zero everywhere, the values are the face's"""
    D, B, ac = 12, 3, True
    gmin, gmax = straddled_box(first_verts(B))
    axis = 0 if side == '+x' else 2
    ext = gmax[axis] - gmin[axis]
    if side == '+x':
        gmin[axis], gmax[axis] = np.float32(100.0), np.float32(100.0) + ext
    else:
        gmin[axis], gmax[axis] = np.float32(-100.0) - ext, np.float32(-100.0)
    sc = scene_of(R.random_volume(3000 + axis, D), gmin, gmax)
    op, _, out = run_once(sc, B, ac=ac)
    ref, rec = check_case('outside ' + side, out, [sc] * B, ac)
    assert not ref['inside'][..., axis].any()
    assert (out['gl'][..., axis] == 0).all()
    co = R.cells_coords(gmin, gmax, D, ac, out['verts'].reshape(-1, 3))
    assert (co['cell'][:, axis] == (0 if side == '+x' else D - 1)).all() and (co['w'][:, axis] == 0).all()
    assert out['mask'].any() and not out['mask'][:, :V].all(), 'both signs occur on a face of an iid volume'
    rec['border_classes'] = class_counts(R.exact_lookup(sc.sdf, gmin, gmax, out['verts'].reshape(-1, 3), ac)['cls']).tolist()


# ---- (d) camera -----------------------------------------------------------------------------------------------------------------------
def test_camera():
    """gl = C^T g: the dot product's three roundings, each of a partial sum <= |g|_1, join the bound"""
    D, B, ac = 12, 3, True
    sc = straddled_case(D, ac, B, 4000, cam=True)
    op, _, out = run_once(sc, B, cam=True, ac=ac)
    assert_straddled(out['verts'], sc, ac)
    check_case('camera D=12 B=3', out, [sc] * B, ac, cam=synth.make_cam_ext(7, B))


# ---- (e) several scenes ---------------------------------------------------------------------------------------------------------------
def test_several_scenes():
    """three grids of different D and box in one engine, two-body workgroups straddling scenes; then other slots on the same engine"""
    B, ac = 5, True
    slots = [2, 0, 1, 1, 0]
    v0 = first_verts(B)
    scenes = []
    for s, D in enumerate([4, 12, 8]):
        # around the (first) body that uses it, cut at its terciles: a third of that body below, inside and above per axis (scene 2 has
        # ONE body for its 27 classes)
        gmin, gmax = straddled_box(v0[slots.index(s)][None], 1.0 / 3.0)
        scenes.append(scene_of(R.random_volume(5000 + s, D), gmin, gmax))
    op, r, out = run_once(scenes, B, ac=ac, slots=slots)
    for s in range(3):
        counts, _ = assert_straddled(out['verts'][[b for b in range(B) if slots[b] == s]], scenes[s], ac)
    check_case('scenes slots=%s' % slots, out, [scenes[s] for s in slots], ac)
    slots2 = [0, 1, 2, 0, 2]
    op.set_scene_ids(slots2)
    r = op.make_step_runner(bodies_of(B, False))
    r.restart()
    r.steps(1)
    out2 = read_engine(op, B)
    assert np.array_equal(out2['verts'], out['verts'])
    check_case('scenes slots=%s' % slots2, out2, [scenes[s] for s in slots2], ac)
    assert not np.array_equal(out2['mask'], out['mask']), 'the results follow the new slots'


# ---- (f) the arms nobody runs by choice -----------------------------------------------------------------------------------------------
def test_split_scene_two_bodies_per_workgroup(monkeypatch):
    """PSI_SPLIT_SCENE=1, PSI_SKIN_NB=2: skinning + SDF as a launch of its own, two bodies per workgroup, the last pair ragged (B = 3).
    No fused backward: psi_skin_bwd_v_kernel writes gl from the stored masked gradient times -w / N (FitGradSource::take) — and adds the
    contact term on the contact vertices, which are therefore compared through their sign only."""
    D, B, ac = 12, 3, True
    monkeypatch.setenv('PSI_SPLIT_SCENE', '1')
    monkeypatch.setenv('PSI_SKIN_NB', '2')
    sc = straddled_case(D, ac, B, 1000 + D)
    op, _, out = run_once(sc, B, ac=ac)
    assert out['mask'] is None, 'this arm has no fused backward'
    assert_straddled(out['verts'], sc, ac)
    check_case('split scene NB=2', out, [sc] * B, ac, scaled=True, contact=op.contact_vertex_ids().cpu().numpy())


def _same_as_operator(out, sc, ac):
    """psi_trilinear in the engine and in the operator: same device function, same inputs — the same numbers (-0 = +0).  (This found the
    one defect of the lookups: with the compiler free to contract, the two kernels fused different products of psi_trilinear and 79 of
    9900 gradient entries differed in their last bits, 1.5e-5 at most; sdf_device.h now writes the fused products out.)"""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    x = t(out['verts']).requires_grad_()
    val = ops.sdf_sample(x, t(sc.sdf), t(sc.grid_min), t(sc.grid_max), align_corners=ac)
    val.sum().backward()
    neg = val.detach().cpu().numpy() < 0
    want = np.where(neg[..., None], x.grad.cpu().numpy(), np.float32(0))
    d = np.abs(out['gl'][:, :V].astype(np.float64) - want)
    print('  engine against operator: %d mask bits differ, %d of %d gl entries differ, largest |d| = %.3g (relative %.3g)'
          % (int((out['mask'][:, :V] != neg).sum()), int((d != 0).sum()), d.size, d.max(), (d / np.maximum(np.abs(want), 1e-30)).max()))
    assert np.array_equal(out['mask'][:, :V], neg)
    assert np.array_equal(out['gl'][:, :V], want)


@pytest.mark.parametrize('arm', ['PSI_SDF_LINEAR', 'D=6'])
def test_plain_volume_arms(monkeypatch, arm):
    """PSI_SDF_LINEAR=1, and D = 6 with nothing set — the plain-volume fallback of psi_fit_create for a D the cell copy cannot hold"""
    D, B, ac = (12, 3, True) if arm == 'PSI_SDF_LINEAR' else (6, 3, True)
    if arm == 'PSI_SDF_LINEAR':
        monkeypatch.setenv('PSI_SDF_LINEAR', '1')
    sc = straddled_case(D, ac, B, 1000 + D)
    op, _, out = run_once(sc, B, ac=ac)
    assert out['mask'] is not None
    assert_straddled(out['verts'], sc, ac)
    _same_as_operator(out, sc, ac)
    check_case('plain volume ' + arm, out, [sc] * B, ac, lookup='operator')


# ---- (g) the operator at planted points -----------------------------------------------------------------------------------------------
OP_BOXES = [((0.7, -2.1, 3.3), (1.9, -0.4, 3.9)), ((-5.25, 0.031, -0.77), (-4.0, 2.6, -0.12))]


def planted_points(gmin, gmax, D, seed):
    """every node (both conventions), gmin and gmax, one float32 step outside and inside each face, one cell outside, 1e6 outside, and
    uniform points over the box enlarged by half its extent; returns the points and the rows that sit exactly on / beyond a border"""
    rs = np.random.RandomState(seed)
    mn, mx = gmin.astype(np.float64), gmax.astype(np.float64)
    ext = mx - mn
    mid = ((mn + mx) / 2).astype(np.float32)
    out = []
    for nodes in (np.arange(D) / (D - 1), (np.arange(D) + 0.5) / D):
        out.append(np.stack(np.meshgrid(*[mn[a] + nodes * ext[a] for a in range(3)], indexing='ij'), -1).reshape(-1, 3).astype(np.float32))
    on = [gmin.copy(), gmax.copy()]
    for a in range(3):
        for face, away in ((gmin, -1), (gmax, 1)):
            p = mid.copy()
            p[a] = np.nextafter(face[a], np.float32(-away * np.inf))           # one float32 step inside
            out.append(p[None])
            p = mid.copy()
            p[a] = np.nextafter(face[a], np.float32(away * np.inf))            # one float32 step outside
            on.append(p)
            for far in (ext[a] / (D - 1), 1e6):
                p = mid.copy()
                p[a] = np.float32(face[a] + away * far)
                on.append(p)
            p = mid.copy()
            p[a] = face[a]
            on.append(p)
    on = np.stack(on).astype(np.float32)
    out.append(on)
    out.append(rs.uniform(mn - 0.5 * ext, mx + 0.5 * ext, (3000, 3)).astype(np.float32))
    pts = np.concatenate(out)
    first_on = sum(len(o) for o in out[:-2])
    return pts, np.arange(first_on, first_on + len(on))


def check_operator(name, sdf, gmin, gmax, pts, sid, ac):
    """ops.sdf_sample on pts [B,n,3] with scene_id sid against exact_lookup: value everywhere, gradient away from the cell faces"""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    x = t(pts).requires_grad_()
    val = ops.sdf_sample(x, t(sdf), t(gmin), t(gmax), scene_id=None if sid is None else t(np.asarray(sid, np.int32)), align_corners=ac)
    val.sum().backward()
    val, grad = val.detach().cpu().numpy(), x.grad.cpu().numpy()
    D = sdf.shape[-1]
    worst_v = worst_g = 0.0
    left, total = 0, 0
    exs = []
    for b in range(pts.shape[0]):
        s = 0 if sid is None else int(sid[b])
        vol, mn, mx = sdf.reshape(-1, D, D, D)[s], gmin.reshape(-1, 3)[s], gmax.reshape(-1, 3)[s]
        ex = R.exact_lookup(vol, mn, mx, pts[b], ac)
        eu = R.eu_operator(mn, mx, D, ac, pts[b])
        k = ((D - 1) if ac else D) / (mx.astype(np.float64) - mn.astype(np.float64))
        bv, bg = R.interp_bounds(ex['M'], k, R.C_VALUE_OP, R.C_GRAD_OP)
        bv = bv + R.transfer_bound(vol, eu)
        ev = np.abs(val[b] - ex['value'])
        assert (ev <= bv).all(), '%s: value, max |d| / bound = %.3f' % (name, (ev / bv).max())
        out_ = R.near_face(ex['u'], eu, D)
        steps = R.node_steps(vol)
        mixed = np.stack([eu[:, [c for c in range(3) if c != a]].sum(1) * 2 * steps[a] * k[a] for a in range(3)], 1)
        eg = np.abs(grad[b] - ex['grad'])
        assert (eg[~out_] <= (bg + mixed)[~out_]).all(), '%s: gradient, max |d| / bound = %.3f' % (name, (eg / (bg + mixed))[~out_].max())
        worst_v, worst_g = max(worst_v, float((ev / bv).max())), max(worst_g, float((eg / (bg + mixed))[~out_].max()) if (~out_).any() else 0.0)
        left, total = left + int(out_.sum()), total + len(out_)
        exs.append(ex)
    return val, grad, exs, {'value_ratio': worst_v, 'grad_ratio': worst_g, 'n_left_out': left, 'n_points': total}


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('D', [2, 3, 5, 16])
def test_operator_at_planted_points(D, ac):
    """S = 2 volumes with different boxes; body 0 samples scene 1 and body 1 scene 0; all planted points in one call (several blocks of
    256 and a partial one), then V = 1 and V = 257"""
    boxes = [(np.asarray(lo, np.float32), np.asarray(hi, np.float32)) for lo, hi in OP_BOXES]
    sdf = np.stack([R.random_volume(6000 + D, D), R.random_volume(6100 + D, D)])
    gmin, gmax = np.stack([b[0] for b in boxes]), np.stack([b[1] for b in boxes])
    sid = [1, 0]
    planted = [planted_points(*boxes[s], D, 60 + D + s) for s in sid]
    n = min(len(p[0]) for p in planted)
    pts = np.stack([p[0][:n] for p in planted])                                # (the uniform tail is cut to a common length)
    name = 'operator D=%d ac=%d' % (D, ac)
    val, grad, exs, rec = check_operator(name, sdf, gmin, gmax, pts, sid, ac)
    uniform = slice(n - 2000, n)
    left_uniform = sum(int(R.near_face(exs[b]['u'][uniform], R.eu_operator(gmin[sid[b]], gmax[sid[b]], D, ac, pts[b, uniform]), D).sum()) for b in range(2))
    assert left_uniform <= LEFT_OUT_CAP * 2 * 2000, 'uniform points left out of the gradient comparison'
    rec['n_left_out_uniform'] = left_uniform
    # exactly on or beyond a border: the operator's chain gives u = 0 and u = D - 1 EXACTLY at x == gmin and x == gmax, so the component
    # of that axis is exactly zero there — nothing left out
    for b in range(2):
        rows = planted[b][1]
        ex = exs[b]
        clamped = ex['cls'][rows] != R.INSIDE
        assert clamped.any(1).all()
        assert (grad[b][rows][clamped] == 0).all(), 'a gradient component on or beyond a border is not zero'
        assert (ex['cls'][rows[:2]] != R.INSIDE).all() and (grad[b][rows[:2]] == 0).all(), 'gmin and gmax themselves'
    for nv in (1, 257):
        sub = pts[:, n - nv:n]
        _, _, _, r2 = check_operator('%s V=%d' % (name, nv), sdf, gmin, gmax, sub, sid, ac)
        rec['V=%d' % nv] = {'value_ratio': r2['value_ratio'], 'grad_ratio': r2['grad_ratio']}
    _records[name] = rec
