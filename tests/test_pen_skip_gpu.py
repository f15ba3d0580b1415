"""The penetration mask of the fused fitting engine (FitDev::penmask) and what fit_bwd_joint_kernel skips with it.

fwd_scene leaves, beside the masked SDF gradient rows gl / g_vp, one bit per (body, vertex): sdf < 0.  A clear bit proves the vertex's
rows zero; fit_bwd_joint_kernel then neither streams the blend-shape columns of a 16-column step nor runs the skinning contraction of a
256-vertex slice whose vertices are clear in all of the workgroup's bodies.  The skipped work adds products with a zero factor to
accumulators that start at +0, so an engine with the skip must equal an engine created under PSI_FIT_PEN_SKIP=0 BIT FOR BIT.

Shapes: a J = 55 model with V = 1100 (5 vertex slices, the last with 76 vertices; 3300 columns = 206 whole 16-column steps and a partial
one), n_c = 64, m = 512, D = 16 / 32; B in {1, 3, 17, 33} (16-body tiles per stream workgroup 1, 1, 2, 4; B = 33 has a ragged last body
group); one case at the production V = 10475, B = 2 for the real slice table."""
import dataclasses

import numpy as np
import pytest
import torch

from psi_release_amd import fitting, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
V_SMALL = 1100
BATCHES = [1, 3, 17, 33]
_cache = {}


def model(V):
    if ('smplx', V) not in _cache:
        _cache[('smplx', V)] = synth.make_smplx(7, V=V)
    return _cache[('smplx', V)]


def base_scene(V, D=16, **kw):
    """make_scene at the test's size (n_c = 64, m = 512); keyword arguments as make_scene's."""
    key = ('scene', V, D, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = synth.make_scene(0, 512, D, 64, V=V, **kw)
    return _cache[key]


def scene_nothing(V):
    """(a) free space everywhere: a spherical room whose radius exceeds the volume's diagonal — also the N = 0 branch"""
    return base_scene(V, 16, kind='room', radius=10.0)


def scene_everything(V):
    """(b) solid everywhere: a ball that swallows the volume"""
    return base_scene(V, 16, kind='sphere', radius=50.0)


def scene_default(V):
    """(d) the default room: dense at iteration 0, sparse later"""
    return base_scene(V, 32)


def scene_ball_at(V, c, D=16, half=0.15):
    """(c) sdf = |p - c| - r on a D^3 grid of half-width `half` around c, r = one grid spacing: a ball that holds the vertex at c and
    hardly any other (the model's vertices are N(0, 0.3) per axis: ~0.1 further vertices per body inside a 2 cm ball)"""
    c = np.asarray(c, np.float32)
    lo, hi = c - np.float32(half), c + np.float32(half)
    ax = [np.linspace(lo[a], hi[a], D, dtype=np.float32) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing='ij')
    r = np.float32(2.0 * half / (D - 1))
    sdf = (np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r).astype(np.float32)
    return dataclasses.replace(scene_nothing(V), sdf=sdf, grid_min=lo.astype(np.float32), grid_max=hi.astype(np.float32), grid_dim=D)


def vposer():
    if 'vposer' not in _cache:
        _cache['vposer'] = synth.make_vposer_state(3)
    return _cache['vposer']


def make_op(V, scenes, B, **extra):
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.1, 'num_iter': 1, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': model(V), 'vposer_state': vposer(), 'engine': 'fused', 'align_corners': True}
    cfg['scenes' if isinstance(scenes, (list, tuple)) else 'scene'] = list(scenes) if isinstance(scenes, (list, tuple)) else scenes
    cfg.update(extra)
    torch.manual_seed(0)
    return fitting.FittingOP(cfg, dict(LOSS))


def bodies_of(B):
    b = synth.make_bodies(21, B)
    b['cam_ext'] = synth.make_cam_ext(7, B)
    return b


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.uint32)


def read_mask(eng, B, V):
    """penmask as bool [B, Vpad]"""
    Vpad = (V + 255) // 256 * 256
    words = bits(eng.buffer('penmask', (B, Vpad // 64 * 2))).view(np.uint64).reshape(B, Vpad // 64)
    return ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(B, Vpad)


def zero_step_share(mask, V):
    """share of the model's 16-column steps whose vertices are clear in ALL bodies (brute force over the 3 Vpad columns)"""
    any_v = mask.any(0)
    cols = np.repeat(any_v, 3)
    return float((~cols.reshape(-1, 16).any(1)).mean())


def run(V, scenes, B, skip, monkeypatch, checkpoints=(1, 2, 12), slots=None, **extra):
    """The engine's state after each of `checkpoints` iterations, as raw bits; the last engine is returned for further reads."""
    if skip:
        monkeypatch.delenv('PSI_FIT_PEN_SKIP', raising=False)
    else:
        monkeypatch.setenv('PSI_FIT_PEN_SKIP', '0')
    op = make_op(V, scenes, B, **extra)
    if slots is not None:
        op.set_scene_ids(slots)
    r = op.make_step_runner(bodies_of(B))
    eng, out, done = op._fused, [], 0
    Kpad = 512
    for n in checkpoints:
        r.steps(n - done)
        done = n
        x, hist, step = eng.read(n)
        assert step == n
        out.append({'gA': bits(eng.buffer('gA', (B, 64, 16))), 'gfeat': bits(eng.buffer('gfeat', (B, Kpad))),
                    'g_transl': bits(eng.buffer('g_transl', (B, 3))), 'x': bits(x), 'adam_m': bits(eng.buffer('adam_m', (B, 75))),
                    'adam_v': bits(eng.buffer('adam_v', (B, 75))), 'losses': bits(hist)})
    return out, eng, op


def assert_same_bits(a, b, what):
    for i, (sa, sb) in enumerate(zip(a, b)):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), '%s: %s differs at checkpoint %d (%d of %d words)' % (what, k, i, int((sa[k] != sb[k]).sum()), sa[k].size)


def check_mask_and_rows(eng, op, scene, B, V, slots=None):
    """assertions 1 and 2: the mask is sdf < 0 of the last forward's vertices; a clear bit means exact zero rows"""
    Vpad = (V + 255) // 256 * 256
    mask = read_mask(eng, B, V)
    verts = eng.buffer('verts', (B, V, 3))
    scs = scene if isinstance(scene, (list, tuple)) else [scene]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    if len(scs) == 1:
        sdf = ops.sdf_sample(verts, t(scs[0].sdf), t(scs[0].grid_min), t(scs[0].grid_max))
    else:
        sdf = ops.sdf_sample(verts, torch.stack([t(s.sdf) for s in scs]), torch.stack([t(s.grid_min) for s in scs]),
                             torch.stack([t(s.grid_max) for s in scs]), scene_id=t(np.asarray(slots, np.int32)))
    sdf = sdf.cpu().numpy()
    print('B=%d: %d of %d vertices penetrate, %d with |sdf| < 1e-6' % (B, int(mask.sum()), B * V, int((np.abs(sdf) < 1e-6).sum())))
    assert not mask[:, V:].any(), 'padding bits set'
    assert np.array_equal(mask[:, :V], sdf < 0)
    Npad = 3 * Vpad
    for name in ('g_vp', 'gl'):
        rows = bits(eng.buffer(name, (B, Npad))).reshape(B, Vpad, 3)
        assert not (rows[~mask] & np.uint32(0x7fffffff)).any(), name + ': a row with a clear mask bit is not zero'
    return mask


# ---- the three global scenes: mask, rows, bit equality ------------------------------------------------------------------------------
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('kind', ['nothing', 'everything', 'default'])
def test_skip_equals_no_skip(monkeypatch, kind, B):
    V = V_SMALL
    scene = {'nothing': scene_nothing, 'everything': scene_everything, 'default': scene_default}[kind](V)
    on, eng, op = run(V, scene, B, True, monkeypatch)
    mask = check_mask_and_rows(eng, op, scene, B, V)
    if kind == 'nothing':
        assert not mask.any()
    if kind == 'everything':
        assert mask[:, :V].all()
    if kind == 'default':                 # (after 12 iterations the room is sparse: the skip arm really skips here)
        assert zero_step_share(mask, V) > 0.5
    # 5. a second run in the same process (same engine, fresh problem): nothing carried in the mask
    r = op.make_step_runner(bodies_of(B))
    r.restart()
    r.steps(12)
    x2, hist2, _ = eng.read(12)
    assert np.array_equal(bits(x2), on[-1]['x']) and np.array_equal(bits(hist2), on[-1]['losses'])
    del eng, op, r
    off, _, _ = run(V, scene, B, False, monkeypatch)
    assert_same_bits(on, off, '%s B=%d' % (kind, B))


# ---- (c) one chosen vertex -------------------------------------------------------------------------------------------------------
def _first_verts(V, B, monkeypatch):
    """posed camera-frame vertices of the first forward (they do not depend on the scene)"""
    if ('verts0', V, B) not in _cache:
        _, eng, _ = run(V, scene_nothing(V), B, True, monkeypatch, checkpoints=(1,))
        _cache[('verts0', V, B)] = eng.buffer('verts', (B, V, 3)).cpu().numpy()
    return _cache[('verts0', V, B)]


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('vstar', [0, 5, 63, 64, 255, 256, V_SMALL - 1])
def test_one_chosen_vertex(monkeypatch, vstar, B):
    """A 2 cm ball around vertex v* of the LAST body: 5 | 63, 64 | 255, 256 | V - 1 straddle two steps | two mask words | two slices | sit in the
    partial slice and the partial last step."""
    V, bstar = V_SMALL, B - 1
    scene = scene_ball_at(V, _first_verts(V, B, monkeypatch)[bstar, vstar])
    on, eng, op = run(V, scene, B, True, monkeypatch, checkpoints=(1,))
    mask = check_mask_and_rows(eng, op, scene, B, V)
    assert mask[bstar, vstar], 'the chosen vertex does not penetrate: broken scene'
    share = zero_step_share(mask, V)
    print('v*=%d B=%d: %d bits set, %.3f of the steps zero in all bodies' % (vstar, B, int(mask.sum()), share))
    assert share >= 0.9, 'the scene is not sparse: broken test'
    del eng, op
    on, _, _ = run(V, scene, B, True, monkeypatch)
    off, _, _ = run(V, scene, B, False, monkeypatch)
    assert_same_bits(on, off, 'v*=%d B=%d' % (vstar, B))


# ---- 4. independent bodies, two scenes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [3, 33])
def test_independent_bodies(monkeypatch, B):
    V = V_SMALL
    scene = scene_default(V)
    on, eng, op = run(V, scene, B, True, monkeypatch, independent_bodies=True)
    check_mask_and_rows(eng, op, scene, B, V)
    del eng, op
    off, _, _ = run(V, scene, B, False, monkeypatch, independent_bodies=True)
    assert_same_bits(on, off, 'independent bodies B=%d' % B)


@pytest.mark.parametrize('B', [3, 17])
def test_two_scenes(monkeypatch, B):
    """psi_fit_create_scenes: the scenes epilogue writes the mask too.  Scene 0 the default room, scene 1 a ball around a vertex of the last body."""
    V = V_SMALL
    c = _first_verts(V, B, monkeypatch)[B - 1, 64]
    scenes = [scene_default(V), scene_ball_at(V, c, D=32, half=0.31)]
    slots = (np.arange(B) + 1) % 2 if B > 1 else [1]
    slots = np.asarray(slots, np.int32)
    slots[B - 1] = 1
    on, eng, op = run(V, scenes, B, True, monkeypatch, slots=slots)
    mask = check_mask_and_rows(eng, op, scenes, B, V, slots)
    del eng, op
    off, _, _ = run(V, scenes, B, False, monkeypatch, slots=slots)
    assert_same_bits(on, off, 'two scenes B=%d' % B)


# ---- the production model's slice table -------------------------------------------------------------------------------------------
def test_production_model(monkeypatch):
    """V = 10475, B = 2, two iterations: 41 vertex slices, the real column slices of the stream workgroups."""
    V, B = 10475, 2
    scene = base_scene(V, 32)
    on, eng, op = run(V, scene, B, True, monkeypatch, checkpoints=(1, 2))
    check_mask_and_rows(eng, op, scene, B, V)
    del eng, op
    off, _, _ = run(V, scene, B, False, monkeypatch, checkpoints=(1, 2))
    assert_same_bits(on, off, 'V=10475')
