"""The schedule of fit_bwd_joint_kernel changes no bit: steps in flight per stream wave (blend_bwd_h_body<MTB, PF>, PSI_FIT_BWD_PF=1 is one
step in both row classes) and bodies per skin_bwd_A workgroup per class (csrc/ska_plan.h, PSI_SKA_NBODY=n is n bodies in both).

Neither changes the order in which an output element is summed: a stream wave multiplies its steps w, w + 4, ... in increasing order
however many are in flight, and a column of the 16x16x4 fp32 MFMA is its own sum over k whichever other columns share its tile.  So the
engines compared here must agree BIT FOR BIT in gA, gfeat, g_transl, x, the Adam moments and the loss history after 1, 2 and 12 iterations.

Shapes: the J = 55 model with V = 500, 1100 and 2000, n_c = 64 / 1024, m = 512, D = 16 / 32, B in {1, 3, 17, 33} (16-body tiles per
stream workgroup 1, 1, 2, 4); one case at the production V = 10475, n_c = 2048, B = 2.
The contact class's column slices, steps per wave (stream_plan below restates the rule of csrc/ska_plan.h, psi_stream_split;
tests/test_fit_plan_cpu.py compares the two):
  V = 1100, n_c = 64:      48 steps, 5 slices of 10 (last 8)           -> 3/3/2/2 and 2/2/2/2 per wave
  V = 1100, n_c = 1024:   192 steps, 14 slices of 14 (last 10)         -> 4/4/3/3 and 3/3/2/2
  V = 2000, n_c = 1024:   192 steps, 11 slices of 18 (last 12)         -> 5/5/4/4 and 3/3/3/3
  V = 500, n_c = 64:       48 steps, 10 slices of 5 (last 3)           -> 2/1/1/1 and 1/1/1/0
  V = 10475, n_c = 2048:  384 steps, 6 slices of 64 (the production table) -> 16/16/16/16"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from psi_release_amd import fitting, synth

gpu = pytest.mark.gpu
DEV = 'cuda'
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
KPAD = 512
_cache = {}

# (V, n_c, B) of every engine shape below
SMALL = [(1100, 64, B) for B in (1, 3, 17, 33)]
SHAPES = SMALL + [(1100, 1024, 3), (1100, 1024, 17), (1100, 1024, 33), (2000, 1024, 3), (500, 64, 3), (10475, 2048, 2)]


# ---- the stream plan of a shape, restated from ska_plan.h (psi_stream_split) and lbs.hip (the workspace layout) ----------------------
def stream_plan(V, n_c, B):
    """-> (depth of the contact class, [per-wave step counts of each contact column slice])"""
    cdiv = lambda a, b: -(-a // b)
    Vpad, ncp = cdiv(V, 256) * 256, cdiv(n_c, 256) * 256
    SM, SC = 3 * Vpad // 16, 3 * ncp // 16
    nsn = min(max(256 // (KPAD // 64), 1), SM)
    best, nsn_c = None, 0
    for c in range(1, nsn):
        longest = max(cdiv(SM, nsn - c), cdiv(SC, c))
        if best is None or longest < best:
            best, nsn_c = longest, c
    spc = cdiv(SC, nsn_c)
    waves = []
    for c in range(nsn_c):
        n = max(min((c + 1) * spc, SC) - c * spc, 0)
        waves.append(tuple((n - w + 3) // 4 if n > w else 0 for w in range(4)))
    src = open(os.path.join(ROOT, 'psi-release_amd', 'csrc', 'fit.hip')).read()
    depth = int(re.search(r'#define PSI_FIT_PF_CONTACT (\d+)', src).group(1))        # (the same at every batch size)
    return depth, waves


def test_cases_cover_the_ragged_groups():
    """Among the shapes a contact-class wave owns fewer steps than the shipped depth, exactly as many, one more, and a larger count that
    is no multiple of it — so that a later change of depth cannot silently stop testing the partial last group."""
    seen = set()
    for V, n_c, B in SHAPES:
        depth, waves = stream_plan(V, n_c, B)
        counts = sorted({n for sl in waves for n in sl if n > 0})
        print('V=%d n_c=%d B=%d: depth %d, %d contact slices, steps per wave %s' % (V, n_c, B, depth, len(waves), sorted(set(waves))))
        for n in counts:
            if depth > 1 and n < depth:
                seen.add('fewer')
            if depth > 1 and n == depth:
                seen.add('exactly')
            if depth > 1 and n == depth + 1:
                seen.add('one more')
            if depth > 1 and n > depth and n % depth:
                seen.add('no multiple')
            if depth > 1 and n > depth and n % depth == 0:
                seen.add('multiple')
    assert seen == {'fewer', 'exactly', 'one more', 'no multiple', 'multiple'}, seen


# ---- engines ---------------------------------------------------------------------------------------------------------------------
def model(V):
    if ('smplx', V) not in _cache:
        _cache[('smplx', V)] = synth.make_smplx(7, V=V)
    return _cache[('smplx', V)]


def scene(V, n_c, kind):
    key = ('scene', V, n_c, kind)
    if key not in _cache:
        kw = {'default': dict(D=32), 'nothing': dict(D=16, kind='room', radius=10.0), 'everything': dict(D=16, kind='sphere', radius=50.0),
              'nothing32': dict(D=32, kind='room', radius=10.0)}[kind]
        D = kw.pop('D')
        _cache[key] = synth.make_scene(0, 512, D, n_c, V=V, **kw)
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.uint32)


def run(monkeypatch, V, n_c, B, kind='default', env=(), checkpoints=(1, 2, 12), slots=None, **extra):
    """The engine's state after each of `checkpoints` iterations, as raw bits, of an engine created under the environment `env`
    (pairs); computed once per argument set and left unchanged."""
    key = ('run', V, n_c, B, kind, tuple(env), tuple(checkpoints), slots, tuple(sorted(extra.items())))
    if key in _cache:
        return _cache[key]
    for k in ('PSI_FIT_BWD_PF', 'PSI_SKA_NBODY'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)                             # read once, when the engine is created
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.1, 'num_iter': 1, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': model(V), 'vposer_state': _cache.setdefault('vposer', synth.make_vposer_state(3)), 'engine': 'fused', 'align_corners': True}
    if isinstance(kind, tuple):
        cfg['scenes'] = [scene(V, n_c, k) for k in kind]
    else:
        cfg['scene'] = scene(V, n_c, kind)
    cfg.update(extra)
    torch.manual_seed(0)
    op = fitting.FittingOP(cfg, dict(LOSS))
    if slots is not None:
        op.set_scene_ids(np.asarray(slots, np.int32))
    bodies = synth.make_bodies(21, B)
    bodies['cam_ext'] = synth.make_cam_ext(7, B)
    r = op.make_step_runner(bodies)
    eng, out, done = op._fused, [], 0
    for n in checkpoints:
        r.steps(n - done)
        done = n
        x, hist, step = eng.read(n)
        assert step == n
        out.append({'gA': bits(eng.buffer('gA', (B, 64, 16))), 'gfeat': bits(eng.buffer('gfeat', (B, KPAD))),
                    'g_transl': bits(eng.buffer('g_transl', (B, 3))), 'x': bits(x), 'adam_m': bits(eng.buffer('adam_m', (B, 75))),
                    'adam_v': bits(eng.buffer('adam_v', (B, 75))), 'losses': bits(hist)})
    for k, v in env:
        monkeypatch.delenv(k, raising=False)
    _cache[key] = out
    return out


def assert_same_bits(a, b, what):
    for i, (sa, sb) in enumerate(zip(a, b)):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), '%s: %s differs at checkpoint %d (%d of %d words)' % (what, k, i, int((sa[k] != sb[k]).sum()), sa[k].size)
    assert any(s['gA'].any() for s in a) and any(s['gfeat'].any() for s in a), what + ': the gradients are all zero: broken case'


PF1 = (('PSI_FIT_BWD_PF', '1'),)


# ---- 2. steps in flight -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('V,n_c,B', SMALL + [(1100, 1024, 3), (2000, 1024, 3), (500, 64, 3), (10475, 2048, 2)])
def test_depth_equals_one_step_in_flight(monkeypatch, V, n_c, B):
    """the default room: the model class live in the first iterations and masked later"""
    depth, waves = stream_plan(V, n_c, B)
    print('depth %d, steps per wave of the contact slices %s' % (depth, waves))
    assert_same_bits(run(monkeypatch, V, n_c, B), run(monkeypatch, V, n_c, B, env=PF1), 'V=%d n_c=%d B=%d' % (V, n_c, B))


@gpu
@pytest.mark.parametrize('kind', ['nothing', 'everything'])
def test_depth_in_the_empty_room_and_the_ball(monkeypatch, kind):
    """nothing penetrates (every model step skipped) / everything does (none skipped)"""
    V, n_c, B = 1100, 64, 3
    assert_same_bits(run(monkeypatch, V, n_c, B, kind), run(monkeypatch, V, n_c, B, kind, env=PF1), kind)


# ---- 3. bodies per skin_bwd_A workgroup -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('V,n_c,B', [(1100, 64, 3), (1100, 64, 17), (1100, 64, 33), (1100, 1024, 3), (1100, 1024, 17), (1100, 1024, 33), (10475, 2048, 2)])
def test_bodies_per_workgroup_change_no_bit(monkeypatch, V, n_c, B):
    """the plan's own counts per class, one body per workgroup, eight: a column's sum does not depend on its tile's other columns"""
    ours = run(monkeypatch, V, n_c, B)
    for n in ('1', '8'):
        assert_same_bits(ours, run(monkeypatch, V, n_c, B, env=(('PSI_SKA_NBODY', n),)), 'V=%d n_c=%d B=%d PSI_SKA_NBODY=%s' % (V, n_c, B, n))


# ---- 4. independent bodies, two scenes -----------------------------------------------------------------------------------------------
@gpu
def test_independent_bodies(monkeypatch):
    V, n_c, B = 1100, 64, 3
    assert_same_bits(run(monkeypatch, V, n_c, B, independent_bodies=True), run(monkeypatch, V, n_c, B, env=PF1, independent_bodies=True), 'independent bodies')


@gpu
def test_two_scenes(monkeypatch):
    """psi_fit_create_scenes: the scenes instance of the launch goes through the same plan.  Scene 0 the default room, scene 1 an empty one."""
    V, n_c, B = 1100, 64, 3
    kinds, slots = ('default', 'nothing32'), (1, 0, 1)
    assert_same_bits(run(monkeypatch, V, n_c, B, kinds, slots=slots), run(monkeypatch, V, n_c, B, kinds, env=PF1, slots=slots), 'two scenes')
