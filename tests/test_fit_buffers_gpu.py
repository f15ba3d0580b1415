"""The fused engine's buffers by name (psi_fit_copy_buffer, include/psi_hip.h) and the reset of the search's warm-start hints.

Every buffer of the engine's blob is declared once (fit.hip: fit_create), with the name psi_fit_copy_buffer exposes it under; a few more
names point into the LBS workspace.  At V = 500, n_c = 64, B = 3, m = 512, D = 16 (Vpad = 512, Npad = 1536, Kpad = 512, ncp = 256), on an
engine with the fused backward and on one created with PSI_FIT_FUSED_BWD=0:
  * every name the header lists copies exactly its documented capacity and refuses one float more;
  * the names of the fused backward's own buffers are unknown on the other engine; an unknown name is refused.
After psi_fit_set_problem on a used engine the hints are all -1 again: a second fit gives the bits of a fresh engine's."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from psi_release_amd import fitting, hip, synth

gpu = pytest.mark.gpu
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
V, N_C, B, M, D = 500, 64, 3, 512, 16
VPAD, NPAD, KPAD, NCP = 512, 1536, 512, 256

# name -> floats, as include/psi_hip.h documents them
ALWAYS = {'verts': B * V * 3, 'pose': B * 165, 'g_pose': B * 165, 'g_rot': B * 55 * 9, 'stats': 8, 'adam_m': B * 75, 'adam_v': B * 75,
          'gA': B * 64 * 16, 'gfeat': B * KPAD, 'g_transl': B * 3, 'gl': B * NPAD, 'g_vp': B * NPAD, 'v_posed': B * NPAD}
FUSED_ONLY = {'glc': B * 3 * NCP, 'gvpc': B * 3 * NCP, 'vpc': B * 3 * NCP, 'spb': B, 'penmask': B * (VPAD // 64) * 2}
_cache = {}


def engine(monkeypatch, fused):
    """(engine, runner) after three iterations; one per kind, created once."""
    if fused in _cache:
        return _cache[fused]
    monkeypatch.delenv('PSI_FIT_FUSED_BWD', raising=False)
    if not fused:
        monkeypatch.setenv('PSI_FIT_FUSED_BWD', '0')             # read once, when the engine is created
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.1, 'num_iter': 1, 'batch_size': B, 'device': torch.device('cuda'),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': _cache.setdefault('smplx', synth.make_smplx(7, V=V)),
           'vposer_state': _cache.setdefault('vposer', synth.make_vposer_state(3)), 'engine': 'fused', 'align_corners': True,
           'scene': _cache.setdefault('scene', synth.make_scene(0, M, D, N_C, V=V))}
    torch.manual_seed(0)
    op = fitting.FittingOP(cfg, dict(LOSS))
    bodies = synth.make_bodies(21, B)
    bodies['cam_ext'] = synth.make_cam_ext(7, B)
    r = op.make_step_runner(bodies)
    r.steps(3)
    monkeypatch.delenv('PSI_FIT_FUSED_BWD', raising=False)
    _cache[fused] = (op._fused, r)
    return _cache[fused]


def copy(eng, name, n):
    """(return code, error text) of a copy of n floats"""
    out = torch.empty(max(n, 1), device='cuda')
    rc = hip.lib().psi_fit_copy_buffer(eng.handle, name.encode(), hip.ptr(out), n, eng.stream.cuda_stream)
    eng.stream.synchronize()
    return rc, (hip.last_error() if rc else '')


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.uint32)


def state(eng, n):
    x, hist, step = eng.read(n)
    assert step == n
    return {'x': bits(x), 'losses': bits(hist), 'adam_m': bits(eng.buffer('adam_m', (B, 75))), 'adam_v': bits(eng.buffer('adam_v', (B, 75))),
            'gA': bits(eng.buffer('gA', (B, 64, 16))), 'gfeat': bits(eng.buffer('gfeat', (B, KPAD)))}


def test_the_header_lists_every_name():
    text = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    doc = text.split('Test/diagnostic copy of an engine-owned device buffer by name')[1].split('int psi_fit_copy_buffer(')[0]
    for name in list(ALWAYS) + list(FUSED_ONLY):
        assert '"%s"' % name in doc, name


@gpu
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
def test_names_and_capacities(monkeypatch, fused):
    eng, _ = engine(monkeypatch, fused)
    names = dict(ALWAYS, **(FUSED_ONLY if fused else {}))
    for name, cap in names.items():
        rc, msg = copy(eng, name, cap)
        assert rc == 0, (name, cap, msg)
        rc, msg = copy(eng, name, cap + 1)
        assert rc != 0 and 'buffer is smaller than requested' in msg, (name, cap + 1, rc, msg)
    if not fused:
        for name in FUSED_ONLY:
            rc, msg = copy(eng, name, 1)
            assert rc != 0 and 'unknown buffer name' in msg, (name, rc, msg)
    rc, msg = copy(eng, 'no_such_buffer', 1)
    assert rc != 0 and 'unknown buffer name' in msg, (rc, msg)
    # a name is a whole name: neither a prefix nor an extension of one
    for name in ('g', 'g_posee', ''):
        rc, msg = copy(eng, name, 1)
        assert rc != 0 and 'unknown buffer name' in msg, (name, rc, msg)


@gpu
def test_set_problem_resets_the_hints(monkeypatch):
    """The engine of the test above has run three iterations (its hints hold the neighbours of the third); restarted — psi_fit_set_problem
    with the same problem and a fresh optimiser — three iterations give bit for bit what the fresh engine gave."""
    eng, r = engine(monkeypatch, True)
    if 'fresh' not in _cache:
        _cache['fresh'] = state(eng, 3)
    r.restart()
    r.steps(3)
    again = state(eng, 3)
    for k, v in _cache['fresh'].items():
        assert np.array_equal(v, again[k]), k
