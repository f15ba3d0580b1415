"""The kinematic chain of the pose stage as a role of blend_fwd's launch (csrc/chain_plan.h, lbs.hip: blend_fwd_h_kernel<.., LINKS>).

By default the fused engine's head kernel ends at the feature row, and the chain (G, A, A's zero tail rows) runs in workgroups of its own
behind blend_fwd's stream workgroups, one wave per body (two bodies per wave above B = 32), from the R rows and rest joints the head stored.
An engine created under PSI_FIT_CHAIN_IN_HEAD=1 keeps the chain in the head kernel.  The role evaluates the same expressions on the same
fp32 values, so the two engines must agree BIT FOR BIT in everything the pose stage writes and everything behind it.

Shapes: a J = 55 model with V = 500 (the chain depends only on the joint tree; 12 stream workgroups), n_c = 64, m = 512, D = 16.
B in {1, 3, 4, 5, 32, 33, 64}: one live wave; a partly filled workgroup (3, 5: the second workgroup of B = 5 has one live wave); a full
workgroup; the full grid of one body per wave (8 workgroups); two bodies per wave with an odd one out (33: the last live wave has one
body) and full (64); the tail rows behind the last body in each.  B = 65 has two grid rows: off in both arms."""
import dataclasses

import numpy as np
import pytest
import torch

from psi_release_amd import body_model, fitting, synth
from psi_release_amd.vposer import load_vposer

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
V, N_C, M, D = 500, 64, 512, 16
NPAD, KPAD, A_TAIL = 1536, 512, 16
KNOB = 'PSI_FIT_CHAIN_IN_HEAD'
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def model():
    return cached('smplx', lambda: synth.make_smplx(7, V=V))


def vposer():
    return cached('vposer', lambda: synth.make_vposer_state(3))


def scene(seed=0):
    return cached(('scene', seed), lambda: synth.make_scene(seed, M, D, N_C, V=V))


def second_scene():
    """another room's points and volume under the first scene's contact parts (the scenes of one engine list the same contact ids)"""
    o = scene(1)
    return dataclasses.replace(scene(0), verts=o.verts, sdf=o.sdf, grid_min=o.grid_min, grid_max=o.grid_max)


def set_arm(monkeypatch, role):
    """the knob is read once, when the engine is created"""
    if role:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, '1')


def make_op(scenes, B):
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.1, 'num_iter': 1, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': model(), 'vposer_state': vposer(), 'engine': 'fused', 'align_corners': True}
    cfg['scenes' if isinstance(scenes, (list, tuple)) else 'scene'] = list(scenes) if isinstance(scenes, (list, tuple)) else scenes
    torch.manual_seed(0)
    return fitting.FittingOP(cfg, dict(LOSS))


def bodies_of(B):
    b = synth.make_bodies(21, B)
    b['cam_ext'] = synth.make_cam_ext(7, B)
    return b


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.uint32)


def pose_stage(eng, B):
    """what the pose stage and blend_fwd leave in the workspace, as raw bits"""
    out = {'A': bits(eng.buffer('A', (B * 55 + A_TAIL, 12))), 'G': bits(eng.buffer('G', (B, 55, 12))), 'R': bits(eng.buffer('R', (B, 55, 12))),
           'feat': bits(eng.buffer('feat', ((B + 31) // 32 * 32, KPAD))), 'v_posed': bits(eng.buffer('v_posed', (B, NPAD)))}
    assert not out['A'][B * 55:].any(), 'the tail rows behind the last body are not zero'
    return out


def run(scenes, B, role, monkeypatch, want_mode, checkpoints=(1, 2, 12), slots=None):
    """The engine's state after each of `checkpoints` iterations, as raw bits"""
    set_arm(monkeypatch, role)
    op = make_op(scenes, B)
    if slots is not None:
        op.set_scene_ids(slots)
    r = op.make_step_runner(bodies_of(B))
    eng, out, done = op._fused, [], 0
    assert eng.chain_mode() == want_mode, 'psi_fit_chain_mode = %d at B = %d, role arm %s' % (eng.chain_mode(), B, role)
    for n in checkpoints:
        r.steps(n - done)
        done = n
        x, hist, step = eng.read(n)           # (psi_fit_read: a non-zero exchange error word is an error here — hip.check raises)
        assert step == n
        s = pose_stage(eng, B)
        s.update({'gA': bits(eng.buffer('gA', (B, 64, 16))), 'gfeat': bits(eng.buffer('gfeat', (B, KPAD))), 'x': bits(x), 'losses': bits(hist)})
        out.append(s)
    return out


def assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for i, (sa, sb) in enumerate(zip(a, b)):
        assert sorted(sa) == sorted(sb)
        bad = ['%s (%d of %d words)' % (k, int((sa[k] != sb[k]).sum()), sa[k].size) for k in sorted(sa) if not np.array_equal(sa[k], sb[k])]
        assert not bad, '%s: checkpoint %d differs in %s' % (what, i, ', '.join(bad))


# ---- case 1: every path of the role ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 4, 5, 32, 33, 64])
def test_role_equals_chain_in_head(monkeypatch, B):
    on = run(scene(), B, True, monkeypatch, 1)
    off = run(scene(), B, False, monkeypatch, 0)
    assert_same_bits(on, off, 'B=%d' % B)
    # (the chain did run: a body's root transform is its global rotation, not the zeros the workspace starts as)
    assert on[0]['G'].any() and on[0]['A'][:B * 55].any()


# ---- case 2: two grid rows -----------------------------------------------------------------------------------------------------------------
def test_two_grid_rows_keep_the_chain_in_the_head(monkeypatch):
    B = 65
    on = run(scene(), B, True, monkeypatch, 0, checkpoints=(1, 2))
    off = run(scene(), B, False, monkeypatch, 0, checkpoints=(1, 2))
    assert_same_bits(on, off, 'B=65')


# ---- case 3: the other callers of the head / blend pair ------------------------------------------------------------------------------------
def test_several_scenes(monkeypatch):
    B = 4
    scenes = [scene(0), second_scene()]
    slots = np.asarray([0, 1, 1, 0], np.int32)
    on = run(scenes, B, True, monkeypatch, 1, slots=slots)
    off = run(scenes, B, False, monkeypatch, 0, slots=slots)
    assert_same_bits(on, off, 'two scenes')


def test_decode_forward(monkeypatch):
    """psi_fit_decode_forward (the training losses' body decode): head kernel, blend_fwd, plain skinning"""
    B = 5
    # [transl | 6D global rotation | betas | VPoser latent | hand PCA]: small random rows around the identity rotation
    x75 = (0.3 * np.random.RandomState(5).randn(B, 75)).astype(np.float32)
    x75[:, 3:9] += np.asarray([1, 0, 0, 0, 1, 0], np.float32)
    x75 = torch.as_tensor(x75, device=DEV)
    cam = torch.as_tensor(synth.make_cam_ext(7, B), device=DEV)
    got = []
    for role in (True, False):
        set_arm(monkeypatch, role)
        vp, _ = load_vposer(vposer(), vp_model='snapshot')
        vp.to(DEV)
        bm = body_model.create(model(), model_type='smplx', gender='neutral', ext='npz', num_pca_comps=12, batch_size=B, device=DEV)
        dec = fitting.BodyDecoder(vp, bm, B, DEV)
        assert dec.engine.chain_mode() == (1 if role else 0)
        verts = dec(x75, cam)
        torch.cuda.synchronize()              # (the decode runs on the current stream, the reads below on the engine's)
        _, _, step = dec.engine.read(0)       # the exchange error word
        s = pose_stage(dec.engine, B)
        s['verts'] = bits(verts)
        got.append([s])
    assert_same_bits(got[0], got[1], 'decode forward')
    assert np.isfinite(got[0][0]['verts'].view(np.float32)).all() and got[0][0]['G'].any()
