"""Winding-number sign on the GPU (csrc/mesh_winding.hip, scene_sdf.py): the exact arm against the NumPy fp64 restatement
(tests/mesh_winding_ref.py) within TOL_F, the pruned arm against the exact arm within 2 E + 2 TOL_F with the restatement's counts, the
closed-form dipole far from an open rectangle, ``compute(sign='winding')`` on the closed room and on its three defects (magnitudes bit for
bit those of ``compute()``, signs those of the analytic field where the pseudonormal sign fails), determinism, refusals, and the way from
the entry script to a fit.

TOL_F = 4 x 4.12e-6 = 1.65e-5 (tests/mesh_winding_cases.py has how it was obtained); E(case, beta) = the restatement's
max |f_pruned - f_exact| in fp64.  Every test prints its figures before it asserts."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_winding_cases as C
from psi_release_amd import fitting, hip, ops, scene_io, scene_sdf, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
_MESHES = {}
PSI_EINVAL = -22                         # include/psi_hip.h


def _mesh(name):
    """One MeshSDF per case, shared by the tests (its clusters are cached on the handle)."""
    if name not in _MESHES:
        cs = C.case(name)
        _MESHES[name] = scene_sdf.MeshSDF(cs.verts, cs.faces)
    return _MESHES[name]


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('name', C.SHAPES)
def test_exact_arm_against_restatement(name):
    cs, mesh = C.case(name), _mesh(name)
    ref, counts = cs.ref(0)
    f = mesh.winding(cs.lo, cs.hi, cs.dim, beta=0).cpu().numpy()
    err = float(np.abs(f.astype(np.float64) - ref).max())
    got = ops.mesh_winding_count(mesh.handle, cs.lo, cs.hi, cs.dim, beta=0)
    print('%s: %d triangles, %d nodes: gpu vs restatement %.3g (TOL_F %.3g); counts %s' % (name, mesh.info[0], cs.dim ** 3, err, C.TOL_F, got))
    assert f.dtype == np.float32 and f.shape == (cs.dim,) * 3 and np.isfinite(f).all()
    assert err <= C.TOL_F
    assert got == counts == (cs.dim ** 3 * mesh.info[0], 0)


@pytest.mark.parametrize('name', C.SHAPES)
def test_pruned_arm_against_exact_arm(name):
    cs, mesh = C.case(name), _mesh(name)
    ref0, _ = cs.ref(0)
    ref3, counts = cs.ref(3.0, 16)
    E = float(np.abs(ref3 - ref0).max())
    exact = mesh.winding(cs.lo, cs.hi, cs.dim, beta=0).cpu().numpy().astype(np.float64)
    pruned = mesh.winding(cs.lo, cs.hi, cs.dim, beta=3.0, cluster=16).cpu().numpy().astype(np.float64)
    got = ops.mesh_winding_count(mesh.handle, cs.lo, cs.hi, cs.dim, beta=3.0, cluster=16)
    diff, err = float(np.abs(pruned - exact).max()), float(np.abs(pruned - ref3).max())
    print('%s: |pruned - exact| %.3g (E %.3g, bound %.3g); pruned vs its restatement %.3g; counts %s (restatement %s)'
          % (name, diff, E, 2 * E + 2 * C.TOL_F, err, got, counts))
    assert diff <= 2 * E + 2 * C.TOL_F
    assert err <= C.TOL_F
    assert got == counts


def test_far_bricks_of_open_rectangle_equal_closed_form_dipole():
    cs, mesh = C.case('rectangle_in_16m_box'), _mesh('rectangle_in_16m_box')
    mask, closed = C.rectangle_far_nodes(3.0)
    f = mesh.winding(cs.lo, cs.hi, cs.dim, beta=3.0, cluster=16).cpu().numpy().astype(np.float64)
    err_far, err_all = float(np.abs(f - closed)[mask].max()), float(np.abs(f - cs.ref(3.0, 16)[0]).max())
    got = ops.mesh_winding_count(mesh.handle, cs.lo, cs.hi, cs.dim, beta=3.0, cluster=16)
    print('rectangle: %d far nodes, |f - dipole| %.3g, all nodes vs restatement %.3g (TOL_F %.3g); counts %s' % (mask.sum(), err_far, err_all, C.TOL_F, got))
    assert mask.sum() >= 512 and err_far <= C.TOL_F and err_all <= C.TOL_F
    assert got == cs.ref(3.0, 16)[1]


@pytest.mark.parametrize('name', ('room_s2_d24',) + C.DEFECTS)
def test_winding_sign_of_the_volume(name):
    cs, mesh = C.case(name), _mesh(name)
    an = cs.analytic()
    f64, _ = cs.ref(3.0, 64)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                       # sign='winding' does not warn, open mesh or not
        vol = mesh.compute(cs.lo, cs.hi, cs.dim, sign='winding')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = mesh.compute(cs.lo, cs.hi, cs.dim)
    assert np.array_equal(_bits(vol.abs()), _bits(plain.abs()))              # the magnitudes are the existing kernel's, bit for bit
    vol, plain = vol.cpu().numpy(), plain.cpu().numpy()
    decided = np.abs(f64 - 0.5) > 10 * C.TOL_F
    wrong_w = int(((vol > 0) != (an > 0))[decided].sum())
    wrong_p = int(((plain > 0) != (an > 0)).sum())
    print('%s: excluded %d of %d; wrong signs: winding %d, pseudonormal %d' % (name, (~decided).sum(), an.size, wrong_w, wrong_p))
    assert (~decided).mean() <= 0.005 and (~decided).sum() == 0             # the reference alone excludes none
    assert wrong_w == 0
    assert (vol > 0).any() and (vol < 0).any()
    if name in C.DEFECTS:
        assert wrong_p >= 1                                                  # why the feature exists
    else:
        assert wrong_p == 0 and np.array_equal(vol.view(np.uint32), plain.view(np.uint32))


def test_exterior_free_lone_box():
    v, fc, (centre, half, _) = C.lone_box()
    lo, hi = (centre - half - 0.37).astype(np.float32), (centre + half + 0.37).astype(np.float32)
    mesh = scene_sdf.MeshSDF(v, fc)
    inside = (np.abs(C.R.node_positions(lo, hi, 12).astype(np.float64) - centre) < half).all(-1)
    f = mesh.winding(lo, hi, 12, beta=0).cpu().numpy()
    print('lone box: f inside %.6f .. %.6f, outside %.3g .. %.3g' % (f[inside].min(), f[inside].max(), f[~inside].min(), f[~inside].max()))
    assert np.abs(f[inside] + 1.0).max() <= C.TOL_F and np.abs(f[~inside]).max() <= C.TOL_F
    free = mesh.compute(lo, hi, 12, sign='winding', exterior='free').cpu().numpy()
    plain = mesh.compute(lo, hi, 12).cpu().numpy()
    assert ((free < 0) == inside).all() and np.array_equal(free.view(np.uint32), plain.view(np.uint32))
    solid = mesh.compute(lo, hi, 12, sign='winding', exterior='solid').cpu().numpy()
    assert (solid < 0).all()                                                 # a room's rule on an object: f <= 0 < 0.5 everywhere


def test_determinism_and_refusals():
    cs, mesh = C.case('room_s6_d21'), _mesh('room_s6_d21')
    for kw in (dict(beta=0), dict(beta=3.0, cluster=16)):
        a, b = mesh.winding(cs.lo, cs.hi, cs.dim, **kw), mesh.winding(cs.lo, cs.hi, cs.dim, **kw)
        assert np.array_equal(_bits(a), _bits(b))
    lo, hi = (ops._mesh_sdf_bounds(cs.lo, cs.hi))
    out = torch.empty(8, 8, 8, device=DEV)
    L = hip.lib()
    for beta, cluster in ((-1.0, 16), (float('nan'), 16), (float('inf'), 16), (3.0, 4), (3.0, 257)):
        assert L.psi_mesh_winding_compute(mesh.handle, lo, hi, 8, beta, cluster, hip.ptr(out), hip.stream()) == PSI_EINVAL
    assert L.psi_mesh_winding_compute(mesh.handle, lo, hi, 1, 3.0, 16, hip.ptr(out), hip.stream()) == PSI_EINVAL
    with pytest.raises(hip.PsiHipError):
        mesh.winding(cs.lo, cs.hi, cs.dim, beta=-1.0)
    with pytest.raises(hip.PsiHipError):
        mesh.winding(cs.lo, cs.hi, cs.dim, cluster=4)
    bad_hi = cs.hi.copy()
    bad_hi[1] = cs.lo[1]
    with pytest.raises(hip.PsiHipError, match='gmax > gmin'):
        mesh.winding(cs.lo, bad_hi, cs.dim)
    with pytest.raises(ValueError):
        mesh.compute(cs.lo, cs.hi, cs.dim, sign='normals')
    torch.cuda.synchronize()
    assert mesh.winding(cs.lo, cs.hi, 8).shape == (8, 8, 8)                  # the mesh object is still good


def test_end_to_end_script_and_fit_on_the_sunk_box_room(tmp_path, smplx_data, vposer_sd):
    sys.path.insert(0, UTILS)
    try:
        import utils_scene_sdf as S
    finally:
        sys.path.pop(0)
    paths = S.main([str(tmp_path / 'prox'), '--name', 'roomW', '--synthetic', '--dim', '32', '--sign', 'winding'])
    for written in (paths['scene_verts_path'], paths['scene_sdf_path'] + '.json', paths['scene_sdf_path'] + '_sdf.npy'):
        assert os.path.exists(written), written
    room = synth.make_oriented_room(2)
    sdf, gmin, gmax, dim = scene_io.read_sdf(paths['scene_sdf_path'])
    same = scene_sdf.scene_from_mesh(room.verts, room.faces, dim=32, margin=0.5)
    assert dim == 32 and np.array_equal(sdf.view(np.uint32), same.sdf.view(np.uint32))      # a closed clean room: both signs agree

    sunk = synth.make_open_room(2, drop_ceiling=False, sink=0.15)
    parts = synth.make_scene(0, m=8, D=2).contact_parts
    scene = scene_sdf.scene_from_mesh(sunk.verts, sunk.faces, dim=32, margin=0.5, contact_parts=parts, sign='winding')
    an = sunk.analytic_sdf(C.R.node_positions(scene.grid_min, scene.grid_max, 32).astype(np.float64))
    assert ((scene.sdf > 0) == (an > 0)).all()
    B = 2
    cfg = {'scene': scene, 'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.05, 'num_iter': 3, 'batch_size': B,
           'device': torch.device(DEV), 'contact_part': synth.CONTACT_PARTS, 'verbose': False, 'smplx_data': smplx_data, 'vposer_state': vposer_sd}
    op = fitting.FittingOP(cfg, {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5})
    place = lambda x, y, z: np.array([[0.35, 0, 0, x], [0, 0.35, 0, y], [0, 0, 0.35, z], [0, 0, 0, 1]], np.float32)
    bodies = synth.make_bodies(11, B)
    bodies['cam_ext'] = np.stack([place(0.0, 0.0, 1.7)] * B)
    runner = op.make_step_runner(bodies)
    runner.steps(3)
    losses = runner.last_losses()
    runner.finish()
    print('fused iterations on the sunk-box room (winding sign): losses', losses)
    assert np.isfinite(losses).all() and torch.isfinite(op.xhr_rec).all()
