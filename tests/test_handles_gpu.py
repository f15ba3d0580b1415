"""Every owner of a library object, on the GPU at the smallest shape: create (one device blob, csrc/blob.h), one call, ``close()``, and
``close()`` again — the library's destroy symbol runs once, at the first close, and the call's result is the known one.  The fake-library
half, without a GPU: tests/test_body_handles_cpu.py."""
import gc

import numpy as np
import pytest
import torch

from psi_release_amd import body_model, evaluation, fitting, hip, ops, rendering, scene_sdf, synth

pytestmark = pytest.mark.gpu
# two triangles of the unit square in the plane z = 0
VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
FACES = np.array([[0, 1, 2], [1, 3, 2]], np.int32)


def _nn_index():
    pts = np.random.RandomState(0).rand(65, 3).astype(np.float32)
    ix = ops.SceneNNIndex(pts)
    dist, idx = ix.query(torch.tensor(pts[None, 7:9] + np.float32(1e-4), device='cuda'))
    assert idx.cpu().tolist() == [[7, 8]] and float(dist.max()) < 1e-6
    return ix, ix.handle.close


def _scene_set():
    pts = np.random.RandomState(1).rand(2, 65, 3).astype(np.float32)
    st = ops.SceneSet(torch.tensor(pts, device='cuda'))
    _, idx = st.query(torch.tensor(pts[[1, 0], 3:5], device='cuda'), torch.tensor([1, 0], dtype=torch.int32, device='cuda'))
    assert idx.cpu().tolist() == [[3, 4], [3, 4]]
    return st, st.handle.close


def _lbs_model():
    V, J, NB = 5, 2, 1                                           # two joints, the second rotates nothing: the template comes back
    vt = np.random.RandomState(2).rand(V, 3).astype(np.float32)
    w = np.zeros((V, J), np.float32)
    w[:, 0] = 1
    m = body_model.LbsModel(vt, np.zeros((V, 3, NB)), np.zeros(((J - 1) * 9, 3 * V)), np.full((J, V), 1.0 / V), w, np.array([-1, 0]), 'cuda')
    ws = m.workspace(1)
    assert ws.numel() == hip.lib().psi_lbs_workspace_floats(m.handle, 1) > 0
    return m, m.handle.close


def _mesh_sdf():
    m = scene_sdf.MeshSDF(VERTS, FACES.astype(np.int64))
    assert tuple(m.info)[:2] == (2, 0)                           # two triangles kept, none dropped
    return m, m.handle.close


def _scene_mesh():
    m = rendering.SceneMesh(VERTS, FACES.astype(np.int64))
    # one camera at (0.5, 0.5, -2) looking along +z: the centre pixel sees the square at depth 2
    w2c = torch.tensor([[[1, 0, 0, -0.5], [0, 1, 0, -0.5], [0, 0, 1, 2.0]]], device='cuda')
    depth, tri, _, _ = ops.raster_render(m.handle, m.nf, w2c, torch.tensor([[16.0, 16.0, 8.0, 8.0]], device='cuda'), (16, 16))
    assert abs(float(depth[0, 8, 8]) - 2.0) < 1e-6 and int(tri[0, 8, 8]) in (0, 1)
    return m, m.handle.close


def _result_renderer():
    r = rendering.ResultRenderer(None, FACES)
    n = r.normals(torch.tensor(VERTS[None], device='cuda'))
    assert n.cpu().tolist() == [[[0, 0, 1], [0, 0, 2], [0, 0, 2], [0, 0, 1]]]            # each vertex: the sum of its faces' (0, 0, 1)
    return r, r.handle.close


def _kmeans():
    obs = torch.tensor(np.repeat(np.array([[0.0, 0, 0], [4, 4, 4]], np.float32), 32, axis=0), device='cuda')       # N = 64, two points
    km = evaluation.KMeansRestarts(obs, torch.tensor([[[1.0, 1, 1], [3, 3, 3]]], device='cuda'))                 # k = 2, R = 1
    km.iterate(2)
    book = km.read()[0]
    assert book.cpu().tolist() == [[[0, 0, 0], [4, 4, 4]]]
    return km, km.close


def _engine():
    V, n_c, B, M, D = 500, 64, 1, 512, 16
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None, 'init_lr_h': 0.1,
           'num_iter': 1, 'batch_size': B, 'device': torch.device('cuda'), 'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None,
           'verbose': False, 'smplx_data': synth.make_smplx(7, V=V), 'vposer_state': synth.make_vposer_state(3), 'engine': 'fused',
           'align_corners': True, 'scene': synth.make_scene(0, M, D, n_c, V=V)}
    op = fitting.FittingOP(cfg, {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5})
    bodies = synth.make_bodies(21, B)
    bodies['cam_ext'] = synth.make_cam_ext(7, B)
    op.make_step_runner(bodies).steps(1)
    eng = op._fused
    assert eng.read(1)[2] == 1 and bool(torch.isfinite(eng.buffer('adam_m', (B, 75))).all())
    return eng, eng.close


OWNERS = {'SceneNNIndex': (_nn_index, 'psi_nn_index_destroy'), 'SceneSet': (_scene_set, 'psi_nn_index_set_destroy'),
          'LbsModel': (_lbs_model, 'psi_lbs_destroy'), 'MeshSDF': (_mesh_sdf, 'psi_mesh_sdf_destroy'),
          'SceneMesh': (_scene_mesh, 'psi_raster_mesh_destroy'), 'ResultRenderer': (_result_renderer, 'psi_raster_bodies_destroy'),
          'KMeansRestarts': (_kmeans, 'psi_kmeans_destroy'), 'FusedEngine': (_engine, 'psi_fit_destroy')}


@pytest.mark.parametrize('name', sorted(OWNERS))
def test_create_call_close_close(monkeypatch, name):
    make, symbol = OWNERS[name]
    L, freed = hip.lib(), []
    real = getattr(L, symbol)
    monkeypatch.setattr(L, symbol, lambda handle: (freed.append(handle.value), real(handle))[1])
    owner, close = make()
    assert isinstance(owner.handle, hip.Handle) and owner.handle.destroy == symbol
    address = owner.handle.value
    torch.cuda.synchronize()
    assert address and address not in freed
    close()
    assert freed.count(address) == 1 and not owner.handle
    close()
    del owner, close
    gc.collect()
    assert freed.count(address) == 1                             # (the collection may free what earlier tests left: other addresses)
    torch.cuda.synchronize()
    assert hip.lib().psi_last_error() is not None                # the library answers: nothing was freed under it
