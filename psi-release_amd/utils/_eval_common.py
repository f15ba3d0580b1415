"""Shared bits of the evaluation entry points (path setup, scene lists, synthetic stand-in trees, pkl reading)."""
import os
import pickle
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
for _p in (_ROOT, os.path.join(os.path.dirname(_HERE), 'source')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HABITAT_ROOMS = ['17DRP5sb8fy-bedroom', '17DRP5sb8fy-familyroomlounge', '17DRP5sb8fy-livingroom', 'sKLMLpTHeUy-familyname_0_1',
                 'X7HyMhZNoso-livingroom_0_16', 'zsNo4HB9uLZ-bedroom0_0', 'zsNo4HB9uLZ-livingroom0_13']
PROXE_SCENES = ['MPH16', 'MPH1Library', 'N0SittingBooth', 'N3OpenArea']
SYNTHETIC_SCENES = ['roomA', 'roomB']


def synthetic_tree(root, scenes, batch=1, write=True):
    """The PROX-E-shaped synthetic tree of the fitting scripts (source/_common.py): (asset root, gen path, smplx data, vposer state)."""
    import _common
    return _common.synthetic_prox_tree(root, scenes, batch=batch, write=write)


def scene_paths(root, scenename):
    """(ply, sdf prefix) of a scene under an MP3D-R root (utils_eval_collision_habitat.py:201-202: <root>/<scene>.ply, <root>/sdf/<scene>;
    <root>/mesh/<scene>.ply as the fitting script reads it) or a PROX-E root (scenes_downsampled/, scenes_sdf/)."""
    if os.path.isdir(os.path.join(root, 'scenes_sdf')):
        return os.path.join(root, 'scenes_downsampled', scenename + '.ply'), os.path.join(root, 'scenes_sdf', scenename)
    ply = os.path.join(root, scenename + '.ply')
    if not os.path.exists(ply):
        ply = os.path.join(root, 'mesh', scenename + '.ply')
    return ply, os.path.join(root, 'sdf', scenename)


def body_vectors(gen_path, scenes, max_files):
    """[N,72] body vectors of gen_path/<scene>/body_gen_%06d.pkl, scene after scene (utils_eval_diversity.py:63-89)."""
    import numpy as np
    from psi_release_amd.geometry import BodyParamParser
    rows = []
    for scenename in scenes:
        for ii in range(max_files):
            fn = os.path.join(gen_path, scenename, 'body_gen_{:06d}.pkl'.format(ii))
            if not os.path.exists(fn):
                continue
            with open(fn, 'rb') as f:
                rows.append(np.asarray(BodyParamParser._vector(pickle.load(f)), dtype=np.float32).reshape(-1, 72))
    if not rows:
        raise SystemExit('no body_gen_*.pkl under %s for scenes %s' % (gen_path, scenes))
    return np.concatenate(rows, axis=0)
