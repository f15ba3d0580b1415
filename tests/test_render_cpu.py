"""CPU checks of the snapshot renderer's host side: the C ABI, the PLY mesh reader / writer, the virtual-camera sampler, the sensor-folder
format, and the NumPy restatement of the rasteriser (tests/raster_ref.py) against an independent fp64 ray caster."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import raster_ref as R
from conftest import ROOT

RASTER_SYMBOLS = ['psi_raster_mesh_create', 'psi_raster_mesh_destroy', 'psi_raster_render', 'psi_raster_workspace_bytes']


def test_raster_symbols_declared_and_exported():
    from psi_release_amd import build, hip
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'psi_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(psi_[a-z0-9_]+)\s*\(', txt))
    build.build()
    for path in (build.LIB, build.LIB_FMA):
        lib = ctypes.CDLL(path)
        for s in RASTER_SYMBOLS:
            assert s in declared and s in hip.SIGNATURES, s
            assert hasattr(lib, s), '%s does not export %s' % (os.path.basename(path), s)
    # a host function, like the other workspace queries: piece records dominate (2 slots of 48 bytes per view and triangle)
    L = hip.lib()
    assert L.psi_raster_workspace_bytes(0, 1, 64, 48) == 0
    small, big = L.psi_raster_workspace_bytes(1000, 1, 64, 48), L.psi_raster_workspace_bytes(1000, 4, 64, 48)
    assert small >= 2 * 1000 * 48 and 3 * small < big <= 4 * small


def test_workspace_bytes_region_by_region():
    """psi_raster_workspace_bytes is the sum of its regions, each rounded up to 256 bytes: two piece slots per (view, triangle) of a 48-byte
    record and a 4-byte tile box, three ints per (view, tile) (count, cursor, offset), a 64-bit bin base per view, and 4-byte bin entries
    for every slot plus 64 per tile.  Zero for arguments the call refuses."""
    from psi_release_amd import build, hip
    build.build()
    L = hip.lib()
    r = lambda x: (x + 255) & ~255
    for nf in (1, 7, 1000, 123457):
        for n in (1, 3, 65535):
            for W, H in ((64, 48), (70, 45), (1, 1), (17, 33), (4096, 4096)):
                nt = -(-W // 16) * -(-H // 16)
                want = r(96 * n * nf) + r(8 * n * nf) + 3 * r(4 * n * nt) + r(8 * n) + r(4 * n * (2 * nf + 64 * nt))
                assert L.psi_raster_workspace_bytes(nf, n, W, H) == want, (nf, n, W, H)
    for args in ((0, 1, 64, 48), (10, 0, 64, 48), (10, 1, 0, 48), (10, 1, 64, 0), (-1, 1, 64, 48)):
        assert L.psi_raster_workspace_bytes(*args) == 0, args


def test_render_refuses_cpu_tensors():
    import torch
    from psi_release_amd import hip, ops, rendering
    with pytest.raises(hip.PsiHipError):
        ops.raster_mesh_create(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(hip.PsiHipError):
        ops.raster_render(None, 1, torch.zeros(1, 3, 4), torch.zeros(1, 4), (4, 4))
    with pytest.raises(hip.PsiHipError):
        rendering.SceneMesh(np.zeros((3, 3)), np.array([[0, 1, 2]]), device='cpu')


@pytest.mark.parametrize('ascii_', [False, True])
@pytest.mark.parametrize('colours', [False, True])
def test_ply_mesh_round_trip(tmp_path, ascii_, colours):
    from psi_release_amd import scene_io, synth
    room = synth.make_room_mesh(3, 20)
    rgb = room.rgb() if colours else None
    fn = str(tmp_path / 'm.ply')
    scene_io.write_ply_mesh(fn, room.verts, room.faces, rgb, ascii=ascii_)
    v, f, c = scene_io.read_ply_mesh(fn)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v, room.verts) and np.array_equal(f, room.faces)
    if colours:
        assert c.dtype == np.uint8 and np.array_equal(c, rgb)
        assert np.array_equal(scene_io.labels_from_colors(c), room.labels)           # grey = 5 * label maps back exactly
    else:
        assert c is None
    assert np.array_equal(scene_io.read_ply_vertices(fn), room.verts)                # the older vertex reader reads the same file


def test_labels_from_colours():
    from psi_release_amd import scene_io
    rgb = np.array([[0, 0, 0], [5, 5, 5], [10, 20, 30], [205, 205, 205], [255, 255, 255], [255, 0, 0], [1, 2, 4]], np.uint8)
    want = np.array([0.0, 1.0, 4.0, 41.0, 41.0, 17.0, 7.0 / 15.0], np.float32)       # 255 -> 51 clamps to 41
    assert np.array_equal(scene_io.labels_from_colors(rgb), want)


def test_sample_virtual_cams():
    from psi_release_amd import rendering, synth
    room = synth.make_room_mesh(0, 0)
    target = np.array([0.2, -0.1, 0.9])
    planes = room.planes()
    poses, shifts = rendering.sample_virtual_cams(room.box_min, room.box_max, target, planes, grid_nodes=12, rng=np.random.RandomState(4),
                                                  return_shifts=True)
    assert poses.shape[1:] == (4, 4) and len(poses) >= 10 and len(shifts) == len(poses)
    for pose, s in zip(poses, shifts):
        Rm, pos = pose[:3, :3], pose[:3, 3]
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
        assert np.array_equal(pose[3], [0, 0, 0, 1])
        to_target = target - (pos - s)                                               # from the lattice node, before the shift
        assert np.abs(Rm[:, 2] - to_target / np.linalg.norm(to_target)).max() < 1e-12
        assert abs(Rm[2, 0]) < 1e-15 and Rm[2, 1] < 0                                # x horizontal, y down (world z is up)
        d = np.linalg.norm(pos - target)
        assert 1.65 < d < 6.5
        assert (((pos[None] - planes[:, 0]) * planes[:, 1]).sum(-1) >= 0).all()
    again = rendering.sample_virtual_cams(room.box_min, room.box_max, target, planes, grid_nodes=12, rng=np.random.RandomState(4))
    assert np.array_equal(again, poses)
    other = rendering.sample_virtual_cams(room.box_min, room.box_max, target, planes, grid_nodes=12, rng=np.random.RandomState(5))
    assert other.shape != poses.shape or not np.array_equal(other, poses)
    # without the planes the distance filter alone decides, and the lattice is the reference's: (n - 2)^2 * (n // 3 - 2) nodes at most
    free = rendering.sample_virtual_cams(room.box_min, room.box_max, target, None, grid_nodes=12, noise=0.0)
    assert 0 < len(free) <= 10 * 10 * 2 and np.array_equal(free[:, 3, :3], np.zeros((len(free), 3)))
    np.random.seed(1)
    state = np.random.get_state()[1].copy()
    rendering.sample_virtual_cams(room.box_min, room.box_max, target, planes)
    assert np.array_equal(np.random.get_state()[1], state)                           # the global generator is left alone


def test_view_is_usable():
    from psi_release_amd import rendering
    K = R.intrinsics(50.0, 50.0, 32.0, 24.0)
    far = np.full((48, 64), 4.0, np.float32)
    assert rendering.view_is_usable(far, [0.0, 0.0, 2.0], K)
    assert not rendering.view_is_usable(far, [0.0, 0.0, 4.5], K)                     # the wall is in front of the target
    assert not rendering.view_is_usable(far, [1.2, 0.0, 2.0], K)                     # projects at x = 62 > 64 - 10
    assert not rendering.view_is_usable(far, [0.0, 0.0, -1.0], K)
    near = far.copy()
    near[14:34, 22:42] = 1.0                                                         # the 20 x 20 window around (32, 24) is occluded
    assert not rendering.view_is_usable(near, [0.0, 0.0, 2.0], K)


def test_sensor_folder_is_what_test_habitat_loads(tmp_path):
    from psi_release_amd import rendering, synth
    rs = np.random.RandomState(0)
    depth, seg = rs.uniform(0, 5, (3, 6, 8)).astype(np.float32), rs.uniform(0, 41, (3, 6, 8)).astype(np.float32)
    ext, K = synth.make_room_cams('inside'), R.intrinsics(50.0, 50.0, 4.0, 3.0)
    folder = str(tmp_path / 'sensor')
    rendering.write_sensor_folder(folder, depth, seg, ext, K)
    files = sorted(glob.glob(folder + '/cam_*'))                                     # the loading lines of TestOP.test_habitat
    assert len(files) == 3
    for i, cam_file in enumerate(files):
        cam_params = np.load(cam_file, allow_pickle=True, encoding='latin1').item()
        assert np.array_equal(cam_params['cam_ext'], ext[i].astype(np.float32)) and np.array_equal(cam_params['cam_int'], K.astype(np.float32))
        assert np.array_equal(np.load(cam_file.replace('cam', 'depth')), depth[i])
        assert np.array_equal(np.load(cam_file.replace('cam', 'seg')), seg[i])
    with pytest.raises(ValueError):
        rendering.write_sensor_folder(str(tmp_path / 'cam_out'), depth, seg, ext, K)


def test_restatement_against_fp64_ray_casting():
    """The fp32 setup + exact integer coverage of tests/raster_ref.py against a brute-force fp64 ray / triangle intersection on
    make_room_mesh(0, 180), three cameras inside the room, 64 x 48: the triangle ids agree wherever the two nearest hits of the ray
    caster differ by more than 1e-4 relative, and the excluded pixels are at most 1 %.

    One more kind of pixel has to be excluded, from the number format alone: snapping to 1/256 pixel moves a vertex by up to 1/512 pixel
    per axis, hence an edge by up to sqrt(2)/512 pixel, so a pixel centre that close to a silhouette edge may fall on the other side of
    it (measured here: 3 of 9216 pixels, each with the sample within that distance of an edge, and none excluded by the depth rule).  A
    pixel counts as edge-stable when the four rays at (+-1/256, +-1/256) pixel around its centre hit the same triangle as the centre
    ray: a line within 1/256 > sqrt(2)/512 of the centre separates those four points.  Measured: 39 of 9216 pixels (0.42 %) are not;
    both exclusions together stay under the 1 % bound."""
    from psi_release_amd import synth
    room = synth.make_room_mesh(0, 180)
    ext, K, size = synth.make_room_cams('inside'), R.intrinsics(50.0, 50.0, 32.0, 24.0), (48, 64)
    ref = R.render_views(room.verts, room.faces, room.labels, ext, K, size)
    ray = R.raycast_fp64(room.verts, room.faces, ext, K, size)
    assert ref['hit'].all() and (ray['tri'] >= 0).all()                              # a closed room: every pixel sees a surface
    clear = (ray['depth2'] - ray['depth']) > 1e-4 * ray['depth']
    stable = np.ones_like(clear)
    h = 1.0 / 256
    for off in ((-h, -h), (h, -h), (-h, h), (h, h)):
        stable &= R.raycast_fp64(room.verts, room.faces, ext, K, size, offset=off)['tri'] == ray['tri']
    excluded = 1.0 - (clear & stable).mean()
    differ = (ref['tri'] != ray['tri']) & clear & stable
    print('excluded share %.2e (depth rule alone %.2e), largest snapped coordinate %.3g, ids differing on compared pixels %d of %d'
          % (excluded, 1.0 - clear.mean(), ref['max_coord'], differ.sum(), clear.size))
    assert excluded <= 0.01
    assert ref['max_coord'] < 2 ** 28 and (ref['dropped'] == 0).all()
    assert not differ.any()
    assert ((ref['tri'] != ray['tri']) & clear).mean() <= 0.001                      # and the edge pixels that do flip are few
    agree = ref['tri'] == ray['tri']
    # depth: 1/512 pixel of snapping times the depth slope of the surface, which has no bound on a grazing triangle: the typical pixel
    rel = np.abs(ref['depth'][agree] / ray['depth'][agree] - 1.0)
    print('depth restatement vs ray caster: median %.2e, max %.2e' % (np.median(rel), rel.max()))
    assert np.median(rel) < 1e-4
