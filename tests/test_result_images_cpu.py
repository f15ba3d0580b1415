"""Result images without a GPU: the NumPy restatement of their contract (tests/compose_ref.py) against an independent fp64 ray caster, the
statements of csrc/raster_bodies.hip run serially on the host (tools/result_images_host_check.hip) against the restatement, the PNG
writer, the capsule stand-in, the vertex -> faces lists, the entry script's arguments and the C ABI."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import compose_ref as C
import raster_ref as R
from conftest import ROOT

UTILS = os.path.join(ROOT, 'psi-release_amd', 'utils')
SYMBOLS = ['psi_raster_bodies_create', 'psi_raster_bodies_destroy', 'psi_raster_bodies_normals', 'psi_raster_bodies_workspace_bytes',
           'psi_raster_bodies_render']


def decode_png(path):
    """An 8-bit RGB PNG with filter 0 on every row, decoded by hand: [H,W,3] uint8."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    W, H, bits, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (bits, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b''.join(b for t, b in chunks if t == b'IDAT')), np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


def test_symbols_declared_exported_and_uncontracted():
    import re
    from psi_release_amd import build, hip
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'psi_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(psi_[a-z0-9_]+)\s*\(', txt))
    build.build()
    L = hip.lib()
    for s in SYMBOLS:
        assert s in declared and s in hip.SIGNATURES and hasattr(L, s), s
    assert build.PER_FILE['raster_bodies.hip'] == ['-ffp-contract=off']
    # a host function: the piece records of a pass dominate (2 slots of 48 + 4 bytes per draw and face), the views add the key image
    one, four = L.psi_raster_bodies_workspace_bytes(1000, 1, 2, 64, 48), L.psi_raster_bodies_workspace_bytes(1000, 4, 2, 64, 48)
    assert four - one >= 3 * 2 * 1000 * 52 and one >= 2 * 1000 * 52 + 2 * 64 * 48 * 8
    assert L.psi_raster_bodies_workspace_bytes(0, 1, 1, 64, 48) == 0 and L.psi_raster_bodies_workspace_bytes(10, 0, 1, 64, 48) == 0
    assert L.psi_raster_bodies_workspace_bytes(1 << 27, 8, 1, 64, 48) == 0              # draws_per_pass * F = 2^30


def test_workspace_bytes_region_by_region():
    """psi_raster_bodies_workspace_bytes is the sum of its regions, each rounded up to 256 bytes: the binning's regions as for the snapshots
    (tests/test_render_cpu.py) with the piece slots of one pass of dpp = min(draws_per_pass, 65535) draws, and the call's own: the pass's
    pair counts per view, the bad-draw word, the 64-bit key image.  ``pick_draws_per_pass`` is built on differences of these values.
    Zero for arguments the call refuses."""
    from psi_release_amd import build, hip
    build.build()
    L = hip.lib()
    r = lambda x: (x + 255) & ~255
    for F in (1, 300, 20908):
        for draws in (1, 2, 24, 65535, 65536, 100000):
            dpp = min(draws, 65535)
            for n in (1, 4, 65535):
                for W, H in ((64, 48), (70, 45), (1, 1), (17, 33)):
                    nt = -(-W // 16) * -(-H // 16)
                    want = (r(96 * dpp * F) + r(8 * dpp * F) + 3 * r(4 * n * nt) + 2 * r(8 * n) + r(4) + r(8 * n * W * H)
                            + r(4 * (2 * dpp * F + 64 * n * nt)))
                    if dpp * F >= 2 ** 30:
                        want = 0
                    assert L.psi_raster_bodies_workspace_bytes(F, draws, n, W, H) == want, (F, draws, n, W, H)
    assert L.psi_raster_bodies_workspace_bytes(300, 2, 1, 4096, 4096) == (r(96 * 600) + r(8 * 600) + 3 * r(4 * 65536) + 2 * r(8) + r(4) + r(8 * 4096 * 4096)
                                                                          + r(4 * (1200 + 64 * 65536)))
    for args in ((0, 1, 1, 64, 48), (10, 0, 1, 64, 48), (10, 1, 0, 64, 48), (10, 1, 65536, 64, 48), (10, 1, 1, 0, 48), (10, 1, 1, 64, 0),
                 (10, 1, 1, 4097, 48), (10, 1, 1, 64, 4097), (1 << 27, 8, 1, 64, 48)):
        assert L.psi_raster_bodies_workspace_bytes(*args) == 0, args


def test_result_renderer_refuses_cpu(tmp_path):
    import torch
    from psi_release_amd import hip, ops, rendering
    with pytest.raises(hip.PsiHipError):
        ops.raster_bodies_create(torch.zeros(1, 3, dtype=torch.int32), 3)
    with pytest.raises(hip.PsiHipError):
        rendering.ResultRenderer(None, np.array([[0, 1, 2]]), device='cpu')
    with pytest.raises(ValueError):
        ops.raster_bodies_workspace_bytes(1 << 27, 16, 1, 64, 48)                        # M * F >= 2^31 cannot even be one pass
    with pytest.raises(ValueError):
        rendering.write_png(str(tmp_path / 'x.png'), np.zeros((4, 4, 3), np.float32))


def test_write_png_round_trip(tmp_path):
    from psi_release_amd import rendering
    rs = np.random.RandomState(0)
    for shape in ((1, 1, 3), (7, 5, 3), (54, 96, 3)):
        img = rs.randint(0, 256, shape).astype(np.uint8)
        fn = str(tmp_path / 'a.png')
        rendering.write_png(fn, img)
        assert np.array_equal(decode_png(fn), img)


def test_capsule_is_closed_and_faces_outwards():
    from psi_release_amd import synth
    v, f = synth.make_capsule_mesh()
    assert v.shape == (178, 3) and f.shape == (352, 3) and v.dtype == np.float32 and f.dtype == np.int32
    assert v[:, 2].min() == 0.0 and abs(v[:, 2].max() - 1.7) < 1e-6 and abs(np.abs(v[:, :2]).max() - 0.16) < 1e-6
    for args in ((), (5, 7, 0.3, 1.1), (4, 3, 0.2, 0.9)):
        v, f = synth.make_capsule_mesh(*args)
        assert sorted(set(f.ravel())) == list(range(len(v)))
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        directed = set(map(tuple, e))
        assert len(directed) == len(e)                                                  # no directed edge twice: consistent winding
        assert all((b, a) in directed for a, b in directed)                             # every edge shared by exactly two faces
        a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
        assert (np.cross(a, b) * c).sum() / 6.0 > 0.5 * np.pi * (args[2] if args else 0.16) ** 2 * ((args[3] if args else 1.7) - 1.0)
        ctr = np.array([0.0, 0.0, v[:, 2].max() / 2])
        assert (((a + b + c) / 3 - ctr) * np.cross(b - a, c - a)).sum(-1).min() > 0     # every face looks away from the axis' centre


def test_restatement_owner_against_fp64_ray_casting():
    """The owner image of tests/compose_ref.py on the fixture at (48, 64) against brute-force fp64 ray casting of the scene and of the
    concatenated bodies (every body is in every view): equal wherever the pixel is edge-stable for both meshes (the +-1/256-pixel rule of
    test_render_cpu.py), the two nearest hits of each ray caster differ by more than 1e-4 relative, and body and scene depth differ by
    more than 1e-4 relative.  The excluded share is held to that file's cap, 1 %."""
    fx = C.fixture()
    size = C.SIZES[0]
    K = C.K_of(size)
    ref = C.fixture_reference(size)
    room = fx['room']
    V = fx['bverts'].shape[1]
    bv = fx['bverts'].reshape(-1, 3)
    bf = np.concatenate([fx['bfaces'].astype(np.int64) + b * V for b in range(len(fx['bverts']))])
    h = 1.0 / 256
    ok = np.ones((4,) + size, bool)
    rays = []
    for verts, faces in ((room.verts, room.faces), (bv, bf)):
        ray = R.raycast_fp64(verts, faces, fx['cams'], K, size)
        with np.errstate(all='ignore'):
            ok &= ~np.isfinite(ray['depth2']) | ((ray['depth2'] - ray['depth']) > 1e-4 * ray['depth'])
        for off in ((-h, -h), (h, -h), (-h, h), (h, h)):
            ok &= R.raycast_fp64(verts, faces, fx['cams'], K, size, offset=off)['tri'] == ray['tri']
        rays.append(ray)
    zs, zb = rays[0]['depth'], rays[1]['depth']
    with np.errstate(all='ignore'):
        ok &= ~(np.isfinite(zs) & np.isfinite(zb)) | (np.abs(zb - zs) > 1e-4 * np.minimum(zb, zs))
    owner = np.where(zb < zs, rays[1]['tri'] // len(fx['bfaces']), -1)                  # the body of the concatenation = draw // 4
    got = np.where(ref['draw'] >= 0, fx['draw_body'][np.maximum(ref['draw'], 0)], -1)
    excluded = 1.0 - ok.mean()
    print('excluded share %.2e; owners differing on compared pixels: %d of %d' % (excluded, ((owner != got) & ok).sum(), ok.size))
    assert excluded <= 0.01
    assert np.array_equal(owner[ok], got[ok])
    assert np.array_equal(ref['scene_hit'][ok], np.isfinite(zs)[ok]) and np.array_equal(ref['body_hit'][ok], np.isfinite(zb)[ok])


def test_fixture_covers_the_cases_that_matter():
    """What the GPU tests rely on: no pixel of the restatement is excluded, and the counts the fixture was chosen for."""
    fx = C.fixture()
    for size in C.SIZES:
        ref = C.fixture_reference(size)
        assert not ref['near_tie'].any() and ref['body_clear'].all()
    counts = C.fixture_reference((48, 64))['counts'].reshape(6, 4, 2)                   # [body, view]
    assert counts[5, 2].tolist() == [3072, 3072]                                       # the body around camera 2 fills its view, all visible
    assert counts[1, 1].tolist() == [268, 268]                                         # a body in the open
    assert counts[2, 0].tolist() == [297, 193] and counts[0, 0].tolist() == [25, 9]    # two partly behind the furniture
    assert counts[2, 3].tolist() == [22, 0]                                            # one wholly hidden (the camera outside sees the walls)
    assert (counts.sum(-1) == 0).sum() >= 3 and (counts[..., 1] <= counts[..., 0]).all()
    assert fx['bverts'].shape == (6, 178, 3) and len(fx['draw_body']) == 24


@pytest.fixture(scope='module')
def host_run(tmp_path_factory):
    """tools/result_images_host_check.hip compiled and run on the fixture at (45, 70)."""
    from psi_release_amd import build
    tmp = tmp_path_factory.mktemp('host_check')
    exe = str(tmp / 'result_images_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-ffp-contract=off',
                        os.path.join(ROOT, 'tools', 'result_images_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    fx, size = C.fixture(), C.SIZES[1]
    H, W = size
    room, K = fx['room'], C.K_of(size)
    B, V, _ = fx['bverts'].shape
    nF, M, n = len(fx['bfaces']), len(fx['draw_body']), len(fx['cams'])
    w2c = R.world_to_camera_rows(fx['cams'])
    intr = np.tile(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32), (n, 1))
    with open(str(tmp / 'in.bin'), 'wb') as f:
        f.write(np.array([len(room.verts), len(room.faces), 1, B, V, nF, M, n, W, H], np.int32).tobytes())
        f.write(np.array((0.05,) + C.BACKGROUND, np.float32).tobytes())
        for a, dt in ((room.verts, np.float32), (room.faces, np.int32), (fx['vrgb'], np.float32), (fx['bverts'], np.float32), (fx['bfaces'], np.int32),
                      (fx['draw_body'], np.int32), (fx['draw_view'], np.int32), (fx['draw_rgb'], np.float32), (w2c, np.float32), (intr, np.float32)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    rr = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True)
    assert rr.returncode == 0, rr.stderr[-2000:]
    raw = open(str(tmp / 'out.bin'), 'rb').read()
    pos, out = 0, {}
    for name, dt, shape in (('rgb', np.uint8, (n, H, W, 3)), ('depth', np.float32, (n, H, W)), ('draw', np.int32, (n, H, W)),
                            ('body_depth', np.float32, (n, H, W)), ('body_id', np.int32, (n, H, W)), ('counts', np.int32, (M, 2)),
                            ('normals', np.float32, (B, V, 3)), ('voff', np.int32, (V + 1,)), ('vface', np.int32, (3 * nF,))):
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[pos:pos + nb], dt).reshape(shape)
        pos += nb
    assert pos == len(raw)
    return out


def test_host_run_of_the_kernels_statements_against_restatement(host_run):
    """The fp32 statements of csrc/raster_bodies.hip, run serially on the CPU, held to the restatement with the GPU tests' rules: hit mask
    and ids exact, depths within 1e-5 relative, colours within one level, counts exact."""
    fx, ref = C.fixture(), C.fixture_reference(C.SIZES[1])
    nF = len(fx['bfaces'])
    excluded, _, _, _ = C.check_images(host_run, ref, nF)
    assert excluded == 0.0
    assert np.array_equal(host_run['counts'], ref['counts'])
    # the counts again from the images and the restatement's scene depth (no pixel's body and scene depths are within 1e-4)
    assert np.array_equal(C.counts_from_images(host_run['body_id'], host_run['body_depth'], ref['scene_depth'], ref['scene_hit'], 24, nF),
                          host_run['counts'])
    assert len(np.unique(host_run['rgb'].reshape(-1, 3), axis=0)) > 200               # shaded, coloured images, not flat ids


def test_vertex_face_lists_and_normals_of_the_host_run(host_run):
    """The CSR lists every vertex's faces in ascending index, and the fp32 normals summed in that order meet the fp64 sums within
    1e-5 x sum |cross_i| per component (under ten fp32 additions of already-rounded products, about 1e-6 relative, tenfold margin)."""
    fx = C.fixture()
    off, lst = C.csr_of_faces(fx['bfaces'], 178)
    assert np.array_equal(host_run['voff'], off) and np.array_equal(host_run['vface'], lst)
    for v in range(178):
        seg = lst[off[v]:off[v + 1]]
        assert (np.diff(seg) > 0).all() and all(v in fx['bfaces'][i] for i in seg)
    n64, a64 = C.vertex_normal_sums(fx['bverts'], fx['bfaces'])
    err = np.abs(host_run['normals'] - n64)
    print('normals: max error / bound %.3f' % (err / (1e-5 * a64)).max())
    assert (err <= 1e-5 * a64).all()


def test_script_arguments():
    sys.path.insert(0, UTILS)
    try:
        import utils_show_test_results as S
    finally:
        sys.path.remove(UTILS)
    a = S.parse_args(['gen', 'scene.ply', 'out'])
    assert (a.gen_folder, a.scene_ply, a.out_dir) == ('gen', 'scene.ply', 'out') and a.size == [540, 960] and not a.no_flip and not a.together
    assert a.fixed_cam is None and a.synthetic is None and a.pack >= 1
    nums = [str(float(i)) for i in range(16)]
    a = S.parse_args(['gen', 'scene.ply', 'out', '--size', '54', '96', '--fixed_cam'] + nums + ['--together', '--no_flip', '--pack', '7',
                                                                                                 '--synthetic', 'syn'])
    assert a.size == [54, 96] and a.together and a.no_flip and a.pack == 7 and a.synthetic == 'syn'
    assert np.array_equal(S.fixed_camera(a.fixed_cam), np.arange(16.0).reshape(4, 4))
    with pytest.raises(SystemExit):
        S.parse_args(['gen', 'scene.ply', 'out', '--fixed_cam', '1', '2', '3'])
    with pytest.raises(SystemExit):
        S.parse_args(['gen', 'scene.ply', 'out', '--together'])                          # one image of all bodies needs the fixed camera
    T = S.habitat_flip()
    assert np.array_equal(T, np.diag([1.0, -1.0, -1.0, 1.0]))
    ext = np.arange(16.0).reshape(4, 4)
    assert np.array_equal(S.camera_pose(ext, no_flip=False), ext @ T) and np.array_equal(S.camera_pose(ext, no_flip=True), ext)
