"""The device-blob table of the library's constructors (csrc/blob.h) without a GPU: tools/blob_host_check.hip declares the buffers of every
constructor at the smallest shapes the GPU tests use, and binds them to a malloc'ed base, under the host's address and
undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'psi-release_amd', 'csrc')
# constructor -> (source file, buffers it declares)
CONSTRUCTORS = {
    'psi_lbs_create': ('lbs.hip', 17), 'psi_nn_index_create': ('nnindex.hip', 5), 'psi_mesh_sdf_create': ('mesh_sdf.hip', 4),
    'psi_raster_mesh_create': ('raster.hip', 4), 'psi_raster_bodies_create': ('raster_bodies.hip', 3), 'psi_kmeans_create': ('kmeans.hip', 11),
    'fit_build_scenes': ('fit.hip', 3), 'psi_body_overlap_create': ('body_overlap.hip', 1),
    'psi_surface_crossings_create': ('surface_crossings.hip', 5),
}


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('blob') / 'blob_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'blob_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_constructors_buffers_lie_where_the_rule_puts_them(host_check):
    """Offsets: multiples of 256, ascending in declaration order, `size` their padded sum; an empty buffer shares the next one's offset; a
    reserve beyond the copy is kept; bind writes one pointer per field, inside the blob, no two buffers overlapping; "null when empty"
    fields stay null; names resolve to their buffer and capacity, parts of names and absent names to nothing.  Exit status 1 at the first
    failure; a stray write is a sanitizer report."""
    rr = subprocess.run([host_check], capture_output=True, text=True)
    print(rr.stdout.strip())
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'runtime error' not in rr.stderr and 'AddressSanitizer' not in rr.stderr and 'FAILED' not in rr.stdout
    assert 'all 15 blobs laid out as declared' in rr.stdout
    # without parts the two optional buffers of the crossings handle reserve nothing: three 256-byte-padded buffers of 352 faces
    assert re.search(r'^psi_surface_crossings_create F 352, no parts +5 buffers, +%d bytes' % (2 * 4352 + 1536), rr.stdout, re.M)
    counted = {m.group(1): int(m.group(2)) for m in re.finditer(r'^(\w+)[^\n]*? +(\d+) buffers,', rr.stdout, re.M)}
    for who, (_, n) in CONSTRUCTORS.items():
        assert counted[who] == n, (who, counted)
    # the LBS model at V = 500, J = 55, NB = 20: Kpad 512, Npad 1536 — the two copies of the blend-shape matrix alone are 6 354 944 bytes
    assert re.search(r'^psi_lbs_create V 500 J 55 NB 20 +17 buffers, +(\d+) bytes', rr.stdout, re.M)
    assert re.search(r'^fit_create [^\n]* 5 names$', rr.stdout, re.M)


@pytest.mark.parametrize('who', sorted(CONSTRUCTORS))
def test_a_constructor_declares_each_buffer_once(who):
    """The body of each converted constructor: exactly the declarations the host check replays, one allocation through psi_blob_realise
    with the constructor's own name for the message, and no offset arithmetic, allocation or upload of its own."""
    name, n = CONSTRUCTORS[who]
    src = open(os.path.join(CSRC, name)).read()
    body = src.split('int %s(' % who)[-1].split('\n}\n')[0]
    assert len(re.findall(r'\bT\.(?:upload|copy|zero|ones|raw)\(', body)) == n, who
    entry = 'psi_fit_create_scenes' if who == 'fit_build_scenes' else who
    assert body.count('psi_blob_realise(T, ') == 1 and '"%s")' % entry in body
    for own in ('& ~(size_t)255', 'hipMemcpyHostToDevice', 'hipMemcpyDeviceToDevice', 'hipMemset('):
        assert own not in body, (who, own)
    assert body.count('hipMalloc(') == (1 if who == 'fit_build_scenes' else 0)          # the per-scene volume copies stay separate allocations


def test_the_engine_keeps_its_table_and_the_rule_has_one_home():
    src = open(os.path.join(CSRC, 'fit.hip')).read()
    assert 'struct FitBlob' not in src and 'PsiBlob table;' in src
    assert 'e->table.find(name)' in src.split('int psi_fit_copy_buffer(')[1].split('\n}\n')[0]
    assert 'psi_blob_realise(T, &e->blob, "psi_fit_create")' in src.split('static int fit_create(')[1].split('\n}\n')[0]
    for f in os.listdir(CSRC):                                   # the rasterisers' caller-owned workspaces keep their own layout functions
        if f.endswith('.hip') and f not in ('raster.hip', 'raster_bodies.hip'):
            assert '+ 255) & ~(size_t)255' not in open(os.path.join(CSRC, f)).read(), f
