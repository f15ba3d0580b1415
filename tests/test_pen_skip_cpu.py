"""The vertex mask -> 16-column step decision of the blend backward (csrc/pen_steps.h) without a GPU: tools/pen_steps_host_check.hip runs
the functions the kernel calls against a brute-force loop over the columns, under the host's address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_step_mask_equals_brute_force(tmp_path):
    """Every V in 1 .. 700 and V = 10475, random and single-bit masks, every step, through the mask-word window of a stream workgroup's
    slice (a heap copy of exactly those words: a read outside it is a sanitizer error).  Exit status 1 at the first difference."""
    from psi_release_amd import build
    exe = str(tmp_path / 'pen_steps_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'pen_steps_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rr = subprocess.run([exe], capture_output=True, text=True)
    print(rr.stdout.strip())
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'step decisions equal brute force' in rr.stdout and 'runtime error' not in rr.stderr


def test_knob_and_buffer_are_declared():
    """PSI_FIT_PEN_SKIP is read with the engine's other switches and documented; "penmask" is a buffer of psi_fit_copy_buffer: a name in
    the blob's table (declared in fit_create, on engines with the fused backward only), which psi_fit_copy_buffer looks names up in."""
    src = open(os.path.join(ROOT, 'psi-release_amd', 'csrc', 'fit.hip')).read()
    assert 'is("PSI_FIT_PEN_SKIP", \'0\')' in src.split('static FitKnobs fit_read_knobs()')[1].split('return k;')[0]
    create = src.split('static int fit_create(')[1].split('extern "C" int psi_fit_create(')[0]
    assert 'T.zero(f.penmask, ' in create.split('if (mode.fused_bwd) {')[1].split('}')[0] and '"penmask");' in create
    copy = src.split('extern "C" int psi_fit_copy_buffer')[1]
    assert 'e->table.find(name)' in copy                             # the table's own lookup (csrc/blob.h): whole names only
    find = open(os.path.join(ROOT, 'psi-release_amd', 'csrc', 'blob.h')).read().split('const PsiBuf *find(const char *name) const')[1].split('return nullptr;')[0]
    assert 'for (const PsiBuf &b : bufs)' in find and '!strcmp(b.name, name)' in find
    assert 'PSI_FIT_PEN_SKIP' in open(os.path.join(ROOT, 'README.md')).read()
    assert 'penmask' in open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
