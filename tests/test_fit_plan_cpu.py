"""Launch plan of fit_bwd_joint_kernel's skin_bwd_A workgroups (csrc/ska_plan.h) without a GPU: tools/fit_plan_host_check.hip walks every
workgroup of every plan through the map the kernel uses, under the host's address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_every_slice_and_body_is_covered_once(tmp_path):
    """Every B in 1 .. 128, n_c in {1, 16, 64, 256, 257, 1024, 2048, 4096}, V in {1100, 10475}, every PSI_SKA_NBODY override 0 .. 8: each
    (class, slice, body) exactly once, at most SKA_NBODY bodies per workgroup, never more workgroups than the single-count rule gave,
    and the production grid (B = 32, V = 10475, n_c = 2048) at most 512.  Exit status 1 at the first failure."""
    from psi_release_amd import build
    exe = str(tmp_path / 'fit_plan_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'fit_plan_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rr = subprocess.run([exe], capture_output=True, text=True)
    print(rr.stdout.strip())
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'covered exactly once' in rr.stdout and 'runtime error' not in rr.stderr
    assert 'grid 485' in rr.stdout           # 41 x 4 + 8 x 8 skin_bwd_A, 256 stream workgroups, statistics


def test_check_and_kernel_share_the_limit_and_the_knob_is_declared():
    """The check's LIMIT is the kernel's SKA_NBODY; the launcher and the kernel both go through ska_plan.h; PSI_FIT_BWD_PF is read with
    the engine's other switches and documented."""
    csrc = os.path.join(ROOT, 'psi-release_amd', 'csrc')
    assert 'constexpr int SKA_NBODY = 8;' in open(os.path.join(csrc, 'lbs_joint_device.h')).read()
    assert 'constexpr int LIMIT = 8;' in open(os.path.join(ROOT, 'tools', 'fit_plan_host_check.hip')).read()
    src = open(os.path.join(csrc, 'fit.hip')).read()
    assert 'psi_ska_plan(' in src.split('static FitPlan fit_plan_make(')[1].split('return p;')[0]
    assert 'psi_ska_map(' in src.split('void fit_bwd_joint_kernel(')[1].split('fit_stats_body(f, stats);')[0]
    assert 'is("PSI_FIT_BWD_PF", \'1\')' in src.split('static FitKnobs fit_read_knobs()')[1].split('return k;')[0]
    assert 'PSI_FIT_BWD_PF' in open(os.path.join(ROOT, 'README.md')).read()
