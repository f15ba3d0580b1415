"""Where the fused fitting engine runs the kinematic chain of the pose stage (csrc/chain_plan.h), without a GPU:
tools/chain_plan_host_check.hip walks every body of every plan through the functions fit_decide and blend_fwd_h_kernel's links role call,
under the host's address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('chain_plan') / 'chain_plan_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'chain_plan_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_body_is_one_waves_turn(host_check):
    """Every B in 1 .. 130, CU counts 256 / 64 / 32, 246 and 8 stream workgroups, cluster and single-workgroup heads, one grid row and more:
    "on" means every body is exactly one (workgroup, wave, turn), at most 8 links workgroups and at most CUs - stream workgroups of them;
    "off" for gridDim.y > 1 and for C = 1.  Exit status 1 at the first failure."""
    rr = subprocess.run([host_check], capture_output=True, text=True)
    print(rr.stdout.strip())
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'every body covered exactly once' in rr.stdout and 'runtime error' not in rr.stderr
    plans = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r'plan B (\d+): links workgroups (\d+), bodies per wave (\d+)', rr.stdout)}
    # the shapes of tests/test_chain_role_gpu.py on a 256-CU device: one live wave; partly filled workgroups; the full grid of one body per
    # wave; two bodies per wave with an odd one out, and full; off at two grid rows
    assert plans == {1: (1, 1), 3: (1, 1), 4: (1, 1), 5: (2, 1), 32: (8, 1), 33: (5, 2), 64: (8, 2), 65: (0, 0)}


def test_engine_and_kernel_go_through_the_rule_and_the_knob_is_declared():
    """fit_decide takes the plan from chain_plan.h, the kernel its bodies; PSI_FIT_CHAIN_IN_HEAD is read with the engine's other switches
    and documented."""
    csrc = os.path.join(ROOT, 'psi-release_amd', 'csrc')
    src = open(os.path.join(csrc, 'fit.hip')).read()
    assert 'psi_chain_plan(' in src.split('static FitModes fit_decide(')[1].split('return d;')[0]
    assert 'psi_chain_plan(' not in src.split('static int fit_create(')[1]
    assert 'is("PSI_FIT_CHAIN_IN_HEAD", \'1\')' in src.split('static FitKnobs fit_read_knobs()')[1].split('return k;')[0]
    lbs = open(os.path.join(csrc, 'lbs.hip')).read()
    assert 'psi_chain_first_body(' in lbs.split('void blend_fwd_h_kernel(')[1].split('psi_pose_fwd_links(')[0]
    assert 'PSI_FIT_CHAIN_IN_HEAD' in open(os.path.join(ROOT, 'README.md')).read()
