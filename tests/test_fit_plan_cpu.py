"""Launch plans of fit_bwd_joint_kernel (csrc/ska_plan.h) without a GPU: tools/fit_plan_host_check.hip walks every skin_bwd_A workgroup of
every plan through the map the kernel uses, and every 16-column step of both row classes through the stream workgroups' slices, under
the host's address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('fit_plan') / 'fit_plan_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'fit_plan_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_slice_and_body_is_covered_once(host_check):
    """Every B in 1 .. 128, n_c in {1, 16, 64, 256, 257, 1024, 2048, 4096}, V in {1100, 10475}, every PSI_SKA_NBODY override 0 .. 8: each
    (class, slice, body) exactly once, at most SKA_NBODY bodies per workgroup, never more workgroups than the single-count rule gave,
    and the production grid (B = 32, V = 10475, n_c = 2048) at most 512.  The stream split of the same V and n_c: each step of both
    classes in exactly one slice, the longest slice the brute-force minimum, 6 contact slices of 64 steps at the production shape.
    Exit status 1 at the first failure."""
    rr = subprocess.run([host_check], capture_output=True, text=True)
    print(rr.stdout.strip())
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'covered exactly once' in rr.stdout and 'runtime error' not in rr.stderr
    assert 'grid 485' in rr.stdout           # 41 x 4 + 8 x 8 skin_bwd_A, 256 stream workgroups, statistics
    assert 'every step in exactly one slice, the longest slice minimal' in rr.stdout
    assert '384 contact steps, 6 slices of 64' in rr.stdout      # the line test_bwd_joint_schedule_gpu's docstring quotes


def test_the_schedule_tests_restatement_agrees_with_the_rule(host_check):
    """stream_plan of tests/test_bwd_joint_schedule_gpu.py is an independent restatement of the stream split; for that file's SHAPES it must
    give the contact slices of psi_stream_split (the host check prints them for shapes given as arguments)."""
    from test_bwd_joint_schedule_gpu import SHAPES, stream_plan
    shapes = sorted({(V, n_c) for V, n_c, _ in SHAPES})
    rr = subprocess.run([host_check] + [str(n) for s in shapes for n in s], capture_output=True, text=True)
    assert rr.returncode == 0 and 'runtime error' not in rr.stderr, rr.stdout[-2000:] + rr.stderr[-4000:]
    rule = {}
    for line in rr.stdout.splitlines():
        m = re.match(r'split V (\d+) n_c (\d+): nsn_m (\d+) nsn_c (\d+) spm (\d+) spc (\d+) SM (\d+) SC (\d+)$', line)
        assert m, line
        V, n_c, nsn_m, nsn_c, spm, spc, SM, SC = map(int, m.groups())
        rule[(V, n_c)] = (nsn_c, spc, SC)
    assert sorted(rule) == shapes
    for V, n_c, B in SHAPES:
        nsn_c, spc, SC = rule[(V, n_c)]
        _, waves = stream_plan(V, n_c, B)
        assert len(waves) == nsn_c, (V, n_c, len(waves), nsn_c)
        # a slice's steps, dealt to its four waves in turn
        assert [sum(w) for w in waves] == [max(min((c + 1) * spc, SC) - c * spc, 0) for c in range(nsn_c)], (V, n_c)
        assert all(w == tuple(len(range(k, sum(w), 4)) for k in range(4)) for w in waves), (V, n_c)


def test_check_and_kernel_share_the_limit_and_the_knob_is_declared():
    """The check's LIMIT is the kernel's SKA_NBODY; the launcher, the engine's decisions and the kernel all go through ska_plan.h;
    PSI_FIT_BWD_PF is read with the engine's other switches and documented."""
    csrc = os.path.join(ROOT, 'psi-release_amd', 'csrc')
    assert 'constexpr int SKA_NBODY = 8;' in open(os.path.join(csrc, 'lbs_joint_device.h')).read()
    assert 'constexpr int LIMIT = 8;' in open(os.path.join(ROOT, 'tools', 'fit_plan_host_check.hip')).read()
    src = open(os.path.join(csrc, 'fit.hip')).read()
    assert 'psi_ska_plan(' in src.split('static FitPlan fit_plan_make(')[1].split('return p;')[0]
    assert 'psi_ska_map(' in src.split('void fit_bwd_joint_kernel(')[1].split('fit_stats_body(f, stats);')[0]
    assert 'psi_stream_split(' in src.split('static FitModes fit_decide(')[1].split('return d;')[0]
    assert 'psi_stream_split(' not in src.split('static int fit_create(')[1]        # the rule has one home: no loop left behind
    assert 'is("PSI_FIT_BWD_PF", \'1\')' in src.split('static FitKnobs fit_read_knobs()')[1].split('return k;')[0]
    assert 'PSI_FIT_BWD_PF' in open(os.path.join(ROOT, 'README.md')).read()
