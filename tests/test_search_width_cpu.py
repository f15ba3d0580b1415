"""The partial sums of the NN search's contact terms for two and four lanes per query (csrc/search_sum_order.h) without a GPU:
tools/search_sum_order_host_check.hip places the terms of every n_c in 1 .. 300 on lanes the way the kernels do, reduces them with the
functions the kernels call, and compares every 64-query slice bit for bit with the 4-lane association written out term by term, under the
host's address and undefined-behaviour sanitizers.  Also: the two kernels go through that header, and the knobs are declared."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    from psi_release_amd import build
    exe = str(tmp_path_factory.mktemp('search_sum_order') / 'search_sum_order_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'search_sum_order_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_slice_equals_the_four_lane_association(host_check):
    """n_c in 1 .. 300, widths 2 and 4, the halving tree (kd_block_fsum) and the pair tree (contact_finish); terms in [0, 1), terms over 40
    binades with -0, +0 and denormals among them, and all -0: every slice below cdiv(n_c, 64) written exactly once with the reference's bits,
    none beyond (the output array has exactly that many floats).  Exit status 1 at the first failure."""
    rr = subprocess.run([host_check], capture_output=True, text=True)
    print(rr.stdout.strip())
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'equal the 4-lane association bit for bit at 2 and 4 lanes per query, each written exactly once' in rr.stdout
    assert 'runtime error' not in rr.stderr and 'AddressSanitizer' not in rr.stderr


def test_the_kernels_go_through_the_header_and_the_knobs_are_declared():
    csrc = os.path.join(ROOT, 'psi-release_amd', 'csrc')
    dev = open(os.path.join(csrc, 'nnindex_device.h')).read()
    fsum = dev.split('void kd_block_fsum(')[1].split('\n}\n')[0]
    for f in ('psi_sum_part_lanes(LPQ)', 'psi_sum_first_lane(LPQ, p)', 'psi_sum_slot(LPQ, ', 'psi_sum_parts(LPQ)'):
        assert f in fsum, f
    assert 'kd_qpb(int lpq) { return psi_sum_slice_queries(lpq); }' in dev       # the slice does not depend on the width
    fit = open(os.path.join(csrc, 'fit.hip')).read()
    finish = fit.split('void contact_finish(')[1].split('\n    }\n')[0]
    for f in ('psi_contact_part_sums<LPQ>', 'psi_sum_slot(LPQ, ', 'psi_sum_parts(LPQ)'):
        assert f in finish, f
    assert 'psi_sum_last_lane(LPQ, p)' in fit.split('void psi_contact_part_sums(')[1].split('\n}\n')[0]
    assert 'num("PSI_FIT_SEARCH_LANES")' in fit.split('static FitKnobs fit_read_knobs()')[1].split('return k;')[0]
    assert 'knobs.search_lanes' in fit.split('static FitModes fit_decide(')[1].split('return d;')[0]
    nn = open(os.path.join(csrc, 'nnindex.hip')).read()
    assert nn.count('getenv("PSI_NN_SEARCH_LANES")') == 1 and 'ix->lanes = kd_lanes_from_env();' in nn
    assert 'return psi_cdiv(n, kd_qpb(LPQ_OPS));' in nn.split('int psi_nn_index_fparts(int n)')[1].split('\n')[0]
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'PSI_FIT_SEARCH_LANES' in readme and 'PSI_NN_SEARCH_LANES' in readme
