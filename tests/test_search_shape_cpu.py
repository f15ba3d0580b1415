"""Two slices per search workgroup (csrc/search_sum_order.h: psi_sum_wg_*) without a GPU: tools/search_sum_order_host_check.hip walks the
two-slice workgroups of the 2-lane search — wave pair r of workgroup bx carries slice 2 bx + r in slots 4 r .. 4 r + 3, the second pair of a
body's last workgroup none when the slice count is odd — for every n_c in 1 .. 300 against the 4-lane association, under the host's address
and undefined-behaviour sanitizers.  tools/search_shape_host_check.hip checks the layout of the walk's stacks and the rule that chooses the shape
(csrc/search_shape.h).  What an engine actually chose is asserted on the GPU (tests/test_search_shape_gpu.py: psi_fit_search_shape)."""
import os
import subprocess

from conftest import ROOT


def test_two_slice_workgroups_equal_the_four_lane_association(tmp_path):
    from psi_release_amd import build
    exe = str(tmp_path / 'search_sum_order_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'search_sum_order_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rr = subprocess.run([exe], capture_output=True, text=True)
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'among them the two-slice workgroups of the 2-lane search' in rr.stdout
    assert 'runtime error' not in rr.stderr and 'AddressSanitizer' not in rr.stderr
    src = open(os.path.join(ROOT, 'tools', 'search_sum_order_host_check.hip')).read()
    for f in ('psi_sum_wg_pair(lpq, spw, ', 'psi_sum_wg_slice(spw, bx, pair)', 'psi_sum_wg_slot(lpq, spw, w, p)'):
        assert f in src, f


def test_stack_layout_bound_and_residency_rule(tmp_path):
    """tools/search_shape_host_check.hip on csrc/search_shape.h: every word of the walk's stack buffer addressed exactly once, the 32-bit
    offset bound, and two slices only where a CU holds as many workgroups as with one (rows <= 37 with the shipped instances)"""
    from psi_release_amd import build
    exe = str(tmp_path / 'search_shape_host_check')
    r = subprocess.run([build.HIPCC, '--offload-arch=' + build.ARCH, '-O2', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'search_shape_host_check.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rr = subprocess.run([exe], capture_output=True, text=True)
    assert rr.returncode == 0, rr.stdout[-2000:] + rr.stderr[-4000:]
    assert 'two slices up to rows = 37' in rr.stdout
    assert 'runtime error' not in rr.stderr and 'AddressSanitizer' not in rr.stderr


def test_the_knob_is_documented():
    assert 'PSI_FIT_SEARCH_SPW' in open(os.path.join(ROOT, 'README.md')).read()
    assert 'psi_fit_search_shape' in open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
