"""The precondition of the zero-tolerance GPU tests (test_cvae_layers_exact_gpu.py), proved without a GPU for EVERY case of
tests/exact_cases.py: the largest sum of |products| of each result is below 2^24 (so every partial sum, in any order, is a number fp32
holds exactly) and torch's own fp32 evaluation of the case has the bits of the float64 one."""
import pytest
import torch

import exact_cases as E


def _same(a32, a64, what):
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64
    assert torch.equal(a32.double(), a64), what


def test_generators():
    t = E.int_tensor((64, 33), seed=5)
    assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().min()) == 1 and float(t.abs().max()) == 4
    assert bool((t > 0).any()) and bool((t < 0).any())
    assert torch.equal(t, E.int_tensor((64, 33), seed=5)) and not torch.equal(t, E.int_tensor((64, 33), seed=6))
    assert torch.equal(t.to(torch.bfloat16).float(), t)                       # exactly representable in bf16
    w = E.int_weight((64, 33), seed=5)
    assert torch.equal(w, w.round()) and float(w.abs().max()) == 3 and bool((w == 0).any())
    g = E.linear_data((4, 32, 32, 'leaky')).gy
    assert torch.equal(g / 2, (g / 2).round()) and float(g.abs().min()) == 2


def test_tables_cover_what_they_claim():
    assert [c[:5] for c in E.CONV3X3] == list(E.CONV3X3_SPLITS)
    # no square map but the four-row-tile one of the weight gradient: an H / W swap cannot pass
    assert [c for c in E.CONV2D if c[6] == c[7]] == [(33, 64, 64, 3, 1, 1, 32, 32, False)]
    assert all(c in E.CONV2D for c in E.CONV2D_UNPREPARED) and {c[3] for c in E.CONV2D_UNPREPARED} == {1, 3}
    assert len(E.all_conv_cases()) == len(E.CONV3X3) + len(E.CONV2D) - 3      # the S 30 / S 34 / unequal-stage geometries are shared


@pytest.mark.parametrize('case', E.all_conv_cases(), ids=lambda c: '-'.join(map(str, c)))
def test_conv_case_is_exact_in_fp32(case):
    data = E.conv_data(case)
    for t in (data.x, data.dy):
        assert float(t.abs().min()) >= 1                                      # a dropped term always moves the sum
    mags = E.conv_magnitudes(data, case[4], case[5])
    assert max(mags) < E.LIMIT, mags
    r64, r32 = E.conv_ref(case), E.conv_eval(data, case[4], case[5], torch.float32)
    for name in r64._fields:
        a64, a32 = getattr(r64, name), getattr(r32, name)
        assert (a64 is None) == (a32 is None) == (name == 'gb' and not case[8])
        if a64 is not None:
            _same(a32, a64, name)


@pytest.mark.parametrize('case', E.all_linear_cases(), ids=lambda c: '-'.join(map(str, c)))
def test_linear_case_is_exact_in_fp32(case):
    data = E.linear_data(case)
    assert float(data.x.abs().min()) >= 1 and float(data.gy.abs().min()) >= 2
    mags = E.linear_magnitudes(data)
    assert max(mags) < E.LIMIT / 2, mags                                      # half-integers (slope 0.5): exact below 2^23
    r64, r32 = E.linear_ref(case), E.linear_eval(data, torch.float32)
    for name in ('y', 'gx', 'gw', 'gb', 'gres'):
        a64, a32 = getattr(r64, name), getattr(r32, name)
        if a64 is not None:
            _same(a32, a64, name)
    assert r32.ties == r64.ties
    if data.act:
        assert r64.ties >= max(E.MIN_TIES, case[1])                            # the whole first row, at least
    if data.res is not None:
        assert torch.equal(r64.gres, data.gy.double())
