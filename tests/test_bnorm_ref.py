"""tests/bnorm_ref.py (the fp64 reference the GPU tests of csrc/bnorm.hip compare with) against torch's own batch-norm and autograd in float64 on
the CPU: the reference is written out by hand (statistics, running buffers, backward formulas), this is the check that it is the operator."""
import pytest
import torch
import torch.nn.functional as F

import bnorm_ref as R


@pytest.mark.parametrize('shape', [(2, 8, 1, 1), (1, 8, 1, 3), (3, 16, 5, 7)])
@pytest.mark.parametrize('relu,with_res', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('training', [True, False])
def test_reference_equals_torch_float64(shape, relu, with_res, training):
    torch.manual_seed(sum(shape))
    N, C, H, W = shape
    x = (torch.randn(shape, dtype=torch.float64) * 1.3 + 0.4).requires_grad_()
    res = torch.randn(shape, dtype=torch.float64).requires_grad_() if with_res else None
    gamma = (torch.randn(C, dtype=torch.float64)).requires_grad_()
    beta = torch.randn(C, dtype=torch.float64).requires_grad_()
    rm0, rv0 = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5
    dy = torch.randn(shape, dtype=torch.float64)
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, training, 0.1, 1e-5)
    if with_res:
        y = y + res
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    f = R.Forward(x.detach(), gamma.detach(), beta.detach(), 1e-5, res.detach() if with_res else None, relu, training, rm0, rv0, 0.1, 3)
    dx, dres, dgamma, dbeta = f.backward(dy)
    tol = dict(rtol=1e-11, atol=1e-12)
    assert torch.allclose(f.y, y.detach(), **tol)
    assert torch.allclose(f.new_running_mean, rm, **tol) and torch.allclose(f.new_running_var, rv, **tol)
    assert f.new_num_batches_tracked == (4 if training else 3)
    assert torch.allclose(dx, x.grad, **tol) and torch.allclose(dgamma, gamma.grad, **tol) and torch.allclose(dbeta, beta.grad, **tol)
    if with_res:
        assert torch.equal(dres, res.grad)
    else:
        assert dres is None


def test_summation_order_simulation_reproduces_the_recorded_table():
    """tools/bnorm_stats_sim.py (the kernel's summation order in numpy) against the table the shifted sums were decided on — relative variance
    error at mean / std = 0 ... 1024, sums of x and x^2 and sums of x - x[0][c] — to a factor of 2, and the two properties the tests of
    the kernel rest on: the first grows like (mean / std)^2 and is past the 64 * 2^-24 bound of the tests at 64, the second stays 10x below it."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('bnorm_stats_sim', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                   'tools', 'bnorm_stats_sim.py'))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    recorded = {'as_coded': {0: 1e-8, 4: 3e-7, 16: 3.4e-6, 64: 8e-5, 256: 1.5e-3, 1024: 3e-2},
                'shifted': {0: 1.1e-7, 4: 1.4e-7, 16: 9e-8, 64: 7e-8, 256: 3e-8, 1024: 5e-8}}
    t = sim.table()
    for k, row in recorded.items():
        for r, v in row.items():
            assert v / 2 <= t[k][str(r)] <= v * 2, (k, r, t[k][str(r)], v)
    assert t['as_coded']['64'] > 64 * R.U > 10 * max(t['shifted'].values())


def test_launch_geometry_of_the_bounds():
    """rows per block, blocks and chain length as csrc/bnorm.hip launches them (bn_blocks)"""
    assert R.rows_per_block(64) == 32 and R.rows_per_block(8) == 256 and R.rows_per_block(256) == 8
    assert R.stat_blocks(2, 8) == 1 and R.stat_blocks(15750, 64) == 493 and R.stat_blocks(86190, 64) == 512
    assert R.chain_length(86190, 64) == 6 + 32 and R.chain_length(2, 8) == 1 + 256
