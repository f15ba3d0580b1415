"""The BatchNorm kernels (csrc/bnorm.hip through ops.bn_act / ops.bn_act_t) against the plain fp64 reference of tests/bnorm_ref.py, on the loops the
training trunk runs: maps above the 512-block cap of the statistics / reduce grids (their unrolled multi-pass loops, the 16-load round of
sum_partials, the grid-stride loops of both apply kernels), the small and odd ones (M = 1, 2, 3, M < rows per block, C = 8 ... 256), element by element.

Bounds.  u = 2^-24 (fp32 unit roundoff), rpb = 2048 / C rows per block, nblk = min(512, ceil(M / rpb)) blocks, L = ceil(M / (nblk rpb)) + rpb the
longest chain of fp32 additions behind a partial sum (a thread's rows, then the block's row-threads in LDS; the partials are then summed in double).

* statistics: |var - var64| <= 64u (var64 + eps), |mean - mean64| <= 16u sigma + u |mean64|.  The sums of x - x[0][c] and its square behave like those
  of a channel with |mean| ~ sigma: simulated (tools/bnorm_stats_sim.py) worst 1.5e-7 of the variance = 2.5u at any mean / std; 64u leaves 25x to
  that and is 1/20 of what sums of x and x^2 give at mean / std = 64.  u |mean64| is the fp32 rounding of the stored mean.
* invstd = (var + eps)^-1/2 therefore has a relative error <= 32u, + u for its rounding to fp32 (33u, D_XHAT_IS), + u for the product gamma * invstd
  (34u, D_INVSTD).
* output, fp32 maps: the kernel evaluates fma(x, sc, shift) (+ res), sc = gamma invstd, shift = fma(-mean, sc, beta):
  |dy| <= 4u (|x sc| + |mean sc| + |beta| + |res| + |y|) + |sc x| D_INVSTD + |sc| d_mean — at most one rounding of the shift, one of the fma, one of the
  residual add (each <= u of a value bounded by the sum in brackets; 4u leaves one to spare), and the statistics' errors carried through sc and mean.
  bf16 maps: + 2^-8 |y64|, half a unit in the last place of an 8-bit significand (and the fp32 bound times 1 + 2^-8: the rounding applies to the
  kernel's value, not to y64).  ReLU does not increase a difference.
  eval mode: no statistics; sc = gamma / sqrtf(rvar + eps) in fp32 is off by <= 8u (the add: u/2 halved by the root; sqrtf: 1 ulp = 2u; the
  division: 2.5 ulp = 5u), which enters through x sc and through rmean sc: 4u (...) + 8u (|x sc| + |rmean sc|).
* dbeta, dgamma: a sum of n fp32 terms accumulated in a chain of length L is off by <= L u sum|terms| (to first order); forming dz * xhat costs three
  more roundings and the result one: (L + 4) u <= 2 L u since L >= 9.  Hence 2 L u sum|dz| and 2 L u sum|dz xhat|, the latter plus
  sum |dz| |d xhat| with |d xhat| <= d_mean invstd + |xhat| (33u + 2u): the statistics and the two roundings of (x - mean) * invstd.
* dx = a dz + b xhat + c with a = gamma invstd, b = -a dgamma / M, c = -a dbeta / M, term by term: |a dz| (34u + 3u) + |b xhat| 3u + |c| 3u (a product
  and two additions per term) + |d b| |xhat| + |b| |d xhat| + |d c| with |d b| <= |b| 35u + |a| d_dgamma / M, |d c| likewise.  bf16 maps: + 2^-8 |dx64|.
* dresidual = dy * mask: exact.
* running buffers: momentum times the statistics bound (the variance's times M / (M - 1)) + 2u (|(1 - m) old| + |m new|): each of the two terms of
  (1 - m) * old + m * new, evaluated in fp32, carries at most a rounded coefficient or conversion, its product and the final addition (1.5u each).
  With momentum = 1 this is the one fp32 rounding of the stored value.

The ReLU mask of the reference's backward is the kernel's own output > 0 (a wrong mask shows in the output check), so every element is compared.
Measured error / bound ratios: profiles/bnorm_fp64_errors.json (written when PSI_BNORM_ERRORS_JSON names a file).  Every bound is reached to more
than 1e-3 by some case (the worst: y, dx 0.99 — bf16 rounding; running statistics 0.97; dgamma 0.83 and dbeta 0.05 on the small maps, where the
LDS chain dominates L; 2.5e-3 / 1e-3 on the large ones, whose rounding errors average out over 10^5 rows; variance 0.06, mean 0.9), so none was
tightened; the parent of the pivoted sums fails the statistics cases from mean / std = 16 on, the constant channel, and M = 2 at C = 256.
"""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

import bnorm_ref as R
from psi_release_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = R.U

# all but the last: M > 4 * 512 * rpb, M % (512 * rpb) != 0, M % rpb != 0, M even; the last has nblk = 493 (sum_partials: some slices take the 16-load
# round and some do not)
PATH_SHAPES = [(3, 64, 169, 170), (2, 128, 131, 133), (1, 256, 129, 130), (1, 32, 363, 366), (1, 8, 725, 728), (1, 64, 125, 126)]
SMALL_SHAPES = [(2, 8, 1, 1), (1, 8, 1, 3), (2, 256, 1, 1), (1, 64, 5, 7)]
COMBOS = [(False, False), (True, False), (False, True), (True, True)]        # (relu, residual)

_RECORD = {}


def _record(case, **ratios):
    _RECORD.setdefault(case, {}).update({k: (v if isinstance(v, (list, dict, str)) else float('%.4g' % v)) for k, v in ratios.items()})
    path = os.environ.get('PSI_BNORM_ERRORS_JSON')
    if path:
        with open(path, 'w') as fh:
            json.dump(_RECORD, fh, indent=1, sort_keys=True)


def test_path_shapes_are_above_every_grid_cap():
    for N, C, H, W in PATH_SHAPES[:-1]:
        M, rpb = N * H * W, R.rows_per_block(C)
        assert M > 4 * 512 * rpb and M % (512 * rpb) and M % rpb and M % 2 == 0 and M * C // 8 > 2048 * 256
        assert R.stat_blocks(M, C) == 512
    N, C, H, W = PATH_SHAPES[-1]                                  # below the caps: its point is the block count, 480 < 493 < 512
    assert R.stat_blocks(N * H * W, C) == 493 and N * H * W % 2 == 0


def _dt(f32):
    return torch.float32 if f32 else torch.bfloat16


def _dev(t, f32, grad=False):
    """NCHW CPU tensor -> channels_last device map of the element type"""
    t = t.to(_dt(f32)).to(DEV).contiguous(memory_format=torch.channels_last)
    return t.requires_grad_() if grad else t


def _op(f32):
    return ops.bn_act_t if f32 else ops.bn_act


def _bn(C, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        if running_mean is not None:
            bn.running_mean.copy_(running_mean)
            bn.running_var.copy_(running_var)
    return bn.train()


def _f32val(v):
    """the value the kernel receives for a Python float argument (a C float)"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# B.1  exact integers: every partial sum is an integer below 2^24, so a dropped, repeated or mis-strided row changes the result
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _integer_inputs(shape):
    N, C, H, W = shape
    M = N * H * W
    g = torch.Generator().manual_seed(1000 + sum(shape))
    sign = torch.ones(M)
    sign[torch.randperm(M, generator=g)[:M // 2]] = -1.0                     # exactly M / 2 of each sign, shuffled
    idx = (torch.arange(M).view(M, 1) + 37 * torch.arange(C).view(1, C)) % M   # every channel: the same multiset, another order
    flip = torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    x = (2.0 * sign[idx] * flip).view(N, H, W, C).permute(0, 3, 1, 2)
    dy = torch.randint(-7, 8, (N, H, W, C), generator=g).float().permute(0, 3, 1, 2)
    res = torch.randint(-3, 4, (N, H, W, C), generator=g).float().permute(0, 3, 1, 2)
    gamma = 2.0 ** ((torch.arange(C) % 3) - 1).float()                       # 1/2, 1, 2
    beta = ((torch.arange(C) % 5) - 2).float()                               # -2 ... 2
    return x, dy, res, gamma, beta


@pytest.mark.parametrize('with_relu_res', [False, True])
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('shape', PATH_SHAPES)
def test_integer_maps_give_exact_statistics_and_sums(shape, f32, with_relu_res):
    """x = +-2 (M / 2 of each per channel), eps = 0: mean = 0, var = 4, invstd = 1/2, xhat = +-1 exactly — also through the shifted sums (x - x[0][c] is 0
    or +-4).  momentum = 1: the running buffers are the batch statistics.  dy, beta, the residual are small integers, gamma a power of two: y, dbeta,
    dgamma and dresidual are exact, and are compared with ==."""
    N, C, H, W = shape
    M = N * H * W
    x, dy, res, gamma, beta = _integer_inputs(shape)
    bn = _bn(C, gamma, beta, momentum=1.0, eps=0.0)
    xd, dyd = _dev(x, f32, True), _dev(dy, f32)
    rd = _dev(res, f32, True) if with_relu_res else None
    y = _op(f32)(xd, bn, relu=with_relu_res, residual=rd)
    y.backward(dyd)
    assert torch.equal(bn.running_mean.cpu(), torch.zeros(C))
    assert torch.equal(bn.running_var.cpu(), torch.full((C,), 4.0 * M / (M - 1), dtype=torch.float64).float())
    assert int(bn.num_batches_tracked) == 1
    xhat = x.double() / 2
    z = gamma.double().view(1, C, 1, 1) * xhat + beta.double().view(1, C, 1, 1)
    dz = dy.double()
    if with_relu_res:
        z = torch.relu(z + res.double())
        mask = R.f64(y) > 0
        dz = dz * mask
    assert torch.equal(R.f64(y), z)
    assert torch.equal(bn.bias.grad.cpu().double(), dz.sum((0, 2, 3)))
    assert torch.equal(bn.weight.grad.cpu().double(), (dz * xhat).sum((0, 2, 3)))
    if with_relu_res:
        assert torch.equal(rd.grad, _dev(dz, f32))                           # dresidual == dy * mask, bit for bit


# ---------------------------------------------------------------------------------------------------------------------------------
# B.2  fp64 accuracy, element by element
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _random_inputs(shape, f32, mean_over_std=None):
    """Stored operand values (rounded to the map type) as CPU tensors.  mean_over_std None: per-channel mean in [-2, 2], std in [0.5, 2]; a number r:
    x ~ N(+-r std, std^2), the sign alternating over the channels (B.3)."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 17 * f32)
    std = torch.rand(C, generator=g, dtype=torch.float64) * 1.5 + 0.5
    if mean_over_std is None:
        mean = torch.rand(C, generator=g, dtype=torch.float64) * 4 - 2
    else:
        mean = mean_over_std * std * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    dt = _dt(f32)
    x = (torch.randn((N, H, W, C), generator=g, dtype=torch.float64) * std + mean).permute(0, 3, 1, 2).to(dt)
    res = torch.randn((N, H, W, C), generator=g).permute(0, 3, 1, 2).to(dt)
    dy = torch.randn((N, H, W, C), generator=g).permute(0, 3, 1, 2).to(dt)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)      # both signs
    beta = torch.rand(C, generator=g) - 0.5
    gamma[1] = 0.0
    beta[2] = 0.0
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) * 1.5 + 0.5
    return x, res, dy, gamma, beta, rm, rv


def _check_stats_via_running(case, f, bn, rm0, rv0, m):
    bm, bv = R.running_bounds(f, rm0, rv0, m)
    em = (R.f64(bn.running_mean) - f.new_running_mean).abs()
    ev = (R.f64(bn.running_var) - f.new_running_var).abs()
    _record(case, running_mean=R.worst_ratio(em, bm), running_var=R.worst_ratio(ev, bv))
    assert bool((em <= bm).all()), (case, 'running_mean', R.worst_ratio(em, bm))
    assert bool((ev <= bv).all()), (case, 'running_var', R.worst_ratio(ev, bv))


def _run_case(case, shape, f32, relu, with_res, training, inputs, backward=True):
    N, C, H, W = shape
    x, res, dy, gamma, beta, rm0, rv0 = inputs
    bn = _bn(C, gamma, beta, rm0, rv0)
    if not training:
        bn.eval()
    m, eps = _f32val(bn.momentum), _f32val(bn.eps)
    xd = _dev(x, f32, True)
    rd = _dev(res, f32, True) if with_res else None
    y = _op(f32 or not training)(xd, bn, relu=relu, residual=rd)             # (eval mode exists in bn_act_t only, for both map types)
    assert y.dtype == _dt(f32) and y.is_contiguous(memory_format=torch.channels_last)
    f = R.Forward(R.f64(x), R.f64(gamma), R.f64(beta), eps, R.f64(res) if with_res else None, relu, training, R.f64(rm0), R.f64(rv0), m, 0)
    ey, by = (R.f64(y) - f.y).abs(), R.output_bound(f, not f32)
    _record(case, y=R.worst_ratio(ey, by))
    assert bool((ey <= by).all()), (case, 'y', R.worst_ratio(ey, by))
    assert int(bn.num_batches_tracked) == f.new_num_batches_tracked == (1 if training else 0)
    if not training:
        assert torch.equal(bn.running_mean.cpu(), rm0) and torch.equal(bn.running_var.cpu(), rv0)
        return
    _check_stats_via_running(case, f, bn, R.f64(rm0), R.f64(rv0), m)
    if not backward:
        return
    y.backward(_dev(dy, f32))
    f.backward(R.f64(dy), R.f64(y) > 0)
    bg, bb = R.param_grad_bounds(f, C)
    eg, eb = (R.f64(bn.weight.grad) - f.dgamma).abs(), (R.f64(bn.bias.grad) - f.dbeta).abs()
    ex, bx = (R.f64(xd.grad) - f.dx).abs(), R.dx_bound(f, not f32, bg, bb)
    _record(case, dgamma=R.worst_ratio(eg, bg), dbeta=R.worst_ratio(eb, bb), dx=R.worst_ratio(ex, bx))
    assert bool((eg <= bg).all()), (case, 'dgamma', R.worst_ratio(eg, bg))
    assert bool((eb <= bb).all()), (case, 'dbeta', R.worst_ratio(eb, bb))
    assert bool((ex <= bx).all()), (case, 'dx', R.worst_ratio(ex, bx))
    if with_res:
        assert torch.equal(R.f64(rd.grad), f.dz)                             # exact


def _case_id(kind, shape, f32, relu, with_res):
    return '%s %s %s%s%s' % (kind, 'x'.join(map(str, shape)), 'fp32' if f32 else 'bf16', ' relu' if relu else '', ' res' if with_res else '')


_TRAIN_CASES = [(s, t, r, w) for s in PATH_SHAPES + SMALL_SHAPES for t in (False, True) for r, w in COMBOS]
_EVAL_CASES = [(s, t, r, w) for s in PATH_SHAPES + SMALL_SHAPES + [(1, 8, 1, 1)] for t in (False, True) for r, w in COMBOS]      # eval: also M = 1


@pytest.mark.parametrize('shape,f32,relu,with_res', _TRAIN_CASES, ids=[_case_id('train', *c).replace(' ', '-') for c in _TRAIN_CASES])
def test_training_mode_matches_fp64(shape, f32, relu, with_res):
    _run_case(_case_id('train', shape, f32, relu, with_res), shape, f32, relu, with_res, True, _random_inputs(shape, f32))


@pytest.mark.parametrize('shape,f32,relu,with_res', _EVAL_CASES, ids=[_case_id('eval', *c).replace(' ', '-') for c in _EVAL_CASES])
def test_eval_mode_matches_fp64(shape, f32, relu, with_res):
    _run_case(_case_id('eval', shape, f32, relu, with_res), shape, f32, relu, with_res, False, _random_inputs(shape, f32))


# ---------------------------------------------------------------------------------------------------------------------------------
# B.3  statistics of channels whose mean is far above their standard deviation
# ---------------------------------------------------------------------------------------------------------------------------------
STAT_SHAPES = [(3, 64, 169, 170), (1, 256, 129, 130)]


def _stats_of(x, f32):
    """batch mean and biased variance as the kernel formed them, read back through the running buffers (momentum = 1: running_mean = the stored
    mean, running_var = fp32(var M / (M - 1))), and the fp64 ones of the same stored values"""
    N, C, H, W = x.shape
    M = N * H * W
    bn = _bn(C, torch.ones(C), torch.zeros(C), momentum=1.0)
    with torch.no_grad():
        _op(f32)(_dev(x, f32), bn, relu=False)
    mean64, var64 = R.batch_stats(R.f64(x))
    return R.f64(bn.running_mean), R.f64(bn.running_var) * (M - 1) / M, mean64, var64, _f32val(bn.eps)


def _check_stats(case, x, f32):
    mean, var, mean64, var64, eps = _stats_of(x, f32)
    ev, bv = (var - var64).abs(), R.var_bound(var64, eps)
    em, bm = (mean - mean64).abs(), R.mean_bound(mean64, var64)
    _record(case, var=R.worst_ratio(ev, bv), mean=R.worst_ratio(em, bm), var_rel_err=float((ev / (var64 + eps)).max()))
    assert bool((ev <= bv).all()), (case, 'var', R.worst_ratio(ev, bv), float((ev / (var64 + eps)).max()))
    assert bool((em <= bm).all()), (case, 'mean', R.worst_ratio(em, bm))


@pytest.mark.parametrize('shape,f32,r', [(s, True, r) for s in STAT_SHAPES for r in (0, 1, 4, 16, 64, 256, 1024)]
                         + [(s, False, r) for s in STAT_SHAPES for r in (0, 1, 4, 16)])         # bf16 cannot represent the larger ratios
def test_statistics_do_not_depend_on_mean_over_std(shape, f32, r):
    x = _random_inputs(shape, f32, float(r))[0]
    _check_stats('stats %s %s r=%d' % ('x'.join(map(str, shape)), 'fp32' if f32 else 'bf16', r), x, f32)


@pytest.mark.parametrize('shape', STAT_SHAPES)
def test_constant_channel_has_zero_variance(shape):
    """a channel that holds float32(3.3) everywhere: var64 = 0, so the bound asks for |var| <= 64u eps"""
    x = _random_inputs(shape, True)[0].clone()
    x[:, 3] = 3.3
    _check_stats('stats %s fp32 constant channel' % 'x'.join(map(str, shape)), x, True)


@pytest.mark.parametrize('f32', [True, False])
def test_output_at_mean_over_std_64(f32):
    """the normalised output of channels at mean / std = 64 within the output bound of the accuracy test (on bf16 maps the stored values are coarse
    there, 0.25 - 1 apart; the statistics and the bound are those of the stored values)"""
    shape = STAT_SHAPES[0]
    _run_case(_case_id('train r=64', shape, f32, False, False), shape, f32, False, False, True, _random_inputs(shape, f32, 64.0), backward=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# B.4  max-pool on a map with NaN and infinities (the large shape is a case of tests/test_bnorm_gpu.py::test_maxpool3x3s2_equals_torch)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True])
def test_maxpool_with_nan_and_infinities_equals_torch(f32):
    """values and gradient bit for bit against F.max_pool2d; NaN compares as NaN (a NaN in a window is its maximum, the last one in scan order takes
    the gradient)"""
    shape = (2, 16, 9, 11)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g)
    k = torch.rand(shape, generator=g)
    x[k < 0.10] = float('nan')
    x[(k >= 0.10) & (k < 0.18)] = float('inf')
    x[(k >= 0.18) & (k < 0.28)] = float('-inf')
    x[1, :, 4:, 5:] = float('nan')                                            # whole windows of NaN
    xd, xr = _dev(x, f32, True), _dev(x, f32, True)
    y = (ops.maxpool3x3s2_t if f32 else ops.maxpool3x3s2)(xd)
    yr = F.max_pool2d(xr, 3, 2, 1)
    assert y.shape == yr.shape
    assert torch.equal(torch.isnan(y), torch.isnan(yr)) and bool(torch.isnan(y).any()) and bool(torch.isinf(y).any())
    assert torch.equal(torch.nan_to_num(y.float(), nan=7.0), torch.nan_to_num(yr.float(), nan=7.0))      # (+-inf -> +-max: still distinct)
    gy = _dev(torch.randn(yr.shape, generator=g), f32)
    y.backward(gy)
    yr.backward(gy)
    assert torch.equal(xd.grad, xr.grad)
