"""Exact-integer cases of the CVAE layer kernels (test infrastructure; shared by test_exact_cases_cpu.py and test_cvae_layers_exact_gpu.py).

Operands that are small integers are exactly representable in bf16 (the ``hi`` part of a three-term split is the value, ``lo`` is 0), and
while the sum of |products| of every output stays below 2^24 every partial sum in every order is an integer fp32 holds exactly: the
kernel's fp32 result has ONE correct bit pattern, that of a float64 evaluation, whatever its tiling, split or reduction order.  A test on
such data needs no tolerance, so one dropped pixel, swapped tap, wrong halo column, missed stage or mis-sized tail is a failure.
test_exact_cases_cpu.py proves the precondition (sums < 2^24, fp32 evaluation == fp64 evaluation) for every case below without a GPU.

Layouts: maps [N,C,H,W], weights [Cout,Cin,KH,KW] (logical NCHW / OIHW, as torch has them), all float32 on the CPU."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

LIMIT = 2 ** 24

# ---- ops.conv3x3 (bf16 maps; csrc/conv.hip): (N, Cin, Cout, H, W, bias)
CONV3X3 = [
    (1, 64, 64, 8, 32, True),        # nstage 2, S 2: reduce lanes 2, 3 have nothing to load
    (15, 64, 64, 8, 32, False),      # S 30: lanes 0, 1 in the eight-deep main loop, lanes 2, 3 only in the tail
    (17, 64, 64, 8, 32, False),      # S 34: main loop for all lanes, then a tail for lanes 0, 1 only
    (33, 64, 64, 32, 32, False),     # nstage 264, S 256: splits 0..7 own two stages, the others one; four row tiles per image
    (3, 128, 128, 8, 16, True),      # S 3: lane 3 idle
    (65, 128, 128, 8, 16, False),    # nstage 65, S 64: split 0 owns two stages
    (2, 64, 64, 8, 64, True),        # W = 2 TW: halo between tile columns; the weight gradient is the library's (bf16 output)
    (2, 128, 128, 16, 48, False),    # W = 3 TW of the Cin 128 instance; the weight gradient is the library's (bf16 output)
    (1, 64, 128, 8, 32, True),       # the input gradient is the library's (no 128 -> 64 instance)
]
# the split counts the cases above are there for: (N, Cin, Cout, H, W) -> S; 0 = no hand-written weight gradient at this width
CONV3X3_SPLITS = {(1, 64, 64, 8, 32): 2, (15, 64, 64, 8, 32): 30, (17, 64, 64, 8, 32): 34, (33, 64, 64, 32, 32): 256, (3, 128, 128, 8, 16): 3,
                  (65, 128, 128, 8, 16): 64, (2, 64, 64, 8, 64): 0, (2, 128, 128, 16, 48): 0, (1, 64, 128, 8, 32): 2}

# ---- ops.conv2d_split (csrc/conv_gemm.hip, conv_stem.hip, conv.hip's three-term kernels): (N, Cin, Cout, K, stride, pad, H, W, bias)
CONV2D = [
    (3, 2, 64, 7, 2, 3, 40, 56, True),        # stem: partial 8 x 16 tiles on both axes, different counts
    (2, 2, 64, 7, 2, 3, 56, 40, False),       # stem with the axes swapped
    (3, 64, 128, 3, 2, 1, 24, 40, False),     # stride-2 3x3
    (3, 64, 128, 1, 2, 0, 24, 40, False),     # 1x1 downsample
    (5, 128, 32, 3, 1, 1, 8, 24, True),       # BN = 32 head; M = 960 is not a multiple of 128
    (3, 64, 64, 3, 1, 1, 16, 64, False),      # conv3x3s_kernel, two tile columns
    (2, 128, 128, 3, 1, 1, 8, 48, False),     # conv3x3s_kernel, three tile columns
    (15, 64, 64, 3, 1, 1, 8, 32, False),      # conv3x3_wrw3_kernel, S 30
    (17, 64, 64, 3, 1, 1, 8, 32, False),      # conv3x3_wrw3_kernel, S 34
    (33, 64, 64, 3, 1, 1, 32, 32, False),     # conv3x3_wrw3_kernel, unequal stages per split
]
# also run without psi_conv2d_prepare_weight (library_paths.conv_weights_split_in_every_workgroup): one 3x3 and the 1x1
CONV2D_UNPREPARED = [CONV2D[2], CONV2D[3]]

# ---- ops.linear_act / ops.linear_act3 (csrc/linear.hip): (M, N, K)
LINEAR = [(4, 32, 32), (100, 48, 64), (130, 128, 544), (128, 256, 8192), (200, 1024, 1024)]
LINEAR3_EXTRA = [(7, 75, 75), (33, 50, 1100)]       # linear_act3 takes any width
LINEAR_MODES = ['plain', 'leaky', 'leaky_res']
SLOPE = 0.5                                         # exact; gy is even, so slope * gy is an integer too
MIN_TIES = 10                                       # entries with pre-activation == 0 every leaky case must have


def conv3x3_as_conv2d(case):
    N, Cin, Cout, H, W, bias = case
    return (N, Cin, Cout, 3, 1, 1, H, W, bias)


def all_conv_cases():
    """Every convolution geometry of the tables, once (a conv3x3 case and a conv2d case of the same geometry share data and reference)."""
    seen = []
    for c in [conv3x3_as_conv2d(c) for c in CONV3X3] + CONV2D:
        if c not in seen:
            seen.append(c)
    return seen


def all_linear_cases():
    return [(M, N, K, mode) for (M, N, K) in LINEAR + LINEAR3_EXTRA for mode in LINEAR_MODES]


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def int_tensor(shape, lo=1, hi=4, seed=0):
    """A random sign times a uniform integer in [lo, hi], as fp32: never 0, so a dropped term always moves the sum."""
    g = _gen(seed)
    mag = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return (mag * sign).float()


def int_weight(shape, hi=3, seed=0):
    """Uniform integers in [-hi, hi], 0 included, as fp32 (weights and biases)."""
    return torch.randint(-hi, hi + 1, tuple(shape), generator=_gen(seed)).float()


def _seed(case):
    s = 0
    for v in case:
        s = (s * 131 + (int(v) if not isinstance(v, str) else sum(map(ord, v)))) % (2 ** 31 - 1)
    return s


# ------------------------------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------------------------------
ConvData = namedtuple('ConvData', 'x w b dy')
ConvOut = namedtuple('ConvOut', 'y dx gw gb')


@functools.lru_cache(maxsize=None)
def conv_data(case):
    N, Cin, Cout, K, stride, pad, H, W, bias = case
    OH, OW = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    s = _seed(case)
    return ConvData(int_tensor((N, Cin, H, W), seed=s), int_weight((Cout, Cin, K, K), seed=s + 1),
                    int_weight((Cout,), hi=4, seed=s + 2) if bias else None, int_tensor((N, Cout, OH, OW), seed=s + 3))


def conv_eval(data, stride, pad, dtype):
    """(y, dx, gw, gb) of conv2d(x, w, b) under the output gradient dy, evaluated by torch on the CPU in ``dtype``."""
    x = data.x.to(dtype).requires_grad_()
    w = data.w.to(dtype).requires_grad_()
    b = data.b.to(dtype).requires_grad_() if data.b is not None else None
    y = F.conv2d(x, w, b, stride, pad)
    y.backward(data.dy.to(dtype))
    return ConvOut(y.detach(), x.grad, w.grad, b.grad if b is not None else None)


@functools.lru_cache(maxsize=None)
def conv_ref(case):
    """The float64 reference of a case (computed once per process, shared by every test that needs it; do not modify)."""
    return conv_eval(conv_data(case), case[4], case[5], torch.float64)


def conv_magnitudes(data, stride, pad):
    """Largest sum of |products| of the forward (+ |bias|), the input gradient and the weight gradient, in float64."""
    x, w, dy = data.x.double().abs(), data.w.double().abs(), data.dy.double().abs()
    fwd = F.conv2d(x, w, data.b.double().abs() if data.b is not None else None, stride, pad)
    dgrad = torch.nn.grad.conv2d_input(x.shape, w, dy, stride, pad)
    wgrad = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride, pad)
    return float(fwd.max()), float(dgrad.max()), float(wgrad.max()), float(dy.sum((0, 2, 3)).max())


# ------------------------------------------------------------------------------------------------------------------
# dense layers
# ------------------------------------------------------------------------------------------------------------------
LinearData = namedtuple('LinearData', 'x w b res gy act')
LinearOut = namedtuple('LinearOut', 'y gx gw gb gres ties')


@functools.lru_cache(maxsize=None)
def linear_data(case):
    """x, W, bias, residual integers, gy even integers.  In the leaky modes the bias is minus the first row's product, so the whole first
    row of pre-activations is exactly 0 (on top of the zeros the integer sums give by themselves): the tie of LeakyReLU's gradient
    (PyTorch: ``slope`` where the pre-activation == 0) is met N times with non-zero weights and gradients."""
    M, N, K, mode = case
    s = _seed(case[:3])                       # the modes of a shape share x, W and gy
    x, w = int_tensor((M, K), seed=s), int_weight((N, K), seed=s + 1)
    gy = 2 * int_tensor((M, N), lo=1, hi=2, seed=s + 2)
    if mode == 'plain':
        b = int_weight((N,), hi=4, seed=s + 3)
    else:
        b = -(x[0].double() @ w.double().t()).float()
    res = int_tensor((M, N), seed=s + 4) if mode == 'leaky_res' else None
    return LinearData(x, w, b, res, gy, mode != 'plain')


def linear_eval(data, dtype):
    x = data.x.to(dtype).requires_grad_()
    w = data.w.to(dtype).requires_grad_()
    b = data.b.to(dtype).requires_grad_()
    r = data.res.to(dtype).requires_grad_() if data.res is not None else None
    pre = x @ w.t() + b
    y = F.leaky_relu(pre, SLOPE) if data.act else pre
    if r is not None:
        y = y + r
    y.backward(data.gy.to(dtype))
    return LinearOut(y.detach(), x.grad, w.grad, b.grad, r.grad if r is not None else None, int((pre.detach() == 0).sum()))


@functools.lru_cache(maxsize=None)
def linear_ref(case):
    return linear_eval(linear_data(case), torch.float64)


def linear_magnitudes(data):
    """Largest sum of |products| of y (+ |bias| + |residual|), gx, gW and gbias (|G| <= |gy|), in float64."""
    x, w, g = data.x.double().abs(), data.w.double().abs(), data.gy.double().abs()
    fwd = x @ w.t() + data.b.double().abs() + (data.res.double().abs() if data.res is not None else 0)
    return float(fwd.max()), float((g @ w).max()), float((g.t() @ x).max()), float(g.sum(0).max())


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def as_dtype(ref64, dtype):
    """The reference in the dtype the operator stores: to fp32, then (round to nearest even) to bf16 where it stores bf16."""
    r = ref64.float()
    return r.to(torch.bfloat16) if dtype == torch.bfloat16 else r


def mismatches(got, want, kind, limit=6):
    """'' when ``got`` and ``want`` (same dtype, CPU) hold the same bits, else a message with the first differing indices: (n, oy, ox, c) for
    a map [N,C,H,W], (co, tap, ci) for a weight [Cout,Cin,KH,KW], plain indices otherwise."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return ''
    bad = torch.nonzero(got != want)
    rows = []
    for idx in bad[:limit].tolist():
        if kind == 'map':
            n, c, oy, ox = idx
            where = '(n %d, oy %d, ox %d, c %d)' % (n, oy, ox, c)
        elif kind == 'weight':
            co, ci, kh, kw = idx
            where = '(co %d, tap %d, ci %d)' % (co, kh * got.shape[3] + kw, ci)
        else:
            where = str(tuple(idx))
        rows.append('%s got %r want %r' % (where, float(got[tuple(idx)]), float(want[tuple(idx)])))
    return '%d of %d entries differ; first: %s' % (len(bad), got.numel(), '; '.join(rows))
