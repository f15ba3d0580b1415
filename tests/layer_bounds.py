"""Per-element error bounds of the CVAE layer kernels on real-valued (Gaussian) data (test infrastructure; test_conv_gpu.py,
test_precise_gpu.py).  "max error <= a fraction of the tensor's largest entry" cannot see one dropped product (4 % of a typical output of
576 products, 3 % of it allowed); these bounds are per element and derived, not tuned:

  * a result stored in bf16 from an fp32 accumulator, against float64 on the same bf16-rounded operands:
        |y - ref64| <= 2^-8 |ref64| + n 2^-24 mag,      mag = sum of |products| (+ |bias|) of that element, n = number of terms
    — half a bf16 ulp of the stored value, plus the worst case of n fp32 additions.
  * an fp32 result of a long sum (a weight gradient over every pixel of the batch): the worst case is hundreds of times what fp32 does, so
    the kernel is measured against a plain fp32 evaluation instead, as per_body.py does:
        d(t) = max over elements of |t - ref64| / mag;   d(kernel) <= K_NOISE d(fp32 torch on the CPU) + 2^-24.
"""
import torch
import torch.nn.functional as F

import arbiter

K_NOISE = arbiter.K_NOISE
EPS32 = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8


def bf16_store_fraction(got, ref64, mag, nterms):
    """Largest used fraction of the per-element bound of a bf16-stored result (<= 1 passes).  CPU tensors; ref64 / mag float64."""
    bound = HALF_ULP_BF16 * ref64.abs() + nterms * EPS32 * mag
    err = (got.double() - ref64).abs()
    assert bool(torch.isfinite(err).all())
    # an element no product reaches (a strided 1x1 layer's input gradient at the skipped pixels) has bound 0: it must be exactly 0
    frac = torch.where(bound > 0, err / bound, torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return float(frac.max())


def noise_distance(t, ref64, mag):
    """d(t) = max |t - ref64| / mag over the elements."""
    err = (t.double() - ref64).abs()
    assert bool(torch.isfinite(err).all())
    return float((err / mag).max())


def conv_report(x64, w64, b64, g64, stride, pad, y=None, dx=None, gw=None):
    """The figures of one convolution on bf16 maps (one-term products, fp32 accumulation) against float64 on the same bf16-rounded operands
    (CPU float64 tensors, [N,C,H,W] / [Cout,Cin,KH,KW]): the largest used fraction of the per-element bound of the bf16 output ``y`` and
    input gradient ``dx``, and the distances of the fp32 weight gradient ``gw`` and of a plain fp32 evaluation.  Pass what the kernel under
    test produced (a tensor the library produced has no business here)."""
    Cout, Cin, KH, KW = w64.shape
    row = {}
    if y is not None:
        ref = F.conv2d(x64, w64, b64, stride, pad)
        mag = F.conv2d(x64.abs(), w64.abs(), b64.abs() if b64 is not None else None, stride, pad)
        row['y_fraction_of_bound'] = bf16_store_fraction(y.detach().cpu(), ref, mag, KH * KW * Cin + 1)
    if dx is not None:
        ref = torch.nn.grad.conv2d_input(x64.shape, w64, g64, stride, pad)
        mag = torch.nn.grad.conv2d_input(x64.shape, w64.abs(), g64.abs(), stride, pad)
        row['dx_fraction_of_bound'] = bf16_store_fraction(dx.detach().cpu(), ref, mag, KH * KW * Cout + 1)
    if gw is not None:
        ref = torch.nn.grad.conv2d_weight(x64, w64.shape, g64, stride, pad)
        mag = torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, g64.abs(), stride, pad)
        f32 = torch.nn.grad.conv2d_weight(x64.float(), w64.shape, g64.float(), stride, pad)        # plain fp32 on the CPU
        row['gw_d_kernel'], row['gw_d_fp32'] = noise_distance(gw.detach().cpu(), ref, mag), noise_distance(f32, ref, mag)
    return row


def assert_conv_report(row):
    for k in ('y_fraction_of_bound', 'dx_fraction_of_bound'):
        assert row.get(k, 0.0) <= 1, (k, row)
    if 'gw_d_kernel' in row:
        assert row['gw_d_kernel'] <= K_NOISE * row['gw_d_fp32'] + EPS32, row


def record(name, row):
    """Keep the measured figures of a case as JSON next to the arbiter's records, in the sub-directory cvae_layers/
    (profiles/cvae_layers_exactness.json is the committed copy)."""
    arbiter.record(name, row, sub='cvae_layers')
