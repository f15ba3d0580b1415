"""The CVAE layer kernels (csrc/conv.hip, conv_gemm.hip, conv_stem.hip, linear.hip; ops.conv3x3, conv2d_split, linear_act, linear_act3) on
EXACT-INTEGER data against a float64 CPU evaluation, bit for bit.

tests/exact_cases.py holds the cases and says why zero tolerance is legitimate (every partial sum is an integer below 2^24: one correct bit
pattern whatever the tiling, split or summation order); tests/test_exact_cases_cpu.py proves that precondition for every case.  The cases
sit on the edges nothing else runs: more than one tile column (the halo is a neighbouring tile, not the zero padding), split counts of the
weight gradient around the four-lane / eight-deep reduce loop (2, 3, 30, 34, 64 of 65, 256 of 264 stages), non-square maps, partial tiles.
Every comparison is ``torch.equal`` on the reference cast to the stored dtype (fp32, then round-to-nearest-even to bf16); the only
tolerances are on the tensors ops.conv3x3 takes from the library (aten.convolution_backward on bf16 maps rounds its output to bf16):
the weight gradient at W = 64 / W = 48 (no hand-written instance at these widths) and the input gradient of the 64 -> 128 layer.

Integer data cannot see rounding (nothing rounds): test_prepare_and_rotate_weight checks the fp32 -> bf16 conversion on ties and their
neighbours, and tests/test_conv_gpu.py / test_precise_gpu.py hold per-element bounds on Gaussian data."""
import pytest
import torch

import exact_cases as E
import library_paths
from psi_release_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CL = torch.channels_last
ids = lambda c: '-'.join(map(str, c)) if isinstance(c, tuple) else str(c)


def _module(case, data):
    N, Cin, Cout, K, stride, pad, H, W, bias = case
    conv = torch.nn.Conv2d(Cin, Cout, K, stride, pad, bias=bias).to(DEV).to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(data.w)                      # integer fp32 master weights, channels_last like the models'
        if bias:
            conv.bias.copy_(data.b)
    return conv


def _same(got, ref64, kind, what):
    """``got`` (device tensor) holds the bits of the float64 reference cast to its dtype."""
    got = got.detach().cpu().contiguous()
    msg = E.mismatches(got, E.as_dtype(ref64, got.dtype).contiguous(), kind)
    assert not msg, '%s: %s' % (what, msg)


# ------------------------------------------------------------------------------------------------------------------
# ops.conv3x3: bf16 maps, fp32 master weights
# ------------------------------------------------------------------------------------------------------------------
LIBRARY_GW = [c for c in E.CONV3X3 if E.CONV3X3_SPLITS[c[:5]] == 0]          # W = 64, W = 48
LIBRARY_DX = [(1, 64, 128, 8, 32, True)]


@pytest.mark.parametrize('case', E.CONV3X3, ids=ids)
def test_conv3x3_exact(case):
    N, Cin, Cout, H, W, bias = case
    geom = E.conv3x3_as_conv2d(case)
    data, ref = E.conv_data(geom), E.conv_ref(geom)
    conv = _module(geom, data)
    x = data.x.to(DEV).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_()
    dy = data.dy.to(DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    assert ops.conv3x3_supported(conv, x)
    L = hip.lib()
    # the case sits where the table says: split count of the weight gradient, hand-written or library gradients
    assert L.psi_conv3x3_wrw_workspace_floats(N, H, W, Cin, Cout) // (Cout * 9 * Cin) == E.CONV3X3_SPLITS[case[:5]]
    assert bool(L.psi_conv3x3_supported(Cout, Cin, H, W)) == (case not in LIBRARY_DX)
    y = ops.conv3x3(x, conv)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL)
    y.backward(dy)
    assert x.grad.dtype == torch.bfloat16 and conv.weight.grad.dtype == torch.float32
    _same(y, ref.y, 'map', 'y')
    if case in LIBRARY_DX:       # the library's bf16 input gradient: its existing bound (tests/test_conv_gpu.py)
        assert float((x.grad.float().cpu().double() - ref.dx).abs().max()) <= 2 ** -7 * float(ref.dx.abs().max())
    else:
        _same(x.grad, ref.dx, 'map', 'dx')
    if case in LIBRARY_GW:       # the library's bf16 weight gradient: its existing bound (tests/test_conv_gpu.py)
        assert float((conv.weight.grad.cpu().double() - ref.gw).abs().max()) <= 2 ** -6 * float(ref.gw.abs().max())
    else:
        _same(conv.weight.grad, ref.gw, 'weight', 'gw')
    if bias:
        _same(conv.bias.grad, ref.gb, 'vector', 'gb')


def test_conv3x3_weight_gradient_is_run_to_run_bit_identical():
    """conv.hip promises a fixed summation order (splits own fixed stages, the reduce adds them in a fixed order): five backward passes of
    the S 34 and the unequal-stage cases on Gaussian data give the same weight-gradient bits."""
    for (N, Cin, Cout, H, W) in [(17, 64, 64, 8, 32), (33, 64, 64, 32, 32)]:
        torch.manual_seed(N)
        conv = torch.nn.Conv2d(Cin, Cout, 3, 1, 1, bias=False).to(DEV).to(memory_format=CL)
        x = torch.randn(N, Cin, H, W, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(N, Cout, H, W, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
        y = ops.conv3x3(x, conv)
        got = []
        for _ in range(5):
            conv.zero_grad()
            y.backward(dy, retain_graph=True)
            got.append(conv.weight.grad.clone())
        assert float(got[0].abs().max()) > 0
        for g in got[1:]:
            assert torch.equal(g, got[0])


def _bits(v):
    """fp32 values from their bit patterns"""
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in v], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize('Cin,Cout', [(64, 64), (128, 256), (64, 128)])
def test_prepare_and_rotate_weight(Cin, Cout):
    """psi_conv3x3_prepare_weight / psi_conv3x3_rotate_weight: the fp32 -> bf16 conversion is round-to-nearest-even (what torch's is) on
    Gaussian weights and on hand-placed ties between two bf16 neighbours (both parities, both signs), values one fp32 ulp either side of a
    tie, +-0 and the largest finite bf16; the rotated layout is [ci][2-kh][2-kw][co]."""
    torch.manual_seed(Cin + Cout)
    w = torch.randn(Cout, 3, 3, Cin)
    special = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x404A, 0x0080, 0x7F7E):                  # even and odd last kept bit
        for sign in (0, 0x8000):
            for low in (0x8000, 0x7FFF, 0x8001):                                # the tie and one fp32 ulp either side
                special.append(((hi | sign) << 16) | low)
    special += [0x00000000, 0x80000000, 0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF]      # +-0, the largest finite bf16 (and the last fp32 that rounds to it)
    sp = _bits(special)
    assert bool(torch.isfinite(sp.to(torch.bfloat16).float()).all())
    flat = w.view(-1)
    pos = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(1))[:4 * len(special)]
    flat[pos] = sp.repeat(4)
    w = w.to(DEV)
    L = hip.lib()
    wb = torch.zeros(Cout, 3, 3, Cin, device=DEV, dtype=torch.bfloat16)
    wt = torch.zeros(Cin, 3, 3, Cout, device=DEV, dtype=torch.bfloat16)
    hip.check(L.psi_conv3x3_prepare_weight(hip.ptr(w), Cin, Cout, hip.ptr(wb), hip.ptr(wt), hip.stream()), 'psi_conv3x3_prepare_weight')
    bits = lambda t: t.contiguous().view(torch.int16).cpu()                      # (torch.equal would call -0 and +0 the same)
    want_b = w.to(torch.bfloat16)
    want_t = want_b.permute(3, 1, 2, 0).flip(1, 2).contiguous()
    assert torch.equal(bits(wb), bits(want_b))
    assert torch.equal(bits(wt), bits(want_t))
    wb_only = torch.zeros_like(wb)                                              # without the rotated layout (no input gradient wanted)
    hip.check(L.psi_conv3x3_prepare_weight(hip.ptr(w), Cin, Cout, hip.ptr(wb_only), None, hip.stream()), 'psi_conv3x3_prepare_weight')
    assert torch.equal(bits(wb_only), bits(want_b))
    wr = torch.zeros_like(wt)
    hip.check(L.psi_conv3x3_rotate_weight(hip.ptr(wb), Cin, Cout, hip.ptr(wr), hip.stream()), 'psi_conv3x3_rotate_weight')
    assert torch.equal(bits(wr), bits(want_t))


# ------------------------------------------------------------------------------------------------------------------
# ops.conv2d_split: three-term products on fp32 maps, one-term products on bf16 maps
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['split3_fp32', 'one_term_bf16'])
@pytest.mark.parametrize('case,prepared', [(c, True) for c in E.CONV2D] + [(c, False) for c in E.CONV2D_UNPREPARED], ids=ids)
def test_conv2d_split_exact(case, prepared, mode, monkeypatch):
    N, Cin, Cout, K, stride, pad, H, W, bias = case
    data, ref = E.conv_data(case), E.conv_ref(case)
    conv = _module(case, data)
    assert ops.conv2d_supported(conv)
    if not prepared:
        assert ops._conv2d_prepared_ok(Cin, Cout, K, K, stride, pad)                # (else the default route is this one already)
        library_paths.conv_weights_split_in_every_workgroup(monkeypatch)
    dt = torch.float32 if mode == 'split3_fp32' else torch.bfloat16
    x = data.x.to(DEV).to(dt).contiguous(memory_format=CL).requires_grad_(Cin > 2)    # (the stem's input needs no gradient)
    dy = data.dy.to(DEV).to(dt).contiguous(memory_format=CL)
    y = ops.conv2d_split(x, conv, nterm=3 if dt == torch.float32 else 1, out_bf16=dt == torch.bfloat16)
    assert y.dtype == dt and y.is_contiguous(memory_format=CL)
    y.backward(dy)
    _same(y, ref.y, 'map', 'y')
    if Cin > 2:
        assert x.grad.dtype == dt
        _same(x.grad, ref.dx, 'map', 'dx')
    assert conv.weight.grad.dtype == torch.float32
    _same(conv.weight.grad, ref.gw, 'weight', 'gw')
    if bias:
        _same(conv.bias.grad, ref.gb, 'vector', 'gb')


# ------------------------------------------------------------------------------------------------------------------
# ops.linear_act (bf16 products) / ops.linear_act3 (three-term products)
# ------------------------------------------------------------------------------------------------------------------
def _linear(op, case, x_bf16=False):
    M, N, K, mode = case
    data, ref = E.linear_data(case), E.linear_ref(case)
    if data.act:
        assert ref.ties >= E.MIN_TIES               # pre-activation == 0: the gradient takes the slope there (PyTorch's convention)
    x = data.x.to(DEV)
    x = (x.to(torch.bfloat16) if x_bf16 else x).requires_grad_()
    w, b = data.w.to(DEV).requires_grad_(), data.b.to(DEV).requires_grad_()
    r = data.res.to(DEV).requires_grad_() if data.res is not None else None
    gy = data.gy.to(DEV)
    y = op(x, w, b, 'leaky_relu' if data.act else None, E.SLOPE, r)
    y.backward(gy)
    assert y.dtype == torch.float32 and x.grad.dtype == x.dtype
    _same(y, ref.y, 'matrix', 'y')
    _same(x.grad, ref.gx, 'matrix', 'gx')
    _same(w.grad, ref.gw, 'matrix', 'gW')
    _same(b.grad, ref.gb, 'vector', 'gbias')
    if r is not None:                               # (here the mask came from the stored activation, not from y)
        assert torch.equal(r.grad, gy)


@pytest.mark.parametrize('mode', E.LINEAR_MODES)
@pytest.mark.parametrize('shape', E.LINEAR, ids=ids)
def test_linear_act_exact(shape, mode):
    _linear(ops.linear_act, shape + (mode,))


def test_linear_act_exact_bf16_input():
    _linear(ops.linear_act, (130, 128, 544, 'leaky_res'), x_bf16=True)          # gx is bf16 then


@pytest.mark.parametrize('mode', E.LINEAR_MODES)
@pytest.mark.parametrize('shape', E.LINEAR + E.LINEAR3_EXTRA, ids=ids)
def test_linear_act3_exact(shape, mode):
    _linear(ops.linear_act3, shape + (mode,))
