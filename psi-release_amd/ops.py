"""Autograd operators over the C ABI (include/psi_hip.h).  Same call signatures as the reference's ops.

* ``chamferFunction`` / ``chamferDist``   <- chamfer_pytorch/dist_chamfer.py:13-53 (+ idx variant, dist_chamfer_idx.py)
* ``sdf_sample``                          <- F.grid_sample call of fitting_proxe.py:144-151
* ``penetration_loss``                    <- fitting_proxe.py:155-158 (no host sync)

Inputs must live on the GPU; there is no CPU path (hip.ptr raises).
"""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import NamedTuple

import torch
from torch import nn
from torch.autograd import Function


from . import hip


# ------------------------------------------------------------------------------------------
# Chamfer
# ------------------------------------------------------------------------------------------
def chamfer_forward_raw(xyz1, xyz2, both=True):
    """chamfer.forward (chamfer_cuda.cpp:17-19): returns dist1, idx1, dist2, idx2 (None, None when both=False)."""
    xyz1 = xyz1.contiguous().float()
    xyz2 = xyz2.contiguous().float()
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if xyz2.shape[0] != B or xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
        raise ValueError('expected xyz1 [B,n,3] and xyz2 [B,m,3]')
    dev = xyz1.device
    dist1 = torch.zeros(B, n, device=dev)
    idx1 = torch.zeros(B, n, dtype=torch.int32, device=dev)
    dist2 = torch.zeros(B, m, device=dev) if both else None
    idx2 = torch.zeros(B, m, dtype=torch.int32, device=dev) if both else None
    L = hip.lib()
    nbytes = L.psi_chamfer_workspace_bytes(B, n, m)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    hip.check(L.psi_chamfer_forward(hip.ptr(xyz1), hip.ptr(xyz2), B, n, m, hip.ptr(dist1), hip.ptr(idx1),
                                    hip.ptr(dist2), hip.ptr(idx2), hip.ptr(ws), hip.stream()), 'psi_chamfer_forward')
    return dist1, idx1, dist2, idx2


class chamferFunction(Function):
    """dist_chamfer.py:13-46.  ``return_idx`` selects the dist_chamfer_idx.py:28 output tuple."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, return_idx=False, both=True):
        xyz1 = xyz1.contiguous()
        xyz2 = xyz2.contiguous()
        dist1, idx1, dist2, idx2 = chamfer_forward_raw(xyz1, xyz2, both)
        ctx.both = both
        if both:
            ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        else:
            ctx.save_for_backward(xyz1, xyz2, idx1)
            dist2 = torch.zeros(xyz2.shape[0], xyz2.shape[1], device=xyz1.device)
            idx2 = torch.zeros(xyz2.shape[0], xyz2.shape[1], dtype=torch.int32, device=xyz1.device)
        ctx.mark_non_differentiable(idx1, idx2)
        if return_idx:
            return dist1, dist2, idx1, idx2
        return dist1, dist2

    @staticmethod
    def backward(ctx, graddist1, graddist2, *unused):
        if ctx.both:
            xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        else:
            xyz1, xyz2, idx1 = ctx.saved_tensors
            idx2 = None
        B, n, _ = xyz1.shape
        m = xyz2.shape[1]
        graddist1 = graddist1.contiguous()
        need2 = ctx.needs_input_grad[1]
        use_dir2 = ctx.both and graddist2 is not None
        gradxyz1 = torch.zeros_like(xyz1)
        gradxyz2 = torch.zeros_like(xyz2) if (need2 or use_dir2) else None
        g2 = graddist2.contiguous() if use_dir2 else None
        hip.check(hip.lib().psi_chamfer_backward(hip.ptr(xyz1), hip.ptr(xyz2), hip.ptr(gradxyz1), hip.ptr(gradxyz2),
                                                 hip.ptr(graddist1), hip.ptr(g2), hip.ptr(idx1),
                                                 hip.ptr(idx2) if use_dir2 else None, B, n, m, hip.stream()),
                  'psi_chamfer_backward')
        return gradxyz1, (gradxyz2 if need2 else None), None, None


class chamferDist(nn.Module):
    """dist_chamfer.py:48-53: ``chamferDist()(xyz1, xyz2) -> (dist1, dist2)``.

    ``one_sided=True`` skips the scene->body direction that PSI discards (fitting_proxe.py:136);
    ``dist2`` is then returned as zeros."""

    def __init__(self, return_idx: bool = False, one_sided: bool = False):
        super().__init__()
        self.return_idx = return_idx
        self.one_sided = one_sided

    def forward(self, input1, input2):
        return chamferFunction.apply(input1, input2, self.return_idx, not self.one_sided)


# ------------------------------------------------------------------------------------------
# SDF lookup
# ------------------------------------------------------------------------------------------
class _SdfSample(Function):
    @staticmethod
    def forward(ctx, verts, sdf, scene_id, gmin, gmax, align_corners):
        verts = verts.contiguous().float()
        B, V, _ = verts.shape
        S, D = sdf.shape[0], sdf.shape[1]
        out = torch.empty(B, V, device=verts.device)
        og = torch.empty(B, V, 3, device=verts.device)
        hip.check(hip.lib().psi_sdf_sample_forward(hip.ptr(sdf), hip.ptr(scene_id), hip.ptr(gmin), hip.ptr(gmax),
                                                   hip.ptr(verts), B, V, D, S, int(bool(align_corners)), hip.ptr(out),
                                                   hip.ptr(og), hip.stream()), 'psi_sdf_sample_forward')
        ctx.save_for_backward(og)
        return out

    @staticmethod
    def backward(ctx, gout):
        (og,) = ctx.saved_tensors
        B, V, _ = og.shape
        gv = torch.zeros_like(og)
        hip.check(hip.lib().psi_sdf_sample_backward(hip.ptr(gout.contiguous()), hip.ptr(og), B, V, hip.ptr(gv),
                                                    hip.stream()), 'psi_sdf_sample_backward')
        return gv, None, None, None, None, None


def sdf_sample(verts, sdf, grid_min, grid_max, scene_id=None, align_corners=True):
    """Trilinear SDF values [B,V] of world-space ``verts`` [B,V,3].

    sdf [S,D,D,D] (or [D,D,D]) holds ONE volume per scene, ``scene_id`` [B] int32 picks it (None = scene 0);
    grid_min / grid_max [S,3] (or [3]).  Equivalent to fitting_proxe.py:144-151 with the volume not replicated."""
    if sdf.dim() == 3:
        sdf = sdf.unsqueeze(0)
    sdf = sdf.contiguous().float()
    S = sdf.shape[0]
    gmin = grid_min.reshape(-1, 3).contiguous().float()
    gmax = grid_max.reshape(-1, 3).contiguous().float()
    if gmin.shape[0] != S or gmax.shape[0] != S:
        raise ValueError('grid_min/grid_max must have one row per scene volume')
    if scene_id is not None:
        scene_id = scene_id.to(device=verts.device, dtype=torch.int32).contiguous()
    return _SdfSample.apply(verts, sdf, scene_id, gmin, gmax, align_corners)


class _PenLoss(Function):
    """mean |sdf| over the negative entries of the whole batch, 0 when there are none (fitting_proxe.py:155-158)."""

    @staticmethod
    def forward(ctx, vals):
        vals = vals.contiguous()
        stats = torch.zeros(2, device=vals.device)
        hip.check(hip.lib().psi_sdf_penetration_stats(hip.ptr(vals), vals.numel(), hip.ptr(stats), hip.stream()),
                  'psi_sdf_penetration_stats')
        ctx.save_for_backward(vals, stats)
        return torch.where(stats[1] > 0, stats[0] / stats[1].clamp(min=1.0), torch.zeros((), device=vals.device))

    @staticmethod
    def backward(ctx, g):
        vals, stats = ctx.saved_tensors
        scale = torch.where(stats[1] > 0, -g / stats[1].clamp(min=1.0), torch.zeros((), device=vals.device))
        return (vals < 0).to(vals.dtype) * scale


def penetration_loss(body_sdf):
    return _PenLoss.apply(body_sdf)


# ------------------------------------------------------------------------------------------
# Exact NN index over a static scene cloud
# ------------------------------------------------------------------------------------------
class SceneNNIndex:
    """kd-tree over one scene's points (psi_nn_index_*).  ``query`` returns exactly what ``chamfer.forward`` returns for
    the body->scene direction against that cloud (bit-identical dist1 / idx1)."""

    def __init__(self, points, device='cuda'):
        import ctypes
        import numpy as np
        pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
        pts = np.ascontiguousarray(pts.reshape(-1, 3), dtype=np.float32)
        self.m = pts.shape[0]
        self.device = torch.device(device)
        self.points = torch.tensor(pts, device=self.device)           # for the backward gather
        h = hip.Handle('psi_nn_index_destroy')
        with torch.cuda.device(self.device):
            hip.check(hip.lib().psi_nn_index_create(ctypes.byref(h), pts.ctypes.data_as(ctypes.c_void_p), self.m),
                      'psi_nn_index_create')
        self.handle = h

    def query(self, xyz1, hint=None):
        """hint: int32 [B,n] warm-start buffer (previous winners, -1 = none), updated in place; results do not depend on it."""
        xyz1 = xyz1.contiguous().float()
        B, n, _ = xyz1.shape
        dist = torch.empty(B, n, device=xyz1.device)
        idx = torch.empty(B, n, dtype=torch.int32, device=xyz1.device)
        hip.check(hip.lib().psi_nn_index_query(self.handle, hip.ptr(xyz1), B, n, hip.ptr(dist), hip.ptr(idx), hip.ptr(hint),
                                               hip.stream()), 'psi_nn_index_query')
        return dist, idx


class _IndexedChamfer(Function):
    @staticmethod
    def forward(ctx, xyz1, index):
        dist, idx = index.query(xyz1)
        ctx.index = index
        ctx.save_for_backward(xyz1, idx)
        return dist

    @staticmethod
    def backward(ctx, gdist):
        xyz1, idx = ctx.saved_tensors
        nn = ctx.index.points[idx.long()]                                  # [B,n,3]
        return 2.0 * gdist.unsqueeze(-1) * (xyz1 - nn), None               # chamfer.cu:155-174, query side


def chamfer_to_scene(xyz1, index: SceneNNIndex):
    """dist1 [B,n] of ``chamferDist()(xyz1, scene.repeat(B))`` through the scene's exact NN index."""
    return _IndexedChamfer.apply(xyz1, index)


class SceneSet:
    """The static scenes of a training set: one exact NN index per scene slot, queried in ONE launch with the per-body
    scene slot (psi_nn_index_set_query).  ``chamfer_to_scenes`` equals ``chamferDist()(xyz1, verts_table[slot])[0]`` bit for
    bit (train_s1.py:159-169) without the O(n*m) scan or the [B,m,3] gather, and its launch shape does not depend on
    which scenes a batch mixes (so a whole training step can live in one HIP graph)."""

    def __init__(self, verts_table, device='cuda'):
        import ctypes
        self.verts_table = verts_table.contiguous()                     # [S,m,3] device (backward gather)
        self.device = torch.device(device)
        self.indices = [SceneNNIndex(self.verts_table[s], self.device) for s in range(self.verts_table.shape[0])]
        arr = (ctypes.c_void_p * len(self.indices))(*[ix.handle.value for ix in self.indices])
        h = hip.Handle('psi_nn_index_set_destroy')
        with torch.cuda.device(self.device):
            hip.check(hip.lib().psi_nn_index_set_create(ctypes.byref(h), arr, len(self.indices)), 'psi_nn_index_set_create')
        self.handle = h

    def query(self, xyz1, slot):
        xyz1 = xyz1.contiguous().float()
        B, n, _ = xyz1.shape
        dist = torch.empty(B, n, device=xyz1.device)
        idx = torch.empty(B, n, dtype=torch.int32, device=xyz1.device)
        hip.check(hip.lib().psi_nn_index_set_query(self.handle, hip.ptr(slot), hip.ptr(xyz1), B, n, hip.ptr(dist), hip.ptr(idx),
                                                   hip.stream()), 'psi_nn_index_set_query')
        return dist, idx


class _SceneSetChamfer(Function):
    @staticmethod
    def forward(ctx, xyz1, scenes, slot):
        dist, idx = scenes.query(xyz1, slot)
        ctx.scenes = scenes
        ctx.save_for_backward(xyz1, idx, slot)
        return dist

    @staticmethod
    def backward(ctx, gdist):
        xyz1, idx, slot = ctx.saved_tensors
        nn = ctx.scenes.verts_table[slot.long().unsqueeze(1), idx.long()]     # [B,n,3]
        return 2.0 * gdist.unsqueeze(-1) * (xyz1 - nn), None, None            # chamfer.cu:155-174, query side


def chamfer_to_scenes(xyz1, scenes: SceneSet, slot):
    """dist1 [B,n] of every body against its own scene.  slot: int32 device [B]."""
    assert slot.dtype == torch.int32 and slot.is_contiguous()
    return _SceneSetChamfer.apply(xyz1, scenes, slot)


# ------------------------------------------------------------------------------------------
# Dense layers on the matrix cores (csrc/linear.hip): y = act(x W^T + b) (+ residual), bf16 MFMA with fp32 accumulation
# ------------------------------------------------------------------------------------------
class _LinearAct(Function):
    """nn.Linear (+ LeakyReLU, + skip connection) as ONE hand-written bf16-MFMA kernel per direction; replaces, on the bf16 path of the
    CVAEs, the cast / GEMM / bias-activation / add kernels PyTorch launches per layer (net_layers.py:28-43, cvae.py:474-492)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, act, slope):
        if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
            raise ValueError('linear_act: x [M,K] and weight [N,K] expected, got %s / %s' % (tuple(x.shape), tuple(weight.shape)))
        M, K = x.shape
        N = weight.shape[0]
        if K % 16 or N % 16:
            raise ValueError('linear_act: K and N must be multiples of 16 (got K=%d, N=%d)' % (K, N))
        xb = x.dtype == torch.bfloat16
        xc = x.detach().contiguous() if xb else x.detach().contiguous().float()
        w = weight.detach().contiguous().float()
        b = bias.detach().contiguous().float() if bias is not None else None
        r = residual.detach().contiguous().float() if residual is not None else None
        y = torch.empty(M, N, device=x.device)
        a_out = torch.empty(M, N, device=x.device) if (act and residual is not None) else None
        L = hip.lib()
        nws = L.psi_linear_workspace_floats(M, N, K)
        ws = torch.empty(nws, device=x.device) if nws else None
        hip.check(L.psi_linear_forward(hip.ptr(xc), int(xb), hip.ptr(w), hip.ptr(b), hip.ptr(r), M, N, K, int(act), float(slope), hip.ptr(y),
                                       hip.ptr(a_out), hip.ptr(ws), hip.stream()), 'psi_linear_forward')
        ctx.act, ctx.slope, ctx.xb = int(act), float(slope), xb
        ctx.has_bias, ctx.has_res = bias is not None, residual is not None
        # without a residual the output itself carries the sign of the pre-activation
        ctx.save_for_backward(xc, w, (a_out if a_out is not None else y) if act else torch.empty(0, device=x.device))
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, w, a_out = ctx.saved_tensors
        M, K = xc.shape
        N = w.shape[0]
        gy = gy.contiguous().float()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        # (dX, dW + dbias as ONE hand-written launch pair with LDS-staged transposed operands: 26 vs 38 us for a 128 x 512 x 512 layer against the
        # library route of mask, cast, two GEMMs, column sum — tests/library_paths.py keeps that route for comparison)
        gx = torch.empty(M, K, device=gy.device, dtype=torch.bfloat16 if ctx.xb else torch.float32) if need_x else None
        gw = torch.empty(N, K, device=gy.device) if (need_w or need_b) else None         # gbias is produced by the dW kernel
        gb = torch.empty(N, device=gy.device) if need_b else None
        nws = hip.lib().psi_linear_backward_workspace_floats(M, N, K) if need_x else 0
        ws = torch.empty(nws, device=gy.device) if nws else None
        hip.check(hip.lib().psi_linear_backward(hip.ptr(gy), hip.ptr(a_out) if ctx.act else None, hip.ptr(xc), int(ctx.xb), hip.ptr(w), M, N, K,
                                                ctx.slope, hip.ptr(gx), hip.ptr(gw), hip.ptr(gb), hip.ptr(ws), hip.stream()), 'psi_linear_backward')
        return gx, gw if need_w else None, gb, gy if (ctx.has_res and ctx.needs_input_grad[3]) else None, None, None


def linear_act(x, weight, bias=None, act=None, slope=0.01, residual=None):
    """act(x @ weight.T + bias) (+ residual) on the HIP bf16-MFMA kernels; ``act`` is None or 'leaky_relu'.  x: [M,K] fp32 or bf16."""
    if act not in (None, 'leaky_relu'):
        raise ValueError('act must be None or "leaky_relu"')
    return _LinearAct.apply(x, weight, bias, residual, 1 if act else 0, slope)


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm (training statistics) + ReLU + skip connection of the scene trunk: psi_bn_forward / psi_bn_backward
# ------------------------------------------------------------------------------------------------------------------
def _ptr_cl(t):
    """Device pointer of a channels_last (NHWC in memory) 4-D tensor (None -> NULL)."""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous(memory_format=torch.channels_last)):
        raise hip.PsiHipError('expected a channels_last GPU tensor')
    return t.data_ptr()


def _bn_mask_from_x():
    """True: a BatchNorm + ReLU layer without a skip connection takes its backward's ReLU mask from x and two per-channel numbers instead of
    reading the stored output (one map less per pass, bit-identical gradients; the tests patch this to False to check exactly that)"""
    return True


class _BNAct(Function):
    """y = act(batch_norm(x) (+ residual)) on NHWC bf16 maps, batch statistics (include/psi_hip.h: psi_bn_forward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        N, C, H, W = x.shape
        M = N * H * W
        xc = x.contiguous(memory_format=torch.channels_last)
        rc = residual.contiguous(memory_format=torch.channels_last) if residual is not None else None
        y = torch.empty_like(xc, memory_format=torch.channels_last)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        invstd = torch.empty(C, device=x.device, dtype=torch.float32)
        L = hip.lib()
        ws = torch.empty(L.psi_bn_workspace_floats(M, C), device=x.device, dtype=torch.float32)
        track = bn.track_running_stats and bn.running_mean is not None
        hip.check(L.psi_bn_forward(_ptr_cl(xc), _ptr_cl(rc), hip.ptr(weight), hip.ptr(bias),
                                   hip.ptr(bn.running_mean) if track else None, hip.ptr(bn.running_var) if track else None,
                                   hip.ptr(bn.num_batches_tracked) if track else None, M, C, int(relu),
                                   float(bn.momentum if bn.momentum is not None else 0.1), float(bn.eps), _ptr_cl(y), hip.ptr(mean),
                                   hip.ptr(invstd), hip.ptr(ws), hip.stream()), 'psi_bn_forward')
        # a ReLU layer without a skip connection: the backward recomputes the mask from x (one map less per pass) and y is not kept for it
        keep_y = relu and (residual is not None or not _bn_mask_from_x())
        ctx.save_for_backward(xc, y if keep_y else None, weight, bias, mean, invstd)
        ctx.relu, ctx.has_res, ctx.dims = bool(relu), residual is not None, (M, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, y, weight, bias, mean, invstd = ctx.saved_tensors
        M, C = ctx.dims
        dyc = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(xc, memory_format=torch.channels_last)
        dres = torch.empty_like(xc, memory_format=torch.channels_last) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        dgamma = torch.empty(C, device=xc.device, dtype=torch.float32)
        dbeta = torch.empty(C, device=xc.device, dtype=torch.float32)
        L = hip.lib()
        ws = torch.empty(L.psi_bn_workspace_floats(M, C), device=xc.device, dtype=torch.float32)
        hip.check(L.psi_bn_backward_t(_ptr_cl(dyc), 0, _ptr_cl(xc), _ptr_cl(y), hip.ptr(weight), hip.ptr(bias.detach().float()), hip.ptr(mean),
                                      hip.ptr(invstd), M, C, int(ctx.relu), _ptr_cl(dx), _ptr_cl(dres), hip.ptr(dgamma), hip.ptr(dbeta), hip.ptr(ws),
                                      hip.stream()), 'psi_bn_backward_t')
        return dx, dgamma, dbeta, dres, None, None


def bn_act(x, bn, relu=True, residual=None):
    """``relu(bn(x) + residual)`` (each part optional) of an ``nn.BatchNorm2d`` in TRAINING mode on a bf16 channels_last map, as one
    fused HIP op (statistics pass + one apply pass; the backward likewise) instead of the library's three BN launches plus separate
    ReLU / add launches.  Updates ``bn.running_mean / running_var / num_batches_tracked`` like the module would."""
    if x.dtype != torch.bfloat16 or not x.is_cuda or x.dim() != 4:
        raise ValueError('bn_act: expected a 4-D bf16 CUDA tensor')
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape):
        raise ValueError('bn_act: residual must match x')
    return _BNAct.apply(x, bn.weight, bn.bias, residual, bn, relu)


class _MaxPool3x3s2(Function):
    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        xc = x.contiguous(memory_format=torch.channels_last)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((N, C, OH, OW), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
        idx = torch.empty(N * OH * OW * C, device=x.device, dtype=torch.uint8)
        hip.check(hip.lib().psi_maxpool3x3s2_forward(_ptr_cl(xc), N, H, W, C, _ptr_cl(y), hip.ptr(idx), hip.stream()), 'psi_maxpool3x3s2_forward')
        ctx.save_for_backward(idx)
        ctx.dims = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        N, C, H, W = ctx.dims
        dyc = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty((N, C, H, W), device=dy.device, dtype=dy.dtype, memory_format=torch.channels_last)
        hip.check(hip.lib().psi_maxpool3x3s2_backward(_ptr_cl(dyc), hip.ptr(idx), N, H, W, C, _ptr_cl(dx), hip.stream()), 'psi_maxpool3x3s2_backward')
        return dx


def maxpool3x3s2(x):
    """``nn.MaxPool2d(kernel_size=3, stride=2, padding=1)`` (the trunk's stem) on a bf16 channels_last map: one gather pass each way."""
    if x.dtype != torch.bfloat16 or not x.is_cuda or x.dim() != 4 or x.shape[1] % 8:
        raise ValueError('maxpool3x3s2: expected a 4-D bf16 CUDA tensor with a multiple of 8 channels')
    return _MaxPool3x3s2.apply(x)


# ------------------------------------------------------------------------------------------------------------------
# 3x3 / stride 1 / padding 1 convolutions of the trunk on the hand-written implicit-GEMM kernel (csrc/conv.hip)
# ------------------------------------------------------------------------------------------------------------------
class _Conv3x3(Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        N, Cin, H, W = x.shape
        Cout = weight.shape[0]
        xc = x.contiguous(memory_format=torch.channels_last)
        w4 = weight.detach().permute(0, 2, 3, 1)                                           # [Cout,3,3,Cin]: a view for a channels_last weight
        wt = None
        if w4.dtype == torch.float32 and w4.is_contiguous():
            # master weight -> bf16, forward layout and (when the input needs a gradient) the rotated layout of the backward: one launch
            wb = torch.empty(Cout, 3, 3, Cin, device=x.device, dtype=torch.bfloat16)
            if ctx.needs_input_grad[0] and hip.lib().psi_conv3x3_supported(Cout, Cin, H, W):
                wt = torch.empty(Cin, 3, 3, Cout, device=x.device, dtype=torch.bfloat16)
            hip.check(hip.lib().psi_conv3x3_prepare_weight(hip.ptr(w4), Cin, Cout, hip.ptr(wb), hip.ptr(wt), hip.stream()), 'psi_conv3x3_prepare_weight')
        else:
            wb = w4.contiguous().to(torch.bfloat16)
        y = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
        b = bias.detach().float().contiguous() if bias is not None else None
        hip.check(hip.lib().psi_conv3x3_forward(_ptr_cl(xc), hip.ptr(wb), hip.ptr(b), N, H, W, Cin, Cout, _ptr_cl(y), hip.stream()),
                  'psi_conv3x3_forward')
        ctx.save_for_backward(xc, wb, wt)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, wb, wt = ctx.saved_tensors
        N, Cin, H, W = xc.shape
        Cout = wb.shape[0]
        dyc = dy.contiguous(memory_format=torch.channels_last)
        L = hip.lib()
        dx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if L.psi_conv3x3_supported(Cout, Cin, H, W):
                if wt is None:
                    wt = torch.empty(Cin, 3, 3, Cout, device=dy.device, dtype=torch.bfloat16)
                    hip.check(L.psi_conv3x3_rotate_weight(hip.ptr(wb), Cin, Cout, hip.ptr(wt), hip.stream()), 'psi_conv3x3_rotate_weight')
                dx = torch.empty((N, Cin, H, W), device=dy.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
                hip.check(L.psi_conv3x3_forward(_ptr_cl(dyc), hip.ptr(wt), None, N, H, W, Cout, Cin, _ptr_cl(dx), hip.stream()),
                          'psi_conv3x3_forward (input gradient)')
            else:
                dx = torch.ops.aten.convolution_backward(dyc, xc, wb.permute(0, 3, 1, 2), None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                         (True, False, False))[0]
        if ctx.needs_input_grad[1]:
            nws = L.psi_conv3x3_wrw_workspace_floats(N, H, W, Cin, Cout)
            if nws:
                # hand-written split-K weight gradient (fp32, deterministic summation order)
                gw4 = torch.empty(Cout, 3, 3, Cin, device=dy.device, dtype=torch.float32)
                ws = torch.empty(nws, device=dy.device, dtype=torch.float32)
                hip.check(L.psi_conv3x3_weight_grad(_ptr_cl(xc), _ptr_cl(dyc), N, H, W, Cin, Cout, hip.ptr(gw4), hip.ptr(ws), hip.stream()),
                          'psi_conv3x3_weight_grad')
                gw = gw4.permute(0, 3, 1, 2)                         # [Cout,Cin,3,3] view (channels_last strides, like the parameter)
            else:
                gw = torch.ops.aten.convolution_backward(dyc, xc, wb.permute(0, 3, 1, 2), None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                         (False, True, False))[1].float()
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = dyc.float().sum((0, 2, 3))
        return dx, gw, gb


def conv3x3_supported(conv, x):
    """True when ``conv`` (an nn.Conv2d) applied to the bf16 CUDA map ``x`` is covered by the hand-written kernel."""
    return (x.is_cuda and x.dim() == 4 and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros'
            and bool(hip.lib().psi_conv3x3_supported(conv.in_channels, conv.out_channels, x.shape[2], x.shape[3])))


def conv3x3(x, conv):
    """``conv(x)`` for a 3x3 / stride 1 / padding 1 ``nn.Conv2d`` on a bf16 map: hand-written bf16-MFMA implicit GEMM, forward and input
    gradient (csrc/conv.hip); output bf16 channels_last."""
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    return _Conv3x3.apply(x, conv.weight, conv.bias)


# ------------------------------------------------------------------------------------------------------------------
# The scene encoders and dense layers at the REFERENCE'S PRECISION (fp32 models, cvae.py:427-455,474-492; net_layers.py:28-43,56-93) on
# hand-written kernels: fp32 NHWC maps, every product a three-term bf16 split with fp32 accumulation (csrc/conv_gemm.hip explains and
# quantifies it: 0.6-3.2e-5 of the reference's recorded forward passes, tests/golden/cvae.npz).  Forward: psi_conv2d_forward (ALL the
# convolutions: 7x7 stem, stride-1 / stride-2 3x3, 1x1 downsample, heads), psi_bn_forward_t (batch or running statistics, + ReLU + skip),
# psi_maxpool3x3s2_forward_t, psi_linear_forward3 (any width).  Backward: BatchNorm and max-pool on the same hand-written kernels, the
# convolutions' input and weight gradients on psi_conv2d_input_grad / psi_conv2d_weight_grad and the dense layers' on psi_linear_backward3
# (the same split products).
# ------------------------------------------------------------------------------------------------------------------
def conv2d_supported(conv):
    return (conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros' and conv.kernel_size[0] == conv.kernel_size[1]
            and conv.stride[0] == conv.stride[1] and conv.padding[0] == conv.padding[1]
            and bool(hip.lib().psi_conv2d_supported(conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.kernel_size[1], conv.stride[0],
                                                    conv.padding[0])))


def _conv2d_prepared_ok(Cin, Cout, KH, KW, stride, pad):
    """shapes whose weight is split / re-laid out ONCE per layer and step (psi_conv2d_prepare_weight) instead of in every workgroup"""
    return bool(hip.lib().psi_conv2d_prepared_ok(Cin, Cout, KH, KW, stride, pad))


def _conv2d_dgrad_covered(Cin, Cout, KH, KW):
    """shapes whose input gradient the general kernel takes in its transposed-gather form (psi_hip.h: psi_conv2d_input_grad)"""
    return Cin % 32 == 0 and (Cout % 64 == 0 or Cout * KH * KW <= 4096)


class _Conv2dSplit(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, nterm, out_bf16):
        N, Cin, H, W = x.shape
        Cout, _, KH, KW = weight.shape
        xc = x.contiguous(memory_format=torch.channels_last)
        w4 = weight.detach().permute(0, 2, 3, 1)                     # [Cout,KH,KW,Cin]: a view of a channels_last weight, else a copy
        w4 = (w4 if w4.is_contiguous() else w4.contiguous()).float()
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        y = torch.empty((N, Cout, OH, OW), device=x.device, dtype=torch.bfloat16 if out_bf16 else torch.float32, memory_format=torch.channels_last)
        b = bias.detach().float().contiguous() if bias is not None else None
        L = hip.lib()
        wt = None
        if _conv2d_prepared_ok(Cin, Cout, KH, KW, stride, pad):
            # the weight's bf16 parts once per layer and step, in the forward's layout and (when x needs a gradient) the input gradient's
            nel = Cout * KH * KW * Cin * (2 if nterm == 3 else 1)
            wf = torch.empty(nel, device=x.device, dtype=torch.bfloat16)
            if ctx.needs_input_grad[0] and _conv2d_dgrad_covered(Cin, Cout, KH, KW):
                wt = torch.empty(nel, device=x.device, dtype=torch.bfloat16)
            hip.check(L.psi_conv2d_prepare_weight(hip.ptr(w4), Cout, KH, KW, Cin, nterm, hip.ptr(wf), hip.ptr(wt), hip.stream()), 'psi_conv2d_prepare_weight')
            hip.check(L.psi_conv2d_forward_p(_ptr_cl(xc), int(xc.dtype == torch.bfloat16), hip.ptr(wf), hip.ptr(b), N, H, W, Cin, Cout, KH, KW, stride, pad,
                                             _ptr_cl(y), int(out_bf16), nterm, hip.stream()), 'psi_conv2d_forward_p')
        else:
            hip.check(L.psi_conv2d_forward(_ptr_cl(xc), int(xc.dtype == torch.bfloat16), hip.ptr(w4), hip.ptr(b), N, H, W, Cin, Cout, KH, KW,
                                           stride, pad, _ptr_cl(y), int(out_bf16), nterm, hip.stream()), 'psi_conv2d_forward')
        ctx.save_for_backward(xc, weight, wt)
        ctx.geom = (stride, pad, bias is not None, nterm)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, weight, wt_prepared = ctx.saved_tensors
        stride, pad, has_bias, nterm = ctx.geom
        N, Cin, H, W = xc.shape
        Cout, _, KH, KW = weight.shape
        dyc = dy.contiguous(memory_format=torch.channels_last)
        if dyc.dtype not in (torch.float32, torch.bfloat16):
            dyc = dyc.float()
        L = hip.lib()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if _conv2d_dgrad_covered(Cin, Cout, KH, KW):
                gx = torch.empty((N, Cin, H, W), device=dy.device, dtype=xc.dtype, memory_format=torch.channels_last)
                if wt_prepared is not None:
                    hip.check(L.psi_conv2d_input_grad_p(_ptr_cl(dyc), int(dyc.dtype == torch.bfloat16), hip.ptr(wt_prepared), N, H, W, Cin, Cout, KH, KW,
                                                        stride, pad, _ptr_cl(gx), int(gx.dtype == torch.bfloat16), nterm, hip.stream()),
                              'psi_conv2d_input_grad_p')
                else:
                    wt = weight.detach().float().permute(1, 2, 3, 0).contiguous()        # [Cin,KH,KW,Cout]
                    hip.check(L.psi_conv2d_input_grad(_ptr_cl(dyc), int(dyc.dtype == torch.bfloat16), hip.ptr(wt), N, H, W, Cin, Cout, KH, KW, stride,
                                                      pad, _ptr_cl(gx), int(gx.dtype == torch.bfloat16), nterm, hip.stream()), 'psi_conv2d_input_grad')
            else:
                gx = torch.ops.aten.convolution_backward(dyc.to(xc.dtype), xc, weight.detach().to(xc.dtype), None, (stride, stride), (pad, pad), (1, 1),
                                                         False, (0, 0), 1, (True, False, False))[0]
        if ctx.needs_input_grad[1]:
            gw4 = torch.empty(Cout, KH, KW, Cin, device=dy.device, dtype=torch.float32)
            ws = torch.empty(L.psi_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, KH, KW, stride, pad), device=dy.device, dtype=torch.float32)
            hip.check(L.psi_conv2d_weight_grad(_ptr_cl(xc), int(xc.dtype == torch.bfloat16), _ptr_cl(dyc), int(dyc.dtype == torch.bfloat16), N, H, W, Cin,
                                               Cout, KH, KW, stride, pad, hip.ptr(gw4), hip.ptr(ws), nterm, hip.stream()), 'psi_conv2d_weight_grad')
            gw = gw4.permute(0, 3, 1, 2)                             # [Cout,Cin,KH,KW] view with channels_last strides, like the parameter
        if has_bias and ctx.needs_input_grad[2]:
            gb = dyc.float().sum((0, 2, 3))
        return gx, gw, gb, None, None, None, None


def conv2d_split(x, conv, nterm=3, out_bf16=False):
    """``conv(x)`` for an ``nn.Conv2d`` on an fp32 (or bf16) channels_last map through the general implicit-GEMM kernel: nterm = 3 = the fp32
    model's precision (three-term split products), nterm = 1 = bf16 products."""
    return _Conv2dSplit.apply(x, conv.weight, conv.bias, conv.stride[0], conv.padding[0], nterm, out_bf16)


class _BNActT(Function):
    """y = act(batch_norm(x) (+ residual)) on NHWC maps of either type, batch statistics (training) or running statistics (eval)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        N, C, H, W = x.shape
        M = N * H * W
        f32 = x.dtype == torch.float32
        xc = x.contiguous(memory_format=torch.channels_last)
        rc = residual.contiguous(memory_format=torch.channels_last) if residual is not None else None
        y = torch.empty_like(xc, memory_format=torch.channels_last)
        evalm = not bn.training
        mean = torch.empty(C, device=x.device, dtype=torch.float32) if not evalm else None
        invstd = torch.empty(C, device=x.device, dtype=torch.float32) if not evalm else None
        L = hip.lib()
        ws = torch.empty(L.psi_bn_workspace_floats(M, C), device=x.device, dtype=torch.float32)
        track = bn.track_running_stats and bn.running_mean is not None
        hip.check(L.psi_bn_forward_t(_ptr_cl(xc), int(f32), _ptr_cl(rc), hip.ptr(weight), hip.ptr(bias),
                                     hip.ptr(bn.running_mean) if track else None, hip.ptr(bn.running_var) if track else None,
                                     hip.ptr(bn.num_batches_tracked) if (track and not evalm) else None, M, C, int(relu),
                                     float(bn.momentum if bn.momentum is not None else 0.1), float(bn.eps), _ptr_cl(y), hip.ptr(mean),
                                     hip.ptr(invstd), hip.ptr(ws), int(evalm), hip.stream()), 'psi_bn_forward_t')
        if evalm:
            # inference form: the gradient is that of an affine map with the running statistics (only needed if someone differentiates an
            # eval-mode model: kept correct through the saved statistics)
            mean, invstd = bn.running_mean.detach().float(), torch.rsqrt(bn.running_var.detach().float() + bn.eps)
        keep_y = relu and (evalm or residual is not None or not _bn_mask_from_x())
        ctx.save_for_backward(xc, y if keep_y else None, weight, bias, mean, invstd)
        ctx.relu, ctx.has_res, ctx.dims, ctx.evalm, ctx.f32 = bool(relu), residual is not None, (M, C), evalm, f32
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, y, weight, bias, mean, invstd = ctx.saved_tensors
        M, C = ctx.dims
        dyc = dy.contiguous(memory_format=torch.channels_last).to(xc.dtype)
        if ctx.evalm:
            dz = dyc if not ctx.relu else dyc * (y > 0).to(dyc.dtype)
            sc = (weight * invstd).view(1, C, 1, 1)
            xhat = (xc.float() - mean.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)
            return ((dz.float() * sc).to(xc.dtype), (dz.float() * xhat).sum((0, 2, 3)), dz.float().sum((0, 2, 3)),
                    dz if (ctx.has_res and ctx.needs_input_grad[3]) else None, None, None)
        dx = torch.empty_like(xc, memory_format=torch.channels_last)
        dres = torch.empty_like(xc, memory_format=torch.channels_last) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        dgamma = torch.empty(C, device=xc.device, dtype=torch.float32)
        dbeta = torch.empty(C, device=xc.device, dtype=torch.float32)
        L = hip.lib()
        ws = torch.empty(L.psi_bn_workspace_floats(M, C), device=xc.device, dtype=torch.float32)
        hip.check(L.psi_bn_backward_t(_ptr_cl(dyc), int(ctx.f32), _ptr_cl(xc), _ptr_cl(y), hip.ptr(weight), hip.ptr(bias.detach().float()), hip.ptr(mean),
                                      hip.ptr(invstd), M, C,
                                      int(ctx.relu), _ptr_cl(dx), _ptr_cl(dres), hip.ptr(dgamma), hip.ptr(dbeta), hip.ptr(ws), hip.stream()),
                  'psi_bn_backward_t')
        return dx, dgamma, dbeta, dres, None, None


def bn_act_t(x, bn, relu=True, residual=None):
    """``relu(bn(x) + residual)`` (each part optional) of an ``nn.BatchNorm2d`` in training OR eval mode on an fp32 or bf16 channels_last map."""
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda or x.dim() != 4:
        raise ValueError('bn_act_t: expected a 4-D fp32 / bf16 CUDA tensor')
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape):
        raise ValueError('bn_act_t: residual must match x')
    return _BNActT.apply(x, bn.weight, bn.bias, residual, bn, relu)


def bn_t_supported(bn):
    return (bn.affine and bn.track_running_stats and bn.running_mean is not None and (bn.momentum is not None or not bn.training)
            and bn.num_features in (8, 16, 32, 64, 128, 256))


class _MaxPoolT(Function):
    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        xc = x.contiguous(memory_format=torch.channels_last)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((N, C, OH, OW), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
        idx = torch.empty(N * OH * OW * C, device=x.device, dtype=torch.uint8) if ctx.needs_input_grad[0] else None
        hip.check(hip.lib().psi_maxpool3x3s2_forward_t(_ptr_cl(xc), int(x.dtype == torch.float32), N, H, W, C, _ptr_cl(y), hip.ptr(idx), hip.stream()),
                  'psi_maxpool3x3s2_forward_t')
        ctx.save_for_backward(idx)
        ctx.dims = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        N, C, H, W = ctx.dims
        dyc = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty((N, C, H, W), device=dy.device, dtype=dy.dtype, memory_format=torch.channels_last)
        hip.check(hip.lib().psi_maxpool3x3s2_backward_t(_ptr_cl(dyc), int(dy.dtype == torch.float32), hip.ptr(idx), N, H, W, C, _ptr_cl(dx), hip.stream()),
                  'psi_maxpool3x3s2_backward_t')
        return dx


def maxpool3x3s2_t(x):
    """``nn.MaxPool2d(3, 2, 1)`` on an fp32 or bf16 channels_last map."""
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda or x.dim() != 4 or x.shape[1] % 8:
        raise ValueError('maxpool3x3s2_t: expected a 4-D fp32 / bf16 CUDA tensor with a multiple of 8 channels')
    return _MaxPoolT.apply(x)


class _LinearAct3(Function):
    """nn.Linear (+ LeakyReLU, + skip connection) at the fp32 model's precision: ONE hand-written kernel forward (psi_linear_forward3: three-term
    split products, any width) and per gradient (psi_linear_backward3: dX, dW + dbias with the same products)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, act, slope):
        M, K = x.shape
        N = weight.shape[0]
        xc = x.detach().contiguous().float()
        w = weight.detach().contiguous().float()
        b = bias.detach().contiguous().float() if bias is not None else None
        r = residual.detach().contiguous().float() if residual is not None else None
        y = torch.empty(M, N, device=x.device)
        a_out = torch.empty(M, N, device=x.device) if (act and residual is not None) else None
        L = hip.lib()
        nws = L.psi_linear_workspace_floats(M, N, K)
        ws = torch.empty(nws, device=x.device) if nws else None
        hip.check(L.psi_linear_forward3(hip.ptr(xc), 0, hip.ptr(w), hip.ptr(b), hip.ptr(r), M, N, K, int(act), float(slope), hip.ptr(y), hip.ptr(a_out),
                                        hip.ptr(ws), hip.stream()), 'psi_linear_forward3')
        ctx.act, ctx.slope = int(act), float(slope)
        ctx.has_bias, ctx.has_res = bias is not None, residual is not None
        ctx.save_for_backward(xc, w, (a_out if a_out is not None else y) if act else torch.empty(0, device=x.device))
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, w, a_out = ctx.saved_tensors
        gy = gy.contiguous().float()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        M, K = xc.shape
        N = w.shape[0]
        gx = torch.empty(M, K, device=gy.device) if need_x else None
        gw = torch.empty(N, K, device=gy.device) if (need_w or need_b) else None         # gbias is produced by the dW kernel
        gb = torch.empty(N, device=gy.device) if need_b else None
        L = hip.lib()
        nws = L.psi_linear_backward_workspace_floats(M, N, K) if need_x else 0
        ws = torch.empty(nws, device=gy.device) if nws else None
        hip.check(L.psi_linear_backward3(hip.ptr(gy), hip.ptr(a_out) if ctx.act else None, hip.ptr(xc), hip.ptr(w), M, N, K, ctx.slope, hip.ptr(gx),
                                         hip.ptr(gw), hip.ptr(gb), hip.ptr(ws), hip.stream()), 'psi_linear_backward3')
        return gx, gw if need_w else None, gb, gy if (ctx.has_res and ctx.needs_input_grad[3]) else None, None, None


def linear_act3(x, weight, bias=None, act=None, slope=0.01, residual=None):
    """act(x @ weight.T + bias) (+ residual) at fp32 precision on the HIP kernels (any K, N); ``act`` is None or 'leaky_relu'."""
    if act not in (None, 'leaky_relu'):
        raise ValueError('act must be None or "leaky_relu"')
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError('linear_act3: x [M,K] and weight [N,K] expected, got %s / %s' % (tuple(x.shape), tuple(weight.shape)))
    return _LinearAct3.apply(x, weight, bias, residual, 1 if act else 0, slope)


# ------------------------------------------------------------------------------------------
# Body-vector glue of a CVAE training step (csrc/cvae_loss.hip): target representation, reconstruction / KL / VPoser losses
# ------------------------------------------------------------------------------------------
def _f32c(t):
    return None if t is None else t.detach().contiguous().float()


def cvae_target(xh, cam_int, max_d):
    """``GeometryTransformer.convert_to_6D_rot(GeometryTransformer.normalize_global_T(xh, cam_int, max_d))`` (cvae.py:118-127, 176-199) in
    one launch: [B,72] -> [B,75].  The training target of the CVAE; a function of the batch only (no gradient)."""
    B = xh.shape[0]
    if xh.dim() != 2 or xh.shape[1] != 72 or tuple(cam_int.shape) != (B, 3, 3) or max_d.numel() != B:
        raise ValueError('cvae_target: xh [B,72], cam_int [B,3,3], max_d [B] expected, got %s / %s / %s'
                         % (tuple(xh.shape), tuple(cam_int.shape), tuple(max_d.shape)))
    out = torch.empty(B, 75, device=xh.device)
    hip.check(hip.lib().psi_cvae_target(hip.ptr(_f32c(xh)), hip.ptr(_f32c(cam_int)), hip.ptr(_f32c(max_d)), B, hip.ptr(out), hip.stream()),
              'psi_cvae_target')
    return out


class _CvaeLosses(Function):
    @staticmethod
    def forward(ctx, rec, target, xh, cam_int, max_d, mu0, lv0, mu1, lv1, fca, w_rec, w_kl, w_vposer):
        B = rec.shape[0]
        if rec.dim() != 2 or rec.shape[1] != 75 or tuple(target.shape) != (B, 75) or tuple(xh.shape) != (B, 72):
            raise ValueError('cvae_losses: rec / target [B,75] and xh [B,72] expected, got %s / %s / %s'
                             % (tuple(rec.shape), tuple(target.shape), tuple(xh.shape)))
        t = [_f32c(v) for v in (rec, target, xh, cam_int, max_d, mu0, lv0, mu1, lv1)]
        fca_t = fca if torch.is_tensor(fca) else None
        ctx.fca = 0.0 if fca_t is not None else float(fca)
        ctx.w = (float(w_rec), float(w_kl), float(w_vposer))
        ctx.nz = (0 if mu0 is None else mu0.shape[1], 0 if mu1 is None else mu1.shape[1])
        xh_rec = torch.empty(B, 75, device=rec.device)
        losses = torch.empty(5, device=rec.device)
        ws = torch.empty(hip.lib().psi_cvae_losses_workspace_floats(), device=rec.device)
        hip.check(hip.lib().psi_cvae_losses_forward(*[hip.ptr(v) for v in t[:7]], ctx.nz[0], hip.ptr(t[7]), hip.ptr(t[8]), ctx.nz[1], B,
                                                    *ctx.w, ctx.fca, hip.ptr(_f32c(fca_t)), hip.ptr(ws), hip.ptr(xh_rec), hip.ptr(losses),
                                                    hip.stream()),
                  'psi_cvae_losses_forward')
        ctx.has = (mu0 is not None, mu1 is not None)
        ctx.dtypes = tuple(None if v is None else v.dtype for v in (rec, mu0, lv0, mu1, lv1))
        ctx.fca_t = _f32c(fca_t)
        ctx.save_for_backward(*[v for v in t if v is not None], xh_rec)
        return xh_rec, losses

    @staticmethod
    def backward(ctx, g_xh_rec, g_losses):
        saved = list(ctx.saved_tensors)
        xh_rec = saved.pop()
        rec, target, xh, cam_int, max_d = saved[:5]
        rest = saved[5:]
        mu0, lv0 = (rest[0], rest[1]) if ctx.has[0] else (None, None)
        mu1, lv1 = (rest[-2], rest[-1]) if ctx.has[1] else (None, None)
        B = rec.shape[0]
        dev = rec.device
        gl = _f32c(g_losses) if g_losses is not None else torch.zeros(5, device=dev)
        g_rec = torch.empty_like(rec)
        g = [torch.empty_like(v) if v is not None else None for v in (mu0, lv0, mu1, lv1)]
        hip.check(hip.lib().psi_cvae_losses_backward(hip.ptr(rec), hip.ptr(target), hip.ptr(xh), hip.ptr(cam_int), hip.ptr(max_d), hip.ptr(mu0),
                                                     hip.ptr(lv0), ctx.nz[0], hip.ptr(mu1), hip.ptr(lv1), ctx.nz[1], B, *ctx.w, ctx.fca,
                                                     hip.ptr(ctx.fca_t), hip.ptr(xh_rec), hip.ptr(gl), hip.ptr(_f32c(g_xh_rec)), hip.ptr(g_rec),
                                                     hip.ptr(g[0]), hip.ptr(g[1]), hip.ptr(g[2]), hip.ptr(g[3]), hip.stream()),
                  'psi_cvae_losses_backward')
        cast = lambda v, dt: v if (v is None or v.dtype == dt) else v.to(dt)            # gradients in the dtype of their inputs
        dt = ctx.dtypes
        return (cast(g_rec, dt[0]), None, None, None, None, cast(g[0], dt[1]), cast(g[1], dt[2]), cast(g[2], dt[3]), cast(g[3], dt[4]),
                None, None, None, None)


def cvae_losses(rec, target, xh, cam_int, max_d, mu0, logvar0, mu1=None, logvar1=None, fca=1.0, w_rec=1.0, w_kl=1.0, w_vposer=1.0):
    """The body-vector losses of ``cal_loss`` (train_s1.py:113-133, train_s2.py:119-139) in one launch per direction.

    rec = xhnr_rec [B,75] (the CVAE's reconstruction, 6D global rotation), target = cvae_target(xh, ...), xh [B,72] the ground truth.
    -> xh_rec [B,75] = recover_global_T(rec, cam_int, max_d) and losses [5] = (rec_t, rec_p, KL of latent 0, KL of latent 1 (0 without
    one), vposer).  ``fca``: the KL annealing factor, a float or a 0-dim device tensor (captured steps change it between replays)."""
    return _CvaeLosses.apply(rec, target, xh, cam_int, max_d, mu0, logvar0, mu1, logvar1, fca, w_rec, w_kl, w_vposer)


# ------------------------------------------------------------------------------------------
# Contact + penetration losses of a training step from the body mesh (csrc/scene_loss.hip)
# ------------------------------------------------------------------------------------------
_CHAIN_CACHE = {}


_VID32_CACHE = {}


def _vid32_of(vid):
    """int32 copy of a contact-id tensor, cached per tensor (storage, length, version): a caller that passes no ``vid32`` gets the SAME int32
    tensor on every call, so the chain below is built once for it as well (it was rebuilt on every call: every cast was a new cache key)."""
    key = (vid.data_ptr(), vid.numel(), vid._version, vid.device)
    hit = _VID32_CACHE.get(key)
    if hit is None:
        if len(_VID32_CACHE) > 64:
            _VID32_CACHE.clear()
        hit = _VID32_CACHE[key] = (vid, vid.to(torch.int32))     # keeps the int64 tensor alive: its address cannot be reused while cached
    return hit[1]


def _contact_chain(vid32):
    """psi_contact_slot_chain of a contact-id tensor, cached per tensor (the ids are a constant of the model; the cache is keyed by storage
    and version, so an id list that is modified in place gets a new chain)."""
    key = (vid32.data_ptr(), vid32.numel(), vid32._version, vid32.device)
    hit = _CHAIN_CACHE.get(key)
    if hit is None:
        chain = torch.empty(2 * vid32.numel(), dtype=torch.int32, device=vid32.device)
        hip.check(hip.lib().psi_contact_slot_chain(hip.ptr(vid32), vid32.numel(), hip.ptr(chain), hip.stream()), 'psi_contact_slot_chain')
        if len(_CHAIN_CACHE) > 64:
            _CHAIN_CACHE.clear()
        hit = _CHAIN_CACHE[key] = (vid32, chain)             # keeps the id tensor alive: its address cannot be reused while cached
    return hit[1]


class _SceneLosses(Function):
    @staticmethod
    def forward(ctx, verts, vid, scenes, slot, sdf, gmin, gmax, align_corners, w_contact, w_collision, gate, vid32):
        ctx.verts_dtype = verts.dtype
        verts = verts.detach().contiguous().float()
        B, V, _ = verts.shape
        L = hip.lib()
        xyz1 = verts.index_select(1, vid)                                   # [B,n_c,3] contact vertices (train_s1.py:161)
        n_c = xyz1.shape[1]
        dist, idx = scenes.query(xyz1, slot)                                # exact body->scene NN (chamfer dist1 / idx1)
        S, D = sdf.shape[0], sdf.shape[1]
        vals = torch.empty(B, V, device=verts.device)
        og = torch.empty(B, V, 3, device=verts.device)
        hip.check(L.psi_sdf_sample_forward(hip.ptr(sdf), hip.ptr(slot), hip.ptr(gmin), hip.ptr(gmax), hip.ptr(verts), B, V, D, S,
                                           int(bool(align_corners)), hip.ptr(vals), hip.ptr(og), hip.stream()), 'psi_sdf_sample_forward')
        ws = torch.empty(L.psi_scene_losses_workspace_floats(), device=verts.device)
        losses = torch.empty(2, device=verts.device)
        stats = torch.empty(2, device=verts.device)
        ctx.w = (float(w_contact), float(w_collision), float(gate))
        hip.check(L.psi_scene_losses_forward(hip.ptr(dist), B * n_c, hip.ptr(vals), B * V, *ctx.w, hip.ptr(ws), hip.ptr(losses), hip.ptr(stats),
                                             hip.stream()), 'psi_scene_losses_forward')
        ctx.scenes = scenes
        ctx.save_for_backward(dist, xyz1, idx, slot, vid32 if vid32 is not None else _vid32_of(vid), vals, og, stats)
        return losses

    @staticmethod
    def backward(ctx, g):
        dist, xyz1, idx, slot, vid32, vals, og, stats = ctx.saved_tensors
        B, V = vals.shape
        table = ctx.scenes.verts_table
        g_verts = torch.empty(B, V, 3, device=vals.device)
        chain = _contact_chain(vid32)                       # slots of a repeated contact vertex, chained in slot order (built once per id list)
        hip.check(hip.lib().psi_scene_losses_backward(hip.ptr(g.contiguous().float()), hip.ptr(stats), hip.ptr(dist), hip.ptr(xyz1), hip.ptr(idx),
                                                      hip.ptr(slot), hip.ptr(table), table.shape[1], hip.ptr(vid32), hip.ptr(vals), hip.ptr(og), B,
                                                      V, xyz1.shape[1], *ctx.w, hip.ptr(chain), hip.ptr(g_verts), hip.stream()),
                  'psi_scene_losses_backward')
        return (g_verts if ctx.verts_dtype == g_verts.dtype else g_verts.to(ctx.verts_dtype),) + (None,) * 11


def scene_losses(body_verts, vid, scenes: SceneSet, slot, sdf, grid_min, grid_max, align_corners, w_contact, w_collision, gate=1.0, vid32=None):
    """(loss_contact, loss_sdf_pene) of ``cal_loss`` (train_s1.py:156-204) from the camera-frame body mesh [B,V,3]: the contact rows ``vid``
    against each body's scene (``scenes`` / ``slot`` as in chamfer_to_scenes), every vertex against its scene's SDF volume (sdf [S,D,D,D],
    grid_min / grid_max [S,3], the same ``slot``).  Two exact-NN / SDF kernels and two small reduction kernels forward, two kernels
    backward — the operator form of the same expressions is chamfer_to_scenes + sdf_sample + penetration_loss plus ~40 elementwise launches.
    ``vid``: int64 [n_c] device; ``vid32``: the same as int32 when the caller keeps one (saves a cast launch per step)."""
    assert slot.dtype == torch.int32 and slot.is_contiguous()
    out = _SceneLosses.apply(body_verts, vid, scenes, slot, sdf.contiguous().float(), grid_min.reshape(-1, 3).contiguous().float(),
                             grid_max.reshape(-1, 3).contiguous().float(), align_corners, w_contact, w_collision, gate, vid32)
    return out[0], out[1]


# ------------------------------------------------------------------------------------------
# Scene snapshots (psi_raster_*)
# ------------------------------------------------------------------------------------------
def raster_mesh_create(verts, faces, vertex_labels=None):
    """Upload-side half of ``rendering.SceneMesh``: verts [nv,3] fp32, faces [nf,3] int32, vertex_labels [nv] fp32 or None, all on the GPU.
    Returns the ``psi_raster_mesh`` handle, a ``hip.Handle``: freed by ``raster_mesh_destroy`` or when its last holder lets go of it."""
    import ctypes
    if verts.dtype != torch.float32 or faces.dtype != torch.int32 or verts.dim() != 2 or faces.dim() != 2 or verts.shape[1] != 3 or faces.shape[1] != 3:
        raise ValueError('expected verts [nv,3] float32 and faces [nf,3] int32')
    if vertex_labels is not None and (vertex_labels.dtype != torch.float32 or vertex_labels.shape != (verts.shape[0],)):
        raise ValueError('expected vertex_labels [nv] float32')
    h = hip.Handle('psi_raster_mesh_destroy')
    pv, pf, pl = hip.ptr(verts), hip.ptr(faces), hip.ptr(vertex_labels)
    with torch.cuda.device(verts.device):
        hip.check(hip.lib().psi_raster_mesh_create(ctypes.byref(h), pv, pf, pl, verts.shape[0], faces.shape[0]), 'psi_raster_mesh_create')
    return h


def _destroy(handle, symbol):
    """``close()`` of a ``hip.Handle``; any other ``c_void_p`` is a handle its caller owns and frees here, through the library's ``symbol``."""
    if isinstance(handle, hip.Handle):
        handle.close()
    elif handle:
        getattr(hip.lib(), symbol)(handle)


def raster_mesh_destroy(handle):
    _destroy(handle, 'psi_raster_mesh_destroy')


def _check_views(w2c, intr, size):
    """n, H, W and the device of w2c [n,3,4] / intr [n,4] fp32 and size = (H, W)."""
    if w2c.dtype != torch.float32 or intr.dtype != torch.float32 or w2c.dim() != 3 or tuple(w2c.shape[1:]) != (3, 4) or tuple(intr.shape) != (w2c.shape[0], 4):
        raise ValueError('expected w2c [n,3,4] and intr [n,4], float32')
    return w2c.shape[0], int(size[0]), int(size[1]), w2c.device


def raster_render(handle, nf, w2c, intr, size, near=0.05, with_seg=True):
    """All views of one call through the tile-binned rasteriser (include/psi_hip.h: psi_raster_render).

    w2c [n,3,4] fp32 world-to-camera rows, intr [n,4] fp32 = fx, fy, cx, cy, size = (H, W).  Returns depth [n,H,W] fp32 (0 = no hit),
    tri [n,H,W] int32 (-1 = no hit), seg [n,H,W] fp32 or None, stats [n,2] int32 (binned pairs, pieces dropped by the 2^28 guard)."""
    pw, pi = hip.ptr(w2c), hip.ptr(intr)
    n, H, W, dev = _check_views(w2c, intr, size)
    depth = torch.empty(n, H, W, device=dev)
    tri = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    seg = torch.empty(n, H, W, device=dev) if with_seg else None
    stats = torch.empty(n, 2, dtype=torch.int32, device=dev)
    L = hip.lib()
    ws = torch.empty(max(L.psi_raster_workspace_bytes(nf, n, W, H), 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        hip.check(L.psi_raster_render(handle, pw, pi, n, W, H, float(near), hip.ptr(depth), hip.ptr(tri), hip.ptr(seg), hip.ptr(stats),
                                      hip.ptr(ws), hip.stream()), 'psi_raster_render')
    return depth, tri, seg, stats


# ------------------------------------------------------------------------------------------
# Result images (psi_raster_bodies_*)
# ------------------------------------------------------------------------------------------
def raster_bodies_create(faces, V):
    """faces [F,3] int32 on the GPU, the one topology of every body; V vertices per body.  Returns the ``psi_raster_bodies`` handle, a
    ``hip.Handle`` (``raster_bodies_destroy``, or its last holder letting go, frees it); a face index outside [0, V) is refused."""
    import ctypes
    pf = hip.ptr(faces)
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('expected faces [F,3] int32')
    h = hip.Handle('psi_raster_bodies_destroy')
    with torch.cuda.device(faces.device):
        hip.check(hip.lib().psi_raster_bodies_create(ctypes.byref(h), pf, int(V), faces.shape[0]), 'psi_raster_bodies_create')
    return h


def raster_bodies_destroy(handle):
    _destroy(handle, 'psi_raster_bodies_destroy')


def _body_verts_ptr(bverts, V):
    p = hip.ptr(bverts)
    if bverts.dtype != torch.float32 or bverts.dim() != 3 or tuple(bverts.shape[1:]) != (V, 3):
        raise ValueError('expected body vertices [B,%d,3] float32' % V)
    return p


def raster_bodies_normals(handle, V, bverts):
    """Unnormalised vertex normals [B,V,3] of bverts [B,V,3]: the faces' cross products summed in ascending face index."""
    pv = _body_verts_ptr(bverts, V)
    out = torch.empty_like(bverts)
    with torch.cuda.device(bverts.device):
        hip.check(hip.lib().psi_raster_bodies_normals(handle, pv, bverts.shape[0], hip.ptr(out), hip.stream()), 'psi_raster_bodies_normals')
    return out


def raster_bodies_workspace_bytes(F, draws_per_pass, n_views, W, H):
    """Bytes of the workspace of ``raster_bodies_render``; ``ValueError`` for arguments the render call refuses (draws_per_pass * F >= 2^30,
    an image beyond 4096 pixels, ...)."""
    if min(F, draws_per_pass, n_views, W, H) < 1 or max(F, draws_per_pass, n_views, W, H) >= 2 ** 31:
        raise ValueError('F, draws_per_pass, n_views, W and H must be positive 32-bit integers')
    n = hip.lib().psi_raster_bodies_workspace_bytes(int(F), int(draws_per_pass), int(n_views), int(W), int(H))
    if n == 0:
        raise ValueError('no workspace for F=%d, draws_per_pass=%d, n_views=%d, W=%d, H=%d: draws_per_pass * F must stay below 2^30, n_views '
                         'at most 65535 and the image within 4096 x 4096' % (F, draws_per_pass, n_views, W, H))
    return n


def raster_bodies_render(bodies, V, F, bverts, draw_body, draw_view, draw_rgb, w2c, intr, size, near, background, draws_per_pass,
                         scene=None, vrgb=None, sdepth=None, stri=None):
    """Bodies composited into scene snapshots (include/psi_hip.h: psi_raster_bodies_render).  bverts [B,V,3] fp32; draw_body, draw_view [M]
    int32; draw_rgb [M,3] fp32; w2c / intr / size as ``raster_render``; scene, sdepth, stri: the ``psi_raster_mesh`` handle and the depth /
    tri images of its ``raster_render`` with the same views, or None.  Returns rgb [n,H,W,3] uint8, depth, draw (int32), body_depth,
    body_id (int32) [n,H,W], counts [M,2] int32, stats [n,2] int32."""
    pv = _body_verts_ptr(bverts, V)
    pw, pi = hip.ptr(w2c), hip.ptr(intr)
    n, H, W, dev = _check_views(w2c, intr, size)
    M = draw_body.shape[0]
    if draw_body.dtype != torch.int32 or draw_view.dtype != torch.int32 or draw_rgb.dtype != torch.float32 or tuple(draw_view.shape) != (M,) \
            or tuple(draw_rgb.shape) != (M, 3) or draw_body.dim() != 1:
        raise ValueError('expected draw_body, draw_view [M] int32 and draw_rgb [M,3] float32')
    if M * F >= 2 ** 31:
        raise ValueError('M * F = %d: the piece index d * F + face must stay below 2^31' % (M * F))
    if scene is not None and (tuple(sdepth.shape) != (n, H, W) or tuple(stri.shape) != (n, H, W) or sdepth.dtype != torch.float32
                              or stri.dtype != torch.int32):
        raise ValueError("expected the scene's depth (float32) and tri (int32) images [n,H,W] of the same views")
    ws = torch.empty(raster_bodies_workspace_bytes(F, draws_per_pass, n, W, H), dtype=torch.uint8, device=dev)
    rgb = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    depth, bdepth = torch.empty(n, H, W, device=dev), torch.empty(n, H, W, device=dev)
    draw, bid = torch.empty(n, H, W, dtype=torch.int32, device=dev), torch.empty(n, H, W, dtype=torch.int32, device=dev)
    counts = torch.zeros(M, 2, dtype=torch.int32, device=dev)
    stats = torch.empty(n, 2, dtype=torch.int32, device=dev)
    bg = [float(c) for c in background]
    args = [hip.ptr(t) if t is not None else None for t in (vrgb, sdepth, stri)] if scene is not None else [None] * 3
    with torch.cuda.device(dev):
        hip.check(hip.lib().psi_raster_bodies_render(scene, args[0], bodies, pv, bverts.shape[0], hip.ptr(draw_body), hip.ptr(draw_view),
                                                     hip.ptr(draw_rgb), M, pw, pi, n, W, H, float(near), args[1], args[2], bg[0], bg[1], bg[2],
                                                     int(draws_per_pass), hip.ptr(rgb), hip.ptr(depth), hip.ptr(draw), hip.ptr(bdepth), hip.ptr(bid),
                                                     hip.ptr(counts), hip.ptr(stats), hip.ptr(ws), hip.stream()), 'psi_raster_bodies_render')
    return rgb, depth, draw, bdepth, bid, counts, stats


# ------------------------------------------------------------------------------------------
# Mesh -> signed distance volume (psi_mesh_sdf_*)
# ------------------------------------------------------------------------------------------
def mesh_sdf_create(verts, faces):
    """Upload-side half of ``scene_sdf.MeshSDF``: verts [nv,3] fp32 and faces [nf,3] int32 on the GPU.  Returns the ``psi_mesh_sdf`` handle,
    a ``hip.Handle`` (``mesh_sdf_destroy``, or its last holder letting go, frees it); a face index out of range, a non-finite vertex or a mesh of degenerate triangles only is refused."""
    import ctypes
    pv, pf = hip.ptr(verts), hip.ptr(faces)
    if verts.dtype != torch.float32 or faces.dtype != torch.int32 or verts.dim() != 2 or faces.dim() != 2 or verts.shape[1] != 3 or faces.shape[1] != 3:
        raise ValueError('expected verts [nv,3] float32 and faces [nf,3] int32')
    h = hip.Handle('psi_mesh_sdf_destroy')
    with torch.cuda.device(verts.device):
        hip.check(hip.lib().psi_mesh_sdf_create(ctypes.byref(h), pv, pf, verts.shape[0], faces.shape[0]), 'psi_mesh_sdf_create')
    return h


def mesh_sdf_destroy(handle):
    _destroy(handle, 'psi_mesh_sdf_destroy')


def mesh_sdf_info(handle):
    """(kept triangles, dropped degenerate triangles, welded vertices, edges not shared by exactly two triangles)."""
    import ctypes
    info = (ctypes.c_int32 * 4)()
    hip.check(hip.lib().psi_mesh_sdf_info(handle, info), 'psi_mesh_sdf_info')
    return tuple(int(x) for x in info)


def _mesh_sdf_bounds(grid_min, grid_max):
    import ctypes
    import numpy as np
    lo, hi = (np.asarray(a, dtype=np.float32).reshape(3) for a in (grid_min, grid_max))
    return (ctypes.c_float * 3)(*lo.tolist()), (ctypes.c_float * 3)(*hi.tolist())


def mesh_sdf_compute(handle, grid_min, grid_max, dim, mode=0, device='cuda'):
    """The volume [D,D,D] fp32, element [ix][iy][iz], of the mesh behind ``handle`` on the node grid grid_min .. grid_max (host values).
    mode 0: pruned search; 1: every node against every triangle (the same bits)."""
    lo, hi = _mesh_sdf_bounds(grid_min, grid_max)
    dim = int(dim)
    if dim < 2 or dim > 1024:
        raise hip.PsiHipError('psi_mesh_sdf_compute: 2 <= D <= 1024 (got %d)' % dim)
    out = torch.empty(dim, dim, dim, device=device)
    with torch.cuda.device(out.device):
        hip.check(hip.lib().psi_mesh_sdf_compute(handle, lo, hi, dim, int(mode), hip.ptr(out), hip.stream()), 'psi_mesh_sdf_compute')
    return out


def mesh_sdf_count_pairs(handle, grid_min, grid_max, dim, mode=0, device='cuda'):
    """Number of (node, triangle) tests the search of ``mesh_sdf_compute`` executes, from the counting build of the kernel."""
    lo, hi = _mesh_sdf_bounds(grid_min, grid_max)
    n = torch.zeros(1, dtype=torch.int64, device=device)
    with torch.cuda.device(n.device):
        hip.check(hip.lib().psi_mesh_sdf_count_pairs(handle, lo, hi, int(dim), int(mode), hip.ptr(n), hip.stream()), 'psi_mesh_sdf_count_pairs')
    return int(n.item())


# ------------------------------------------------------------------------------------------
# Generalised winding number of the same mesh (psi_mesh_winding_*, psi_mesh_sdf_apply_sign)
# ------------------------------------------------------------------------------------------
def _mesh_winding_args(dim, beta, cluster):
    import math
    dim, beta, cluster = int(dim), float(beta), int(cluster)
    if dim < 2 or dim > 1024:
        raise hip.PsiHipError('psi_mesh_winding: 2 <= D <= 1024 (got %d)' % dim)
    if not math.isfinite(beta) or beta < 0:
        raise hip.PsiHipError('psi_mesh_winding: beta is finite and not negative (got %r)' % beta)
    if cluster < 8 or cluster > 256:
        raise hip.PsiHipError('psi_mesh_winding: 8 <= cluster <= 256 (got %d)' % cluster)
    return dim, beta, cluster


def mesh_winding_compute(handle, grid_min, grid_max, dim, beta=3.0, cluster=64, device='cuda'):
    """The free-space winding number f [D,D,D] fp32, element [ix][iy][iz], of the mesh behind ``handle`` on the nodes of
    ``mesh_sdf_compute``: 1 in the free space of a closed room, 0 in furniture and outside.  ``beta`` = 0: every node against every
    triangle; ``beta`` > 0: clusters of ``cluster`` triangles farther than beta x their radius from a brick of nodes count as dipoles."""
    lo, hi = _mesh_sdf_bounds(grid_min, grid_max)
    dim, beta, cluster = _mesh_winding_args(dim, beta, cluster)
    out = torch.empty(dim, dim, dim, device=device)
    with torch.cuda.device(out.device):
        hip.check(hip.lib().psi_mesh_winding_compute(handle, lo, hi, dim, beta, cluster, hip.ptr(out), hip.stream()), 'psi_mesh_winding_compute')
    return out


def mesh_winding_count(handle, grid_min, grid_max, dim, beta=3.0, cluster=64, device='cuda'):
    """(exact (node, triangle) tests, (node, dipole) tests) that ``mesh_winding_compute`` executes, from the counting build of the kernel."""
    lo, hi = _mesh_sdf_bounds(grid_min, grid_max)
    dim, beta, cluster = _mesh_winding_args(dim, beta, cluster)
    n = torch.zeros(2, dtype=torch.int64, device=device)
    with torch.cuda.device(n.device):
        hip.check(hip.lib().psi_mesh_winding_count(handle, lo, hi, dim, beta, cluster, hip.ptr(n), hip.stream()), 'psi_mesh_winding_count')
    return tuple(int(x) for x in n.tolist())


def mesh_sdf_apply_sign(f, level, vol):
    """In place: vol = -|vol| where f < level, |vol| elsewhere (f and vol fp32 on the GPU, the same number of elements).  Returns vol."""
    pf, pv = hip.ptr(f), hip.ptr(vol)
    if f.dtype != torch.float32 or vol.dtype != torch.float32 or f.numel() != vol.numel() or f.numel() == 0:
        raise ValueError('expected f and vol float32 with the same, non-zero number of elements')
    with torch.cuda.device(vol.device):
        hip.check(hip.lib().psi_mesh_sdf_apply_sign(pf, float(level), pv, vol.numel(), hip.stream()), 'psi_mesh_sdf_apply_sign')
    return vol


# ------------------------------------------------------------------------------------------
# Training records (psi_snapshot_canvas)
# ------------------------------------------------------------------------------------------
CANVAS_CLIP_DEPTH, CANVAS_CLIP_SEG = 6.0, 41.0


def snapshot_canvas(depth, seg, size=(128, 128), windows=None, target_z=None):
    """The CVAE's input images of n rendered views in one call (include/psi_hip.h: psi_snapshot_canvas).

    depth, seg [n,H,W] fp32 on the GPU, as ``rendering.SnapshotRenderer.render`` returns them (only read); size = (th, tw), both even;
    windows [n,4] int32 = x0, y0, x1, y1 and target_z [n] fp32 (GPU tensors, or anything ``torch.as_tensor`` takes) come together or not at
    all.  Returns depth_canvas, seg_canvas [n,1,th,tw], max_d, seg_max [n] fp32 and usable [n] int32."""
    pd, ps = hip.ptr(depth), hip.ptr(seg)
    if depth.dtype != torch.float32 or seg.dtype != torch.float32 or depth.dim() != 3 or depth.shape != seg.shape or depth.device != seg.device:
        raise ValueError('expected depth and seg [n,H,W] float32 of the same shape on the same device')
    if (windows is None) != (target_z is None):
        raise ValueError('windows and target_z come together')
    n, H, W = depth.shape
    th, tw = int(size[0]), int(size[1])
    dev = depth.device
    dc, sc = torch.empty(n, 1, th, tw, device=dev), torch.empty(n, 1, th, tw, device=dev)
    max_d, seg_max = torch.empty(n, device=dev), torch.empty(n, device=dev)
    usable = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return dc, sc, max_d, seg_max, usable
    if windows is not None:
        windows = torch.as_tensor(windows, dtype=torch.int32).to(dev).contiguous()
        target_z = torch.as_tensor(target_z, dtype=torch.float32).to(dev).contiguous()
        if tuple(windows.shape) != (n, 4) or tuple(target_z.shape) != (n,):
            raise ValueError('expected windows [n,4] and target_z [n]')
    L = hip.lib()
    ws = torch.empty(max(L.psi_snapshot_canvas_workspace_bytes(n), 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        hip.check(L.psi_snapshot_canvas(pd, ps, n, H, W, th, tw, CANVAS_CLIP_DEPTH, CANVAS_CLIP_SEG, hip.ptr(windows), hip.ptr(target_z),
                                        hip.ptr(dc), hip.ptr(sc), hip.ptr(max_d), hip.ptr(seg_max), hip.ptr(usable), hip.ptr(ws), hip.stream()),
                  'psi_snapshot_canvas')
    return dc, sc, max_d, seg_max, usable


# ------------------------------------------------------------------------------------------
# Scene contact cloud: even surface samples of a mesh (psi_mesh_cloud_*)
# ------------------------------------------------------------------------------------------
MESH_CLOUD_MAX_CANDIDATES = 2 ** 31 - 1


def mesh_cloud(verts, faces, spacing, out=None, return_counts=False):
    """Points on the surface of a mesh, about one per ``spacing`` cell whatever the tessellation (include/psi_hip.h: psi_mesh_cloud_*;
    DESIGN.md section 10b).  verts [nv,3] fp32 and faces [nf,3] int32 on the GPU, the caller's own (unwelded) mesh.  Returns points [m,3]
    fp32 and tri [m] int32 (the caller's face index of every point) on the GPU, in ascending candidate number; with ``return_counts``
    also (candidates, rows).  ``out`` = (points [cap,3] fp32, tri [cap] int32) receives the result in its first m rows (the returned tensors
    are views of them); nothing is written to them when the call is refused.

    The five kernels run on the current stream; the scans (``torch.cumsum``, int64) and the stable sort of the cell indices between them
    are plumbing, and two values are read back: the verdict and the totals of the count pass, and the number of kept points.
    ``PsiHipError`` (PSI_EINVAL) for what the library refuses; ``ValueError`` when the mesh has more than 2^31 - 1 candidates at this
    spacing."""
    import ctypes
    import math
    pv, pf = hip.ptr(verts), hip.ptr(faces)
    if verts.dtype != torch.float32 or faces.dtype != torch.int32 or verts.dim() != 2 or faces.dim() != 2 or verts.shape[1] != 3 or faces.shape[1] != 3:
        raise ValueError('expected verts [nv,3] float32 and faces [nf,3] int32')
    if verts.device != faces.device:
        raise ValueError('verts and faces lie on different devices')
    spacing = float(spacing)
    if not math.isfinite(spacing) or spacing <= 0:
        raise hip.PsiHipError('psi_mesh_cloud: spacing is finite and positive (got %r)' % spacing)
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    if nf < 1 or nv < 1:
        raise hip.PsiHipError('psi_mesh_cloud: nf >= 1 and nv >= 1')
    dev = verts.device
    if out is not None:
        out_p, out_t = out
        hip.ptr(out_p), hip.ptr(out_t)
        if out_p.dtype != torch.float32 or out_t.dtype != torch.int32 or out_p.dim() != 2 or out_p.shape[1] != 3 or out_t.dim() != 1 \
                or out_p.shape[0] != out_t.shape[0] or out_p.device != dev or out_t.device != dev:
            raise ValueError('expected out = (points [cap,3] float32, tri [cap] int32) on the device of the mesh')
    L = hip.lib()
    with torch.cuda.device(dev):
        st = hip.stream()
        tri_rows = torch.empty(nf, dtype=torch.int32, device=dev)
        origin = (ctypes.c_float * 3)()
        n_rows, n_cands = ctypes.c_longlong(0), ctypes.c_longlong(0)
        rc = L.psi_mesh_cloud_count(pv, pf, nv, nf, spacing, hip.ptr(tri_rows), origin, ctypes.byref(n_rows), ctypes.byref(n_cands), st)
        if rc != 0 and n_cands.value > MESH_CLOUD_MAX_CANDIDATES:
            raise ValueError('the mesh has %d candidates at spacing %g: more than 2^31 - 1 (use a larger spacing)' % (n_cands.value, spacing))
        hip.check(rc, 'psi_mesh_cloud_count')
        n_rows, n_cands = n_rows.value, n_cands.value
        tri_row_inc = torch.cumsum(tri_rows, 0, dtype=torch.int64)
        tri_row_off = tri_row_inc - tri_rows
        row_tri = torch.empty(n_rows, dtype=torch.int32, device=dev)
        row_cnt = torch.empty(n_rows, dtype=torch.int32, device=dev)
        hip.check(L.psi_mesh_cloud_rows(pv, pf, nv, nf, spacing, hip.ptr(tri_row_off), n_rows, hip.ptr(row_tri), hip.ptr(row_cnt), st),
                  'psi_mesh_cloud_rows')
        row_off = torch.cumsum(row_cnt, 0, dtype=torch.int64) - row_cnt
        pos = torch.empty(n_cands, 3, dtype=torch.float32, device=dev)
        tri = torch.empty(n_cands, dtype=torch.int32, device=dev)
        cell = torch.empty(n_cands, dtype=torch.int64, device=dev)
        key = torch.empty(n_cands, dtype=torch.int32, device=dev)
        hip.check(L.psi_mesh_cloud_emit(pv, pf, nv, nf, spacing, origin, hip.ptr(tri_row_off), hip.ptr(row_tri), hip.ptr(row_off), n_rows, n_cands,
                                        hip.ptr(pos), hip.ptr(tri), hip.ptr(cell), hip.ptr(key), st), 'psi_mesh_cloud_emit')
        cell_sorted, perm = torch.sort(cell, stable=True)
        keep = torch.empty(n_cands, dtype=torch.int32, device=dev)
        hip.check(L.psi_mesh_cloud_winners(hip.ptr(cell_sorted), hip.ptr(perm), hip.ptr(key), n_cands, hip.ptr(keep), st), 'psi_mesh_cloud_winners')
        keep_scan = torch.cumsum(keep, 0, dtype=torch.int64)
        m = int(keep_scan[-1].item())
        if m < 1:
            raise hip.PsiHipError('psi_mesh_cloud_winners marked no candidate')
        if out is None:
            out_p, out_t = torch.empty(m, 3, dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
        elif out_p.shape[0] < m:
            raise ValueError('out holds %d points, the cloud has %d' % (out_p.shape[0], m))
        hip.check(L.psi_mesh_cloud_compact(hip.ptr(pos), hip.ptr(tri), hip.ptr(keep), hip.ptr(keep_scan), n_cands, m, hip.ptr(out_p), hip.ptr(out_t),
                                           st), 'psi_mesh_cloud_compact')
    points, tri_out = out_p[:m], out_t[:m]
    if return_counts:
        return points, tri_out, (n_cands, n_rows)
    return points, tri_out


# ------------------------------------------------------------------------------------------
# Orienting a mesh towards free space: flood fill of a node mask and the votes of the triangles (psi_flood_fill, psi_mesh_orient_votes)
# ------------------------------------------------------------------------------------------
FLOOD_MIN_EDGE, FLOOD_MAX_EDGE = 2, 1024


def flood_fill(open_mask, seed_nodes, return_rounds=False):
    """The nodes of ``open_mask`` [Dx,Dy,Dz] (bool or uint8 on the GPU, non-zero = open) that are 6-connected through open nodes to one of
    ``seed_nodes`` [n,3] (ix, iy, iz; a tensor or anything ``torch.as_tensor`` takes): a bool tensor of the same shape (include/psi_hip.h:
    psi_flood_fill).  With ``return_rounds`` also the number of launches up to and including the first that gained
    nothing.  ``ValueError``: an edge outside 2 .. 1024, no seed, a seed node outside the grid or on a node that is not open (the message
    names the seed).  The call synchronises the stream once per 8 launches, and once before them for the seeds' verdict."""
    import ctypes
    if not torch.is_tensor(open_mask) or open_mask.dim() != 3 or open_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError('expected open_mask [Dx,Dy,Dz] bool or uint8')
    hip.ptr(open_mask)
    dims = tuple(int(d) for d in open_mask.shape)
    if min(dims) < FLOOD_MIN_EDGE or max(dims) > FLOOD_MAX_EDGE:
        raise ValueError('psi_flood_fill: every edge lies in %d .. %d (got %r)' % (FLOOD_MIN_EDGE, FLOOD_MAX_EDGE, dims))
    dev = open_mask.device
    seeds = torch.as_tensor(seed_nodes).reshape(-1, 3)
    if seeds.is_floating_point() or seeds.shape[0] < 1:
        raise ValueError('expected at least one seed node [n,3] of integers')
    seeds = seeds.to(dev, torch.int64)
    mask = open_mask.view(torch.uint8) if open_mask.dtype == torch.bool else open_mask
    hi = torch.tensor(dims, device=dev)
    inside = ((seeds >= 0) & (seeds < hi)).all(1)
    clamped = torch.minimum(seeds.clamp(min=0), hi - 1)
    is_open = mask[clamped[:, 0], clamped[:, 1], clamped[:, 2]] != 0
    verdict = torch.stack([inside, is_open], 1).cpu().numpy()                   # the one read before the launches
    for i, (ins, opn) in enumerate(verdict):
        if not ins:
            raise ValueError('seed %d: node %r lies outside the %r grid' % (i, tuple(seeds[i].tolist()), dims))
        if not opn:
            raise ValueError('seed %d: node %r is not open' % (i, tuple(seeds[i].tolist())))
    seeds32 = seeds.to(torch.int32).contiguous()
    free = torch.empty(dims, dtype=torch.uint8, device=dev)
    rounds = ctypes.c_int(0)
    with torch.cuda.device(dev):
        hip.check(hip.lib().psi_flood_fill(hip.ptr(mask), dims[0], dims[1], dims[2], hip.ptr(seeds32), int(seeds32.shape[0]), hip.ptr(free),
                                           ctypes.byref(rounds), hip.stream()), 'psi_flood_fill')
    free = free.view(torch.bool)
    return (free, rounds.value) if return_rounds else free


def mesh_orient_votes(points, tri, verts, faces, free, grid_min, grid_max, delta):
    """votes [nf,2] int32 on the GPU: per triangle the samples whose probe ``p + delta n`` (column 0) and ``p - delta n`` (column 1) has a
    free nearest node (include/psi_hip.h: psi_mesh_orient_votes).  points [n,3] fp32 and tri [n] int32 are the
    samples and their triangles, verts [nv,3] fp32 and faces [nf,3] int32 the caller's mesh, free [D,D,D] bool or uint8 the free nodes of
    the grid grid_min .. grid_max (host values), all on one GPU."""
    import math
    pp, pt, pv, pf = hip.ptr(points), hip.ptr(tri), hip.ptr(verts), hip.ptr(faces)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or tri.dtype != torch.int32 or tri.dim() != 1 \
            or tri.shape[0] != points.shape[0]:
        raise ValueError('expected points [n,3] float32 and tri [n] int32')
    if verts.dtype != torch.float32 or faces.dtype != torch.int32 or verts.dim() != 2 or faces.dim() != 2 or verts.shape[1] != 3 or faces.shape[1] != 3:
        raise ValueError('expected verts [nv,3] float32 and faces [nf,3] int32')
    if free.dtype not in (torch.bool, torch.uint8) or free.dim() != 3 or free.shape[0] != free.shape[1] or free.shape[1] != free.shape[2]:
        raise ValueError('expected free [D,D,D] bool or uint8')
    if len({t.device for t in (points, tri, verts, faces, free)}) != 1:
        raise ValueError('the tensors lie on different devices')
    dim, nv, nf = int(free.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    delta = float(delta)
    if dim < FLOOD_MIN_EDGE or dim > FLOOD_MAX_EDGE or nv < 1 or nf < 1 or not (math.isfinite(delta) and delta > 0):
        raise hip.PsiHipError('psi_mesh_orient_votes: 2 <= D <= 1024, nv >= 1, nf >= 1, delta positive and finite')
    lo, hi = _mesh_sdf_bounds(grid_min, grid_max)
    mask = free.view(torch.uint8) if free.dtype == torch.bool else free
    votes = torch.empty(nf, 2, dtype=torch.int32, device=verts.device)
    with torch.cuda.device(verts.device):
        hip.check(hip.lib().psi_mesh_orient_votes(pp, pt, int(points.shape[0]), pv, nv, pf, nf, hip.ptr(mask), lo, hi, dim, delta, hip.ptr(votes),
                                                  hip.stream()), 'psi_mesh_orient_votes')
    return votes


# ------------------------------------------------------------------------------------------
# What the ops over a batch of bodies share (body_overlap, surface_crossings)
# ------------------------------------------------------------------------------------------
def _host_array(x, dtype, what):
    import numpy as np
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.dtype != dtype:
        raise ValueError('expected %s of dtype %s, got %s' % (what, np.dtype(dtype).name, a.dtype))
    return np.ascontiguousarray(a)


def _batch_args(verts, group, name, then=None, max_B=None):
    """The checks of ``verts`` [B,V,3] fp32 and ``group`` [B] int32 or None, in the order that decides which exception a doubly-wrong call
    raises: verts, the caller's own argument checks (``then``), group, B <= ``max_B``, the device pointers (``PsiHipError`` for a CPU or
    non-contiguous tensor), B >= 1.  Returns B, V, dev, pv, pg."""
    _check_batch_verts(verts)
    if then is not None:
        then()
    B, V = int(verts.shape[0]), int(verts.shape[1])
    dev = verts.device
    if group is not None and (not torch.is_tensor(group) or group.dtype != torch.int32 or tuple(group.shape) != (B,) or group.device != dev):
        raise ValueError('expected group [%d] int32 on the device of verts' % B)
    if max_B is not None and B > max_B:
        raise ValueError('%s: B = %d is more than %d' % (name, B, max_B))
    pv, pg = hip.ptr(verts), hip.ptr(group)
    if B < 1:
        raise hip.PsiHipError('psi_%s: B >= 1' % name)
    return B, V, dev, pv, pg


def _check_batch_verts(verts):
    if not torch.is_tensor(verts) or verts.dtype != torch.float32 or verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1:
        raise ValueError('expected verts [B,V,3] float32')


def _check_real(x, ok, message, *shown):
    """``float(x)`` of a finite real number ``x``, not a bool, for which ``ok(x)`` holds; otherwise ``ValueError(message % shown)``."""
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(x) or not ok(x):
        raise ValueError(message % shown)
    return float(x)


def _chunks_of(n, chunk):
    """ceil(n / chunk) of a count or of a tensor of counts"""
    return (n + (chunk - 1)) // chunk


# kind of handle -> how an operator makes one of faces [F,3] and V when it is given no handle (None: only its own constructor makes one,
# scene_crossings_create of a scene mesh); psi_<kind>_info reads the integers of every kind
_HANDLE_KINDS = {'body_overlap': lambda faces, V: body_overlap_create(faces, V),
                 'surface_crossings': lambda faces, V: surface_crossings_create(faces, V),
                 'scene_crossings': None}


def _with_info(handle, kind):
    """Fills in the integers of the ``hip.Handle`` of ``kind`` (a key of ``_HANDLE_KINDS``) through psi_<kind>_info: ``V``, ``F`` and
    ``n_chunks`` (vertices, faces and 256-face chunks; of the scene mesh for 'scene_crossings'; 'body_overlap' has no chunks: 0)."""
    assert kind in _HANDLE_KINDS, kind
    info = (ctypes.c_int32 * 4)()               # body_overlap writes two of them
    hip.check(getattr(hip.lib(), 'psi_%s_info' % kind)(handle, info), 'psi_%s_info' % kind)
    handle.V, handle.F, handle.n_chunks = int(info[0]), int(info[1]), int(info[2])
    return handle


def _handle_of(handle_or_faces, V, kind):
    """The ``hip.Handle`` of ``kind`` an operator works with: the one the kind's constructor in ``_HANDLE_KINDS`` makes of faces (it lives
    as long as somebody holds it), or the handle given, which must have been made for ``V`` vertices per body.  Any other ``c_void_p``
    is a handle its caller owns: it is viewed, with its integers read from the library, and never freed from here."""
    if not isinstance(handle_or_faces, ctypes.c_void_p):
        return _HANDLE_KINDS[kind](handle_or_faces, V)
    handle = handle_or_faces
    if not isinstance(handle, hip.Handle):
        handle = hip.Handle(None)
        handle.value = handle_or_faces.value
        _with_info(handle, kind)
    if handle.V != V:
        raise ValueError('the handle was made for %d vertices per body, verts has %d' % (handle.V, V))
    return handle


def _unpack_bits(mask, n):
    """mask [B, ceil(n / 32)] int32, bit k of a row in word k >> 5 at position k & 31 -> [B,n] bool"""
    bit = torch.arange(n, device=mask.device)
    return ((mask[:, bit >> 5] >> (bit & 31).to(torch.int32)) & 1).bool()


# ------------------------------------------------------------------------------------------
# Body against body: interpenetration counts of a batch (psi_body_overlap_*)
# ------------------------------------------------------------------------------------------
BODY_OVERLAP_CHUNK = 256
BODY_OVERLAP_MAX_CANDIDATES = 2 ** 31 - 1


def body_overlap_create(faces, V):
    """faces [F,3] int32 (a tensor on any device, or an array), the one topology of every body, wound outwards; V vertices per body.  Returns
    the ``psi_body_overlap`` handle, a ``hip.Handle``: freed by ``body_overlap_destroy`` or when its last holder lets go of it.
    ``ValueError`` for a wrong dtype or shape; ``PsiHipError`` for what the library refuses: F < 1, a face index outside [0, V)."""
    import numpy as np
    f = _host_array(faces, np.int32, 'faces [F,3]')
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('expected faces [F,3] int32')
    h = hip.Handle('psi_body_overlap_destroy')
    hip.check(hip.lib().psi_body_overlap_create(ctypes.byref(h), f.ctypes.data_as(ctypes.c_void_p), int(V), int(f.shape[0])),
              'psi_body_overlap_create')
    return _with_info(h, 'body_overlap')


def body_overlap_destroy(handle):
    handle.close()


def body_overlap(verts, faces_handle_or_tensor, group=None, return_candidates=False):
    """Which vertices of one body of a batch lie inside another body of the batch (include/psi_hip.h: psi_body_overlap_*; DESIGN.md
    section 10d).  verts [B,V,3] fp32 on the GPU, world frame; ``faces_handle_or_tensor``: a handle of ``body_overlap_create`` or faces
    [F,3] int32 (a handle is then made and freed by the call); ``group`` [B] int32 on the GPU or None: only bodies of equal group are
    compared.  Returns counts [B,B] int32 (counts[i,j] = vertices of i inside j; zero diagonal, not symmetric) and inside [B,V] bool
    (inside at least one other body), with ``return_candidates`` also cand [n,3] int32 in ascending (i, j, v) order and w [n] fp32: all
    on the device.

    The kernels run on the current stream; the two scans (``torch.cumsum``, int64) are plumbing, and one read-back returns the number of
    candidates, the number of 256-candidate chunks and the non-finite flag: the call's only host synchronisation.  ``ValueError`` for
    wrong dtypes, shapes or devices, for a non-finite vertex (it names the first such body) and for more than 2^31 - 1 candidates;
    ``PsiHipError`` for what the library refuses, CPU tensors included."""
    B, V, dev, pv, pg = _batch_args(verts, group, 'body_overlap')
    L = hip.lib()
    with torch.cuda.device(dev):
        handle = _handle_of(faces_handle_or_tensor, V, 'body_overlap')
        F = handle.F
        st = hip.stream()
        boxes = torch.empty(B, 6, dtype=torch.float32, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        pair_count = torch.empty(B * B, dtype=torch.int32, device=dev)
        hip.check(L.psi_body_overlap_boxes(handle, pv, B, hip.ptr(boxes), hip.ptr(bad), st), 'psi_body_overlap_boxes')
        hip.check(L.psi_body_overlap_count(handle, pv, pg, B, hip.ptr(boxes), hip.ptr(pair_count), st), 'psi_body_overlap_count')
        pair_chunks = _chunks_of(pair_count, BODY_OVERLAP_CHUNK)
        cand_inc = torch.cumsum(pair_count, 0, dtype=torch.int64)
        chunk_inc = torch.cumsum(pair_chunks, 0, dtype=torch.int64)
        n_cand, n_chunks, first_bad = torch.stack([cand_inc[-1], chunk_inc[-1], bad[0].to(torch.int64)]).cpu().tolist()
        if first_bad < B:
            raise ValueError('body %d has a non-finite vertex coordinate' % first_bad)
        if n_cand > BODY_OVERLAP_MAX_CANDIDATES:
            raise ValueError('the batch has %d candidates: more than 2^31 - 1' % n_cand)
        counts = torch.zeros(B, B, dtype=torch.int32, device=dev)
        words = (V + 31) // 32
        mask = torch.zeros(B, words, dtype=torch.int32, device=dev)
        cand = torch.empty(n_cand, 3, dtype=torch.int32, device=dev)
        w = torch.empty(n_cand, dtype=torch.float32, device=dev)
        if n_cand > 0:                      # never an empty grid
            cand_off, chunk_off = cand_inc - pair_count, chunk_inc - pair_chunks
            chunks = torch.empty(n_chunks, 4, dtype=torch.int32, device=dev)
            hip.check(L.psi_body_overlap_emit(handle, pv, pg, B, hip.ptr(boxes), hip.ptr(pair_count), hip.ptr(cand_off), hip.ptr(chunk_off),
                                              n_cand, n_chunks, hip.ptr(cand), hip.ptr(chunks), st), 'psi_body_overlap_emit')
            ws_bytes = int(L.psi_body_overlap_workspace_bytes(n_cand, F))
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            hip.check(L.psi_body_overlap_wind(handle, pv, B, hip.ptr(cand), n_cand, hip.ptr(chunks), n_chunks, hip.ptr(ws), ws_bytes, st),
                      'psi_body_overlap_wind')
            hip.check(L.psi_body_overlap_decide(handle, B, hip.ptr(cand), n_cand, hip.ptr(ws), ws_bytes, hip.ptr(w), hip.ptr(counts),
                                                hip.ptr(mask), st), 'psi_body_overlap_decide')
        inside = _unpack_bits(mask, V)
    if return_candidates:
        return counts, inside, cand, w
    return counts, inside


# ------------------------------------------------------------------------------------------
# Body against body: penetration depth, its aggregates, the loss and its gradient (psi_body_depth_*, psi_segment_sum3)
# ------------------------------------------------------------------------------------------
BODY_DEPTH_MAX_TRIPLES = 2 ** 29 - 1
BODY_DEPTH_PENALTIES = {'depth': 0, 'squared': 1}


class DepthRows(NamedTuple):
    face: torch.Tensor         # [n] int32: the nearest face of body j
    region: torch.Tensor       # [n] int32: 0 face, 1 edge ab, 2 edge bc, 3 edge ca, 4 5 6 vertex a b c
    depth: torch.Tensor        # [n] fp32: the distance of the vertex to that face
    r: torch.Tensor            # [n,3] fp32: the vertex minus its closest point c
    bary: torch.Tensor         # [n,3] fp32: the barycentric coordinates of c in the face


class PenetrationResult(NamedTuple):
    triples: torch.Tensor      # [n,3] int32 (i, j, v): the inside triples, ascending
    rows: DepthRows
    max_depth: torch.Tensor    # [B,B] fp32: the deepest vertex of i inside j
    sum_depth: torch.Tensor    # [B,B] fp64: the depths of the vertices of i inside j, added in triple order
    sum_sq: torch.Tensor       # [B,B] fp64: their squares
    depth_of: torch.Tensor     # [B,V] fp32: the largest depth of the vertex over all j, 0 where it is inside no body
    loss: torch.Tensor         # [2,B] fp32: row 0 = (float) sum_j sum_depth[i,j], row 1 the same of sum_sq
    counts: torch.Tensor       # [B,B] int32 and
    inside: torch.Tensor       # [B,V] bool: as body_overlap returns them


def _depth_chunk_table(pair_count, B, n_chunks):
    """The chunk table of psi_body_overlap_emit, [n_chunks,4] int32 = (first triple, triples, i, j), for an ascending triple list with
    ``pair_count`` [B*B] int64 triples per ordered pair: plumbing, no host synchronisation."""
    pair_chunks = _chunks_of(pair_count, BODY_OVERLAP_CHUNK)
    chunk_inc, trip_inc = torch.cumsum(pair_chunks, 0), torch.cumsum(pair_count, 0)
    c = torch.arange(n_chunks, dtype=torch.int64, device=pair_count.device)
    p = torch.searchsorted(chunk_inc, c, right=True).clamp_(max=B * B - 1)
    k = c - (chunk_inc - pair_chunks)[p]
    first = (trip_inc - pair_count)[p] + k * BODY_OVERLAP_CHUNK
    cnt = (pair_count[p] - k * BODY_OVERLAP_CHUNK).clamp_(min=0, max=BODY_OVERLAP_CHUNK)
    return torch.stack([first, cnt, p // B, p % B], 1).to(torch.int32).contiguous()


def _new_depth_rows(n, dev):
    return DepthRows(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                     torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, 3, dtype=torch.float32, device=dev),
                     torch.empty(n, 3, dtype=torch.float32, device=dev))


def _depth_rows(handle, verts, trip, pair_count, n_chunks):
    """nearest and finish for the ascending triples ``trip`` [n,3], n >= 1."""
    L, st, dev = hip.lib(), hip.stream(), verts.device
    B, n = int(verts.shape[0]), int(trip.shape[0])
    chunks = _depth_chunk_table(pair_count, B, n_chunks)
    ws_bytes = int(L.psi_body_depth_workspace_bytes(n, handle.F))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    rows = _new_depth_rows(n, dev)
    hip.check(L.psi_body_depth_nearest(handle, hip.ptr(verts), B, hip.ptr(trip), n, hip.ptr(chunks), n_chunks, hip.ptr(ws), ws_bytes, st),
              'psi_body_depth_nearest')
    hip.check(L.psi_body_depth_finish(handle, hip.ptr(verts), B, hip.ptr(trip), n, hip.ptr(ws), ws_bytes, hip.ptr(rows.face),
                                      hip.ptr(rows.region), hip.ptr(rows.depth), hip.ptr(rows.r), hip.ptr(rows.bary), st), 'psi_body_depth_finish')
    return rows


def body_depth(verts, handle_or_faces, triples):
    """How far vertex v of body i is from the surface of body j, for every row (i, j, v) of ``triples`` (include/psi_hip.h:
    psi_body_depth_*): the nearest of the F current triangles of j by the seven-region closest point, bit-equal to
    the fp32 NumPy restatement.  verts [B,V,3] fp32 on the GPU; ``handle_or_faces``: a handle of ``body_overlap_create`` or faces [F,3]
    int32; ``triples`` [n,3] int32 on the device of verts, strictly ascending, i != j, every index in range — any such triple, not only
    one whose vertex is inside.  Returns ``DepthRows``, on the device.

    Two kernels on the current stream; the chunk table is plumbing.  ONE read-back: the verdict on the triples together with the number
    of 256-triple chunks.  n = 0 launches nothing.  ``ValueError`` for wrong dtypes, shapes or devices and for triples that are not strictly
    ascending, have i == j or an index out of range; ``PsiHipError`` for what the library refuses, CPU tensors included."""
    def check_triples():
        if not torch.is_tensor(triples) or triples.dtype != torch.int32 or triples.dim() != 2 or triples.shape[1] != 3:
            raise ValueError('expected triples [n,3] int32')
        if triples.device != verts.device:
            raise ValueError('expected triples on the device of verts')
        if triples.shape[0] > BODY_DEPTH_MAX_TRIPLES:
            raise ValueError('%d triples: more than 2^29 - 1' % triples.shape[0])

    B, V, dev, pv, _ = _batch_args(verts, None, 'body_depth', then=check_triples)
    n = int(triples.shape[0])
    with torch.cuda.device(dev), torch.no_grad():
        handle = _handle_of(handle_or_faces, V, 'body_overlap')
        if n == 0:
            return _new_depth_rows(0, dev)
        trip = triples.contiguous()
        t = trip.to(torch.int64)
        i, j, v = t[:, 0], t[:, 1], t[:, 2]
        key = (i * B + j) * V + v
        bad = ((i < 0) | (i >= B) | (j < 0) | (j >= B) | (v < 0) | (v >= V) | (i == j)).any() | (key[1:] <= key[:-1]).any()
        pair_count = torch.zeros(B * B, dtype=torch.int64, device=dev).scatter_add_(0, (i * B + j).clamp(0, B * B - 1), torch.ones_like(i))
        n_chunks = _chunks_of(pair_count, BODY_OVERLAP_CHUNK).sum()
        is_bad, n_chunks = torch.stack([bad.to(torch.int64), n_chunks]).cpu().tolist()
        if is_bad:
            raise ValueError('triples must be strictly ascending (i, j, v) rows with i != j, i and j in [0, %d) and v in [0, %d)' % (B, V))
        return _depth_rows(handle, verts, trip, pair_count, n_chunks)


def body_penetration(verts, handle_or_faces, group=None):
    """``body_overlap`` and, for its inside triples (the candidates with w > 0.5, in their order), ``body_depth`` and the aggregates of
    DESIGN.md section 10f.  Arguments as ``body_overlap``.  Returns ``PenetrationResult``, on the device.

    Host read-backs: ``body_overlap``'s one, and ONE more (the number of inside triples and of their 256-triple chunks); the inside
    triples are gathered with a stable sort of the decisions, whose size is then known, not with a boolean index.  A batch with no candidate
    stops after ``body_overlap``; one with no inside vertex gives zeros and launches nothing more."""
    B, V, dev, pv, pg = _batch_args(verts, group, 'body_penetration')
    L = hip.lib()
    with torch.cuda.device(dev), torch.no_grad():
        handle = _handle_of(handle_or_faces, V, 'body_overlap')
        counts, inside, cand, w = body_overlap(verts, handle, group=group, return_candidates=True)
        max_depth = torch.zeros(B, B, dtype=torch.float32, device=dev)
        sum_depth, sum_sq = torch.zeros(B, B, dtype=torch.float64, device=dev), torch.zeros(B, B, dtype=torch.float64, device=dev)
        depth_of = torch.zeros(B, V, dtype=torch.float32, device=dev)
        loss = torch.zeros(2, B, dtype=torch.float32, device=dev)
        n_in = n_chunks = 0
        if cand.shape[0] > 0:
            pair_count = counts.reshape(-1).to(torch.int64)
            n_in, n_chunks = torch.stack([pair_count.sum(), _chunks_of(pair_count, BODY_OVERLAP_CHUNK).sum()]).cpu().tolist()
        if n_in == 0:
            return PenetrationResult(cand[:0], _new_depth_rows(0, dev), max_depth, sum_depth, sum_sq, depth_of, loss, counts, inside)
        if n_in > BODY_DEPTH_MAX_TRIPLES:
            raise ValueError('the batch has %d inside triples: more than 2^29 - 1' % n_in)
        keep = torch.sort((~(w > 0.5)).to(torch.uint8), stable=True).indices[:n_in]       # the triples with w > 0.5, in their order
        trip = cand[keep].contiguous()
        rows = _depth_rows(handle, verts, trip, pair_count, n_chunks)
        row_start = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        row_start[1:] = torch.cumsum(pair_count.view(B, B).sum(1), 0)
        hip.check(L.psi_body_depth_pairs(handle, B, hip.ptr(trip), n_in, hip.ptr(rows.depth), hip.ptr(row_start), hip.ptr(max_depth),
                                         hip.ptr(sum_depth), hip.ptr(sum_sq), hip.ptr(depth_of), hip.ptr(loss), hip.stream()),
                  'psi_body_depth_pairs')
        return PenetrationResult(trip, rows, max_depth, sum_depth, sum_sq, depth_of, loss, counts, inside)


def segment_sum3(targets_sorted, rows, n_out, order=None):
    """out [n_out,3] fp32 with out[t] = ((0 + x0) + x1) + ... over the run of rows whose target is t, in the order of the list
    (psi_segment_sum3): ``targets_sorted`` [m] int64 ascending, ``rows`` [m,3] fp32, ``order`` [m] int64 or None: sorted position k takes
    row order[k].  Rows of untouched targets are 0; a target outside [0, n_out) is ignored.  No floating-point atomics."""
    if (not torch.is_tensor(targets_sorted) or targets_sorted.dtype != torch.int64 or targets_sorted.dim() != 1 or not torch.is_tensor(rows)
            or rows.dtype != torch.float32 or tuple(rows.shape) != (targets_sorted.shape[0], 3) or rows.device != targets_sorted.device):
        raise ValueError('expected targets_sorted [m] int64 and rows [m,3] float32 on one device')
    if order is not None and (not torch.is_tensor(order) or order.dtype != torch.int64 or order.shape != targets_sorted.shape
                              or order.device != rows.device):
        raise ValueError('expected order [m] int64 on the device of rows')
    if int(n_out) < 1:
        raise ValueError('n_out >= 1')
    pt, pr, po = hip.ptr(targets_sorted), hip.ptr(rows), hip.ptr(order)
    m = int(targets_sorted.shape[0])
    with torch.cuda.device(rows.device):
        out = torch.zeros(int(n_out), 3, dtype=torch.float32, device=rows.device)
        if m > 0:
            hip.check(hip.lib().psi_segment_sum3(pt, po, pr, m, hip.ptr(out), int(n_out), hip.stream()), 'psi_segment_sum3')
    return out


def _sum_rows_by_target(targets, grows, B, V):
    """G [B,V,3] fp32 of the gradient rows ``grows`` [m,3] and their target vertices ``targets`` [m] int64: a stable ``torch.sort`` of the
    targets, then the rows of one target added in list order (``segment_sum3``)."""
    srt = torch.sort(targets, stable=True)
    return segment_sum3(srt.values, grows, B * V, order=srt.indices).view(B, V, 3)


def body_penetration_grad(verts_shape, handle, triples, rows, g, penalty='depth'):
    """G [B,V,3] fp32: the gradient of sum_i g[i] loss[i] with respect to the vertices, for the inside ``triples`` and their ``rows``
    (``PenetrationResult``): grad_rows, a stable ``torch.sort`` of the targets, the segment sum.  No read-back."""
    if penalty not in BODY_DEPTH_PENALTIES:
        raise ValueError('penalty is one of %s, got %r' % (sorted(BODY_DEPTH_PENALTIES), penalty))
    B, V = int(verts_shape[0]), int(verts_shape[1])
    if not torch.is_tensor(g) or g.dtype != torch.float32 or tuple(g.shape) != (B,):
        raise ValueError('expected g [%d] float32' % B)
    dev, n = g.device, int(triples.shape[0])
    with torch.cuda.device(dev), torch.no_grad():
        if n == 0:
            return torch.zeros(B, V, 3, dtype=torch.float32, device=dev)
        g = g.contiguous()
        targets = torch.empty(4 * n, dtype=torch.int64, device=dev)
        grows = torch.empty(4 * n, 3, dtype=torch.float32, device=dev)
        hip.check(hip.lib().psi_body_depth_grad_rows(handle, B, hip.ptr(triples), n, hip.ptr(rows.face), hip.ptr(rows.depth), hip.ptr(rows.r),
                                                     hip.ptr(rows.bary), hip.ptr(g), BODY_DEPTH_PENALTIES[penalty], hip.ptr(targets),
                                                     hip.ptr(grows), hip.stream()), 'psi_body_depth_grad_rows')
        return _sum_rows_by_target(targets, grows, B, V)


class _BodyPenetrationLoss(Function):
    @staticmethod
    def forward(ctx, verts, handle, group, penalty):
        res = body_penetration(verts, handle, group=group)
        ctx.handle, ctx.penalty, ctx.shape = handle, penalty, tuple(verts.shape)        # the graph holds the handle it will need
        ctx.save_for_backward(res.triples, *res.rows)
        return res.loss[BODY_DEPTH_PENALTIES[penalty]].clone()

    @staticmethod
    def backward(ctx, g):
        trip, *rows = ctx.saved_tensors
        G = body_penetration_grad(ctx.shape, ctx.handle, trip, DepthRows(*rows), g.to(torch.float32).contiguous(), ctx.penalty)
        return G, None, None, None


def body_penetration_loss(verts, handle_or_faces, group=None, penalty='depth'):
    """loss [B] fp32: how deep body i stands in the other bodies of the batch, (float) sum_j sum_depth[i,j] for ``penalty='depth'`` (the
    L1 form of the scene collision term; the default) or (float) sum_j sum_sq[i,j] for ``'squared'``.
    Differentiable with respect to ``verts``: the gradient reaches the inside vertex and, with the barycentric weights of its closest
    point, the three corners of the nearest face of the other body; it is exact by the envelope theorem wherever the winner is unique.
    The backward pass runs grad_rows, a stable ``torch.sort`` and the segment sum: no floating-point atomics, bit-identical from run to
    run, no read-back.  The forward pass is ``body_penetration`` (two read-backs, ``body_overlap``'s included).  No inside vertex: zeros, a
    zero gradient and no launch.  ``ValueError`` for an unknown penalty and for what ``body_overlap`` refuses."""
    if penalty not in BODY_DEPTH_PENALTIES:
        raise ValueError('penalty is one of %s, got %r' % (sorted(BODY_DEPTH_PENALTIES), penalty))
    _check_batch_verts(verts)
    hip.ptr(verts)                              # a CPU or non-contiguous tensor is refused before a handle is made
    return _BodyPenetrationLoss.apply(verts, _handle_of(handle_or_faces, int(verts.shape[1]), 'body_overlap'), group, penalty)


# ------------------------------------------------------------------------------------------
# Surface crossings: triangle pairs of the bodies of a batch that intersect (psi_surface_crossings_*)
# ------------------------------------------------------------------------------------------
SURFACE_CROSSINGS_CHUNK = 256
SURFACE_CROSSINGS_MAX = 2 ** 31 - 1             # tiles, and pairs
SURFACE_CROSSINGS_MAX_B = 46340                  # GEOM_MAX_B of csrc/geom_shared.h: B * B < 2^31
SURFACE_CROSSINGS_MAX_F = 2 ** 21


class CrossingsResult(NamedTuple):
    pairs: torch.Tensor        # [n,4] int32 (i, s, j, t), ascending: face s of body i crosses face t of body j
    events: torch.Tensor       # [n] int32: piercing edges of the pair, 1 to 6; 2 is the regular case
    length: torch.Tensor       # [n] fp32: the length of the pair's intersection segment (0 unless events == 2)
    counts: torch.Tensor       # [B,B] int32, symmetric: crossing pairs of bodies i and j; the diagonal holds self crossings
    contour: torch.Tensor      # [B,B] fp64, symmetric: the lengths of the pairs of (i, j) added in pair order
    face_hit: torch.Tensor     # [B,F] bool: the face is in at least one crossing pair
    irregular: torch.Tensor    # [] int32: pairs with events != 2


def surface_crossings_create(faces, V, order_verts=None, face_part=None, part_skip=None):
    """faces [F,3] int32 (a tensor on any device, or an array): the one topology of every body; V vertices per body.  ``order_verts`` [V,3]
    fp32 or None: a representative pose (``v_template``); with it the faces are sorted once along a Morton curve of their centroids into the
    chunks of 256 the search prunes by (results are in the caller's face indices either way).  ``face_part`` [F] int32 and ``part_skip``
    [P,P] uint8 (symmetric; non-zero: self pairs of faces of these two parts are ignored) or both None.  Returns the
    ``psi_surface_crossings`` handle, a ``hip.Handle``: freed by ``surface_crossings_destroy`` or when its last holder lets go of it.
    ``ValueError`` for wrong dtypes or shapes, F < 1, F >= 2^21, V < 1, a face index outside [0, V), a part outside [0, P), an
    asymmetric matrix."""
    import numpy as np
    f = _host_array(faces, np.int32, 'faces [F,3]')
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('expected faces [F,3] int32')
    F, V = int(f.shape[0]), int(V)
    if F < 1 or F >= SURFACE_CROSSINGS_MAX_F or V < 1:
        raise ValueError('surface_crossings_create: 1 <= F < 2^21 and V >= 1, got F = %d, V = %d' % (F, V))
    if f.min() < 0 or f.max() >= V:
        raise ValueError('surface_crossings_create: a face index outside [0, %d)' % V)
    ov = fp = ps = None
    P = 0
    if order_verts is not None:
        ov = _host_array(order_verts, np.float32, 'order_verts [V,3]')
        if ov.shape != (V, 3) or not np.isfinite(ov).all():
            raise ValueError('expected finite order_verts [%d,3] float32' % V)
    if (face_part is None) != (part_skip is None):
        raise ValueError('surface_crossings_create: face_part and part_skip come together')
    if face_part is not None:
        fp, ps = _host_array(face_part, np.int32, 'face_part [F]'), _host_array(part_skip, np.uint8, 'part_skip [P,P]')
        P = int(ps.shape[0]) if ps.ndim == 2 else 0
        if fp.shape != (F,) or ps.ndim != 2 or ps.shape != (P, P) or P < 1:
            raise ValueError('expected face_part [%d] int32 and part_skip [P,P] uint8' % F)
        if fp.min() < 0 or fp.max() >= P:
            raise ValueError('surface_crossings_create: a face_part entry outside [0, %d)' % P)
        if not np.array_equal(ps != 0, (ps != 0).T):
            raise ValueError('surface_crossings_create: part_skip is not symmetric')
    as_p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    h = hip.Handle('psi_surface_crossings_destroy')
    hip.check(hip.lib().psi_surface_crossings_create(ctypes.byref(h), as_p(f), V, F, as_p(ov), as_p(fp), as_p(ps), P),
              'psi_surface_crossings_create')
    return _with_info(h, 'surface_crossings')


def surface_crossings_destroy(handle):
    handle.close()


def _faces_in_chunk(n, chunk):
    """how many of n faces lie in 256-face chunk ``chunk`` (a tensor of chunk indices): 256 but for a partial last chunk"""
    return (n - chunk * SURFACE_CROSSINGS_CHUNK).clamp(max=SURFACE_CROSSINGS_CHUNK)


def _crossings_search(kind, lead, tile_args, body, pv, B, n_jobs, key_stride, width, outs):
    """The passes of a crossing search, psi_<kind>_{tiles,test,finish} of ``kind`` 'surface_crossings' or 'scene_crossings', on the current
    stream and device of the caller: the boxes of the ``body`` handle's chunks and bodies, the tile count pass, a scan, read-back 1 (the
    tiles with the non-finite flag), the tile emit pass, the test count pass, a scan, read-back 2 (the pairs), the test emit pass, the
    sort of the int64 keys, the row starts of the bodies (``key_stride`` keys per body) and finish, which fills the caller's zeroed
    ``outs`` (counts, contour, the bit masks, irregular, as psi_<kind>_finish takes them).  ``lead``: the handles that lead every
    argument list of the kind; ``tile_args``: what follows them in tiles; ``n_jobs``: the workgroups of the tile passes (0: nothing is
    admitted and nothing is launched); ``width``: the columns of a pair row.  A pass with nothing to do is not launched: no tile ends
    after read-back 1, no pair after read-back 2.  Returns pairs [n,width] int32, events [n] int32, length [n] fp32, n_tiles, n_pairs
    and the tile table [n_tiles,4] int32 (None without tiles).  ``ValueError`` for a non-finite vertex and for more than 2^31 - 1
    tiles or pairs."""
    L, st, dev = hip.lib(), hip.stream(), outs[0].device
    i32, i64, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev), dict(dtype=torch.float32, device=dev)

    def run(name, *args):
        hip.check(getattr(L, name)(*args, st), name)

    tiles_pass, test_pass, finish = ('psi_%s_%s' % (kind, p) for p in ('tiles', 'test', 'finish'))
    pairs, events, length = torch.empty(0, width, **i32), torch.empty(0, **i32), torch.empty(0, **f32)
    if n_jobs == 0:
        return pairs, events, length, 0, 0, None
    chunk_boxes, body_boxes = torch.empty(B, body.n_chunks, 6, **f32), torch.empty(B, 6, **f32)
    bad, job_tiles = torch.empty(1, **i32), torch.empty(n_jobs, **i32)
    cb, bb, jt = hip.ptr(chunk_boxes), hip.ptr(body_boxes), hip.ptr(job_tiles)
    run('psi_surface_crossings_boxes', body, pv, B, cb, bb, hip.ptr(bad))
    run(tiles_pass, *lead, *tile_args, cb, bb, jt, None, 0, None)
    job_inc = torch.cumsum(job_tiles, 0, dtype=torch.int64)
    n_tiles, first_bad = torch.stack([job_inc[-1], bad[0].to(torch.int64)]).cpu().tolist()                  # read-back 1
    if first_bad < B:
        raise ValueError('body %d has a non-finite vertex coordinate' % first_bad)
    if n_tiles > SURFACE_CROSSINGS_MAX:
        raise ValueError('the batch has %d tiles: more than 2^31 - 1' % n_tiles)
    if n_tiles == 0:                            # never an empty grid
        return pairs, events, length, 0, 0, None
    tiles, job_off = torch.empty(n_tiles, 4, **i32), job_inc - job_tiles
    run(tiles_pass, *lead, *tile_args, cb, bb, jt, hip.ptr(job_off), n_tiles, hip.ptr(tiles))
    tile_hits = torch.empty(n_tiles, **i32)
    run(test_pass, *lead, pv, B, hip.ptr(tiles), n_tiles, hip.ptr(tile_hits), None, 0, None, None, None)
    tile_inc = torch.cumsum(tile_hits, 0, dtype=torch.int64)
    n_pairs = int(tile_inc[-1].item())                                                                      # read-back 2
    if n_pairs > SURFACE_CROSSINGS_MAX:
        raise ValueError('the batch has %d crossing pairs: more than 2^31 - 1' % n_pairs)
    if n_pairs == 0:
        return pairs, events, length, n_tiles, 0, tiles
    keys, ev_raw, len_raw = torch.empty(n_pairs, **i64), torch.empty(n_pairs, **i32), torch.empty(n_pairs, **f32)
    tile_off = tile_inc - tile_hits
    run(test_pass, *lead, pv, B, hip.ptr(tiles), n_tiles, hip.ptr(tile_hits), hip.ptr(tile_off), n_pairs, hip.ptr(keys), hip.ptr(ev_raw),
        hip.ptr(len_raw))
    keys_sorted, order = torch.sort(keys)
    row_start = torch.searchsorted(keys_sorted, torch.arange(B + 1, **i64) * key_stride).contiguous()
    pairs, events, length = torch.empty(n_pairs, width, **i32), torch.empty(n_pairs, **i32), torch.empty(n_pairs, **f32)
    run(finish, *lead, B, hip.ptr(keys_sorted), hip.ptr(order), hip.ptr(ev_raw), hip.ptr(len_raw), n_pairs, hip.ptr(row_start), hip.ptr(pairs),
        hip.ptr(events), hip.ptr(length), *(hip.ptr(o) for o in outs))
    return pairs, events, length, n_tiles, n_pairs, tiles


def surface_crossings(verts, handle_or_faces, group=None, self_pairs=True, between=True, mode='pruned', return_stats=False):
    """Which pairs of triangles of the body surfaces of a batch properly intersect (include/psi_hip.h: psi_surface_crossings_*; DESIGN.md
    section 10e).  verts [B,V,3] fp32 on the GPU, world frame; ``handle_or_faces``: a handle of ``surface_crossings_create`` or faces [F,3]
    int32 (a handle is then made and freed by the call); ``group`` [B] int32 on the GPU or None: only bodies of equal group are compared
    with each other; ``self_pairs``: pairs of faces of one body that share no vertex (and whose parts the handle does not skip);
    ``between``: pairs of faces of two bodies; ``mode``: 'pruned', or 'brute', which tests every chunk pair of every admitted pair of
    bodies and gives the same bits.  Returns a ``CrossingsResult`` on the device (with ``return_stats`` also {'tiles', 'pairs', 'box_tests'}, at the
    price of one more read-back).

    The kernels run on the current stream; two scans (``torch.cumsum``), one sort of the int64 pair keys and one ``searchsorted`` are
    plumbing.  Two read-backs: the number of tiles with the non-finite flag, and the number of pairs.  ``ValueError`` for wrong dtypes,
    shapes or devices, a non-finite vertex (it names the first such body), B > 46340, (B F)^2 >= 2^63 and more than 2^31 - 1 tiles or
    pairs; ``PsiHipError`` for what the library refuses, CPU tensors included."""
    def check_mode():
        if mode not in ('pruned', 'brute'):
            raise ValueError("mode is 'pruned' or 'brute', got %r" % (mode,))
    B, V, dev, pv, pg = _batch_args(verts, group, 'surface_crossings', then=check_mode, max_B=SURFACE_CROSSINGS_MAX_B)
    flags = (1 if self_pairs else 0) | (2 if between else 0) | (4 if mode == 'brute' else 0)
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        handle = _handle_of(handle_or_faces, V, 'surface_crossings')
        F = handle.F
        if (B * F) ** 2 >= 2 ** 63:
            raise ValueError('surface_crossings: (B F)^2 = (%d x %d)^2 does not fit the int64 pair key' % (B, F))
        counts = torch.zeros(B, B, **i32)
        contour = torch.zeros(B, B, dtype=torch.float64, device=dev)
        mask = torch.zeros(B, (F + 31) // 32, **i32)
        irregular = torch.zeros(1, **i32)
        pairs, events, length, n_tiles, n_pairs, tiles = _crossings_search(
            'surface_crossings', (handle,), (pg, B, flags), handle, pv, B, n_jobs=B * B if flags & 3 else 0, key_stride=F * B * F, width=4,
            outs=(counts, contour, mask, irregular))
        face_hit = _unpack_bits(mask, F)
    res = CrossingsResult(pairs, events, length, counts, contour, face_hit, irregular[0])
    if not return_stats:
        return res
    box_tests = 0
    if n_tiles > 0:                             # the (pair, box) tests the test pass executes, counted from the tile table
        t = tiles.long()
        na, nb = _faces_in_chunk(F, t[:, 2]), _faces_in_chunk(F, t[:, 3])
        diagonal = (t[:, 0] == t[:, 1]) & (t[:, 2] == t[:, 3])
        box_tests = int(torch.where(diagonal, na * (na - 1) // 2, na * nb).sum().item())
    return res, {'tiles': int(n_tiles), 'pairs': int(n_pairs), 'box_tests': box_tests}


# ------------------------------------------------------------------------------------------
# Scene crossings: body triangles of a batch that intersect triangles of a static scene mesh (psi_scene_crossings_*)
# ------------------------------------------------------------------------------------------
class SceneCrossingsResult(NamedTuple):
    pairs: torch.Tensor        # [n,3] int32 (i, s, t), strictly ascending: face s of body i crosses scene triangle t (the caller's indices)
    events: torch.Tensor       # [n] int32: piercing edges of the pair, 1 to 6; 2 is the regular case
    length: torch.Tensor       # [n] fp32: the length of the pair's intersection segment (0 unless events == 2)
    counts: torch.Tensor       # [B] int32: crossing pairs of body i
    contour: torch.Tensor      # [B] fp64: the lengths of body i added one after the other in pair order
    face_hit: torch.Tensor     # [B,F] bool: the body face is in a crossing pair
    tri_hit: torch.Tensor      # [nf] bool: the scene triangle is crossed by some body
    irregular: torch.Tensor    # [] int32: pairs with events != 2


def scene_crossings_create(scene_verts, scene_faces):
    """scene_verts [nv,3] fp32 and scene_faces [nf,3] int32 (tensors on any device, or arrays): the scene mesh, fixed for the life of the
    handle; degenerate triangles are kept.  The triangles are sorted once on the host along a Morton curve of their centroids into chunks of
    256 with exact boxes; no kernel runs.  Returns the ``psi_scene_crossings`` handle, a ``hip.Handle`` (``V`` = nv, ``F`` = nf,
    ``n_chunks`` scene chunks): freed by ``scene_crossings_destroy`` or when its last holder lets go of it.  ``ValueError`` for wrong
    dtypes or shapes, nf < 1, a face index outside [0, nv), a non-finite referenced vertex."""
    import numpy as np
    v, f = _host_array(scene_verts, np.float32, 'scene_verts [nv,3]'), _host_array(scene_faces, np.int32, 'scene_faces [nf,3]')
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('expected scene_verts [nv,3] float32 and scene_faces [nf,3] int32')
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if nf < 1 or nf >= 2 ** 31 or nv < 1:
        raise ValueError('scene_crossings_create: 1 <= nf < 2^31 and nv >= 1, got nf = %d, nv = %d' % (nf, nv))
    if f.min() < 0 or f.max() >= nv:
        raise ValueError('scene_crossings_create: a face index outside [0, %d)' % nv)
    used = np.zeros(nv, bool)
    used[f.ravel()] = True
    if not np.isfinite(v[used]).all():
        raise ValueError('scene_crossings_create: vertex %d, which a triangle refers to, is not finite'
                         % int(np.nonzero(used & ~np.isfinite(v).all(1))[0][0]))
    h = hip.Handle('psi_scene_crossings_destroy')
    hip.check(hip.lib().psi_scene_crossings_create(ctypes.byref(h), v.ctypes.data_as(ctypes.c_void_p), nv, f.ctypes.data_as(ctypes.c_void_p), nf),
              'psi_scene_crossings_create')
    return _with_info(h, 'scene_crossings')


def scene_crossings_destroy(handle):
    handle.close()


def scene_crossings(verts, scene_handle, body_handle_or_faces, mode='pruned', return_stats=False):
    """Which triangles of the body surfaces of a batch properly intersect which triangles of a scene mesh (include/psi_hip.h:
    psi_scene_crossings_*).  verts [B,V,3] fp32 on the GPU, world frame; ``scene_handle``: a handle of
    ``scene_crossings_create``; ``body_handle_or_faces``: a handle of ``surface_crossings_create`` or faces [F,3] int32 (a handle is then
    made and freed by the call); ``mode``: 'pruned', or 'brute', which tests every body chunk against every scene chunk and gives the same
    bits.  Returns a ``SceneCrossingsResult`` on the device (with ``return_stats`` also {'tiles', 'pairs', 'box_tests'}, at the price of
    one more read-back).

    The kernels run on the current stream; two scans (``torch.cumsum``), one sort of the int64 pair keys and one ``searchsorted`` are
    plumbing.  Two read-backs: the number of tiles with the non-finite flag, and the number of pairs; no empty grid is launched.
    ``ValueError`` for wrong dtypes, shapes or devices, a non-finite vertex (it names the first such body), B > 46340, B F nf >= 2^63 and
    more than 2^31 - 1 tiles or pairs; ``PsiHipError`` for what the library refuses, CPU tensors included."""
    def check():
        if mode not in ('pruned', 'brute'):
            raise ValueError("mode is 'pruned' or 'brute', got %r" % (mode,))
        if not isinstance(scene_handle, hip.Handle) or scene_handle.destroy != 'psi_scene_crossings_destroy' or not scene_handle:
            raise ValueError('scene_crossings: scene_handle is a live handle of scene_crossings_create')
    B, V, dev, pv, _ = _batch_args(verts, None, 'scene_crossings', then=check, max_B=SURFACE_CROSSINGS_MAX_B)
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        body = _handle_of(body_handle_or_faces, V, 'surface_crossings')
        F, nC, nf = body.F, body.n_chunks, scene_handle.F
        if B * F * nf >= 2 ** 63:
            raise ValueError('scene_crossings: B F nf = %d x %d x %d does not fit the int64 pair key' % (B, F, nf))
        counts = torch.zeros(B, **i32)
        contour = torch.zeros(B, dtype=torch.float64, device=dev)
        face_mask = torch.zeros(B, (F + 31) // 32, **i32)
        tri_mask = torch.zeros(1, (nf + 31) // 32, **i32)
        irregular = torch.zeros(1, **i32)
        pairs, events, length, n_tiles, n_pairs, tiles = _crossings_search(
            'scene_crossings', (scene_handle, body), (B, 1 if mode == 'brute' else 0), body, pv, B, n_jobs=B * nC, key_stride=F * nf, width=3,
            outs=(counts, contour, face_mask, tri_mask, irregular))
        res = SceneCrossingsResult(pairs, events, length, counts, contour, _unpack_bits(face_mask, F), _unpack_bits(tri_mask, nf)[0], irregular[0])
    if not return_stats:
        return res
    box_tests = 0
    if n_tiles > 0:                             # the (face, triangle) box tests the test pass executes, counted from the tile table
        t = tiles.long()
        box_tests = int((_faces_in_chunk(F, t[:, 1]) * _faces_in_chunk(nf, t[:, 2])).sum().item())
    return res, {'tiles': int(n_tiles), 'pairs': int(n_pairs), 'box_tests': box_tests}


# ------------------------------------------------------------------------------------------
# Surface crossings: the conic distance field of triangle pairs, its loss and gradient (psi_crossing_field_*)
# ------------------------------------------------------------------------------------------
CROSSING_FIELD_MAX_PAIRS = 2 ** 27 - 1
CROSSING_FIELD_SIGMA = 1e-3                      # the reference's constructor default (body_model.py:461); SMPLify-X uses 0.5


class FieldRows(NamedTuple):
    energy: torch.Tensor       # [n,2] fp32: column 0 = face s of body i in the field of face t of body j (i intrudes), column 1 the reverse
    psi: torch.Tensor          # [n,2,3] fp32: the six values Psi, per role in corner order


class CrossingFieldResult(NamedTuple):
    crossings: CrossingsResult
    rows: FieldRows            # of crossings.pairs
    pair_energy: torch.Tensor  # [B,B] fp64, NOT symmetric: E[i,j] = what body i pays for being inside body j; the diagonal is self energy
    loss: torch.Tensor         # [B] fp32: (float) sum_j E[i,j] in j order


def _check_sigma(sigma):
    return _check_real(sigma, lambda s: 0.0 < s <= 0.5, 'sigma is a finite number in (0, 0.5], got %r', sigma)


def _new_field_rows(n, dev):
    return FieldRows(torch.empty(n, 2, dtype=torch.float32, device=dev), torch.empty(n, 2, 3, dtype=torch.float32, device=dev))


def _field_rows(handle, verts, pairs, sigma):
    """eval for the pairs [n,4], n >= 1"""
    B, n = int(verts.shape[0]), int(pairs.shape[0])
    rows = _new_field_rows(n, verts.device)
    hip.check(hip.lib().psi_crossing_field_eval(handle, hip.ptr(verts), B, hip.ptr(pairs), n, sigma, hip.ptr(rows.psi), hip.ptr(rows.energy),
                                                hip.stream()), 'psi_crossing_field_eval')
    return rows


def _check_pairs_arg(pairs, verts):
    if not torch.is_tensor(pairs) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 4:
        raise ValueError('expected pairs [n,4] int32')
    if pairs.device != verts.device:
        raise ValueError('expected pairs on the device of verts')
    if pairs.shape[0] > CROSSING_FIELD_MAX_PAIRS:
        raise ValueError('%d pairs: more than 2^27 - 1' % pairs.shape[0])


def crossing_field(verts, handle_or_faces, pairs, sigma=CROSSING_FIELD_SIGMA):
    """The conic distance field (Tzionas et al. 2016; zero outside the cone) of every row (i, s, j, t) of ``pairs``: the three corners of face
    s of body i evaluated in the cone of face t of body j, and the other way round (include/psi_hip.h: psi_crossing_field_*; DESIGN.md
    section 10g), bit-equal to the fp32 NumPy restatement.  verts [B,V,3] fp32 on the GPU; ``handle_or_faces``: a handle of
    ``surface_crossings_create`` or faces [F,3] int32; ``pairs`` [n,4] int32 on the device of verts, in the handle's caller face indices,
    strictly ascending, i <= j, every index in range: any such pair, not only a crossing one; ``sigma`` in (0, 0.5] (the default 1e-3 is
    the reference's; SMPLify-X uses 0.5).  Returns ``FieldRows`` on the device.

    One kernel on the current stream and ONE read-back, the verdict on the pairs.  n = 0 launches nothing.  ``ValueError`` for wrong dtypes,
    shapes or devices, a sigma outside (0, 0.5] and a bad pair list; ``PsiHipError`` for what the library refuses, CPU tensors included."""
    def check():
        _check_sigma(sigma)
        _check_pairs_arg(pairs, verts)

    B, V, dev, pv, _ = _batch_args(verts, None, 'crossing_field', then=check, max_B=SURFACE_CROSSINGS_MAX_B)
    n = int(pairs.shape[0])
    with torch.cuda.device(dev), torch.no_grad():
        handle = _handle_of(handle_or_faces, V, 'surface_crossings')
        F = handle.F
        if n == 0:
            return _new_field_rows(0, dev)
        prs = pairs.contiguous()
        p = prs.to(torch.int64)
        i, s, j, t = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        bad = ((i < 0) | (i >= B) | (j < i) | (j >= B) | (s < 0) | (s >= F) | (t < 0) | (t >= F)).any()
        if (B * F) ** 2 < 2 ** 63:
            key = ((i * F + s) * B + j) * F + t
            bad = bad | (key[1:] <= key[:-1]).any()
        else:                               # the key does not fit one int64: compare the rows lexicographically
            d = p[1:] - p[:-1]
            first = (d != 0).to(torch.int8).argmax(1)
            bad = bad | ((d == 0).all(1) | (d.gather(1, first[:, None])[:, 0] < 0)).any()
        if bool(bad.item()):                                                                            # the read-back
            raise ValueError('pairs must be strictly ascending (i, s, j, t) rows with i <= j, i and j in [0, %d) and s and t in [0, %d)'
                             % (B, F))
        return _field_rows(handle, verts, prs, float(sigma))


def _field_aggregates(handle, B, pairs, energy):
    """pair_energy [B,B] fp64 and loss [B] fp32 of the pairs [n,4], n >= 1: the stable sort of the 2n entries by cell is plumbing."""
    dev, n = pairs.device, int(pairs.shape[0])
    p = pairs.to(torch.int64)
    cells = torch.stack([p[:, 0] * B + p[:, 2], p[:, 2] * B + p[:, 0]], 1).reshape(-1)
    srt = torch.sort(cells, stable=True)
    row_start = torch.searchsorted(srt.values, torch.arange(B + 1, dtype=torch.int64, device=dev) * B).contiguous()
    pair_energy = torch.zeros(B, B, dtype=torch.float64, device=dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    hip.check(hip.lib().psi_crossing_field_pairs(handle, B, hip.ptr(pairs), n, hip.ptr(energy), hip.ptr(srt.values), hip.ptr(srt.indices),
                                                 hip.ptr(row_start), hip.ptr(pair_energy), hip.ptr(loss), hip.stream()),
              'psi_crossing_field_pairs')
    return pair_energy, loss


def crossing_penetration(verts, handle_or_faces, group=None, self_pairs=True, between=True, sigma=CROSSING_FIELD_SIGMA, mode='pruned'):
    """``surface_crossings`` and, for its pairs, the conic distance field and the aggregates of DESIGN.md section 10g.  Arguments as
    ``surface_crossings``, and ``sigma`` as ``crossing_field``.  Returns ``CrossingFieldResult`` on the device: ``pair_energy[i,j]`` is what
    body i pays for standing in body j (not symmetric; the diagonal is the energy of a body that passes through itself), ``loss[i]`` its
    row sum.  The only term of the family that sees a body passing through itself and surfaces that cross with no vertex inside.

    No read-back beyond ``surface_crossings``' two.  No crossing pair: zeros, and nothing more is launched."""
    _check_sigma(sigma)
    B, V, dev, pv, pg = _batch_args(verts, group, 'crossing_penetration', max_B=SURFACE_CROSSINGS_MAX_B)
    with torch.cuda.device(dev), torch.no_grad():
        handle = _handle_of(handle_or_faces, V, 'surface_crossings')
        res = surface_crossings(verts, handle, group=group, self_pairs=self_pairs, between=between, mode=mode)
        n = int(res.pairs.shape[0])
        if n == 0:
            return CrossingFieldResult(res, _new_field_rows(0, dev), torch.zeros(B, B, dtype=torch.float64, device=dev),
                                       torch.zeros(B, dtype=torch.float32, device=dev))
        if n > CROSSING_FIELD_MAX_PAIRS:
            raise ValueError('the batch has %d crossing pairs: more than 2^27 - 1' % n)
        rows = _field_rows(handle, verts, res.pairs, float(sigma))
        pair_energy, loss = _field_aggregates(handle, B, res.pairs, rows.energy)
        return CrossingFieldResult(res, rows, pair_energy, loss)


def crossing_field_grad(verts, handle, pairs, g, sigma=CROSSING_FIELD_SIGMA):
    """G [B,V,3] fp32: the exact gradient of sum_i g[i] loss[i] with respect to the vertices for the constant list ``pairs`` (role 0 of a
    pair scaled by g[i], role 1 by g[j]): grad_rows, a stable ``torch.sort`` of the targets, the segment sum.  No read-back, no
    floating-point atomics."""
    _check_sigma(sigma)
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if not torch.is_tensor(g) or g.dtype != torch.float32 or tuple(g.shape) != (B,) or g.device != verts.device:
        raise ValueError('expected g [%d] float32 on the device of verts' % B)
    _check_pairs_arg(pairs, verts)
    dev, n = verts.device, int(pairs.shape[0])
    with torch.cuda.device(dev), torch.no_grad():
        if n == 0:
            return torch.zeros(B, V, 3, dtype=torch.float32, device=dev)
        g, pairs = g.contiguous(), pairs.contiguous()
        targets = torch.empty(12 * n, dtype=torch.int64, device=dev)
        grows = torch.empty(12 * n, 3, dtype=torch.float32, device=dev)
        hip.check(hip.lib().psi_crossing_field_grad_rows(handle, hip.ptr(verts), B, hip.ptr(pairs), n, float(sigma), hip.ptr(g), hip.ptr(targets),
                                                         hip.ptr(grows), hip.stream()), 'psi_crossing_field_grad_rows')
        return _sum_rows_by_target(targets, grows, B, V)


class _CrossingPenetrationLoss(Function):
    @staticmethod
    def forward(ctx, verts, handle, group, self_pairs, between, sigma, mode):
        res = crossing_penetration(verts, handle, group=group, self_pairs=self_pairs, between=between, sigma=sigma, mode=mode)
        ctx.handle, ctx.sigma = handle, sigma                                           # the graph holds the handle it will need
        ctx.save_for_backward(verts.detach(), res.crossings.pairs)
        return res.loss.clone()

    @staticmethod
    def backward(ctx, g):
        verts, pairs = ctx.saved_tensors
        G = crossing_field_grad(verts, ctx.handle, pairs, g.to(torch.float32).contiguous(), ctx.sigma)
        return G, None, None, None, None, None, None


def crossing_penetration_loss(verts, handle_or_faces, group=None, self_pairs=True, between=True, sigma=CROSSING_FIELD_SIGMA, mode='pruned'):
    """loss [B] fp32 of ``crossing_penetration``: what body i pays for passing through the other bodies of the batch and through itself
    (DESIGN.md section 10g).  Differentiable with respect to ``verts``: the gradient is exact for the pair list of the forward pass, which
    is a constant (the loss jumps when a pair appears); it reaches the three corners of the intruding face and, through the normal, the
    circumcentre and the circumradius, the three corners of the receiving face.  The backward pass runs grad_rows (which recomputes the
    forward), a stable ``torch.sort`` and the segment sum: no floating-point atomics, bit-identical from run to run, no read-back.  No
    crossing pair: zeros, a zero gradient and no launch.  ``ValueError`` as ``crossing_penetration``."""
    _check_sigma(sigma)
    if mode not in ('pruned', 'brute'):
        raise ValueError("mode is 'pruned' or 'brute', got %r" % (mode,))
    _check_batch_verts(verts)
    hip.ptr(verts)                              # a CPU or non-contiguous tensor is refused before a handle is made
    return _CrossingPenetrationLoss.apply(verts, _handle_of(handle_or_faces, int(verts.shape[1]), 'surface_crossings'), group, bool(self_pairs),
                                          bool(between), float(sigma), mode)


# ------------------------------------------------------------------------------------------
# Body against body: move overlapping bodies apart rigidly (psi_body_separate_*)
# ------------------------------------------------------------------------------------------
RIGID_CHUNK = 256


class RigidState(NamedTuple):
    quat: torch.Tensor         # [B,4] fp32 (w, x, y, z)
    transl: torch.Tensor       # [B,3] fp32
    pivot: torch.Tensor        # [B,3] fp32, constant: the body turns about pivot + transl
    m: torch.Tensor            # [B,6] fp32 and
    s: torch.Tensor            # [B,6] fp32: the Adam moments of (force, torque)


class SeparationResult(NamedTuple):
    verts: torch.Tensor        # [B,V,3] fp32: the bodies under their final state
    quat: torch.Tensor         # [B,4] fp32
    transl: torch.Tensor       # [B,3] fp32
    pivot: torch.Tensor        # [B,3] fp32
    transform: torch.Tensor    # [B,4,4] fp64: x' = M x for the vertices given
    iterations: int            # steps taken
    separated: bool            # the last pass found nothing inside, nothing crossing and, with a scene, no vertex of a free body in it
    history: dict              # per pass: 'triples', 'pairs' (lists of int; -1: not searched), 'loss_pen', 'loss_cross' ([passes,B] fp32);
                               # with a scene also 'scene_inside' (a list of [B] int64 on the host) and 'loss_scene' ([passes,B] fp64)
    shift: torch.Tensor        # [B] fp64: |transl|
    angle: torch.Tensor        # [B] fp64: the rotation angle, radians


class SceneSeparationResult(SeparationResult):
    """What ``rigid_separate`` returns with a scene: the ten fields of ``SeparationResult`` in their order, and beside them the attribute
    ``scene_inside`` [B] int64 on the host, the vertices of every body in its scene at the last pass."""

    def __new__(cls, *fields, scene_inside=None):
        self = super().__new__(cls, *fields)
        self.scene_inside = scene_inside
        return self


def rigid_state(pivot):
    """The identity state about ``pivot`` [B,3] fp32: quat (1,0,0,0), transl 0, zero moments."""
    if not torch.is_tensor(pivot) or pivot.dtype != torch.float32 or pivot.dim() != 2 or pivot.shape[1] != 3 or pivot.shape[0] < 1:
        raise ValueError('expected pivot [B,3] float32')
    B, dev = int(pivot.shape[0]), pivot.device
    quat = torch.zeros(B, 4, dtype=torch.float32, device=dev)
    quat[:, 0] = 1.0
    return RigidState(quat, torch.zeros(B, 3, dtype=torch.float32, device=dev), pivot.contiguous(),
                      torch.zeros(B, 6, dtype=torch.float32, device=dev), torch.zeros(B, 6, dtype=torch.float32, device=dev))


def _check_rows(t, B, width, name, dev, dtype=torch.float32):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (B, width) or t.device != dev:
        raise ValueError('expected %s [%d,%d] %s on the device of the vertices' % (name, B, width, str(dtype).replace('torch.', '')))


def _check_verts3(v, name):
    if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 3 or v.shape[2] != 3 or v.shape[1] < 1 or v.shape[0] < 1:
        raise ValueError('expected %s [B,V,3] float32' % name)


def rigid_pose(base, quat, transl, pivot):
    """verts [B,V,3] fp32 = R(quat) (base - pivot) + (pivot + transl) per body (psi_body_separate_pose), bit-equal to
    the fp32 NumPy restatement.  A body whose state is exactly quat = (1,0,0,0), transl = 0 gets the bits of ``base``.  One kernel on the
    current stream, no read-back.  ``ValueError`` for wrong dtypes, shapes or devices; ``PsiHipError`` for CPU tensors."""
    _check_verts3(base, 'base')
    B, V, dev = int(base.shape[0]), int(base.shape[1]), base.device
    _check_rows(quat, B, 4, 'quat', dev), _check_rows(transl, B, 3, 'transl', dev), _check_rows(pivot, B, 3, 'pivot', dev)
    pb, pq, pt, pc = hip.ptr(base), hip.ptr(quat), hip.ptr(transl), hip.ptr(pivot)
    with torch.cuda.device(dev):
        verts = torch.empty_like(base)
        hip.check(hip.lib().psi_body_separate_pose(pb, pq, pt, pc, B, V, hip.ptr(verts), hip.stream()), 'psi_body_separate_pose')
    return verts


def _rigid_chunks(verts, G, p, g6):
    B, V = int(verts.shape[0]), int(verts.shape[1])
    chunks = torch.empty(B, _chunks_of(V, RIGID_CHUNK), 6, dtype=torch.float64, device=verts.device)
    hip.check(hip.lib().psi_body_separate_wrench(hip.ptr(verts), hip.ptr(G), hip.ptr(p), B, V, hip.ptr(chunks), hip.ptr(g6), hip.stream()),
              'psi_body_separate_wrench')
    return chunks


def rigid_wrench(verts, G, pivot_plus_transl, return_chunks=False):
    """g6 [B,6] fp32 = (force, torque about p) of the gradient ``G`` [B,V,3] = dL/dverts on the bodies ``verts`` [B,V,3], p =
    ``pivot_plus_transl`` [B,3] (psi_body_separate_wrench): sum_v G and sum_v (x - p) x G, the terms in fp32, the sums in fp64 in a fixed
    order (a 256-lane tree per chunk of 256 vertices, then the chunks in order), rounded once.  No floating-point atomics; bit-equal to
    the restatement and from run to run.  ``return_chunks``: also the chunk sums [B, ceil(V/256), 6] fp64.  Two kernels, no read-back."""
    _check_verts3(verts, 'verts')
    B, dev = int(verts.shape[0]), verts.device
    if not torch.is_tensor(G) or G.dtype != torch.float32 or G.shape != verts.shape or G.device != dev:
        raise ValueError('expected G float32 of the shape and on the device of verts')
    _check_rows(pivot_plus_transl, B, 3, 'pivot_plus_transl', dev)
    hip.ptr(verts), hip.ptr(G), hip.ptr(pivot_plus_transl)
    with torch.cuda.device(dev):
        g6 = torch.empty(B, 6, dtype=torch.float32, device=dev)
        chunks = _rigid_chunks(verts, G, pivot_plus_transl, g6)
    return (g6, chunks) if return_chunks else g6


def _check_w_scene(w_scene, positive=False):
    _check_real(w_scene, lambda w: w >= 0, 'w_scene is a finite number >= 0, got %r', w_scene)
    if positive and w_scene == 0:
        raise ValueError('w_scene is zero with a scene given: leave the scene out instead')


def _check_scene(sdf, grid_min, grid_max, scene_id, B, dev):
    """The scene table of the separation: sdf [S,D,D,D] fp32 with D >= 2, grid_min, grid_max [S,3] fp32, scene_id [B] int32 or None, all
    on ``dev``.  ``ValueError`` otherwise.  Returns S, D."""
    if not torch.is_tensor(sdf) or sdf.dtype != torch.float32 or sdf.dim() != 4 or sdf.shape[0] < 1 or sdf.device != dev:
        raise ValueError('expected sdf [S,D,D,D] float32 on the device of the vertices')
    S, D = int(sdf.shape[0]), int(sdf.shape[1])
    if tuple(sdf.shape[1:]) != (D, D, D):
        raise ValueError('the volumes are cubic, got %s' % (tuple(sdf.shape[1:]),))
    if D < 2:
        raise ValueError('D >= 2, got %d' % D)
    _check_rows(grid_min, S, 3, 'grid_min', dev), _check_rows(grid_max, S, 3, 'grid_max', dev)
    if scene_id is not None and (not torch.is_tensor(scene_id) or scene_id.dtype != torch.int32 or tuple(scene_id.shape) != (B,) or scene_id.device != dev):
        raise ValueError('expected scene_id [%d] int32 on the device of the vertices, or None' % B)
    return S, D


def _scene_launch(verts, p, scene, w_scene, value=None, G=None):
    """psi_body_separate_scene on checked arguments: chunks [B,nchunk,6] fp64, count [B,nchunk] int32, loss [B,nchunk] fp64."""
    sdf, gmin, gmax, scene_id = scene
    B, V, dev = int(verts.shape[0]), int(verts.shape[1]), verts.device
    nchunk = _chunks_of(V, RIGID_CHUNK)
    chunks = torch.empty(B, nchunk, 6, dtype=torch.float64, device=dev)
    count = torch.empty(B, nchunk, dtype=torch.int32, device=dev)
    loss = torch.empty(B, nchunk, dtype=torch.float64, device=dev)
    hip.check(hip.lib().psi_body_separate_scene(hip.ptr(verts), hip.ptr(p), hip.ptr(sdf), hip.ptr(gmin), hip.ptr(gmax), hip.ptr(scene_id), B, V,
                                                int(sdf.shape[1]), int(sdf.shape[0]), float(w_scene), hip.ptr(chunks), hip.ptr(count),
                                                hip.ptr(loss), hip.ptr(value), hip.ptr(G), hip.stream()), 'psi_body_separate_scene')
    return chunks, count, loss


def _chunk_order_sum(rows):
    """[..., nchunk] -> [...]: the chunk rows added in chunk order from +0 (an fp64 sum whose order is part of the contract)."""
    acc = torch.zeros(rows.shape[:-1], dtype=rows.dtype, device=rows.device)
    for c in range(rows.shape[-1]):
        acc = acc + rows[..., c]
    return acc


def rigid_scene_wrench(verts, pivot_plus_transl, sdf, grid_min, grid_max, scene_id=None, w_scene=1.0, return_fields=False):
    """The scene term of ``rigid_separate`` on the bodies ``verts`` [B,V,3] fp32 (psi_body_separate_scene).  ``sdf``
    [S,D,D,D] fp32 holds one node-centred signed distance volume per scene (element [ix][iy][iz]) over the boxes ``grid_min``, ``grid_max``
    [S,3] fp32; ``scene_id`` [B] int32 picks the volume of a body (None: scene 0; clamped to [0, S)).  A vertex whose trilinear value is
    < 0 is in the scene: G = -w_scene * gradient (zero along an axis on which the vertex is outside the box), loss -value.  Returns
    ``chunks`` [B, ceil(V/256), 6] fp64, the sums of (G, (x - p) x G) per chunk of 256 vertices by the tree of ``rigid_wrench`` with p =
    ``pivot_plus_transl`` [B,3]; ``count`` [B] int64, the vertices in the scene; ``loss`` [B] fp64, the chunk sums of -value added in chunk
    order.  ``return_fields``: also the value [B,V] and G [B,V,3] of every vertex.  One kernel, no read-back, no floating-point atomics;
    bit-equal to the fp32 NumPy restatement and from run to run.  ``ValueError`` for wrong shapes, dtypes or devices, a volume that is not
    cubic, D < 2, a negative or non-finite w_scene; ``PsiHipError`` for CPU tensors."""
    _check_verts3(verts, 'verts')
    B, V, dev = int(verts.shape[0]), int(verts.shape[1]), verts.device
    _check_rows(pivot_plus_transl, B, 3, 'pivot_plus_transl', dev)
    _check_scene(sdf, grid_min, grid_max, scene_id, B, dev)
    _check_w_scene(w_scene)
    for t in (verts, pivot_plus_transl, sdf, grid_min, grid_max, scene_id):
        hip.ptr(t)
    with torch.cuda.device(dev), torch.no_grad():
        value = torch.empty(B, V, dtype=torch.float32, device=dev) if return_fields else None
        G = torch.empty(B, V, 3, dtype=torch.float32, device=dev) if return_fields else None
        chunks, count, loss = _scene_launch(verts, pivot_plus_transl, (sdf, grid_min, grid_max, scene_id), w_scene, value, G)
        count, loss = count.to(torch.int64).sum(1), _chunk_order_sum(loss)
    return (chunks, count, loss, value, G) if return_fields else (chunks, count, loss)


def _check_scene_tuple(scene, B, dev):
    if not isinstance(scene, (tuple, list)) or len(scene) != 4:
        raise ValueError('scene is a tuple (sdf, grid_min, grid_max, scene_id) of tensors on the device of the vertices; scene_id may be None')
    _check_scene(scene[0], scene[1], scene[2], scene[3], B, dev)


class _RigidScene:
    """A checked scene tuple for the loop, with what a pass needs beside it: the pinned host buffer its counts are copied to, the event
    that marks the copy, and the bodies that may move, on the host (one read-back when it is made, none in a pass)."""

    def __init__(self, scene, B, dev, fixed_mask):
        _check_scene_tuple(scene, B, dev)
        self.tensors = tuple(scene)
        for t in self.tensors:
            hip.ptr(t)
        self.free = None if fixed_mask is None else (fixed_mask == 0).cpu()
        self.host = torch.empty(B, dtype=torch.int64).pin_memory()
        self.copied = torch.cuda.Event()
        self.loss_rows = False         # rigid_separate sets it: a pass then hands on its [B,nchunk] loss rows, added once after the loop


def _check_step_args(lr_t, lr_r, betas, eps):
    for name, lr in (('lr_t', lr_t), ('lr_r', lr_r)):
        _check_real(lr, lambda x: x > 0, '%s is a finite positive number, got %r', name, lr)
    for b in betas if isinstance(betas, (tuple, list)) and len(betas) == 2 else (None,):        # None: not a pair, refused in the same words
        _check_real(b, lambda x: 0.0 <= x < 1.0, 'betas is a pair of numbers in [0, 1), got %r', betas)
    _check_real(eps, lambda x: x >= 0, 'eps is a finite number >= 0, got %r', eps)


def _fixed_mask(fixed, B, dev):
    """[B] int32 on ``dev`` (1: the body is held) or None, of a list of body indices or a [B] bool / int32 tensor."""
    if fixed is None:
        return None
    if torch.is_tensor(fixed):
        if fixed.dtype not in (torch.bool, torch.int32) or tuple(fixed.shape) != (B,) or fixed.device != dev:
            raise ValueError('expected fixed [%d] bool or int32 on the device of the vertices, or a list of bodies' % B)
        return fixed.to(torch.int32).contiguous()
    try:
        idx = [int(i) for i in fixed]
    except TypeError:
        raise ValueError('fixed is a list of bodies or a [B] mask, got %r' % (fixed,))
    if any(not 0 <= i < B or i != f for i, f in zip(idx, fixed)):
        raise ValueError('fixed: a body outside [0, %d)' % B)
    mask = torch.zeros(B, dtype=torch.int32)
    if idx:
        mask[idx] = 1
    return mask.to(dev)


def _rigid_step(state, g6, chunks, k, lr_t, lr_r, betas, eps, mask):
    B = int(state.quat.shape[0])
    c1, c2 = 1.0 - float(betas[0]) ** k, 1.0 - float(betas[1]) ** k         # fp64; rounded to fp32 once on the way into the library
    hip.check(hip.lib().psi_body_separate_step(hip.ptr(chunks), 0 if chunks is None else int(chunks.shape[1]), hip.ptr(g6), hip.ptr(state.quat),
                                               hip.ptr(state.transl), hip.ptr(state.m), hip.ptr(state.s), hip.ptr(mask), B, float(betas[0]),
                                               float(betas[1]), c1, c2, float(eps), float(lr_t), float(lr_r), hip.stream()),
              'psi_body_separate_step')


def rigid_step(state, g6, k, lr_t=0.01, lr_r=0.01, betas=(0.9, 0.999), eps=1e-8, fixed=None):
    """Step ``k`` = 1, 2, ... of Adam on the wrench ``g6`` [B,6], in place on ``state`` (a ``RigidState``; psi_body_separate_step): the
    moments, transl -= lr_t u[0:3], and the quaternion turned by delta = -lr_r u[3:6] through the Cayley map, normalise((1, delta/2) (x)
    quat); a body whose delta is exactly zero keeps its quaternion's bits, a body in ``fixed`` (a list of bodies or a [B] mask) sees g6 = 0.
    The bias corrections 1 - beta^k are computed in fp64 on the host.  One kernel, no read-back.  Returns ``state``."""
    if not isinstance(state, RigidState):
        raise ValueError('expected a RigidState')
    _check_rows(state.quat, int(state.quat.shape[0]) if torch.is_tensor(state.quat) and state.quat.dim() == 2 else 0, 4, 'quat',
                getattr(state.quat, 'device', None))
    B, dev = int(state.quat.shape[0]), state.quat.device
    if B < 1:
        raise ValueError('B >= 1')
    _check_rows(state.transl, B, 3, 'transl', dev), _check_rows(state.m, B, 6, 'm', dev), _check_rows(state.s, B, 6, 's', dev)
    _check_rows(g6, B, 6, 'g6', dev)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError('k is an integer >= 1, got %r' % (k,))
    _check_step_args(lr_t, lr_r, betas, eps)
    mask = _fixed_mask(fixed, B, dev)
    for t in (state.quat, state.transl, state.m, state.s, g6):
        hip.ptr(t)
    with torch.cuda.device(dev):
        _rigid_step(state, g6, None, k, lr_t, lr_r, betas, eps, mask)
    return state


def _rigid_transform(quat, transl, pivot):
    """M [B,4,4] fp64, shift [B] and angle [B] fp64 of a state: the nine entries of R in fp64, t = (pivot + transl) - R pivot."""
    q, t, c = quat.double(), transl.double(), pivot.double()
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    M = torch.zeros(q.shape[0], 4, 4, dtype=torch.float64, device=q.device)
    M[:, :3, :3] = R
    M[:, :3, 3] = (c + t) - torch.einsum('bkl,bl->bk', R, c)
    M[:, 3, 3] = 1.0
    return M, t.norm(dim=1), 2.0 * torch.atan2(q[:, 1:].norm(dim=1), w.abs())


class RigidPass(NamedTuple):
    verts: torch.Tensor        # [B,V,3] fp32: the pose of the state the pass was given
    triples: int               # inside triples found (-1: w_pen == 0, not searched)
    pairs: int                 # crossing pairs found (-1: w_cross == 0, not searched)
    loss_pen: torch.Tensor     # [B] fp32
    loss_cross: torch.Tensor   # [B] fp32
    clean: bool                # nothing inside and nothing crossing
    stepped: bool              # the state was advanced
    g6: torch.Tensor           # [B,6] fp32 when stepped, else None
    scene_inside: torch.Tensor = None      # with a scene: [B] int64 on the host, the vertices of every body in its scene
    stop: bool = None                      # with a scene: clean, and no body that may move has a vertex in its scene
    loss_scene: torch.Tensor = None        # with a scene: [B] fp64
    chunks: torch.Tensor = None            # with a scene, when stepped: [B,nchunk,6] fp64, the bodies' chunk sums plus the scene's


def rigid_pass(base, state, k, overlap_handle, crossings_handle, group=None, fixed_mask=None, step=True, lr_t=0.01, lr_r=0.01,
               betas=(0.9, 0.999), eps=1e-8, w_pen=1.0, w_cross=1.0, penalty='depth', sigma=0.5, mode='pruned', scene=None, w_scene=1.0):
    """One pass of ``rigid_separate``'s loop from ``state`` (a ``RigidState``, advanced in place when the pass steps): the pose, the two
    searches, the stop test and, unless the batch is clean or ``step`` is false, the two gradients, their sum, the wrench and step ``k`` of
    the optimiser (the chunk sums go straight into the step's launch).  ``fixed_mask``: [B] int32 on the device or None.  The arguments
    are ``rigid_separate``'s, which has checked them.  Returns ``RigidPass``.

    ``scene``: None, or the tuple (sdf, grid_min, grid_max, scene_id) of ``rigid_scene_wrench``.  The scene kernel is then launched after
    the pose and before the searches, and its [B] counts go to a pinned host buffer with a non-blocking copy on the same stream.  Every
    search reads its own counts back with a blocking copy on that stream, queued after ours, so ours has landed when the first search
    returns: the pass has no host wait of its own (the event recorded behind the copy is queried, and waited for only if a search ever
    returned without a read-back).  The pass stops when the bodies are clean and no body outside ``fixed_mask`` has a vertex in its
    scene; otherwise the bodies' chunk sums (zeros when they are clean) and the scene's are added in fp64 and go into the step."""
    B, dev = int(base.shape[0]), base.device
    if scene is not None and not isinstance(scene, _RigidScene):
        scene = _RigidScene(scene, B, dev, fixed_mask)
    with torch.cuda.device(dev), torch.no_grad():
        verts = rigid_pose(base, state.quat, state.transl, state.pivot)
        if scene is not None:
            p = state.pivot + state.transl
            chunks_scene, count, loss = _scene_launch(verts, p, scene.tensors, w_scene)
            scene.host.copy_(count.to(torch.int64).sum(1), non_blocking=True)
            scene.copied.record()
            loss_scene = loss if scene.loss_rows else _chunk_order_sum(loss)
        pen = body_penetration(verts, overlap_handle, group=group) if w_pen != 0 else None
        cr = crossing_penetration(verts, crossings_handle, group=group, self_pairs=False, between=True, sigma=sigma, mode=mode) if w_cross != 0 else None
        if scene is not None:
            if not scene.copied.query():
                scene.copied.synchronize()
            inside = scene.host.clone()
        n_tri = -1 if pen is None else int(pen.triples.shape[0])
        n_pairs = -1 if cr is None else int(cr.crossings.pairs.shape[0])
        loss_pen = torch.zeros(B, dtype=torch.float32, device=dev) if pen is None else pen.loss[BODY_DEPTH_PENALTIES[penalty]]
        loss_cross = torch.zeros(B, dtype=torch.float32, device=dev) if cr is None else cr.loss
        stop = clean = n_tri <= 0 and n_pairs <= 0
        with_scene = ()                         # the fields of RigidPass that only a pass with a scene fills
        if scene is not None:
            stop = clean and int((inside if scene.free is None else inside[scene.free]).sum()) == 0
            with_scene = (inside, stop, loss_scene)
        if stop or not step:
            return RigidPass(verts, n_tri, n_pairs, loss_pen, loss_cross, clean, False, None, *with_scene)
        G = None                                # stays None for clean bodies, which only a scene makes step
        if pen is not None and not clean:
            G = body_penetration_grad(verts.shape, overlap_handle, pen.triples, pen.rows, torch.full((B,), float(w_pen), dtype=torch.float32, device=dev),
                                      penalty)
        if cr is not None and not clean:
            Gc = crossing_field_grad(verts, crossings_handle, cr.crossings.pairs, torch.full((B,), float(w_cross), dtype=torch.float32, device=dev),
                                     sigma)
            G = Gc if G is None else G + Gc
        g6 = torch.empty(B, 6, dtype=torch.float32, device=dev)
        if scene is None:
            chunks = _rigid_chunks(verts, G, state.pivot + state.transl, None)
        elif clean:
            chunks = torch.zeros_like(chunks_scene) + chunks_scene         # the bodies' chunk sums are +0: the same fp64 add
        else:
            chunks = _rigid_chunks(verts, G, p, None) + chunks_scene
        _rigid_step(state, g6, chunks, k, lr_t, lr_r, betas, eps, fixed_mask)
        if scene is not None:
            with_scene += (chunks,)
        return RigidPass(verts, n_tri, n_pairs, loss_pen, loss_cross, clean, True, g6, *with_scene)


def rigid_separate(base, overlap_handle_or_faces, crossings_handle_or_faces, group=None, fixed=None, pivot=None, max_iter=100, lr_t=0.01,
                   lr_r=0.01, betas=(0.9, 0.999), eps=1e-8, w_pen=1.0, w_cross=1.0, penalty='depth', sigma=0.5, mode='pruned', scene=None,
                   w_scene=1.0):
    """Moves the bodies ``base`` [B,V,3] fp32 rigidly, each by a rotation about its pivot and a translation, until no vertex of one lies
    inside another and no surfaces cross.  Shape and pose of every body are kept.  ``overlap_handle_or_faces``: a
    handle of ``body_overlap_create`` or faces [F,3] int32 (a tensor); ``crossings_handle_or_faces``: a handle of
    ``surface_crossings_create`` or faces; ``group`` [B] int32 on the device or None: only bodies of equal group meet; ``fixed``: bodies
    that must not move (a list, or a [B] mask on the device) — two fixed bodies that overlap each other never separate; ``pivot`` [B,3] fp32
    on the device or None: the mean of the body's vertices, in fp64, rounded once.

    One pass: ``rigid_pose``; ``body_penetration`` and ``crossing_penetration(self_pairs=False, between=True)``; stop when there is no
    inside triple and no crossing pair (these counts are on the host already: no read-back of the loop's own); otherwise
    ``body_penetration_grad`` with g = w_pen and ``crossing_field_grad`` with g = w_cross from the rows and lists just found (nothing is
    searched twice, no autograd graph), one fp32 add, ``rigid_wrench`` and ``rigid_step``.  A weight of zero leaves that term's search out
    (its history entry is -1) and the stop test looks at the other term alone.  At most ``max_iter`` steps.  Self crossings are not looked
    at: a rigid motion cannot change them.  Returns ``SeparationResult``; ``verts`` is always the pose of the state returned.

    ``scene`` = (sdf [S,D,D,D], grid_min [S,3], grid_max [S,3], scene_id [B] int32 or None), fp32 tensors on the device (the table of
    ``rigid_scene_wrench``), keeps the bodies out of their scenes as well: every pass adds the wrench of the hinge term w_scene * sum of
    -sdf over the vertices with sdf < 0 to the bodies' (``rigid_pass`` says how, and why without a host wait), and the loop goes on until
    the bodies are clean AND no body that may move has a vertex in its scene.  The scene term is always the hinge, whatever ``penalty``
    is: a squared depth has no gradient at the surface and does not finish.  The result then is a ``SceneSeparationResult``, with ``scene_inside`` [B], and the history
    keys 'scene_inside' and 'loss_scene'; a fixed body's vertices are counted there but do not hold the loop open.  A body wedged between
    furniture and another body may not finish: ``separated`` says so.  Without a scene every launch and every bit is what it was.

    ``ValueError`` for wrong shapes, dtypes or devices, max_iter < 1, a non-positive or non-finite learning rate, sigma outside (0, 0.5], a
    negative weight, both weights zero, an unknown penalty or mode, a scene that is not such a tuple, a volume that is not cubic, D < 2,
    a negative or non-finite w_scene, w_scene == 0 with a scene; ``PsiHipError`` for what the library refuses, CPU tensors included."""
    import numpy as np

    def check():
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
            raise ValueError('max_iter is an integer >= 1, got %r' % (max_iter,))
        _check_step_args(lr_t, lr_r, betas, eps)
        _check_sigma(sigma)
        for name, w in (('w_pen', w_pen), ('w_cross', w_cross)):
            _check_real(w, lambda x: x >= 0, '%s is a finite number >= 0, got %r', name, w)
        if w_pen == 0 and w_cross == 0:
            raise ValueError('w_pen and w_cross are both zero: nothing to separate by')
        if penalty not in BODY_DEPTH_PENALTIES:
            raise ValueError('penalty is one of %s, got %r' % (sorted(BODY_DEPTH_PENALTIES), penalty))
        if mode not in ('pruned', 'brute'):
            raise ValueError("mode is 'pruned' or 'brute', got %r" % (mode,))
        if scene is not None:
            _check_w_scene(w_scene, positive=True)
            _check_scene_tuple(scene, int(base.shape[0]), base.device)
        if base.shape[0] >= 1:
            if pivot is not None:
                _check_rows(pivot, int(base.shape[0]), 3, 'pivot', base.device)
            if fixed is not None:
                _fixed_mask(fixed, int(base.shape[0]), base.device if torch.is_tensor(fixed) else 'cpu')

    if torch.is_tensor(base) and base.dim() == 3 and base.shape[0] < 1:
        raise ValueError('expected base [B,V,3] float32 with B >= 1')
    B, V, dev, pb, pg = _batch_args(base, group, 'rigid_separate', then=check, max_B=SURFACE_CROSSINGS_MAX_B)
    with torch.cuda.device(dev), torch.no_grad():
        mask = _fixed_mask(fixed, B, dev)
        if pivot is None:
            pivot = torch.from_numpy(base.detach().cpu().numpy().astype(np.float64).mean(1).astype(np.float32)).to(dev)
        state = rigid_state(pivot.clone())
        hist = {'triples': [], 'pairs': [], 'loss_pen': [], 'loss_cross': []}
        table = None
        if scene is not None:
            table = _RigidScene(scene, B, dev, mask)
            table.loss_rows = True
            hist['scene_inside'], hist['loss_scene'] = [], []
        k, separated = 0, False
        oh, ch = _handle_of(overlap_handle_or_faces, V, 'body_overlap'), _handle_of(crossings_handle_or_faces, V, 'surface_crossings')
        while True:
            one = rigid_pass(base, state, k + 1, oh, ch, group=group, fixed_mask=mask, step=k < max_iter, lr_t=lr_t, lr_r=lr_r, betas=betas,
                             eps=eps, w_pen=w_pen, w_cross=w_cross, penalty=penalty, sigma=sigma, mode=mode, scene=table, w_scene=w_scene)
            verts = one.verts
            hist['triples'].append(one.triples), hist['pairs'].append(one.pairs)
            hist['loss_pen'].append(one.loss_pen), hist['loss_cross'].append(one.loss_cross)
            separated = one.clean
            if table is not None:
                hist['scene_inside'].append(one.scene_inside), hist['loss_scene'].append(one.loss_scene)
                separated = one.stop
            if not one.stepped:
                break
            k += 1
        hist['loss_pen'], hist['loss_cross'] = torch.stack(hist['loss_pen']), torch.stack(hist['loss_cross'])
        M, shift, angle = _rigid_transform(state.quat, state.transl, state.pivot)
        if table is not None:
            hist['loss_scene'] = _chunk_order_sum(torch.stack(hist['loss_scene']))        # [passes,B,nchunk] -> [passes,B], in chunk order
            return SceneSeparationResult(verts, state.quat, state.transl, state.pivot, M, k, separated, hist, shift, angle,
                                         scene_inside=hist['scene_inside'][-1])
        return SeparationResult(verts, state.quat, state.transl, state.pivot, M, k, separated, hist, shift, angle)
