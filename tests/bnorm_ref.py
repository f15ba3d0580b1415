"""Plain fp64 reference of the fused BatchNorm operator of csrc/bnorm.hip (ops.bn_act / ops.bn_act_t), CPU torch, float64 throughout.

    y = act(gamma * (x - mean_c) / sqrt(var_c + eps) + beta (+ residual)),   act = ReLU or identity

with the batch statistics of x over (N, H, W) (training: biased variance in y, unbiased in the running buffer) or the running statistics
(eval), and its backward for a given ReLU mask.  Inputs are the STORED values of the operands (a bf16 tensor upcasts exactly); nothing here
is rounded to a narrower type, and no library batch-norm is called.  Also the error bounds the tests hold the kernels to, derived in
tests/test_bnorm_fp64_gpu.py, since they are functions of the reference's own intermediate values.
"""
import torch

U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)
F64 = torch.float64


def f64(t):
    """A tensor's stored values as CPU float64 (exact for bf16 / fp32 / integer tensors), plain contiguous NCHW."""
    return t.detach().to('cpu').to(F64).contiguous()


def _c(v):
    return v.view(1, -1, 1, 1)


def batch_stats(x):
    """mean and biased variance per channel of x [N,C,H,W] (two-pass, fp64)"""
    mean = x.mean((0, 2, 3))
    var = (x - _c(mean)).square().mean((0, 2, 3))
    return mean, var


class Forward:
    """Everything the forward computes, kept for the backward and for the bounds.  training: batch statistics and the running-buffer update
    (momentum, unbiased variance, counter + 1); else the running statistics, nothing updated."""

    def __init__(self, x, gamma, beta, eps, residual=None, relu=False, training=True, running_mean=None, running_var=None, momentum=0.1,
                 num_batches_tracked=0):
        self.x, self.gamma, self.beta, self.res, self.relu, self.eps, self.training = x, gamma, beta, residual, relu, float(eps), training
        N, C, H, W = x.shape
        self.M = M = N * H * W
        if training:
            self.mean, self.var = batch_stats(x)
            self.new_running_mean = self.new_running_var = None
            if running_mean is not None:
                unb = self.var * M / (M - 1) if M > 1 else self.var
                self.unbiased = unb
                self.new_running_mean = (1.0 - momentum) * running_mean + momentum * self.mean
                self.new_running_var = (1.0 - momentum) * running_var + momentum * unb
            self.new_num_batches_tracked = num_batches_tracked + 1
        else:
            self.mean, self.var = running_mean, running_var
            self.new_running_mean, self.new_running_var, self.new_num_batches_tracked = running_mean, running_var, num_batches_tracked
        self.invstd = 1.0 / torch.sqrt(self.var + self.eps)
        self.sc = gamma * self.invstd
        self.xhat = (x - _c(self.mean)) * _c(self.invstd)
        z = _c(gamma) * self.xhat + _c(beta)
        if residual is not None:
            z = z + residual
        self.y = torch.relu(z) if relu else z

    def backward(self, dy, mask=None):
        """dx, dresidual (None without a skip connection), dgamma, dbeta for dL/dy = dy; mask: the ReLU mask "y > 0" as a boolean tensor (the
        tests pass the kernel's own, so that no element is left out of a comparison), None: this reference's."""
        dz = dy
        if self.relu:
            dz = dy * (self.y > 0 if mask is None else mask).to(F64)
        self.dz = dz
        self.dbeta = dz.sum((0, 2, 3))
        self.dgamma = (dz * self.xhat).sum((0, 2, 3))
        if self.training:
            self.a = self.sc
            self.b = -self.sc * self.dgamma / self.M
            self.c = -self.sc * self.dbeta / self.M
            self.dx = _c(self.a) * dz + _c(self.b) * self.xhat + _c(self.c)
        else:
            self.dx = _c(self.sc) * dz
        return self.dx, (dz if self.res is not None else None), self.dgamma, self.dbeta


# ---------------------------------------------------------------------------------------------------------------------------------
# launch geometry of the kernels (csrc/bnorm.hip: bn_blocks), for the chain length of the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def rows_per_block(C):
    return 2048 // C


def stat_blocks(M, C):
    rpb = rows_per_block(C)
    return max(1, min(512, -(-M // rpb)))


def chain_length(M, C):
    """L: the longest chain of fp32 additions behind one partial sum: a thread's rows, then the block's rpb row-threads in LDS"""
    rpb, nblk = rows_per_block(C), stat_blocks(M, C)
    return -(-M // (nblk * rpb)) + rpb


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds (see the docstring of tests/test_bnorm_fp64_gpu.py for where each constant comes from)
# ---------------------------------------------------------------------------------------------------------------------------------
D_INVSTD = 34 * U       # relative error of gamma * invstd: half the variance bound (32u), invstd's fp32 rounding, the product's (<= u each)
D_XHAT_IS = 33 * U      # relative error of save_invstd alone
D_EVAL_SC = 8 * U       # eval: gamma / sqrtf(rvar + eps) in fp32: the add (u/4 after the root), sqrtf (1 ulp = 2u), the division (2.5 ulp = 5u)


def var_bound(var, eps):
    return 64 * U * (var + eps)


def mean_bound(mean, var):
    return 16 * U * torch.sqrt(var) + U * mean.abs()


def output_bound(f, bf16):
    """element-wise bound of |y_kernel - y64|"""
    sc, x = _c(f.sc), f.x
    terms = (x * sc).abs() + _c((f.mean * f.sc).abs() + f.beta.abs()) + f.y.abs()
    if f.res is not None:
        terms = terms + f.res.abs()
    if f.training:
        b = 4 * U * terms + (x * sc).abs() * D_INVSTD + _c(f.sc.abs() * mean_bound(f.mean, f.var))
    else:
        b = 4 * U * terms + ((x * sc).abs() + _c((f.mean * f.sc).abs())) * D_EVAL_SC
    if bf16:
        b = b * (1 + 2.0 ** -8) + 2.0 ** -8 * f.y.abs()
    return b


def xhat_bound(f):
    """element-wise bound of the kernel's xhat = (x - save_mean) * save_invstd against the reference's: the statistics, two roundings"""
    return _c(mean_bound(f.mean, f.var) * f.invstd) + f.xhat.abs() * (D_XHAT_IS + 2 * U)


def param_grad_bounds(f, C):
    """bounds of |dgamma - dgamma64|, |dbeta - dbeta64| per channel"""
    L = chain_length(f.M, C)
    s_dz = f.dz.abs().sum((0, 2, 3))
    s_dzx = (f.dz * f.xhat).abs().sum((0, 2, 3))
    db = 2 * L * U * s_dz
    dg = 2 * L * U * s_dzx + (f.dz.abs() * xhat_bound(f)).sum((0, 2, 3))
    return dg, db


def dx_bound(f, bf16, dg, db):
    """element-wise bound of |dx_kernel - dx64| for dx = a dz + b xhat + c evaluated in fp32 with the kernel's coefficients; dg, db: the bounds
    of dgamma and dbeta (param_grad_bounds)"""
    a, b, c = f.a.abs(), f.b.abs(), f.c.abs()
    e_b = b * (D_INVSTD + U) + a * dg / f.M            # |b_kernel - b64|: a's error, the fp32 rounding, dgamma's error
    e_c = c * (D_INVSTD + U) + a * db / f.M
    t_a, t_b = (_c(f.a) * f.dz).abs(), (_c(f.b) * f.xhat).abs()
    bound = t_a * (D_INVSTD + 3 * U) + t_b * 3 * U + _c(e_b) * f.xhat.abs() + _c(b) * xhat_bound(f) + _c(c * 3 * U + e_c)
    if bf16:
        bound = bound * (1 + 2.0 ** -8) + 2.0 ** -8 * f.dx.abs()
    return bound


def running_bounds(f, running_mean, running_var, momentum):
    """bounds of the updated running buffers: the statistics bound times momentum, and the fp32 evaluation of (1 - m) * old + m * new"""
    M = f.M
    k = M / (M - 1) if M > 1 else 1.0
    bm = momentum * mean_bound(f.mean, f.var) + 2 * U * (((1 - momentum) * running_mean).abs() + (momentum * f.mean).abs())
    bv = momentum * k * var_bound(f.var, f.eps) + 2 * U * (((1 - momentum) * running_var).abs() + (momentum * f.unbiased).abs())
    return bm, bv


def worst_ratio(err, bound):
    """max over elements of error / bound (0 / 0 counts as 0, anything above a zero bound as inf)"""
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(r.max())
