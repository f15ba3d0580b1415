"""CPU simulation of the summation order of bn_stats_kernel / bn_fwd_finalize_kernel (csrc/bnorm.hip) in numpy: what the variance of a channel loses
at a given mean / std, with sums of x and x^2 ("as coded" before the pivot) and with sums of x - x[0][c] and its square (the kernel now).

    python tools/bnorm_stats_sim.py [--json FILE]

Order simulated, per channel: a thread's rows r, r + stride, ... (stride = nblk * rpb) as one fp32 chain (acc += d; acc2 = fma(d, d, acc2)), the
rpb row-threads of a block as one fp32 chain in row order (block_reduce_store), the nblk block partials in double (sum_partials: a different
association of exact-enough double additions), var = Q/M - (S/M)^2 in double.  Inputs N(r, 1) rounded to fp32; the error is relative to the fp64
two-pass variance of the same fp32 values, worst channel of the map.
"""
import argparse
import json

import numpy as np

SHAPES = [(70000, 64), (14000, 256)]
RATIOS = [0, 4, 16, 64, 256, 1024]


def kernel_sums(d):
    """d [M, C] fp32 (the addends of the first sum) -> S, Q [C] float64 in the kernel's order"""
    M, C = d.shape
    rpb = 2048 // C
    nblk = max(1, min(512, -(-M // rpb)))
    stride = nblk * rpb
    passes = -(-M // stride)
    pad = np.zeros((passes * stride, C), np.float32)
    pad[:M] = d                                                  # (a zero addend leaves an fp32 accumulator unchanged)
    pad = pad.reshape(passes, nblk, rpb, C)
    s = np.zeros((nblk, rpb, C), np.float32)
    q = np.zeros((nblk, rpb, C), np.float32)
    for k in range(passes):                                      # the per-thread chain
        v = pad[k]
        s = s + v
        q = (q.astype(np.float64) + v.astype(np.float64) * v.astype(np.float64)).astype(np.float32)      # fma: one rounding
    bs = np.zeros((nblk, C), np.float32)
    bq = np.zeros((nblk, C), np.float32)
    for r in range(rpb):                                         # the LDS chain over the block's row-threads
        bs = bs + s[:, r]
        bq = bq + q[:, r]
    return bs.astype(np.float64).sum(0), bq.astype(np.float64).sum(0)


def variance_errors(M, C, r, seed=0):
    rng = np.random.default_rng(seed + 1000 * C + r)
    x = (rng.standard_normal((M, C)) + r).astype(np.float32)
    x64 = x.astype(np.float64)
    var64 = ((x64 - x64.mean(0)) ** 2).mean(0)
    out = {}
    for name, d in (('as_coded', x), ('shifted', x - x[0:1])):
        S, Q = kernel_sums(d)
        var = Q / M - (S / M) ** 2
        out[name] = float((np.abs(var - var64) / var64).max())
    return out


def table():
    t = {'as_coded': {}, 'shifted': {}}
    for r in RATIOS:
        e = [variance_errors(M, C, r) for M, C in SHAPES]
        for k in t:
            t[k][str(r)] = max(v[k] for v in e)
    return t


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    t = table()
    print('relative variance error (worst channel of M, C = %s), mean / std = %s' % (SHAPES, RATIOS))
    for k in ('as_coded', 'shifted'):
        print('%-9s ' % k + '  '.join('%.1e' % t[k][str(r)] for r in RATIOS))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump({'shapes_M_C': SHAPES, 'relative_variance_error': t}, fh, indent=1)
