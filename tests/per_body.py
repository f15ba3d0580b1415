"""Per-body accuracy against an fp64 evaluation (test infrastructure).

A batch of bodies is B independent problems: nothing in a body's result may depend on how large the OTHER bodies' numbers are.
``conftest.rel_err`` normalises by the largest entry of the whole tensor, so a body whose result is a million times smaller than the
largest body's can be wrong, or zero, and still pass.  Here every body b is measured against its own scale:

    d(b) = max |x_b - ref64_b| / max |ref64_b|

for the implementation (d_prod) and for a plain fp32 evaluation of the same operation (d_f32), and each body must be in the fp32
accuracy class of its own:  d_prod(b) <= K d_f32(b) + FLOOR,  K = the arbiter's K_NOISE (arbiter.py).
"""
import numpy as np

import arbiter

FLOOR = 2e-7


def per_body_dist(x, ref64):
    """max |x_b - ref64_b| / max |ref64_b| for every body b (the first axis).  A NaN or Inf in x_b gives NaN / Inf (the check fails)."""
    x = np.asarray(x, np.float64)
    r = np.asarray(ref64, np.float64)
    x, r = x.reshape(len(x), -1), r.reshape(len(r), -1)
    assert x.shape == r.shape, (x.shape, r.shape)
    scale = np.abs(r).max(1)
    assert (scale > 0).all(), 'a body whose reference is all zero: the per-body measure needs a non-zero reference'
    return np.abs(x - r).max(1) / scale


def assert_per_body_accuracy_class(x, ref64, ref32, what='', k=arbiter.K_NOISE, floor=FLOOR):
    """Every body of x is as close to ref64 as the fp32 evaluation ref32 is (K = k), measured on the body's own scale."""
    d_prod, d_f32 = per_body_dist(x, ref64), per_body_dist(ref32, ref64)
    bad = np.nonzero(~(d_prod <= k * d_f32 + floor))[0]             # (a NaN distance fails too)
    assert bad.size == 0, '%s: bodies %s outside the fp32 accuracy class: d_prod %s, d_f32 %s' % (
        what, bad.tolist()[:8], d_prod[bad][:8].tolist(), d_f32[bad][:8].tolist())
    return d_prod, d_f32
