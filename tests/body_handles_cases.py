"""What the GPU tests of a handle's lifetime share (tests/test_body_depth_gpu.py, tests/test_crossing_field_gpu.py): the loss of an
evaluator whose handle only the autograd graph still holds."""
import gc

import torch

from psi_release_amd import hip

LET_GO = ('deleted', 'closed', 'another V')


def graph_outlives_evaluator(monkeypatch, symbol, make, loss_of, run_other_V, verts, g, what):
    """``make()`` gives an evaluator, ``loss_of(evaluator, leaf)`` its differentiable loss [B] of the leaf ``verts`` [B,V,3],
    ``run_other_V(evaluator)`` puts a batch of another vertex count through it.  The library's ``symbol`` (the destroy of the evaluator's
    handle) is counted.  The evaluator lets go of its handle as ``what`` says between forward and backward: the handle must not be freed
    before the backward pass, whose gradient has the bits of the one taken with the evaluator alive, and is freed once when the graph
    goes.  The count is asserted BEFORE the backward pass runs: a handle freed too early fails there, on the host, and never reaches the
    kernel."""
    alive = make()
    leaf = verts.clone().requires_grad_(True)
    (loss_of(alive, leaf) * g).sum().backward()
    want = leaf.grad
    gc.collect()
    L, freed = hip.lib(), []
    real = getattr(L, symbol)
    monkeypatch.setattr(L, symbol, lambda handle: (freed.append(handle.value), real(handle))[1])
    evaluator = make()
    leaf = verts.clone().requires_grad_(True)
    loss = loss_of(evaluator, leaf)
    if what == 'deleted':
        del evaluator
    elif what == 'closed':
        evaluator.close()
    else:
        run_other_V(evaluator)
    gc.collect()
    print('%s, evaluator %s: %d handles freed before the backward pass' % (symbol, what, len(freed)))
    assert freed == []                                                                   # the guard
    (loss * g).sum().backward()
    other_bits = int((leaf.grad.view(torch.int32) != want.view(torch.int32)).sum().item())
    del loss
    gc.collect()
    print('   gradient values with other bits %d, largest %.4g; handles freed with the graph %d' % (other_bits, want.abs().max().item(), len(freed)))
    assert other_bits == 0 and want.abs().max().item() > 0 and len(freed) == 1
