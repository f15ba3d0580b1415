"""The handles of the body-against-body family without a GPU (hip.Handle; ops.body_overlap_create, ops.surface_crossings_create,
ops._handle_of; evaluation.BodyOverlap, SurfaceCrossings, BodySeparator): the library is replaced by a fake that hands out addresses and
counts what it is asked to free.  A handle is freed exactly once, when its last holder lets go or at ``close()``; a holder standing in for
an autograd graph keeps it alive whatever the evaluator does; the integers come from one query at creation.  And the one range check of
the family's real arguments, with the message of each of its callers."""
import contextlib
import ctypes
import gc
import weakref

import numpy as np
import pytest
import torch

from psi_release_amd import evaluation, hip, ops

FACES = np.array([[0, 1, 2], [1, 2, 4]], np.int32)
KINDS = ('body_overlap', 'surface_crossings')
CREATE = {'body_overlap': ops.body_overlap_create, 'surface_crossings': ops.surface_crossings_create}
DESTROY = {'body_overlap': ops.body_overlap_destroy, 'surface_crossings': ops.surface_crossings_destroy}


class FakeLib:
    """The create, info and destroy symbols of both kinds; ``freed`` lists (symbol, address) in call order."""

    def __init__(self):
        self.made, self.freed, self.info_calls, self.live, self._next = {}, [], 0, [], 0x1000

    def _create(self, out, V, F, n_chunks):
        self._next += 0x100
        out._obj.value = self._next
        self.made[self._next] = (V, F, n_chunks)
        self.live.append(weakref.ref(out._obj))
        return 0

    def _info(self, handle, info):
        self.info_calls += 1
        info[0], info[1], info[2] = self.made[handle.value]
        return 0

    def psi_body_overlap_create(self, out, faces, V, F):
        return self._create(out, V, F, 0)

    def psi_surface_crossings_create(self, out, faces, V, F, order_verts, face_part, part_skip, P):
        return self._create(out, V, F, (F + 255) // 256)

    psi_body_overlap_info = psi_surface_crossings_info = _info

    def psi_body_overlap_destroy(self, handle):
        self.freed.append(('psi_body_overlap_destroy', handle.value))

    def psi_surface_crossings_destroy(self, handle):
        self.freed.append(('psi_surface_crossings_destroy', handle.value))


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(hip, 'lib', lambda: fake)
    monkeypatch.setattr(torch.cuda, 'device', lambda device: contextlib.nullcontext())      # the evaluators make their handle under it
    yield fake
    for ref in fake.live:                       # an address of the fake must never reach the library: whatever a failed test left is emptied
        if ref() is not None:
            ref().value = None


def _freed(lib):
    gc.collect()
    return list(lib.freed)


@pytest.mark.parametrize('kind', KINDS)
def test_a_handle_is_a_pointer_with_its_integers(lib, kind):
    h = CREATE[kind](torch.tensor(FACES), 5)
    assert isinstance(h, hip.Handle) and isinstance(h, ctypes.c_void_p) and bool(h) and h.value in lib.made
    assert (h.V, h.F, h.n_chunks) == (5, 2, 0 if kind == 'body_overlap' else 1) and h.destroy == 'psi_%s_destroy' % kind
    assert lib.info_calls == 1
    assert ops._handle_of(h, 5, kind) is h and lib.info_calls == 1                      # no query per operator call
    with pytest.raises(ValueError, match='the handle was made for 5 vertices per body, verts has 6'):
        ops._handle_of(h, 6, kind)
    made = ops._handle_of(FACES, 7, kind)                                               # faces, an array included: a handle of its own
    assert isinstance(made, hip.Handle) and made.V == 7 and made.value != h.value


@pytest.mark.parametrize('kind', KINDS)
def test_destroy_runs_once_when_the_last_reference_goes(lib, kind):
    h = CREATE[kind](FACES, 5)
    address, second = h.value, h
    del h
    assert _freed(lib) == []
    del second
    assert _freed(lib) == [('psi_%s_destroy' % kind, address)]


@pytest.mark.parametrize('kind', KINDS)
def test_close_frees_once(lib, kind):
    h = CREATE[kind](FACES, 5)
    address = h.value
    h.close()
    assert not h and h.value is None and _freed(lib) == [('psi_%s_destroy' % kind, address)]
    h.close()
    DESTROY[kind](h)
    DESTROY[kind](h)
    del h
    assert _freed(lib) == [('psi_%s_destroy' % kind, address)]
    g = CREATE[kind](FACES, 5)
    other = g.value
    DESTROY[kind](g)                                                                     # the operators' own names: the same close
    DESTROY[kind](g)
    del g
    assert _freed(lib) == [('psi_%s_destroy' % kind, address), ('psi_%s_destroy' % kind, other)]


@pytest.mark.parametrize('kind', KINDS)
def test_a_null_or_borrowed_handle_is_never_freed(lib, kind):
    h = hip.Handle('psi_%s_destroy' % kind)
    assert not h
    h.close()
    del h
    assert _freed(lib) == []
    owner = CREATE[kind](FACES, 5)
    raw = ctypes.c_void_p(owner.value)                                                   # a handle its caller owns
    view = ops._handle_of(raw, 5, kind)
    assert isinstance(view, hip.Handle) and view.value == raw.value and (view.V, view.F) == (5, 2) and lib.info_calls == 2
    with pytest.raises(ValueError, match='the handle was made for 5 vertices per body, verts has 4'):
        ops._handle_of(raw, 4, kind)
    view.close()
    del view
    assert _freed(lib) == [] and raw.value == owner.value


def _evaluator(kind):
    return evaluation.BodyOverlap(FACES) if kind == 'body_overlap' else evaluation.SurfaceCrossings(FACES)


class _Graph:
    """Stands in for the ``ctx`` of an autograd Function: it holds the handle the backward pass will need."""


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('what', ['deleted', 'closed', 'another V'])
def test_a_second_holder_keeps_the_handle_alive(lib, kind, what):
    ev = _evaluator(kind)
    ctx = _Graph()
    ctx.handle = ev._handle_for(5)
    address = ctx.handle.value
    assert ev._handle_for(5) is ctx.handle and len(lib.made) == 1                       # one handle per vertex count
    if what == 'deleted':
        del ev
    elif what == 'closed':
        ev.close()
        ev.close()
    else:
        assert ev._handle_for(6).V == 6 and len(lib.made) == 2
    assert _freed(lib) == [] and ctx.handle.value == address and ctx.handle.V == 5
    del ctx
    assert _freed(lib) == [('psi_%s_destroy' % kind, address)]


def test_an_evaluator_alone_frees_its_handle(lib):
    for kind in KINDS:
        ev = _evaluator(kind)
        first = ev._handle_for(5).value
        second = ev._handle_for(6).value                                                 # the handle for 5 has no other holder
        assert _freed(lib) == [('psi_%s_destroy' % kind, first)]
        ev.close()
        assert _freed(lib) == [('psi_%s_destroy' % kind, first), ('psi_%s_destroy' % kind, second)]
        third = ev._handle_for(6).value                                                  # usable again after close()
        del ev
        assert _freed(lib)[2:] == [('psi_%s_destroy' % kind, third)]
        lib.freed.clear()


def test_separator_close_leaves_held_handles(lib):
    sep = evaluation.BodySeparator(FACES)
    oh, ch = sep.overlap._handle_for(5), sep.crossings._handle_for(5)
    free = evaluation.BodySeparator(FACES)
    addresses = free.overlap._handle_for(5).value, free.crossings._handle_for(5).value
    sep.close()
    free.close()
    assert _freed(lib) == [('psi_body_overlap_destroy', addresses[0]), ('psi_surface_crossings_destroy', addresses[1])]
    assert oh and ch
    kept = oh.value, ch.value
    del oh, ch
    assert _freed(lib)[2:] == [('psi_body_overlap_destroy', kept[0]), ('psi_surface_crossings_destroy', kept[1])]


NOT_REAL = (True, False, float('nan'), float('inf'), -float('inf'), None, '0.1', [0.1], torch.tensor(0.1))


def _refused(call, bad, message):
    with pytest.raises(ValueError) as e:
        call(bad)
    assert str(e.value) == message % (bad,), (bad, str(e.value))


def test_the_range_check_and_the_messages_of_its_callers():
    assert ops._check_real(3, lambda x: x > 0, 'unused') == 3.0 and isinstance(ops._check_real(3, lambda x: True, 'unused'), float)
    assert ops._check_real(np.float32(0.25), lambda x: x < 1, 'unused') == 0.25
    for bad in NOT_REAL + (-1.0, 2):
        with pytest.raises(ValueError, match='^x is 7 and y$'):
            ops._check_real(bad, lambda x: 0 <= x < 2, 'x is %d and %s', 7, 'y')
    step = dict(lr_t=0.01, lr_r=0.01, betas=(0.9, 0.999), eps=1e-8)
    base = torch.zeros(2, 5, 3)
    callers = [
        (lambda s: ops._check_sigma(s), 'sigma is a finite number in (0, 0.5], got %r', (0.0, -1e-3, 0.5000001), (0.5, 1e-3)),
        (lambda w: ops._check_w_scene(w), 'w_scene is a finite number >= 0, got %r', (-1e-9, -1), (0, 0.0, 2.5)),
        (lambda w: ops._check_w_scene(w, positive=True), 'w_scene is a finite number >= 0, got %r', (-1e-9,), (2.5,)),
        (lambda x: ops._check_step_args(**dict(step, lr_t=x)), 'lr_t is a finite positive number, got %r', (0, 0.0, -0.01), (1, 1e-3)),
        (lambda x: ops._check_step_args(**dict(step, lr_r=x)), 'lr_r is a finite positive number, got %r', (0, 0.0, -0.01), (1, 1e-3)),
        (lambda x: ops._check_step_args(**dict(step, eps=x)), 'eps is a finite number >= 0, got %r', (-1e-12,), (0, 0.0, 1e-8)),
        (lambda x: ops.rigid_separate(base, None, None, w_pen=x), 'w_pen is a finite number >= 0, got %r', (-1.0,), ()),
        (lambda x: ops.rigid_separate(base, None, None, w_cross=x), 'w_cross is a finite number >= 0, got %r', (-1.0,), ()),
        (lambda x: ops.rigid_separate(base, None, None, sigma=x), 'sigma is a finite number in (0, 0.5], got %r', (0.6,), ()),
    ]
    for call, message, outside, inside in callers:
        for bad in NOT_REAL + outside:
            _refused(call, bad, message)
        for good in inside:
            call(good)
    with pytest.raises(ValueError, match='w_scene is zero with a scene given'):
        ops._check_w_scene(0, positive=True)
    for bad in ((0.9,), (0.9, 0.999, 0.5), [0.9, 1.0], (True, 0.5), (0.9, float('nan')), (-0.1, 0.5), 0.9, None, 'ab', (0.9, None)):
        _refused(lambda b: ops._check_step_args(**dict(step, betas=b)), bad, 'betas is a pair of numbers in [0, 1), got %r')
    ops._check_step_args(**dict(step, betas=[0, 0.5]))
