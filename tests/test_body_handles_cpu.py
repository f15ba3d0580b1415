"""The handles of the body-against-body family without a GPU (hip.Handle; ops.body_overlap_create, ops.surface_crossings_create,
ops._handle_of; evaluation.BodyOverlap, SurfaceCrossings, BodySeparator): the library is replaced by a fake that hands out addresses and
counts what it is asked to free.  A handle is freed exactly once, when its last holder lets go or at ``close()``; a holder standing in for
an autograd graph keeps it alive whatever the evaluator does; the integers come from one query at creation.  And the one range check of
the family's real arguments, with the message of each of its callers.

The library's other owners go through the same fake (ops.raster_mesh_create, raster_bodies_create, mesh_sdf_create; ops.SceneNNIndex,
SceneSet; body_model.LbsModel; fitting.FusedEngine; evaluation.KMeansRestarts; rendering.SceneMesh, ResultRenderer; scene_sdf.MeshSDF):
nothing is freed while a holder lives, everything once when the last goes or at ``close()``, a second ``close()`` does nothing, and the
two owners that wait for the device do so before their destroy."""
import contextlib
import ctypes
import gc
import re
import weakref
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from psi_release_amd import body_model, evaluation, fitting, hip, ops, rendering, scene_sdf

FACES = np.array([[0, 1, 2], [1, 2, 4]], np.int32)
KINDS = ('body_overlap', 'surface_crossings')
CREATE = {'body_overlap': ops.body_overlap_create, 'surface_crossings': ops.surface_crossings_create}
DESTROY = {'body_overlap': ops.body_overlap_destroy, 'surface_crossings': ops.surface_crossings_destroy}
OWNED = ('nn_index_set', 'nn_index', 'lbs', 'fit', 'kmeans', 'raster_mesh', 'raster_bodies', 'mesh_sdf')


class FakeLib:
    """The create, info and destroy symbols of both kinds; ``freed`` lists (symbol, address) in call order."""

    def __init__(self):
        self.made, self.freed, self.events, self.info_calls, self.live, self._next = {}, [], [], 0, [], 0x1000

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

    def __getattr__(self, name):
        """The other families: ``made`` maps an address to the family that created it; ``events`` adds the device synchronisations to the
        destroys.  Every further symbol succeeds and does nothing."""
        m = re.fullmatch(r'psi_(%s)_(create|create_scenes|destroy)' % '|'.join(OWNED), name)
        if not name.startswith('psi_'):
            raise AttributeError(name)
        if not m:
            return lambda *args: 0
        if m.group(2) == 'destroy':
            return lambda handle: (self.freed.append((name, handle.value)), self.events.append((name, handle.value)))[0]
        return lambda out, *args: self._create(out, m.group(1), 0, 0)


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


# ------------------------------------------------------------------------------------------
# The library's other owners
# ------------------------------------------------------------------------------------------
class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU and stays where it is: what the owners' argument checks ask of their inputs."""
    is_cuda = True

    def to(self, *args, **kwargs):
        return self


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


@pytest.fixture
def no_gpu(lib, monkeypatch):
    """The fake library, and a device to match: tensors made "on the GPU" land on the CPU, a pointer is a number, the stream an object,
    and ``torch.cuda.synchronize`` is an event in ``lib.events``."""
    real = torch.tensor
    monkeypatch.setattr(torch, 'tensor', lambda data, *args, device=None, **kwargs: real(data, *args, **kwargs))
    monkeypatch.setattr(hip, 'ptr', lambda t: None if t is None else 0x40)
    monkeypatch.setattr(torch.cuda, 'Stream', lambda device=None: SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda device=None: lib.events.append(('synchronize', None)))
    return lib


TRIANGLES = dict(verts=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32), faces=np.array([[0, 1, 2], [1, 3, 2]], np.int64))


def _lbs_model():
    V, J, NB = 4, 2, 1
    return body_model.LbsModel(np.zeros((V, 3)), np.zeros((V, 3, NB)), np.zeros(((J - 1) * 9, 3 * V)), np.zeros((J, V)), np.zeros((V, J)),
                               np.array([-1, 0]), 'cuda')


def _engine():
    dec = {'bodyprior_dec_fc1': (512, 32), 'bodyprior_dec_fc2': (512, 512), 'bodyprior_dec_out': (126, 512)}
    sd = {k + '.weight': torch.zeros(*s) for k, s in dec.items()}
    sd.update({k + '.bias': torch.zeros(s[0]) for k, s in dec.items()})
    bm = SimpleNamespace(left_hand_components=torch.zeros(6, 45), right_hand_components=torch.zeros(6, 45), pose_mean=torch.zeros(165),
                         lbs_model=SimpleNamespace(handle=ctypes.c_void_p(0x80)))
    op = SimpleNamespace(device='cpu', vposer=SimpleNamespace(state_dict=lambda: sd), body_mesh_model=bm, batch_size=2, align_corners=False,
                         contact_vertex_ids=lambda: torch.zeros(4, dtype=torch.int64), s_grid_min_batch=torch.zeros(1, 3),
                         s_grid_max_batch=torch.ones(1, 3), s_verts=torch.zeros(1, 8, 3), s_sdf=torch.zeros(1, 4, 4, 4), weight_loss_rec=1.0,
                         weight_loss_vposer=0.01, weight_contact=0.1, weight_collision=0.5, contact_const=0.0, init_lr_h=0.1, nn_mode='kdtree')
    return fitting.FusedEngine(op)


def _result_renderer():
    r = rendering.ResultRenderer(None, TRIANGLES['faces'])
    r._bodies(_gpu(1, 4, 3))                                                             # the handle is made for the first bodies' V
    return r


# owner -> (what makes one, the families of the handles it then holds)
OWNERS = {
    'SceneNNIndex': (lambda: ops.SceneNNIndex(np.zeros((65, 3), np.float32), device='cpu'), ['nn_index']),
    'SceneSet': (lambda: ops.SceneSet(torch.zeros(2, 65, 3), device='cpu'), ['nn_index', 'nn_index', 'nn_index_set']),
    'LbsModel': (_lbs_model, ['lbs']),
    'FusedEngine': (_engine, ['fit']),
    'KMeansRestarts': (lambda: evaluation.KMeansRestarts(_gpu(64, 3), _gpu(1, 2, 3)), ['kmeans']),
    'SceneMesh': (lambda: rendering.SceneMesh(**TRIANGLES), ['raster_mesh']),
    'ResultRenderer': (_result_renderer, ['raster_bodies']),
    'MeshSDF': (lambda: scene_sdf.MeshSDF(**TRIANGLES), ['mesh_sdf']),
}
WAITS_FOR_THE_DEVICE = ('FusedEngine', 'KMeansRestarts')


def _made_by(lib, owner):
    """What ``owner`` must free: (destroy symbol, address) of every handle the fake made, sorted."""
    assert isinstance(owner.handle, hip.Handle) and owner.handle.value in lib.made
    return sorted(('psi_%s_destroy' % family, address) for address, (family, _, _) in lib.made.items())


@pytest.mark.parametrize('name', sorted(OWNERS))
def test_an_owner_frees_its_handle_once_when_its_last_holder_goes(no_gpu, name):
    make, families = OWNERS[name]
    owner = make()
    made = _made_by(no_gpu, owner)
    assert [symbol for symbol, _ in made] == sorted('psi_%s_destroy' % f for f in families)
    assert owner.handle.destroy == 'psi_%s_destroy' % families[-1]
    second = owner
    del owner
    assert _freed(no_gpu) == []
    if name not in WAITS_FOR_THE_DEVICE:                                                 # (their ``__del__`` is their ``close()``)
        second = second.handle                                                           # the owner is gone, its handle has a holder
        assert sorted(_freed(no_gpu)) == [f for f in made if f[1] != second.value]       # (a set's indices go with the set)
    del second
    assert sorted(_freed(no_gpu)) == made
    if name in WAITS_FOR_THE_DEVICE:
        assert no_gpu.events == [('synchronize', None), made[0]]
    else:
        assert ('synchronize', None) not in no_gpu.events


@pytest.mark.parametrize('name', sorted(OWNERS))
def test_closing_an_owners_handle_twice_frees_it_once(no_gpu, name):
    owner = OWNERS[name][0]()
    mine = ('psi_%s_destroy' % OWNERS[name][1][-1], owner.handle.value)
    close = owner.close if name in WAITS_FOR_THE_DEVICE else owner.handle.close
    close()
    assert _freed(no_gpu) == [mine] and not owner.handle and isinstance(owner.handle, hip.Handle)
    close()
    assert _freed(no_gpu) == [mine]
    if name in WAITS_FOR_THE_DEVICE:
        assert no_gpu.events == [('synchronize', None), mine]                            # the device is idle before the destroy, and asked once
    made = sorted(('psi_%s_destroy' % family, address) for address, (family, _, _) in no_gpu.made.items())
    del owner
    assert sorted(_freed(no_gpu)) == made and no_gpu.events.count(('synchronize', None)) == (1 if name in WAITS_FOR_THE_DEVICE else 0)


OPS_CREATE = {
    'raster_mesh': lambda: ops.raster_mesh_create(_gpu(4, 3), _gpu(2, 3, dtype=torch.int32), _gpu(4)),
    'raster_bodies': lambda: ops.raster_bodies_create(_gpu(2, 3, dtype=torch.int32), 4),
    'mesh_sdf': lambda: ops.mesh_sdf_create(_gpu(4, 3), _gpu(2, 3, dtype=torch.int32)),
}
OPS_DESTROY = {'raster_mesh': ops.raster_mesh_destroy, 'raster_bodies': ops.raster_bodies_destroy, 'mesh_sdf': ops.mesh_sdf_destroy}


@pytest.mark.parametrize('kind', sorted(OPS_CREATE))
def test_the_create_operators_hand_out_handles_that_own_themselves(no_gpu, kind):
    symbol = 'psi_%s_destroy' % kind
    h = OPS_CREATE[kind]()
    assert isinstance(h, hip.Handle) and h.destroy == symbol and no_gpu.made[h.value][0] == kind
    address, second = h.value, h
    del h
    assert _freed(no_gpu) == []
    del second
    assert _freed(no_gpu) == [(symbol, address)]
    g = OPS_CREATE[kind]()
    other = g.value
    OPS_DESTROY[kind](g)                                                                 # the operators' own names: the same close
    assert not g and _freed(no_gpu) == [(symbol, address), (symbol, other)]
    OPS_DESTROY[kind](g)
    g.close()
    del g
    assert _freed(no_gpu) == [(symbol, address), (symbol, other)]
    raw = ctypes.c_void_p(0x7700)                                                        # a handle its caller owns: freed through the library, as before
    OPS_DESTROY[kind](raw)
    OPS_DESTROY[kind](ctypes.c_void_p())
    OPS_DESTROY[kind](None)
    assert _freed(no_gpu)[2:] == [(symbol, 0x7700)]
